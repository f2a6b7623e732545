"""The engine's float statistics -- NICH (count, mean, count_times_variance)
and GammaPoisson's log_prod -- held to the float64 moments of their rows
(tests/f64_stats.py).

Ordered paths (k_replay_sorted after the counting sort, the additions-only
replay of load_rows, k_chains' stats_add / stats_remove): counts equal to the
rows', floats within the ordered Welford / log_prod bounds over the history
of sweeps.

Merged path (float_stats = 1: k_merge_float_moves / _reduce / _apply /
_export): within `merged_bounds` after EVERY sub-sweep, from a load and from
float64 moments installed through import_float_moments_dev; the exported
image against the rows' sums; export then import; two half-engines' images
summed into a third; and score_rows_dev (the group caches) against the
float64 predictives with the merged bounds in place of the Welford ones.

Statistics are read with get_group(f, slot), the slot of a global id being
core.global_to_packed's.  Histories are the engine's own assignments() after
each sweep or sub-sweep: the truth is always that of the engine's own
assignment.

`drain` (tests/test_f64_stats.py) is held on the kernels' restatement only:
no entry point applies chosen moves to an engine (see that file).

The binary64 LDS atomics of k_merge_float_moves add in no fixed order, so the
last binary32 bit of a merged statistic may differ from run to run; nothing
here asserts against that."""
import numpy as np
import pytest

import f64_scores as fx
import f64_stats as fs
import oracle_lib as ol
from test_f64_scores import worst
from test_f64_stats import (MERGED, ORDERED, SEED, batches_of, fmt,
                            merged_inputs, ordered_inputs, read_groups)
from test_gpu_scores_f64 import score_rows

pytestmark = pytest.mark.gpu

ALPHA, D = 20.0, 0.5


def make_engine(gsh, vals, assign, k, opts):
    from distributions_amd import engine
    gpu = engine.Gibbs(ALPHA, D, gsh)
    for key, value in opts.items():
        gpu.set_option(key, value)
    gpu.load_rows(vals, assign, k, 1)
    return gpu


def stats_of(gpu, osh):
    got = read_groups(gpu, osh)
    for f in got:
        for gid in got[f]:
            slot = gpu.core.global_to_packed(gid)
            assert int(gpu.core.packed_to_global(slot)) == gid
    return got


def check(got, want, bounds, osh, what):
    ok, w = fs.excursions(got, want, bounds, osh)
    assert ok, (what, "counts differ from the rows'")
    assert w and max(w.values()) <= 1.0, (what, w)
    return w


def merge_worst(a, b):
    for key, v in b.items():
        a[key] = max(a.get(key, 0.0), v)
    return a


# ---------------------------------------------------------------------------
# ordered paths

ORDERED_RUNS = [(c, 0) for c in ORDERED] + [("gp", 2)]


@pytest.mark.parametrize("config,value_sorted", ORDERED_RUNS)
def test_ordered_statistics_are_in_the_band(config, value_sorted):
    osh, gsh, vals, assign = ordered_inputs(config)
    n, k = len(assign), 16
    gpu = make_engine(gsh, vals, assign, k, {"value_sorted": value_sorted})
    hist = [gpu.assignments().copy()]
    stages = [("load_rows", stats_of(gpu, osh), list(hist))]
    # (batches of 16 rows let groups die and appear; the value-sorted run
    # takes eight batches a sweep)
    batch = 16 if value_sorted == 0 else 250
    for s in range(2):
        gpu.sweep(0, n, batch, SEED, draw_base=s * n)
        hist.append(gpu.assignments().copy())
    assert len(set(hist[-1]) - set(hist[0])) > 0, "no group appeared"
    stages.append(("two sweeps", stats_of(gpu, osh), list(hist)))
    gpu.sweep_sequential(0, n, ol.oracle().orc_rng_seed(SEED + 1))
    hist.append(gpu.assignments().copy())
    stages.append(("sweep_sequential", stats_of(gpu, osh), list(hist)))
    if value_sorted == 2:
        assert gpu.core.debug_counts()["value_sorted_batches"] > 0
    for stage, got, h in stages:
        w = check(got, fs.truth(vals, osh, h[-1]),
                  fs.ordered_bounds(vals, osh, h), osh, (config, stage))
        print("ordered %s value_sorted=%d %s: excursion / band: %s" % (
            config, value_sorted, stage, fmt(w)))
    # the band sees a lost row where the issue's condition asks it to
    if config == "nich":
        h = stages[1][2]
        _, w = fs.excursions(stages[1][1],
                             fs.truth(vals, osh, h[-1], mut=("lost_add",)),
                             fs.ordered_bounds(vals, osh, h), osh)
        assert w["mean"] > 1.0, w


# ---------------------------------------------------------------------------
# merged path


def image_array(gpu, osh, image):
    """the image in the engine's layout: per feature in order, NICH
    [n | sum x | sum x^2] of K slots each, GammaPoisson [log_prod]"""
    K = len(gpu)
    blocks = []
    for f, kind in fs.float_features(osh):
        width = 3 if kind == fx.NICH else 1
        block = np.zeros((width, K))
        for gid, w in image[f].items():
            block[:, gpu.core.global_to_packed(int(gid))] = w
        blocks.append(block.ravel())
    return np.concatenate(blocks)


def expected_words(gpu, osh):
    K = len(gpu)
    return sum(3 * K if kind == fx.NICH else K
               for _, kind in fs.float_features(osh))


def import_image(gpu, arr):
    import torch
    assert gpu.core.float_delta_words() == arr.size
    t = torch.from_numpy(np.ascontiguousarray(arr, np.float64)).cuda()
    torch.cuda.synchronize()
    gpu.core.import_float_moments_dev(int(t.data_ptr()))
    torch.cuda.synchronize()


def export_image(gpu):
    import torch
    t = torch.zeros(gpu.core.float_delta_words(), dtype=torch.float64,
                    device="cuda")
    torch.cuda.synchronize()
    gpu.core.export_float_moments_dev(int(t.data_ptr()))
    torch.cuda.synchronize()
    return t.cpu().numpy()


def merged_engine(name, sampling=0):
    """loaded, and for an "import" start holding the float64 moments"""
    n, k, _, _, start, opts = MERGED[name]
    osh, gsh, vals, assign = merged_inputs(name)
    o = {"value_sorted": 0, "sampling": sampling, "float_stats": 1}
    o.update(opts)
    gpu = make_engine(gsh, vals, assign, k, o)
    assert gpu.core.float_delta_words() == expected_words(gpu, osh)
    if start == "import":
        first = gpu.assignments()
        import_image(gpu, image_array(gpu, osh,
                                      fs.image_of(vals, osh, first)))
    return gpu, osh, vals


_RUNS = {}


def merged_run(name, sampling=0, cached=True):
    """the case's sub-sweeps on the engine -> dict(gpu, osh, vals, hist,
    stats per step, bounds per step, truth per step)"""
    if cached and (name, sampling) in _RUNS:
        return _RUNS[name, sampling]
    n, start = MERGED[name][0], MERGED[name][4]
    gpu, osh, vals = merged_engine(name, sampling)
    hist = [gpu.assignments().copy()]
    stats = [stats_of(gpu, osh)]
    steps = batches_of(name)
    for s, b0, b1 in steps:
        gpu.sweep(b0, b1, b1 - b0, SEED, draw_base=s * n)
        hist.append(gpu.assignments().copy())
        stats.append(stats_of(gpu, osh))
    counts = gpu.core.debug_counts()
    assert counts["merged_batches"] == len(steps), counts
    if MERGED[name][5].get("value_sorted") == 2:
        assert counts["value_sorted_batches"] == len(steps), counts
    run = dict(gpu=gpu, osh=osh, vals=vals, hist=hist, stats=stats,
               bounds=fs.merged_bounds(vals, osh, hist, start),
               want=[fs.truth(vals, osh, h) for h in hist])
    if cached:
        _RUNS[name, sampling] = run
    return run


GPU_CASES = [(name, 0) for name in MERGED if name != "drain"] + [("benign", 1)]


@pytest.mark.parametrize("name,sampling", GPU_CASES)
def test_merged_statistics_are_in_the_band_after_every_sub_sweep(name,
                                                                 sampling):
    run = merged_run(name, sampling)
    hist, osh = run["hist"], run["osh"]
    moved = sum(int((a != b).sum()) for a, b in zip(hist[:-1], hist[1:]))
    assert moved > 0, "nothing moved"
    w = {}
    for t, (got, want, b) in enumerate(zip(run["stats"], run["want"],
                                           run["bounds"])):
        merge_worst(w, check(got, want, b, osh, (name, sampling, t)))
    print("merged %s sampling=%d (%s start, %d sub-sweeps, %d moves, K %d -> "
          "%d): excursion / band: %s" % (
              name, sampling, MERGED[name][4], len(hist) - 1, moved,
              len(run["stats"][0][next(iter(run["stats"][0]))]),
              len(run["gpu"]), fmt(w)))
    # the band is tight enough to see a lost row on the engine's own moves
    # (asserted where tests/test_f64_stats.py sets the condition, reported
    # elsewhere: how large the engine lets a group grow is its own business)
    mut = fs.truth(run["vals"], osh, hist[-1], mut=("lost_add",))
    _, seen = fs.excursions(run["stats"][-1], mut, run["bounds"][-1], osh)
    print("merged %s sampling=%d: lost_add shift / band: %s" % (
        name, sampling, fmt(seen)))
    if name in ("benign", "off100", "off1000", "pairs"):
        assert max(seen.values()) > 1.0, seen
    if name == "ten_blocks":
        # ten workgroups: one unrolled group of eight and a tail of two
        assert (MERGED[name][2][0] + fs.KAPPLY_ROWS - 1) // fs.KAPPLY_ROWS \
            == 10


def split_image(gpu, osh, arr):
    """-> {feature: (n, S, Q) arrays over the slots | (log_prod,)}"""
    K = len(gpu)
    out, at = {}, 0
    for f, kind in fs.float_features(osh):
        width = 3 if kind == fx.NICH else 1
        out[f] = arr[at:at + width * K].reshape(width, K)
        at += width * K
    assert at == arr.size
    return out


def check_export(gpu, osh, vals, assign, bounds, what):
    """the exported image against the rows' sums -> the image"""
    arr = export_image(gpu)
    img = split_image(gpu, osh, arr)
    rows = fs.image_of(vals, osh, assign)
    tr = fs.truth(vals, osh, assign)
    worst_s = worst_q = 0.0
    for f, kind in fs.float_features(osh):
        for gid, w in rows[f].items():
            slot = gpu.core.global_to_packed(int(gid))
            if kind != fx.NICH:
                # log_prod travels as it is held
                assert abs(img[f][0, slot] - w[0]) <= bounds[f][gid][1], (
                    what, gid)
                continue
            n, mu, _ = tr[f][gid]
            _, em, ec = bounds[f][gid]
            es, eq = fs.export_bounds(n, mu, em, ec)
            assert img[f][0, slot] == n, (what, gid)
            ds, dq = abs(img[f][1, slot] - w[1]), abs(img[f][2, slot] - w[2])
            assert ds <= es and dq <= eq, (what, gid, ds, es, dq, eq)
            worst_s = max(worst_s, fs._ratio(ds, es))
            worst_q = max(worst_q, fs._ratio(dq, eq))
    print("export %s: sum x %.3g, sum x^2 %.3g of the bound" % (
        what, worst_s, worst_q))
    return arr


@pytest.mark.parametrize("name", ["benign", "off100", "off1000", "off1e4",
                                  "constant", "pairs"])
def test_export_is_the_rows_sums_and_import_returns_the_bits(name):
    run = merged_run(name, cached=False)
    gpu, osh, vals, hist = run["gpu"], run["osh"], run["vals"], run["hist"]
    before = run["stats"][-1]
    arr = check_export(gpu, osh, vals, hist[-1], run["bounds"][-1], name)
    import_image(gpu, arr)
    after = stats_of(gpu, osh)
    band = fs.reimport_bounds(vals, osh, hist[-1], [np.arange(len(hist[0]))],
                              [run["bounds"][-1]])
    w = check(after, run["want"][-1], band, osh, (name, "re-imported"))
    same = other = 0
    for f, kind in fs.float_features(osh):
        for gid, s in before[f].items():
            t = after[f][gid]
            if kind == fx.GP:
                assert np.float32(t[1]) == np.float32(s[1]), (name, gid)
                continue
            assert t[:2] == s[:2], (name, gid, s, t)
            if s[0] < 2 or s[0] * s[1] * s[1] <= 2.0 ** 24 * s[2]:
                assert t[2] == s[2], (name, gid, s, t)
                same += 1
            else:
                other += 1
    print("%s: %d groups return bit for bit, %d within the band (%s)" % (
        name, same, other, fmt(w)))
    if name in ("benign", "off100", "off1000"):
        assert other == 0


@pytest.mark.parametrize("name", ["benign", "off1000", "pairs"])
def test_two_half_engines_images_sum_to_the_whole(name):
    n, k = MERGED[name][:2]
    osh, gsh, vals, assign = merged_inputs(name)
    opts = {"value_sorted": 0, "float_stats": 1}
    parts = [np.arange(0, n // 2), np.arange(n // 2, n)]
    total, pbounds = None, []
    for rows in parts:
        sub = [v[rows] for v in vals]
        half = make_engine(gsh, sub, assign[rows], k, opts)
        a = half.assignments()
        assert np.array_equal(a, assign[rows]), "slot layouts differ"
        b = fs.ordered_bounds(sub, osh, [a])
        pbounds.append(b)
        arr = check_export(half, osh, sub, a, b, "%s half" % name)
        total = arr if total is None else total + arr
    whole = make_engine(gsh, vals, assign, k, opts)
    import_image(whole, total)
    band = fs.reimport_bounds(vals, osh, assign, parts, pbounds)
    w = check(stats_of(whole, osh), fs.truth(vals, osh, assign), band, osh,
              name)
    print("%s, two halves: excursion / band: %s" % (name, fmt(w)))


# ---------------------------------------------------------------------------
# the caches follow the statistics


def merged_state(run):
    """fx.State of the run's last assignment with NICH's em / ec those of
    merged_bounds"""
    gpu, osh = run["gpu"], run["osh"]
    assign = run["hist"][-1]
    p2g = [int(gpu.core.packed_to_global(s)) for s in range(len(gpu))]
    st = fx.State(run["vals"], osh, assign, p2g,
                  ("py", float(np.float32(ALPHA)), float(np.float32(D))))
    for f, kind in fs.float_features(osh):
        if kind != fx.NICH:
            continue
        em, ec = np.zeros(st.K), np.zeros(st.K)
        for s, gid in enumerate(p2g):
            b = run["bounds"][-1][f].get(gid)
            if b is not None:
                assert b[0] == st.counts[s]
                em[s], ec[s] = b[1], b[2]
        st.stats[f].update(em=em, ec=ec)
    return st


@pytest.mark.parametrize("name", ["benign", "off100"])
def test_score_rows_follow_the_merged_statistics(name):
    """a NICH cache left stale by k_merge_float_apply or by the import shows
    as a score outside the float64 band"""
    run = merged_run(name)
    gpu = run["gpu"]
    n = MERGED[name][0]
    st = merged_state(run)
    out = score_rows(gpu, 0, n)
    w = 0.0
    for r0 in range(0, n, 500):
        sel = np.arange(r0, min(n, r0 + 500))
        v, b, _ = fx.score_rows_f64(st, sel)
        w = max(w, worst(out[sel], v, b))
    print("%s: score_rows_dev after the merged sub-sweeps, worst excursion / "
          "band %.3f" % (name, w))
    assert w <= 1.0
    # ... and right after an import, before any sweep
    fresh, osh, vals = merged_engine("off100")
    run0 = dict(gpu=fresh, osh=osh, vals=vals, hist=[fresh.assignments()],
                bounds=fs.merged_bounds(vals, osh, [fresh.assignments()],
                                        "import"))
    st0 = merged_state(run0)
    v, b, _ = fx.score_rows_f64(st0, np.arange(0, 500))
    w0 = worst(score_rows(fresh, 0, 500), v, b)
    print("off100 after the import alone: worst excursion / band %.3f" % w0)
    assert w0 <= 1.0


def test_scores_are_finite_on_a_constant_group():
    run = merged_run("constant")
    out = score_rows(run["gpu"], 0, MERGED["constant"][0])
    assert np.all(np.isfinite(out))
    # the constant group held its rows' exact moments after the import
    f = 1
    n, mean, ctv = run["stats"][0][f][0]
    assert (mean, ctv) == (1000.125, 0.0), (n, mean, ctv)
