"""The float statistics held to the float64 moments of their rows
(tests/f64_stats.py), without a GPU.

Ordered path: the oracle's NICH (count, mean, count_times_variance) and
GammaPoisson log_prod -- what k_replay_sorted, the load's replay and
k_chains are bit-exact to -- after init_from_assignments, after two sweeps of
small batches and after a sequential sweep: counts equal to the truth, floats
within the ordered bounds.

Merged path (float_stats = 1): the kernels' numpy restatement
(f64_stats.Restated) stays inside `merged_bounds` after every sub-sweep of
the cases tests/test_gpu_stats_f64.py runs on the engine, and every planted
bug leaves the band on the cases named for it.  The histories are drawn with
numpy; the engine's own moves are the GPU file's subject.

`drain` (a group down to one row, to none, two rows back, then all) is held
on the restatement only: the engine offers no entry point that applies
chosen moves -- batch_apply_float_delta_dev takes an image, but on an open
batch whose integer statistics and assignments are the engine's own draw, and
an image at odds with them would leave NICH's count (which the merged apply
writes) different from the driver's."""
import numpy as np
import pytest

import f64_stats as fs
import f64_scores as fx
import oracle_lib as ol
import workloads
from distributions_amd import engine

SEED = 5


# ---------------------------------------------------------------------------
# the merged cases (shared with tests/test_gpu_stats_f64.py)

# name: (n, k, [batch sizes of one sweep] or batch, sweeps, start, options)
MERGED = {
    "benign": (2000, 16, 500, 2, "load", {}),
    "off100": (2000, 16, 500, 2, "import", {}),
    "off1000": (2000, 16, 500, 2, "import", {}),
    "off1e4": (2000, 16, 500, 2, "import", {}),
    "tiny_sd": (2000, 16, 500, 2, "import", {}),
    "constant": (512, 8, 128, 2, "import", {}),
    "drain": (512, 8, None, 1, "import", {}),
    "pairs": (256, 128, 64, 2, "load", {}),
    "ten_blocks": (73729 + 4096, 16, [73729, 4096], 1, "import", {}),
    "gp_value_sorted": (8192, 16, 4096, 2, "load", {"value_sorted": 2}),
}
OFFSETS = {"off100": (100.0, 1.0), "off1000": (1000.0, 1.0),
           "off1e4": (1e4, 1.0), "tiny_sd": (0.0, 1e-3),
           "constant": (1000.0, 1.0), "drain": (1000.0, 1.0),
           "ten_blocks": (100.0, 1.0)}


def gp_nich(n, mean, sd, seed=workloads.SEED):
    """GammaPoisson + NICH with N(mean, sd) values, the prior centred there
    -> (oracle shareds, engine shareds, values)"""
    rng = np.random.default_rng(seed)
    vals = [rng.poisson(5.0, n).astype(np.uint32),
            (mean + sd * rng.normal(0, 1, n)).astype(np.float32)]
    s2 = float(np.float32(sd * sd))
    osh = [ol.make_shared(ol.GP, alpha=1.0, inv_beta=1.0),
           ol.make_shared(ol.NICH, mu=mean, kappa=1.0, sigmasq=s2, nu=1.0)]
    gsh = [engine.gp_shared(1.0, 1.0), engine.nich_shared(mean, 1.0, s2, 1.0)]
    return osh, gsh, vals


def merged_inputs(name):
    """-> (oracle shareds, engine shareds, values, packed assignment)"""
    n, k = MERGED[name][:2]
    assign = (np.arange(n) % k).astype(np.uint32)
    if name in ("benign", "pairs"):
        osh, gsh, vals, _ = workloads.make("gp_nich", n, k)
    elif name == "gp_value_sorted":
        osh, gsh, vals, _ = workloads.make("gp", n, k)
    else:
        osh, gsh, vals = gp_nich(n, *OFFSETS[name])
        if name == "constant":
            vals[1][assign == 0] = np.float32(1000.125)
    return osh, gsh, vals, assign


def batches_of(name):
    n, _, batch, sweeps = MERGED[name][:4]
    out = []
    for s in range(sweeps):
        b = 0
        sizes = batch if isinstance(batch, list) else [batch] * (
            (n + batch - 1) // batch)
        for size in sizes:
            out.append((s, b, min(n, b + size)))
            b += size
    return out


def drawn_history(name):
    """assignments at the start and after every sub-sweep, drawn with numpy:
    half of a batch's rows move, to a group alive at the time or (one row in
    fifty) to a group new with this batch"""
    n, k = MERGED[name][:2]
    rng = np.random.default_rng(SEED)
    cur = (np.arange(n) % k).astype(np.int64)
    hist = [cur.copy()]
    if name == "drain":
        g = np.nonzero(cur == 3)[0]
        other = (np.arange(len(g)) % 3).astype(np.int64)   # groups 0, 1, 2
        for keep in (g[:1], g[:0], g[:2], g):
            cur = cur.copy()
            cur[g] = other
            cur[keep] = 3
            # (and some traffic among the other groups)
            rest = rng.choice(np.nonzero(hist[0] != 3)[0], 60, replace=False)
            cur[rest] = rng.choice([0, 1, 2, 4, 5, 6, 7], 60)
            hist.append(cur)
        return hist
    next_id = k
    for _, b0, b1 in batches_of(name):
        cur = cur.copy()
        rows = np.arange(b0, b1)
        alive = np.unique(cur)
        move = rng.random(len(rows)) < 0.5
        to = rng.choice(alive, len(rows))
        fresh = rng.random(len(rows)) < 0.02
        to[fresh] = next_id
        next_id += 1
        cur[rows[move]] = to[move]
        hist.append(cur)
    return hist


_MERGED = {}


def merged_case(name):
    """(oracle shareds, values, history, bounds per step, truth per step)"""
    if name not in _MERGED:
        osh, _, vals, _ = merged_inputs(name)
        hist = drawn_history(name)
        start = MERGED[name][4]
        bounds = fs.merged_bounds(vals, osh, hist, start)
        want = [fs.truth(vals, osh, h) for h in hist]
        _MERGED[name] = (osh, vals, hist, bounds, want)
    return _MERGED[name]


def worst_over_steps(got, want, bounds, osh):
    """-> {statistic: largest excursion / band over the steps}"""
    worst = {}
    for g, w, b in zip(got, want, bounds):
        ok, r = fs.excursions(g, w, b, osh)
        assert ok, "counts differ from the rows'"
        for key, v in r.items():
            worst[key] = max(worst.get(key, 0.0), v)
    return worst


def fmt(worst):
    return ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))


# ---------------------------------------------------------------------------
# the ordered path: the oracle

ORDERED = ["nich", "nich2", "gp", "gp_nich", "planted"]


def ordered_inputs(config, n=2000, k=16):
    if config == "planted":
        _, osh, gsh, vals = workloads.planted(n, k_true=16, n_cat=4, n_real=2)
        assign = (np.arange(n) % k).astype(np.uint32)
    else:
        osh, gsh, vals, assign = workloads.make(config, n, k)
    return osh, gsh, vals, assign


def read_groups(mix, osh):
    """the statistics of a mixture (oracle or engine) per global id
    -> {feature: {id: (n, mean, ctv) | (n, log_prod)}}"""
    out = {}
    K = len(mix)
    gids = [int(mix.core.packed_to_global(s)) for s in range(K)]
    for f, kind in fs.float_features(osh):
        res = {}
        for s, gid in enumerate(gids):
            w = np.ascontiguousarray(mix.get_group(f, s)).view(np.uint32)
            fl = w.view(np.float32)
            if kind == fx.NICH:
                res[gid] = (int(w[:1].view(np.int32)[0]), float(fl[1]),
                            float(fl[2]))
            else:
                res[gid] = (int(w[0]), float(fl[2]))
        out[f] = res
    return out


_ORDERED = {}


def ordered_states(config):
    """[(stage, oracle statistics, history)] at the three stages"""
    if config in _ORDERED:
        return _ORDERED[config]
    osh, _, vals, assign = ordered_inputs(config)
    n, k = len(assign), 16
    orc = ol.OracleMixture(20.0, 0.5, osh)
    orc.init_from_assignments(vals, assign, k, 1)
    hist = [orc.assign.copy()]
    out = [("init", read_groups(orc, osh), list(hist))]
    seed = ol.oracle().orc_rng_seed(SEED)
    for s in range(2):
        for b in range(0, n, 16):
            orc.gibbs_batch(b, min(n, b + 16), seed, s * n)
        hist.append(orc.assign.copy())
    assert len(set(hist[-1]) - set(hist[0])) > 0, "no group appeared"
    out.append(("two sweeps", read_groups(orc, osh), list(hist)))
    orc.gibbs_sequential(0, n, ol.oracle().orc_rng_seed(SEED + 1))
    hist.append(orc.assign.copy())
    out.append(("sequential", read_groups(orc, osh), list(hist)))
    _ORDERED[config] = (osh, vals, out)
    return _ORDERED[config]


@pytest.mark.parametrize("config", ORDERED)
def test_oracle_float_statistics_are_in_the_ordered_band(config):
    osh, vals, stages = ordered_states(config)
    for stage, got, hist in stages:
        want = fs.truth(vals, osh, hist[-1])
        ok, worst = fs.excursions(got, want,
                                  fs.ordered_bounds(vals, osh, hist), osh)
        print("%s %s: excursion / band: %s" % (config, stage, fmt(worst)))
        assert ok, (config, stage, "counts differ from the rows'")
        assert worst and max(worst.values()) <= 1.0, (config, stage, worst)


def test_ordered_lost_add_is_seen_on_the_mean_at_nich():
    """a condition, not a measurement: at the benign column a member missing
    from the largest group's sums must leave the MEAN's ordered band after
    two sweeps of batches"""
    osh, vals, stages = ordered_states("nich")
    for stage, got, hist in stages[:2]:
        want = fs.truth(vals, osh, hist[-1], mut=("lost_add",))
        _, worst = fs.excursions(got, want,
                                 fs.ordered_bounds(vals, osh, hist), osh)
        print("lost_add, ordered nich %s: %s" % (stage, fmt(worst)))
        assert worst["mean"] > 1.0, (stage, worst)


@pytest.mark.parametrize("config", ORDERED)
def test_ordered_truth_mutants(config):
    """the float64-side mutants against the oracle after two sweeps; what the
    worst-case Welford band cannot see is in UNSEEN_ORDERED"""
    osh, vals, stages = ordered_states(config)
    stage, got, hist = stages[1]
    bounds = fs.ordered_bounds(vals, osh, hist)
    kinds = {kind for _, kind in fs.float_features(osh)}
    for mutant in fs.TRUTH_MUTANTS:
        if mutant == "gp_factorial_off" and fx.GP not in kinds:
            continue
        want = fs.truth(vals, osh, hist[-1], mut=(mutant,), prev=hist[-2])
        _, worst = fs.excursions(got, want, bounds, osh)
        w = max(worst.values())
        print("%s at ordered %s: shift / band %.3g (%s)" % (
            mutant, config, w, fmt(worst)))
        if (mutant, config) in UNSEEN_ORDERED:
            assert w <= 1.0, "seen after all: take it off the list"
        else:
            assert w > 1.0, (mutant, config, worst)


# (mutant, config) the ordered bounds do not see after two sweeps, with the
# measured largest shift / band.  nich_welford_bounds charges each of a
# group's ~250 adds and removes per sweep its worst case, so on `planted`,
# whose columns sit at cluster means of up to ~10 with a spread of 0.5 and
# whose groups mix clusters after the load, the band on the mean and on ctv
# is wider than what one row moves.
UNSEEN_ORDERED = {("lost_add", "planted"): 0.67}


# ---------------------------------------------------------------------------
# the merged path: the restatement


@pytest.mark.parametrize("name", list(MERGED))
def test_restated_merge_stays_in_the_band_after_every_sub_sweep(name):
    osh, vals, hist, bounds, want = merged_case(name)
    start = MERGED[name][4]
    # (the binary64 sums are order-free in the band: row order and a drawn
    # order must both hold)
    for rng in (None, np.random.default_rng(1)):
        got = fs.merged_restated(vals, osh, hist, start, rng=rng)
        per_step = []
        for g, w, b in zip(got, want, bounds):
            ok, r = fs.excursions(g, w, b, osh)
            assert ok, name
            per_step.append(max(r.values()))
        worst = worst_over_steps(got, want, bounds, osh)
        print("%s (%s start, %d sub-sweeps, sums in %s order): excursion / "
              "band: %s" % (name, start, len(hist) - 1,
                            "row" if rng is None else "drawn", fmt(worst)))
        assert max(per_step) <= 1.0, (name, per_step)


def test_drain_goes_through_one_row_and_none():
    osh, vals, hist, bounds, want = merged_case("drain")
    sizes = [int((h == 3).sum()) for h in hist]
    assert sizes == [64, 1, 0, 2, 64]
    got = fs.merged_restated(vals, osh, hist, "import")
    f = 1
    assert got[1][f][3][2] == 0.0            # one row: no variance
    assert got[2][f][3] == (0, 0.0, 0.0)     # none: zeros, then gone
    assert 3 not in fs.truth(vals, osh, hist[2])[f]
    assert got[3][f][3][0] == 2 and got[3][f][3][2] > 0.0


# which cases each mutant is run on
NAMED = {
    "sq_f32": ["benign", "off100", "off1000", "off1e4", "ten_blocks"],
    "no_recentre": ["benign", "off100", "off1000", "off1e4", "constant",
                    "tiny_sd"],
    "skip_n_unchanged": ["benign", "off100", "pairs"],
    "stale_on_empty": ["drain", "pairs"],
    "var_at_one": ["drain", "pairs"],
    "gp_sign": ["benign", "off100", "gp_value_sorted"],
    "lost_add": list(MERGED),
    "lost_remove": ["benign", "off100", "off1000", "pairs", "drain"],
    "gp_factorial_off": ["benign", "off100", "gp_value_sorted", "pairs",
                         "ten_blocks"],
}

# (mutant, case) that stay inside the band, with the measured largest
# shift / band over the sub-sweeps and why.  None at present: the per-batch
# band is a few binary32 roundings wide, and every planted bug moves a
# statistic by at least a row's worth on every case named for it --
# ten_blocks included, where one member in about 4 600 still moves the mean
# by 8 bands and log_prod by 2 000.
UNSEEN = {}


def mutant_ratio(mutant, name):
    osh, vals, hist, bounds, want = merged_case(name)
    start = MERGED[name][4]
    if mutant in fs.KERNEL_MUTANTS:
        got = fs.merged_restated(vals, osh, hist, start, mut=(mutant,))
    else:
        got = fs.merged_restated(vals, osh, hist, start)
        want = [want[0]] + [fs.truth(vals, osh, h, mut=(mutant,), prev=p)
                            for p, h in zip(hist[:-1], hist[1:])]
    worst = {}
    for g, w, b in zip(got, want, bounds):
        _, r = fs.excursions(g, w, b, osh)
        for key, v in r.items():
            worst[key] = max(worst.get(key, 0.0), v)
    return worst


PAIRS = [(m, c) for m, cases in NAMED.items() for c in cases]


@pytest.mark.parametrize("mutant,name", PAIRS)
def test_planted_bug_leaves_the_merged_band(mutant, name):
    worst = mutant_ratio(mutant, name)
    w = max(worst.values())
    print("%s at %s: shift / band %.3g (%s)" % (mutant, name, w, fmt(worst)))
    if (mutant, name) in UNSEEN:
        assert w <= 1.0, "seen after all: take it off the list"
        return
    assert w > 1.0, (mutant, name, worst)


def test_every_mutant_is_seen_somewhere():
    for mutant, cases in NAMED.items():
        assert [c for c in cases if (mutant, c) not in UNSEEN], mutant


@pytest.mark.parametrize("mutant", ["lost_add", "sq_f32", "no_recentre"])
@pytest.mark.parametrize("name", ["off100", "off1000"])
def test_conditions_on_the_import_cases(mutant, name):
    """conditions, not measurements: where the column's mean is large against
    its spread the band must still see a lost member, binary32 squares and a
    forgotten re-centring, each by more than a factor of two"""
    worst = mutant_ratio(mutant, name)
    print("%s at %s: %s" % (mutant, name, fmt(worst)))
    assert max(worst["mean"], worst["ctv"]) > 2.0, (mutant, name, worst)


# ---------------------------------------------------------------------------
# import / export


def bits(x):
    return np.float32(x).view(np.uint32)


@pytest.mark.parametrize("name", list(MERGED))
def test_export_then_import_is_the_identity_on_the_bits(name):
    """k_merge_float_export then apply(reset): n mean is exact in binary64,
    so the mean returns; ctv returns as fl(fl(c + q) - q) with q =
    fl(n mean mean), whose error v (c + q) is below half a binary32 ulp of c
    wherever n mean^2 <= 2^24 ctv.  Elsewhere: within the band of a
    re-import of the statistics' own image."""
    osh, vals, hist, bounds, want = merged_case(name)
    r = fs.Restated(vals, osh)
    r.load(hist[0])
    if MERGED[name][4] == "import":
        r.import_image(fs.image_of(vals, osh, hist[0]))
    for old, new in zip(hist[:-1], hist[1:]):
        r.batch(old, new)
    before = {f: dict(s) for f, s in r.st.items()}
    r.import_image(r.export_image())
    band = fs.reimport_bounds(vals, osh, hist[-1], [np.arange(len(hist[0]))],
                              [bounds[-1]])
    ok, worst = fs.excursions(r.st, want[-1], band, osh)
    assert ok and max(worst.values()) <= 1.0, (name, worst)
    same = other = 0
    for f, kind in fs.float_features(osh):
        for g, s in before[f].items():
            t = r.st[f][g]
            if kind == fx.GP:
                assert bits(t[1]) == bits(s[1])
                continue
            assert t[0] == s[0] and bits(t[1]) == bits(s[1]), (name, g)
            if s[0] * s[1] * s[1] <= 2.0 ** 24 * s[2] or s[0] < 2:
                assert bits(t[2]) == bits(s[2]), (name, g, s, t)
                same += 1
            else:
                other += 1
    print("%s: %d groups return bit for bit, %d within the band (%s)" % (
        name, same, other, fmt(worst)))


@pytest.mark.parametrize("name", ["benign", "off1000", "pairs"])
def test_images_of_two_halves_sum_to_the_whole(name):
    osh, vals, hist, _, _ = merged_case(name)
    assign = hist[0]
    n = len(assign)
    parts = [np.arange(0, n // 2), np.arange(n // 2, n)]
    total, pbounds = {}, []
    for rows in parts:
        sub = [np.asarray(v)[rows] for v in vals]
        r = fs.Restated(sub, osh)
        r.load(assign[rows])
        pbounds.append(fs.ordered_bounds(sub, osh, [assign[rows]]))
        for f, img in r.export_image().items():
            for g, w in img.items():
                a = total.setdefault(f, {}).get(g, (0.0,) * len(w))
                total[f][g] = tuple(x + y for x, y in zip(a, w))
    whole = fs.Restated(vals, osh)
    whole.set_counts(assign)
    whole.import_image(total)
    band = fs.reimport_bounds(vals, osh, assign, parts, pbounds)
    ok, worst = fs.excursions(whole.st, fs.truth(vals, osh, assign), band,
                              osh)
    print("%s, two halves: excursion / band: %s" % (name, fmt(worst)))
    assert ok and max(worst.values()) <= 1.0, (name, worst)
    # a half left out is seen
    part = fs.Restated(vals, osh)
    part.set_counts(assign)
    r = fs.Restated([np.asarray(v)[parts[0]] for v in vals], osh)
    r.load(assign[parts[0]])
    part.import_image(r.export_image())
    for f, kind in fs.float_features(osh):      # (n as the whole's)
        if kind == fx.NICH:
            part.st[f] = {g: (whole.st[f][g][0],) + s[1:]
                          for g, s in part.st[f].items()}
    _, seen = fs.excursions(part.st, fs.truth(vals, osh, assign), band, osh)
    assert max(seen.values()) > 1.0, seen
