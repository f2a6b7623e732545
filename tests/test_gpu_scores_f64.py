"""The engine's row scores held to float64 predictives (tests/f64_scores.py):
`row_scores` (k_row_scores, batch semantics) and `score_rows_dev`
(k_score_rows, Mixture::score_value over resident rows into a device buffer).

Both are compared bit for bit with the oracle (orc_mix_batch_row_scores; the
oracle's driver + slave score_value in sequence) and against the float64
band.  score_rows_dev reads the group caches (shifted, shift_full, counts),
which every sweep path must leave current: after sweeps on each path it must
still equal the oracle after the same sweeps."""
import numpy as np
import pytest

import f64_scores as fx
import oracle_lib as ol
import workloads
from test_f64_scores import CONFIGS, oracle_sequential_scores, worst

pytestmark = pytest.mark.gpu

SEED = 5
SENTINEL = -12345.5


def _le(orc, dataset_size):
    import ctypes
    orc.L.orc_mix_set_low_entropy.restype = None
    orc.L.orc_mix_set_low_entropy.argtypes = [ctypes.c_void_p, ctypes.c_int]
    orc.L.orc_mix_set_low_entropy(orc.h, dataset_size)


def both(osh, gsh, vals, assign, k, empty, alpha=1.0, d=0.0, le=None,
         opts=None):
    from distributions_amd import engine
    orc = ol.OracleMixture(alpha, d, osh)
    if le is not None:
        _le(orc, le)
    orc.init_from_assignments(vals, assign, k, empty)
    gpu = (engine.Gibbs(alpha, d, gsh) if le is None
           else engine.Gibbs(alpha, d, gsh, dataset_size=le))
    for key, value in (opts or {}).items():
        gpu.set_option(key, value)
    gpu.load_rows(vals, assign, k, empty)
    return orc, gpu


def sweep_both(orc, gpu, sweeps, batch, alpha_seed=SEED):
    n = orc.n_rows
    history = [orc.assign.copy()]
    st = ol.oracle().orc_rng_seed(alpha_seed)
    for s in range(sweeps):
        for b in range(0, n, batch):
            orc.gibbs_batch(b, min(n, b + batch), st, s * n)
        gpu.sweep(0, n, batch, alpha_seed, draw_base=s * n)
        history.append(orc.assign.copy())
    assert np.array_equal(gpu.assignments(), orc.assign)
    return history


def f64_state(orc, vals, prior, history):
    p2g = [orc.packed_to_global(i) for i in range(len(orc))]
    return fx.State(vals, orc.shareds, orc.assign, p2g, prior, history)


def score_rows(gpu, r0, r1, ld=None):
    """score_rows_dev into a sentinel-filled device buffer -> numpy"""
    import torch
    K = len(gpu)
    ld = K if ld is None else ld
    out = torch.full((max(r1 - r0, 1), ld), SENTINEL, dtype=torch.float32,
                     device="cuda")
    torch.cuda.synchronize()
    gpu.core.score_rows_dev(r0, r1, int(out.data_ptr()), ld)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# name: (config, n, k, empty, d, sweeps, prior)
CASES = {}
for _c in CONFIGS:
    CASES[_c] = (_c, 2000, 16, 3, 0.5, 0, None)
    CASES[_c + "_swept"] = (_c, 2000, 16, 1, 0.5, 2, None)
CASES["dd256_k1024"] = ("dd", 4096, 1024, 1, 0.5, 0, None)
CASES["le_dd"] = ("dd", 2000, 16, 1, 0.0, 0, 2000)
CASES["le_gp_nich"] = ("gp_nich", 2000, 16, 1, 0.0, 0, 3000)
CASES["planted"] = ("planted", 2000, 16, 1, 0.5, 1, None)


@pytest.mark.parametrize("name", list(CASES))
def test_scores_bit_exact_and_in_the_float64_band(name):
    config, n, k, empty, d, sweeps, le = CASES[name]
    if config == "planted":
        _, osh, gsh, vals = workloads.planted(n, k_true=16, n_cat=4,
                                              n_real=2)
        assign = (np.arange(n) % k).astype(np.uint32)
    else:
        osh, gsh, vals, assign = workloads.make(
            config, n, k, dim=256 if k == 1024 else None)
    alpha = 20.0 if sweeps else 1.0
    orc, gpu = both(osh, gsh, vals, assign, k, empty, alpha, d, le)
    history = sweep_both(orc, gpu, sweeps, 16) if sweeps else [
        orc.assign.copy()]
    prior = ("le", le) if le else ("py", float(np.float32(alpha)),
                                   float(np.float32(d)))
    st = f64_state(orc, vals, prior, history)
    K = st.K
    assert len(gpu) == K
    # row_scores: a handful of rows (k_row_scores is one thread)
    rows = fx.checked_rows(st)
    rows = np.unique(np.r_[rows[np.linspace(0, len(rows) - 1, 6).astype(int)],
                           np.nonzero(st.counts[st.slot] == 1)[0][:2]])
    v, b, kl = fx.row_scores_f64(st, rows)
    got = np.full((len(rows), K), np.nan)
    for i, r in enumerate(rows):
        s = gpu.row_scores(int(r))
        assert bits_equal(s, orc.row_scores(int(r), int(st.slot[r]))), r
        got[i, :len(s)] = s
    w_rows = worst(got, v, b)
    # score_rows_dev: every row
    out = score_rows(gpu, 0, n)
    want = oracle_sequential_scores(orc, st, np.arange(n))
    assert bits_equal(out, want), "score_rows_dev != oracle score_value"
    w_dev = 0.0
    for r0 in range(0, n, 512):
        sel = np.arange(r0, min(n, r0 + 512))
        v2, b2, _ = fx.score_rows_f64(st, sel)
        w_dev = max(w_dev, worst(out[sel], v2, b2))
    kinds = "+".join(fx.NAMES[f.kind] for f in st.feats)
    print("%s (%s) K=%d: worst excursion / band: row_scores %.3f, "
          "score_rows_dev %.3f" % (name, kinds, K, w_rows, w_dev))
    assert w_rows <= 1.0 and w_dev <= 1.0


def test_score_rows_leading_dimension_row_begin_and_empty_range():
    osh, gsh, vals, assign = workloads.make("gp_nich", 3000, 40)
    orc, gpu = both(osh, gsh, vals, assign, 40, 2, 1.0, 0.2)
    K = len(gpu)
    st = f64_state(orc, vals, ("py", 1.0, float(np.float32(0.2))),
                   [orc.assign.copy()])
    full = score_rows(gpu, 0, 3000)
    padded = score_rows(gpu, 0, 3000, ld=K + 7)
    assert bits_equal(padded[:, :K], full)
    assert np.all(padded[:, K:] == SENTINEL), "padding columns written"
    part = score_rows(gpu, 1234, 2001, ld=K + 1)
    assert bits_equal(part[:, :K], full[1234:2001])
    assert np.all(part[:, K:] == SENTINEL)
    none = score_rows(gpu, 700, 700)
    assert np.all(none == SENTINEL), "an empty range wrote"
    v, b, _ = fx.score_rows_f64(st, np.arange(1234, 2001))
    assert worst(part[:, :K], v, b) <= 1.0
    # launches cut into chunks of whole rows: the same bits
    for chunk in (3 * K + 5, 1):
        gpu.set_option("debug.score_rows_chunk", chunk)
        assert bits_equal(score_rows(gpu, 11, 2999), full[11:2999]), chunk
    with pytest.raises(RuntimeError, match="score_rows_chunk"):
        gpu.set_option("debug.score_rows_chunk", 0)


def test_score_rows_refuses_an_open_batch():
    """the caches are the frozen state's only between batches: like
    row_scores, score_rows_dev refuses while one is open"""
    osh, gsh, vals, assign = workloads.make("dd", 2048, 16)
    orc, gpu = both(osh, gsh, vals, assign, 16, 1, 1.0, 0.2)
    before = score_rows(gpu, 0, 2048)
    gpu.core.batch_sample(0, 1024, ol.oracle().orc_rng_seed(3), 0)
    with pytest.raises(RuntimeError, match="batch open"):
        gpu.row_scores(0)
    with pytest.raises(RuntimeError, match="batch open"):
        score_rows(gpu, 0, 2048)
    gpu.core.batch_apply_local()
    gpu.core.batch_finish()
    orc.gibbs_batch(0, 1024, ol.oracle().orc_rng_seed(3), 0)
    assert np.array_equal(gpu.assignments(), orc.assign)
    after = score_rows(gpu, 0, 2048)
    st = f64_state(orc, vals, ("py", 1.0, float(np.float32(0.2))), None)
    assert bits_equal(after, oracle_sequential_scores(orc, st,
                                                      np.arange(2048)))
    assert not bits_equal(after, before)


def test_score_rows_k8192_dpd_10000_values():
    n = 24000
    osh, gsh, vals, assign = workloads.make("dpd", n, 8191, dim=10000)
    orc, gpu = both(osh, gsh, vals, assign, 8191, 1, 1.0, 0.2)
    K = len(gpu)
    assert K == 8192
    st = f64_state(orc, vals, ("py", 1.0, float(np.float32(0.2))), None)
    out = score_rows(gpu, 0, n)
    rows = np.r_[np.arange(0, n, 97), n - 1]
    want = oracle_sequential_scores(orc, st, rows)
    assert bits_equal(out[rows], want)
    sel = rows[::8]
    v, b, _ = fx.score_rows_f64(st, sel)
    w = worst(out[sel], v, b)
    print("dpd K=8192 V=10000: worst excursion / band %.3f" % w)
    assert w <= 1.0


# path: (config, options, how the state moves)
PATHS = {
    "default": ("dd", {}, "batch"),
    "value_sorted": ("dd", {"value_sorted": 2, "value_stream": 0,
                            "narrow_tiles": 0}, "batch"),
    "stream": ("dpd", {"value_sorted": 2, "value_stream": 2,
                       "narrow_tiles": 0}, "batch"),
    "narrow": ("dd", {"value_sorted": 2, "value_stream": 0,
                      "narrow_tiles": 2}, "batch"),
    "generic": ("dd", {"value_sorted": 0}, "batch"),
    "program_kernel": ("gp_nich", {"value_sorted": 0,
                                   "debug.rows_scratch": 0}, "batch"),
    "rows_scratch": ("gp_nich", {}, "batch"),
    "sweep_sequential": ("gp_nich", {}, "sequential"),
    "sweep_sequential_dd": ("dd", {}, "sequential"),
    "init_sequential": ("dd_bb_gp", {}, "init"),
    "init_sequential_nich": ("nich", {}, "init"),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_score_rows_after_sweeps_on_every_path(path):
    """a stale `shifted`, `shift_full`, `counts` or feature cache left by a
    sweep path shows here as a difference from the oracle after the same
    sweeps"""
    from distributions_amd import engine
    config, opts, how = PATHS[path]
    n, k = 4096, 32
    osh, gsh, vals, assign = workloads.make(config, n, k)
    alpha, d = 1.0, 0.2
    if how == "init":
        orc = ol.OracleMixture(alpha, d, osh)
        orc.init_empty(vals, 1)
        gpu = engine.Gibbs(alpha, d, gsh)
        gpu.load_rows_unassigned(vals, 1)
        st0 = ol.oracle().orc_rng_seed(11)
        assert orc.init_sequential(0, n, st0) == gpu.init_sequential(0, n,
                                                                     st0)
    else:
        orc, gpu = both(osh, gsh, vals, assign, k, 1, alpha, d, opts=opts)
    checks = 0
    for sweep in range(3):
        if how == "sequential":
            s0 = ol.oracle().orc_rng_seed(100 + sweep)
            assert orc.gibbs_sequential(0, n, s0) == gpu.sweep_sequential(
                0, n, s0)
        elif how == "batch":
            stt = ol.oracle().orc_rng_seed(21)
            for b in range(0, n, 1024):
                orc.gibbs_batch(b, b + 1024, stt, sweep * n)
            gpu.sweep(0, n, 1024, 21, draw_base=sweep * n)
        elif sweep > 0:
            stt = ol.oracle().orc_rng_seed(31)
            orc.gibbs_batch(0, n, stt, sweep * n)
            gpu.sweep(0, n, n, 31, draw_base=sweep * n)
        assert np.array_equal(gpu.assignments(), orc.assign), sweep
        st = f64_state(orc, vals, ("py", 1.0, float(np.float32(d))), None)
        got = score_rows(gpu, 0, n)
        want = oracle_sequential_scores(orc, st, np.arange(n))
        assert bits_equal(got, want), "%s: stale after sweep %d" % (path,
                                                                    sweep)
        checks += 1
    assert checks == 3
    if how == "batch" and opts.get("value_sorted") == 2:
        counts = gpu.core.debug_counts()
        key = {"stream": "stream_batches", "narrow": "narrow_batches"}.get(
            path, "value_sorted_batches")
        assert counts[key] > 0, counts
