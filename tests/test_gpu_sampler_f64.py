"""Every batched sampling path held to the float64 inverse CDF, row by row
(tests/f64_sampling.py).

One batch from a known state: every checked row's draw must be the float64
index of its batch-semantics scores and uniform, or -- where u W falls within
the path's proven band of a boundary -- a neighbour whose interval comes
within that band.  The exact paths are bit-exact against the oracle elsewhere;
the scan paths (sampling = 1) have no other per-row reference.

The scores are the oracle's (orc_mix_batch_row_scores), which
test_row_scores_match_oracle pins bit for bit to the engine's row_scores;
here every case re-checks that on a sample of its rows."""
import ctypes
import time

import numpy as np
import pytest

import f64_sampling as fs
import oracle_lib as ol
import wide_rows
import workloads

pytestmark = pytest.mark.gpu

SEED = 90210


def tab_scores(orc, x_values, g):
    """per row, the score of its value in its own slot with the row still in
    the group (what k_vs_scan_prepare tabulates), batch shift"""
    K = len(orc)
    alpha = orc._alpha
    fix = (np.float32(np.log(orc.n_rows + alpha))
           - np.float32(np.log(orc.n_rows - 1 + alpha)))
    out = np.zeros(len(g), np.float64)
    sc = np.zeros(K, np.float32)
    for x in np.unique(x_values):
        at = x_values == x
        orc.L.orc_mix_driver_score_value(orc.h, sc)
        orc.L.orc_mix_slave_score_value(orc.h, 0, int(x), sc)
        out[at] = sc[g[at]] + fix
    return out


def nich_dominant(n, k):
    """k well separated clusters of a real feature with a tiny prior
    variance, rows in their own cluster: one group dominates every row and
    the others lie far below max - 88 (fast_exp's flush edge)"""
    from distributions_amd import engine
    rng = np.random.default_rng(7)
    assign = (np.arange(n) % k).astype(np.uint32)
    x = (assign * 40.0 + rng.normal(0, 0.05, n)).astype(np.float32)
    osh = [ol.make_shared(ol.NICH, mu=0.0, kappa=1.0, sigmasq=1e-3, nu=1.0)]
    gsh = [engine.nich_shared(0.0, 1.0, 1e-3, 1.0)]
    return osh, gsh, [x], assign


def dd_ties(n, k):
    """every group holds the same multiset of values: the scores of all
    slots but the row's own are exactly equal"""
    from distributions_amd import engine
    dim = 16
    assign = (np.arange(n) % k).astype(np.uint32)
    x = ((np.arange(n) // k) % dim).astype(np.uint32)
    osh = [ol.make_shared(ol.DD, alphas=[0.5] * dim)]
    gsh = [engine.dd_shared([0.5] * dim)]
    return osh, gsh, [x], assign


def with_singletons(config, n, k, dim=None, alone=512):
    """the last `alone` groups hold one row each"""
    osh, gsh, vals, _ = workloads.make(config, n, k, dim=dim)
    assign = np.r_[np.arange(n - alone) % (k - alone),
                   np.arange(k - alone, k)].astype(np.uint32)
    return osh, gsh, vals, assign


VS = {"value_sorted": 2}
VS_SCAN = {"value_sorted": 2, "sampling": 1}
ROWS = {"value_sorted": 0}
ROWS_SCAN = {"value_sorted": 0, "sampling": 1}

# name: workload (config, n, k[, dim]) or a builder, options, the debug
# counters expected after the batch, the band.  K = k + 1 (one empty group).
# "dpd" has beta0 = 0 (workloads.make).
CASES = {
    "vs_exact_dd": (("dd", 60000, 1024, 256), VS,
                    {"value_sorted_batches": 1, "scan_batches": 0}, "exact"),
    "vs_exact_k63": (("dd", 40001, 62, 64), VS,
                     {"value_sorted_batches": 1}, "exact"),
    "vs_exact_ties_k64": (lambda: dd_ties(40000, 63), VS,
                          {"value_sorted_batches": 1}, "exact"),
    "narrow_dd": (("dd", 65536, 64, 256), dict(VS, narrow_tiles=2),
                  {"narrow_batches": 1}, "exact"),
    "stream_dpd_beta0_0": (("dpd", 40000, 8191, 1000),
                           dict(VS, value_stream=2), {"stream_batches": 1},
                           "exact"),
    "vs_scan_dd": (("dd", 60000, 1023, 256), VS_SCAN,
                   {"scan_batches": 1}, "vs_scan"),
    "vs_scan_dd_zipf_k65": (("dd_zipf", 50001, 64, 256), VS_SCAN,
                            {"scan_batches": 1}, "vs_scan"),
    "vs_scan_ties_k64": (lambda: dd_ties(40000, 63), VS_SCAN,
                         {"scan_batches": 1}, "vs_scan"),
    "vs_scan_dpd_beta0_0_8192": (("dpd", 60000, 8191, 1000), VS_SCAN,
                                 {"scan_batches": 1}, "vs_scan"),
    "vs_scan_new_groups": (("dd", 60000, 64, 16), VS_SCAN,
                           {"scan_batches": 1}, "vs_scan", 3000.0),
    "vs_scan_singletons": (("dd", 1536, 1024, 256), VS_SCAN,
                           {"scan_batches": 1}, "vs_scan"),
    "vs_exact_low_entropy": (("dd", 40000, 200, 64), VS,
                             {"value_sorted_batches": 1}, "exact", "le"),
    "scratch_exact_fold0": (("gp_nich", 30000, 1024), dict(ROWS, **{
        "debug.rows_fold": 0}), {"scratch_batches": 1, "fold_batches": 0},
        "exact"),
    "scratch_exact_fold2": (("dd_bb_gp", 30000, 1025), dict(ROWS, **{
        "debug.rows_fold": 2}), {"scratch_batches": 1, "fold_batches": 1},
        "exact"),
    "scratch_exact_nich_dominant": (lambda: nich_dominant(30000, 64), ROWS,
                                    {"scratch_batches": 1}, "exact"),
    "scratch_exact_low_entropy": (("gp_nich", 30000, 300), ROWS,
                                  {"scratch_batches": 1}, "exact", "le"),
    "scratch_scan": (("gp_nich", 30000, 1024), ROWS_SCAN,
                     {"scratch_batches": 1}, "rows_scan"),
    "scratch_scan_nich_dominant": (lambda: nich_dominant(30000, 64),
                                   ROWS_SCAN, {"scratch_batches": 1},
                                   "rows_scan"),
    "scratch_scan_new_groups": (("nich", 30000, 64), ROWS_SCAN,
                                {"scratch_batches": 1}, "rows_scan",
                                (3000.0, 0.9)),
    "scratch_scan_singletons": (
        lambda: with_singletons("gp_nich", 30000, 1024), ROWS_SCAN,
        {"scratch_batches": 1}, "rows_scan"),
    # long lists (tests/wide_rows.py): rows_score_lane's loop over up to
    # eight ops, unfolded (wide8: eight ops) and behind a fold of four
    # (mixed5: NormalInverseChiSq alone remains)
    "scratch_scan_wide8": (lambda: wide_rows.make("wide8", 6000, 64),
                           ROWS_SCAN, {"scratch_batches": 1,
                                       "rows_folded_last": 0}, "rows_scan"),
    "scratch_scan_mixed5_fold": (
        lambda: wide_rows.make("mixed5", 6000, 64),
        dict(ROWS_SCAN, **{"debug.rows_fold": 2}),
        {"scratch_batches": 1, "fold_batches": 1, "rows_folded_last": 4,
         "rows_instance_last": 2}, "rows_scan"),
    "program_kernel": (("gp_nich", 20000, 65), dict(ROWS, **{
        "debug.rows_scratch": 0}), {"scratch_batches": 0, "fold_batches": 0,
                                    "value_sorted_batches": 0}, "exact"),
    # BASELINE's C2 and C5 at full batch size, exact and scan: a stratified
    # sample of the rows plus every row alone in its group and every row the
    # kernel sent to the empty slot
    "C2_exact": (("dd", 1_000_000, 1024, 256), {},
                 {"value_sorted_batches": 1, "scan_batches": 0}, "exact"),
    "C2_scan": (("dd", 1_000_000, 1024, 256), {"sampling": 1},
                {"scan_batches": 1}, "vs_scan"),
    "C5_exact": (("dpd", 1_000_000, 8192, 10_000), {},
                 {"value_sorted_batches": 1, "scan_batches": 0}, "exact"),
    "C5_scan": (("dpd", 1_000_000, 8192, 10_000), {"sampling": 1},
                {"scan_batches": 1}, "vs_scan"),
}
SAMPLE = 20000


@pytest.mark.parametrize("name", list(CASES))
def test_every_row_is_the_float64_draw_or_within_the_band(name):
    from distributions_amd import engine
    spec = CASES[name]
    work, opts, expect, kind = spec[:4]
    extra = spec[4] if len(spec) > 4 else None
    alpha, d, le = 1.0, 0.2, None
    if isinstance(extra, tuple):
        alpha, d = extra
    elif isinstance(extra, float):
        alpha = extra
    t_start = time.time()
    if callable(work):
        osh, gsh, vals, assign = work()
    else:
        config, n, k = work[:3]
        osh, gsh, vals, assign = workloads.make(
            config, n, k, dim=work[3] if len(work) > 3 else None)
    n = len(assign)
    k = int(assign.max()) + 1
    if extra == "le":
        # LowEntropy(dataset_size) (clustering.hpp:245-331), scored through
        # the generic driver
        le = n + 1000
        alpha, d = 0.0, 0.0
    gpu = (engine.Gibbs(alpha, d, gsh) if le is None
           else engine.Gibbs(alpha, d, gsh, dataset_size=le))
    for key, value in opts.items():
        gpu.set_option(key, value)
    gpu.load_rows(vals, assign, k, 1)
    # (the oracle's PitmanYor parameters are unused under LowEntropy)
    orc = ol.OracleMixture(alpha if le is None else 1.0, d, osh)
    orc._alpha = alpha
    if le is not None:
        orc.L.orc_mix_set_low_entropy.restype = None
        orc.L.orc_mix_set_low_entropy.argtypes = [ctypes.c_void_p,
                                                  ctypes.c_int]
        orc.L.orc_mix_set_low_entropy(orc.h, le)
    orc.init_from_assignments(vals, assign, k, 1)
    K = len(orc)
    assert len(gpu) == K
    p2g = np.array([gpu.core.packed_to_global(i) for i in range(K)])
    counts = orc.counts()
    g = np.array([orc.L.orc_mix_global_to_packed(orc.h, int(a))
                  for a in orc.assign], np.int64)
    kl = np.where(counts[g] == 1, K - 1, K)
    rows = np.arange(n)
    # the engine's row_scores against the oracle's on a sample (and its cost)
    probe = np.unique(np.r_[np.linspace(0, n - 1, 24).astype(int),
                            np.nonzero(kl != K)[0][:8]])
    t0 = time.time()
    for r in probe:
        got = gpu.row_scores(int(r))
        want = orc.row_scores(int(r), int(g[r]))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), r
    cost = (time.time() - t0) / len(probe)
    gpu.sweep(0, n, n, SEED, draw_base=0)       # ONE batch
    counts_after = gpu.core.debug_counts()
    for key, want in expect.items():
        assert counts_after[key] == want, (key, counts_after)
    new_ids = gpu.assignments().astype(np.int64)
    # back from ids to the slot of each row's score vector
    g2p = {int(p2g[i]): i for i in range(K)}
    new_slot = np.array([g2p.get(int(x), -1) for x in new_ids])
    assert (new_slot >= 0).all(), "an id the pre-batch map does not hold"
    slot = np.where((kl != K) & (new_slot == K - 1), g, new_slot)
    assert np.array_equal(fs.slot_to_global(slot, g, kl, K, p2g), new_ids)
    u = fs.uniforms(SEED, 0, rows)
    empty = np.where(kl != K, g, np.nonzero(counts == 0)[0][0])
    if n > 65536:
        # a stratified sample (one row of every n / SAMPLE), every row alone
        # in its group, every row sent to the empty slot
        strata = np.arange(SAMPLE) * (n // SAMPLE)
        pick = strata + np.random.default_rng(5).integers(0, n // SAMPLE,
                                                          SAMPLE)
        rows = np.unique(np.r_[pick, np.nonzero(kl != K)[0],
                               np.nonzero(slot == empty)[0]])
    tab = (tab_scores(orc, vals[0][rows], g[rows]) if kind == "vs_scan"
           else None)
    rep = fs.Report("%s K=%d" % (name, K))
    chunk = max(64, (1 << 21) // K)
    for i0 in range(0, len(rows), chunk):
        sel = rows[i0:i0 + chunk]
        tsel = tab[i0:i0 + chunk] if tab is not None else None
        sc = np.full((len(sel), K), -np.inf, np.float32)
        for j, r in enumerate(sel):
            s = orc.row_scores(int(r), int(g[r]))
            sc[j, :len(s)] = s
        rr = fs.Rows(sc, kl[sel], u[sel])
        B = fs.band_exact(rr)
        if kind == "rows_scan":
            B = np.maximum(B, fs.band_rows_scan(rr))
        elif kind == "vs_scan":
            single = kl[sel] != K
            Bs = fs.band_vs_scan(rr, np.where(single, 0, g[sel]),
                                 np.where(single, rr.m, tsel))
            B = np.where(single[:, None], B, Bs)
        rep.add(rr, B, slot[sel], sel)
    n_new = int((slot == empty).sum())
    assert rep.n == len(rows)
    print("%s; %d rows to the empty slot, %d alone in their group; "
          "row_scores %.0f us a call; %.1f s" % (
              rep.line(), n_new, int((kl != K).sum()), 1e6 * cost,
              time.time() - t_start))
    assert rep.bad == 0, rep.line()
    if alpha >= 1000:
        assert n_new >= 50, n_new
