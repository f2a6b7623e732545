"""dist_gibbs_sample_rows (k_sample_rows, both instances, and
k_sample_prior_lik): whole rows and missing cells drawn from the mixture.

The group bit for bit against the expectation tests/sample_expect.py composes
from the oracle; every drawn cell against dist_group_sample_value (the host
side of the same inline function, which tests/test_sample_value_host.py holds
to the float64 laws) on the drawn group's statistics; the law of whole rows
on the device against float64 without going through the host entry; launch
geometry; the reader rules."""
import copy
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import f64_scores as fx  # noqa: E402
import feature_expect as fe  # noqa: E402
import oracle_lib as ol  # noqa: E402
import predict_expect as pe  # noqa: E402
import sample_expect as sx  # noqa: E402
from test_gpu_predict import same, snapshot  # noqa: E402

pytestmark = pytest.mark.gpu

NQ = 48
SENTINEL = 0x5EEDF00D
STATES = ["dd", "bb", "gp", "bnb", "nich", "dpd", "dpd_other", "gp_nich",
          "gp_nich_swept", "mixed4", "mixed4_swept", "le_dd", "le_gp_nich",
          "only_empty_k1", "only_empty_k3", "dd256_k1025"]
INEXACT = (ol.GP, ol.BNB, ol.NICH)

_ENGINES = {}


def engine_of(name):
    """one engine per case, shared: sample_rows leaves it as it was"""
    if name not in _ENGINES:
        _ENGINES[name] = fe.case(name).engine()
    return _ENGINES[name]


def seed_state():
    return ol.oracle().orc_rng_seed(pe.DRAW_SEED)


def words_of(c, cols):
    return [ol.value_words(s.kind, v) for s, v in zip(c.osh, cols)]


def check_cells(c, gpu, cols, groups, masks, given, draw_base, what):
    """observed cells unchanged; every other cell the host entry's draw on
    the drawn group's statistics.  -> (cells compared, mismatches) over the
    kinds that may part in a last place; the other kinds must be equal"""
    n = len(groups)
    got = words_of(c, cols)
    st = seed_state()
    cells = wrong = 0
    packed = {int(g): gpu.core.global_to_packed(int(g))
              for g in np.unique(groups)}
    stats = {}
    for f, (osh, gsh) in enumerate(zip(c.osh, gpu.shareds)):
        for q in range(n):
            ob = 0 if masks is None else (int(masks[q]) >> f) & 1
            if ob:
                assert got[f][q] == given[f][q], (what, "observed", q, f)
                continue
            k = packed[int(groups[q])]
            if (f, k) not in stats:
                stats[f, k] = gpu.get_group(f, k)
            want = gsh.group_sample_value(stats[f, k], st, draw_base + q, 1,
                                          f)[0]
            if osh.kind in INEXACT:
                cells += 1
                wrong += int(got[f][q] != want)
            else:
                assert got[f][q] == want, (what, q, f, int(got[f][q]),
                                           int(want))
    return cells, wrong


@pytest.mark.parametrize("name", STATES)
def test_groups_and_cells_under_per_row_masks(name):
    c = fe.case(name)
    gpu = engine_of(name)
    before = snapshot(gpu)
    F = len(c.osh)
    q = [v[:NQ] for v in c.qvals]
    given = words_of(c, q)
    masks = fe.random_masks(NQ, F, 41)
    want = sx.expect_groups(c.orc, q, masks, seed_state(), pe.DRAW_BASE)
    cols, groups = gpu.sample_rows(values=q, observed=masks,
                                   seed=pe.DRAW_SEED, draw_base=pe.DRAW_BASE)
    print("%s: K=%d, groups differ in %d of %d rows" % (
        name, c.K, int((groups != want).sum()), NQ))
    assert np.array_equal(groups, want)
    cells, wrong = check_cells(c, gpu, cols, groups, masks, given,
                               pe.DRAW_BASE, name)
    # every feature observed: predict's draw; the cells are the query's
    full = np.full(NQ, (1 << F) - 1, np.uint32)
    cols_f, groups_f = gpu.sample_rows(values=q, observed=full,
                                       seed=pe.DRAW_SEED,
                                       draw_base=pe.DRAW_BASE)
    _, draw, _ = gpu.predict(q, "sample", seed=pe.DRAW_SEED,
                             draw_base=pe.DRAW_BASE)
    assert np.array_equal(groups_f, draw)
    for f in range(F):
        assert np.array_equal(words_of(c, cols_f)[f], given[f])
    # no mask: the oracle's draw over the driver's scores; the
    # nothing-observed instance and the generic one (a mask of zeros) agree
    want0 = sx.expect_groups(c.orc, None, None, seed_state(), pe.DRAW_BASE,
                             nq=NQ)
    cols_u, groups_u = gpu.sample_rows(n=NQ, seed=pe.DRAW_SEED,
                                       draw_base=pe.DRAW_BASE)
    cols_g, groups_g = gpu.sample_rows(observed=np.zeros(NQ, np.uint32),
                                       seed=pe.DRAW_SEED,
                                       draw_base=pe.DRAW_BASE)
    assert np.array_equal(groups_u, want0)
    assert np.array_equal(groups_g, want0)
    for a, b in zip(words_of(c, cols_u), words_of(c, cols_g)):
        assert np.array_equal(a, b)
    c2, w2 = check_cells(c, gpu, cols_u, groups_u, None, None, pe.DRAW_BASE,
                         name + " unconditional")
    cells, wrong = cells + c2, wrong + w2
    print("%s: %d cells of GP / BNB / NICH compared, %d differ" % (
        name, cells, wrong))
    assert wrong * 100000 <= cells
    assert same(before, snapshot(gpu))
    assert gpu.validate()["code"] == 0


@pytest.mark.parametrize("name", ["gp_nich_swept", "bnb"])
def test_many_cells_of_the_inexact_kinds_match_the_host_entry(name):
    """20 000 unconditional rows: every GP, BNB and NICH cell against the
    host entry (all rows drawn from every group on the host, the drawn
    group's picked), where the device's double log / lgamma and the host's
    may part in a last place: at most 1 cell in 10^5"""
    c = fe.case(name)
    gpu = engine_of(name)
    n, base = 20000, 1 << 32          # (rows beyond 32 bits)
    cols, groups = gpu.sample_rows(n=n, seed=pe.DRAW_SEED, draw_base=base)
    got = words_of(c, cols)
    slots = np.array([gpu.core.global_to_packed(int(g))
                      for g in np.unique(groups)])
    cells = wrong = 0
    for f, gsh in enumerate(gpu.shareds):
        want = np.zeros(n, np.uint32)
        for g, k in zip(np.unique(groups), slots):
            rows = groups == g
            want[rows] = gsh.group_sample_value(
                gpu.get_group(f, int(k)), seed_state(), base, n, f)[rows]
        cells += n
        wrong += int((got[f] != want).sum())
    print("%s: %d cells, %d differ" % (name, cells, wrong))
    assert wrong * 100000 <= cells


# ---------------------------------------------------------------------------
# the law on the device


def test_law_of_whole_rows_on_the_device():
    """2 * 10^5 unconditional rows at mixed4_swept: the group histogram
    against the float64 driver probabilities, each feature's marginal against
    sum_k w_k P_k in float64 (nothing here goes through the host entry)"""
    name, n = "mixed4_swept", 200000
    c = fe.case(name)
    gpu = engine_of(name)
    cols, groups = gpu.sample_rows(n=n, seed=11, draw_base=0)
    # the driver's score_value in float64
    s = copy.copy(c.st)
    s.feats, s.cols, s.stats = [], [], []
    s.slot = np.zeros(1, np.int64)
    v, _, _ = s.scores(np.arange(1), remove=False)
    w = np.exp(v[0] - v[0].max())
    w = w / w.sum()
    K = c.K
    p2g = np.array([c.orc.packed_to_global(k) for k in range(K)])
    g2p = {int(g): k for k, g in enumerate(p2g)}
    slots = np.array([g2p[int(g)] for g in groups])
    p = sx.chi2_p(slots, np.arange(K), w)
    print("groups: chi-square p = %.3g" % p)
    assert p > 1e-4
    for f, osh in enumerate(c.osh):
        feat = fx.Feature(osh)
        col = np.asarray(c.st.cols[f])
        mem = [col[c.st.slot == k] for k in range(K)]
        if osh.kind == ol.NICH:
            mem = [m.view(np.float32) for m in mem]
            laws = [sx.nich_t(feat.kw(), m) for m in mem]
            x = np.asarray(cols[f], np.float32).astype(np.float64)
            p = sx.stats.kstest(
                x, lambda t: sum(wk * lk.cdf(t) for wk, lk in zip(w, laws))
            ).pvalue
            print("feature %d (NICH): KS p = %.3g" % (f, p))
        else:
            values, pm = None, 0.0
            for wk, m in zip(w, mem):
                values, pk = sx.law_pmf(osh.kind, feat.kw(), m)
                pm = pm + wk * pk
            p = sx.chi2_p(cols[f], values, pm)
            print("feature %d: chi-square p = %.3g" % (f, p))
        assert p > 1e-4


# ---------------------------------------------------------------------------
# geometry


def rows_dev(gpu, c, n, values, masks, draw_base, want_group=True,
             in_place=False, pad=8):
    """through the device entry with sentinel-filled, padded outputs
    -> (columns [n + pad] uint32 each, groups or None)"""
    import torch
    F = len(c.osh)
    vals = None
    if values is not None:
        vals = [None if v is None else
                torch.from_numpy(v.view(np.int32).copy()).cuda()
                for v in values]
    mk = (None if masks is None
          else torch.from_numpy(masks.view(np.int32).copy()).cuda())
    if in_place:
        outs = vals
    else:
        outs = [torch.from_numpy(np.full(n + pad, SENTINEL, np.uint32)
                                 .view(np.int32)).cuda() for _ in range(F)]
    grp = torch.from_numpy(np.full(n + pad, SENTINEL, np.uint32)
                           .view(np.int32)).cuda()
    torch.cuda.synchronize()
    gpu.core.sample_rows_dev(
        None if vals is None
        else [0 if v is None else int(v.data_ptr()) for v in vals], n,
        0 if mk is None else int(mk.data_ptr()),
        [int(o.data_ptr()) for o in outs],
        int(grp.data_ptr()) if want_group else 0, seed_state(), draw_base)
    return ([o.cpu().numpy().view(np.uint32) for o in outs],
            grp.cpu().numpy().view(np.uint32))


def test_row_counts_chunks_and_split_calls():
    name = "mixed4_swept"
    c = fe.case(name)
    gpu = engine_of(name)
    F = len(c.osh)
    N = 257
    q = [np.resize(v, N) for v in c.qvals]
    given = words_of(c, q)
    masks = fe.random_masks(N, F, 77)
    base = pe.DRAW_BASE
    ref_c, ref_g = gpu.sample_rows(values=q, observed=masks,
                                   seed=pe.DRAW_SEED, draw_base=base)
    ref_w = words_of(c, ref_c)
    unc_c, unc_g = gpu.sample_rows(n=N, seed=pe.DRAW_SEED, draw_base=base)
    unc_w = words_of(c, unc_c)
    try:
        for chunk in (1 << 22, 100):
            gpu.set_option("debug.predict_chunk", chunk)
            for n in (1, 63, 64, 65, 257):
                cols, grp = rows_dev(gpu, c, n, [g[:n] for g in given],
                                     masks[:n], base)
                assert np.array_equal(grp[:n], ref_g[:n]), (chunk, n)
                assert np.all(grp[n:] == SENTINEL)
                for f in range(F):
                    assert np.array_equal(cols[f][:n], ref_w[f][:n])
                    assert np.all(cols[f][n:] == SENTINEL)
                cols, grp = rows_dev(gpu, c, n, None, None, base)
                assert np.array_equal(grp[:n], unc_g[:n]), (chunk, n)
                assert np.all(grp[n:] == SENTINEL)
                for f in range(F):
                    assert np.array_equal(cols[f][:n], unc_w[f][:n])
                    assert np.all(cols[f][n:] == SENTINEL)
        # one call against two with draw_base advanced
        a_c, a_g = rows_dev(gpu, c, 100, [g[:100] for g in given],
                            masks[:100], base, pad=0)
        b_c, b_g = rows_dev(gpu, c, 157, [g[100:] for g in given],
                            masks[100:], base + 100, pad=0)
        assert np.array_equal(np.r_[a_g, b_g], ref_g)
        for f in range(F):
            assert np.array_equal(np.r_[a_c[f], b_c[f]], ref_w[f])
        # no rows: nothing happens
        cols, grp = rows_dev(gpu, c, 0, None, None, base)
        assert np.all(grp == SENTINEL)
        assert all(np.all(col == SENTINEL) for col in cols)
    finally:
        gpu.set_option("debug.predict_chunk", 1 << 22)


def test_null_group_null_column_in_place_and_unread_cells():
    name = "mixed4_swept"
    c = fe.case(name)
    gpu = engine_of(name)
    F = len(c.osh)
    n = 130
    q = [np.resize(v, n) for v in c.qvals]
    given = words_of(c, q)
    masks = fe.random_masks(n, F, 78)
    masks &= ~np.uint32(1 << 2)          # no row observes feature 2
    base = 5
    ref_c, ref_g = rows_dev(gpu, c, n, given, masks, base, pad=0)
    # group_dev NULL: the same cells, the group buffer untouched
    cols, grp = rows_dev(gpu, c, n, given, masks, base, want_group=False,
                         pad=0)
    assert np.all(grp == SENTINEL)
    for f in range(F):
        assert np.array_equal(cols[f], ref_c[f])
    # a NULL column for the feature no row observes
    holes = list(given)
    holes[2] = None
    cols, grp = rows_dev(gpu, c, n, holes, masks, base, pad=0)
    assert np.array_equal(grp, ref_g)
    for f in range(F):
        assert np.array_equal(cols[f], ref_c[f])
    # unobserved cells filled with 0xFFFFFFFF are never read; completion in
    # place writes only those
    filled = []
    for f in range(F):
        w = given[f].copy()
        w[((masks >> f) & 1) == 0] = 0xFFFFFFFF
        filled.append(w)
    cols, grp = rows_dev(gpu, c, n, filled, masks, base, in_place=True,
                         pad=0)
    assert np.array_equal(grp, ref_g)
    for f in range(F):
        assert np.array_equal(cols[f], ref_c[f])
    # an observed cell of a column that was not given is refused
    masks_bad = masks.copy()
    masks_bad[17] |= 1 << 2
    with pytest.raises(RuntimeError, match="row 17, feature 2"):
        rows_dev(gpu, c, n, holes, masks_bad, base, pad=0)


def test_sample_rows_torch_returns_device_tensors():
    import torch
    name = "mixed4"
    c = fe.case(name)
    gpu = engine_of(name)
    F = len(c.osh)
    q = [v[:NQ] for v in c.qvals]
    given = words_of(c, q)
    masks = fe.random_masks(NQ, F, 33)
    host_c, host_g = gpu.sample_rows(values=q, observed=masks, seed=3,
                                     draw_base=9)
    vals = [torch.from_numpy(w.view(np.int32).copy()).cuda() for w in given]
    mk = torch.from_numpy(masks.view(np.int32).copy()).cuda()
    dev_c, dev_g = gpu.sample_rows_torch(values=vals, observed=mk, seed=3,
                                         draw_base=9)
    assert dev_g.is_cuda and all(t.is_cuda for t in dev_c)
    assert dev_c[2].dtype == torch.float32
    assert np.array_equal(dev_g.cpu().numpy().view(np.uint32), host_g)
    for f in range(F):
        assert np.array_equal(dev_c[f].cpu().numpy().view(np.uint32),
                              words_of(c, host_c)[f])
    host_c, host_g = gpu.sample_rows(n=NQ, seed=3, draw_base=9)
    dev_c, dev_g = gpu.sample_rows_torch(n=NQ, seed=3, draw_base=9)
    assert np.array_equal(dev_g.cpu().numpy().view(np.uint32), host_g)
    for f in range(F):
        assert np.array_equal(dev_c[f].cpu().numpy().view(np.uint32),
                              words_of(c, host_c)[f])
    with pytest.raises(RuntimeError, match="observed mask"):
        gpu.sample_rows(values=q)


# ---------------------------------------------------------------------------
# rules


def test_refused_with_a_batch_open():
    c = fe.case("dd_bb_gp")
    gpu = c.engine()          # (its own engine: the state moves)
    st = ol.oracle().orc_rng_seed(3)
    gpu.core.batch_sample(0, 1024, st, 0)
    with pytest.raises(RuntimeError, match="batch open"):
        gpu.sample_rows(n=4)
    gpu.core.batch_apply_local()
    gpu.core.batch_finish()
    gpu.sample_rows(n=4)


def test_observed_values_out_of_their_domain():
    name = "dd_bb_gp"
    c = fe.case(name)
    gpu = engine_of(name)
    before = snapshot(gpu)
    n = 200
    q = [np.resize(v, n).copy() for v in c.qvals]
    full = np.full(n, 0b111, np.uint32)
    good = gpu.sample_rows(values=q, observed=full, seed=1)
    gpu.set_option("debug.predict_chunk", 64)
    try:
        bad = [v.copy() for v in q]
        bad[1][150] = 2
        bad[1][130] = 2                  # the first offending row is named
        bad[0][170] = 200                # (a later row, an earlier feature)
        with pytest.raises(RuntimeError, match="row 130, feature 1"):
            gpu.sample_rows(values=bad, observed=full, seed=1)
        # the same words in cells that are not observed are never read
        masks = full.copy()
        masks[[130, 150]] = 0b101
        masks[170] = 0b110
        a = gpu.sample_rows(values=bad, observed=masks, seed=1)
        b = gpu.sample_rows(values=q, observed=masks, seed=1)
        assert np.array_equal(a[1], b[1])
        for x, y in zip(a[0], b[0]):
            assert np.array_equal(x, y)
        # process and engine go on
        again = gpu.sample_rows(values=q, observed=full, seed=1)
        assert np.array_equal(again[1], good[1])
    finally:
        gpu.set_option("debug.predict_chunk", 1 << 22)
    assert same(before, snapshot(gpu))
