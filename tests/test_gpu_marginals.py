"""dist_gibbs_marginals[_many] (k_marginals_many, k_ensemble_fold): the log
marginals of S feature subsets per held-out row, on one engine and averaged
over M engines, bit for bit against the expectation tests/marginals_expect.py
composes from the oracle (and tests/test_marginals_oracle.py holds to float64).

Every subset of the mixed lists dd_bb_gp and gp_nich at M = 3, LowEntropy at
M = 1, 2, 5, a member of only empty groups, DPD with a member whose OTHER has
no mass, K = 4 beside K = 1025, M = 66, the eight-feature list; then the
launch geometry (S around a wave and beyond a workgroup, n = 1 and 257,
several chunks, each output alone, sentinels), the identities with
Gibbs.predict_feature (both forms), predict, predict_many and
predict_feature_many, permutations, the torch form, and the refusals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ensemble_expect as ee  # noqa: E402
import marginals_expect as mx  # noqa: E402
import predict_expect as pe  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5

# (tests/test_gpu_predict_feature_many.py's ensembles, rebuilt here)
LE5 = [dict(k=k, empty=1, alpha=1.0, d=0.0, sweeps=0)
       for k in (4, 17, 41, 8, 25)]
# K = 4 beside K = 1025: a member below one LDS tile beside one that crosses
# tiles
K4_K1025 = [dict(k=3, empty=1, alpha=1.0, d=0.0, sweeps=0, n=200),
            dict(k=1024, empty=1, alpha=4.0, d=0.2, sweeps=0, n=4096)]
# 66 members of 64-row tables: one more than a block of
# k_predict_prior_totals' lanes plus one
SMALL66 = [dict(k=3 + e % 3, empty=1 + e % 2, alpha=1.0 + e % 4,
                d=0.25 * (e % 3), sweeps=0, n=64) for e in range(66)]

ENSEMBLES = {
    "dd_bb_gp": lambda: ee.Ensemble("dd_bb_gp", ee.SPECS3),
    "gp_nich": lambda: ee.Ensemble("gp_nich", ee.SPECS3),
    "le_m1": lambda: ee.Ensemble("dd_bb_gp", LE5[:1], le=2000),
    "le_m2": lambda: ee.Ensemble("dd_bb_gp", LE5[:2], le=2000),
    "le_m5": lambda: ee.Ensemble("dd_bb_gp", LE5, le=2000),
    "only_empty_member": lambda: ee.Ensemble(
        "dd_bb_gp", [ee.SPECS3[0],
                     dict(k=0, empty=1, alpha=1.0, d=0.5, sweeps=0, n=64),
                     ee.SPECS3[2]]),
    # member 1's OTHER has no mass: fast_log(alpha * 0) in its planes
    "dpd_other_mixed": lambda: ee.Ensemble(
        "dpd_other", ee.SPECS3, beta0=[0.1, 0.0, 0.1], other=(1, 2)),
    "dd70_k4_k1025": lambda: ee.Ensemble("dd_bb_gp", K4_K1025, nq=96,
                                         dim=70),
    "small66": lambda: ee.Ensemble("dd_bb_gp", SMALL66, nq=257),
    "eight": lambda: mx.Ensemble8(),
}
_ENS = {}
_GPUS = {}
_EXPECT = {}


def ensemble(name):
    if name not in _ENS:
        _ENS[name] = ENSEMBLES[name]()
    return _ENS[name]


def engines_of(name):
    """one set of engines per ensemble, shared: the readers leave them as
    they were"""
    if name not in _GPUS:
        _GPUS[name] = ensemble(name).engines()
    return _GPUS[name]


def masks_of(name):
    """every subset of the feature list, 0 included; the eight-feature list:
    its 8 + 28 singles and pairs, the full mask and 0"""
    if name == "eight":
        return mx.eight_masks()
    return mx.all_masks(len(ensemble(name).members[0].osh))


def expect_of(name):
    """the expectation under masks_of(name), computed once"""
    if name not in _EXPECT:
        ens = ensemble(name)
        _EXPECT[name] = mx.expect_many([m.orc for m in ens.members],
                                       ens.qvals, masks_of(name),
                                       ens.le is not None)
    return _EXPECT[name]


def same_bits(got, want):
    """float32 arrays equal bit for bit, NaNs as patterns that are both NaN"""
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return (got.shape == want.shape and np.array_equal(np.isnan(got), nan)
            and np.array_equal(got.view(np.uint32)[~nan],
                               want.view(np.uint32)[~nan]))


def word(x):
    return int(np.float32(x).view(np.uint32))


def unchanged(gpus, before):
    for g, (c, a) in zip(gpus, before):
        assert np.array_equal(g.counts(), c)
        assert np.array_equal(g.assignments(), a)
        g.validate()       # (raises on the first inconsistency)


def snapshot(gpus):
    return [(g.counts().copy(), g.assignments().copy()) for g in gpus]


@pytest.mark.parametrize("name", list(ENSEMBLES))
def test_marginals_many_is_the_oracles_bit_for_bit(name):
    from distributions_amd import engine
    ens, gpus, masks = ensemble(name), engines_of(name), masks_of(name)
    e = expect_of(name)
    before = snapshot(gpus)
    logp, planes, totals = engine.marginals_many(gpus, ens.qvals, masks,
                                                 members=True)
    logp_n, no_planes, totals_n = engine.marginals_many(gpus, ens.qvals,
                                                        masks)
    print("%s: M=%d, K=%s, %d rows x %d masks: logp bits differ in %d cells, "
          "planes in %d" % (
              name, ens.M, [m.K for m in ens.members][:8], ens.nq, len(masks),
              int((logp.view(np.uint32) != e["logp"].view(np.uint32)).sum()),
              int((planes.view(np.uint32) != e["w"].view(np.uint32)).sum())))
    assert same_bits(planes, e["w"])
    assert same_bits(logp, e["logp"]) and same_bits(logp_n, e["logp"])
    assert no_planes is None
    assert [word(t) for t in totals] == [word(t) for t in e["prior_totals"]]
    assert [word(t) for t in totals_n] == [word(t) for t in totals]
    # the single-engine entry is each member's plane (of 66 members: the
    # first three, one in the middle and the last)
    for i in (range(ens.M) if ens.M <= 5 else (0, 1, 2, 33, ens.M - 1)):
        assert same_bits(gpus[i].marginals(ens.qvals, masks), planes[i]), i
    unchanged(gpus, before)


# ---------------------------------------------------------------------------
# geometry


def marginals_dev(gpus, words, n, masks, want="lp", ld=None, pad=64,
                  single=False):
    """marginals_many_dev on the first n query rows into sentinel-filled
    device buffers -> dict of host copies, padding included (l: logp,
    p: the planes with leading dimension ld, t: the totals)"""
    import torch
    from distributions_amd import _core
    M, S = len(gpus), len(masks)
    ld = n * S if ld is None else ld
    cols = [None if w is None else
            torch.from_numpy(np.ascontiguousarray(w[:n]).view(np.int32)
                             .copy()).cuda() for w in words]
    logp = torch.full((n * S + pad,), SENTINEL, dtype=torch.float32,
                      device="cuda")
    planes = torch.full((M * ld + pad,), SENTINEL, dtype=torch.float32,
                        device="cuda")
    torch.cuda.synchronize()
    totals = _core.marginals_many_dev(
        [g.core for g in gpus],
        [0 if c is None else int(c.data_ptr()) for c in cols], n, masks,
        int(logp.data_ptr()) if "l" in want else 0,
        int(planes.data_ptr()) if "p" in want else 0, ld, "t" in want,
        single)
    return dict(l=logp.cpu().numpy(), p=planes.cpu().numpy(), t=totals)


def check_dev(out, want_w, want_logp, n, M, S, want, ld=None):
    """what was asked for is the expectation's first n rows, everything else
    still holds the sentinel"""
    ld = n * S if ld is None else ld
    sent = word(SENTINEL)
    lw, pw = out["l"].view(np.uint32), out["p"].view(np.uint32)
    if "l" in want:
        assert same_bits(out["l"][:n * S].reshape(n, S), want_logp[:n])
        assert np.all(lw[n * S:] == sent)
    else:
        assert np.all(lw == sent)
    if "p" in want:
        for i in range(M):
            assert same_bits(out["p"][i * ld:i * ld + n * S].reshape(n, S),
                             want_w[i, :n]), i
            assert np.all(pw[i * ld + n * S:(i + 1) * ld] == sent)
        assert np.all(pw[M * ld:] == sent)
    else:
        assert np.all(pw == sent)


@pytest.mark.parametrize("S", [1, 7, 8, 63, 64, 65, 300])
def test_mask_counts_around_a_wave_and_beyond_a_workgroup(S):
    """masks repeated: a row's items around a wave (63, 64, 65) and over two
    workgroups (300); n = 1 and n = 257"""
    ens, gpus = ensemble("dd_bb_gp"), engines_of("dd_bb_gp")
    e = expect_of("dd_bb_gp")
    # (from mask 5 on: S = 1 names two features, S = 7 leaves one subset out)
    idx = (np.arange(S) + 5) % 8
    masks = masks_of("dd_bb_gp")[idx]
    words = pe.query_words(ens.members[0].orc, ens.qvals)
    for n in (1, 257):
        out = marginals_dev(gpus, words, n, masks, ld=n * S + 3)
        check_dev(out, e["w"][:, :, idx], e["logp"][:, idx], n, ens.M, S,
                  "lp", n * S + 3)


@pytest.mark.parametrize("name", ["dd_bb_gp", "gp_nich", "le_m2",
                                  "dpd_other_mixed", "dd70_k4_k1025",
                                  "eight"])
def test_one_mask_alone_is_its_column(name):
    """S = 1: a row has one chain and the plain form runs (a lane per row,
    k_predict's instances by the feature list; the full mask takes its loop
    without the per-feature test) -- every mask on its own gives its column
    of the staged call"""
    from distributions_amd import engine
    ens, gpus, masks = ensemble(name), engines_of(name), masks_of(name)
    e = expect_of(name)
    for s, mask in enumerate(masks):
        logp, planes, _ = engine.marginals_many(gpus, ens.qvals, [mask],
                                                members=True)
        assert same_bits(planes[:, :, 0], e["w"][:, :, s]), s
        assert same_bits(logp[:, 0], e["logp"][:, s]), s
    one = gpus[0].marginals(ens.qvals, masks[:1])
    assert same_bits(one[:, 0], e["w"][0, :, 0])


def test_chunks_each_output_alone_and_the_scratch_path():
    ens, gpus = ensemble("small66"), engines_of("small66")
    e, masks = expect_of("small66"), masks_of("small66")
    M, S = ens.M, len(masks)
    words = pe.query_words(ens.members[0].orc, ens.qvals)
    try:
        for chunk in (1 << 22, 37):
            gpus[0].set_option("debug.predict_chunk", chunk)
            for n in (1, 64, 257):
                out = marginals_dev(gpus, words, n, masks)
                check_dev(out, e["w"], e["logp"], n, M, S, "lp")
        gpus[0].set_option("debug.predict_chunk", 37)
        # (l alone: the planes stay in engine scratch)
        for want in ("l", "p", "t", "lt", ""):
            out = marginals_dev(gpus, words, 257, masks, want)
            check_dev(out, e["w"], e["logp"], 257, M, S, want)
            if "t" in want:
                assert [word(x) for x in out["t"]] == [
                    word(x) for x in e["prior_totals"]]
            else:
                assert out["t"] is None
        # no rows: nothing is written
        out = marginals_dev(gpus, words, 0, masks)
        check_dev(out, e["w"], e["logp"], 0, M, S, "")
        # the single-engine entry, chunked
        gpus[5].set_option("debug.predict_chunk", 37)
        one = marginals_dev(gpus[5:6], words, 257, masks, "l", single=True)
        check_dev(one, None, e["w"][5], 257, 1, S, "l")
    finally:
        gpus[0].set_option("debug.predict_chunk", 1 << 22)
        gpus[5].set_option("debug.predict_chunk", 1 << 22)


def test_a_null_column_under_no_mask_is_never_read():
    """masks that name features 0 and 2 only: feature 1's column is None"""
    from distributions_amd import engine
    ens, gpus = ensemble("dd_bb_gp"), engines_of("dd_bb_gp")
    e = expect_of("dd_bb_gp")
    idx = np.array([5, 1, 0, 4])
    q = [ens.qvals[0], None, ens.qvals[2]]
    logp, planes, _ = engine.marginals_many(gpus, q, masks_of("dd_bb_gp")[idx],
                                            members=True)
    assert same_bits(logp, e["logp"][:, idx])
    assert same_bits(planes, e["w"][:, :, idx])


# ---------------------------------------------------------------------------
# identities


@pytest.mark.parametrize("name", ["dd_bb_gp", "gp_nich", "le_m5",
                                  "dpd_other_mixed"])
def test_every_mask_is_predict_features_base_predict_and_prior_total(name):
    """w[e][.][s] is Gibbs.predict_feature's base under the row mask masks[s]
    for a target outside it (staged and recompute), Gibbs.predict's logp for
    the full mask and its prior_total for mask 0"""
    from distributions_amd import engine
    ens, gpus, masks = ensemble(name), engines_of(name), masks_of(name)
    q = ens.qvals
    F = len(ens.members[0].osh)
    le = ens.le is not None
    _, planes, totals = engine.marginals_many(gpus, q, masks, members=True)

    def member_value(x, i):
        if not le:
            return x
        with np.errstate(invalid="ignore"):
            return (x - totals[i]).astype(np.float32)

    for s, mask in enumerate(masks):
        mask = int(mask)
        free = [t for t in range(F) if not (mask >> t) & 1]
        for i, g in enumerate(gpus):
            if free:
                for staged in (True, False):
                    _, b, _ = g.predict_feature(
                        q, free[0], np.zeros(1, q[free[0]].dtype),
                        np.full(ens.nq, mask, np.uint32), None, staged=staged)
                    assert same_bits(planes[i, :, s], member_value(b, i)), \
                        (s, i, staged)
            else:
                lp, _, total = g.predict(q, None)
                assert same_bits(planes[i, :, s], member_value(lp, i)), (s, i)
                assert word(total) == word(totals[i])
            if mask == 0:
                want = np.float32(0.0) if le else totals[i]
                assert np.all(planes[i, :, s].view(np.uint32) == word(want))


@pytest.mark.parametrize("name", ["dd_bb_gp", "le_m2", "small66"])
def test_the_folded_planes_are_predict_feature_manys_base_and_predict_many(
        name):
    from distributions_amd import engine
    ens, gpus, masks = ensemble(name), engines_of(name), masks_of(name)
    q = ens.qvals
    F = len(ens.members[0].osh)
    logp, _, _ = engine.marginals_many(gpus, q, masks)
    for s, mask in enumerate(masks):
        mask = int(mask)
        free = [t for t in range(F) if not (mask >> t) & 1]
        if free:
            base = engine.predict_feature_many(
                gpus, q, free[0], np.zeros(1, q[free[0]].dtype),
                np.full(ens.nq, mask, np.uint32), None)[1]
        else:
            base = engine.predict_many(gpus, q, None)[0]
        assert same_bits(logp[:, s], base), s


def test_permuting_rows_and_masks_permutes_the_results():
    from distributions_amd import engine
    ens, gpus = ensemble("gp_nich"), engines_of("gp_nich")
    masks = masks_of("gp_nich")
    logp, planes, _ = engine.marginals_many(gpus, ens.qvals, masks,
                                            members=True)
    rng = np.random.default_rng(5)
    pr, pm = rng.permutation(ens.nq), rng.permutation(len(masks))
    logp_p, planes_p, _ = engine.marginals_many(
        gpus, [c[pr] for c in ens.qvals], masks[pm], members=True)
    assert same_bits(logp_p, logp[pr][:, pm])
    assert same_bits(planes_p, planes[:, pr][:, :, pm])


@pytest.mark.parametrize("name", ["dd_bb_gp", "le_m2"])
def test_the_torch_form_is_the_host_form(name):
    import torch
    from distributions_amd import engine
    ens, gpus, masks = ensemble(name), engines_of(name), masks_of(name)
    e = expect_of(name)
    words = pe.query_words(ens.members[0].orc, ens.qvals)
    cols = [torch.from_numpy(w.view(np.int32).copy()).cuda() for w in words]
    logp, planes, totals = engine.marginals_many_torch(gpus, cols, masks,
                                                       members=True)
    assert logp.is_cuda and planes.is_cuda
    assert same_bits(logp.cpu().numpy(), e["logp"])
    assert same_bits(planes.cpu().numpy(), e["w"])
    assert [word(t) for t in totals] == [word(t) for t in e["prior_totals"]]
    logp_n, none, _ = engine.marginals_many_torch(gpus, cols, masks)
    assert none is None and same_bits(logp_n.cpu().numpy(), e["logp"])
    one = gpus[1].marginals_torch(cols, masks)
    assert same_bits(one.cpu().numpy(), e["w"][1])
    # a column of another length is refused before anything reads it
    with pytest.raises(RuntimeError, match="differ in length"):
        engine.marginals_many_torch(gpus, [cols[0], cols[1][:-1], cols[2]],
                                    masks)


# ---------------------------------------------------------------------------
# refusals


def test_refusals_launch_nothing_and_leave_the_engines_alone():
    from distributions_amd import engine
    ens, gpus = ensemble("dd_bb_gp"), engines_of("dd_bb_gp")
    e, masks = expect_of("dd_bb_gp"), masks_of("dd_bb_gp")
    q = ens.qvals
    before = snapshot(gpus)
    with pytest.raises(RuntimeError, match="mask 2 names a feature"):
        engine.marginals_many(gpus, q, [1, 7, 8, 16])
    with pytest.raises(RuntimeError, match="mask 1 names feature 1, whose"):
        engine.marginals_many(gpus, [q[0], None, q[2]], [1, 3, 2])
    with pytest.raises(RuntimeError, match="no mask"):
        engine.marginals_many(gpus, q, [])
    with pytest.raises(RuntimeError, match="no mask"):
        gpus[0].marginals(q, [])
    with pytest.raises(RuntimeError, match="one feature list"):
        engine.marginals_many([gpus[0], engines_of("gp_nich")[0]], q, [1])
    # a DD word >= dim under a named feature names the first such row
    bad = [c.copy() for c in q]
    bad[0][211] = 8
    bad[0][130] = 200
    with pytest.raises(RuntimeError, match="row 130, feature 0"):
        engine.marginals_many(gpus, bad, masks)
    with pytest.raises(RuntimeError, match="row 130, feature 0"):
        gpus[1].marginals(bad, [1])
    # ... and is accepted when no mask names that feature
    idx = np.array([2, 4, 6, 0])
    logp, _, _ = engine.marginals_many(gpus, bad, masks[idx])
    assert same_bits(logp, e["logp"][:, idx])
    # process and engines go on
    logp, _, _ = engine.marginals_many(gpus, q, masks)
    assert same_bits(logp, e["logp"])
    unchanged(gpus, before)
