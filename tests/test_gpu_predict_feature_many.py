"""dist_gibbs_predict_feature_many (k_predict_feature_many, k_ensemble_fold,
k_predict_feature_choice on the folded plane): one feature's predictive given
the others averaged over M engines, bit for bit against the expectation
tests/feature_many_expect.py composes from the oracle (and
tests/test_feature_many_oracle.py holds to float64).

Every feature of the mixed lists dd_bb_gp and gp_nich as the target under
random masks at M = 3, LowEntropy at M = 1, 2, 5, a member of only empty
groups, DPD with a member whose OTHER has no mass; then the identities with
Gibbs.predict_feature (both forms) and predict_many, launch geometry (C + 1
around a wave, K = 4 beside K = 1025, M = 66, several chunks, each output
alone, sentinels), permutations, the torch form, the chains of
sweep_sequential_many, and the refusals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import eight_expect as xe  # noqa: E402
import ensemble_expect as ee  # noqa: E402
import feature_expect as fe  # noqa: E402
import feature_many_expect as fm  # noqa: E402
import oracle_lib as ol  # noqa: E402
import predict_expect as pe  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
WORD_SENTINEL = -7
MASK_SEED = 11

LE5 = [dict(k=k, empty=1, alpha=1.0, d=0.0, sweeps=0)
       for k in (4, 17, 41, 8, 25)]
# K = 4 beside K = 1025: with DD(70) first on dd_bb_gp the LDS tile is between
# 127 (C = 1) and 818 (C = 64) groups, which the second member crosses and the
# first does not
K4_K1025 = [dict(k=3, empty=1, alpha=1.0, d=0.0, sweeps=0, n=200),
            dict(k=1024, empty=1, alpha=4.0, d=0.2, sweeps=0, n=4096)]
# 66 members of 64-row tables: one more than a block of
# k_predict_prior_totals' lanes plus one
SMALL66 = [dict(k=3 + e % 3, empty=1 + e % 2, alpha=1.0 + e % 4,
                d=0.25 * (e % 3), sweeps=0, n=64) for e in range(66)]
DPD_CAND = [0, 3, 49, fe.OTHER, 77]      # 77: not in the table, OTHER

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
    # eight features, K = 8, 34 and 43 (tests/eight_expect.py); with fewer
    # query rows where the target has many candidates (the float64 law is
    # computed per row, mask and candidate)
    "eight3": lambda: xe.eight3(),
    "eight3_30": lambda: xe.eight3_head(30),
    "eight3_12": lambda: xe.eight3_head(12),
}
# name: ensemble, target, candidates (None: the kind's list or the domain)
CASES = {
    "mixed_dd": ("dd_bb_gp", 0, None),
    "mixed_bb": ("dd_bb_gp", 1, None),
    "mixed_gp": ("dd_bb_gp", 2, fe.COUNT_CANDIDATES),
    "gp_nich_gp": ("gp_nich", 0, fe.COUNT_CANDIDATES),
    "gp_nich_nich": ("gp_nich", 1, fe.REAL_CANDIDATES),
    "le_m1": ("le_m1", 1, None),
    "le_m2": ("le_m2", 0, None),
    "le_m5": ("le_m5", 2, fe.COUNT_CANDIDATES),
    "only_empty_member": ("only_empty_member", 1, None),
    "dpd_other_mixed": ("dpd_other_mixed", 0, DPD_CAND),
    "small66": ("small66", 1, None),
    # ten planes after the target; NICH with DD, BNB, DPD, DD after it;
    # DD(70); DPD with OTHER among the default candidates; the tight loop
    "eight3_t0": ("eight3", 0, None),
    "eight3_t3": ("eight3", 3, fe.REAL_CANDIDATES),
    "eight3_t4": ("eight3_12", 4, None),
    "eight3_t6": ("eight3_30", 6, None),
    "eight3_t7": ("eight3", 7, None),
}
_ENS = {}
_GPUS = {}
_FENS = {}


def ensemble(name):
    if name not in _ENS:
        _ENS[name] = ENSEMBLES[name]()
    return _ENS[name]


def engines_of(name):
    """one set of engines per ensemble, shared: the readers leave them as
    they were"""
    if name.startswith("eight3"):
        name = "eight3"     # (its shorter forms share the members)
    if name not in _GPUS:
        _GPUS[name] = ensemble(name).engines()
    return _GPUS[name]


def as_candidates(shared, cand):
    if cand is None:
        return None
    return np.array(cand, np.float32 if shared.kind == ol.NICH else np.uint32)


def masks_of(n, F, seed):
    """random per-row masks; past four features also the fixed ones (only
    features >= 4, only features < 4, alternating)"""
    return xe.masks_for(n, F, seed) if F > 4 else fe.random_masks(n, F, seed)


def case(name):
    """-> (FeatureEnsemble under random masks, its engines)"""
    ens_name, target, cand = CASES[name]
    if name not in _FENS:
        ens = ensemble(ens_name)
        osh = ens.members[0].osh
        _FENS[name] = fm.FeatureEnsemble(
            ens, target, as_candidates(osh[target], cand),
            masks_of(ens.nq, len(osh), MASK_SEED))
    return _FENS[name], engines_of(ens_name)


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


def many(gpus, fens, mode, qvals=None, observed="own", cand="own", **kw):
    from distributions_amd import engine
    return engine.predict_feature_many(
        gpus, fens.ens.qvals if qvals is None else qvals, fens.target,
        fens.cand if isinstance(cand, str) else cand,
        fens.observed if isinstance(observed, str) else observed, mode,
        seed=fm.DRAW_SEED, draw_base=kw.pop("draw_base", fm.DRAW_BASE), **kw)


@pytest.mark.parametrize("name", [n for n in CASES if n != "small66"])
def test_predict_feature_many_is_the_oracles_bit_for_bit(name):
    fens, gpus = case(name)
    e = fens.expect()
    joint, base, choice, member, pj, pb, totals = many(gpus, fens, "sample",
                                                       members=True)
    joint_m, base_m, choice_m, member_m, pj_m, pb_m, totals_m = many(
        gpus, fens, "map", members=True)
    joint_n, base_n, no_c, no_m, no_pj, no_pb, _ = many(gpus, fens, None)
    print("%s: M=%d, K=%s, %d rows x %d candidates: joint bits differ in %d "
          "cells, base in %d rows, planes in %d + %d cells, choices in %d / "
          "%d, members in %d / %d" % (
              name, fens.M, [m.K for m in fens.ens.members], fens.nq, fens.C,
              int((joint.view(np.uint32) != e["joint"].view(np.uint32)).sum()),
              int((base.view(np.uint32) != e["base"].view(np.uint32)).sum()),
              int((pj.view(np.uint32) != e["wj"].view(np.uint32)).sum()),
              int((pb.view(np.uint32) != e["wb"].view(np.uint32)).sum()),
              int((choice != e["choice_draw"]).sum()),
              int((choice_m != e["choice_map"]).sum()),
              int((member != e["member_draw"]).sum()),
              int((member_m != e["member_map"]).sum())))
    assert same_bits(pj, e["wj"]) and same_bits(pj_m, e["wj"])
    assert same_bits(pb, e["wb"]) and same_bits(pb_m, e["wb"])
    assert [word(t) for t in totals] == [word(t) for t in e["prior_totals"]]
    assert [word(t) for t in totals_m] == [word(t) for t in totals]
    for got in (joint, joint_m, joint_n):
        assert same_bits(got, e["joint"])
    for got in (base, base_m, base_n):
        assert same_bits(got, e["base"])
    assert no_c is None and no_m is None and no_pj is None and no_pb is None
    assert np.array_equal(choice, e["choice_draw"])
    assert np.array_equal(choice_m, e["choice_map"])
    assert np.array_equal(member, e["member_draw"])
    assert np.array_equal(member_m, e["member_map"])
    if name != "dpd_other_mixed":   # (the band takes no fast_log(0))
        law = fens.f64()
        print("%s: worst excursion / band: joint %.3f, base %.3f" % (
            name, (np.abs(joint - law["joint"]) / law["joint_band"]).max(),
            (np.abs(base - law["base"]) / law["base_band"]).max()))
        assert (np.abs(joint - law["joint"]) / law["joint_band"]).max() <= 1
        assert (np.abs(base - law["base"]) / law["base_band"]).max() <= 1


# ---------------------------------------------------------------------------
# identities


@pytest.mark.parametrize("name", ["mixed_dd", "gp_nich_nich", "le_m5",
                                  "dpd_other_mixed", "eight3_t0", "eight3_t3",
                                  "eight3_t6"])
def test_the_planes_are_the_members_own_predict_feature(name):
    """M separate Gibbs.predict_feature calls, the staged and the plain form
    as witnesses; and M = 1 is predict_feature itself"""
    fens, gpus = case(name)
    q = fens.ens.qvals
    _, _, _, _, pj, pb, totals = many(gpus, fens, "map", members=True)
    for staged in (True, False):
        for i, g in enumerate(gpus):
            j, b, c = g.predict_feature(q, fens.target, fens.cand,
                                        fens.observed, "sample",
                                        seed=fm.DRAW_SEED,
                                        draw_base=fm.DRAW_BASE, staged=staged)
            if fens.le:
                with np.errstate(invalid="ignore"):
                    j = (j - totals[i]).astype(np.float32)
                    b = (b - totals[i]).astype(np.float32)
            assert same_bits(pj[i], j), (i, staged)
            assert same_bits(pb[i], b), (i, staged)
            if staged:
                continue
            one = many(gpus[i:i + 1], fens, "sample")
            assert same_bits(one[0], j) and same_bits(one[1], b)
            assert np.all(one[3] == 0)
            if not fens.le:     # (under LowEntropy the choice is drawn from
                assert np.array_equal(one[2], c)    # the shifted values)


@pytest.mark.parametrize("name", ["mixed_bb", "gp_nich_gp", "le_m5",
                                  "eight3_t3"])
def test_everything_else_observed_is_predict_many_on_completed_rows(name):
    from distributions_amd import engine
    fens, gpus = case(name)
    q = fens.ens.qvals
    _, _, _, _, pj, _, _ = many(gpus, fens, None, observed=None,
                                members=True)
    for c, v in enumerate(fens.values):
        done = fe.completed(q, fens.target, v, fens.shared.kind)
        planes = engine.predict_many(gpus, done, None, members=True)[3]
        assert same_bits(pj[:, :, c], planes), c


@pytest.mark.parametrize("name", ["mixed_gp", "le_m5", "eight3_t0"])
def test_nothing_observed_gives_the_prior_totals(name):
    fens, gpus = case(name)
    nothing = np.zeros(fens.nq, np.uint32)
    _, base, _, _, _, pb, totals = many(gpus, fens, None, observed=nothing,
                                        members=True)
    for i in range(fens.M):
        want = np.float32(0.0) if fens.le else totals[i]
        assert np.all(pb[i].view(np.uint32) == word(want)), i
    assert same_bits(base, ee.fold(pb, 1, 0)[0])


# ---------------------------------------------------------------------------
# geometry


def many_dev(gpus, words, n, observed, target, cand, mode, want="jbcmJB",
             ldj=None, ldb=None, flags=0, pad=64, draw_base=fm.DRAW_BASE,
             C=None):
    """predict_feature_many_dev on the first n query rows into sentinel-filled
    device buffers -> dict of host copies, padding included (j: joint,
    b: base, c: choice, m: member, J / B: the planes with leading dimensions
    ldj / ldb, t: the totals)"""
    import torch
    from distributions_amd import _core
    M = len(gpus)
    C = len(cand) if C is None else C
    ldj = n * C if ldj is None else ldj
    ldb = n if ldb is None else ldb
    cols = [torch.from_numpy(np.ascontiguousarray(w[:n]).view(np.int32)
                             .copy()).cuda() for w in words]
    mask = None if observed is None else torch.from_numpy(
        np.ascontiguousarray(observed[:n]).view(np.int32).copy()).cuda()

    def floats(k):
        return torch.full((k + pad,), SENTINEL, dtype=torch.float32,
                          device="cuda")

    def ints(k):
        return torch.full((k + pad,), WORD_SENTINEL, dtype=torch.int32,
                          device="cuda")

    buf = dict(j=floats(n * C), b=floats(n), c=ints(n), m=ints(n),
               J=floats(max(M, 1) * ldj), B=floats(max(M, 1) * ldb))
    torch.cuda.synchronize()
    L = ol.oracle()
    ptr = {k: int(v.data_ptr()) if k in want else 0 for k, v in buf.items()}
    totals = _core.predict_feature_many_dev(
        [None if g is None else g.core for g in gpus],
        [int(t.data_ptr()) for t in cols], n,
        0 if mask is None else int(mask.data_ptr()), target, cand,
        ptr["j"], ptr["b"], ptr["c"], ptr["m"], mode,
        L.orc_rng_seed(fm.DRAW_SEED), L.orc_rng_seed(fm.MEMBER_SEED),
        draw_base, ptr["J"], ldj, ptr["B"], ldb, "t" in want, flags)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in buf.items()}
    out["t"] = totals
    return out


def check_dev(out, e, n, M, C, mode, want, ldj=None, ldb=None):
    """every asked output right on its first n rows, everything else
    untouched"""
    ldj = n * C if ldj is None else ldj
    ldb = n if ldb is None else ldb
    c_key, m_key = (("choice_draw", "member_draw") if mode == 0
                    else ("choice_map", "member_map"))
    for key, name, width in (("j", "joint", C), ("b", "base", 1)):
        if key in want:
            assert same_bits(out[key][:n * width],
                             e[name][:n].reshape(-1)), key
            assert np.all(out[key][n * width:] == SENTINEL), key
        else:
            assert np.all(out[key] == SENTINEL), key
    for key, name in (("c", c_key), ("m", m_key)):
        if key in want:
            assert np.array_equal(out[key][:n].view(np.uint32),
                                  e[name][:n]), key
            assert np.all(out[key][n:] == WORD_SENTINEL), key
        else:
            assert np.all(out[key] == WORD_SENTINEL), key
    for key, name, ld, width in (("J", "wj", ldj, C), ("B", "wb", ldb, 1)):
        if key in want:
            planes = out[key][:M * ld].reshape(M, ld)
            assert same_bits(planes[:, :n * width],
                             e[name][:M, :n].reshape(M, -1)), key
            assert np.all(planes[:, n * width:] == SENTINEL), key
            assert np.all(out[key][M * ld:] == SENTINEL), key
        else:
            assert np.all(out[key] == SENTINEL), key


def expect_for(ens, observed, target, cand, M=None):
    L = ol.oracle()
    return fm.expect_many([m.orc for m in ens.members[:M]], ens.qvals,
                          observed, target, cand,
                          L.orc_rng_seed(fm.DRAW_SEED),
                          L.orc_rng_seed(fm.MEMBER_SEED), fm.DRAW_BASE,
                          ens.le is not None)


@pytest.mark.parametrize("C", [1, 62, 63, 64])
def test_candidate_counts_around_a_wave_and_a_tile_one_member_crosses(C):
    """C + 1 = 2, 63, 64, 65 chains per row on a DD(70) target; members of
    K = 4 and K = 1025 in one call: the tile is the larger member's, the
    smaller ends its tile loop early; the scratch path against the caller's
    buffers; base alone (C = 0 in the kernel)"""
    ens = ensemble("dd70_k4_k1025")
    gpus = engines_of("dd70_k4_k1025")
    assert [m.K for m in ens.members] == [4, 1025]
    cand = ((np.arange(C, dtype=np.uint32) * 37 + 5) % 70).astype(np.uint32)
    observed = fe.random_masks(ens.nq, 3, MASK_SEED)
    words = pe.query_words(ens.members[0].orc, ens.qvals)
    e = expect_for(ens, observed, 0, cand)
    n = ens.nq
    try:
        for chunk in (1 << 22, 37):
            gpus[0].set_option("debug.predict_chunk", chunk)
            for mode in (0, 1):
                out = many_dev(gpus, words, n, observed, 0, cand, mode)
                check_dev(out, e, n, 2, C, mode, "jbcmJB")
                # choice without joint: joint stays in engine scratch
                out = many_dev(gpus, words, n, observed, 0, cand, mode, "c")
                check_dev(out, e, n, 2, C, mode, "c")
            out = many_dev(gpus, words, n, observed, 0, cand, 0, "b")
            check_dev(out, e, n, 2, C, 0, "b")
    finally:
        gpus[0].set_option("debug.predict_chunk", 1 << 22)


def test_row_counts_chunks_members_and_each_output_alone():
    """n = 1, 63, 64, 65, 257 at M = 66, several chunks (row q draws with
    engine step draw_base + q + 1 of either stream whatever the chunk), each
    output alone, leading dimensions beyond their planes, nothing written
    past n * C or n"""
    fens, gpus = case("small66")
    ens, M, C, t = fens.ens, fens.M, fens.C, fens.target
    assert M == 66
    words = pe.query_words(ens.members[0].orc, ens.qvals)
    e = fens.expect()
    try:
        for chunk in (1 << 22, 37):
            gpus[0].set_option("debug.predict_chunk", chunk)
            for n in (1, 63, 64, 65, 257):
                for mode in (0, 1):
                    out = many_dev(gpus, words, n, fens.observed, t, None,
                                   mode, ldj=n * C + 3, ldb=n + 5, C=C)
                    check_dev(out, e, n, M, C, mode, "jbcmJB", n * C + 3,
                              n + 5)
        gpus[0].set_option("debug.predict_chunk", 37)
        for want in ("j", "b", "c", "m", "J", "B", "t", ""):
            out = many_dev(gpus, words, 257, fens.observed, t, None, 0, want,
                           C=C)
            check_dev(out, e, 257, M, C, 0, want)
            if "t" in want:
                assert [word(x) for x in out["t"]] == [
                    word(x) for x in e["prior_totals"]]
            else:
                assert out["t"] is None
        # no rows: nothing happens
        out = many_dev(gpus, words, 0, fens.observed, t, None, 0, C=C)
        check_dev(out, e, 0, M, C, 0, "")
    finally:
        gpus[0].set_option("debug.predict_chunk", 1 << 22)


@pytest.mark.parametrize("name", ["mixed_dd", "gp_nich_nich"])
def test_permuting_queries_and_candidates_permutes_the_results(name):
    fens, gpus = case(name)
    q = fens.ens.qvals
    joint, base, choice, member, _, _, _ = many(gpus, fens, "map")
    perm = np.random.default_rng(3).permutation(fens.nq)
    jp, bp, cp, mp, _, _, _ = many(gpus, fens, "map",
                                   qvals=[c[perm] for c in q],
                                   observed=fens.observed[perm])
    assert same_bits(jp, joint[perm]) and same_bits(bp, base[perm])
    assert np.array_equal(cp, choice[perm])
    assert np.array_equal(mp, member[perm])
    cperm = np.random.default_rng(4).permutation(fens.C)
    jc, bc, _, _, _, _, _ = many(gpus, fens, None,
                                 cand=fens.values[cperm])
    assert same_bits(jc, joint[:, cperm]) and same_bits(bc, base)
    # a draw belongs to the row's engine step: row q alone, at its own step
    _, _, choice, member, _, _, _ = many(gpus, fens, "sample")
    for i in (0, 17, fens.nq - 1):
        one = many(gpus, fens, "sample", qvals=[c[i:i + 1] for c in q],
                   observed=fens.observed[i:i + 1],
                   draw_base=fm.DRAW_BASE + i)
        assert same_bits(one[0], joint[i:i + 1])
        assert one[2][0] == choice[i] and one[3][0] == member[i]


def test_predict_feature_many_torch_returns_device_tensors():
    import torch
    from distributions_amd import engine
    fens, gpus = case("gp_nich_nich")
    e = fens.expect()
    words = pe.query_words(fens.ens.members[0].orc, fens.ens.qvals)
    cols = [torch.from_numpy(w.view(np.int32).copy()).cuda() for w in words]
    cols[fens.target] = None
    mask = torch.from_numpy(fens.observed.view(np.int32).copy()).cuda()
    out = engine.predict_feature_many_torch(
        gpus, cols, fens.target, fens.cand, mask, "sample",
        seed=fm.DRAW_SEED, draw_base=fm.DRAW_BASE, members=True)
    assert all(x.is_cuda for x in out[:6])
    joint, base, choice, member, pj, pb, totals = out
    assert same_bits(joint.cpu().numpy(), e["joint"])
    assert same_bits(base.cpu().numpy(), e["base"])
    assert same_bits(pj.cpu().numpy(), e["wj"])
    assert same_bits(pb.cpu().numpy(), e["wb"])
    assert np.array_equal(choice.cpu().numpy().view(np.uint32),
                          e["choice_draw"])
    assert np.array_equal(member.cpu().numpy().view(np.uint32),
                          e["member_draw"])
    assert [word(t) for t in totals] == [word(t) for t in e["prior_totals"]]
    host = many(gpus, fens, "sample", members=True)
    assert same_bits(joint.cpu().numpy(), host[0])
    assert same_bits(base.cpu().numpy(), host[1])
    out = engine.predict_feature_many_torch(gpus, cols, fens.target,
                                            fens.cand, mask, None,
                                            seed=fm.DRAW_SEED)
    assert out[2] is None and out[3] is None and out[4] is None
    assert same_bits(out[0].cpu().numpy(), e["joint"])


def test_the_chains_of_sweep_sequential_many():
    """8 chains advanced in one launch, questioned in one call, advanced
    again: the reader left every engine alone"""
    from distributions_amd import _core, engine
    from test_gpu_chains import assert_same, make_chain
    import workloads
    m, n, k = 8, 300, 20
    chains = [make_chain("dd_bb_gp", n, k + i, 4.0 + i, 0.3, 1 + i % 2,
                         60 + i) for i in range(m)]
    gpus = [g for _, g in chains]
    states = np.array([_core.rng_seed(500 + i) for i in range(m)], np.uint32)
    got = engine.sweep_sequential_many(gpus, 0, n, states)
    for i, (orc, _) in enumerate(chains):
        assert int(got[i]) == orc.gibbs_sequential(0, n, int(states[i]))
    _, _, q, _ = workloads.make("dd_bb_gp", 200, 1, seed=pe.QSEED)
    observed = fe.random_masks(200, 3, MASK_SEED)
    L = ol.oracle()
    e = fm.expect_many([o for o, _ in chains], q, observed, 0, None,
                       L.orc_rng_seed(fm.DRAW_SEED),
                       L.orc_rng_seed(fm.MEMBER_SEED), 0, False)
    joint, base, choice, member, pj, pb, _ = engine.predict_feature_many(
        gpus, q, 0, None, observed, "sample", seed=fm.DRAW_SEED,
        members=True)
    assert same_bits(pj, e["wj"]) and same_bits(pb, e["wb"])
    assert same_bits(joint, e["joint"]) and same_bits(base, e["base"])
    assert np.array_equal(choice, e["choice_draw"])
    assert np.array_equal(member, e["member_draw"])
    assert len(set(member.tolist())) > 1
    again = engine.sweep_sequential_many(gpus, 0, n, got)
    for i, (orc, gpu) in enumerate(chains):
        assert int(again[i]) == orc.gibbs_sequential(0, n, int(got[i]))
        assert_same(orc, gpu, "chain %d after predict_feature_many" % i)


# ---------------------------------------------------------------------------
# refusals


def test_an_open_batch_on_one_member_is_refused():
    fens, _ = case("mixed_dd")
    gpus = [m.engine() for m in fens.ens.members]   # (their own: a state moves)
    e = fens.expect()
    gpus[1].core.batch_sample(0, 256, ol.oracle().orc_rng_seed(3), 0)
    with pytest.raises(RuntimeError, match="batch open"):
        many(gpus, fens, "map")
    gpus[1].core.batch_apply_local()
    gpus[1].core.batch_finish()
    joint = many(gpus, fens, "map")[0]
    assert not same_bits(joint, e["joint"])     # (member 1 has moved on)
    assert same_bits(many(gpus[:1], fens, None)[0], e["wj"][0])


def test_bad_values_and_bad_candidates_are_named():
    fens, gpus = case("mixed_gp")
    e = fens.expect()
    q = fens.ens.qvals
    gpus[0].set_option("debug.predict_chunk", 64)
    try:
        everything = np.full(fens.nq, 7, np.uint32)
        bad = [c.copy() for c in q]
        bad[1][211] = 2
        bad[1][130] = 2                 # the first offending row is named
        bad[0][250] = 200               # (a later row, an earlier feature)
        with pytest.raises(RuntimeError, match="row 130, feature 1"):
            many(gpus, fens, "sample", qvals=bad, observed=everything)
        # the same words in unobserved cells are never read
        hidden = everything.copy()
        hidden[[130, 211]] = 5
        hidden[250] = 6
        many(gpus, fens, "sample", qvals=bad, observed=hidden)
        # process and engines go on
        joint, base, choice, _, _, _, _ = many(gpus, fens, "map")
        assert same_bits(joint, e["joint"]) and same_bits(base, e["base"])
        assert np.array_equal(choice, e["choice_map"])
    finally:
        gpus[0].set_option("debug.predict_chunk", 1 << 22)
    dd, _ = case("mixed_dd")
    with pytest.raises(RuntimeError, match="candidate 2 is outside"):
        many(gpus, dd, "map", cand=np.array([0, 7, 8], np.uint32))
    bb, _ = case("mixed_bb")
    with pytest.raises(RuntimeError, match="candidate 1 is outside"):
        many(gpus, bb, "map", cand=np.array([1, 2], np.uint32))
    with pytest.raises(RuntimeError, match="needs a candidate list"):
        many(gpus, fens, "map", cand=None)
    with pytest.raises(RuntimeError, match="no such target"):
        from distributions_amd import engine
        engine.predict_feature_many(gpus, q, 3, None)


def test_refused_engine_lists_and_arguments():
    from distributions_amd import engine
    fens, gpus = case("mixed_dd")
    q = fens.ens.qvals
    with pytest.raises(RuntimeError, match="one feature list"):
        many([gpus[0], engines_of("gp_nich")[0]], fens, "map")
    other_dim = engine.Gibbs(1.0, 0.0, [engine.dd_shared([0.5] * 12),
                                        engine.bb_shared(0.5, 2.0),
                                        engine.gp_shared(1.0, 1.0)])
    other_dim.load_rows_unassigned([np.zeros(4, np.uint32)] * 3, 1)
    with pytest.raises(RuntimeError, match="one feature list"):
        many([gpus[0], other_dim], fens, "map")
    with pytest.raises(RuntimeError, match="one clustering model"):
        many([gpus[0], engines_of("le_m1")[0]], fens, "map")
    with pytest.raises(RuntimeError, match="null engine"):
        many([gpus[0], None], fens, "map")
    with pytest.raises(RuntimeError, match="the same engine twice"):
        many([gpus[0], gpus[1], gpus[0]], fens, "map")
    with pytest.raises(RuntimeError, match="at most 65535 engines"):
        many([gpus[0]] * 65536, fens, "map")
    words = pe.query_words(fens.ens.members[0].orc, q)
    args = (gpus, words, 10, fens.observed, 0, None)
    with pytest.raises(RuntimeError, match="mode is 0"):
        many_dev(*args, 2, C=fens.C)
    with pytest.raises(RuntimeError, match="unknown flag"):
        many_dev(*args, 0, flags=1, C=fens.C)
    with pytest.raises(RuntimeError, match="members_joint_ld"):
        many_dev(*args, 0, ldj=10 * fens.C - 1, C=fens.C)
    with pytest.raises(RuntimeError, match="members_base_ld"):
        many_dev(*args, 0, ldb=9, C=fens.C)
