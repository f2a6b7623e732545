"""dist_gibbs_predict_many (k_predict_many, k_ensemble_fold,
k_predict_many_pick): held-out rows' predictive averaged over M engines, bit
for bit against the expectation tests/ensemble_expect.py composes from the
oracle (and tests/test_ensemble_oracle.py holds to float64).

Feature lists dd, gp_nich, dd_bb_gp and dpd with a member whose OTHER has no
mass (fast_log(0) in its plane there), LowEntropy at M = 1, 2, 5, a member of
only empty groups, DD-256 at K = 1025; then the identities with Gibbs.predict, both
draw forms, launch geometry (M up to 130: the fold loops past a wave), a
permutation of the queries, the chains of sweep_sequential_many, and the
reader rules."""
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
import oracle_lib as ol  # noqa: E402
import predict_expect as pe  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
WORD_SENTINEL = -7

LE5 = [dict(k=k, empty=1, alpha=1.0, d=0.0, sweeps=0)
       for k in (4, 17, 41, 8, 25)]
BIG3 = [dict(k=1024, empty=1, alpha=a, d=d, sweeps=0, n=4096)
        for a, d in ((1.0, 0.5), (4.0, 0.2), (0.5, 0.0))]
# 130 members of 64-row tables: cheap to build, and the fold loops past a wave
SMALL130 = [dict(k=3 + e % 3, empty=1 + e % 2, alpha=1.0 + e % 4,
                 d=0.25 * (e % 3), sweeps=0, n=64) for e in range(130)]

ENSEMBLES = {
    "dd": lambda: ee.Ensemble("dd", ee.SPECS3),
    "gp_nich": lambda: ee.Ensemble("gp_nich", ee.SPECS3),
    "dd_bb_gp": lambda: ee.Ensemble("dd_bb_gp", ee.SPECS3),
    # member 1's OTHER has no mass: fast_log(alpha * 0) at rows 1 and 2, the
    # table's value for a zero argument (about -88, not -inf)
    "dpd_other_mixed": lambda: ee.Ensemble(
        "dpd_other", ee.SPECS3, beta0=[0.1, 0.0, 0.1], other=(1, 2)),
    "le_dd_m1": lambda: ee.Ensemble("dd", LE5[:1], le=2000),
    "le_dd_m2": lambda: ee.Ensemble("dd", LE5[:2], le=2000),
    "le_dd_m5": lambda: ee.Ensemble("dd", LE5, le=2000),
    "only_empty_member": lambda: ee.Ensemble(
        "dd_bb_gp", [ee.SPECS3[0],
                     dict(k=0, empty=1, alpha=1.0, d=0.5, sweeps=0, n=64),
                     ee.SPECS3[2]]),
    "dd256_k1025": lambda: ee.Ensemble("dd", BIG3, nq=256, dim=256),
    "small130": lambda: ee.Ensemble("dd", SMALL130, nq=257),
    # eight features, K = 8, 34 and 43 (tests/eight_expect.py)
    "eight3": lambda: xe.eight3(),
}
_ENS = {}
_GPUS = {}


def ensemble(name):
    if name not in _ENS:
        _ENS[name] = ENSEMBLES[name]()
    return _ENS[name]


def engines_of(name):
    """one set of engines per ensemble, shared: predict_many leaves them as
    they were"""
    if name not in _GPUS:
        _GPUS[name] = ensemble(name).engines()
    return _GPUS[name]


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


def predict_many(gpus, qvals, mode, **kw):
    from distributions_amd import engine
    return engine.predict_many(gpus, qvals, mode, seed=ee.DRAW_SEED,
                               draw_base=kw.pop("draw_base", ee.DRAW_BASE),
                               **kw)


@pytest.mark.parametrize("name", [n for n in ENSEMBLES if n != "small130"])
def test_predict_many_is_the_oracles_bit_for_bit(name):
    from distributions_amd import engine
    ens = ensemble(name)
    e = ens.expect()
    gpus = engines_of(name)
    logp, member, group, planes, totals = predict_many(
        gpus, ens.qvals, "sample", members=True)
    logp_m, first, group_m, planes_m, totals_m = predict_many(
        gpus, ens.qvals, "map", members=True)
    logp_n, none_m, none_g, no_planes, _ = predict_many(gpus, ens.qvals, None)
    print("%s: M=%d, K=%s, %d held-out rows: logp bits differ in %d rows, "
          "planes in %d cells, members in %d / %d, groups in %d / %d; "
          "-inf cells %d, NaN logp %d" % (
              name, ens.M, [m.K for m in ens.members], ens.nq,
              int((logp.view(np.uint32) != e["logp"].view(np.uint32)).sum()),
              int((planes.view(np.uint32) != e["w"].view(np.uint32)).sum()),
              int((member != e["member_draw"]).sum()),
              int((first != e["member_map"]).sum()),
              int((group != e["group_draw"]).sum()),
              int((group_m != e["group_map"]).sum()),
              int(np.isinf(e["w"]).sum()), int(np.isnan(e["logp"]).sum())))
    assert same_bits(planes, e["w"]) and same_bits(planes_m, e["w"])
    assert [word(t) for t in totals] == [word(t) for t in e["prior_totals"]]
    assert [word(t) for t in totals_m] == [word(t) for t in totals]
    for got in (logp, logp_m, logp_n):
        assert same_bits(got, e["logp"])
    assert none_m is None and none_g is None and no_planes is None
    assert np.array_equal(member, e["member_draw"])
    assert np.array_equal(first, e["member_map"])
    assert np.array_equal(group, e["group_draw"])
    assert np.array_equal(group_m, e["group_map"])
    if name != "dpd_other_mixed":   # (the band takes no fast_log(0))
        print("%s: worst excursion / band %.3f" % (
            name, ee.excursion(logp, ens).max()))
        assert ee.excursion(logp, ens).max() <= 1.0
    # the draw-all form: the same bits
    for mode, m_key, g_key in (("sample", "member_draw", "group_draw"),
                               ("map", "member_map", "group_map")):
        logp_a, member_a, group_a, _, _ = predict_many(
            gpus, ens.qvals, mode, flags=engine.PREDICT_MANY_DRAW_ALL)
        assert same_bits(logp_a, e["logp"])
        assert np.array_equal(member_a, e[m_key])
        assert np.array_equal(group_a, e[g_key])


@pytest.mark.parametrize("name", ["gp_nich", "le_dd_m5", "dpd_other_mixed",
                                  "eight3"])
def test_identities_with_predict(name):
    ens = ensemble(name)
    gpus = engines_of(name)
    for mode in ("sample", "map"):
        logp, member, group, planes, totals = predict_many(
            gpus, ens.qvals, mode, members=True)
        own = [g.predict(ens.qvals, mode, seed=ee.DRAW_SEED,
                         draw_base=ee.DRAW_BASE) for g in gpus]
        for e, (lp, _, total) in enumerate(own):
            assert word(total) == word(totals[e])
            with np.errstate(invalid="ignore"):
                want = (lp - np.float32(total)).astype(np.float32) \
                    if ens.le is not None else lp
            assert same_bits(planes[e], want), e
        groups = np.stack([o[1] for o in own])
        assert np.array_equal(group, groups[member, np.arange(ens.nq)])


def many_dev(gpus, words, n, mode, want="lmgp", ld=None, flags=0, pad=64,
             draw_base=ee.DRAW_BASE):
    """predict_many_dev on the first n held-out rows into sentinel-filled
    device buffers -> dict of host copies, padding included (l: logp,
    m: member, g: group, p: the planes with leading dimension ld)"""
    import torch
    from distributions_amd import _core
    M = len(gpus)
    ld = n if ld is None else ld
    cols = [torch.from_numpy(np.ascontiguousarray(w[:n]).view(np.int32)
                             .copy()).cuda() for w in words]
    logp = torch.full((n + pad,), SENTINEL, dtype=torch.float32,
                      device="cuda")
    member = torch.full((n + pad,), WORD_SENTINEL, dtype=torch.int32,
                        device="cuda")
    group = torch.full((n + pad,), WORD_SENTINEL, dtype=torch.int32,
                       device="cuda")
    planes = torch.full((max(M, 1) * ld + pad,), SENTINEL,
                        dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    L = ol.oracle()
    totals = _core.predict_many_dev(
        [None if g is None else g.core for g in gpus],
        [int(t.data_ptr()) for t in cols], n,
        int(logp.data_ptr()) if "l" in want else 0,
        int(member.data_ptr()) if "m" in want else 0,
        int(group.data_ptr()) if "g" in want else 0, mode,
        L.orc_rng_seed(ee.DRAW_SEED), L.orc_rng_seed(ee.MEMBER_SEED),
        draw_base, int(planes.data_ptr()) if "p" in want else 0, ld,
        "t" in want, flags)
    torch.cuda.synchronize()
    return dict(l=logp.cpu().numpy(), m=member.cpu().numpy(),
                g=group.cpu().numpy(), p=planes.cpu().numpy(), t=totals)


def check_dev(out, e, n, M, mode, want, ld):
    """every asked output right on [0, n), everything else untouched"""
    m_key, g_key = (("member_draw", "group_draw") if mode == 0
                    else ("member_map", "group_map"))
    if "l" in want:
        assert same_bits(out["l"][:n], e["logp"][:n])
        assert np.all(out["l"][n:] == SENTINEL)
    else:
        assert np.all(out["l"] == SENTINEL)
    for key, name in (("m", m_key), ("g", g_key)):
        if key in want:
            assert np.array_equal(out[key][:n].view(np.uint32), e[name][:n])
            assert np.all(out[key][n:] == WORD_SENTINEL)
        else:
            assert np.all(out[key] == WORD_SENTINEL)
    if "p" in want:
        planes = out["p"][:M * ld].reshape(M, ld)
        assert same_bits(planes[:, :n], e["w"][:M, :n])
        assert np.all(planes[:, n:] == SENTINEL)
        assert np.all(out["p"][M * ld:] == SENTINEL)
    else:
        assert np.all(out["p"] == SENTINEL)


@pytest.mark.parametrize("M", [1, 2, 65, 130])
def test_launch_geometry_chunks_and_optional_outputs(M):
    """whole and partial waves of rows, 1 .. 130 members, several chunks (row
    q draws with engine step draw_base + q + 1 of either stream whatever the
    chunk), each output alone, a leading dimension beyond n, nothing written
    past n"""
    from distributions_amd import engine
    ens = ensemble("small130")
    gpus = engines_of("small130")[:M]
    words = pe.query_words(ens.members[0].orc, ens.qvals)
    L = ol.oracle()
    e = ee.expect_many([m.orc for m in ens.members[:M]], ens.qvals,
                       L.orc_rng_seed(ee.DRAW_SEED),
                       L.orc_rng_seed(ee.MEMBER_SEED), ee.DRAW_BASE, False)
    try:
        for chunk in (1 << 22, 100):
            gpus[0].set_option("debug.predict_chunk", chunk)
            for n in (1, 63, 64, 65, 257):
                for mode in (0, 1):
                    out = many_dev(gpus, words, n, mode, ld=n + 3)
                    check_dev(out, e, n, M, mode, "lmgp", n + 3)
                out = many_dev(gpus, words, n, 0, "lmg",
                               flags=engine.PREDICT_MANY_DRAW_ALL)
                check_dev(out, e, n, M, 0, "lmg", n)
        gpus[0].set_option("debug.predict_chunk", 100)
        for want in ("l", "m", "g", "p", "t", ""):
            out = many_dev(gpus, words, 257, 0, want)
            check_dev(out, e, 257, M, 0, want, 257)
            if "t" in want:
                assert [word(t) for t in out["t"]] == [
                    word(t) for t in e["prior_totals"]]
            else:
                assert out["t"] is None
        # no rows, no engines: nothing happens
        for n, who in ((0, gpus), (65, [])):
            out = many_dev(who, words, n, 0)
            for key in "lp":
                assert np.all(out[key] == SENTINEL)
            for key in "mg":
                assert np.all(out[key] == WORD_SENTINEL)
    finally:
        gpus[0].set_option("debug.predict_chunk", 1 << 22)


def test_predict_many_torch_returns_device_tensors():
    import torch
    from distributions_amd import engine
    ens = ensemble("gp_nich")
    e = ens.expect()
    gpus = engines_of("gp_nich")
    words = pe.query_words(ens.members[0].orc, ens.qvals)
    cols = [torch.from_numpy(w.view(np.int32).copy()).cuda() for w in words]
    logp, member, group, planes, totals = engine.predict_many_torch(
        gpus, cols, "sample", seed=ee.DRAW_SEED, draw_base=ee.DRAW_BASE,
        members=True)
    assert logp.is_cuda and member.is_cuda and group.is_cuda and planes.is_cuda
    assert same_bits(logp.cpu().numpy(), e["logp"])
    assert same_bits(planes.cpu().numpy(), e["w"])
    assert np.array_equal(member.cpu().numpy().view(np.uint32),
                          e["member_draw"])
    assert np.array_equal(group.cpu().numpy().view(np.uint32),
                          e["group_draw"])
    assert [word(t) for t in totals] == [word(t) for t in e["prior_totals"]]
    logp, member, group, planes, _ = engine.predict_many_torch(
        gpus, cols, None, seed=ee.DRAW_SEED)
    assert member is None and group is None and planes is None
    assert same_bits(logp.cpu().numpy(), e["logp"])


@pytest.mark.parametrize("name", ["dd", "dd_bb_gp"])
def test_permuting_the_queries_permutes_the_results(name):
    ens = ensemble(name)
    gpus = engines_of(name)
    logp, first, group, _, _ = predict_many(gpus, ens.qvals, "map")
    perm = np.random.default_rng(3).permutation(ens.nq)
    logp_p, first_p, group_p, _, _ = predict_many(
        gpus, [q[perm] for q in ens.qvals], "map")
    assert same_bits(logp_p, logp[perm])
    assert np.array_equal(first_p, first[perm])
    assert np.array_equal(group_p, group[perm])
    # a draw belongs to the row's engine step: row q moved to position i
    # draws as before when position i's step is q's
    lp, member, group, _, _ = predict_many(gpus, ens.qvals, "sample")
    for i in (0, 17, ens.nq - 1):
        q = int(perm[i])
        one = predict_many(gpus, [c[q:q + 1] for c in ens.qvals], "sample",
                           draw_base=ee.DRAW_BASE + q)
        assert same_bits(one[0], lp[q:q + 1])
        assert one[1][0] == member[q] and one[2][0] == group[q]


def test_the_chains_of_sweep_sequential_many():
    """8 chains advanced in one launch, questioned in one call, advanced
    again: the readers left every engine alone"""
    from distributions_amd import _core, engine
    from test_gpu_chains import assert_same, make_chain
    m, n, k = 8, 300, 20
    chains = [make_chain("dd_bb_gp", n, k + i, 4.0 + i, 0.3, 1 + i % 2,
                         60 + i) for i in range(m)]
    gpus = [g for _, g in chains]
    states = np.array([_core.rng_seed(500 + i) for i in range(m)], np.uint32)
    got = engine.sweep_sequential_many(gpus, 0, n, states)
    for i, (orc, _) in enumerate(chains):
        assert int(got[i]) == orc.gibbs_sequential(0, n, int(states[i]))
    import workloads
    _, _, q, _ = workloads.make("dd_bb_gp", 200, 1, seed=pe.QSEED)
    L = ol.oracle()
    e = ee.expect_many([o for o, _ in chains], q,
                       L.orc_rng_seed(ee.DRAW_SEED),
                       L.orc_rng_seed(ee.MEMBER_SEED), 0, False)
    logp, member, group, planes, totals = engine.predict_many(
        gpus, q, "sample", seed=ee.DRAW_SEED, members=True)
    assert same_bits(planes, e["w"])
    assert same_bits(logp, e["logp"])
    assert np.array_equal(member, e["member_draw"])
    assert np.array_equal(group, e["group_draw"])
    assert len(set(member.tolist())) > 1
    again = engine.sweep_sequential_many(gpus, 0, n, got)
    for i, (orc, gpu) in enumerate(chains):
        assert int(again[i]) == orc.gibbs_sequential(0, n, int(got[i]))
        assert_same(orc, gpu, "chain %d after predict_many" % i)


# ---------------------------------------------------------------------------
# reader rules


def test_an_open_batch_on_one_member_is_refused():
    ens = ensemble("dd")
    gpus = [m.engine() for m in ens.members]    # (their own: a state moves)
    e = ens.expect()
    gpus[1].core.batch_sample(0, 256, ol.oracle().orc_rng_seed(3), 0)
    with pytest.raises(RuntimeError, match="batch open"):
        predict_many(gpus, ens.qvals, "map")
    gpus[1].core.batch_apply_local()
    gpus[1].core.batch_finish()
    logp, _, _, _, _ = predict_many(gpus, ens.qvals, "map")
    assert not same_bits(logp, e["logp"])       # (member 1 has moved on)
    assert same_bits(predict_many(gpus[:1], ens.qvals, None)[0],
                     ee.fold(e["w"][:1], 1, 0)[0])


def test_a_value_outside_its_domain_fails_and_names_the_row():
    ens = ensemble("dd_bb_gp")
    e = ens.expect()
    gpus = engines_of("dd_bb_gp")
    gpus[0].set_option("debug.predict_chunk", 64)
    try:
        bad = [q.copy() for q in ens.qvals]
        bad[1][211] = 2
        bad[1][130] = 2                 # the first offending row is named
        bad[2][130] = 2 ** 31           # (GammaPoisson takes any count)
        bad[0][250] = 200               # (a later row, an earlier feature)
        with pytest.raises(RuntimeError, match="row 130, feature 1"):
            predict_many(gpus, bad, "sample")
        # process and engines go on
        logp, first, group, _, _ = predict_many(gpus, ens.qvals, "map")
        assert same_bits(logp, e["logp"])
        assert np.array_equal(first, e["member_map"])
        assert np.array_equal(group, e["group_map"])
    finally:
        gpus[0].set_option("debug.predict_chunk", 1 << 22)


def test_refused_engine_lists():
    from distributions_amd import engine
    dd = engines_of("dd")
    q = ensemble("dd").qvals
    with pytest.raises(RuntimeError, match="one feature list"):
        predict_many([dd[0], engines_of("gp_nich")[0]], q, "map")
    other_dim = engine.Gibbs(1.0, 0.0, [engine.dd_shared([0.5] * 12)])
    other_dim.load_rows_unassigned([np.zeros(4, np.uint32)], 1)
    with pytest.raises(RuntimeError, match="one feature list"):
        predict_many([dd[0], other_dim], q, "map")
    with pytest.raises(RuntimeError, match="one clustering model"):
        predict_many([dd[0], engines_of("le_dd_m1")[0]], q, "map")
    with pytest.raises(RuntimeError, match="null engine"):
        predict_many([dd[0], None], q, "map")
    with pytest.raises(RuntimeError, match="the same engine twice"):
        predict_many([dd[0], dd[1], dd[0]], q, "map")
    words = pe.query_words(ensemble("dd").members[0].orc, q)
    with pytest.raises(RuntimeError, match="mode is 0"):
        many_dev(dd, words, 10, 2)
    with pytest.raises(RuntimeError, match="unknown flag"):
        many_dev(dd, words, 10, 0, flags=2)
    with pytest.raises(RuntimeError, match="members_ld"):
        many_dev(dd, words, 10, 0, ld=9)
