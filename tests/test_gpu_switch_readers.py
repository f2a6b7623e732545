"""The held-out readers AFTER a hyper-parameter step: predict,
responsibilities, coassign, coassign_topk, predict_feature, marginals,
sample_rows, relate and their _many and ShardedGibbs forms on engines whose
hyper-parameters were switched by set_shared / set_clustering or drawn by
sample_hypers / sample_clustering, bit for bit against the expectation of the
same oracle state adopted under the new values (tests/switch_expect.py, held to
float64 and shown to tell a stale reader apart by tests/test_switch_oracle.py).

A reader that kept anything the hyper step has to rebuild -- a feature's
prior[], alpha_sum, gp_lut, the DPD `other`, the per-group caches and S,
base[], the clustering model's tables, its own scratch (predict_prior, the
many_* buffers in an ensemble's first engine), an entry of the process-wide
small-lgamma table -- returns the old values' answer, which is finite and
plausible and differs from the expectation in every row.

a. every reader after every row of switch_expect.SWITCHES by route "set",
   three of them by route "sample" as well; the engine is unchanged after
b. there and back: every reader's output before a switch is its output after
   the switch was made, read under, and undone -- in every bit; also with one
   feature alone switched and restored
c. a reader between the switch and a sweep: the sweep is the adopted oracle's
d. an ensemble of three, member 0 (which owns the _many scratch) switched
   alone, then member 1 alone
e. two value-partitioned ranks switch alike and predict
f. the small-lgamma table taken through two purges by 48 set_shared calls on a
   DD-256 engine, while another engine holds arguments in it; then a
   score_data_grid that holds more arguments than the table has room for

relate is held as tests/test_gpu_relate.py holds it: its sums are those of
sample_rows_many's rows under marginals on the same engine.  That is an
identity between readers, not a comparison with the oracle: it follows the
switch through sample_rows and marginals, which are held to the oracle here.

Planted once, not committed: Gibbs.set_shared taking the new Shared into
self.shareds without handing it to the core.  On gp_nich_swept and
dd_bb_gp_swept switch_expect's check of the core's record failed first
(core.shared(f) against the installed Shared); with that check passed over,
predict (logp in 300 of 300 rows, 16 and 77 draws), responsibilities,
coassign_topk, predict_feature (every joint cell), marginals (every cell
that names a feature), sample_rows' groups and check_cells on the device's own
groups all failed; relate alone did not notice, as said above.
"""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import coassign_topk_expect as ct  # noqa: E402
import ensemble_expect as ee  # noqa: E402
import feature_expect as fe  # noqa: E402
import feature_many_expect as fm  # noqa: E402
import marginals_expect as mx  # noqa: E402
import oracle_lib as ol  # noqa: E402
import predict_expect as pe  # noqa: E402
import sample_expect as se  # noqa: E402
import switch_expect as sx  # noqa: E402
import workloads  # noqa: E402
from test_gpu_coassign import assert_cells  # noqa: E402
from test_gpu_coassign_topk import assert_same  # noqa: E402
from test_gpu_hypers import assert_scores, oracle_grid  # noqa: E402
from test_gpu_marginals import same_bits  # noqa: E402
from test_gpu_predict import (  # noqa: E402
    DIM, N, PER, WORLD, bits, rank_queries, same, snapshot, word)
from test_gpu_predict_feature import check as check_feature  # noqa: E402
from test_gpu_relate import (  # noqa: E402
    BASE as RELATE_BASE, MEMBER_SEED as RELATE_MEMBER_SEED,
    SEED as RELATE_SEED, check_sums, host_d)
from test_gpu_sample_rows import check_cells, words_of  # noqa: E402

pytestmark = pytest.mark.gpu

NQ = 48                 # rows of predict_feature and sample_rows
RELATE_N = 256
KEYS = [(n, "set") for n in sx.SWITCHES] + [(n, "sample") for n in sx.SAMPLED]
_STATE = {}


def seed_state():
    return ol.oracle().orc_rng_seed(pe.DRAW_SEED)


def subject(name, route):
    """one switched engine per (row, route), shared by the tests of that row:
    the readers change nothing -> (Switched, engine, snapshot at the switch)"""
    key = (name, route)
    if key not in _STATE:
        sw = sx.switched(name)
        gpu = sw.engine(route)
        if route == "sample":
            print("%s: sample_hypers / sample_clustering drew %s"
                  % (name, sw.drawn))
        _STATE[key] = (sw, gpu, snapshot(gpu))
    return _STATE[key]


def unchanged(gpu, before):
    assert same(before, snapshot(gpu))
    assert gpu.validate()["code"] == 0


# ---------------------------------------------------------------------------
# the readers, each held as its own test holds it on an unswitched engine


def check_predict(sw, gpu, e=None, excursion=True):
    e = sw.expect() if e is None else e
    logp, draw, total = gpu.predict(sw.qvals, "sample", seed=pe.DRAW_SEED,
                                    draw_base=pe.DRAW_BASE)
    logp_m, first, total_m = gpu.predict(sw.qvals, "map")
    logp_n, none, _ = gpu.predict(sw.qvals, None)
    print("%s: K=%d, %d held-out rows: logp bits differ in %d rows, draws in "
          "%d, maxima in %d" % (
              sw.name, sw.K, len(logp),
              int((bits(logp) != bits(e["logp"])).sum()),
              int((draw != e["draw"]).sum()), int((first != e["map"]).sum())))
    assert np.array_equal(bits(logp), bits(e["logp"]))
    assert np.array_equal(bits(logp_m), bits(e["logp"]))
    assert np.array_equal(bits(logp_n), bits(e["logp"]))
    assert none is None
    assert np.array_equal(draw, e["draw"])
    assert np.array_equal(first, e["map"])
    assert word(total) == word(e["prior_total"]) == word(total_m)
    if excursion:
        x = pe.excursion(logp, sw)
        print("%s: worst excursion / band %.3f" % (sw.name, x.max()))
        assert x.max() <= 1.0


def check_coassign(sub, gpus, what):
    """responsibilities, coassign rectangular and symmetric, the law's band"""
    from test_gpu_coassign import call
    q, t = sub.cols(sub.rq), sub.cols(sub.rt)
    rows = np.concatenate([sub.rq, sub.rt])
    ok = sub.specified(rows)
    for gpu, want in zip(gpus, sub.r()):
        got = gpu.responsibilities(sub.cols(rows))
        assert got.shape == want.shape == (len(rows), len(gpu))
        assert np.array_equal(bits(got)[ok], bits(want)[ok]), what
        assert (got[ok] >= 0).all()
    rect = call(gpus, q, t)
    assert_cells(rect, sub.expect(False), sub.mask(False), what + " rect")
    sym = call(gpus, q)
    assert_cells(sym, sub.expect(True), sub.mask(True), what + " sym")
    assert np.array_equal(bits(sym), bits(sym.T))
    C, band = sub.law(False)
    mask = sub.mask(False)
    assert (np.abs(rect.astype(np.float64) - C)[mask] <= band[mask]).all()


def check_topk(sub, gpus, what, k=10):
    from test_gpu_coassign_topk import topk
    case = sx.TopkCase(sub)
    q, t = sub.cols(case.rq), sub.cols(case.rt)
    assert_same(topk(gpus, q, t, k), ct.topk(case.expect(False), k),
                what + " rect")
    assert_same(topk(gpus, q, None, k), ct.topk(case.expect(True), k, True),
                what + " sym without self")


def check_predict_feature(sw, gpu):
    F = len(sw.osh)
    n = 24 if sw.K > 256 else NQ
    q = [v[:n] for v in sw.qvals]
    for target in range(F):
        cand = fe.candidates_for(sw.osh[target])
        masks = fe.random_masks(n, F, 100 + target)
        e = fe.expect(sw.orc, q, masks, target, cand, seed_state(),
                      pe.DRAW_BASE)
        check_feature(gpu, q, target, cand, masks, e,
                      "%s target %d" % (sw.name, target))


def check_marginals(sw, gpu):
    masks = mx.all_masks(len(sw.osh))
    # (the single-engine entry is the member's plane of marginals_many:
    # under LowEntropy minus the prior total)
    want = mx.expect_many([sw.orc], sw.qvals, masks, sw.le is not None)["w"][0]
    got = gpu.marginals(sw.qvals, masks)
    print("%s: %d rows x %d masks: bits differ in %d cells" % (
        sw.name, got.shape[0], len(masks),
        int((bits(got) != bits(want)).sum())))
    assert same_bits(got, want)


def check_sample_rows(sw, gpu):
    F = len(sw.osh)
    q = [v[:NQ] for v in sw.qvals]
    given = words_of(sw, q)
    masks = fe.random_masks(NQ, F, 41)
    want = se.expect_groups(sw.orc, q, masks, seed_state(), pe.DRAW_BASE)
    cols, groups = gpu.sample_rows(values=q, observed=masks,
                                   seed=pe.DRAW_SEED, draw_base=pe.DRAW_BASE)
    assert np.array_equal(groups, want)
    cells, wrong = check_cells(sw, gpu, cols, groups, masks, given,
                               pe.DRAW_BASE, sw.name)
    want0 = se.expect_groups(sw.orc, None, None, seed_state(), pe.DRAW_BASE,
                             nq=NQ)
    cols_u, groups_u = gpu.sample_rows(n=NQ, seed=pe.DRAW_SEED,
                                       draw_base=pe.DRAW_BASE)
    assert np.array_equal(groups_u, want0)
    c2, w2 = check_cells(sw, gpu, cols_u, groups_u, None, None, pe.DRAW_BASE,
                         sw.name + " unconditional")
    cells, wrong = cells + c2, wrong + w2
    print("%s: %d cells of GP / BNB / NICH compared, %d differ" % (
        sw.name, cells, wrong))
    assert wrong * 100000 <= cells


def check_relate(gpu):
    d = host_d([gpu], RELATE_N, single=True)
    mo = gpu.relate(RELATE_N, seed=RELATE_SEED,
                    member_seed=RELATE_MEMBER_SEED, draw_base=RELATE_BASE,
                    moments=True)[2]
    check_sums(mo, d, RELATE_N)


# ---------------------------------------------------------------------------
# a. every reader after the switch is the switched oracle's


@pytest.mark.parametrize("name,route", KEYS)
def test_predict_after_the_switch(name, route):
    sw, gpu, before = subject(name, route)
    check_predict(sw, gpu)
    unchanged(gpu, before)


@pytest.mark.parametrize("name,route", KEYS)
def test_responsibilities_and_coassign_after_the_switch(name, route):
    sw, gpu, before = subject(name, route)
    check_coassign(sw.subject(), [gpu], "%s %s" % (name, route))
    unchanged(gpu, before)


@pytest.mark.parametrize("name,route", KEYS)
def test_coassign_topk_after_the_switch(name, route):
    sw, gpu, before = subject(name, route)
    check_topk(sw.subject(), [gpu], "%s %s" % (name, route))
    unchanged(gpu, before)


@pytest.mark.parametrize("name,route", KEYS)
def test_predict_feature_after_the_switch(name, route):
    sw, gpu, before = subject(name, route)
    check_predict_feature(sw, gpu)
    unchanged(gpu, before)


@pytest.mark.parametrize("name,route", KEYS)
def test_marginals_after_the_switch(name, route):
    sw, gpu, before = subject(name, route)
    check_marginals(sw, gpu)
    unchanged(gpu, before)


@pytest.mark.parametrize("name,route", KEYS)
def test_sample_rows_after_the_switch(name, route):
    sw, gpu, before = subject(name, route)
    check_sample_rows(sw, gpu)
    unchanged(gpu, before)


@pytest.mark.parametrize("name,route", KEYS)
def test_relate_after_the_switch(name, route):
    sw, gpu, before = subject(name, route)
    check_relate(gpu)
    unchanged(gpu, before)


# ---------------------------------------------------------------------------
# b. there and back


def read_all(gpu, c):
    """every reader's output on the case's held-out rows, as bytes"""
    F = len(c.osh)
    q = c.qvals
    head = [v[:NQ] for v in q]
    a, b = [v[:70] for v in q], [v[100:145] for v in q]
    masks = fe.random_masks(NQ, F, 41)
    out = list(gpu.predict(q, "sample", seed=pe.DRAW_SEED,
                           draw_base=pe.DRAW_BASE))
    out += list(gpu.predict(q, "map"))[:2]
    out += [gpu.responsibilities(a), gpu.coassign(a, b), gpu.coassign(a)]
    out += list(gpu.coassign_topk(a, b, 10))
    for target in range(F):
        out += list(gpu.predict_feature(
            head, target, fe.candidates_for(c.osh[target]), masks, "sample",
            seed=pe.DRAW_SEED, draw_base=pe.DRAW_BASE))
    out.append(gpu.marginals(q, mx.all_masks(F)))
    cols, groups = gpu.sample_rows(values=head, observed=masks,
                                   seed=pe.DRAW_SEED, draw_base=pe.DRAW_BASE)
    out += words_of(c, cols) + [groups]
    cols, groups = gpu.sample_rows(n=NQ, seed=pe.DRAW_SEED,
                                   draw_base=pe.DRAW_BASE)
    out += words_of(c, cols) + [groups]
    out += list(gpu.relate(RELATE_N, seed=RELATE_SEED,
                           member_seed=RELATE_MEMBER_SEED,
                           draw_base=RELATE_BASE, moments=True))
    return [np.ascontiguousarray(x).tobytes() for x in out]


def differing(a, b):
    return [i for i, (x, y) in enumerate(zip(a, b)) if x != y]


@pytest.mark.parametrize("name", ["gp_nich_swept", "dd_bb_gp_swept",
                                  "dpd_other_swept"])
def test_there_and_back_gives_the_first_readings_bits(name):
    c = fe.case(name)
    sw = sx.switched(name)
    gpu = c.engine()
    first = read_all(gpu, c)
    assert not differing(first, read_all(gpu, c))
    # the whole switch: read under it (the readers' scratch is then the new
    # values'), and back to the constructor's values
    sx.install(gpu, sw.gsh, sw.clustering)
    under = read_all(gpu, c)
    assert 0 in differing(first, under)      # (predict's logp, at the least)
    sx.install(gpu, c.gsh, (c.alpha, c.d))
    back = read_all(gpu, c)
    assert not differing(first, back), differing(first, back)
    # one feature alone, switched and restored
    for f in range(len(c.osh)):
        gpu.set_shared(f, sw.gsh[f])
        assert differing(first, read_all(gpu, c))
        gpu.set_shared(f, c.gsh[f])
        back = read_all(gpu, c)
        assert not differing(first, back), (f, differing(first, back))
    assert gpu.validate()["code"] == 0
    assert np.array_equal(gpu.assignments(), c.orc.assign)


# ---------------------------------------------------------------------------
# c. a reader between the switch and a sweep


@pytest.mark.parametrize("name", ["gp_nich_swept", "dd_bb_gp_swept"])
def test_readers_between_the_switch_and_a_sweep(name):
    sw = sx.switched(name)          # (its own oracle: the state moves)
    gpu = sw.engine("set")
    sub = sw.subject()
    check_predict(sw, gpu)
    gpu.coassign(sub.cols(sub.rq), sub.cols(sub.rt))
    orc = sw.orc
    st = ol.oracle().orc_rng_seed(11)
    base = 7 * sw.n
    for b in range(0, sw.n, 500):
        orc.gibbs_batch(b, min(sw.n, b + 500), st, base)
    gpu.sweep(0, sw.n, 500, 11, draw_base=base)
    gpu.predict(sw.qvals, "map")     # (closes a run the sweep left open)
    assert np.array_equal(gpu.assignments(), orc.assign)
    assert np.array_equal(gpu.counts(), orc.counts())
    assert not np.array_equal(orc.assign, sw.case.orc.assign)
    gpu.validate()
    e = pe.expect(orc, sw.qvals, seed_state(), pe.DRAW_BASE)
    assert not np.array_equal(bits(e["logp"]), bits(sw.expect()["logp"]))
    check_predict(sw, gpu, e, excursion=False)


# ---------------------------------------------------------------------------
# d. ensembles: one member of three switched


def check_ensemble(ens, gpus, what):
    from distributions_amd import engine
    from test_gpu_predict_many import predict_many
    from test_gpu_sample_rows_many import check_against, expect, host
    F = len(ens.members[0].osh)
    e = ens.expect()
    # predict_many
    logp, member, group, planes, totals = predict_many(
        gpus, ens.qvals, "sample", members=True)
    logp_m, first, group_m, _, _ = predict_many(gpus, ens.qvals, "map",
                                                members=True)
    assert same_bits(planes, e["w"]), what
    assert [word(t) for t in totals] == [word(t) for t in e["prior_totals"]]
    assert same_bits(logp, e["logp"]) and same_bits(logp_m, e["logp"]), what
    assert np.array_equal(member, e["member_draw"])
    assert np.array_equal(first, e["member_map"])
    assert np.array_equal(group, e["group_draw"])
    assert np.array_equal(group_m, e["group_map"])
    assert ee.excursion(logp, ens).max() <= 1.0
    # coassign_many, coassign_topk_many
    sub = sx.Subject(ens)
    check_coassign(sub, gpus, what)
    check_topk(sub, gpus, what)
    # marginals_many
    masks = mx.all_masks(F)
    em = mx.expect_many([m.orc for m in ens.members], ens.qvals, masks, False)
    mlogp, mplanes, mtotals = engine.marginals_many(gpus, ens.qvals, masks,
                                                    members=True)
    assert same_bits(mplanes, em["w"]), what
    assert same_bits(mlogp, em["logp"]), what
    assert [word(t) for t in mtotals] == [word(t) for t in em["prior_totals"]]
    # predict_feature_many, every feature as the target
    for target in range(F):
        osh = ens.members[0].osh[target]
        fens = fm.FeatureEnsemble(ens, target, fe.candidates_for(osh),
                                  fe.random_masks(ens.nq, F, 11))
        fx_ = fens.expect()
        for mode, ck, mk in (("sample", "choice_draw", "member_draw"),
                             ("map", "choice_map", "member_map")):
            joint, base, choice, mem, pj, pb, tot = \
                engine.predict_feature_many(
                    gpus, ens.qvals, target, fens.cand, fens.observed, mode,
                    seed=fm.DRAW_SEED, draw_base=fm.DRAW_BASE, members=True)
            assert same_bits(pj, fx_["wj"]) and same_bits(pb, fx_["wb"]), \
                (what, target)
            assert same_bits(joint, fx_["joint"]), (what, target)
            assert same_bits(base, fx_["base"]), (what, target)
            assert np.array_equal(choice, fx_[ck]), (what, target)
            assert np.array_equal(mem, fx_[mk]), (what, target)
    # sample_rows_many
    n = 96
    q = [v[:n] for v in ens.qvals]
    cells = wrong = 0
    for tag, observed in (("masks", fe.random_masks(n, F, 23)),
                          ("none", None)):
        want = expect(ens, observed, n, qvals=q)
        got = host(gpus, ens, observed, n, qvals=q)
        c, w = check_against(ens, got, want, (what, tag))
        cells, wrong = cells + c, wrong + w
    print("%s: %d cells of GP compared with the host entry, %d differ"
          % (what, cells, wrong))
    assert wrong * 100000 <= cells


def test_an_ensemble_with_one_member_switched():
    from distributions_amd import engine
    ens = ee.Ensemble("dd_bb_gp", ee.SPECS3)
    gpus = ens.engines()
    before = [snapshot(g) for g in gpus]
    new, clustering = sx.SWITCHES["dd_bb_gp_swept"]
    # (every _many reader once under the constructors' values: member 0's
    # scratch then holds those)
    check_ensemble(ens, gpus, "unswitched")
    for which in (0, 1):
        pairs = new()
        sw_ens = sx.switched_ensemble(ens, which, pairs, clustering)
        sx.install(gpus[which], [p[1] for p in pairs], clustering)
        sw_ens.members[which].check_installed(gpus[which])
        check_ensemble(sw_ens, gpus, "member %d switched" % which)
        m = ens.members[which]
        sx.install(gpus[which], m.gsh, (m.alpha, m.d))
    check_ensemble(ens, gpus, "restored")
    for b, g in zip(before, gpus):
        assert same(b, snapshot(g))
        assert g.validate()["code"] == 0
    assert engine.predict_many(gpus, ens.qvals, None)[0].shape == (ens.nq,)


# ---------------------------------------------------------------------------
# e. two value-partitioned ranks on one GPU (tests/test_gpu_predict.py's
# worker, with the switch between the sweep and the queries)

RANK_ALPHAS = [0.05 + 0.3 * i for i in range(DIM)]
RANK_CLUSTERING = (2.5, 0.45)


def worker(rank, world, port, out):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("DIST_COMM_TIMEOUT_S", "120")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from distributions_amd import _core, engine
    from test_gpu_native_ranks import K, SEED, place
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    osh, gsh, vals, assign, bounds = place("dd", N, world, "value", DIM, K)
    lo, hi = bounds[rank]
    cols = [torch.from_numpy(ol.value_words(s.kind, v[lo:hi]).view(np.int32)
                             .copy()).to(dev) for s, v in zip(osh, vals)]
    packed = torch.from_numpy(assign[lo:hi].view(np.int32).copy()).to(dev)
    gpu = engine.Gibbs(1.0, 0.2, gsh)
    gpu.set_option("value_sorted", 2)
    gpu.set_option("device_normalise", 1)
    gpu.load_rows_torch(cols, packed.clone(), K, 2, row_offset=lo)
    sharded = engine.ShardedGibbs(gpu.core, hi - lo, lo, device=dev,
                                  columns=cols, assign_packed=packed)
    sharded.sync_initial_stats()
    assert sharded.use_native_comm()
    sharded.partition_by_value()
    sharded.sweep(PER, _core.rng_seed(SEED), draw_base=0)
    sharded.set_shared(0, sx.dd(RANK_ALPHAS)[1])
    sharded.set_clustering(*RANK_CLUSTERING)
    q = rank_queries(rank)
    logp, draw, total = sharded.predict(q, "sample",
                                        _core.rng_seed(pe.DRAW_SEED), 17)
    _, first, _ = sharded.predict(q, "map")
    np.save(os.path.join(out, "logp_%d.npy" % rank), logp)
    np.save(os.path.join(out, "draw_%d.npy" % rank), draw)
    np.save(os.path.join(out, "map_%d.npy" % rank), first)
    np.save(os.path.join(out, "alphas_%d.npy" % rank),
            np.array(gpu.core.shared(0).alphas, np.float32))
    dist.destroy_process_group()


def test_value_partitioned_ranks_switch_alike_and_predict(tmp_path):
    import torch.multiprocessing as mp
    from test_gpu_native_ranks import K, SEED, free_port, place
    mp.spawn(worker, args=(WORLD, free_port(), str(tmp_path)), nprocs=WORLD,
             join=True)
    osh, gsh, vals, assign, bounds = place("dd", N, WORLD, "value", DIM, K)
    m = ol.OracleMixture(1.0, 0.2, osh)
    m.init_from_assignments(vals, assign, K, 2)
    L = ol.oracle()
    ol._phase_sigs(L)
    st = L.orc_rng_seed(SEED)
    longest = max(hi - lo for lo, hi in bounds)
    for b in range(0, longest, PER):   # one pass, the ranks' composition
        snap = m.counts().copy()
        moves = []
        for lo, hi in bounds:
            r0, r1 = min(hi, lo + b), min(hi, lo + b + PER)
            old = np.zeros(r1 - r0 + 1, np.uint32)
            new = np.zeros(r1 - r0 + 1, np.uint32)
            L.orc_mix_batch_sample(m.h, r0, r1, m._vals, m.assign, st, 0, 0,
                                   old, new)
            moves.append((r0, r1, old, new))
        for r0, r1, old, new in moves:
            L.orc_mix_apply_moves(m.h, r0, r1, m._vals, m.assign, old, new)
        L.orc_mix_batch_finish(m.h, np.ascontiguousarray(snap, np.int32))
    after = ol.OracleMixture(RANK_CLUSTERING[0], RANK_CLUSTERING[1],
                             [sx.dd(RANK_ALPHAS)[0]])
    after.adopt(m, vals)
    for r in range(WORLD):
        np.testing.assert_array_equal(
            np.load(tmp_path / ("alphas_%d.npy" % r)),
            np.array(RANK_ALPHAS, np.float32))
        e = pe.expect(after, rank_queries(r), L.orc_rng_seed(pe.DRAW_SEED), 17)
        stale = pe.expect(m, rank_queries(r), L.orc_rng_seed(pe.DRAW_SEED), 17)
        assert not np.array_equal(bits(e["logp"]), bits(stale["logp"]))
        assert np.array_equal(bits(np.load(tmp_path / ("logp_%d.npy" % r))),
                              bits(e["logp"])), r
        assert np.array_equal(np.load(tmp_path / ("draw_%d.npy" % r)),
                              e["draw"]), r
        assert np.array_equal(np.load(tmp_path / ("map_%d.npy" % r)),
                              e["map"]), r


# ---------------------------------------------------------------------------
# f. the small-lgamma table turns over


def lgamma_lut_cap():
    text = open(os.path.join(ROOT, "distributions_amd", "csrc",
                             "special.h")).read()
    return int(re.search(r"kLgammaLutCap\s*=\s*(\d+)", text).group(1))


CHURN_DIM, CHURN_CALLS, CHURN_GRID = 256, 48, 24


def churn_alphas(j):
    v = np.arange(CHURN_DIM)
    return (0.001 + (CHURN_DIM * j + v) * 1e-5).astype(np.float32)


def check_score_data(gpu, orc, osh, alpha, d, what):
    """score_data() as tests/test_gpu_hypers.py holds it: the features' bit
    for bit (DPD: 1e-5), the clustering model's to 1e-6"""
    got, got_c = gpu.score_data()
    want = np.array([orc.L.orc_mix_slave_score_data(orc.h, f)
                     for f in range(len(osh))], np.float32)
    for f, sh in enumerate(osh):
        assert_scores(sh.kind, got[f:f + 1], want[f:f + 1],
                      "%s score_data feature %d" % (what, f))
    counts = np.ascontiguousarray(gpu.counts(), np.int32)
    want_c = orc.L.orc_py_score_counts(alpha, d, counts, counts.size)
    assert abs(got_c - want_c) <= 1e-6 * (1 + abs(want_c)), (what, got_c,
                                                             want_c)
    return got


def test_the_small_lgamma_table_turns_over():
    from distributions_amd import engine
    cap = lgamma_lut_cap()
    args = np.concatenate([churn_alphas(j)[:, None]
                           + np.arange(3, dtype=np.float32)[None, :]
                           for j in range(CHURN_CALLS)]).ravel()
    assert args.dtype == np.float32 and args.max() < 2.5 and args.min() > 0
    per_call = 3 * CHURN_DIM
    assert len(np.unique(args)) == CHURN_CALLS * per_call > 2 * cap
    assert CHURN_GRID * per_call > cap
    # 1. engine A holds arguments below 2.5 (gp_lut, nu below 1/16)
    sw_a = sx.switched("gp_nich_swept")
    a = sw_a.engine("set")
    check_predict(sw_a, a)
    data_a = check_score_data(a, sw_a.orc, sw_a.osh, sw_a.alpha, sw_a.d, "A")
    # 2. engine B: DD-256, 512 rows, K = 5
    osh, gsh, vals, assign = workloads.make("dd", 512, 4, dim=CHURN_DIM)
    b = engine.Gibbs(1.0, 0.2, gsh)
    b.load_rows(vals, assign, 4, 1)
    assert len(b) == 5
    # 3., 4. 48 installs, each of 768 new arguments
    for j in range(CHURN_CALLS):
        pair = sx.dd(churn_alphas(j))
        b.set_shared(0, pair[1])
        if j + 1 in (22, 44, 48):
            what = "after %d installs" % (j + 1)
            check_predict(sw_a, a, excursion=False)
            again = check_score_data(a, sw_a.orc, sw_a.osh, sw_a.alpha,
                                     sw_a.d, "A " + what)
            assert np.array_equal(bits(again), bits(data_a)), what
            orc_b = ol.OracleMixture(1.0, 0.2, [pair[0]])
            orc_b.adopt(b, vals)
            check_score_data(b, orc_b, [pair[0]], 1.0, float(np.float32(0.2)),
                             "B " + what)
    # 5. an engine built after the churn
    sw_c = sx.Switched(fe.case("bnb"), [sx.bnb(0.6, 2.0, 5)], None)
    c = sw_c.engine("set")
    check_predict(sw_c, c)
    # 6. a grid that holds more arguments than the table has room for
    cands = [sx.dd(churn_alphas(j)) for j in range(CHURN_GRID)]
    want = oracle_grid(orc_b, 0, cands)
    got = b.score_data_grid(0, [p[1] for p in cands])
    assert_scores(ol.DD, got, want, "the over-full grid")
    check_predict(sw_a, a, excursion=False)
    assert np.array_equal(bits(a.score_data()[0]), bits(data_a))
    b.validate()
