"""dist_gibbs_coassign_topk[_many] (k_coassign_topk, k_coassign_topk_merge):
per query the k most co-assigned targets over M engines, index words and
probability bits exactly equal to tests/coassign_topk_expect.py's selection
from the expectation of tests/coassign_expect.py, and from coassign_many's own
matrix on the same engines.  Only rows with finite logp are passed (the others'
results are unspecified).

Shapes: 70 x 45 rectangular with k = 1, 5, 45 (the full sort of a row) and 64
(> n_t: the fill); 70 x 70 with the targets the queries, with and without
self; n = 1 and 33; three targets with k = 8; 300 rows (three tiles a side:
the rows' and the columns' selections and the merge of three lists) with
k = 7 and 128 under debug.predict_chunk = default, 130, 128 and 33; targets
repeated 140 and 280 columns away (ties across tile and chunk edges); the
forms; the rules."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import coassign_expect as ce  # noqa: E402
import coassign_topk_expect as ct  # noqa: E402
import oracle_lib as ol  # noqa: E402
import predict_expect as pe  # noqa: E402

pytestmark = pytest.mark.gpu

_GPUS = {}
DEFAULT_CHUNK = 1 << 22


def engines_of(name):
    """one set of engines per subject, shared: the calls leave them as they
    were"""
    if name not in _GPUS:
        _GPUS[name] = ce.subject(name).engines()
    return _GPUS[name]


def topk(gpus, values, other=None, k=10, exclude_self=None):
    """the single form for one engine, the _many form otherwise"""
    from distributions_amd import engine
    if len(gpus) == 1:
        return gpus[0].coassign_topk(values, other, k, exclude_self)
    return engine.coassign_topk_many(gpus, values, other, k, exclude_self)


def matrix(gpus, values, other=None):
    from distributions_amd import engine
    if len(gpus) == 1:
        return gpus[0].coassign(values, other)
    return engine.coassign_many(gpus, values, other)


def assert_same(got, want, what):
    """got: (int32 index, float32 prob) of the library; want: (uint32 index,
    float32 prob) of the expectation"""
    index, prob = got
    assert index.dtype == np.int32 and prob.dtype == np.float32, what
    assert index.shape == prob.shape == want[0].shape, what
    bad = np.argwhere((index.view(np.uint32) != want[0])
                      | (ct.bits(prob) != ct.bits(want[1])))
    if len(bad):
        a, j = bad[0]
        raise AssertionError(
            "%s: %d entries differ, the first at (%d, %d): got %d, %r, "
            "expected %d, %r" % (what, len(bad), a, j, index[a, j],
                                 prob[a, j], want[0].view(np.int32)[a, j],
                                 want[1][a, j]))


@pytest.mark.parametrize("name", ce.NAMES)
def test_topk_is_the_expectations_selection_bit_for_bit(name):
    case = ct.case(name)
    sub = case.sub
    gpus = engines_of(name)
    q, t = sub.cols(case.rq), sub.cols(case.rt)
    rect = case.expect(False)
    for k in (1, 5, 45, 64):
        assert_same(topk(gpus, q, t, k), ct.topk(rect, k),
                    "%s %d x %d, k = %d" % (name, len(case.rq), len(case.rt),
                                            k))
    sym = case.expect(True)
    with_self = topk(gpus, q, None, 5, False)
    assert_same(with_self, ct.topk(sym, 5, False), name + " with self")
    assert_same(topk(gpus, q, None, 5, True), ct.topk(sym, 5, True),
                name + " without self")
    assert_same(topk(gpus, q, k=5), ct.topk(sym, 5, True),
                name + " exclude_self=None")
    same = topk(gpus, q, q, 5)
    assert np.array_equal(same[0], with_self[0])
    assert np.array_equal(ct.bits(same[1]), ct.bits(with_self[1]))


@pytest.mark.parametrize("name", ["dd", "ens3_gp_nich"])
def test_small_shapes(name):
    case = ct.case(name)
    sub = case.sub
    gpus = engines_of(name)
    sym, rect = case.expect(True), case.expect(False)
    for n in (1, 33):
        q = sub.cols(case.rq[:n])
        assert_same(topk(gpus, q, None, 4, False),
                    ct.topk(sym[:n, :n], 4, False), "%s n = %d" % (name, n))
        assert_same(topk(gpus, q, None, 4, True),
                    ct.topk(sym[:n, :n], 4, True),
                    "%s n = %d without self" % (name, n))
        assert_same(topk(gpus, q, sub.cols(case.rt), 4),
                    ct.topk(rect[:n], 4), "%s %d x 45" % (name, n))
    index, prob = topk(gpus, sub.cols(case.rq[:1]), None, 3, True)
    assert (index == -1).all() and (ct.bits(prob) == 0).all()
    assert_same(topk(gpus, sub.cols(case.rq), sub.cols(case.rt[:3]), 8),
                ct.topk(rect[:, :3], 8), name + " three targets, k = 8")


@pytest.mark.parametrize("name", ["dd", "ens3_dd_bb_gp"])
def test_three_tiles_a_side_and_the_merge(name):
    sub = ce.subject(name)
    gpus = engines_of(name)
    rows = np.arange(300)
    rows = sub.cols(rows[sub.specified(rows)])
    n = len(rows[0])
    assert n > 256
    whole = matrix(gpus, rows)
    try:
        for k in (7, 128):
            want = ct.topk(whole, k, True)
            for chunk in (DEFAULT_CHUNK, 130, 128, 33):
                gpus[0].set_option("debug.predict_chunk", chunk)
                assert_same(topk(gpus, rows, None, k, True), want,
                            "%s 300 rows, k = %d, chunk %d" % (name, k, chunk))
        # with self, and a rectangular call of more than one tile each way
        gpus[0].set_option("debug.predict_chunk", 130)
        assert_same(topk(gpus, rows, None, 7, False), ct.topk(whole, 7, False),
                    name + " 300 rows with self")
        a, b = [c[:130] for c in rows], [c[40:] for c in rows]
        assert_same(topk(gpus, a, b, 7), ct.topk(whole[:130, 40:], 7),
                    name + " 130 x 260")
    finally:
        gpus[0].set_option("debug.predict_chunk", DEFAULT_CHUNK)


def test_ties_across_tile_and_chunk_edges():
    sub = ce.subject("gp_nich")
    gpus = engines_of("gp_nich")
    rows = np.arange(300)
    rows = rows[sub.specified(rows)][:140]
    assert len(rows) == 140
    t = sub.cols(np.concatenate([rows, rows, rows[:20]]))
    q = sub.cols(rows[:70])
    whole = matrix(gpus, q, t)
    want = ct.topk(whole, 6)
    # every target's duplicates tie with it bit for bit; the lower index first
    assert np.array_equal(ct.bits(whole[:, :140]), ct.bits(whole[:, 140:280]))
    assert (want[0][:, 1] == want[0][:, 0] + 140).all()
    try:
        for chunk in (DEFAULT_CHUNK, 128):
            gpus[0].set_option("debug.predict_chunk", chunk)
            assert_same(topk(gpus, q, t, 6), want, "ties, chunk %d" % chunk)
    finally:
        gpus[0].set_option("debug.predict_chunk", DEFAULT_CHUNK)


def test_the_forms_agree():
    import torch
    from distributions_amd import engine
    for name in ("gp_nich", "ens3_dd_bb_gp"):
        case = ct.case(name)
        sub = case.sub
        gpus = engines_of(name)
        q, t = sub.cols(case.rq), sub.cols(case.rt)

        def dev(cols):
            return [torch.from_numpy(
                np.ascontiguousarray(c).view(np.int32).copy()).cuda()
                for c in pe.query_words(sub.members[0].orc, cols)]
        wq, wt = dev(q), dev(t)
        for other, wo, flag in ((t, wt, None), (None, None, None),
                                (None, None, False)):
            host = engine.coassign_topk_many(gpus, q, other, 5, flag)
            assert host[0].dtype == np.int32 and host[0].shape == (len(q[0]), 5)
            index, prob = engine.coassign_topk_many_torch(gpus, wq, wo, 5,
                                                          flag)
            assert index.is_cuda and index.dtype == torch.int32
            assert prob.is_cuda and prob.dtype == torch.float32
            assert np.array_equal(index.cpu().numpy(), host[0])
            assert np.array_equal(ct.bits(prob.cpu().numpy()),
                                  ct.bits(host[1]))
            if len(gpus) == 1:
                one = gpus[0].coassign_topk(q, other, 5, flag)
                assert np.array_equal(one[0], host[0])
                assert np.array_equal(ct.bits(one[1]), ct.bits(host[1]))
                index, prob = gpus[0].coassign_topk_torch(wq, wo, 5, flag)
                assert np.array_equal(index.cpu().numpy(), host[0])
                assert np.array_equal(ct.bits(prob.cpu().numpy()),
                                      ct.bits(host[1]))
        # the fill is -1 and +0
        index, prob = engine.coassign_topk_many(gpus, q, [c[:2] for c in t], 4)
        assert (index[:, 2:] == -1).all() and (index[:, :2] >= 0).all()
        assert (ct.bits(prob[:, 2:]) == 0).all()
        with pytest.raises(RuntimeError, match="one value column per feature"):
            engine.coassign_topk_many_torch(gpus, wq[:-1] if len(wq) > 1
                                            else [])
        with pytest.raises(RuntimeError, match="one CUDA device"):
            engine.coassign_topk_many_torch(gpus, [wq[0].cpu()] + wq[1:])


# ---------------------------------------------------------------------------
# rules


def test_limits_and_flags():
    from distributions_amd import _core, engine
    case = ct.case("ens3_dd_bb_gp")
    sub = case.sub
    gpus = engines_of("ens3_dd_bb_gp")
    cores = [g.core for g in gpus]
    q, t = sub.cols(case.rq), sub.cols(case.rt)
    assert engine.coassign_topk_many(gpus, q, t, 128)[0].shape == (70, 128)
    with pytest.raises(RuntimeError, match="k is at most 128"):
        engine.coassign_topk_many(gpus, q, t, 129)
    with pytest.raises(RuntimeError, match="ld is less than k"):
        _core.coassign_topk_many(cores, q, t, 5, 0, False, 4)
    got = _core.coassign_topk_many(cores, q, t, 5, 0, False, 9)
    assert_same((got[0].view(np.int32), got[1]),
                ct.topk(case.expect(False), 5), "ld = 9")
    with pytest.raises(RuntimeError, match="EXCLUDE_SELF"):
        engine.coassign_topk_many(gpus, q, t, 5, True)
    with pytest.raises(RuntimeError, match="EXCLUDE_SELF"):
        gpus[0].coassign_topk(q, q, 5, True)
    with pytest.raises(RuntimeError, match="unknown flag"):
        _core.coassign_topk_many(cores, q, None, 5, 2)
    with pytest.raises(RuntimeError, match="the same engine twice"):
        engine.coassign_topk_many([gpus[0], gpus[0]], q)
    # nothing to do
    none = sub.cols(case.rq[:0])
    assert engine.coassign_topk_many(gpus, none)[0].shape == (0, 10)
    assert engine.coassign_topk_many(gpus, q, k=0)[1].shape == (70, 0)
    index, prob = engine.coassign_topk_many(gpus, q, none, 3)
    assert index.shape == (70, 3)


def test_a_value_outside_its_domain_fails_and_names_the_row():
    from distributions_amd import engine
    case = ct.case("ens3_dd_bb_gp")
    sub = case.sub
    gpus = engines_of("ens3_dd_bb_gp")
    q, t = sub.cols(case.rq), sub.cols(case.rt)
    bad = [c.copy() for c in q]
    bad[1][61] = 2
    bad[1][37] = 2                      # the first offending row is named
    bad[0][66] = 200                    # (a later row, an earlier feature)
    with pytest.raises(RuntimeError, match="row 37, feature 1"):
        engine.coassign_topk_many(gpus, bad)
    with pytest.raises(RuntimeError, match="target row 37, feature 1"):
        engine.coassign_topk_many(gpus, t, bad)
    with pytest.raises(RuntimeError, match="target row 37, feature 1"):
        gpus[0].coassign_topk(t, bad)
    # process and engines go on
    assert_same(engine.coassign_topk_many(gpus, q, t, 5),
                ct.topk(case.expect(False), 5), "after the refusal")


def test_an_open_batch_is_refused():
    from distributions_amd import engine
    sub = ce.subject("ens3_dd_bb_gp")
    gpus = sub.engines()                        # (their own: a state moves)
    q = sub.cols(sub.rq)
    gpus[1].core.batch_sample(0, 256, ol.oracle().orc_rng_seed(3), 0)
    with pytest.raises(RuntimeError, match="batch open"):
        engine.coassign_topk_many(gpus, q)
    with pytest.raises(RuntimeError, match="batch open"):
        gpus[1].coassign_topk(q)
    gpus[1].core.batch_apply_local()
    gpus[1].core.batch_finish()
    assert engine.coassign_topk_many(gpus, q)[0].shape == (70, 10)


def test_the_calls_change_nothing_and_a_sweep_goes_on_as_its_twins():
    from distributions_amd import engine
    sub = ce.subject("ens3_dd_bb_gp")
    gpus, twins = sub.engines(), sub.engines()
    q, t = sub.cols(sub.rq), sub.cols(sub.rt)
    before = [(g.assignments().copy(), g.counts().copy()) for g in gpus]
    engine.coassign_topk_many(gpus, q)
    engine.coassign_topk_many(gpus, q, t, 64)
    gpus[0].coassign_topk(q, k=3)
    for g, (a, c) in zip(gpus, before):
        assert np.array_equal(g.assignments(), a)
        assert np.array_equal(g.counts(), c)
    for g, twin in zip(gpus, twins):
        n = len(g.assignments())
        g.sweep(0, n, 500, 11)
        twin.sweep(0, n, 500, 11)
        # (a run the sweep left open stays resumable under the call)
        engine.coassign_topk_many([g], q, k=3)
        assert np.array_equal(g.assignments(), twin.assignments())
        assert np.array_equal(g.counts(), twin.counts())
        g.validate()
