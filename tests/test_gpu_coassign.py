"""dist_gibbs_coassign[_many] and dist_gibbs_responsibilities
(k_coassign_resp, k_coassign_gemm): the co-assignment of pairs of held-out
rows over M engines, bit for bit against the expectation
tests/coassign_expect.py composes from the oracle and libm's fmaf (and
tests/test_coassign_oracle.py holds to float64).

Shapes: 70 x 45 rectangular with targets that are not the queries (a row /
column swap shows), 70 x 70 with the targets the queries, n = 1 and 33,
K = 3, 19 and 1025 (odd: k is padded), M = 3 with K = 5, 20, 43; 300 rows
(three tiles a side, the mirrored ones among them) against the expectation
at the tiles' edges and against calls on its blocks; debug.predict_chunk = 33;
the single form against the m = 1 _many form; the device-tensor forms; a
planted-cluster state whose cells run from near 0 to near 1; the reader
rules.  Cells in (0, 2^-100) pass with got < 2^-99, at most 1 % of a case."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import coassign_expect as ce  # noqa: E402
import oracle_lib as ol  # noqa: E402
import predict_expect as pe  # noqa: E402

pytestmark = pytest.mark.gpu

_GPUS = {}


def engines_of(name):
    """one set of engines per subject, shared: the calls leave them as they
    were"""
    if name not in _GPUS:
        _GPUS[name] = ce.subject(name).engines()
    return _GPUS[name]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_cells(got, want, mask, what):
    assert got.shape == want.shape, what
    ok, share = ce.same_cells(got, want, mask)
    if not ok:
        bad = np.argwhere(mask & (bits(got) != bits(want)))
        a, b = bad[0]
        raise AssertionError("%s: %d cells differ, the first at (%d, %d): "
                             "got %r, expected %r"
                             % (what, len(bad), a, b, got[a, b], want[a, b]))
    assert share <= ce.UNDERFLOW_SHARE, (what, share)


def call(gpus, values, other=None):
    """the single form for one engine, the _many form otherwise"""
    from distributions_amd import engine
    if len(gpus) == 1:
        return gpus[0].coassign(values, other)
    return engine.coassign_many(gpus, values, other)


@pytest.mark.parametrize("name", ce.NAMES)
def test_coassign_is_the_expectation_bit_for_bit(name):
    from distributions_amd import engine
    sub = ce.subject(name)
    gpus = engines_of(name)
    q, t = sub.cols(sub.rq), sub.cols(sub.rt)
    rect = call(gpus, q, t)
    assert_cells(rect, sub.expect(False), sub.mask(False), name + " 70 x 45")
    sym = call(gpus, q)
    assert_cells(sym, sub.expect(True), sub.mask(True), name + " 70 x 70")
    assert np.array_equal(bits(sym), bits(sym.T))
    same = call(gpus, q, q)
    m = sub.mask(True)
    assert np.array_equal(bits(same)[m], bits(sym)[m])
    # the _many form at m = 1 is the single form; the single form's rows
    many = engine.coassign_many(gpus, q, t)
    assert np.array_equal(bits(many)[sub.mask(False)],
                          bits(rect)[sub.mask(False)])
    # the float64 law, within its band
    C, band = sub.law(False)
    mask = sub.mask(False)
    assert (np.abs(rect.astype(np.float64) - C)[mask] <= band[mask]).all()


@pytest.mark.parametrize("name", ce.NAMES)
def test_responsibilities_are_the_expectations_r(name):
    sub = ce.subject(name)
    rows = np.concatenate([sub.rq, sub.rt])
    ok = sub.specified(rows)
    for gpu, want in zip(engines_of(name), sub.r()):
        got = gpu.responsibilities(sub.cols(rows))
        assert got.shape == want.shape == (len(rows), len(gpu))
        assert np.array_equal(bits(got)[ok], bits(want)[ok])
        assert (got[ok] >= 0).all()


@pytest.mark.parametrize("name", ["dd", "ens3_gp_nich"])
@pytest.mark.parametrize("n", [1, 33])
def test_small_row_counts(name, n):
    sub = ce.subject(name)
    gpus = engines_of(name)
    q = sub.cols(sub.rq[:n])
    got = call(gpus, q)
    assert_cells(got, sub.expect(True)[:n, :n], sub.mask(True)[:n, :n],
                 "%s n = %d" % (name, n))
    got = call(gpus, q, sub.cols(sub.rt))
    assert_cells(got, sub.expect(False)[:n], sub.mask(False)[:n],
                 "%s %d x 45" % (name, n))


@pytest.mark.parametrize("name", ["dd", "ens3_dd_bb_gp"])
def test_chunked_launches_give_the_same_bits(name):
    sub = ce.subject(name)
    gpus = engines_of(name)
    q, t = sub.cols(sub.rq), sub.cols(sub.rt)
    rect, sym = call(gpus, q, t), call(gpus, q)
    resp = gpus[0].responsibilities(q)
    gpus[0].set_option("debug.predict_chunk", 33)
    try:
        rect33, sym33 = call(gpus, q, t), call(gpus, q)
        resp33 = gpus[0].responsibilities(q)
    finally:
        gpus[0].set_option("debug.predict_chunk", 1 << 22)
    assert np.array_equal(bits(rect33), bits(rect))
    assert np.array_equal(bits(sym33), bits(sym))
    assert np.array_equal(bits(sym33), bits(sym33.T))
    assert np.array_equal(bits(resp33), bits(resp))
    # blocks of more than one tile, those left of the diagonal written as
    # the mirrors of their twins
    rows = sub.cols(np.arange(300))
    whole = call(gpus, rows)
    gpus[0].set_option("debug.predict_chunk", 130)
    try:
        whole130 = call(gpus, rows)
    finally:
        gpus[0].set_option("debug.predict_chunk", 1 << 22)
    ok = sub.specified(np.arange(300))
    m = np.outer(ok, ok)
    assert np.array_equal(bits(whole130)[m], bits(whole)[m])
    assert np.array_equal(bits(whole130), bits(whole130.T))


@pytest.mark.parametrize("name", ["dd", "ens3_dd_bb_gp"])
def test_three_tiles_a_side(name):
    """300 rows: tiles (i, j) for i, j in 0..2, those below the diagonal
    mirrored.  The expectation at the rows around the tiles' edges, and every
    100-row block against the call on those rows alone (which runs in tile
    (0, 0), held to the expectation above)."""
    sub = ce.subject(name)
    gpus = engines_of(name)
    n = 300
    rows = np.arange(n)
    ok = sub.specified(rows)
    whole = call(gpus, sub.cols(rows))
    assert whole.shape == (n, n)
    assert np.array_equal(bits(whole), bits(whole.T))
    edge = np.array([0, 31, 32, 63, 64, 127, 128, 129, 191, 192, 255, 256,
                     257, 299])
    r = [ce.responsibilities(s[edge]) for s in sub.scores()]
    want = ce.chain(r, r, True)
    assert_cells(whole[np.ix_(edge, edge)], want, np.outer(ok[edge], ok[edge]),
                 name + " tile edges")
    for a in range(0, n, 100):
        for b in range(0, n, 100):
            ra, rb = rows[a:a + 100], rows[b:b + 100]
            block = call(gpus, sub.cols(ra), sub.cols(rb))
            m = np.outer(ok[ra], ok[rb])
            assert np.array_equal(bits(block)[m],
                                  bits(whole[a:a + 100, b:b + 100])[m]), (a, b)
    # a rectangular call of more than one tile each way
    rect = call(gpus, sub.cols(rows[:130]), sub.cols(rows[40:300]))
    m = np.outer(ok[:130], ok[40:300])
    assert np.array_equal(bits(rect)[m], bits(whole[:130, 40:300])[m])


def test_torch_forms_equal_the_host_forms():
    import torch
    from distributions_amd import engine
    for name in ("gp_nich", "ens3_dd_bb_gp"):
        sub = ce.subject(name)
        gpus = engines_of(name)
        q, t = sub.cols(sub.rq), sub.cols(sub.rt)

        def dev(cols):
            return [torch.from_numpy(
                np.ascontiguousarray(c).view(np.int32).copy()).cuda()
                for c in cols]
        words = pe.query_words(sub.members[0].orc, q)
        wq = dev(words)
        wt = dev(pe.query_words(sub.members[0].orc, t))
        rect = engine.coassign_many_torch(gpus, wq, wt)
        assert rect.is_cuda and tuple(rect.shape) == (70, 45)
        assert np.array_equal(bits(rect.cpu().numpy()), bits(call(gpus, q, t)))
        sym = engine.coassign_many_torch(gpus, wq)
        assert np.array_equal(bits(sym.cpu().numpy()), bits(call(gpus, q)))
        if len(gpus) == 1:
            one = gpus[0].coassign_torch(wq, wt)
            assert np.array_equal(bits(one.cpu().numpy()),
                                  bits(rect.cpu().numpy()))
        # columns the library could not read are refused before any launch
        with pytest.raises(RuntimeError, match="one value column per feature"):
            engine.coassign_many_torch(gpus, wq[:-1] if len(wq) > 1 else [])
        with pytest.raises(RuntimeError, match="one value column per feature"):
            engine.coassign_many_torch(gpus, wq, wt + wt[:1])
        with pytest.raises(RuntimeError, match="4 bytes per row"):
            engine.coassign_many_torch(gpus, [wq[0].long()] + wq[1:])
        with pytest.raises(RuntimeError, match="one CUDA device"):
            engine.coassign_many_torch(gpus, [wq[0].cpu()] + wq[1:])
        with pytest.raises(RuntimeError, match="one CUDA device"):
            gpus[0].responsibilities_torch([c.cpu() for c in wq])
        resp = gpus[0].responsibilities_torch(wq)
        assert resp.is_cuda and tuple(resp.shape) == (70, len(gpus[0]))
        assert np.array_equal(bits(resp.cpu().numpy()),
                              bits(gpus[0].responsibilities(q)))


def test_planted_clusters_run_from_near_0_to_near_1():
    """DirichletDiscrete of dim 16, every row's value its group, 16 groups
    and one empty: rows of one value share a group almost surely, rows of two
    values almost never"""
    from distributions_amd import engine
    dim, per = 16, 64
    assign = np.repeat(np.arange(dim), per).astype(np.uint32)
    values = assign.copy()
    alphas = [0.001] * dim
    gpu = engine.Gibbs(alpha=0.01, d=0.0, shareds=[engine.dd_shared(alphas)])
    gpu.load_rows([values], assign, nonempty_groups=dim, empty_groups=1)
    assert len(gpu) == 17
    orc = ol.OracleMixture(0.01, 0.0, [ol.make_shared(ol.DD, alphas=alphas)])
    orc.init_from_assignments([values], assign, dim, 1)
    q = [(np.arange(48) % dim).astype(np.uint32)]
    e = pe.expect(orc, q, ol.oracle().orc_rng_seed(1), 0)
    r = [ce.responsibilities(e["scores"])]
    want = ce.chain(r, r, True)
    mask = np.ones(want.shape, bool)
    soft = (want > 0) & (want < ce.UNDERFLOW)
    assert soft.sum() <= ce.UNDERFLOW_SHARE * want.size
    assert want.min() < 1e-3 and want.max() > 0.99
    assert_cells(gpu.coassign(q), want, mask, "planted clusters")
    assert np.array_equal(bits(gpu.responsibilities(q)), bits(r[0]))


# ---------------------------------------------------------------------------
# reader rules


def test_the_calls_change_nothing():
    from distributions_amd import engine
    sub = ce.subject("ens3_dd_bb_gp")
    gpus = sub.engines()                        # (their own)
    q = sub.cols(sub.rq)
    before = [(g.assignments().copy(), g.counts().copy(),
               g.predict(q, None)[0].copy()) for g in gpus]
    engine.coassign_many(gpus, q)
    engine.coassign_many(gpus, q, sub.cols(sub.rt))
    gpus[0].coassign(q)
    gpus[0].responsibilities(q)
    for g, (a, c, lp) in zip(gpus, before):
        assert np.array_equal(g.assignments(), a)
        assert np.array_equal(g.counts(), c)
        assert np.array_equal(bits(g.predict(q, None)[0]), bits(lp))


def test_an_open_batch_is_refused():
    from distributions_amd import engine
    sub = ce.subject("ens3_dd_bb_gp")
    gpus = sub.engines()                        # (their own: a state moves)
    q = sub.cols(sub.rq)
    gpus[1].core.batch_sample(0, 256, ol.oracle().orc_rng_seed(3), 0)
    with pytest.raises(RuntimeError, match="batch open"):
        engine.coassign_many(gpus, q)
    with pytest.raises(RuntimeError, match="batch open"):
        gpus[1].coassign(q)
    with pytest.raises(RuntimeError, match="batch open"):
        gpus[1].responsibilities(q)
    gpus[1].core.batch_apply_local()
    gpus[1].core.batch_finish()
    assert engine.coassign_many(gpus, q).shape == (70, 70)


def test_a_value_outside_its_domain_fails_and_names_the_row():
    from distributions_amd import engine
    sub = ce.subject("ens3_dd_bb_gp")
    gpus = engines_of("ens3_dd_bb_gp")
    q, t = sub.cols(sub.rq), sub.cols(sub.rt)
    bad = [c.copy() for c in q]
    bad[1][61] = 2
    bad[1][37] = 2                      # the first offending row is named
    bad[0][66] = 200                    # (a later row, an earlier feature)
    with pytest.raises(RuntimeError, match="row 37, feature 1"):
        engine.coassign_many(gpus, bad)
    with pytest.raises(RuntimeError, match="target row 37, feature 1"):
        engine.coassign_many(gpus, t, bad)
    with pytest.raises(RuntimeError, match="row 37, feature 1"):
        gpus[0].responsibilities(bad)
    # a DirichletDiscrete value beyond its dim, the first offending cell
    bad = [c.copy() for c in q]
    bad[0][52] = 200
    bad[1][60] = 2
    with pytest.raises(RuntimeError, match="row 52, feature 0"):
        engine.coassign_many(gpus, bad)
    with pytest.raises(RuntimeError, match="target row 52, feature 0"):
        gpus[0].coassign(t, bad)
    with pytest.raises(RuntimeError, match="row 52, feature 0"):
        gpus[0].responsibilities(bad)
    # process and engines go on
    assert_cells(engine.coassign_many(gpus, q, t), sub.expect(False),
                 sub.mask(False), "after the refusal")


def test_zero_rows_do_nothing():
    from distributions_amd import engine
    sub = ce.subject("dd")
    gpus = engines_of("dd")
    none = sub.cols(sub.rq[:0])
    q = sub.cols(sub.rq)
    assert engine.coassign_many(gpus, none).shape == (0, 0)
    assert gpus[0].coassign(none, q).shape == (0, 70)
    assert gpus[0].coassign(q, none).shape == (70, 0)
    assert gpus[0].responsibilities(none).shape == (0, len(gpus[0]))
    with pytest.raises(RuntimeError, match="the same engine twice"):
        engine.coassign_many([gpus[0], gpus[0]], q)
