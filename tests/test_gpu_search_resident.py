"""dist_gibbs_search_resident[_many] and
dist_gibbs_coassign_resident_topk[_many] (k_resident_topk): per
query the k most co-assigned RESIDENT rows over M engines.  Index words and
probability bits exactly equal to tests/search_resident_expect.py's selection
from its cells, and for resident queries to the selection from
coassign_resident_many's own matrix.  Only queries with finite logp are passed
(the others' results are unspecified).

Shapes: every subject with k = 1, 5, 64, 128; ranges of 3, 1 and 0 rows;
eight planted-table chains of 2 000 rows with 300 resident queries; 66 engines
of 64 rows; debug.predict_chunk = default, 130, 128 and 33 (several slices,
tile edges, query chunks, the merge of up to 61 lists; resident cells are all
ties); ranges strictly inside the table; the forms; the refusals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle_lib as ol  # noqa: E402
import predict_expect as pe  # noqa: E402
import search_resident_expect as se  # noqa: E402
import workloads  # noqa: E402

pytestmark = pytest.mark.gpu

_GPUS = {}
DEFAULT_CHUNK = 1 << 22
CHUNKS = (DEFAULT_CHUNK, 130, 128, 33)


def engines_of(name):
    """one set of engines per subject, shared: the calls leave them as they
    were"""
    if name not in _GPUS:
        _GPUS[name] = se.case(name).sub.engines()
    return _GPUS[name]


def search(gpus, values, k=10, row_begin=0, row_end=None):
    """the single form for one engine, the _many form otherwise"""
    from distributions_amd import engine
    if len(gpus) == 1:
        return gpus[0].search_resident(values, k, row_begin, row_end)
    return engine.search_resident_many(gpus, values, k, row_begin, row_end)


def resident(gpus, rows, k=10, exclude_self=True, row_begin=0, row_end=None):
    from distributions_amd import engine
    if len(gpus) == 1:
        return gpus[0].coassign_resident_topk(rows, k, exclude_self,
                                              row_begin, row_end)
    return engine.coassign_resident_topk_many(gpus, rows, k, exclude_self,
                                              row_begin, row_end)


def assert_same(got, want, what):
    """got: (int32 index, float32 prob) of the library; want: (uint32 index,
    float32 prob) of the expectation"""
    index, prob = got
    assert index.dtype == np.int32 and prob.dtype == np.float32, what
    assert index.shape == prob.shape == want[0].shape, what
    bad = np.argwhere((index.view(np.uint32) != want[0])
                      | (se.bits(prob) != se.bits(want[1])))
    if len(bad):
        a, j = bad[0]
        raise AssertionError(
            "%s: %d entries differ, the first at (%d, %d): got %d, %r, "
            "expected %d, %r" % (what, len(bad), a, j, index[a, j],
                                 prob[a, j], want[0].view(np.int32)[a, j],
                                 want[1][a, j]))


def query_rows(n):
    rows = np.random.default_rng(5).integers(0, n, 40)
    rows[1] = rows[0]
    rows[2] = n - 1
    rows[3] = 0
    return rows


@pytest.mark.parametrize("name", se.NAMES)
def test_both_kinds_are_the_expectations_selection_bit_for_bit(name):
    c = se.case(name)
    gpus = engines_of(name)
    q = c.cols()
    cells = c.cells()
    rows = query_rows(c.n)
    res = se.resident_cells(c.assigns, rows)
    for k in (1, 5, 64, 128):
        assert_same(search(gpus, q, k), se.topk(cells, k),
                    "%s held-out, k = %d" % (name, k))
        assert_same(resident(gpus, rows, k), se.topk(res, k, 0, None, rows),
                    "%s resident, k = %d" % (name, k))
    assert_same(resident(gpus, rows, 5, False), se.topk(res, 5),
                name + " resident with self")
    # a range strictly inside the table
    lo, hi = 5, c.n - 3
    assert_same(search(gpus, q, 5, lo, hi), se.topk(cells, 5, lo, hi),
                name + " held-out, rows 5 .. n - 3")
    assert_same(resident(gpus, rows, 5, True, lo, hi),
                se.topk(res, 5, lo, hi, rows), name + " resident, inside")


@pytest.mark.parametrize("name", ["dd", "ens3_gp_nich"])
def test_the_fill(name):
    c = se.case(name)
    gpus = engines_of(name)
    q, cells = c.cols(), c.cells()
    rows = query_rows(c.n)
    rows[4:7] = (4, 5, 9)
    res = se.resident_cells(c.assigns, rows)
    for lo, hi, live in ((4, 7, 3), (9, 10, 1), (6, 6, 0), (c.n, c.n, 0)):
        got = search(gpus, q, 8, lo, hi)
        assert_same(got, se.topk(cells, 8, lo, hi), "%s %d .. %d" % (name, lo,
                                                                    hi))
        assert (got[0][:, live:] == -1).all()
        assert (se.bits(got[1][:, live:]) == 0).all()
        assert (got[0][:, :live] >= lo).all()
        for exclude in (False, True):
            assert_same(resident(gpus, rows, 8, exclude, lo, hi),
                        se.topk(res, 8, lo, hi, rows if exclude else None),
                        "%s resident %d .. %d, exclude %r" % (name, lo, hi,
                                                              exclude))


@pytest.mark.parametrize("name", ["dd", "ens3_dd_bb_gp"])
def test_slices_tile_edges_query_chunks_and_the_merge(name):
    """(the table's rows share groups: every kind's cells tie across the
    slices' edges)"""
    c = se.case(name)
    gpus = engines_of(name)
    q, cells = c.cols(), c.cells()
    rows = np.concatenate([query_rows(c.n), np.arange(0, c.n, 7)[:60]])
    res = se.resident_cells(c.assigns, rows)
    assert len(q[0]) > 33 and len(rows) > 66
    tied = se.bits(se.topk(cells, 128)[1])
    assert (tied[:, :-1] == tied[:, 1:]).any()
    try:
        for k in (7, 128):
            want = se.topk(cells, k)
            want_r = se.topk(res, k, 0, None, rows)
            for chunk in CHUNKS:
                gpus[0].set_option("debug.predict_chunk", chunk)
                assert_same(search(gpus, q, k), want,
                            "%s held-out k = %d, chunk %d" % (name, k, chunk))
                assert_same(resident(gpus, rows, k), want_r,
                            "%s resident k = %d, chunk %d" % (name, k, chunk))
        gpus[0].set_option("debug.predict_chunk", 130)
        assert_same(search(gpus, q, 7, 100, 391),
                    se.topk(cells, 7, 100, 391), name + " rows 100 .. 391")
        assert_same(resident(gpus, rows, 7, False, 100, 391),
                    se.topk(res, 7, 100, 391), name + " resident 100 .. 391")
    finally:
        gpus[0].set_option("debug.predict_chunk", DEFAULT_CHUNK)


# ---------------------------------------------------------------------------
# resident queries against coassign_resident_many's own matrix


@pytest.fixture(scope="module")
def chains():
    """tests/test_gpu_partitions.py's recipe: eight engines on one planted
    table, different starts and seeds, three exact sweeps each -> (engines,
    their assignments)"""
    from distributions_amd import _core, engine
    n, k, m = 2000, 16, 8
    _, _, gsh, vals = workloads.planted(n, k)
    gpus = []
    for i in range(m):
        start = np.random.default_rng(100 + i).permutation(n) % (k + i)
        g = engine.Gibbs(1.0, 0.1, gsh)
        g.load_rows(vals, start.astype(np.uint32), k + i, 1)
        gpus.append(g)
    states = np.array([_core.rng_seed(900 + i) for i in range(m)], np.uint32)
    for _ in range(3):
        states = engine.sweep_sequential_many(gpus, 0, n, states)
    return gpus, [g.assignments() for g in gpus]


def test_eight_chains_against_the_dense_matrix(chains):
    import torch
    from distributions_amd import engine
    gpus, assign = chains
    n = assign[0].size
    assert max(int(a.max()) for a in assign) >= max(len(g) for g in gpus)
    rows = np.random.default_rng(16).integers(0, n, 300)
    rows[7] = rows[3]
    rows[299] = n - 1
    dense = engine.coassign_resident_many(gpus, rows, np.arange(n))
    assert np.array_equal(se.bits(dense),
                          se.bits(se.resident_cells(assign, rows)))
    assert len(np.unique(dense)) > 4
    try:
        for chunk in CHUNKS:
            gpus[0].set_option("debug.predict_chunk", chunk)
            for k, exclude in ((16, True), (16, False), (128, True)):
                got = engine.coassign_resident_topk_many(gpus, rows, k,
                                                         exclude)
                assert_same(got, se.topk(dense, k, 0, None,
                                         rows if exclude else None),
                            "8 chains, k = %d, exclude %r, chunk %d"
                            % (k, exclude, chunk))
    finally:
        gpus[0].set_option("debug.predict_chunk", DEFAULT_CHUNK)
    got = engine.coassign_resident_topk_many(gpus, rows, 16)
    assert (got[0] != rows[:, None]).all()
    dev = engine.coassign_resident_topk_many_torch(
        gpus, torch.from_numpy(rows).cuda(), 16)
    assert dev[0].is_cuda and dev[0].dtype == torch.int32
    assert dev[1].is_cuda and dev[1].dtype == torch.float32
    assert_same((dev[0].cpu().numpy(), dev[1].cpu().numpy()),
                (got[0].view(np.uint32), got[1]), "the torch form")
    # _many at m = 1 against the single form
    one = gpus[2].coassign_resident_topk(rows, 9, True, 10, n - 10)
    assert_same(engine.coassign_resident_topk_many([gpus[2]], rows, 9, True,
                                                   10, n - 10),
                (one[0].view(np.uint32), one[1]), "m = 1")
    assert_same(one, se.topk(se.resident_cells(assign[2:3], rows), 9, 10,
                             n - 10, rows), "one engine")
    index, prob = gpus[2].coassign_resident_topk_torch(
        torch.from_numpy(rows.astype(np.int32)).cuda(), 9, True, 10, n - 10)
    assert_same((index.cpu().numpy(), prob.cpu().numpy()),
                (one[0].view(np.uint32), one[1]), "one engine, torch")
    # the readers left the engines alone
    for g, a in zip(gpus, assign):
        assert np.array_equal(g.assignments(), a)


def test_66_engines_of_64_rows():
    from distributions_amd import engine
    n, m = 64, 66
    gpus, assign = [], []
    for i in range(m):
        k = 2 + i % 7
        _, gsh, vals, _ = workloads.make("dd", n, k)
        start = (np.random.default_rng(i).permutation(n) % k).astype(
            np.uint32)
        g = engine.Gibbs(1.0, 0.2, gsh)
        g.load_rows(vals, start, k, 1)
        gpus.append(g)
        assign.append(g.assignments())
    rows = np.arange(n)
    res = se.resident_cells(assign, rows)
    assert len(np.unique(res)) > 10
    for k in (5, 64):
        assert_same(engine.coassign_resident_topk_many(gpus, rows, k),
                    se.topk(res, k, 0, None, rows), "66 engines, k = %d" % k)
    # held-out queries over 66 engines: the table's own values as queries,
    # against the dense route the library already has
    _, _, vals, _ = workloads.make("dd", n, 2)
    q = [np.ascontiguousarray(v[:20]) for v in vals]
    r = [g.responsibilities(q) for g in gpus]
    slots = [np.array([g.core.global_to_packed(int(a)) for a in col])
             for g, col in zip(gpus, assign)]
    cells = se.held_out_cells(r, slots)
    assert_same(engine.search_resident_many(gpus, q, 7), se.topk(cells, 7),
                "66 engines, held-out")


# ---------------------------------------------------------------------------
# forms and rules


def test_the_forms_agree():
    import torch
    from distributions_amd import engine
    for name in ("gp_nich", "ens3_dd_bb_gp"):
        c = se.case(name)
        gpus = engines_of(name)
        q = c.cols()
        words = [torch.from_numpy(
            np.ascontiguousarray(w).view(np.int32).copy()).cuda()
            for w in pe.query_words(c.orcs[0], q)]
        host = engine.search_resident_many(gpus, q, 5, 3, c.n - 1)
        assert host[0].dtype == np.int32 and host[0].shape == (len(q[0]), 5)
        assert_same(host, se.topk(c.cells(), 5, 3, c.n - 1), name)
        index, prob = engine.search_resident_many_torch(gpus, words, 5, 3,
                                                        c.n - 1)
        assert index.is_cuda and index.dtype == torch.int32
        assert prob.is_cuda and prob.dtype == torch.float32
        assert_same((index.cpu().numpy(), prob.cpu().numpy()),
                    (host[0].view(np.uint32), host[1]), name + " torch")
        if len(gpus) == 1:
            one = gpus[0].search_resident(q, 5, 3, c.n - 1)
            assert_same(one, (host[0].view(np.uint32), host[1]), "single")
            index, prob = gpus[0].search_resident_torch(words, 5, 3, c.n - 1)
            assert_same((index.cpu().numpy(), prob.cpu().numpy()),
                        (host[0].view(np.uint32), host[1]), "single torch")
        with pytest.raises(RuntimeError, match="one value column per feature"):
            engine.search_resident_many_torch(gpus, words + words[:1])
        with pytest.raises(RuntimeError, match="one CUDA device"):
            engine.search_resident_many_torch(gpus,
                                              [words[0].cpu()] + words[1:])


def test_limits_flags_and_ranges():
    from distributions_amd import _core, engine
    c = se.case("ens3_dd_bb_gp")
    gpus = engines_of("ens3_dd_bb_gp")
    cores = [g.core for g in gpus]
    q, n = c.cols(), c.n
    rows = query_rows(n)
    with pytest.raises(RuntimeError, match="k is at most 128"):
        engine.search_resident_many(gpus, q, 129)
    with pytest.raises(RuntimeError, match="k is at most 128"):
        engine.coassign_resident_topk_many(gpus, rows, 129)
    with pytest.raises(RuntimeError, match="ld is less than k"):
        _core.search_resident_many(cores, q, 0, n, 5, 0, False, 4)
    with pytest.raises(RuntimeError, match="ld is less than k"):
        _core.coassign_resident_topk_many(cores, rows, 0, n, 5, 0, False, 4)
    got = _core.search_resident_many(cores, q, 0, n, 5, 0, False, 9)
    assert_same((got[0].view(np.int32), got[1]), se.topk(c.cells(), 5),
                "ld = 9")
    with pytest.raises(RuntimeError, match="EXCLUDE_SELF"):
        _core.search_resident_many(cores, q, 0, n, 5,
                                   _core.COASSIGN_EXCLUDE_SELF)
    with pytest.raises(RuntimeError, match="unknown flag"):
        _core.coassign_resident_topk_many(cores, rows, 0, n, 5, 2)
    with pytest.raises(RuntimeError, match="unknown flag"):
        _core.search_resident_many(cores, q, 0, n, 5, 2)
    for call in (lambda lo, hi: engine.search_resident_many(gpus, q, 5, lo,
                                                            hi),
                 lambda lo, hi: engine.coassign_resident_topk_many(
                     gpus, rows, 5, True, lo, hi)):
        with pytest.raises(RuntimeError, match="row_begin is past row_end"):
            call(8, 7)
        with pytest.raises(RuntimeError,
                           match="row_end is past the engines' %d rows" % n):
            call(0, n + 1)
    # nothing to do
    none = [col[:0] for col in q]
    assert engine.search_resident_many(gpus, none)[0].shape == (0, 10)
    assert engine.search_resident_many(gpus, q, k=0)[1].shape == (len(q[0]),
                                                                  0)
    assert engine.coassign_resident_topk_many(gpus, [])[0].shape == (0, 10)
    assert engine.coassign_resident_topk_many(gpus, rows, 0)[0].shape == (
        len(rows), 0)


def test_refusals_of_the_engines(chains):
    from distributions_amd import engine
    gpus, _ = chains
    c = se.case("dd")
    dd = engines_of("dd")
    _, gsh, vals, assign = workloads.make("dd", 500, 4)
    short = engine.Gibbs(1.0, 0.2, gsh)
    short.load_rows(vals, assign, 4, 1)
    q = c.cols()
    with pytest.raises(RuntimeError, match="unequal row counts: engine 1 "
                       "holds 500 rows, engine 0 2000"):
        engine.coassign_resident_topk_many([gpus[0], short], [0, 1])
    with pytest.raises(RuntimeError, match="unequal row counts"):
        engine.search_resident_many([dd[0], short], q)
    with pytest.raises(RuntimeError, match="the same engine twice"):
        engine.coassign_resident_topk_many([gpus[0], gpus[1], gpus[0]], [0])
    with pytest.raises(RuntimeError, match="the same engine twice"):
        engine.search_resident_many([dd[0], dd[0]], q)
    with pytest.raises(RuntimeError, match="null engine"):
        engine.coassign_resident_topk_many([gpus[0], None], [0])
    unassigned = engine.Gibbs(1.0, 0.2, gsh)
    unassigned.load_rows_unassigned(vals, 1)
    with pytest.raises(RuntimeError, match="engine 1 has unassigned rows"):
        engine.coassign_resident_topk_many([short, unassigned], [0, 1])
    with pytest.raises(RuntimeError, match="engine 0 has unassigned rows"):
        unassigned.search_resident([v[:3] for v in vals])
    # held-out queries need one feature list and one clustering model
    with pytest.raises(RuntimeError, match="engines of one feature list"):
        engine.search_resident_many([dd[0], gpus[0]], q)
    # (LowEntropy beside PitmanYor, the same table and feature)
    with pytest.raises(RuntimeError, match="engines of one clustering model"):
        engine.search_resident_many([dd[0], engines_of("le_dd")[0]], q)
    # an open batch on one member
    short.core.batch_sample(0, 256, ol.oracle().orc_rng_seed(3), 0)
    with pytest.raises(RuntimeError, match="batch open on engine 0"):
        short.coassign_resident_topk([0, 1])
    with pytest.raises(RuntimeError, match="batch open on engine 0"):
        short.search_resident([v[:3] for v in vals])
    short.core.batch_apply_local()
    short.core.batch_finish()
    assert short.coassign_resident_topk([0, 1], 3)[0].shape == (2, 3)


def test_a_query_index_past_the_rows_fails_naming_it(chains):
    import torch
    from distributions_amd import engine
    gpus, assign = chains
    n = assign[0].size
    rows = np.arange(300)
    rows[211] = n
    rows[250] = n + 5
    with pytest.raises(RuntimeError, match=r"rows\[211\]"):
        engine.coassign_resident_topk_many(gpus, rows)
    with pytest.raises(RuntimeError, match=r"rows\[211\]"):
        engine.coassign_resident_topk_many_torch(
            gpus, torch.from_numpy(rows).cuda())
    try:
        gpus[0].set_option("debug.predict_chunk", 128)
        with pytest.raises(RuntimeError, match=r"2000 rows at rows\[211\]"):
            gpus[0].coassign_resident_topk(rows)
    finally:
        gpus[0].set_option("debug.predict_chunk", DEFAULT_CHUNK)
    rows[211], rows[250] = 1, 2
    assert (engine.coassign_resident_topk_many(gpus, rows)[0] >= 0).all()


def test_a_value_outside_its_domain_fails_and_names_the_row():
    from distributions_amd import engine
    c = se.case("ens3_dd_bb_gp")
    gpus = engines_of("ens3_dd_bb_gp")
    q = c.cols()
    bad = [col.copy() for col in q]
    bad[1][61] = 2
    bad[1][37] = 2                      # the first offending row is named
    bad[0][66] = 200                    # (a later row, an earlier feature)
    with pytest.raises(RuntimeError, match="row 37, feature 1"):
        engine.search_resident_many(gpus, bad)
    # process and engines go on
    assert_same(engine.search_resident_many(gpus, q, 5),
                se.topk(c.cells(), 5), "after the refusal")


def test_the_calls_change_nothing_and_a_sweep_goes_on_as_its_twins():
    from distributions_amd import engine
    c = se.case("ens3_dd_bb_gp")
    gpus, twins = c.sub.engines(), c.sub.engines()
    q = c.cols()
    rows = query_rows(c.n)
    before = [(g.assignments().copy(), g.counts().copy()) for g in gpus]
    engine.search_resident_many(gpus, q)
    engine.coassign_resident_topk_many(gpus, rows, 64)
    gpus[0].search_resident(q, k=3)
    gpus[1].coassign_resident_topk(rows, k=3)
    for g, (a, cnt) in zip(gpus, before):
        assert np.array_equal(g.assignments(), a)
        assert np.array_equal(g.counts(), cnt)
    for g, twin in zip(gpus, twins):
        n = len(g.assignments())
        g.sweep(0, n, 500, 11)
        twin.sweep(0, n, 500, 11)
        # (a run the sweep left open stays resumable under the calls)
        engine.search_resident_many([g], q, k=3)
        engine.coassign_resident_topk_many([g], rows, k=3)
        g.sweep(0, n, 500, 12, draw_base=n)
        twin.sweep(0, n, 500, 12, draw_base=n)
        assert np.array_equal(g.assignments(), twin.assignments())
        assert np.array_equal(g.counts(), twin.counts())
        g.validate()
