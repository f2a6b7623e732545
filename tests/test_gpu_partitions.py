"""What M chains say about their resident rows:
engine.partition_agreement_labels / partition_agreement_many /
Gibbs.partition_agreement and engine.coassign_resident_many against the numpy
restatement of tests/partition_expect.py.

sq must be EQUAL everywhere.  nlogn must be within
    (cells + 4) * 2^-52 * sum n log n
of the restatement -- one ulp for log and one rounding per add, over the
cells that add anything (n > 1; log 1 is an exact zero); derived, not fitted
-- and bit-equal between two equal calls."""
import ctypes
import os

import numpy as np
import pytest

import partition_expect as pe
import workloads

pytestmark = pytest.mark.gpu

# include/distributions_hip.h: one uint32 count and one uint32 first-row word
# per label in 144 KiB of LDS
BIN_LIMIT = 144 * 1024 // 8
# kernels_apply.h, kCsMaxKeys: the counting sort's keys (the labels and one
# padding key); beyond, the library sort
CS_MAX_LABELS = 7000 - 1


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and (
        a.tobytes() == b.tobytes())


def hold(res, columns, m=0):
    """res against the restatement on `columns`"""
    want, cells = pe.agreement(columns, m=m)
    p = len(columns)
    assert res.n == len(columns[0]) and res.m == m
    assert res.sq.dtype == np.uint64 and res.sq.shape == (p, p)
    assert np.array_equal(res.sq, want.sq)
    if res.nlogn is not None:
        assert res.nlogn.dtype == np.float64 and res.nlogn.shape == (p, p)
        bound = (cells + 4) * 2.0 ** -52 * want.nlogn
        err = np.abs(res.nlogn - want.nlogn)
        assert (err <= bound).all(), (err.max(), bound[err > bound])
        assert same_bits(res.nlogn, res.nlogn.T)
    return want


def labels_twice(columns, n_labels=None):
    """the labels entry, called twice: held to the restatement, nlogn equal
    in every bit"""
    from distributions_amd import engine
    res = engine.partition_agreement_labels(columns, n_labels)
    again = engine.partition_agreement_labels(columns, n_labels)
    assert same_bits(res.nlogn, again.nlogn)
    assert np.array_equal(res.sq, again.sq)
    hold(res, columns)
    return res


# ---------------------------------------------------------------------------
# the labels entry


@pytest.mark.parametrize("n", [1, 2, 257])
@pytest.mark.parametrize("p", [1, 2, 3, 65])
def test_small_shapes(n, p):
    rng = np.random.default_rng(1000 * n + p)
    cols = [rng.integers(0, 1 + (a * 5) % 11, n).astype(np.uint32)
            for a in range(p)]
    labels_twice(cols)


def test_segment_lengths_about_the_wave_and_the_workgroup():
    """one column whose groups hold 1, 63, 64, 65, 1023, 1024 and 1025 rows,
    rows in random order"""
    sizes = [1, 63, 64, 65, 1023, 1024, 1025]
    rng = np.random.default_rng(11)
    a = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    n = a.size
    cols = [a.astype(np.uint32), rng.integers(0, 3, n).astype(np.uint32),
            rng.integers(0, 700, n).astype(np.uint32),
            np.arange(n, dtype=np.uint32) // 2]
    labels_twice(cols)


def test_one_group_and_all_singletons():
    n = 5000
    rng = np.random.default_rng(12)
    cols = [np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32),
            rng.integers(0, 37, n).astype(np.uint32),
            rng.permutation(n).astype(np.uint32)]
    res = labels_twice(cols)
    assert int(res.sq[0, 0]) == n * n and int(res.sq[1, 1]) == n
    assert res.nlogn[1, 1] == 0.0 and res.nlogn[0, 1] == 0.0


def test_a_group_of_70000_rows_needs_64_bits():
    n = 70001
    one = np.zeros(n, np.uint32)
    a = one.copy()
    a[-1] = 1
    rng = np.random.default_rng(13)
    cols = [a, one, rng.integers(0, 3, n).astype(np.uint32)]
    res = labels_twice(cols)
    assert int(res.sq[0, 1]) == 70000 ** 2 + 1 > 2 ** 32
    assert int(res.sq[1, 1]) == n * n


@pytest.mark.parametrize("k", [CS_MAX_LABELS, CS_MAX_LABELS + 1, BIN_LIMIT])
def test_label_counts_at_the_sorts_threshold_and_the_bin_limit(k):
    """the counting sort's last size, the library sort's first, and the most
    bins the pairs kernel's LDS holds (past 64 KiB: the kernel opts in)"""
    n = 20011
    rng = np.random.default_rng(k)
    a = rng.integers(0, k, n).astype(np.uint32)
    a[5] = k - 1
    a[6] = 0
    cols = [a, (a // 3).astype(np.uint32),
            rng.integers(0, 5, n).astype(np.uint32)]
    labels_twice(cols, [k, k, 5])


def test_one_bin_past_the_limit_is_refused_naming_the_partition():
    from distributions_amd import engine
    cols = [np.zeros(300, np.uint32)] * 3
    with pytest.raises(RuntimeError, match="partition 1 has %d labels"
                       % (BIN_LIMIT + 1)):
        engine.partition_agreement_labels(cols, [5, BIN_LIMIT + 1, 5])
    hold(engine.partition_agreement_labels(cols, [5, BIN_LIMIT, 5]), cols)


def abi():
    here = os.path.dirname(os.path.abspath(__file__))
    lib = ctypes.CDLL(os.path.join(here, "..", "distributions_amd",
                                   "libdistributions_hip.so"))
    lib.dist_partition_agreement.restype = ctypes.c_int
    lib.dist_partition_agreement.argtypes = [
        ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p]
    lib.dist_last_error.restype = ctypes.c_char_p
    return lib


def abi_call(lib, cols, n_labels, sq, nl):
    ptrs = (ctypes.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
    bounds = np.asarray(n_labels, np.uint32)
    return lib.dist_partition_agreement(
        cols[0].size, len(cols), ptrs, bounds.ctypes.data, sq.ctypes.data,
        None if nl is None else nl.ctypes.data)


def test_a_label_at_its_bound_fails_naming_it_and_writes_nothing():
    """through the C ABI, so that the outputs are the test's own: a label
    equal to n_labels in the last row of the last column"""
    from distributions_amd import engine
    lib = abi()
    n, p = 1000, 3
    rng = np.random.default_rng(14)
    cols = [rng.integers(0, 9, n).astype(np.uint32) for _ in range(p)]
    bad = [c.copy() for c in cols]
    bad[2][n - 1] = 9
    sq = np.full(p * p + 8, 0xA5A5A5A5A5A5A5A5, np.uint64)
    nl = np.full(p * p + 8, -7.25, np.float64)
    assert abi_call(lib, bad, [9] * p, sq, nl) != 0
    assert b"partition 2 at row 999" in lib.dist_last_error()
    assert (sq == 0xA5A5A5A5A5A5A5A5).all() and (nl == -7.25).all()
    with pytest.raises(RuntimeError, match="partition 2 at row 999"):
        engine.partition_agreement_labels(bad, 9)
    # the first such row of the first such partition
    bad[1][400] = 2 ** 31
    bad[1][17] = 77
    with pytest.raises(RuntimeError, match="partition 1 at row 17"):
        engine.partition_agreement_labels(bad, 9)
    # the same buffers, a good call: the matrices and nothing beyond them
    assert abi_call(lib, cols, [9] * p, sq, nl) == 0
    want, _ = pe.agreement(cols)
    assert np.array_equal(sq[:p * p].reshape(p, p), want.sq)
    assert (sq[p * p:] == 0xA5A5A5A5A5A5A5A5).all()
    assert (nl[p * p:] == -7.25).all() and (nl[:p * p] != -7.25).all()
    # no nlogn: nothing is written there
    sq[:] = 0xA5A5A5A5A5A5A5A5
    assert abi_call(lib, cols, [9] * p, sq, None) == 0
    assert np.array_equal(sq[:p * p].reshape(p, p), want.sq)
    res = engine.partition_agreement_labels(cols, 9, nlogn=False)
    assert res.nlogn is None and np.array_equal(res.sq, want.sq)
    # p == 0 and n_rows == 0 do nothing
    sq[:] = 0xA5A5A5A5A5A5A5A5
    assert abi_call(lib, [c[:0] for c in cols], [9] * p, sq, None) == 0
    assert (sq == 0xA5A5A5A5A5A5A5A5).all()


def test_host_arrays_and_device_tensors_agree():
    import torch
    from distributions_amd import engine
    rng = np.random.default_rng(15)
    n = 3001
    cols = [rng.integers(0, 1 + 13 * a, n).astype(np.uint32)
            for a in range(5)]
    host = labels_twice(cols)
    dev = engine.partition_agreement_labels(
        [torch.from_numpy(c.astype(np.int32)).cuda() for c in cols])
    assert np.array_equal(dev.sq, host.sq)
    assert same_bits(dev.nlogn, host.nlogn)
    wide = engine.partition_agreement_labels(
        [torch.from_numpy(c.astype(np.int64)).cuda() for c in cols],
        n_labels=[int(c.max()) + 3 for c in cols])
    assert np.array_equal(wide.sq, host.sq)
    assert same_bits(wide.nlogn, host.nlogn)
    with pytest.raises(RuntimeError, match="extra column 1 has"):
        engine.partition_agreement_labels([cols[0], cols[1][:-1]])


# ---------------------------------------------------------------------------
# engines


@pytest.fixture(scope="module")
def chains():
    """eight engines on one planted table, different starts and seeds, three
    exact sweeps each in launches that cover all: global ids have outrun the
    group counts.  -> (truth, engines, their assignments); left as they are"""
    from distributions_amd import _core, engine
    n, k, m = 2000, 16, 8
    truth, _, gsh, vals = workloads.planted(n, k)
    gpus = []
    for i in range(m):
        start = np.random.default_rng(100 + i).permutation(n) % (k + i)
        g = engine.Gibbs(1.0, 0.1, gsh)
        g.load_rows(vals, start.astype(np.uint32), k + i, 1)
        gpus.append(g)
    states = np.array([_core.rng_seed(900 + i) for i in range(m)], np.uint32)
    for _ in range(3):
        states = engine.sweep_sequential_many(gpus, 0, n, states)
    return truth.astype(np.uint32), gpus, [g.assignments() for g in gpus]


def test_eight_chains_and_the_truth(chains):
    from distributions_amd import engine
    truth, gpus, assign = chains
    assert max(int(a.max()) for a in assign) >= max(len(g) for g in gpus)
    assert len({a.tobytes() for a in assign}) > 1
    res = engine.partition_agreement_many(gpus, extra=[truth])
    again = engine.partition_agreement_many(gpus, extra=[truth])
    assert same_bits(res.nlogn, again.nlogn)
    want = hold(res, assign + [truth], m=8)
    ari = engine.adjusted_rand_index(res)
    for i, a in enumerate(assign):
        assert abs(ari[i, 8] - workloads.adjusted_rand_index(truth, a)) \
            <= 1e-12
    index, total = engine.consensus(res)
    want_index, want_total = pe.consensus(want)
    assert index == want_index and np.array_equal(total, want_total)
    # the readers left the engines alone
    for g, a in zip(gpus, assign):
        assert np.array_equal(g.assignments(), a)
    # one engine, no extra, and the single-engine form
    one = gpus[3].partition_agreement(extra=[truth, assign[0]])
    hold(one, [assign[3], truth, assign[0]], m=1)
    hold(engine.partition_agreement_many(gpus[:2], nlogn=False), assign[:2],
         m=2)


def test_an_engine_of_1025_groups_beside_one_of_5():
    from distributions_amd import engine
    n = 4100
    gpus = []
    for k in (1025, 5):
        _, gsh, vals, assign = workloads.make("dd", n, k, dim=256)
        g = engine.Gibbs(1.0, 0.2, gsh)
        g.load_rows(vals, assign, k, 1)
        g.sweep(0, n, 1024, 77)
        gpus.append(g)
    res = engine.partition_agreement_many(gpus)
    hold(res, [g.assignments() for g in gpus], m=2)


def swept_once(**options):
    from test_gpu_engine_lifetime import BATCH, N, SEED, make_engine
    gpu = make_engine(**options)
    gpu.sweep(0, N, BATCH, SEED)
    return gpu


def test_a_run_left_open_stays_resumable():
    """a batched sweep leaves a device-normalised run open: the reader
    settles what it needs, the next sweep goes on as a twin's that nobody
    read"""
    from test_gpu_engine_lifetime import BATCH, N, SEED
    options = {"value_sorted": 2, "device_normalise": 1}
    read, twin, third = [swept_once(**options) for _ in range(3)]
    res = read.partition_agreement()
    assert third.validate()["code"] == 0
    mid = third.assignments()
    hold(res, [mid], m=1)
    hold(third.partition_agreement(), [mid], m=1)
    assert third.validate()["code"] == 0
    for g in (read, twin):
        g.sweep(0, N, BATCH, SEED, draw_base=N)
    assert np.array_equal(read.assignments(), twin.assignments())
    assert np.array_equal(read.counts(), twin.counts())
    assert read.validate()["code"] == 0
    assert twin.core.debug_counts()["device_normalised"] > 0


def test_refusals(chains):
    import oracle_lib as ol
    from distributions_amd import engine
    truth, gpus, _ = chains
    _, gsh, vals, assign = workloads.make("dd", 500, 4)
    short = engine.Gibbs(1.0, 0.2, gsh)
    short.load_rows(vals, assign, 4, 1)
    with pytest.raises(RuntimeError, match="unequal row counts: engine 1 "
                       "holds 500 rows, engine 0 2000"):
        engine.partition_agreement_many([gpus[0], short])
    with pytest.raises(RuntimeError, match="unequal row counts"):
        engine.coassign_resident_many([gpus[0], short], [0, 1])
    with pytest.raises(RuntimeError, match="extra column 0 has 1999 rows"):
        engine.partition_agreement_many(gpus[:2], extra=[truth[:-1]])
    with pytest.raises(RuntimeError, match="the same engine twice"):
        engine.partition_agreement_many([gpus[0], gpus[1], gpus[0]])
    with pytest.raises(RuntimeError, match="null engine"):
        engine.partition_agreement_many([gpus[0], None])
    unassigned = engine.Gibbs(1.0, 0.2, gsh)
    unassigned.load_rows_unassigned(vals, 1)
    with pytest.raises(RuntimeError, match="engine 1 has unassigned rows"):
        engine.partition_agreement_many([short, unassigned])
    with pytest.raises(RuntimeError, match="engine 0 has unassigned rows"):
        unassigned.coassign_resident([0, 1])
    # a split batch open on one member
    short.core.batch_sample(0, 256, ol.oracle().orc_rng_seed(3), 0)
    with pytest.raises(RuntimeError, match="batch open on engine 0"):
        short.partition_agreement()
    with pytest.raises(RuntimeError, match="batch open on engine 0"):
        short.coassign_resident([0, 1])
    short.core.batch_apply_local()
    short.core.batch_finish()
    hold(short.partition_agreement(), [short.assignments()], m=1)


# ---------------------------------------------------------------------------
# coassign_resident_many


def coassign_expect(assign, rows, other):
    c = np.zeros((len(rows), len(other)), np.int64)
    for a in assign:
        c += a[rows][:, None] == a[other][None, :]
    return c


def test_coassign_resident_counts(chains):
    import torch
    from distributions_amd import engine
    _, gpus, assign = chains
    n = assign[0].size
    rng = np.random.default_rng(16)
    rows = rng.integers(0, n, 300)
    other = rng.integers(0, n, 200)
    rows[7] = rows[3]
    other[5] = rows[3]
    other[199] = n - 1
    got = engine.coassign_resident_many(gpus, rows, other)
    want = coassign_expect(assign, rows, other)
    assert got.dtype == np.float32 and got.shape == (300, 200)
    assert same_bits(got, (want.astype(np.float32) / np.float32(8)))
    assert want.max() == 8 and (want < 8).any()
    dev = engine.coassign_resident_many_torch(
        gpus, torch.from_numpy(rows).cuda(),
        torch.from_numpy(other.astype(np.int32)).cuda())
    assert same_bits(dev.cpu().numpy(), got)
    # the rows against themselves
    sym = engine.coassign_resident_many(gpus, rows)
    assert same_bits(sym, sym.T.copy())
    assert (np.diag(sym) == 1.0).all()
    assert same_bits(sym, (coassign_expect(assign, rows, rows).astype(
        np.float32) / np.float32(8)))
    sym_dev = engine.coassign_resident_many_torch(
        gpus, torch.from_numpy(rows.astype(np.int32)).cuda())
    assert same_bits(sym_dev.cpu().numpy(), sym)
    # one engine
    one = gpus[2].coassign_resident(rows, other)
    assert same_bits(one, coassign_expect(assign[2:3], rows, other).astype(
        np.float32))
    assert same_bits(gpus[2].coassign_resident_torch(
        torch.from_numpy(rows).cuda(),
        torch.from_numpy(other).cuda()).cpu().numpy(), one)
    # an index equal to N
    bad = other.copy()
    bad[11] = n
    with pytest.raises(RuntimeError, match=r"rows_b\[11\]"):
        engine.coassign_resident_many(gpus, rows, bad)
    with pytest.raises(RuntimeError, match=r"rows_b\[11\]"):
        engine.coassign_resident_many_torch(
            gpus, torch.from_numpy(rows).cuda(),
            torch.from_numpy(bad).cuda())
    bad = rows.copy()
    bad[299] = n
    with pytest.raises(RuntimeError, match=r"rows_a\[299\]"):
        engine.coassign_resident_many(gpus, bad)
    with pytest.raises(RuntimeError, match=r"rows_a\[299\]"):
        engine.coassign_resident_many_torch(gpus,
                                            torch.from_numpy(bad).cuda())


def test_coassign_resident_over_66_engines():
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
    got = engine.coassign_resident_many(gpus, rows)
    want = coassign_expect(assign, rows, rows)
    assert same_bits(got, want.astype(np.float32) / np.float32(m))
    assert len(np.unique(want)) > 10
    # ... and their agreement in one call: 66 partitions
    hold(engine.partition_agreement_many(gpus), assign, m=m)
