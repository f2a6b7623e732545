"""The expectation of dist_gibbs_search_resident[_many] and
dist_gibbs_coassign_resident_topk[_many] (tests/search_resident_expect.py) held
to itself, to the float64 law and against planted bugs; and the new entry
points' refusal without a device.  No GPU.

The law, as tests/test_coassign_topk_oracle.py states it: a cell's float is
within `band` of C64, so the j-th largest float cell of a query is at least
the j-th largest of C64 - band over its targets, and the cell of the j-th
returned target is at most its C64 + band.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import coassign_expect as ce  # noqa: E402
import search_resident_expect as se  # noqa: E402

TINY = float(ce.TINY32)


def test_without_a_device_the_new_entries_fail_loudly():
    """(with one they do nothing for no engine)"""
    import torch
    from distributions_amd import engine
    calls = [lambda: engine.search_resident_many([], [], k=3),
             lambda: engine.coassign_resident_topk_many([], [0, 1], k=3)]
    for name in ("search_resident", "search_resident_torch",
                 "coassign_resident_topk", "coassign_resident_topk_torch"):
        assert callable(getattr(engine.Gibbs, name))
    for name in ("search_resident_many", "search_resident_many_torch",
                 "coassign_resident_topk_many",
                 "coassign_resident_topk_many_torch"):
        assert callable(getattr(engine, name))
    for call in calls:
        if torch.cuda.is_available():
            index, prob = call()
            assert index.dtype == np.int32 and prob.dtype == np.float32
            assert index.shape == prob.shape and index.shape[1] == 3
        else:
            with pytest.raises(RuntimeError, match="no HIP device"):
                call()


def test_the_subjects_are_those_whose_members_hold_assigned_rows():
    assert set(ce.NAMES) - set(se.NAMES) == {"only_empty_k3"}
    # (members loaded with 5, 20 and 43 slots; the swept ones have grown)
    sizes = [len(o) for o in se.case("ens3_gp_nich").orcs]
    assert se.case("ens3_gp_nich").M == 3 and sizes[0] == 5
    assert sizes[1] >= 20 and sizes[2] >= 43 and sizes[1] != sizes[2]
    for name in se.NAMES:
        c = se.case(name)
        for orc, slots in zip(c.orcs, c.slots):
            assert (np.asarray(orc.assign) != 0xFFFFFFFF).all()
            assert slots.min() >= 0 and slots.max() < len(orc)


@pytest.mark.parametrize("name", se.NAMES)
def test_the_two_forms_agree_and_no_cell_is_near_underflow(name):
    c = se.case(name)
    cells = c.cells()
    assert cells.shape == (len(c.rq), c.n) and len(c.rq) >= 30
    assert (cells >= 0).all() and not np.signbit(cells).any()
    # (the division by M flushes below the smallest normal: no cell is there)
    assert not ((cells > 0) & (cells < 4 * TINY)).any()
    rows = np.array([0, 7, 7, c.n - 1, 129])
    res = se.resident_cells(c.assigns, rows)
    assert (np.diag(res[:, rows]) == 1).all()
    for k in (1, 5, 64, 128):
        for lo, hi in ((0, None), (5, c.n - 3)):
            a = se.topk(cells, k, lo, hi)
            assert se.same(a, se.topk_sorted(cells, k, lo, hi)), (name, k, lo)
            assert ((a[0] >= lo) & (a[0] < (c.n if hi is None else hi))).all()
            for self_rows in (None, rows):
                b = se.topk(res, k, lo, hi, self_rows)
                assert se.same(b, se.topk_sorted(res, k, lo, hi, self_rows))
    # the fill
    for lo, hi, live in ((4, 7, 3), (9, 10, 1), (6, 6, 0)):
        a = se.topk(cells, 8, lo, hi)
        assert se.same(a, se.topk_sorted(cells, 8, lo, hi))
        assert (a[0][:, live:] == se.FILL_INDEX).all()
        assert (se.bits(a[1][:, live:]) == 0).all()
        assert (a[0][:, :live] != se.FILL_INDEX).all()
    # rows 7 of the range [7, 8) without self: nothing is left
    b = se.topk(res[1:3], 2, 7, 8, rows[1:3])
    assert (b[0] == se.FILL_INDEX).all() and (se.bits(b[1]) == 0).all()


@pytest.mark.parametrize("name", se.NAMES)
def test_ranks_agree_with_the_float64_law_within_its_bands(name):
    c = se.case(name)
    cells = c.cells()
    C, band = c.law()
    assert C.shape == cells.shape == band.shape
    assert (band >= 0).all() and np.isfinite(band).all()
    # every cell is within its band of the law
    assert (np.abs(cells.astype(np.float64) - C) <= band).all(), name
    n = c.n
    index, _ = se.topk(cells, 128)
    for a in range(len(c.rq)):
        lower = np.sort(C[a] - band[a])[::-1][:128]
        got = index[a].astype(np.int64)
        assert len(set(got)) == min(128, n) and got.max() < n
        upper = (C[a] + band[a])[got]
        assert (upper >= lower).all(), (name, a)


# ---------------------------------------------------------------------------
# planted bugs


def ascending(cells, k):
    key = se.ct.keys(cells, False)
    return se.ct.decode(np.sort(key, axis=1)[:, :k])


def ties_to_the_larger_index(cells, k):
    n = cells.shape[1]
    index, prob = se.topk(cells[:, ::-1], k)
    live = index != se.FILL_INDEX
    index[live] = n - 1 - index[live]
    return index, prob


def slices_concatenated(cells, k, width):
    index, prob = [], []
    for lo in range(0, cells.shape[1], width):
        i, p = se.topk(cells, k, lo, min(lo + width, cells.shape[1]))
        index.append(i)
        prob.append(p)
    return np.hstack(index)[:, :k], np.hstack(prob)[:, :k]


def offset_in_the_range(cells, k, lo, hi):
    index, prob = se.topk(cells, k, lo, hi)
    index[index != se.FILL_INDEX] -= lo
    return index, prob


@pytest.mark.parametrize("name", ["dd_swept", "ens3_gp_nich"])
def test_planted_bugs_differ(name):
    c = se.case(name)
    cells = c.cells()
    k = 6
    want = se.topk(cells, k)
    # 1 / M missing (M = 1 divides by one: the ensemble shows it)
    if c.M > 1:
        no_mean = se.held_out_cells(c.r(), c.slots, use_m=False)
        assert not se.same(se.topk(no_mean, k), want)
    # the global id taken for the slot: a swept subject's ids have outrun
    # the packed indices
    if name.endswith("_swept"):
        orc, slots, ids = c.orcs[0], c.slots[0], c.assigns[0].astype(np.int64)
        assert (ids != slots).any() and ids.max() >= len(orc)
        r = c.r()[0]
        padded = np.zeros((r.shape[0], int(ids.max()) + 1), np.float32)
        padded[:, :r.shape[1]] = r
        assert not se.same(se.topk(se.held_out_cells([padded], [ids]), k),
                           want)
    assert not se.same(ties_to_the_larger_index(cells, k), want)
    assert not se.same(ascending(cells, k), want)
    assert not se.same(slices_concatenated(cells, k, 130), want)
    assert se.same(slices_concatenated(cells, k, c.n), want)
    assert not se.same(offset_in_the_range(cells, k, 5, c.n - 3),
                       se.topk(cells, k, 5, c.n - 3))
    # resident queries: all ties
    rows = np.array([3, 3, c.n - 1, 200])
    res = se.resident_cells(c.assigns, rows)
    want_r = se.topk(res, k, 0, None, rows)
    assert not se.same(se.topk(res, k), want_r)              # self kept
    assert not se.same(ties_to_the_larger_index(res, k), se.topk(res, k))
    assert not se.same(ascending(res, k), se.topk(res, k))
    assert not se.same(slices_concatenated(res, k, 130), se.topk(res, k))
    assert not se.same(offset_in_the_range(res, k, 5, c.n - 3),
                       se.topk(res, k, 5, c.n - 3))
    if c.M > 1:
        counts = (res * np.float32(c.M)).astype(np.float32)
        assert not se.same(se.topk(counts, k), se.topk(res, k))
