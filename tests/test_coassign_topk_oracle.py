"""The expectation of dist_gibbs_coassign_topk[_many]
(tests/coassign_topk_expect.py) held to itself, to the float64 law and against
planted bugs.  No GPU.

The law: a cell's float is within `band` of C64 (tests/coassign_expect.py), so
the j-th largest float cell of a row is at least the j-th largest of
C64 - band over the row's eligible targets, and the cell of the j-th returned
target is at most its C64 + band: the ranks agree with the law wherever the
bands separate them.
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
import coassign_topk_expect as ct  # noqa: E402


def same(a, b):
    return (np.array_equal(a[0], b[0])
            and np.array_equal(ct.bits(a[1]), ct.bits(b[1])))


@pytest.mark.parametrize("name", ce.NAMES)
def test_the_two_forms_agree_and_no_cell_is_near_underflow(name):
    case = ct.case(name)
    for sym in (False, True):
        want = case.expect(sym)
        soft = (want > 0) & (want < ce.UNDERFLOW)
        assert not soft.any(), "%s: %d cells in (0, 2^-100)" % (name,
                                                                soft.sum())
        assert (want >= 0).all() and not np.signbit(want).any()
        n_t = want.shape[1]
        for k in (1, 5, n_t, 64):
            for exclude in ((False, True) if sym else (False,)):
                a = ct.topk(want, k, exclude)
                b = ct.topk_sorted(want, k, exclude)
                assert same(a, b), (name, sym, k, exclude)
                assert a[0].shape == a[1].shape == (want.shape[0], k)
                left = n_t - (1 if exclude else 0)
                assert (a[0][:, left:] == ct.FILL_INDEX).all()
                assert (ct.bits(a[1][:, left:]) == 0).all()
                assert (a[0][:, :min(k, left)] < n_t).all()


@pytest.mark.parametrize("name", ce.NAMES)
def test_ranks_agree_with_the_float64_law_within_its_bands(name):
    case = ct.case(name)
    for sym in (False, True):
        want = case.expect(sym)
        C, band = case.law(sym)
        n_q, n_t = want.shape
        for exclude in ((False, True) if sym else (False,)):
            index, _ = ct.topk(want, n_t, exclude)
            for a in range(n_q):
                elig = np.ones(n_t, bool)
                if exclude:
                    elig[a] = False
                lower = np.sort((C[a] - band[a])[elig])[::-1]
                got = index[a][index[a] != ct.FILL_INDEX].astype(np.int64)
                assert len(got) == elig.sum()
                assert sorted(got) == list(np.flatnonzero(elig))
                upper = (C[a] + band[a])[got]
                assert (upper >= lower).all(), (name, sym, exclude, a)


# ---------------------------------------------------------------------------
# planted bugs


def ties_matrix(name):
    """16 queries against 300 targets, every target repeated 140 and 280
    columns away (as tests/test_gpu_coassign_topk.py's ties case)"""
    sub = ce.subject(name)
    rows = np.arange(300)
    rows = rows[sub.specified(rows)][:140]
    assert len(rows) == 140
    t = np.concatenate([rows, rows, rows[:20]])
    rq = [ce.responsibilities(s[rows[:16]]) for s in sub.scores()]
    rt = [ce.responsibilities(s[t]) for s in sub.scores()]
    return ce.chain(rq, rt, False)


_TIES = {}


def ties(name):
    if name not in _TIES:
        _TIES[name] = ties_matrix(name)
    return _TIES[name]


def ascending(matrix, k, exclude):
    key = ct.keys(matrix, exclude)
    out = np.zeros((key.shape[0], k), np.uint64)
    for a in range(key.shape[0]):
        live = np.sort(key[a][key[a] != 0])[:k]
        out[a, :len(live)] = live
    return ct.decode(out)


def ties_to_the_larger_index(matrix, k, exclude):
    n_t = matrix.shape[1]
    index, prob = ct.topk(matrix[:, ::-1], k, False)
    assert not exclude
    live = index != ct.FILL_INDEX
    index[live] = n_t - 1 - index[live]
    return index, prob


def tiles_concatenated(matrix, k, exclude):
    assert not exclude
    index, prob = [], []
    for j0 in range(0, matrix.shape[1], 128):
        i, p = ct.topk(matrix[:, j0:j0 + 128], k, False)
        i[i != ct.FILL_INDEX] += j0
        index.append(i)
        prob.append(p)
    return np.hstack(index)[:, :k], np.hstack(prob)[:, :k]


def padding_columns(matrix, k, exclude):
    pad = -matrix.shape[1] % 128
    return ct.topk(np.pad(matrix, ((0, 0), (0, pad))), k, exclude)


@pytest.mark.parametrize("name", ["dd", "gp_nich"])
def test_planted_bugs_differ(name):
    case = ct.case(name)
    rect, sym, wide = case.expect(False), case.expect(True), ties(name)
    n_t = rect.shape[1]
    for matrix, exclude in ((rect, False), (sym, True), (wide, False)):
        assert not same(ascending(matrix, 5, exclude),
                        ct.topk(matrix, 5, exclude))
    # bit-equal cells in one row: dd's single categorical feature gives them
    # within the subject's own rows, the repeated targets in both
    if name == "dd":
        assert not same(ties_to_the_larger_index(rect, n_t, False),
                        ct.topk(rect, n_t, False))
    assert not same(ties_to_the_larger_index(wide, 6, False),
                    ct.topk(wide, 6, False))
    for k in (5, sym.shape[1]):
        assert not same(ct.topk(sym, k, False), ct.topk(sym, k, True))
    assert not same(tiles_concatenated(wide, 6, False), ct.topk(wide, 6, False))
    assert same(tiles_concatenated(rect, 6, False), ct.topk(rect, 6, False))
    assert not same(padding_columns(rect, 64, False), ct.topk(rect, 64, False))
    assert same(padding_columns(rect, 5, False), ct.topk(rect, 5, False))
