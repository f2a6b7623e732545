"""What dist_gibbs_coassign_topk[_many] must return: per query row the k
largest cells of the co-assignment matrix and their targets, ties to the
smaller index, key-0 fill -- from a matrix (tests/coassign_expect.py's
expectation, or coassign_many's own result).

TEST INFRASTRUCTURE (imported by tests only).

Two independent forms:
  topk         by the uint64 key (bits(cell) << 32) | (0xFFFFFFFF - b), sorted
               descending, masked cells key 0
  topk_sorted  Python's sorted on (-value, b) tuples
"""
import numpy as np

import coassign_expect as ce

FILL_INDEX = np.uint32(0xFFFFFFFF)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def keys(matrix, exclude_self):
    """[n_q, n_t] uint64 keys; the excluded self cell is key 0"""
    matrix = np.ascontiguousarray(matrix, np.float32)
    n_q, n_t = matrix.shape
    b = np.arange(n_t, dtype=np.uint64)
    key = (bits(matrix).astype(np.uint64) << np.uint64(32)) | (
        np.uint64(0xFFFFFFFF) - b)[None, :]
    if exclude_self:
        d = np.arange(min(n_q, n_t))
        key[d, d] = 0
    return key


def decode(key):
    """uint64 keys -> (uint32 index, float32 prob): key 0 is the fill"""
    key = np.ascontiguousarray(key, np.uint64)
    index = (np.uint64(0xFFFFFFFF) - (key & np.uint64(0xFFFFFFFF))).astype(
        np.uint32)
    prob = (key >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return index, prob


def topk(matrix, k, exclude_self=False):
    """-> (index uint32 [n_q, k], prob float32 [n_q, k])"""
    key = keys(matrix, exclude_self)
    n_q = key.shape[0]
    out = np.zeros((n_q, k), np.uint64)
    srt = np.sort(key, axis=1)[:, ::-1]
    take = min(k, key.shape[1])
    out[:, :take] = srt[:, :take]
    return decode(out)


def topk_sorted(matrix, k, exclude_self=False):
    matrix = np.ascontiguousarray(matrix, np.float32)
    n_q, n_t = matrix.shape
    index = np.full((n_q, k), FILL_INDEX, np.uint32)
    prob = np.zeros((n_q, k), np.float32)
    for a in range(n_q):
        row = [(-float(matrix[a, b]), b) for b in range(n_t)
               if not (exclude_self and b == a)]
        for j, (v, b) in enumerate(sorted(row)[:k]):
            index[a, j] = b
            prob[a, j] = matrix[a, b]
    return index, prob


class Case(object):
    """a coassign_expect subject restricted to its specified rows: the
    queries, the targets and the expected matrices of those rows"""

    def __init__(self, name):
        self.sub = ce.subject(name)
        sub = self.sub
        self.rq = sub.rq[sub.specified(sub.rq)]
        self.rt = sub.rt[sub.specified(sub.rt)]
        self._ok_q = np.flatnonzero(sub.specified(sub.rq))
        self._ok_t = np.flatnonzero(sub.specified(sub.rt))

    def expect(self, sym):
        cols = self._ok_q if sym else self._ok_t
        return self.sub.expect(sym)[np.ix_(self._ok_q, cols)]

    def law(self, sym):
        cols = self._ok_q if sym else self._ok_t
        C, band = self.sub.law(sym)
        ix = np.ix_(self._ok_q, cols)
        return C[ix], band[ix]


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]
