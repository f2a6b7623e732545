"""What the partition-agreement calls are held to: a numpy restatement of
include/distributions_hip.h's definitions, independent of the device code.
Contingency tables by np.add.at in int64; sq, nlogn and the derived measures
from them.

`bug` plants a mistake, so that the tests can show that the restatement tells
a wrong answer from a right one:
    "sq_no_diagonal"   sq without the cells on the table's diagonal
    "pairs_n2"         C taken as n^2 / 2
    "binder_half"      Binder's distance with the factor 2 missing"""
import numpy as np


def contingency(a, b):
    """-> int64 [labels of a, labels of b] (labels renamed to 0 .. in order
    of value: the measures do not depend on names)"""
    ua, ia = np.unique(np.asarray(a), return_inverse=True)
    ub, ib = np.unique(np.asarray(b), return_inverse=True)
    c = np.zeros((ua.size, ub.size), np.int64)
    np.add.at(c, (ia.reshape(-1), ib.reshape(-1)), 1)
    return c


def cells_sq(c, bug=None):
    c = c.astype(np.int64)
    if bug == "sq_no_diagonal":
        k = min(c.shape)
        return int((c * c).sum() - (np.diag(c)[:k] ** 2).sum())
    return int((c * c).sum())


def cells_nlogn(c):
    """-> (sum n log n over the cells, the number of cells with n > 1 -- the
    ones that add something)"""
    n = c[c > 1].astype(np.float64)
    return float((n * np.log(n)).sum()), int(n.size)


class Result(object):
    """engine.PartitionAgreement's fields"""

    def __init__(self, sq, nlogn, n, m):
        self.sq, self.nlogn, self.n, self.m = sq, nlogn, n, m


def agreement(columns, m=None, bug=None):
    """-> (Result, cells int64 [P, P]: the cells that add to nlogn[a, b])"""
    p = len(columns)
    n = len(columns[0]) if p else 0
    sq = np.zeros((p, p), np.uint64)
    nl = np.zeros((p, p), np.float64)
    cells = np.zeros((p, p), np.int64)
    for a in range(p):
        for b in range(a, p):
            c = contingency(columns[a], columns[b])
            sq[a, b] = sq[b, a] = cells_sq(c, bug)
            nl[a, b], cells[a, b] = cells_nlogn(c)
            nl[b, a], cells[b, a] = nl[a, b], cells[a, b]
    return Result(sq, nl, n, p if m is None else m), cells


def pair_counts(res, bug=None):
    """(T_ab, T_a, C): the unordered row pairs joined by both partitions, by
    one, and all of them"""
    sq = res.sq.astype(np.int64)
    n = int(res.n)
    t = (sq - n) // 2
    c = n * n / 2.0 if bug == "pairs_n2" else n * (n - 1) / 2.0
    return t.astype(np.float64), np.diag(t).astype(np.float64), c


def rand_index(res, bug=None):
    t, ta, c = pair_counts(res, bug)
    if c == 0:
        return np.ones_like(t)
    return (c - ta[:, None] - ta[None, :] + 2 * t) / c


def adjusted_rand_index(res, bug=None):
    t, ta, c = pair_counts(res, bug)
    out = np.ones_like(t)
    if c == 0:
        return out
    for a in range(t.shape[0]):
        for b in range(t.shape[1]):
            e = ta[a] * ta[b] / c
            den = (ta[a] + ta[b]) / 2.0 - e
            if den != 0:
                out[a, b] = (t[a, b] - e) / den
    return out


def binder_distance(res, bug=None):
    sq = res.sq.astype(np.int64)
    d = np.diag(sq)
    factor = 1 if bug == "binder_half" else 2
    return d[:, None] + d[None, :] - factor * sq


def variation_of_information(res):
    d = np.diag(res.nlogn)
    return (d[:, None] + d[None, :] - 2.0 * res.nlogn) / float(res.n)


def consensus(res, among=None, bug=None):
    among = np.arange(res.m) if among is None else np.asarray(among)
    d = binder_distance(res, bug)[np.ix_(among, among)]
    total = d.sum(axis=1)
    return int(among[int(np.argmin(total))]), total


# -- brute force over the explicit N x N matrices (small N only) -------------
def joined(a):
    """delta_a[i, j] = 1 where rows i and j share a label (int64 [N, N])"""
    a = np.asarray(a)
    return (a[:, None] == a[None, :]).astype(np.int64)


def binder_brute(a, b):
    """the ordered pairs (i, j) that one partition joins and the other
    separates"""
    return int((joined(a) != joined(b)).sum())


def consensus_brute(columns):
    """Dahl's least-squares clustering from the posterior similarity matrix
    -> (argmin, sum_ij (delta_a(i, j) - PSM_ij)^2 per sample, in float64)"""
    deltas = [joined(c) for c in columns]
    psm = np.mean(deltas, axis=0)
    loss = np.array([((d - psm) ** 2).sum() for d in deltas])
    return int(np.argmin(loss)), loss
