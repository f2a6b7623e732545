"""What dist_gibbs_search_resident[_many] and
dist_gibbs_coassign_resident_topk[_many] must return: per query the k RESIDENT
rows it is most co-assigned with over M engines.

TEST INFRASTRUCTURE (imported by tests only; numpy and the expectation
modules beside it).

Held-out queries (`Case.cells`): with r_e,q of coassign_expect.Subject.r() and
slot_e(b) the packed index of member e's orc.assign[b],
  acc = float32(0); engines ascending: acc = float32(acc + r_e,q[slot_e(b)])
  cell(q, b) = float32(acc / float32(M))
in numpy float32, subnormal results flushed to zero as the build flushes them.
Resident queries (`resident_cells`): integer counts / float32(M).

Selection over the targets [row_begin, row_end), two independent forms:
  topk         coassign_topk_expect's uint64 keys of the whole table's cells,
               the keys of rows outside the range and of the excluded self row
               set to 0, sorted descending, decoded
  topk_sorted  Python's sorted on (-value, b) tuples

The float64 law (`Case.law`): C64[q, b] = (1/M) sum_e p_e,q[slot_e(b)] with
coassign_expect.law_parts' p and d, and the band, derived, nothing fitted:
  (1/M) sum_e p d  +  (M + 1) eps (1/M) sum_e p (1 + d)
each term's own error; then the chain's M roundings and the division's one
over the inflated sum.
"""
import numpy as np

import coassign_expect as ce
import coassign_topk_expect as ct
import f64_scores as fx

FILL_INDEX = ct.FILL_INDEX
bits = ct.bits

# coassign_expect's subjects whose members all hold assigned rows
NAMES = [n for n in ce.NAMES if n != "only_empty_k3"]


def slots_of(orc):
    """the packed index of every resident row's group: g2p[assign[b]]"""
    g2p = {int(orc.packed_to_global(k)): k for k in range(len(orc))}
    return np.array([g2p[int(a)] for a in orc.assign], np.int64)


def held_out_cells(r, slots, use_m=True):
    """r: per engine [n_q, K_e] float32; slots: per engine [N] -> [n_q, N]
    float32, one chain of binary32 adds per cell"""
    M = len(r)
    acc = np.zeros((r[0].shape[0], len(slots[0])), np.float32)
    with np.errstate(all="ignore"):
        for re_, s in zip(r, slots):
            acc = (acc + np.asarray(re_, np.float32)[:, s]).astype(np.float32)
        if not use_m:
            return acc
        return ce.flush((acc / np.float32(M)).astype(np.float32))


def resident_cells(assigns, rows):
    """assigns: per engine [N] group ids; rows: query row indices -> [n_q, N]
    float32: (engines in which rows[a] and b carry the same id) / M"""
    rows = np.asarray(rows, np.int64)
    c = np.zeros((len(rows), len(assigns[0])), np.int64)
    for a in assigns:
        a = np.asarray(a)
        c += a[rows][:, None] == a[None, :]
    return (c.astype(np.float32) / np.float32(len(assigns))).astype(
        np.float32)


def _bounds(n, row_begin, row_end):
    return row_begin, n if row_end is None else row_end


def topk(cells, k, row_begin=0, row_end=None, self_rows=None):
    """cells: [n_q, N] over the WHOLE table -> (index uint32 [n_q, k], prob
    float32 [n_q, k]); self_rows: per query the row that is left out"""
    n_q, n = cells.shape
    lo, hi = _bounds(n, row_begin, row_end)
    key = ct.keys(cells, False)
    key[:, :lo] = 0
    key[:, hi:] = 0
    if self_rows is not None:
        key[np.arange(n_q), np.asarray(self_rows, np.int64)] = 0
    out = np.zeros((n_q, k), np.uint64)
    take = min(k, n)
    if take:
        out[:, :take] = np.sort(key, axis=1)[:, ::-1][:, :take]
    return ct.decode(out)


def topk_sorted(cells, k, row_begin=0, row_end=None, self_rows=None):
    cells = np.ascontiguousarray(cells, np.float32)
    n_q, n = cells.shape
    lo, hi = _bounds(n, row_begin, row_end)
    index = np.full((n_q, k), FILL_INDEX, np.uint32)
    prob = np.zeros((n_q, k), np.float32)
    for a in range(n_q):
        row = [(-float(cells[a, b]), b) for b in range(lo, hi)
               if self_rows is None or b != int(self_rows[a])]
        for j, (_, b) in enumerate(sorted(row)[:k]):
            index[a, j] = b
            prob[a, j] = cells[a, b]
    return index, prob


def same(a, b):
    return (np.array_equal(a[0], b[0])
            and np.array_equal(bits(a[1]), bits(b[1])))


class Case(object):
    """a coassign_expect subject: its specified queries (the subject's rq)
    against its members' resident rows"""

    def __init__(self, name):
        self.name = name
        self.sub = ce.subject(name)
        sub = self.sub
        self.M = sub.M
        ok = np.flatnonzero(sub.specified(sub.rq))
        self._ok = ok
        self.rq = sub.rq[ok]
        self.orcs = [m.orc for m in sub.members]
        self.n = len(self.orcs[0].assign)
        assert all(len(o.assign) == self.n for o in self.orcs)
        self.assigns = [np.asarray(o.assign, np.uint32).copy()
                        for o in self.orcs]
        self.slots = [slots_of(o) for o in self.orcs]
        self._cells = None
        self._law = None

    def cols(self):
        return self.sub.cols(self.rq)

    def r(self):
        """per engine [n_q, K_e] float32 of the specified queries"""
        return [r[self._ok] for r in self.sub.r()]

    def cells(self):
        if self._cells is None:
            self._cells = held_out_cells(self.r(), self.slots)
            self._cells.setflags(write=False)
        return self._cells

    def law(self):
        """-> (C64 [n_q, N], band)"""
        if self._law is None:
            C = band = infl = 0.0
            cols = self.cols()
            with np.errstate(all="ignore"):
                for m, s in zip(self.sub.members, self.slots):
                    assert np.array_equal(m.st.slot, s)
                    p, d = ce.law_parts(m.st, cols)
                    C = C + p[:, s]
                    band = band + (p * d)[:, s]
                    infl = infl + (p * (1 + d))[:, s]
            M = self.M
            self._law = (C / M, band / M + (M + 1) * fx.EPS * infl / M)
        return self._law


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]
