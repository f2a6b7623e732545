"""What dist_gibbs_predict must return, composed from the oracle's existing
entry points, and a float64 band around the log predictive density.

TEST INFRASTRUCTURE (imported by tests only).

The expectation (`expect`):
  scores   orc_mix_driver_score_value, then orc_mix_slave_score_value per
           feature with the QUERY's values (mixture.hpp:416-425)
  logp     orc_log_sum_exp of them (random.cc:78-92)
  draw     orc_sample_from_scores_overwrite on a state positioned by
           orc_rng_jump(seed_state, draw_base + q): the draw is then engine
           step draw_base + q + 1, the batch's convention
  map      the first index of maximal score
both as global ids.

The band (`logp_f64`): with s_k the float64 scores of tests/f64_scores.py,
b_k their bands, L = log sum_k exp(s_k), p_k = exp(s_k - L), bm = max b_k and
the float32 computation

    m^ = max s^_k;  l_k = fast_exp(fl(s^_k - m^));  T^ = (..(l_0 + l_1) ..)
    L^ = fl(fast_log(T^) + m^)

the distance |L^ - L| is at most the sum of

  scores      sum_k p_k b_k e^(2 bm): log-sum-exp's gradient is the softmax,
              whose weights move by at most e^(2 bm) along the segment
  exp, sum    delta = sum_k p_k r_k e^(2 bm) + eps sum_{j>=1} C_j, with
              r_k = eps g_k + FAST_EXP_REL[bin of g_k] for the gap
              g_k = m - s_k + 2 bm (the rounded subtraction, then the
              exponential table's measured error, tests/f64_sampling.py; the
              largest over the bins the gap may fall in; below -87 the whole
              term, which may be flushed or clamped), and one eps per rounded
              partial C_j of the K-term sum
  fast_log    the table's value is constant over a bucket of 2^9 binary32
              arguments: the largest |table - log| at the ends of every
              bucket T^ can fall in, T^ within T e^(+-2 bm) (1 +- delta);
              plus the roundings of (e + T[m]) ln2 as f64_scores.flog has them
  the add     eps |L|
and second-order terms, covered by the factor 1 / (1 - 2 K eps).  Nothing in
it is fitted to oracle or kernel output.
"""
import copy
import ctypes

import numpy as np

import f64_sampling as fs
import f64_scores as fx
import oracle_lib as ol
import workloads
from test_f64_scores import CONFIGS, SEED, build

OTHER = fx.OTHER
QSEED = 977            # the held-out rows' seed (the table's is workloads.SEED)
DRAW_SEED = 7
DRAW_BASE = 1000

# name: config, table rows, groups, empty groups, d, sweeps, LowEntropy
# dataset size, held-out rows, dim, unassigned table
CASES = {}
for _c in CONFIGS:
    CASES[_c] = dict(config=_c, n=2000, k=16, empty=3, d=0.5, sweeps=0)
    CASES[_c + "_swept"] = dict(config=_c, n=2000, k=16, empty=3, d=0.5,
                                sweeps=2)
CASES["le_dd"] = dict(config="dd", n=2000, k=16, empty=1, d=0.0, le=2000)
CASES["le_gp_nich"] = dict(config="gp_nich", n=2000, k=16, empty=1, d=0.0,
                           le=3000)
CASES["only_empty_k1"] = dict(config="dd_bb_gp", n=64, k=0, empty=1, d=0.5,
                              unassigned=True)
CASES["only_empty_k3"] = dict(config="gp_nich", n=64, k=0, empty=3, d=0.5,
                              unassigned=True)
CASES["k17"] = dict(config="nich2", n=500, k=16, empty=1, d=0.5)
CASES["dd256_k1025"] = dict(config="dd", n=4096, k=1024, empty=1, d=0.5,
                            dim=256, nq=256)
CASES["dpd10000_k8193"] = dict(config="dpd", n=24000, k=8192, empty=1, d=0.2,
                               dim=10000, nq=64)


class Case(object):
    """one state and its held-out rows: the oracle in that state, the float64
    restatement, and everything a GPU engine needs to reach the same state"""

    def __init__(self, name):
        c = dict(sweeps=0, le=None, nq=300, dim=None, unassigned=False)
        c.update(CASES[name])
        self.name = name
        self.__dict__.update(c)
        k = max(self.k, 1)
        osh, gsh, vals, assign = workloads.make(self.config, self.n, k,
                                                dim=self.dim)
        _, _, qvals, _ = workloads.make(self.config, self.nq, k, seed=QSEED,
                                        dim=self.dim)
        qvals = [q.copy() for q in qvals]
        for f, sh in enumerate(osh):
            if sh.kind in (ol.DD, ol.DPD):
                # the last value has no row in the table: zero count in
                # every group, and a held-out row carries it
                vals[f][vals[f] == sh.dim - 1] = 0
                qvals[f][0] = sh.dim - 1
            if sh.kind == ol.DPD and sh.p[1] > 0:
                # a value the table does not hold at all: OTHER (with
                # beta0 = 0 it has no mass and every score is -inf)
                qvals[f][[1, 2]] = OTHER
        self.osh, self.gsh, self.vals, self.assign0 = osh, gsh, vals, assign
        self.qvals = qvals
        self.alpha = 20.0 if self.sweeps else 1.0
        if self.unassigned:
            self.orc = ol.OracleMixture(self.alpha, self.d, osh)
            self.orc.init_empty(vals, self.empty)
            p2g = [self.orc.packed_to_global(i) for i in range(len(self.orc))]
            prior = ("py", float(np.float32(self.alpha)),
                     float(np.float32(self.d)))
            self.st = fx.State([v[:0] for v in vals], osh, [], p2g, prior)
        else:
            self.orc, self.st = build(osh, vals, assign, self.k, self.empty,
                                      self.alpha, self.d, self.sweeps,
                                      self.le)
        self.K = len(self.orc)
        self._expect = None
        self._f64 = None

    def engine(self):
        """a GPU engine brought to the oracle's state the same way"""
        from distributions_amd import engine
        kw = {} if self.le is None else dict(dataset_size=self.le)
        gpu = engine.Gibbs(self.alpha, self.d, self.gsh, **kw)
        if self.unassigned:
            gpu.load_rows_unassigned(self.vals, self.empty)
        else:
            gpu.load_rows(self.vals, self.assign0, self.k, self.empty)
            for s in range(self.sweeps):
                gpu.sweep(0, self.n, 16, SEED, draw_base=s * self.n)
            assert np.array_equal(gpu.assignments(), self.orc.assign)
        assert len(gpu) == self.K
        return gpu

    def expect(self):
        if self._expect is None:
            self._expect = expect(self.orc, self.qvals,
                                  ol.oracle().orc_rng_seed(DRAW_SEED),
                                  DRAW_BASE)
        return self._expect

    def f64(self):
        if self._f64 is None:
            self._f64 = logp_f64(self.st, self.qvals)
        return self._f64


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def query_words(orc, qvals):
    return [ol.value_words(s.kind, v) for s, v in zip(orc.shareds, qvals)]


def expect(orc, qvals, seed_state, draw_base):
    """-> dict(scores [nq, K] float32, logp [nq] float32, draw [nq], map [nq]
    (global ids, uint32), prior_total float32)"""
    L = orc.L
    K = len(orc)
    words = query_words(orc, qvals)
    nq = len(words[0]) if words else 0
    p2g = np.array([orc.packed_to_global(k) for k in range(K)], np.uint32)
    prior = np.zeros(K, np.float32)
    L.orc_mix_driver_score_value(orc.h, prior)
    out = dict(scores=np.zeros((nq, K), np.float32),
               logp=np.zeros(nq, np.float32), draw=np.zeros(nq, np.uint32),
               map=np.zeros(nq, np.uint32),
               prior_total=np.float32(L.orc_log_sum_exp(K, prior)))
    for q in range(nq):
        s = prior.copy()
        for f in range(orc.F):
            L.orc_mix_slave_score_value(orc.h, f, int(words[f][q]), s)
        out["scores"][q] = s
        out["logp"][q] = L.orc_log_sum_exp(K, s)
        out["map"][q] = p2g[int(np.argmax(s))]      # (the first maximum)
        st = ctypes.c_uint32(L.orc_rng_jump(seed_state, draw_base + q))
        out["draw"][q] = p2g[L.orc_sample_from_scores_overwrite(
            ctypes.byref(st), K, s.copy())]
    return out


# ---------------------------------------------------------------------------
# float64


def query_scores_f64(state, qcols):
    """Mixture::score_value of rows that are not in the table: the float64
    scores (and bands) of `state`'s groups at the query rows' values"""
    nq = len(qcols[0]) if qcols else 0
    q = copy.copy(state)
    q.cols = [np.asarray(c) for c in qcols]
    q.slot = np.zeros(nq, np.int64)     # (unused without removal)
    v, b, _ = q.scores(np.arange(nq), remove=False)
    return v, b


def _fast_log_excursion(lo, hi):
    """sup |fast_log(x) - log(x)| over the binary32 x in [lo, hi] (> 0): the
    table is constant over a bucket of 2^9 arguments and log is monotone, so
    the supremum is at an end of one of the buckets the interval meets"""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    if float(lo32) > lo:
        lo32 = np.nextafter(lo32, np.float32(0))
    if float(hi32) < hi:
        hi32 = np.nextafter(hi32, np.float32(np.inf))
    b0 = int(np.float32(lo32).view(np.uint32))
    b1 = int(np.float32(hi32).view(np.uint32))
    ends = []
    for bucket in range(b0 >> 9, (b1 >> 9) + 1):
        ends += [max(bucket << 9, b0), min((bucket << 9) | 0x1FF, b1)]
    x = np.array(ends, np.uint32).view(np.float32)
    et, A = fx._fast_log_parts(x)
    table = np.abs(A - np.log(x.astype(np.float64))).max()
    rounding = (np.abs(et) * (fx.EPS + abs(fx.LN2_F32 / fx.LN2 - 1.0)) * fx.LN2
                + fx.EPS * np.abs(A)).max()
    return float(table + rounding * (1 + 4 * fx.EPS))


def logp_f64(state, qcols):
    """-> (L [nq], band [nq], p [nq, K]): the float64 log-sum-exp of the
    float64 scores, the band of the module docstring, the responsibilities"""
    v, b = query_scores_f64(state, qcols)
    nq, K = v.shape
    m = v.max(1)
    w = np.exp(v - m[:, None])
    T = w.sum(1)
    Lv = np.log(T) + m
    p = w / T[:, None]
    bm = b.max(1)
    grow = np.exp(2 * bm)
    scores = (p * b).sum(1) * grow
    gap = m[:, None] - v
    lo_bin = np.clip(np.floor(gap - 2 * bm[:, None]), 0, 87).astype(int)
    hi_bin = np.clip(np.floor(gap + 2 * bm[:, None]), 0, 87).astype(int)
    rel_tab = np.append(fs.FAST_EXP_REL, 1.0)
    rel = np.maximum(rel_tab[lo_bin], rel_tab[hi_bin])
    for mid in range(1, 3):   # (a gap's uncertainty never spans 3 bins)
        rel = np.maximum(rel, rel_tab[np.minimum(lo_bin + mid, hi_bin)])
    r = fx.EPS * (gap + 2 * bm[:, None]) + rel
    C = np.cumsum(p, 1)
    delta = ((p * r).sum(1) * grow + 2 * K * fs.TINY / T
             + fx.EPS * C[:, 1:].sum(1) * grow)
    delta = delta * (1 + delta)
    band = np.zeros(nq)
    for q in range(nq):
        width = grow[q] * (1 + delta[q])
        band[q] = _fast_log_excursion(T[q] / width, T[q] * width)
    band = band + delta + scores + fx.EPS * np.abs(Lv)
    return Lv, band / (1.0 - 2.0 * K * fx.EPS), p


def excursion(got, case_):
    """|got - L| / band per held-out row"""
    Lv, band, _ = case_.f64()
    return np.abs(np.asarray(got, np.float64) - Lv) / band
