"""What dist_gibbs_coassign[_many] and dist_gibbs_responsibilities must return
-- the co-assignment of pairs of held-out rows over M engines -- composed from
the oracle's existing entry points, and a float64 band around it.

TEST INFRASTRUCTURE (imported by tests only).

The expectation (`Subject.expect`), per engine e and row a:
  scores    predict_expect.expect's (the driver's score_value plus every
            feature's, mixture.hpp:416-425)
  lik,total orc_scores_to_likelihoods (random.cc:94-103) on a copy
  r_e,a[k]  float32(lik[k] * (float32(1) / total)) in numpy float32, with
            subnormal results flushed to zero
  acc[a,b]  libm's fmaf through ctypes: acc = fmaf(r_e,a[k], r_e,b[k], acc)
            from 0, engines ascending, k ascending (a float64 emulation is
            double rounding and is not used)
  out[a,b]  float32(acc) / float32(M)
With the targets the queries only a <= b is chained and mirrored: fmaf is
commutative in its factors.

The float64 law (`Subject.law`): C64 = (1/M) sum_e p_e p_e^T with
predict_expect.logp_f64's responsibilities p.

The band, derived, nothing fitted: with bm_a the row's largest score band and
r_ak = eps g_ak + FAST_EXP_REL[bin of g_ak] the subtraction's rounding plus
the exponential table's error as predict_expect.logp_f64 has them (g the gap
to the maximum, widened by 2 bm),

  |r^_ak - p_ak| <= p_ak d_ak,
  d_ak = e^(2 bm_a) (1 + r_ak)(1 + K eps)(1 + 2 eps) / (1 - sum_j p_aj r_aj) - 1

(the scores move the softmax by at most e^(2 bm); the likelihood's own error;
the K-term float sum; the division and the multiply; the total's relative
error in the denominator).  A term whose exponential or whose product may
flush is charged in full (d_ak >= 1).  A cell's band is then

  (1/M) sum_e sum_k p_ak p_bk (d_ak + d_bk + d_ak d_bk)
  + ((K_total + 1) eps + eps) (1/M) sum_e sum_k p_ak p_bk (1 + d_ak)(1 + d_bk)

the chain's K_total roundings over the inflated sum, and one eps for the
division by M.
"""
import ctypes
import ctypes.util

import numpy as np

import ensemble_expect as ee
import f64_sampling as fs
import f64_scores as fx
import oracle_lib as ol
import predict_expect as pe

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
fmaf = _libm.fmaf
fmaf.restype = ctypes.c_float
fmaf.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]

TINY32 = np.float32(np.finfo(np.float32).tiny)
# cells in (0, 2^-100) are compared as got < 2^-99 (whether a product inside
# the matrix unit flushes is not documented); at most 1 % of a case's cells
UNDERFLOW, UNDERFLOW_GOT, UNDERFLOW_SHARE = 2.0 ** -100, 2.0 ** -99, 0.01

SINGLES = ["dd", "gp_nich", "dd_bb_gp", "dpd", "bnb", "le_dd", "le_gp_nich",
           "only_empty_k3", "dd_swept", "gp_nich_swept", "nich2", "dpd_swept",
           "dd256_k1025"]
ENSEMBLES = {"ens3_dd_bb_gp": "dd_bb_gp", "ens3_gp_nich": "gp_nich"}
# eight_expect's subjects over the eight-feature list (100 held-out rows):
# one engine after two sweeps, and the ensemble of three
WIDE = ["eight_swept", "eight3"]
NAMES = SINGLES + sorted(ENSEMBLES) + WIDE


def flush(x):
    x = np.asarray(x, np.float32).copy()
    x[np.abs(x) < TINY32] = 0
    return x


def responsibilities(scores, reverse_sum=False):
    """[n, K] float32 scores -> r [n, K] float32 as the module docstring has
    them.  reverse_sum: the total summed in the other order (NOT a bug: the
    float64 band must hold it)"""
    L = ol.oracle()
    n, K = scores.shape
    r = np.zeros((n, K), np.float32)
    with np.errstate(all="ignore"):
        for q in range(n):
            lik = np.ascontiguousarray(scores[q], np.float32).copy()
            total = np.float32(L.orc_scores_to_likelihoods(K, lik))
            if reverse_sum:
                total = np.float32(0)
                for x in lik[::-1]:
                    total = np.float32(total + x)
            inv = np.float32(1) / total
            r[q] = flush(lik * inv)
    return r


def chain(rq, rt, sym):
    """rq, rt: per engine [n_q, K_e] / [n_t, K_e] float32 -> [n_q, n_t]
    float32, ONE fmaf chain per cell, divided by float32(M)"""
    M = len(rq)
    n_q, n_t = rq[0].shape[0], rt[0].shape[0]
    A = [r.astype(np.float64).tolist() for r in rq]
    B = [r.astype(np.float64).tolist() for r in rt]
    out = np.zeros((n_q, n_t), np.float32)
    for a in range(n_q):
        for b in range(a if sym else 0, n_t):
            acc = 0.0
            for e in range(M):
                for x, y in zip(A[e][a], B[e][b]):
                    acc = fmaf(x, y, acc)
            out[a, b] = acc
            if sym:
                out[b, a] = acc
    with np.errstate(all="ignore"):
        return (out / np.float32(M)).astype(np.float32)


def law_parts(state, cols):
    """-> (p [n, K], d [n, K]) of the module docstring for one engine"""
    v, b = pe.query_scores_f64(state, cols)
    n, K = v.shape
    with np.errstate(all="ignore"):
        m = v.max(1)
        w = np.exp(v - m[:, None])
        p = w / w.sum(1)[:, None]
        bm = b.max(1)
        gap = m[:, None] - v
        lo_bin = np.clip(np.floor(gap - 2 * bm[:, None]), 0, 87).astype(int)
        hi_bin = np.clip(np.floor(gap + 2 * bm[:, None]), 0, 87).astype(int)
        rel_tab = np.append(fs.FAST_EXP_REL, 1.0)
        rel = np.maximum(rel_tab[lo_bin], rel_tab[hi_bin])
        for mid in range(1, 3):
            rel = np.maximum(rel, rel_tab[np.minimum(lo_bin + mid, hi_bin)])
        r = fx.EPS * (gap + 2 * bm[:, None]) + rel
        d = (np.exp(2 * bm)[:, None] * (1 + r) * (1 + K * fx.EPS)
             * (1 + 2 * fx.EPS) / (1 - (p * r).sum(1))[:, None] - 1)
        # the product lik * inv may flush where it can come under 2 tiny
        d = np.where(p * (1 + d) < 4 * float(TINY32), np.maximum(d, 1.0), d)
    return p, d


def law_f64(states, qcols, tcols, variant=None, counts=None):
    """-> (C64 [n_q, n_t], band) of the module docstring.
    variant: a planted bug instead of the law (band None then):
      "unnormalised"  likelihoods exp(s - max), never divided by their total
      "no_mean"       the sum over the engines, 1/M missing
      "hard"          the mean per engine AFTER rounding: each engine's rows
                      rounded to their first maximal group (0 / 1 agreement)
      "no_empty"      empty groups dropped (counts: per engine)"""
    M = len(states)
    C = band = infl = 0.0
    k_total = 0
    with np.errstate(all="ignore"):
        for e, st in enumerate(states):
            pa, da = law_parts(st, qcols)
            pb, db = law_parts(st, tcols)
            k_total += pa.shape[1]
            if variant == "unnormalised":
                pa = pa / pa.max(1)[:, None]
                pb = pb / pb.max(1)[:, None]
            elif variant == "hard":
                pa = np.eye(pa.shape[1])[pa.argmax(1)]
                pb = np.eye(pb.shape[1])[pb.argmax(1)]
            elif variant == "no_empty":
                live = np.asarray(counts[e]) > 0
                pa, pb = pa * live, pb * live
            C = C + pa @ pb.T
            band = band + ((pa * da) @ pb.T + pa @ (pb * db).T
                           + (pa * da) @ (pb * db).T)
            infl = infl + (pa * (1 + da)) @ (pb * (1 + db)).T
    if variant == "no_mean":
        return C, None
    if variant is not None:
        return C / M, None
    return C / M, band / M + (k_total + 2) * fx.EPS * infl / M


class Subject(object):
    """a case of predict_expect (M = 1) or an ensemble of ensemble_expect
    (M = 3) with the rows a call takes: queries `rq`, targets `rt`"""

    def __init__(self, name):
        self.name = name
        self.many = name in ENSEMBLES or name == "eight3"
        if name in WIDE:
            import eight_expect as xe
            self.src = xe.eight3() if self.many else xe.case(name)
        elif self.many:
            self.src = ee.Ensemble(ENSEMBLES[name], ee.SPECS3)
        else:
            self.src = pe.case(name)
        self.members = self.src.members if self.many else [self.src]
        self.M = len(self.members)
        self.qvals = self.src.qvals
        big = max(m.K for m in self.members) > 256
        self.rq = np.arange(40 if big else 70)
        self.rt = np.arange(100, 125 if big else 145)
        if name in WIDE:
            self.rq, self.rt = np.arange(56), np.arange(56, 100)
        self._r = None
        self._expect = {}
        self._law = {}

    def cols(self, rows):
        return [np.ascontiguousarray(c[rows]) for c in self.qvals]

    def engines(self):
        return [m.engine() for m in self.members]

    def scores(self):
        """per engine [nq_all, K_e] float32"""
        if self.many:
            return [p["scores"] for p in self.src.expect()["per_member"]]
        return [self.src.expect()["scores"]]

    def logp(self):
        if self.many:
            return [p["logp"] for p in self.src.expect()["per_member"]]
        return [self.src.expect()["logp"]]

    def specified(self, rows):
        """rows whose logp is finite on every engine (the others' cells are
        unspecified)"""
        ok = np.ones(len(rows), bool)
        for lp in self.logp():
            ok &= np.isfinite(lp[rows])
        return ok

    def r(self):
        """per engine: r of the rows rq and rt together, rq first"""
        if self._r is None:
            rows = np.concatenate([self.rq, self.rt])
            self._r = [responsibilities(s[rows]) for s in self.scores()]
        return self._r

    def expect(self, sym):
        if sym not in self._expect:
            n = len(self.rq)
            rq = [r[:n] for r in self.r()]
            rt = rq if sym else [r[n:] for r in self.r()]
            self._expect[sym] = chain(rq, rt, sym)
        return self._expect[sym]

    def law(self, sym):
        if sym not in self._law:
            self._law[sym] = law_f64(
                [m.st for m in self.members], self.cols(self.rq),
                self.cols(self.rq if sym else self.rt))
        return self._law[sym]

    def mask(self, sym):
        """[n_q, n_t] bool: the specified cells"""
        return np.outer(self.specified(self.rq),
                        self.specified(self.rq if sym else self.rt))


_SUBJECTS = {}


def subject(name):
    if name not in _SUBJECTS:
        _SUBJECTS[name] = Subject(name)
    return _SUBJECTS[name]


def same_cells(got, want, mask):
    """the comparison of the module's header: bits, but for cells with
    0 < want < 2^-100, which pass with got < 2^-99 -> (ok, share of cells
    that took that exit)"""
    got = np.asarray(got, np.float32)
    want = np.asarray(want, np.float32)
    soft = mask & (want > 0) & (want < UNDERFLOW)
    hard = mask & ~soft
    ok = (np.array_equal(got[hard].view(np.uint32), want[hard].view(np.uint32))
          and bool(np.all(got[soft] < UNDERFLOW_GOT))
          and bool(np.all(got[soft] >= 0)))
    return ok, float(soft.sum()) / max(int(mask.sum()), 1)
