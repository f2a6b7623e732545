"""What dist_gibbs_predict_feature must return, composed from the oracle's
existing entry points as tests/predict_expect.py composes predict's, and the
float64 values it is held to.

TEST INFRASTRUCTURE (imported by tests only).

The expectation (`expect`), per query row q, target t, candidates cand[0..C)
and mask observed[q] (bit t ignored; None: everything else observed):
  scores_c orc_mix_driver_score_value, then in feature order
           orc_mix_slave_score_value of every OBSERVED feature with the
           query's value and, at position t, of the target with cand[c]
           (mixture.hpp:416-425); an unobserved feature is skipped
  joint    orc_log_sum_exp of scores_c (random.cc:78-92)
  base     orc_log_sum_exp of the same fold without the target
  draw     orc_sample_from_scores_overwrite over a COPY of joint[q] on a state
           positioned by orc_rng_jump(seed_state, draw_base + q): engine step
           draw_base + q + 1, the batch's convention; an index into cand
  map      the first index of maximal joint[q]

States and engines are predict_expect's cases, plus one feature list of this
module's own, "mixed4": [BB, DD(5), NICH, DD(70)] at K = 16 + 3 empty, as
loaded and after 2 sweeps -- a categorical target in the middle, two-float
terms after it, a ragged small domain, a domain of two strips of 64 with a
ragged end.
"""
import copy
import ctypes

import numpy as np

import oracle_lib as ol
import predict_expect as pe
from test_f64_scores import build

OTHER = pe.OTHER
COUNT_CANDIDATES = [0, 1, 2, 5, 9, 40, 300]   # 300: beyond the value tables
REAL_CANDIDATES = [-2.5, 0.0, 0.3, 7.0]


def make_mixed4(n, k, seed):
    """[BB, DD(5), NICH, DD(70)], built like workloads.make"""
    from distributions_amd import engine
    rng = np.random.default_rng(seed)
    assign = (np.arange(n) % k).astype(np.uint32)
    vals = [(rng.random(n) < 0.4).astype(np.uint32),
            rng.integers(0, 5, n).astype(np.uint32),
            rng.normal(1, 2, n).astype(np.float32),
            rng.integers(0, 70, n).astype(np.uint32)]
    a5 = [0.5, 1.0, 0.25, 2.0, 0.75]
    osh = [ol.make_shared(ol.BB, alpha=0.5, beta=2.0),
           ol.make_shared(ol.DD, alphas=a5),
           ol.make_shared(ol.NICH, mu=0.0, kappa=1.0, sigmasq=1.0, nu=1.0),
           ol.make_shared(ol.DD, alphas=[0.5] * 70)]
    gsh = [engine.bb_shared(0.5, 2.0), engine.dd_shared(a5),
           engine.nich_shared(0.0, 1.0, 1.0, 1.0),
           engine.dd_shared([0.5] * 70)]
    return osh, gsh, vals, assign


class Mixed4(pe.Case):
    """predict_expect.Case over this module's feature list"""

    def __init__(self, name, sweeps):
        self.name = name
        self.config = "mixed4"
        self.n, self.k, self.empty, self.d = 2000, 16, 3, 0.5
        self.sweeps, self.le, self.nq, self.dim = sweeps, None, 300, None
        self.unassigned = False
        self.osh, self.gsh, self.vals, self.assign0 = make_mixed4(
            self.n, self.k, pe.workloads.SEED)
        _, _, qvals, _ = make_mixed4(self.nq, self.k, pe.QSEED)
        self.qvals = [q.copy() for q in qvals]
        self.alpha = 20.0 if sweeps else 1.0
        self.orc, self.st = build(self.osh, self.vals, self.assign0, self.k,
                                  self.empty, self.alpha, self.d, sweeps,
                                  None)
        self.K = len(self.orc)
        self._expect = None
        self._f64 = None


_OWN = {"mixed4": 0, "mixed4_swept": 2}
_CASES = {}


def case(name):
    if name in _OWN:
        if name not in _CASES:
            _CASES[name] = Mixed4(name, _OWN[name])
        return _CASES[name]
    return pe.case(name)


def default_candidates(shared):
    """the whole domain of a DD, BB or DPD target"""
    if shared.kind == ol.DD:
        return np.arange(shared.dim, dtype=np.uint32)
    if shared.kind == ol.BB:
        return np.arange(2, dtype=np.uint32)
    if shared.kind == ol.DPD:
        return np.append(np.arange(shared.dim, dtype=np.uint32),
                         np.uint32(OTHER))
    raise ValueError("this target needs a candidate list")


def candidates_for(shared):
    """the issue's candidate lists by the target's kind (None: the default)"""
    if shared.kind in (ol.GP, ol.BNB):
        return np.array(COUNT_CANDIDATES, np.uint32)
    if shared.kind == ol.NICH:
        return np.array(REAL_CANDIDATES, np.float32)
    return None


def random_masks(n, F, seed):
    """one mask per row: random bits, row 0 nothing observed, row 1
    everything, junk above bit F (which nothing may read)"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 1 << F, n).astype(np.uint32)
    m[0] = 0
    if n > 1:
        m[1] = (1 << F) - 1
    m[2::3] |= np.uint32(0xA5000000)
    return m


def expect(orc, qvals, observed, target, cand, seed_state, draw_base):
    """-> dict(joint [nq, C] float32, base [nq] float32, draw [nq] uint32,
    map [nq] uint32).  cand: values of the target (None: its whole domain);
    observed: uint32 masks or None; qvals[target] may be None."""
    L = orc.L
    K = len(orc)
    F = orc.F
    sh = orc.shareds
    if cand is None:
        cand = default_candidates(sh[target])

    def as_words(f, v):
        w = ol.value_words(sh[f].kind, v).copy()
        if sh[f].kind == ol.DPD:
            # dpd.hpp:534-542: a value the table does not hold is OTHER
            w[w >= sh[f].dim] = OTHER
        return w

    cw = as_words(target, cand)
    words = [None if (v is None and f == target) else as_words(f, v)
             for f, v in enumerate(qvals)]
    nq = len(next(w for w in words if w is not None)) \
        if observed is None else len(observed)
    C = len(cw)
    prior = np.zeros(K, np.float32)
    L.orc_mix_driver_score_value(orc.h, prior)
    out = dict(joint=np.zeros((nq, C), np.float32),
               base=np.zeros(nq, np.float32), draw=np.zeros(nq, np.uint32),
               map=np.zeros(nq, np.uint32))
    for q in range(nq):
        ob = (1 << F) - 1 if observed is None else int(observed[q])
        before = prior.copy()
        for f in range(target):
            if (ob >> f) & 1:
                L.orc_mix_slave_score_value(orc.h, f, int(words[f][q]),
                                            before)

        def finish(s):
            for f in range(target + 1, F):
                if (ob >> f) & 1:
                    L.orc_mix_slave_score_value(orc.h, f, int(words[f][q]),
                                                s)
            return L.orc_log_sum_exp(K, s)

        out["base"][q] = finish(before.copy())
        for c in range(C):
            s = before.copy()
            L.orc_mix_slave_score_value(orc.h, target, int(cw[c]), s)
            out["joint"][q, c] = finish(s)
        j = out["joint"][q]
        out["map"][q] = int(np.argmax(j))          # (the first maximum)
        st = ctypes.c_uint32(L.orc_rng_jump(seed_state, draw_base + q))
        out["draw"][q] = L.orc_sample_from_scores_overwrite(
            ctypes.byref(st), C, j.copy())
    return out


# ---------------------------------------------------------------------------
# float64


def without(state, drop):
    """a copy of the float64 state that leaves the features in `drop` out
    (f64_scores.State folds every feature it holds)"""
    keep = [f for f in range(len(state.feats)) if f not in drop]
    s = copy.copy(state)
    s.feats = [state.feats[f] for f in keep]
    s.cols = [state.cols[f] for f in keep]
    s.stats = [state.stats[f] for f in keep]
    return s, keep


def completed(qvals, target, value, kind):
    """the query columns with the target's filled with one value"""
    n = len(next(v for f, v in enumerate(qvals) if f != target)) \
        if len(qvals) > 1 else len(qvals[target])
    dtype = np.float32 if kind == ol.NICH else np.uint32
    return [np.full(n, value, dtype) if f == target else v
            for f, v in enumerate(qvals)]


def base_f64(state, qvals, target):
    """-> (L [nq], band [nq]) of the fold without the target: the float64
    log marginal of the other cells and predict_expect.logp_f64's band over
    the feature list without the target"""
    s, keep = without(state, {target})
    Lv, band, _ = pe.logp_f64(s, [qvals[f] for f in keep])
    return Lv, band
