"""What dist_gibbs_predict_many must return -- the predictive of held-out rows
averaged over M engines -- composed from the oracle's existing entry points,
and a float64 band around it.

TEST INFRASTRUCTURE (imported by tests only).

The members of an ensemble are M oracle states of ONE feature list that share
nothing else: their own rows (seed), group count, empty groups, alpha, d,
sweeps and hyper-parameters.  Their GPU twins are built the way
predict_expect.Case.engine builds its engine.

The expectation (`expect_many`), per held-out row q:
  w[e][q]   predict_expect.expect's logp on member e; under LowEntropy minus
            that member's prior_total, one float32 subtraction
  logp[q]   orc_log_sum_exp(w[.][q]) - orc_fast_log(M), in float32
  member    orc_sample_from_scores_overwrite over w[.][q] on a state
            positioned by orc_rng_jump(member_seed_state, draw_base + q): the
            draw is engine step draw_base + q + 1 of the member stream; for
            "map" the first index that attains orc_vector_max
  group     the chosen member's own draw / first maximum of row q, as
            predict_expect.expect gives them (global ids of THAT member)

The float64 law (`law_f64`): L[q] = logsumexp_e(W_e[q]) - log M with
W_e = L_e (predict_expect.logp_f64), under LowEntropy minus the float64
log-sum-exp of the member's prior scores.

The band: predict_expect.logp_f64's second stage (the log-sum-exp of K
float32 scores, each within its band of a float64 score) applied to the M
member values (W_e, band_e) in the place of the scores (s_k, b_k) -- the
fold over members is the same float32 computation as the fold over groups --
plus |orc_fast_log(M) - log M| and one eps |L| for the subtraction.  Under
LowEntropy band_e is the member's band plus its prior total's (the same
second stage over the prior scores alone) plus one eps for the subtraction.
Nothing in it is fitted to oracle or kernel output.
"""
import copy
import ctypes
import math

import numpy as np

import f64_scores as fx
import oracle_lib as ol
import predict_expect as pe
import workloads
from test_f64_scores import SEED, build

DRAW_SEED = pe.DRAW_SEED
MEMBER_SEED = pe.DRAW_SEED + 1
DRAW_BASE = pe.DRAW_BASE

# three members that differ in everything but the feature list
SPECS3 = [dict(k=4, empty=1, alpha=1.0, d=0.0, sweeps=0),
          dict(k=17, empty=3, alpha=20.0, d=0.5, sweeps=1),
          dict(k=41, empty=2, alpha=5.0, d=0.25, sweeps=2)]


def member_shareds(config, e, dim=None, beta0=None):
    """member e's hyper-parameters for `config`: workloads.make's, scaled by
    (1 + e / 2) (exact in float32) -> (oracle shareds, engine shareds)"""
    from distributions_amd import engine
    osh, _, _, _ = workloads.make(config, 1, 1, dim=dim)
    g = 1.0 + 0.5 * e
    oo, gg = [], []
    for s in osh:
        p = [float(x) for x in s.p]
        if s.kind == ol.DD:
            a = [float(s.alphas[i]) * g for i in range(s.dim)]
            oo.append(ol.make_shared(ol.DD, alphas=a))
            gg.append(engine.dd_shared(a))
        elif s.kind == ol.BB:
            oo.append(ol.make_shared(ol.BB, alpha=p[0] * g, beta=p[1]))
            gg.append(engine.bb_shared(p[0] * g, p[1]))
        elif s.kind == ol.GP:
            oo.append(ol.make_shared(ol.GP, alpha=p[0] * g, inv_beta=p[1]))
            gg.append(engine.gp_shared(p[0] * g, p[1]))
        elif s.kind == ol.NICH:
            kw = dict(mu=p[0] + 0.25 * e, kappa=p[1], sigmasq=p[2] * g,
                      nu=p[3])
            oo.append(ol.make_shared(ol.NICH, **kw))
            gg.append(engine.nich_shared(kw["mu"], kw["kappa"],
                                         kw["sigmasq"], kw["nu"]))
        elif s.kind == ol.BNB:
            oo.append(ol.make_shared(ol.BNB, alpha=p[0] * g, beta=p[1],
                                     r=p[2]))
            gg.append(engine.bnb_shared(p[0] * g, p[1], int(p[2])))
        else:
            betas = np.array([s.betas[i] for i in range(s.dim)], np.float32)
            b0 = p[1] if beta0 is None else beta0[e]
            oo.append(ol.make_shared(ol.DPD, alpha=p[0] * g, betas=betas,
                                     beta0=b0))
            gg.append(engine.dpd_shared(p[0] * g, betas, b0))
    return oo, gg


class Member(object):
    """one oracle state, its float64 restatement and what its GPU twin needs"""

    def __init__(self, config, e, spec, n, le, dim, beta0):
        self.__dict__.update(spec)
        self.n, self.le = n, le
        k = max(self.k, 1)
        _, _, vals, assign = workloads.make(config, n, k,
                                            seed=workloads.SEED + 31 * e,
                                            dim=dim)
        self.osh, self.gsh = member_shareds(config, e, dim, beta0)
        self.vals, self.assign0 = vals, assign
        if self.k == 0:       # only empty groups, every row unassigned
            self.orc = ol.OracleMixture(self.alpha, self.d, self.osh)
            self.orc.init_empty(vals, self.empty)
            p2g = [self.orc.packed_to_global(i) for i in range(len(self.orc))]
            prior = ("py", float(np.float32(self.alpha)),
                     float(np.float32(self.d)))
            self.st = fx.State([v[:0] for v in vals], self.osh, [], p2g,
                               prior)
        else:
            self.orc, self.st = build(self.osh, vals, assign, self.k,
                                      self.empty, self.alpha, self.d,
                                      self.sweeps, le)
        self.K = len(self.orc)

    def engine(self):
        from distributions_amd import engine
        kw = {} if self.le is None else dict(dataset_size=self.le)
        gpu = engine.Gibbs(self.alpha, self.d, self.gsh, **kw)
        if self.k == 0:
            gpu.load_rows_unassigned(self.vals, self.empty)
        else:
            gpu.load_rows(self.vals, self.assign0, self.k, self.empty)
            for s in range(self.sweeps):
                gpu.sweep(0, self.n, 16, SEED, draw_base=s * self.n)
            assert np.array_equal(gpu.assignments(), self.orc.assign)
        assert len(gpu) == self.K
        return gpu


class Ensemble(object):
    def __init__(self, config, specs, n=600, nq=300, le=None, dim=None,
                 beta0=None, other=()):
        self.config, self.le, self.nq = config, le, nq
        self.members = [Member(config, e, s, s.get("n", n), le, dim, beta0)
                        for e, s in enumerate(specs)]
        self.M = len(self.members)
        _, _, q, _ = workloads.make(config, nq, 1, seed=pe.QSEED, dim=dim)
        self.qvals = [c.copy() for c in q]
        for i in other:       # DPD: values no member's table holds
            self.qvals[0][i] = pe.OTHER
        self._expect = {}
        self._f64 = None

    def engines(self):
        return [m.engine() for m in self.members]

    def expect(self, draw_base=DRAW_BASE):
        if draw_base not in self._expect:
            L = ol.oracle()
            self._expect[draw_base] = expect_many(
                [m.orc for m in self.members], self.qvals,
                L.orc_rng_seed(DRAW_SEED), L.orc_rng_seed(MEMBER_SEED),
                draw_base, self.le is not None)
        return self._expect[draw_base]

    def f64(self):
        if self._f64 is None:
            self._f64 = law_f64([m.st for m in self.members], self.qvals,
                                self.le is not None)
        return self._f64


def first_maximum(col):
    """the first index that attains orc_vector_max (x > max moves it)"""
    arg, mx = 0, col[0]
    for e in range(len(col)):
        if col[e] > mx:
            arg, mx = e, col[e]
    return arg


def fold(w, member_seed_state, draw_base):
    """the fold over the members of the planes w [M, n] -> (logp, member
    draws, first maxima)"""
    L = ol.oracle()
    M, n = w.shape
    log_m = np.float32(L.orc_fast_log(float(M)))
    logp = np.zeros(n, np.float32)
    draw = np.zeros(n, np.uint32)
    first = np.zeros(n, np.uint32)
    with np.errstate(invalid="ignore"):
        for q in range(n):
            col = np.ascontiguousarray(w[:, q], np.float32)
            logp[q] = np.float32(L.orc_log_sum_exp(M, col)) - log_m
            first[q] = first_maximum(col)
            st = ctypes.c_uint32(L.orc_rng_jump(member_seed_state,
                                                draw_base + q))
            draw[q] = L.orc_sample_from_scores_overwrite(ctypes.byref(st), M,
                                                         col.copy())
    return logp, draw, first


def expect_many(orcs, qvals, seed_state, member_seed_state, draw_base, le):
    """-> dict(w [M, nq] float32, prior_totals [M], logp [nq], member_draw,
    member_map, group_draw, group_map (uint32; groups as the chosen member's
    global ids), per_member: predict_expect.expect of each member)"""
    per = [pe.expect(o, qvals, seed_state, draw_base) for o in orcs]
    totals = np.array([p["prior_total"] for p in per], np.float32)
    w = np.stack([p["logp"] for p in per]).astype(np.float32)
    if le:
        with np.errstate(invalid="ignore"):
            w = (w - totals[:, None]).astype(np.float32)
    logp, draw, first = fold(w, member_seed_state, draw_base)
    rows = np.arange(w.shape[1])
    draws = np.stack([p["draw"] for p in per])
    maps = np.stack([p["map"] for p in per])
    return dict(w=w, prior_totals=totals, logp=logp, member_draw=draw,
                member_map=first, group_draw=draws[draw, rows],
                group_map=maps[first, rows], per_member=per)


# ---------------------------------------------------------------------------
# float64


class _Given(object):
    """stands in for a State in predict_expect.logp_f64, whose second stage
    then runs over the values and bands given here"""

    def __init__(self, v, b):
        self.v, self.b = np.asarray(v, np.float64), np.asarray(b, np.float64)

    def scores(self, rows, remove=True):
        return self.v[rows], self.b[rows], None


def lse_band(v, b):
    """predict_expect.logp_f64's second stage over v [n, K] within b:
    -> (L [n], band [n], p [n, K])"""
    return pe.logp_f64(_Given(v, b), [np.zeros(len(v), np.uint32)])


def prior_total_f64(state):
    """the float64 log-sum-exp of the clustering model's scores alone and the
    band of orc_log_sum_exp of their float32 versions"""
    bare = copy.copy(state)
    bare.feats, bare.cols, bare.stats = [], [], []
    bare.slot = np.zeros(1, np.int64)
    v, b, _ = bare.scores(np.arange(1), remove=False)
    Lp, band, _ = lse_band(v, b)
    return float(Lp[0]), float(band[0])


def members_f64(states, qvals, le):
    """-> (W [nq, M], band [nq, M]): each member's float64 log predictive
    density of every held-out row and the band of its float32 value"""
    W, B = [], []
    for st in states:
        Lv, band, _ = pe.logp_f64(st, qvals)
        if le:
            Lp, bp = prior_total_f64(st)
            Lv = Lv - Lp
            band = band + bp + fx.EPS * np.abs(Lv)
        W.append(Lv)
        B.append(band)
    return np.stack(W, 1), np.stack(B, 1)


def law_f64(states, qvals, le, variant=None):
    """-> (L [nq], band [nq], r [nq, M]): the float64 log of the mean over the
    members of their predictive densities, the band of the module docstring,
    the member responsibilities exp(W_e - L) / M.

    variant: a planted bug instead of the law (no band then):
      "mean_of_logs"   the mean of the log densities
      "no_log_m"       the log of the SUM of the densities
      "unnormalised"   LowEntropy without the members' own normalisation"""
    M = len(states)
    if variant == "unnormalised":
        W, B = members_f64(states, qvals, False)
    else:
        W, B = members_f64(states, qvals, le)
    if variant == "mean_of_logs":
        return W.mean(1), None, None
    Lv, band, r = lse_band(W, B)
    if variant == "no_log_m":
        return Lv, None, None
    log_m = math.log(M)
    Lv = Lv - log_m
    table = abs(float(np.float32(ol.oracle().orc_fast_log(float(M))))
                - log_m)
    return Lv, band + table + fx.EPS * np.abs(Lv), r


def excursion(got, ens):
    Lv, band, _ = ens.f64()
    return np.abs(np.asarray(got, np.float64) - Lv) / band
