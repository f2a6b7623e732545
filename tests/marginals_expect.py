"""What dist_gibbs_marginals[_many] must return -- the log marginals of S
feature subsets per held-out row, on one engine and averaged over M engines --
composed from the oracle's existing entry points, the float64 law it is held
to, and the exact mutual information dist_gibbs_relate_many estimates.

TEST INFRASTRUCTURE (imported by tests only).

The expectation (`expect`), per query row q and mask masks[s] (bit f: feature
f is named; the masks are shared by all rows):
  scores   orc_mix_driver_score_value, then in feature order
           orc_mix_slave_score_value of every NAMED feature with the query's
           value (mixture.hpp:416-425); an unnamed feature is skipped -- how
           feature_expect.expect builds `base`
  w[q][s]  orc_log_sum_exp of them (random.cc:78-92)
`expect_many`: w[e] per member, under LowEntropy minus that member's prior
total (one float32 subtraction), and ensemble_expect.fold over the planes
[M, n * S]: orc_log_sum_exp minus orc_fast_log(M), in float32.

The float64 law (`law_f64`): per member predict_expect.logp_f64 on
feature_expect.without(state, the features the mask does not name), for mask
0 ensemble_expect.prior_total_f64; under LowEntropy minus the member's
float64 prior total (its band and one eps added); then
ensemble_expect.lse_band over the members, - log M with the fast_log(M) table
term and one eps: exactly how feature_many_expect.law_f64 builds `base`.
Nothing in a band is fitted to oracle or kernel output.

`EIGHT`: a list of this module's own with one feature of every kind and two
more DDs, [DD(5), BB, GP, NICH, DD(70), BNB, DPD(20), DD(3)] -- the widest
staging the kernel can have, 17 planes -- with its own rows, query rows and
three member specs in the manner of ensemble_expect.SPECS3.

`enumerate_pair`: the exact float64 mutual information of a pair of
categorical features under the ensemble's predictive, by enumerating the
pair's domain with every other feature unobserved.
"""
import copy
import math

import numpy as np

import ensemble_expect as ee
import f64_scores as fx
import feature_expect as fe
import feature_many_expect as fm
import oracle_lib as ol
import predict_expect as pe
from test_f64_scores import build

OTHER = pe.OTHER


def all_masks(F):
    """every subset of F features, 0 included"""
    return np.arange(1 << F, dtype=np.uint32)


def singles_and_pairs(F):
    """{i} for i < F, then {i, j} for i < j in row-major order:
    dist_gibbs_relate's masks"""
    m = [1 << i for i in range(F)]
    m += [(1 << i) | (1 << j) for i in range(F) for j in range(i + 1, F)]
    return np.array(m, np.uint32)


def query_words(orc, qvals):
    """the query columns as the scorers take them (None stays None; a DPD
    value the table does not hold is OTHER, dpd.hpp:534-542)"""
    words = []
    for s, v in zip(orc.shareds, qvals):
        if v is None:
            words.append(None)
            continue
        w = ol.value_words(s.kind, v).copy()
        if s.kind == ol.DPD:
            w[w >= s.dim] = OTHER
        words.append(w)
    return words


def expect(orc, qvals, masks, nq=None):
    """-> w [nq, S] float32.  Each distinct (mask, named words) is scored
    once: the fold depends on nothing else."""
    L = orc.L
    K, F = len(orc), orc.F
    words = query_words(orc, qvals)
    if nq is None:
        nq = len(next(w for w in words if w is not None))
    prior = np.zeros(K, np.float32)
    L.orc_mix_driver_score_value(orc.h, prior)
    out = np.zeros((nq, len(masks)), np.float32)
    seen = {}
    for s, mask in enumerate(masks):
        mask = int(mask)
        named = [f for f in range(F) if (mask >> f) & 1]
        for q in range(nq):
            key = (mask,) + tuple(int(words[f][q]) for f in named)
            if key not in seen:
                sc = prior.copy()
                for f in named:
                    L.orc_mix_slave_score_value(orc.h, f, key[1 + named.index(f)],
                                                sc)
                seen[key] = np.float32(L.orc_log_sum_exp(K, sc))
            out[q, s] = seen[key]
    return out


def expect_many(orcs, qvals, masks, le, nq=None):
    """-> dict(w [M, nq, S] float32, prior_totals [M], logp [nq, S])"""
    w = np.stack([expect(o, qvals, masks, nq) for o in orcs])
    totals = np.array([fm.prior_total(o) for o in orcs], np.float32)
    if le:
        with np.errstate(invalid="ignore"):
            w = (w - totals[:, None, None]).astype(np.float32)
    M, n, S = w.shape
    logp, _, _ = ee.fold(w.reshape(M, n * S), 1, 0)
    return dict(w=w, prior_totals=totals, logp=logp.reshape(n, S))


# ---------------------------------------------------------------------------
# float64


def _cat_numerator(state, f, x):
    """log(prior_x + c_x) of categorical feature f at words x -> [nq, K]"""
    feat, st = state.feats[f], state.stats[f]
    xr = np.broadcast_to(np.asarray(x, np.int64)[:, None],
                         (len(x), state.K))
    xi = np.where(xr == OTHER, 0, xr)
    c = st["cnt"][np.arange(state.K)[None, :], np.minimum(xi, feat.dim - 1)]
    S, _ = fx.cat_terms(feat, np.broadcast_to(st["n"], xr.shape), c, xr)
    return S.v


def member_f64(state, qvals, masks, variant=None):
    """one member -> (W [nq, S], band [nq, S]): the float64 log marginal of
    every query row's cells under every mask, and the band of its float32
    value.

    variant: a planted bug instead of the law (the bands mean nothing then):
      "wrong_feature"  bit f of a mask names feature F - 1 - f
      "plus_zero_cat"  an unnamed categorical feature still adds its c1 (the
                       log numerator) and leaves c0 out"""
    F = len(state.feats)
    nq = len(next(v for v in qvals if v is not None))
    W, B = np.zeros((nq, len(masks))), np.zeros((nq, len(masks)))
    done = {}
    for s, mask in enumerate(masks):
        mask = int(mask)
        if mask in done:
            W[:, s], B[:, s] = done[mask]
            continue
        named = [f for f in range(F) if (mask >> f) & 1]
        if variant == "wrong_feature":
            named = sorted(F - 1 - f for f in named)
        extra = [f for f in range(F) if f not in named
                 and state.feats[f].kind in (fx.DD, fx.DPD)
                 and qvals[f] is not None] \
            if variant == "plus_zero_cat" else []
        if not named and not extra:
            Lp, bp = ee.prior_total_f64(state)
            W[:, s], B[:, s] = Lp, bp
        elif not extra:
            sub, keep = fe.without(state, set(range(F)) - set(named))
            W[:, s], B[:, s], _ = pe.logp_f64(sub, [qvals[f] for f in keep])
        else:
            sub, keep = fe.without(state, set(range(F)) - set(named))
            v, _ = pe.query_scores_f64(sub, [np.asarray(qvals[f])
                                             for f in keep]) \
                if keep else (np.repeat(_prior_scores(state)[None, :], nq,
                                        0), None)
            for f in extra:
                v = v + _cat_numerator(state, f, qvals[f])
            m = v.max(1)
            W[:, s] = np.log(np.exp(v - m[:, None]).sum(1)) + m
        done[mask] = (W[:, s].copy(), B[:, s].copy())
    return W, B


def _prior_scores(state):
    """the clustering model's float64 score of every slot [K]"""
    bare = copy.copy(state)
    bare.feats, bare.cols, bare.stats = [], [], []
    bare.slot = np.zeros(1, np.int64)
    v, _, _ = bare.scores(np.arange(1), remove=False)
    return v[0]


def law_f64(states, qvals, masks, le, variant=None):
    """-> (L [nq, S], band [nq, S] or None): the float64 log of the mean over
    the members of their marginal densities and the band of the module
    docstring.

    variant: a planted bug instead of the law (no band then): member_f64's, or
      "mean_of_logs"   the mean of the members' log values
      "no_log_m"       the log of the SUM over the members
      "unnormalised"   LowEntropy without the members' normalisation"""
    M = len(states)
    W, B = [], []
    for st in states:
        Lv, band = member_f64(st, qvals, masks, variant)
        if le and variant != "unnormalised":
            Lp, bp = ee.prior_total_f64(st)
            Lv = Lv - Lp
            band = band + bp + fx.EPS * np.abs(Lv)
        W.append(Lv)
        B.append(band)
    W, B = np.stack(W, 2), np.stack(B, 2)
    nq, S, _ = W.shape
    if variant == "mean_of_logs":
        return W.mean(2), None
    Lv, band, _ = ee.lse_band(W.reshape(nq * S, M), B.reshape(nq * S, M))
    Lv, band = Lv.reshape(nq, S), band.reshape(nq, S)
    if variant == "no_log_m":
        return Lv, None
    log_m = math.log(M)
    Lv = Lv - log_m
    if variant is not None:
        return Lv, None
    table = abs(float(np.float32(ol.oracle().orc_fast_log(float(M))))
                - log_m)
    return Lv, band + table + fx.EPS * np.abs(Lv)


# ---------------------------------------------------------------------------
# the eight-feature list

A5 = [0.5, 1.0, 0.25, 2.0, 0.75]
A3 = [1.5, 0.5, 1.0]
DPD_DIM = 20
EIGHT_KINDS = [ol.DD, ol.BB, ol.GP, ol.NICH, ol.DD, ol.BNB, ol.DPD, ol.DD]
# three members that differ in everything but the feature list
SPECS8 = [dict(k=6, empty=2, alpha=1.0, d=0.0, sweeps=0),
          dict(k=19, empty=1, alpha=20.0, d=0.5, sweeps=1),
          dict(k=33, empty=3, alpha=5.0, d=0.25, sweeps=2)]


def eight_rows(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 5, n).astype(np.uint32),
            (rng.random(n) < 0.4).astype(np.uint32),
            rng.poisson(3.0, n).astype(np.uint32),
            rng.normal(1, 2, n).astype(np.float32),
            rng.integers(0, 70, n).astype(np.uint32),
            rng.negative_binomial(3, 0.4, n).astype(np.uint32),
            rng.integers(0, DPD_DIM, n).astype(np.uint32),
            rng.integers(0, 3, n).astype(np.uint32)]


def eight_shareds(e):
    """member e's hyper-parameters, scaled by (1 + e / 2) (exact in float32)
    -> (oracle shareds, engine shareds)"""
    from distributions_amd import engine
    g = 1.0 + 0.5 * e
    betas = np.full(DPD_DIM, 0.9 / DPD_DIM, np.float32)
    a5 = [a * g for a in A5]
    a70 = [0.5 * g] * 70
    a3 = [a * g for a in A3]
    osh = [ol.make_shared(ol.DD, alphas=a5),
           ol.make_shared(ol.BB, alpha=0.5 * g, beta=2.0),
           ol.make_shared(ol.GP, alpha=1.0 * g, inv_beta=1.0),
           ol.make_shared(ol.NICH, mu=0.25 * e, kappa=1.0, sigmasq=1.0 * g,
                          nu=1.0),
           ol.make_shared(ol.DD, alphas=a70),
           ol.make_shared(ol.BNB, alpha=1.5 * g, beta=0.75, r=3),
           ol.make_shared(ol.DPD, alpha=0.5 * g, betas=betas, beta0=0.1),
           ol.make_shared(ol.DD, alphas=a3)]
    gsh = [engine.dd_shared(a5), engine.bb_shared(0.5 * g, 2.0),
           engine.gp_shared(1.0 * g, 1.0),
           engine.nich_shared(0.25 * e, 1.0, 1.0 * g, 1.0),
           engine.dd_shared(a70), engine.bnb_shared(1.5 * g, 0.75, 3),
           engine.dpd_shared(0.5 * g, betas, 0.1), engine.dd_shared(a3)]
    return osh, gsh


class Member8(ee.Member):
    """an ensemble_expect.Member over the eight-feature list"""

    def __init__(self, e, spec, n):
        self.__dict__.update(spec)
        self.n, self.le = n, None
        self.vals = eight_rows(n, pe.workloads.SEED + 31 * e)
        self.assign0 = (np.arange(n) % self.k).astype(np.uint32)
        self.osh, self.gsh = eight_shareds(e)
        self.orc, self.st = build(self.osh, self.vals, self.assign0, self.k,
                                  self.empty, self.alpha, self.d, self.sweeps,
                                  None)
        self.K = len(self.orc)


class Ensemble8(ee.Ensemble):
    """an ensemble_expect.Ensemble over the eight-feature list (its own
    expect / f64 are predict_many's and need every feature's column)"""

    def __init__(self, specs=SPECS8, n=600, nq=100):
        self.config, self.le, self.nq = "eight", None, nq
        self.members = [Member8(e, s, n) for e, s in enumerate(specs)]
        self.M = len(self.members)
        self.qvals = eight_rows(nq, pe.QSEED)
        # values no member's table holds: OTHER
        self.qvals[6][[1, 2]] = OTHER
        self._expect = {}
        self._f64 = None


def eight_masks():
    """all 8 singles and 28 pairs, the full mask and 0"""
    return np.concatenate([singles_and_pairs(8),
                           np.array([0xFF, 0], np.uint32)])


# ---------------------------------------------------------------------------
# the exact mutual information of a pair of categorical features


def _domain(feat):
    return 2 if feat.kind == fx.BB else feat.dim


def _member_tables(state, i, j, normalise, slots=None):
    """one member -> (p_ij [di, dj], p_i [di], p_j [dj]): its float64
    marginal densities over the pair's domain, every other feature
    unobserved.  normalise: divided by the total mass of the clustering
    model's scores (LowEntropy's are not normalised).  slots: the mixture's
    components that take part (None: all of them)."""
    F = len(state.feats)
    di, dj = _domain(state.feats[i]), _domain(state.feats[j])
    xi = np.repeat(np.arange(di, dtype=np.uint32), dj)
    xj = np.tile(np.arange(dj, dtype=np.uint32), di)
    sub, _ = fe.without(state, set(range(F)) - {i, j})
    vij, _ = pe.query_scores_f64(sub, [xi, xj] if i < j else [xj, xi])
    sub, _ = fe.without(state, set(range(F)) - {i})
    vi, _ = pe.query_scores_f64(sub, [np.arange(di, dtype=np.uint32)])
    sub, _ = fe.without(state, set(range(F)) - {j})
    vj, _ = pe.query_scores_f64(sub, [np.arange(dj, dtype=np.uint32)])
    slots = np.arange(state.K) if slots is None else np.asarray(slots)
    z = np.exp(_prior_scores(state)[slots]).sum() if normalise else 1.0
    return (np.exp(vij[:, slots]).sum(1).reshape(di, dj) / z,
            np.exp(vi[:, slots]).sum(1) / z, np.exp(vj[:, slots]).sum(1) / z)


def enumerate_pair(states, i, j, le, slots=None):
    """-> dict(mi, sigma, h_i, sigma_i, h_j, sigma_j, mass): under
    p = (1/M) sum_e p_e, the exact float64 mutual information of features i
    and j (categorical or BetaBernoulli) and the standard deviation of
    d = log p(x_i, x_j) - log p(x_i) - log p(x_j) under p; the entropies of
    the two features and the standard deviations of -log p(x_i), -log p(x_j);
    the total mass of the pair's table (1 for a proper predictive).  le (or
    slots, which restricts every member to those components): the members are
    normalised by their clustering scores' mass first."""
    tabs = [_member_tables(st, i, j, le or slots is not None, slots)
            for st in states]
    pij = np.mean([t[0] for t in tabs], 0)
    pi = np.mean([t[1] for t in tabs], 0)
    pj = np.mean([t[2] for t in tabs], 0)
    d = np.log(pij) - np.log(pi)[:, None] - np.log(pj)[None, :]
    mi = float((pij * d).sum())
    var = float((pij * d * d).sum()) - mi * mi

    def entropy(p):
        h = float(-(p * np.log(p)).sum())
        v = float((p * np.log(p) ** 2).sum()) - h * h
        return h, math.sqrt(max(v, 0.0))

    hi, si = entropy(pi)
    hj, sj = entropy(pj)
    return dict(mi=mi, sigma=math.sqrt(max(var, 0.0)), h_i=hi, sigma_i=si,
                h_j=hj, sigma_j=sj, mass=float(pij.sum()))


def one_group_state(config="dd_bb_gp", n=200, seed=3):
    """a float64 state whose every row sits in slot 0 (slot 1 is empty):
    restricted to slot 0 (enumerate_pair's slots=[0]) it is a product law, in
    which no two features depend on each other"""
    osh, _, vals, _ = pe.workloads.make(config, n, 1, seed=seed)
    return fx.State(vals, osh, np.zeros(n, np.int64), [0, 1],
                    ("py", 1.0, 0.0))
