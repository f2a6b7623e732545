"""A float64 reference for the row scores, and a band around each score
derived from the float32 operations the kernels perform.

TEST INFRASTRUCTURE (imported by tests only).

A row's score against a slot is the clustering prior of joining that slot plus,
per feature, the log posterior predictive of the row's value under the slot's
group.  Here both are computed in float64 from the group's MEMBERS (rebuilt
from the columns and the assignments); nothing reads the engine's or the
oracle's statistics.

  float64_score        one group, one value: the textbook predictive (scipy)
  row_scores_f64       batch semantics: row r taken out of its own group;
                       alone in it, the group vanishes as
                       MixtureDriver::remove_value does (the last slot moves
                       into slot g, one slot fewer)
  score_rows_f64       Mixture::score_value: nothing removed

The model parameters are the binary32 values the models hold (Shared stores
floats); they are taken as exact.  Mathematical constants (ln 2, pi, the
LowEntropy 0.45 and 0.1) are the real numbers, and their binary32 stand-ins'
distance from them goes into the band.

The band is a running-error bound (every value carries a bound on the
distance of its float32 counterpart from it, class `R`):

  rounded + - * /   eps = 2^-24 times the magnitude of the result, plus the
                    operands' bounds carried through
  fast_log          fast_log(y) = (e + T[m]) ln2 with T the committed 2^14
                    table (ref_tables.h): T is constant over a bucket and log
                    is monotone, so over every float32 argument the operation
                    can see (the value +- its bound) the worst distance from
                    log(value) is at the two end buckets; plus the rounding of
                    e + T, of ln2 and of the product
  fast_lgamma, fast_lgamma_nu, fast_log_factorial
                    the error against scipy.special.gammaln MEASURED through
                    the oracle's exported functions at the float32 arguments
                    the row uses (the value and its neighbours within the
                    bound), plus |psi| times the argument's bound
  NICH              mean and count_times_variance are float32 Welford sums
                    whose error depends on the order of every add and remove
                    the group has seen: `nich_welford_bounds` replays that
                    history with running-error bounds (the float64 values are
                    still the members' two-pass ones)

Nothing in a band is fitted to kernel or oracle output.
"""
import math
import os
import re

import numpy as np
from scipy import special, stats

EPS = 2.0 ** -24
LN2 = math.log(2.0)
LN2_F32 = float(np.float32(0.69314718055994529))
OTHER = 0xFFFFFFFF

DD, BB, GP, NICH, DPD, BNB = 0, 1, 2, 3, 4, 5
NAMES = {DD: "DD", BB: "BB", GP: "GP", NICH: "NICH", DPD: "DPD", BNB: "BNB"}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _log_table():
    path = os.path.join(ROOT, "distributions_amd", "csrc", "ref_tables.h")
    with open(path) as f:
        text = f.read()
    body = text[text.index("DIST_REF_LOG_TABLE[16384]"):]
    body = body[:body.index("};")]
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]+)u", body)]
    assert len(words) == 16384
    return np.array(words, np.uint32).view(np.float32).astype(np.float64)


LOG_TABLE = _log_table()


def float64_score(kind, kw, group_values, value):
    """log predictive density of `value` given the group's values, in float64.

    DPD: `value` OTHER (0xFFFFFFFF) scores alpha * beta0 (dpd.hpp:534-542).
    BNB: the reference's Scorer (bnb.hpp:200-223; oracle.c scorer_init and
    noncat_term) is B(post_alpha + r, post_beta + x) / B(post_alpha,
    post_beta), the beta-negative-binomial pmf WITHOUT its binomial
    coefficient C(x + r - 1, x).  That factor depends on x alone, so it is
    the same in every slot; this function reproduces the reference's
    definition, and `bnb_log_binomial` is the missing term."""
    v = np.asarray(group_values, np.float64)
    n = len(v)
    if kind == DD:
        a = np.asarray(kw["alphas"], np.float64)
        c = np.bincount(np.asarray(group_values, int), minlength=len(a))
        return np.log((a[value] + c[value]) / (a.sum() + n))
    if kind == DPD:
        b = np.asarray(kw["betas"], np.float64) * kw["alpha"]
        if value == OTHER:
            return np.log(kw["alpha"] * kw.get("beta0", 0.0)
                          / (kw["alpha"] + n))
        c = np.bincount(np.asarray(group_values, int), minlength=len(b))
        return np.log((b[value] + c[value]) / (kw["alpha"] + n))
    if kind == BB:
        h = v.sum()
        a, b = kw["alpha"] + h, kw["beta"] + n - h
        return np.log((a if value else b) / (a + b))
    if kind == GP:
        a = kw["alpha"] + v.sum()
        ib = kw["inv_beta"] + n
        # negative binomial predictive
        return (special.gammaln(a + value) - special.gammaln(a)
                - special.gammaln(value + 1) + a * np.log(ib / (ib + 1.0))
                - value * np.log(ib + 1.0))
    if kind == BNB:
        r = float(int(kw["r"]))
        pa = kw["alpha"] + r * n
        pb = kw["beta"] + v.sum()
        return (special.betaln(pa + r, pb + value) - special.betaln(pa, pb))
    if kind == NICH:
        mu, kappa, sigmasq, nu = (kw["mu"], kw["kappa"], kw["sigmasq"],
                                  kw["nu"])
        mean = v.mean() if n else 0.0
        ctv = ((v - mean) ** 2).sum() if n else 0.0
        kn = kappa + n
        mun = (kappa * mu + mean * n) / kn
        nun = nu + n
        sn = (nu * sigmasq + ctv + n * kappa * (mu - mean) ** 2 / kn) / nun
        scale = np.sqrt(sn * (kn + 1.0) / kn)
        return stats.t.logpdf(value, nun, loc=mun, scale=scale)
    raise ValueError(kind)


def bnb_log_binomial(r, x):
    """log C(x + r - 1, x): what BNB's reference score leaves out"""
    return (special.gammaln(x + r) - special.gammaln(r)
            - special.gammaln(x + 1.0))


# ---------------------------------------------------------------------------
# running-error arithmetic


def _rounding(v, *ops):
    """eps |v|, or 0 where exact operands give a binary32 result (no
    rounding happens)"""
    exact = np.asarray(v, np.float32).astype(np.float64) == v
    for o in ops:
        exact = exact & (o.e == 0)
    return np.where(exact, 0.0, EPS * np.abs(v))


class R(object):
    """a float64 value `v` and a bound `e` on the distance of the float32
    value the kernel computes for it (numpy arrays or scalars)"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.asarray(e, np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, R) else R(x)

    def __add__(self, o):
        o = R.of(o)
        v = self.v + o.v
        return R(v, self.e + o.e + _rounding(v, self, o))

    __radd__ = __add__

    def __sub__(self, o):
        o = R.of(o)
        v = self.v - o.v
        return R(v, self.e + o.e + _rounding(v, self, o))

    def __rsub__(self, o):
        return R.of(o) - self

    def __neg__(self):
        return R(-self.v, self.e)

    def __mul__(self, o):
        o = R.of(o)
        v = self.v * o.v
        return R(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e
                 + self.e * o.e + _rounding(v, self, o))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = R.of(o)
        v = self.v / o.v
        den = np.abs(o.v) - o.e
        assert np.all(den > 0), "a divisor's bound reaches zero"
        return R(v, (self.e + np.abs(v) * o.e) / den + _rounding(v, self, o))

    def __rtruediv__(self, o):
        return R.of(o) / self


def const(true_value, f32_value):
    """a constant the kernels hold as a binary32 literal"""
    return R(true_value, abs(float(np.float32(f32_value)) - true_value))


PI = const(math.pi, 3.14159265358979)
C045 = const(0.45, 0.45)
C01 = const(0.1, 0.1)


def _f32_interval(v, e):
    """the float32 values within [v - e, v + e], as their outermost bits"""
    lo = (v - e).astype(np.float32)
    hi = (v + e).astype(np.float32)
    lo = np.where(lo.astype(np.float64) > v - e,
                  np.nextafter(lo, np.float32(-np.inf)), lo)
    hi = np.where(hi.astype(np.float64) < v + e,
                  np.nextafter(hi, np.float32(np.inf)), hi)
    return lo.astype(np.float32), hi.astype(np.float32)


def _fast_log_parts(x32):
    bits = np.asarray(x32, np.float32).view(np.uint32).astype(np.int64)
    ex = ((bits >> 23) & 255) - 127
    man = (bits & 0x7FFFFF) >> 9
    et = ex + LOG_TABLE[man]
    return et, et * LN2


def flog(a):
    """fast_log (special.hpp:57-67) of a float32 argument within a.e of a.v"""
    a = R.of(a)
    v = np.log(a.v)
    lo, hi = _f32_interval(a.v, a.e)
    assert np.all(lo > 0), "fast_log of a non-positive argument"
    et_lo, A_lo = _fast_log_parts(lo)
    et_hi, A_hi = _fast_log_parts(hi)
    table = np.maximum(np.abs(A_lo - v), np.abs(A_hi - v))
    et = np.maximum(np.abs(et_lo), np.abs(et_hi))
    rounding = (et * (EPS + abs(LN2_F32 / LN2 - 1.0)) * LN2
                + EPS * np.maximum(np.abs(A_lo), np.abs(A_hi)))
    return R(v, table + rounding * (1 + 4 * EPS))


def _oracle():
    import oracle_lib
    return oracle_lib.oracle()


def _measured(fn_name, args32):
    """|fast_fn(x) - exact(x)| at float32 arguments, through the oracle"""
    a = np.ascontiguousarray(args32, np.float32)
    out = np.zeros_like(a)
    getattr(_oracle(), "orc_vec_" + fn_name)(a.size, a, out)
    x = a.astype(np.float64)
    if fn_name == "fast_lgamma":
        exact = special.gammaln(x)
    else:
        exact = special.gammaln((x + 1.0) * 0.5) - special.gammaln(x * 0.5)
    return np.abs(out.astype(np.float64) - exact)


def _neighbourhood(v, e):
    """float32 points the operation may see: the interval's ends, the
    nearest float32 to the value and two neighbours on either side"""
    lo, hi = _f32_interval(v, e)
    mid = v.astype(np.float32)
    pts = [lo, hi, mid]
    up, down = mid, mid
    for _ in range(2):
        up = np.nextafter(up, np.float32(np.inf))
        down = np.nextafter(down, np.float32(-np.inf))
        pts += [np.minimum(np.maximum(up, lo), hi),
                np.minimum(np.maximum(down, lo), hi)]
    return lo, hi, np.stack([np.broadcast_to(p, v.shape) for p in pts])


def flgamma(a):
    """fast_lgamma (special.hpp:114-171; glibc lgammaf below 2.5)"""
    a = R.of(a)
    v = special.gammaln(a.v)
    lo, hi, pts = _neighbourhood(a.v, a.e)
    err = _measured("fast_lgamma", pts.ravel()).reshape(pts.shape).max(0)
    slope = np.maximum(np.abs(special.digamma(lo.astype(np.float64))),
                       np.abs(special.digamma(hi.astype(np.float64))))
    width = np.maximum(hi.astype(np.float64) - a.v, a.v - lo.astype(np.float64))
    return R(v, err + slope * width)


def flgamma_nu(a):
    """fast_lgamma_nu(nu) = lgamma((nu + 1) / 2) - lgamma(nu / 2)
    (special.hpp:224-273)"""
    a = R.of(a)
    v = special.gammaln((a.v + 1.0) * 0.5) - special.gammaln(a.v * 0.5)
    lo, hi, pts = _neighbourhood(a.v, a.e)
    err = _measured("fast_lgamma_nu", pts.ravel()).reshape(pts.shape).max(0)
    l64 = lo.astype(np.float64)
    slope = 0.5 * np.abs(special.digamma((l64 + 1.0) * 0.5)
                         - special.digamma(l64 * 0.5))   # decreasing in nu
    width = np.maximum(hi.astype(np.float64) - a.v, a.v - l64)
    return R(v, err + slope * width)


def flog_factorial(x):
    """fast_log_factorial (special.hpp:208-214): an exact argument"""
    x = np.ascontiguousarray(x, np.uint32)
    flat = np.ascontiguousarray(x.ravel())
    o = np.zeros(flat.size, np.float32)
    _oracle().orc_vec_fast_log_factorial(flat.size, flat, o)
    out = o.reshape(x.shape).astype(np.float64)
    v = special.gammaln(x.astype(np.float64) + 1.0)
    return R(v, np.abs(out - v))


# ---------------------------------------------------------------------------
# the models


class Feature(object):
    """one feature's hyperparameters (binary32, as the Shared holds them)"""

    def __init__(self, shared):
        self.kind = int(shared.kind)
        self.dim = int(shared.dim)
        self.p = [float(x) for x in shared.p]
        if self.kind == DD:
            self.alphas = np.array(shared.alphas[:self.dim], np.float64)
        if self.kind == DPD:
            self.betas = np.array(
                [float(np.float32(shared.betas[i])) for i in range(self.dim)])

    def kw(self):
        p = self.p
        if self.kind == DD:
            return dict(alphas=self.alphas)
        if self.kind == DPD:
            return dict(alpha=p[0], betas=self.betas, beta0=p[1])
        if self.kind == BB:
            return dict(alpha=p[0], beta=p[1])
        if self.kind == GP:
            return dict(alpha=p[0], inv_beta=p[1])
        if self.kind == BNB:
            return dict(alpha=p[0], beta=p[1], r=p[2])
        return dict(mu=p[0], kappa=p[1], sigmasq=p[2], nu=p[3])


def _alpha_sum(f):
    """DD's alpha_sum: the float32 sum of the alphas in order
    (dd.hpp update_all); DPD's is alpha itself (dpd.hpp)"""
    if f.kind == DPD:
        return R(f.p[0])
    s = R(0.0)
    for a in f.alphas:
        s = s + R(a)
    return s


def cat_terms(f, n, c, x, mut=()):
    """(S, H): log(prior_x + c_x) and log(alpha_sum + n), the score being
    (acc + S) - H (dd.hpp:433-445, dpd.hpp:517-543)"""
    n = np.asarray(n, np.float64)
    if "dd_alpha_sum_row" in mut and f.kind == DD:
        n = n + 1.0
    H = flog(_alpha_sum(f) + R(n))
    if f.kind == DD:
        prior = R(f.alphas[np.minimum(x, f.dim - 1)])
    else:
        beta = R(f.betas[np.minimum(x, f.dim - 1)])
        prior = beta if "dpd_beta_unscaled" in mut else R(f.p[0]) * beta
    S = flog(prior + R(np.asarray(c, np.float64)))
    if f.kind == DPD and np.any(x == OTHER):
        other = flog(R(f.p[0]) * R(f.p[1]))
        S = R(np.where(x == OTHER, other.v, S.v),
              np.where(x == OTHER, other.e, S.e))
    return S, H


def noncat_term(f, st, x, mut=()):
    """the term a non-categorical feature adds, as scorer_init + noncat_term
    evaluate it (bb.hpp:189-204, gp.hpp:198-217, bnb.hpp:200-223,
    nich.hpp:239-259)"""
    p = f.p
    if f.kind == BB:
        a = R(p[0]) + R(st["h"])
        b = R(p[1]) + R(st["t"])
        ab = a + b
        c0, c1 = flog(a / ab), flog(b / ab)
        one = (x != 0) if "bb_swapped" not in mut else (x == 0)
        return R(np.where(one, c0.v, c1.v), np.where(one, c0.e, c1.e))
    if f.kind == GP:
        fv = R(x.astype(np.float64))
        pa = R(p[0]) + R(st["sum"])
        pib = R(p[1]) + R(st["n"])
        sc = -flog(1.0 + pib)
        c0 = -flgamma(pa) + pa * (flog(pib) + sc)
        t = c0 + flgamma(pa + fv)
        if "gp_no_logfact" not in mut:
            t = t - flog_factorial(x)
        return t + sc * fv
    if f.kind == BNB:
        r = R(p[2])
        n = R(st["n"])
        pa = R(p[0]) + (n if "bnb_r_count" in mut else r * n)
        pb = R(p[1]) + R(st["sum"])
        al = pa + r
        c0 = ((flgamma(pa + pb) - flgamma(pa)) - flgamma(pb)) + flgamma(al)
        beta = pb + R(x.astype(np.float64))
        return (c0 + flgamma(beta)) - flgamma(beta + al)
    if f.kind == NICH:
        mu, kappa, sigmasq, nu = (R(q) for q in p)
        count = R(st["n"])
        mean = R(st["mean"], st["em"])
        ctv = R(st["ctv"], st["ec"])
        mu_1 = mu - mean
        pk = kappa + count
        if "nich_kappa" in mut:
            pk = kappa + count + 1.0
        pm = (kappa * mu + mean * count) / pk
        pn = nu + count
        ps = (1.0 / pn) * ((nu * sigmasq + ctv)
                           + (((count * kappa) * mu_1) * mu_1) / pk)
        lam = pk / ((pk + 1.0) * ps)
        c0 = flgamma_nu(pn) + 0.5 * flog(lam / (PI * pn))
        c1 = -0.5 * pn - 0.5
        c2 = lam / pn
        d = R(x.view(np.float32).astype(np.float64)) - pm
        return c0 + c1 * flog(1.0 + c2 * (d * d))
    raise ValueError(f.kind)


# ---------------------------------------------------------------------------
# NICH: float32 Welford statistics and their error bounds


def _add(s, x):
    n, m, c, em, ec = s
    n += 1
    delta = x - m
    ed = em + EPS * abs(delta)
    q = delta / n
    m2 = m + q
    em2 = em + ed / n + EPS * abs(q) + EPS * abs(m2)
    t = x - m2
    et = em2 + EPS * abs(t)
    prod = delta * t
    ep = abs(delta) * et + abs(t) * ed + ed * et + EPS * abs(prod)
    c2 = c + prod
    return [n, m2, c2, em2, ec + ep + EPS * abs(c2)]


def _remove(s, x):
    n, m, c, em, ec = s
    total = m * n
    etot = n * em + EPS * abs(total)
    delta = x - m
    ed = em + EPS * abs(delta)
    n -= 1
    if n == 0:
        return [0, 0.0, 0.0, 0.0, 0.0]
    num = total - x
    m2 = num / n
    em2 = (etot + EPS * abs(num)) / n + EPS * abs(m2)
    if n <= 1:
        return [n, m2, 0.0, em2, 0.0]
    t = x - m2
    et = em2 + EPS * abs(t)
    prod = delta * t
    ep = abs(delta) * et + abs(t) * ed + ed * et + EPS * abs(prod)
    c2 = c - prod
    return [n, m2, c2, em2, ec + ep + EPS * abs(c2)]


def nich_welford_bounds(x, history):
    """bounds on |mean32 - mean| and |ctv32 - ctv| per group id, after the
    group_add / group_remove sequence (nich.hpp:125-165) the history
    describes: history[0] the assignment the rows were loaded with (added in
    row order), each later entry one batch over all rows (row by row in row
    order: removed from its old id, added to its new one).  -> dict id ->
    (n, em, ec)"""
    x = np.asarray(x, np.float32).astype(np.float64).tolist()
    st = {}
    for i, gid in enumerate(np.asarray(history[0]).tolist()):
        st[gid] = _add(st.get(gid, [0, 0.0, 0.0, 0.0, 0.0]), x[i])
    for old, new in zip(history[:-1], history[1:]):
        old = np.asarray(old).tolist()
        new = np.asarray(new).tolist()
        for i in range(len(x)):
            st[old[i]] = _remove(st[old[i]], x[i])
            st[new[i]] = _add(st.get(new[i], [0, 0.0, 0.0, 0.0, 0.0]), x[i])
    return {gid: (s[0], s[3], s[4]) for gid, s in st.items()}


def nich_remove_bounds(n, mean, ctv, em, ec, x):
    """the bounds after one more group_remove of x (a row's own slot)"""
    s = _remove([int(n), float(mean), float(ctv), float(em), float(ec)],
                float(x))
    return s[3], s[4]


# ---------------------------------------------------------------------------
# the clustering priors


def py_terms(n, ne, n_empty, N, alpha, d, mut=()):
    """PitmanYor(alpha, d) score of joining a group of size n
    (clustering.hpp:126-234 restated): log(n - d) for n > 0,
    log((alpha + d * nonempty) / n_empty) for an empty group, both shifted by
    -log(N + alpha).  N is the sample size the row joins (N - 1 in batch
    semantics)."""
    n = np.asarray(n, np.float64)
    occ = n > 0
    arg = R(np.where(occ, n, 1.0)) if "log_n" in mut else (
        R(np.where(occ, n, 1.0)) - R(d))
    c_occ = flog(arg)
    numer = R(alpha) + R(d) * R(np.asarray(ne, np.float64))
    if "alpha_undivided" not in mut:
        numer = numer / R(np.asarray(n_empty, np.float64))
    c_emp = flog(numer)
    shift = -flog(R(float(N)) + R(alpha))
    c = R(np.where(occ, c_occ.v, c_emp.v), np.where(occ, c_occ.e, c_emp.e))
    return c + shift


def le_terms(n, sample_size, n_empty, dataset_size, mut=()):
    """LowEntropy(dataset_size).score_add_value (clustering.hpp:267-327) in
    float64: -log(n_empty) plus the postpred correction at sample_size + 1
    (when below dataset_size) for an empty group; n log((n + 1) / n) +
    log(n + 1), or 1 + log(n + 1) above very_large = 10000, otherwise."""
    n = np.asarray(n, np.float64)
    D = float(dataset_size)
    s = float(sample_size) + (0.0 if "le_corr_at_sample" in mut else 1.0)
    empty = -flog(R(np.full(n.shape, float(n_empty))))
    if s < D:
        corr = flog(R(D) / R(s)) * ((C045 - C01 / R(s)) - C01 / R(D))
        empty = empty + corr
    nn = np.where(n > 0, n, 1.0)
    bigger = 1.0 + R(nn)
    small = flog(bigger / R(nn)) * R(nn) + flog(bigger)
    large = 1.0 + flog(bigger)
    very_large = 10 ** 9 if "le_very_large" in mut else 10000
    big = n > very_large
    v = np.where(n == 0, empty.v, np.where(big, large.v, small.v))
    e = np.where(n == 0, empty.e, np.where(big, large.e, small.e))
    return R(v, e)


# ---------------------------------------------------------------------------
# a state: members rebuilt from the columns and the assignments


class State(object):
    """cols: one value array per feature (uint32, or float32 for NICH);
    shareds: the oracle Shared structs (hyperparameters only);
    assign: each row's global group id; p2g: the global id of each slot;
    prior: ("py", alpha, d) or ("le", dataset_size);
    history: the assignments NICH statistics went through
    (`nich_welford_bounds`), default [assign]."""

    def __init__(self, cols, shareds, assign, p2g, prior, history=None):
        self.cols = [np.asarray(c) for c in cols]
        self.feats = [Feature(s) for s in shareds]
        self.assign = np.asarray(assign, np.int64)
        self.p2g = np.asarray(p2g, np.int64)
        self.prior = prior
        self.K = len(self.p2g)
        self.N = len(self.assign)
        g2p = {int(gid): k for k, gid in enumerate(self.p2g)}
        self.slot = np.array([g2p[int(a)] for a in self.assign], np.int64)
        self.counts = np.bincount(self.slot, minlength=self.K)
        self.n_empty = int((self.counts == 0).sum())
        history = [self.assign] if history is None else history
        self.stats = []
        for f, col in zip(self.feats, self.cols):
            st = {"n": self.counts.astype(np.float64)}
            if f.kind in (DD, DPD):
                cnt = np.zeros((self.K, f.dim), np.int64)
                np.add.at(cnt, (self.slot, col.astype(np.int64)), 1)
                st["cnt"] = cnt
            elif f.kind == BB:
                st["h"] = np.bincount(self.slot, weights=(col != 0),
                                      minlength=self.K)
                st["t"] = self.counts - st["h"]
            elif f.kind in (GP, BNB):
                st["sum"] = np.bincount(self.slot,
                                        weights=col.astype(np.float64),
                                        minlength=self.K)
            else:
                xv = col.view(np.float32).astype(np.float64)
                s1 = np.bincount(self.slot, weights=xv, minlength=self.K)
                mean = np.where(self.counts > 0,
                                s1 / np.maximum(self.counts, 1), 0.0)
                ctv = np.bincount(self.slot, weights=(xv - mean[self.slot])
                                  ** 2, minlength=self.K)
                b = nich_welford_bounds(col.view(np.float32), history)
                em = np.zeros(self.K)
                ec = np.zeros(self.K)
                for k, gid in enumerate(self.p2g):
                    if int(gid) in b:
                        nb, em[k], ec[k] = b[int(gid)]
                        assert nb == self.counts[k], "history != assignment"
                st.update(mean=mean, ctv=ctv, em=em, ec=ec)
            self.stats.append(st)

    # -- the scores ---------------------------------------------------------
    def scores(self, rows, remove=True, mut=()):
        """-> (value [R, K], band [R, K], Kl [R]); entries at or past Kl are
        NaN.  remove: batch semantics (row_scores_f64), else score_value
        (score_rows_f64)."""
        rows = np.atleast_1d(np.asarray(rows, np.int64))
        K = self.K
        Rn = len(rows)
        g = self.slot[rows]
        single = (self.counts[g] == 1) & remove
        kl = np.where(single, K - 1, K)
        src = np.broadcast_to(np.arange(K), (Rn, K)).copy()
        if "singleton_old" not in mut:
            src[single, g[single]] = K - 1
        own = np.zeros((Rn, K), bool)
        if remove:
            own[~single, g[~single]] = True
        valid = np.arange(K)[None, :] < kl[:, None]
        own_prior = own if "own_prior" not in mut else np.zeros_like(own)
        own_feat = own if "own_feat" not in mut else np.zeros_like(own)
        if "own_both" in mut:
            own_prior = own_feat = np.zeros_like(own)
        # (mutant singleton_old: slot g keeps the old group, row included)
        n = self.counts[src] - own_prior
        N = self.N - (1 if remove else 0)
        if self.prior[0] == "py":
            alpha, d = self.prior[1], self.prior[2]
            ne = (K - self.n_empty) - (single.astype(int)
                                       if "vanish_nonempty" not in mut
                                       else 0)
            ne = np.broadcast_to(np.asarray(ne)[:, None] if np.ndim(ne)
                                 else ne, (Rn, K))
            Ns = N + (1 if "shift_N" in mut and remove else 0)
            acc = py_terms(n, ne, self.n_empty, Ns, alpha, d, mut)
        else:
            acc = le_terms(n, N, self.n_empty, self.prior[1], mut)
        for f, col, st in zip(self.feats, self.cols, self.stats):
            x = col[rows]
            xr = np.broadcast_to(x[:, None], (Rn, K))
            nf = st["n"][src] - own_feat
            if f.kind in (DD, DPD):
                xi = np.where(xr == OTHER, 0, xr).astype(np.int64)
                c = st["cnt"][src, np.minimum(xi, f.dim - 1)] - own_feat
                S, H = cat_terms(f, nf, c, xr.astype(np.int64), mut)
                acc = (acc + S) - H
                continue
            sub = {"n": nf}
            if f.kind == BB:
                one = (xr != 0)
                sub["h"] = st["h"][src] - own_feat * one
                sub["t"] = st["t"][src] - own_feat * (~one)
            elif f.kind in (GP, BNB):
                sub["sum"] = st["sum"][src] - own_feat * xr.astype(np.float64)
            else:
                xv = x.view(np.float32).astype(np.float64)
                mean = st["mean"][src].copy()
                ctv = st["ctv"][src].copy()
                em = st["em"][src].copy()
                ec = st["ec"][src].copy()
                for i in np.nonzero(own_feat.any(1))[0]:
                    k = g[i]
                    n0 = self.counts[k]
                    m0, c0 = mean[i, k], ctv[i, k]
                    em[i, k], ec[i, k] = nich_remove_bounds(
                        n0, m0, c0, em[i, k], ec[i, k], xv[i])
                    if n0 == 1:
                        mean[i, k], ctv[i, k] = 0.0, 0.0
                    else:
                        m1 = (n0 * m0 - xv[i]) / (n0 - 1)
                        mean[i, k] = m1
                        ctv[i, k] = (max(c0 - (xv[i] - m0) * (xv[i] - m1),
                                         0.0) if n0 > 2 else 0.0)
                sub.update(mean=mean, ctv=ctv, em=em, ec=ec)
            acc = acc + noncat_term(f, sub, xr, mut)
        v = np.where(valid, acc.v, np.nan)
        e = np.where(valid, acc.e, np.nan)
        return v, e, kl


def row_scores_f64(state, rows, mut=()):
    """batch-semantics scores of `rows` (row removed from its own slot)"""
    return state.scores(rows, remove=True, mut=mut)


def score_rows_f64(state, rows, mut=()):
    """Mixture::score_value of `rows` against every slot, nothing removed"""
    return state.scores(rows, remove=False, mut=mut)


def checked_rows(state, cap=64):
    """every row alone in its group, rows of groups of size 2 (fast_lgamma's
    glibc branch, below 2.5), rows of the largest group, first and last"""
    c = state.counts[state.slot]
    single = np.nonzero(c == 1)[0]
    pairs = np.nonzero(c == 2)[0][:2 * cap]
    big = np.nonzero(state.slot == int(np.argmax(state.counts)))[0]
    big = big[np.linspace(0, len(big) - 1, min(cap, len(big))).astype(int)]
    return np.unique(np.r_[single, pairs, big, 0, state.N - 1])


def excursion(got, want, band):
    """|got - want| / band over the valid entries (0 where both agree)"""
    got = np.asarray(got, np.float64)
    ok = ~np.isnan(want)
    d = np.abs(got - want)
    out = np.zeros(want.shape)
    out[ok] = np.where(d[ok] == 0, 0.0, d[ok] / np.maximum(band[ok], 1e-300))
    return out
