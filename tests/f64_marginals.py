"""A float64 reference for the log marginal likelihoods the hyper-parameter
step draws from, and a band around each derived from the float32 operations
the kernels perform.

TEST INFRASTRUCTURE (imported by tests only).  Built on f64_scores: like that
module it reads nothing from the engine's or the oracle's statistics;
everything is rebuilt from the columns, the assignments and the history of
assignments (`f64_scores.State`).

Float64 values (`Marginals.data`, `Marginals.counts`), closed forms summed
over the non-empty groups:

  DD, DPD   Dirichlet-multinomial: sum_v lgamma(a_v + c_v) - lgamma(a_v)
            + lgamma(A) - lgamma(A + n); DPD's a_v = alpha beta_v, A = alpha
  BB        beta-binomial: B(a + heads, b + tails) / B(a, b)
  GP        gamma-Poisson: lgamma(a + S) - lgamma(a) + a log(ib)
            - (a + S) log(ib + n) - sum log x!
  BNB       B(a + r n, b + S) / B(a, b): the reference's definition, which
            like its predictive (f64_scores.float64_score) leaves out the
            binomial coefficients sum log C(x + r - 1, x); they depend on the
            data alone, not on the hyper-parameters other than r and not on
            the partition
  NICH      the four terms of nich.hpp:262-288 from the members' two-pass
            mean and sum of squares
  PitmanYor score_counts(alpha, d): the EPPF,
            sum_{j<k} log(alpha + j d) - [lgamma(alpha + N) - lgamma(alpha)]
            + sum_b lgamma(n_b - d) - lgamma(1 - d)

The band is a running-error bound (f64_scores.R) that follows the float32
operations of the code under test in their order:

  DD        k_score_data_dd / k_hyper_dd_chains: one accumulator per value
            plus the shift accumulator, fed group by group in slot order,
            empty groups skipped; closed in the association of
            vector_sum_as_built (four lanes, (l1 + l3) + (l0 + l2), tail in
            order, plain order below four).  alpha_sum is the binary32 value
            the Shared holds: the float sum in index order for the first
            candidate of a grid; for later ones the host carries it in
            binary64 from candidate to candidate and narrows once, so it is
            within the first candidate's summation error plus one rounding
            of the true sum.
  scalar    the terms of scalar_mixture_score_terms, each an R expression,
            added into ONE accumulator group by group and term by term
            (k_score_data_serial).  BB includes empty groups, the others
            skip them.  NICH's mean and count_times_variance carry
            nich_welford_bounds over the history, GammaPoisson's log_prod
            `gp_log_prod_bounds`.
  DPD       sum="f64": binary64 sum of the float terms, narrowed once
            (k_score_data_grid + k_hyper_narrow): the terms' own bounds plus
            one float32 rounding of the total.  sum="serial": the oracle's
            float accumulation in group-then-value order; it contains the
            other.
  score_counts  binary64 sum of float terms, narrowed once.

Nothing in a band is fitted to kernel or oracle output.

Planted bugs (mut=) change the FLOAT64 side only; the band stays the one of
the operations performed:
  drop_group        the smallest non-empty group left out
  cell_off          one count cell of the largest group off by one (DD/DPD a
                    cell, BB heads, GP/BNB the sum, NICH the count)
  alpha_sum_other   DD: alpha_sum the float64 sum of the NEXT candidate's
                    alphas (the host's candidate diffing gone wrong)
  bb_skip_empty     BB without its empty groups
  gp_no_log_prod    GP without sum log x!
  nich_nu_prior     NICH with nu in place of nu + n in the sigmasq term
  py_no_d           score_counts with d dropped from the per-group product
"""
import math

import numpy as np
from scipy import special

import f64_scores as fx
from f64_scores import (BB, BNB, DD, DPD, EPS, GP, NICH, R, const, flgamma,
                        flog)

LOG_PI = const(math.log(math.pi), 1.1447298858493991)
SLACK = 1.0 + 1e-6      # second-order terms of the running error

MUTANTS = ["drop_group", "cell_off", "alpha_sum_other", "bb_skip_empty",
           "gp_no_log_prod", "nich_nu_prior", "py_no_d"]


# ---------------------------------------------------------------------------
# GammaPoisson's log_prod


def _log_factorials(x):
    """(float64 log x!, the binary32 fast_log_factorial(x) as float64)"""
    r = fx.flog_factorial(np.ascontiguousarray(x, np.uint32))
    x32 = np.ascontiguousarray(x, np.uint32)
    out = np.zeros(x32.size, np.float32)
    fx._oracle().orc_vec_fast_log_factorial(x32.size, x32, out)
    return r.v, out.astype(np.float64)


def gp_log_prod_bounds(x, history):
    """bounds on |log_prod32 - sum log x!| per group id after the float32
    `log_prod += fast_log_factorial(x)` / `-=` sequence (gp.hpp:115,134) the
    history describes (as nich_welford_bounds: history[0] added in row order,
    each later entry row by row, removed from its old id and added to its
    new one).

    The binary32 value is (the exact sum of the members' binary32
    fast_log_factorial) + (the roundings of the adds and subtracts so far):
    a value added and later removed cancels exactly but for those roundings.
    So the bound is the running sum of eps |log_prod| over the operations
    plus, over the CURRENT members, |fast_log_factorial(x) - log x!|.
    -> dict id -> (n, bound)"""
    x = np.ascontiguousarray(x, np.uint32)
    true, lf32 = _log_factorials(x)
    err = np.abs(lf32 - true).tolist()
    lf = lf32.tolist()
    st = {}

    def step(gid, i, sign):
        n, s, D, m = st.get(gid, (0, 0.0, 0.0, 0.0))
        s2 = s + sign * lf[i]
        exact = D == 0.0 and float(np.float32(s2)) == s2
        st[gid] = (n + sign, s2, D + (0.0 if exact else EPS * abs(s2)),
                   m + sign * err[i])

    for i, gid in enumerate(np.asarray(history[0]).tolist()):
        step(gid, i, 1)
    for old, new in zip(history[:-1], history[1:]):
        old = np.asarray(old).tolist()
        new = np.asarray(new).tolist()
        for i in range(len(lf)):
            step(old[i], i, -1)
            step(new[i], i, 1)
    return {gid: (s[0], (s[2] + max(s[3], 0.0)) * SLACK)
            for gid, s in st.items()}


# ---------------------------------------------------------------------------
# accumulation orders


def _serial(t, axis=0):
    """one float32 accumulator starting at +0, the terms added in order
    along `axis`"""
    if t.v.shape[axis] == 0:
        shape = list(t.v.shape)
        del shape[axis]
        return R(np.zeros(shape), np.zeros(shape))
    cs = np.cumsum(t.v, axis)
    # (the first add, 0 + t, is exact)
    tail = np.take(cs, np.arange(1, cs.shape[axis]), axis)
    return R(np.take(cs, -1, axis),
             (t.e.sum(axis) + EPS * np.abs(tail).sum(axis)) * SLACK)


def _vector_sum(x):
    """vector_sum_as_built (models.h) over the last axis"""
    W = x.v.shape[-1]

    def col(i):
        return R(x.v[..., i], x.e[..., i])
    if W < 4:
        s = col(0)
        for i in range(1, W):
            s = s + col(i)
        return s
    body = W & ~3
    lanes = [col(j) for j in range(4)]
    for i in range(4, body, 4):
        lanes = [lanes[j] + col(i + j) for j in range(4)]
    s = (lanes[1] + lanes[3]) + (lanes[0] + lanes[2])
    for i in range(body, W):
        s = s + col(i)
    return s


def _narrowed(terms, extra=0.0):
    """a binary64 sum of float32 terms (R, flat), narrowed to float32 once"""
    total = terms.v.sum()
    e = (terms.e.sum() + 2.0 ** -50 * np.abs(terms.v).sum() + extra)
    exact = e == 0.0 and float(np.float32(total)) == total
    return R(total, e + (0.0 if exact else EPS * abs(total)))


def shift_term(A, n):
    """fast_lgamma(alpha_sum) - fast_lgamma(alpha_sum + n) with ONE binary32
    alpha_sum (A32, within A.e of A.v) in both places.  With L32 the kernel's
    fast_lgamma, L the true one, y32 = fl(A32 + n) and g(x) = L(x) - L(x + n):

      result - g(A) = [L32(A32) - L(A32)] - [L32(y32) - L(y32)]
                      + [g(A32) - g(A)] + [L(A32 + n) - L(y32)] + rounding

    so the bound is fast_lgamma's measured error at both arguments, A.e times
    the largest |psi(x + n) - psi(x)| over the interval (at its lower end:
    the difference decreases in x) -- not psi(x) + psi(x + n), as two
    unrelated arguments would give --, psi times the rounding of A32 + n,
    and the rounding of the difference.  A: R [C]; n: [Kl] -> R [Kl, C]"""
    n = np.asarray(n, np.float64)[:, None]
    Ab = R(A.v[None], A.e[None])
    y = Ab + R(n)
    v = special.gammaln(Ab.v) - special.gammaln(y.v)
    meas_first = np.maximum(flgamma(A).e - _argument_part(A), 0.0)
    meas_whole = np.maximum(flgamma(y).e - _argument_part(y), 0.0)
    lo = np.maximum(Ab.v - Ab.e, 1e-300)
    moved = Ab.e * np.abs(special.digamma(lo + n) - special.digamma(lo))
    rounded = (y.e - Ab.e) * np.abs(special.digamma(y.v + y.e))
    return R(v, (meas_first[None] + meas_whole + moved + rounded
                 + EPS * np.abs(v)) * SLACK)


def _argument_part(a):
    """the slope * width term of f64_scores.flgamma's bound"""
    lo, hi = fx._f32_interval(a.v, a.e)
    slope = np.maximum(np.abs(special.digamma(lo.astype(np.float64))),
                       np.abs(special.digamma(hi.astype(np.float64))))
    width = np.maximum(hi.astype(np.float64) - a.v,
                       a.v - lo.astype(np.float64))
    return slope * width


def dd_alpha_sums(cands):
    """the binary32 alpha_sum of every candidate of a DD grid, as R:
    candidate 0's float sum in index order (dd.hpp _init); later ones
    binary64-carried differences narrowed once (dd.hpp:259-284 _update)"""
    first = fx._alpha_sum(cands[0])
    out = [first]
    for f in cands[1:]:
        v = float(f.alphas.sum())
        out.append(R(v, float(first.e) + EPS * abs(v)))
    return out


# ---------------------------------------------------------------------------


class Marginals(object):
    """state: f64_scores.State; history: the assignments it went through
    (for GammaPoisson's log_prod; NICH's is already in the State)"""

    def __init__(self, state, history=None):
        self.st = state
        s = state
        history = [s.assign] if history is None else history
        self.live = np.nonzero(s.counts > 0)[0]
        self.gp = {}
        for fi, (f, col) in enumerate(zip(s.feats, s.cols)):
            if f.kind != GP:
                continue
            true, _ = _log_factorials(col)
            lp = np.bincount(s.slot, weights=true, minlength=s.K)
            b = gp_log_prod_bounds(col, history)
            elp = np.zeros(s.K)
            for k, gid in enumerate(s.p2g):
                if int(gid) in b:
                    nb, elp[k] = b[int(gid)]
                    assert nb == s.counts[k], "history != assignment"
            self.gp[fi] = (lp, elp)

    # -- which groups and cells the planted bugs touch ----------------------
    def _groups(self, mut):
        live = self.live
        if "drop_group" in mut and len(live):
            small = live[np.argmin(self.st.counts[live])]
            live = live[live != small]
        return live

    def _largest(self):
        return int(np.argmax(self.st.counts))

    # -- float64 -------------------------------------------------------------
    def data_f64(self, fi, cands, mut=()):
        """float64 log marginal likelihood of feature fi's data given the
        partition under each candidate (f64_scores.Feature) -> [C]"""
        s = self.st
        stt = s.stats[fi]
        kind = s.feats[fi].kind
        live = self._groups(mut)
        big = self._largest()
        off = (np.arange(s.K) == big).astype(np.float64) \
            if "cell_off" in mut and s.counts[big] else np.zeros(s.K)
        n = stt["n"]
        out = []
        for ci, f in enumerate(cands):
            if kind in (DD, DPD):
                cnt = stt["cnt"].astype(np.float64)
                if off.any():
                    cnt = cnt.copy()
                    cnt[big, int(np.argmax(cnt[big]))] += 1.0
                if kind == DD:
                    a = f.alphas
                    src = cands[(ci + 1) % len(cands)] \
                        if "alpha_sum_other" in mut else f
                    A = float(src.alphas.sum())
                else:
                    a = f.p[0] * f.betas
                    A = f.p[0]
                c = cnt[live]
                v = (special.gammaln(a + c) - special.gammaln(a)).sum() + (
                    special.gammaln(A) - special.gammaln(A + n[live])).sum()
            elif kind == BB:
                g = live if "bb_skip_empty" in mut else np.r_[
                    live, np.nonzero(s.counts == 0)[0]].astype(int)
                h = (stt["h"] + off)[g]
                t = stt["t"][g]
                v = (special.betaln(f.p[0] + h, f.p[1] + t)
                     - special.betaln(f.p[0], f.p[1])).sum()
            elif kind == GP:
                S = (stt["sum"] + off)[live]
                lp = self.gp[fi][0][live]
                if "gp_no_log_prod" in mut:
                    lp = 0.0 * lp
                a, ib = f.p[0], f.p[1]
                v = (special.gammaln(a + S) - special.gammaln(a)
                     + a * np.log(ib) - (a + S) * np.log(ib + n[live])
                     - lp).sum()
            elif kind == BNB:
                S = (stt["sum"] + off)[live]
                a, b, r = f.p[0], f.p[1], float(int(f.p[2]))
                v = (special.betaln(a + r * n[live], b + S)
                     - special.betaln(a, b)).sum()
            else:
                assert kind == NICH
                mu, kappa, sig, nu = f.p
                nn = (n + off)[live]
                mean, ctv = stt["mean"][live], stt["ctv"][live]
                pk = kappa + nn
                pnu = nu + nn
                psig = (nu * sig + ctv
                        + nn * kappa * (mu - mean) ** 2 / pk) / pnu
                w = nu if "nich_nu_prior" in mut else pnu
                v = (special.gammaln(0.5 * pnu) - special.gammaln(0.5 * nu)
                     + 0.5 * np.log(kappa / pk)
                     + 0.5 * nu * np.log(nu * sig)
                     - 0.5 * w * np.log(pnu * psig)
                     - 0.5 * nn * math.log(math.pi)).sum()
            out.append(float(v))
        return np.array(out)

    # -- the float32 operations, with running error --------------------------
    def data_r(self, fi, cands, total="serial"):
        """-> R [C]: the float64 value through the kernels' expressions and
        the bound on the float32 result's distance from it"""
        s = self.st
        stt = s.stats[fi]
        kind = s.feats[fi].kind
        live = self.live
        n = stt["n"]
        vs, es = [], []
        if kind == DD:
            sums = dd_alpha_sums(cands)
            a = R(np.array([f.alphas for f in cands]))            # [C, dim]
            A = R(np.array([float(x.v) for x in sums]),
                  np.array([float(x.e) for x in sums]))           # [C]
            c = stt["cnt"][live].astype(np.float64)               # [Kl, dim]
            shared = flgamma(a)
            t = flgamma(R(a.v[None]) + R(c[:, None, :])) - R(
                shared.v[None], shared.e[None])
            u = shift_term(A, n[live])                            # [Kl, C]
            chains = _serial(t)                                   # [C, dim]
            shift = _serial(u)                                    # [C]
            x = R(np.concatenate([chains.v, shift.v[:, None]], 1),
                  np.concatenate([chains.e, shift.e[:, None]], 1))
            return _vector_sum(x)
        for f in cands:
            p = f.p
            if kind == DPD:
                alpha = R(p[0])
                c = stt["cnt"][live].astype(np.float64)
                prior = alpha * R(f.betas)
                lg0 = flgamma(prior)
                t = flgamma(R(prior.v[None], prior.e[None]) + R(c)) - R(
                    lg0.v[None], lg0.e[None])
                u = flgamma(alpha) - flgamma(alpha + R(n[live]))
                # group by group: its non-zero cells in value order, then
                # its shift term
                tv = np.concatenate([t.v, u.v[:, None]], 1)
                te = np.concatenate([t.e, u.e[:, None]], 1)
                keep = np.concatenate([c > 0, np.ones((len(live), 1), bool)],
                                      1)
                flat = R(tv[keep], te[keep])
                acc = _serial(flat) if total == "serial" else _narrowed(flat)
                vs.append(float(acc.v))
                es.append(float(acc.e))
                continue
            g = np.arange(s.K) if kind == BB else live
            ng = R(n[g])
            if kind == BB:
                a, b = R(p[0]), R(p[1])
                shared = (flgamma(a + b) - flgamma(a)) - flgamma(b)
                pa, pb = a + R(stt["h"][g]), b + R(stt["t"][g])
                group = (flgamma(pa) + flgamma(pb)) - flgamma(pa + pb)
                terms = [shared + group]
            elif kind == BNB:
                a, b, r = R(p[0]), R(p[1]), R(p[2])
                shared = (flgamma(a + b) - flgamma(a)) - flgamma(b)
                pa, pb = a + r * ng, b + R(stt["sum"][g])
                terms = [(flgamma(pa) + flgamma(pb)) - flgamma(pa + pb),
                         shared]
            elif kind == GP:
                a, ib = R(p[0]), R(p[1])
                pa, pib = a + R(stt["sum"][g]), ib + ng
                lp, elp = self.gp[fi]
                terms = [flgamma(pa) - flgamma(a),
                         a * flog(ib) - pa * flog(pib),
                         -R(lp[g], elp[g])]
            else:
                mu, kappa, sig, nu = (R(q) for q in p)
                mean = R(stt["mean"][g], stt["em"][g])
                ctv = R(stt["ctv"][g], stt["ec"][g])
                mu_1 = mu - mean
                pk = kappa + ng
                pnu = nu + ng
                psig = (1.0 / pnu) * ((nu * sig + ctv)
                                      + (((ng * kappa) * mu_1) * mu_1) / pk)
                terms = [flgamma(0.5 * pnu) - flgamma(0.5 * nu),
                         0.5 * flog(kappa) - 0.5 * flog(pk),
                         (0.5 * nu) * flog(nu * sig)
                         - (0.5 * pnu) * flog(pnu * psig),
                         (-0.5 * LOG_PI) * ng]
            flat = R(np.stack([np.broadcast_to(t.v, (len(g),))
                               for t in terms], 1).ravel(),
                     np.stack([np.broadcast_to(t.e, (len(g),))
                               for t in terms], 1).ravel())
            acc = _serial(flat)
            vs.append(float(acc.v))
            es.append(float(acc.e))
        return R(np.array(vs), np.array(es))

    def data(self, fi, cands, mut=(), total="serial"):
        """-> (float64 scores [C], bands [C])"""
        r = self.data_r(fi, cands, total)
        v = self.data_f64(fi, cands, mut)
        if not mut:
            # the two float64 evaluations are of the same quantity
            assert np.all(np.abs(r.v - v) <= 1e-9 * (1.0 + np.abs(v))), (r.v,
                                                                         v)
        return v, np.asarray(r.e, np.float64) + 0.0 * v

    def group_r(self, fi, f, k):
        """Group::score_data of slot k alone (dd.hpp:160-177, bb.hpp:141-151,
        gp.hpp:155-164, nich.hpp:190-202, bnb.hpp:157-166, dpd.hpp:234-250)
        in ITS order of float32 operations -> R.  The sum of its float64
        values over the non-empty slots is data_f64."""
        s = self.st
        stt = s.stats[fi]
        kind = s.feats[fi].kind
        n = R(float(stt["n"][k]))
        p = f.p

        def serial(terms):
            acc = R(0.0)
            for t in terms:
                acc = acc + t
            return acc
        if kind in (DD, DPD):
            c = stt["cnt"][k].astype(np.float64)
            if kind == DD:
                prior, A = R(f.alphas), fx._alpha_sum(f)
                sel = np.ones(f.dim, bool)
            else:
                prior, A = R(p[0]) * R(f.betas), R(p[0])
                sel = c > 0
            t = flgamma(prior + R(c)) - flgamma(prior)
            acc = _serial(R(t.v[sel], t.e[sel]))
            u = shift_term(R(np.atleast_1d(A.v), np.atleast_1d(A.e)),
                           [float(n.v)])
            return acc + R(u.v[0, 0], u.e[0, 0])
        if kind == BB:
            a, b = R(p[0]), R(p[1])
            pa, pb = a + R(float(stt["h"][k])), b + R(float(stt["t"][k]))
            return serial([flgamma(pa) - flgamma(a), flgamma(pb) - flgamma(b),
                           flgamma(a + b) - flgamma(pa + pb)])
        if kind == BNB:
            a, b, r = R(p[0]), R(p[1]), R(p[2])
            pa, pb = a + r * n, b + R(float(stt["sum"][k]))
            return serial([flgamma(a + b) - flgamma(pa + pb),
                           flgamma(pa) - flgamma(a), flgamma(pb) - flgamma(b)])
        if kind == GP:
            a, ib = R(p[0]), R(p[1])
            pa, pib = a + R(float(stt["sum"][k])), ib + n
            lp, elp = self.gp[fi]
            return serial([flgamma(pa) - flgamma(a),
                           a * flog(ib) - pa * flog(pib),
                           -R(float(lp[k]), float(elp[k]))])
        mu, kappa, sig, nu = (R(q) for q in p)
        mean = R(float(stt["mean"][k]), float(stt["em"][k]))
        ctv = R(float(stt["ctv"][k]), float(stt["ec"][k]))
        mu_1 = mu - mean
        pk = kappa + n
        pnu = nu + n
        psig = (1.0 / pnu) * ((nu * sig + ctv)
                              + (((n * kappa) * mu_1) * mu_1) / pk)
        return serial([flgamma(0.5 * pnu) - flgamma(0.5 * nu),
                       0.5 * flog(kappa / pk),
                       (0.5 * nu) * flog(nu * sig)
                       - (0.5 * pnu) * flog(pnu * psig),
                       (-0.5 * n) * LOG_PI])

    # -- PitmanYor -----------------------------------------------------------
    def counts_f64(self, alpha, d, mut=()):
        """the EPPF of the non-empty groups' sizes"""
        c = self.st.counts[self._groups(mut)].astype(np.float64)
        if "cell_off" in mut and len(c):
            c = c.copy()
            c[int(np.argmax(c))] += 1.0
        k, N = len(c), c.sum()
        if k == 0:
            return 0.0
        dd = 0.0 if "py_no_d" in mut else d
        return float(np.log(alpha + d * np.arange(k)).sum()
                     - (special.gammaln(alpha + N) - special.gammaln(alpha))
                     + (special.gammaln(c - dd) - special.gammaln(1.0 - dd)
                        ).sum())

    def counts_r(self, alpha, d):
        """PitmanYor::score_counts (clustering.cc:152-183) over the slots in
        order: float32 terms summed in binary64, narrowed once"""
        c = self.st.counts[self.live].astype(np.float64)
        if not len(c):
            return R(0.0)
        ne = R(np.arange(len(c), dtype=np.float64))
        ss = R(np.r_[0.0, np.cumsum(c)[:-1]])
        a, dr = R(alpha), R(d)
        numer = a + dr * ne
        base = a + ss
        one = flog(numer / base)
        two = flog((numer * (1.0 - dr)) / (base * (base + 1.0)))
        cc = np.maximum(c, 3.0)
        log_part = flog(numer)
        up = flgamma((1.0 - dr) + R(cc - 1.0)) - flgamma(1.0 - dr)
        down = flgamma(base + R(cc)) - flgamma(base)
        v = np.where(c == 1, one.v, np.where(c == 2, two.v,
                                             log_part.v + up.v - down.v))
        e = np.where(c == 1, one.e, np.where(c == 2, two.e,
                                             log_part.e + up.e + down.e))
        return _narrowed(R(v, e))

    def counts(self, alphas, ds, mut=()):
        """-> (float64 scores [C], bands [C]) for (alphas[c], ds[c]), the
        binary32 values taken as exact"""
        v, b = [], []
        for alpha, d in zip(alphas, ds):
            alpha = float(np.float32(alpha))
            d = float(np.float32(d))
            r = self.counts_r(alpha, d)
            x = self.counts_f64(alpha, d, mut)
            if not mut:
                assert abs(float(r.v) - x) <= 1e-9 * (1.0 + abs(x)), (r.v, x)
            v.append(x)
            b.append(float(r.e))
        return np.array(v), np.array(b)


# ---------------------------------------------------------------------------
# the grid posterior


def log_softmax(scores):
    s = np.asarray(scores, np.float64)
    m = s.max()
    return s - (m + np.log(np.exp(s - m).sum()))


def grid_posterior(v, band):
    """-> (float64 log softmax of the grid's scores, bound on
    |log p32_c - log p64_c|).

    log p_c = s_c - L(s) with L = log sum exp.  With |s32_c - s64_c| <= b_c
    <= B = max b: L is monotone in every argument and L(s + B) = L(s) + B, so
    |L(s32) - L(s64)| <= B; hence |log p32_c - log p64_c| <= b_c + B <= 2 B.
    (p32 is the softmax of the float32 scores evaluated exactly; the draw's
    own arithmetic is the sampler tests' subject.)"""
    return log_softmax(v), 2.0 * float(np.max(band)) if len(band) else 0.0


def total_variation(a, b):
    """between the softmaxes of two score vectors"""
    return 0.5 * float(np.abs(np.exp(log_softmax(a))
                              - np.exp(log_softmax(b))).sum())


def features(shareds):
    return [fx.Feature(s) for s in shareds]
