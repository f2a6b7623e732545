"""What dist_group_sample_value and dist_gibbs_sample_rows must return.

TEST INFRASTRUCTURE (imported by tests only).

  cell_word      the Python restatement of csrc/sample.h, operation by
                 operation: the counter-based stream, Marsaglia's polar normal,
                 Marsaglia-Tsang's gamma, inversion / Hoermann's PTRS for the
                 Poisson, and the six kinds' draws.  Python's float is the
                 platform's binary64 and math.log / exp / sqrt are the C
                 library's; math.lgamma is CPython's own, which is why a PTRS
                 acceptance may part in its last place (`ptrs_margin`).
  law_pmf, nich_t
                 the float64 laws a draw is held to: exp of
                 f64_scores.float64_score (+ bnb_log_binomial for BNB), from
                 the group's MEMBERS, not from the statistic words.
  chi2_p, pair_p the tests' statistics: chi-square over cells merged to an
                 expected count >= 50; independence of a pair.
  expect_groups  the expected group under a mask: feature_expect.expect's
                 `base` fold (driver score_value, then every observed
                 feature's in feature order), then
                 orc_sample_from_scores_overwrite on
                 orc_rng_jump(seed_state, draw_base + q); global ids.
"""
import ctypes
import math

import numpy as np
from scipy import stats

import f64_scores as fx
import oracle_lib as ol

DD, BB, GP, NICH, DPD, BNB = fx.DD, fx.BB, fx.GP, fx.NICH, fx.DPD, fx.BNB
OTHER = fx.OTHER
M64 = (1 << 64) - 1
COUNT_MAX = 2147483647


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class Stream(object):
    """cell (row, f) of seed_state's stream of uniforms in (0, 1)"""

    def __init__(self, seed_state, row, f):
        self.key = mix64(mix64(mix64(seed_state) ^ row) ^ (f + 1))
        self.j = 0
        self.exhausted = False
        # the smallest |lhs - rhs| over the PTRS acceptance tests that called
        # lgamma, relative to their magnitude (None: none did)
        self.ptrs_margin = None

    def u(self):
        w = mix64((self.key + self.j) & M64)
        self.j += 1
        return (float(w >> 11) + 0.5) * 2.0 ** -53


def normal(s):
    for _ in range(64):
        a = 2.0 * s.u() - 1.0
        b = 2.0 * s.u() - 1.0
        r = a * a + b * b
        if 0.0 < r < 1.0:
            return a * math.sqrt(-2.0 * math.log(r) / r)
    s.exhausted = True
    return 0.0


def gamma(s, a):
    boost = 1.0
    if a < 1.0:
        boost = math.exp(math.log(s.u()) / a)
        a += 1.0
    d = a - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    for _ in range(64):
        z = normal(s)
        v = 1.0 + c * z
        if v <= 0.0:
            continue
        v = v * v * v
        w = s.u()
        z2 = z * z
        if w < 1.0 - 0.0331 * (z2 * z2):
            return d * v * boost
        if math.log(w) < 0.5 * z2 + d * (1.0 - v + math.log(v)):
            return d * v * boost
    s.exhausted = True
    return d * boost


def count_word(k):
    if not k < 2147483647.0:
        return COUNT_MAX
    return 0 if k < 0.0 else int(k)


def poisson(s, lam):
    if not lam < 2147483648.0:
        return COUNT_MAX
    if lam < 10.0:
        p = math.exp(-lam)
        w = s.u()
        k = 0
        cum = p
        while w > cum and k < 1000:
            k += 1
            p *= lam / float(k)
            cum += p
        return k
    b = 0.931 + 2.53 * math.sqrt(lam)
    a = -0.059 + 0.02483 * b
    ia = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    log_lam = math.log(lam)
    for _ in range(64):
        U = s.u() - 0.5
        V = s.u()
        us = 0.5 - abs(U)
        k = math.floor((2.0 * a / us + b) * U + lam + 0.43)
        k = float(k)
        if us >= 0.07 and V <= vr:
            return count_word(k)
        if k < 0.0 or (us < 0.013 and V > us):
            continue
        lhs = math.log(V) + math.log(ia) - math.log(a / (us * us) + b)
        lg = math.lgamma(k + 1.0)
        rhs = -lam + k * log_lam - lg
        margin = abs(lhs - rhs) / max(abs(lg), abs(lam), 1.0)
        if s.ptrs_margin is None or margin < s.ptrs_margin:
            s.ptrs_margin = margin
        if lhs <= rhs:
            return count_word(k)
    s.exhausted = True
    return count_word(float(math.floor(lam)))


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def cell_word(shared, group, seed_state, row, f, stream_out=None):
    """sample_cell_word: `shared` an oracle_lib / engine Shared (kind, dim, p,
    alphas / betas), `group` its statistic words.  -> the uint32 word"""
    kind = int(shared.kind)
    p = [float(np.float32(x)) for x in shared.p]
    g = np.asarray(group, np.uint32)
    i32 = g.view(np.int32)
    s = Stream(seed_state, row, f)
    if stream_out is not None:
        stream_out.append(s)
    if kind in (DD, DPD):
        dim = int(shared.dim)
        if kind == DD:
            w = [float(np.float32(shared.alphas[v])) + float(i32[1 + v])
                 for v in range(dim)]
            other = 0.0
        else:
            alpha = p[0]
            betas = _betas(shared)
            w = [float(betas[v]) * alpha + float(i32[1 + v])
                 for v in range(dim)]
            other = p[1] * alpha
        total = 0.0
        for a_v in w:
            total += a_v
        if other > 0.0:
            total += other
        t = s.u() * total
        for v in range(dim):
            t -= w[v]
            if t < 0.0:
                return v
        return OTHER if other > 0.0 else dim - 1
    if kind == BB:
        a = p[0] + float(i32[0])
        b = p[1] + float(i32[1])
        return 1 if s.u() < a / (a + b) else 0
    if kind == GP:
        shape = p[0] + float(i32[1])
        rate = p[1] + float(i32[0])
        return poisson(s, gamma(s, shape) / rate)
    if kind == BNB:
        r = p[2]
        a = p[0] + r * float(i32[0])
        b = p[1] + float(i32[1])
        x = gamma(s, a)
        y = gamma(s, b)
        if x == 0.0 and y == 0.0:
            pp = 1.0 if s.u() < a / (a + b) else 0.0
        else:
            pp = x / (x + y)
        gr = gamma(s, r)
        lam = gr * (1.0 - pp) / pp if pp != 0.0 else math.inf
        return poisson(s, lam)
    assert kind == NICH
    mu, kappa, sigmasq, nu = p
    n = float(i32[0])
    mean = float(g[1:2].view(np.float32)[0])
    ctv = float(g[2:3].view(np.float32)[0])
    kn = kappa + n
    mun = (kappa * mu + mean * n) / kn
    nun = nu + n
    dm = mu - mean
    sn = (nu * sigmasq + ctv + n * kappa * (dm * dm) / kn) / nun
    z = normal(s)
    gg = gamma(s, nun / 2.0)
    return f32_bits(mun + math.sqrt(sn * (kn + 1.0) / kn) * z
                    * math.sqrt(nun / (2.0 * gg)))


def _betas(shared):
    b = shared.betas
    if isinstance(b, np.ndarray):
        return b.astype(np.float32)
    return np.array([b[v] for v in range(int(shared.dim))], np.float32)


# ---------------------------------------------------------------------------
# the float64 laws


def law_pmf(kind, kw, members, bnb_binomial=True, tail=1e-9):
    """-> (values, pmf) of the posterior predictive given the group's members
    (DPD: the last value is OTHER when it has mass); counts are listed up to
    where the remaining mass is below `tail` (chi2_p gives the remainder a
    cell of its own, merged with its neighbours)"""
    if kind == DD:
        xs = list(range(len(kw["alphas"])))
    elif kind == DPD:
        xs = list(range(len(kw["betas"])))
        if kw.get("beta0", 0.0) > 0:
            xs.append(OTHER)
    elif kind == BB:
        xs = [0, 1]
    else:
        xs, pm, mass = [], [], 0.0
        x = 0
        while mass < 1.0 - tail and x < 200000:
            lp = float(fx.float64_score(kind, kw, members, x))
            if kind == BNB and bnb_binomial:
                lp += float(fx.bnb_log_binomial(float(int(kw["r"])), x))
            xs.append(x)
            pm.append(math.exp(lp))
            if kind == BNB and not bnb_binomial:
                # (not normalised: stop where the terms have died out)
                if x > 50 and pm[-1] < tail * sum(pm):
                    break
            else:
                mass += pm[-1]
            x += 1
        pm = np.array(pm)
        if kind == BNB and not bnb_binomial:
            pm = pm / pm.sum()
        return np.array(xs, np.int64), pm
    pm = np.array([math.exp(float(fx.float64_score(kind, kw, members, x)))
                   for x in xs])
    return np.array(xs, np.int64), pm


def nich_t(kw, members, scale_bug=False):
    """the Student-t law of a NICH group's predictive (scipy frozen)"""
    v = np.asarray(members, np.float64)
    n = len(v)
    mu, kappa, sigmasq, nu = kw["mu"], kw["kappa"], kw["sigmasq"], kw["nu"]
    mean = v.mean() if n else 0.0
    ctv = ((v - mean) ** 2).sum() if n else 0.0
    kn = kappa + n
    mun = (kappa * mu + mean * n) / kn
    nun = nu + n
    sn = (nu * sigmasq + ctv + n * kappa * (mu - mean) ** 2 / kn) / nun
    scale = math.sqrt(sn if scale_bug else sn * (kn + 1.0) / kn)
    return stats.t(nun, loc=mun, scale=scale)


def chi2_p(draws, values, pmf, min_expected=50.0):
    """p-value of the draws' histogram against (values, pmf): cells merged in
    order to an expected count >= min_expected; whatever falls outside
    `values` (a count beyond the listed ones) goes into the last cell with
    the law's remaining mass"""
    draws = np.asarray(draws, np.int64)
    n = len(draws)
    index = {int(v): i for i, v in enumerate(values)}
    obs = np.zeros(len(values) + 1)
    for v, c in zip(*np.unique(draws, return_counts=True)):
        obs[index.get(int(v), len(values))] += c
    exp = np.append(pmf, max(0.0, 1.0 - float(np.sum(pmf)))) * n
    cells_o, cells_e = [], []
    o = e = 0.0
    for oi, ei in zip(obs, exp):
        o += oi
        e += ei
        if e >= min_expected:
            cells_o.append(o)
            cells_e.append(e)
            o = e = 0.0
    if cells_e:
        cells_o[-1] += o
        cells_e[-1] += e
    else:
        cells_o, cells_e = [o], [e]
    cells_o = np.array(cells_o)
    cells_e = np.array(cells_e)
    if len(cells_e) < 2:
        return 1.0 if cells_o[0] == n else 0.0
    chi = ((cells_o - cells_e) ** 2 / cells_e).sum()
    return float(stats.chi2.sf(chi, len(cells_e) - 1))


def pair_p(a, b):
    """p-value of independence of two columns of small integers"""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    ua, ia = np.unique(a, return_inverse=True)
    ub, ib = np.unique(b, return_inverse=True)
    table = np.zeros((len(ua), len(ub)))
    np.add.at(table, (ia, ib), 1)
    if min(table.shape) < 2:
        return 1.0
    return float(stats.chi2_contingency(table)[1])


# ---------------------------------------------------------------------------
# the expected group


def expect_groups(orc, qvals, observed, seed_state, draw_base, nq=None):
    """-> global ids [nq] (uint32).  observed: uint32 masks, or None: nothing
    observed (qvals is then not read and nq tells the rows)"""
    L = orc.L
    K = len(orc)
    F = orc.F
    sh = orc.shareds
    if observed is not None:
        nq = len(observed)
    words = None
    if observed is not None and qvals is not None:
        words = []
        for f, v in enumerate(qvals):
            if v is None:
                words.append(None)
                continue
            w = ol.value_words(sh[f].kind, v).copy()
            if sh[f].kind == ol.DPD:
                # dpd.hpp:534-542: a value the table does not hold is OTHER
                w[w >= sh[f].dim] = OTHER
            words.append(w)
    p2g = np.array([orc.packed_to_global(k) for k in range(K)], np.uint32)
    prior = np.zeros(K, np.float32)
    L.orc_mix_driver_score_value(orc.h, prior)
    out = np.zeros(nq, np.uint32)
    for q in range(nq):
        ob = 0 if observed is None else int(observed[q])
        s = prior.copy()
        for f in range(F):
            if (ob >> f) & 1:
                L.orc_mix_slave_score_value(orc.h, f, int(words[f][q]), s)
        st = ctypes.c_uint32(L.orc_rng_jump(seed_state, draw_base + q))
        out[q] = p2g[L.orc_sample_from_scores_overwrite(ctypes.byref(st), K,
                                                        s)]
    return out
