"""A float64 reference for the batched samplers: the inverse CDF of the
softmax of a row's scores, and, per summation order, a proven band around
every boundary inside which a float32 sampler may pick a neighbour.

TEST INFRASTRUCTURE (imported by tests only).

A batched draw for row r depends on two things: the row's score vector in
batch semantics (`row_scores(r)`, pinned bit-exact to the oracle) and its
uniform u, engine step `draw_base + r` from the seed (oracle.c:1596-1606).
With w_k = exp(s_k - max s), C_k = w_0 + ... + w_k, W = C_{K-1} and t = u W,
all in float64, the mathematical draw is the first k with C_k >= t.

A float32 sampler works with perturbed prefixes and a perturbed target.  If
every comparison it makes between its k-th prefix and its target is off by at
most B_k from the comparison of C_k with t, the index it returns, k^, obeys

    k^ == 0      or  C_{k^-1} <  t + B_{k^-1}
    k^ == K - 1  or  C_{k^}   >= t - B_{k^}

(it went past k^-1, and it stopped at k^ or ran out of groups).  These two
conditions are `accepted`.  Outside the band the index is the float64 one;
inside it only the indices whose interval comes within B of t are allowed.

Every quantity below is scaled by 1 / W, so bands are fractions of the row's
total likelihood.  eps = 2^-24 is the unit roundoff of binary32.  The bands
are bounds, derived from the operations each kernel performs (running-error
analysis: a rounded add, subtract or multiply errs by at most eps times the
magnitude of its result); nothing in them is fitted to observed draws.  The
second-order terms (rounded partials that exceed the exact ones by the error
itself) are covered by dividing by (1 - 2 n eps), n the number of rounded
steps on the longest chain.
"""
import numpy as np

EPS = 2.0 ** -24
# The smallest binary32 normal: what a flushed (FTZ) result can lose, per op.
TINY = 2.0 ** -126

# |fast_exp(x) / exp(x) - 1|, maximum over every binary32 x with
# -(i + 1) < x <= -i (and |x| >= 2^-30 in bin 0), i = 0 .. 86, host fast_exp
# (oracle.c:48-66, bit-identical to the device's), rounded up to 1e-9:
#
#   b = np.arange(f32(2**-30).view(u32), f32(88).view(u32) + 1, dtype=u32)
#   x = (b | 0x80000000).view(f32)
#   r = |orc_vec_fast_exp(x) / np.exp(x.astype(f64)) - 1|
#   np.maximum.at(out, floor(-x), r);  ceil(out * 1e9) / 1e9
#
# The error is the rounding of (x + 1) in fmath's evaluation order, so it
# doubles with each binade of |x|.  Below -87 the result may be flushed to 0:
# there the whole value counts as error (`_fast_exp_err`).
FAST_EXP_REL = np.array([
    3.410e-07, 2.890e-07, 3.580e-07, 3.560e-07, 4.300e-07, 5.060e-07,
    5.030e-07, 4.990e-07, 6.800e-07, 7.220e-07, 7.250e-07, 6.880e-07,
    7.290e-07, 7.330e-07, 7.370e-07, 6.990e-07, 1.185e-06, 1.182e-06,
    1.223e-06, 1.193e-06, 1.189e-06, 1.231e-06, 1.201e-06, 1.238e-06,
    1.192e-06, 1.208e-06, 1.246e-06, 1.199e-06, 1.216e-06, 1.254e-06,
    1.223e-06, 1.220e-06, 2.161e-06, 2.177e-06, 2.189e-06, 2.159e-06,
    2.226e-06, 2.179e-06, 2.192e-06, 2.149e-06, 2.204e-06, 2.242e-06,
    2.194e-06, 2.180e-06, 2.208e-06, 2.160e-06, 2.219e-06, 2.257e-06,
    2.209e-06, 2.223e-06, 2.179e-06, 2.234e-06, 2.272e-06, 2.225e-06,
    2.176e-06, 2.238e-06, 2.191e-06, 2.249e-06, 2.287e-06, 2.240e-06,
    2.253e-06, 2.210e-06, 2.265e-06, 2.235e-06, 4.121e-06, 4.166e-06,
    4.150e-06, 4.170e-06, 4.154e-06, 4.174e-06, 4.190e-06, 4.124e-06,
    4.224e-06, 4.129e-06, 4.183e-06, 4.151e-06, 4.197e-06, 4.181e-06,
    4.201e-06, 4.152e-06, 4.205e-06, 4.154e-06, 4.220e-06, 4.255e-06,
    4.159e-06, 4.213e-06, 4.182e-06])
# v_exp_f32 (the device's exp2 builtin): 1 ulp, the ISA's stated accuracy.
EXP2_REL = 2.0 ** -23
# log2(e) as the kernels hold it (kLog2e, a binary32), and its distance from
# the real number relative to it: < eps / 4.
LOG2E_F32 = float(np.float32(1.44269504088896341))
LOG2E_REL = abs(LOG2E_F32 / 1.4426950408889634074 - 1.0)

# ---------------------------------------------------------------------------
# the row's uniform: minstd_rand0 (random_fwd.hpp:34) restated in numpy

_M = 2147483647
_A = 16807


def rng_seed(seed):
    s = int(seed) % _M
    return 1 if s == 0 else s


def rng_jump(state, steps):
    """state * a^steps mod m, vectorised over `steps` (numpy int64)"""
    steps = np.asarray(steps, np.int64).copy()
    result = np.full(steps.shape, int(state), np.uint64)
    base = np.full(steps.shape, _A, np.uint64)
    m = np.uint64(_M)
    while steps.any():
        odd = (steps & 1).astype(bool)
        result = np.where(odd, (result * base) % m, result)
        base = (base * base) % m
        steps >>= 1
    return result


def uniforms(seed, draw_base, rows):
    """u of rows `rows` of a batch drawn with (seed, draw_base): one engine
    step each, std::uniform_real_distribution<float>(0, 1) over it
    (random.hpp:47-50): float(x - 1) / 2^31, clamped below 1."""
    rows = np.asarray(rows, np.int64)
    x = (rng_jump(rng_seed(seed), int(draw_base) + rows) * np.uint64(_A)
         % np.uint64(_M))
    u = (x - np.uint64(1)).astype(np.float32) / np.float32(2.0 ** 31)
    return np.minimum(u, np.float32(np.nextafter(np.float32(1),
                                                 np.float32(0))))


# ---------------------------------------------------------------------------
# slots and group ids


def slot_to_global(slot, g, kl, K, p2g):
    """the id a batch assigns for a drawn slot (orc_mix_batch_sample,
    oracle.c:1596-1606): a row alone in its group sees Kl = K - 1 slots and
    slot g then holds group K - 1; ids are the pre-batch packed-to-global
    map's (a new group keeps the id its empty slot had)."""
    slot = np.asarray(slot, np.int64)
    g = np.asarray(g, np.int64)
    kl = np.asarray(kl, np.int64)
    s = np.where((kl != K) & (slot == g), K - 1, slot)
    return np.asarray(p2g, np.int64)[s]


# ---------------------------------------------------------------------------
# the float64 inverse CDF


class Rows(object):
    """A batch of checked rows: scores padded with -inf to a common width.

    scores: float32 [R, K]; kl: the valid length of each row; u: float32 [R].
    Attributes (float64, scaled by the row total W): w, C, t; m = max s."""

    def __init__(self, scores, kl, u):
        self.s32 = np.ascontiguousarray(scores, np.float32)
        R, K = self.s32.shape
        self.K = K
        self.kl = np.asarray(kl, np.int64)
        self.valid = np.arange(K)[None, :] < self.kl[:, None]
        s32 = np.where(self.valid, self.s32, np.float32(-np.inf))
        self.s32 = s32
        self.m32 = s32.max(1)
        s = s32.astype(np.float64)
        self.m = s.max(1)
        self.s = s
        w = np.exp(s - self.m[:, None])
        w[~self.valid] = 0.0
        W = w.sum(1)
        self.W = W
        self.w = w / W[:, None]
        self.C = np.cumsum(self.w, 1)
        self.u = np.asarray(u, np.float64)
        self.t = self.u * self.C[np.arange(R), self.kl - 1]
        # (s - m) at full precision, >= 0
        self.gap = np.where(self.valid, self.m[:, None] - s, 0.0)
        self.scale = 1.0 / W      # converts an absolute (max = 1) error

    def index(self):
        """the float64 draw: first k with C_k >= t (C_{Kl-1} = 1 >= t)"""
        k = (self.C < self.t[:, None]).sum(1)
        return np.minimum(k, self.kl - 1)


def accepted(rows, B, drawn):
    """-> (ok[R], excursion[R], in_band[R]).  excursion: how far outside the
    float64 interval t lies, as a fraction of the band at the boundary the
    draw went past (0 where the draw is the float64 index; <= 1 where it is
    accepted).  in_band: some boundary of the row lies within its band of t,
    so more than one index is allowed."""
    R = rows.C.shape[0]
    r = np.arange(R)
    k = np.asarray(drawn, np.int64)
    C, t = rows.C, rows.t
    lo_ok = (k == 0) | (C[r, np.maximum(k - 1, 0)]
                        < t + B[r, np.maximum(k - 1, 0)])
    hi_ok = (k >= rows.kl - 1) | (C[r, np.minimum(k, rows.K - 1)]
                                  >= t - B[r, np.minimum(k, rows.K - 1)])
    ok = lo_ok & hi_ok & (k >= 0) & (k < rows.kl)
    k64 = rows.index()
    exc = np.zeros(R)
    above = (k > k64) & (k < rows.kl)     # went past boundary k - 1 too early
    km = np.maximum(k - 1, 0)
    exc[above] = ((C[r, km] - t) / np.maximum(B[r, km], 1e-300))[above]
    below = (k < k64) & (k >= 0)          # stopped before reaching t
    kc = np.clip(k, 0, rows.K - 1)
    exc[below] = ((t - C[r, kc]) / np.maximum(B[r, kc], 1e-300))[below]
    exc[(k < 0) | (k >= rows.kl)] = np.inf
    near = (np.abs(C - t[:, None]) <= B) & rows.valid
    near[r, rows.kl - 1] = False          # (C_{Kl-1} = 1 is no boundary)
    return ok, exc, near.any(1)


def _second_order(B, n):
    return B / (1.0 - 2.0 * n * EPS)


def _fast_exp_err(rows):
    """per entry, |l_k - w_k| (scaled) for l_k = fast_exp(fl(s_k - m)):
    the rounded argument's own effect, computed exactly, plus FAST_EXP_REL
    of its bin; below -87 the whole value (it may be flushed)."""
    d32 = (rows.s32 - rows.m32[:, None]).astype(np.float64)   # fl(s - m)
    d32 = np.where(rows.valid, d32, 0.0)
    e32 = np.exp(d32) * rows.scale[:, None]
    arg = np.abs(e32 - rows.w)
    b = np.minimum(np.floor(-d32).astype(np.int64), 87)
    rel = np.append(FAST_EXP_REL, 1.0)[b]
    err = arg + rel * e32 + TINY * rows.scale[:, None]
    return np.where(rows.valid, err, 0.0)


def band_exact(rows):
    """The reference's sampler (random.cc:94-106, random.hpp:316-333;
    oracle.c:221-236) and every exact kernel, bit-identical to it:

        l_k = fast_exp(fl(s_k - m));  total = (..(l_0 + l_1) + ..) + l_{K-1}
        t^ = fl(total * u);  t_k = fl(t_{k-1} - l_k);  first k with t_k <= 0

    Terms of |t_k - (t - C_k)|:
      e_j        |l_j - w_j|: the argument's rounding (exact) and the measured
                 FAST_EXP_REL (per bin of |s_j - m|); A_k = sum_{j<=k} e_j;
      u (A + eps sum_{j>=1} C_j)   the ascending sum's error, scaled by u;
      eps t      the product total * u;
      eps sum_{j<=k} |t - C_j|     the running subtraction;
    with the partial sums taken at their float64 values plus A (first order),
    the rest in _second_order (n = 2 K rounded steps)."""
    e = _fast_exp_err(rows)
    A = np.cumsum(e, 1)
    At = A[np.arange(len(A)), rows.kl - 1]
    C, t, u = rows.C, rows.t[:, None], rows.u[:, None]
    total_err = EPS * (np.where(rows.valid, C + A, 0.0)[:, 1:].sum(1))[:, None]
    sub = EPS * np.cumsum(np.where(rows.valid, np.abs(t - C) + A + u * At[:, None],
                                   0.0), 1)
    B = A + u * (At[:, None] + total_err) + EPS * (t + At[:, None]) + sub
    return _second_order(B, 2 * rows.K)


def band_rows_scan(rows, super_=32, block=8):
    """k_rows_scratch with SCAN (kernels_rows.h:973-1130): one pass of a
    running log-sum-exp over blocks of 8 groups -- running maximum m_i,
    S = S * exp2(fl(fl(m_i - m_new) L)) when it grows, S += exp2(fma(s, L,
    fl(-m L))) -- a snapshot (S, m_i) every 32 groups, target = fl(S u), the
    block located by v.x * exp2(fl(fl(v.y - m) L)) >= target and its 32
    groups summed again from the snapshot before it.  L = fl(log2 e).

    Per entry j, relative to the final frame (in units of ln 2 log2-exponent
    error, ln 2 L = 1):
      fma:        |s_j - m_i| (eps + LOG2E_REL) + |m_i| eps   (fl(-m_i L))
      rescales:   sum over them of |dm| (2 eps + LOG2E_REL) <= (m - s_j) (..),
                  each also EXP2_REL and one rounded multiply
      the frames' fl(-m_i L) differ from the final one's: (|m_i| + |m|) eps
    so rho_j <= 2.5 eps (m - s_j) + 2 eps max|s| [any rescale]
                + (n_r + 2)(EXP2_REL + eps),  n_r the blocks that raised the
    running maximum.  Summation: eps sum_{j<=k} C_j (the running sum S),
    eps sum over the block's groups <= k of C_j (the re-summation), u times
    the whole running sum's error for the target, eps t for the product."""
    R, K = rows.s32.shape
    nb = (K + block - 1) // block
    pad = np.full((R, nb * block), -np.inf, np.float32)
    pad[:, :K] = rows.s32
    bm = pad.reshape(R, nb, block).max(2)
    run = np.maximum.accumulate(bm, 1)
    n_r = (bm[:, 1:] > run[:, :-1]).sum(1)
    sabs = np.where(rows.valid, np.abs(rows.s), 0.0).max(1)
    rho = (2.5 * EPS * rows.gap + 2.0 * EPS * sabs[:, None] * (n_r > 0)[:, None]
           + (n_r[:, None] + 2) * (EXP2_REL + EPS))
    e = np.where(rows.valid, rho * rows.w + 2 * TINY * rows.scale[:, None], 0.0)
    A = np.cumsum(e, 1)
    At = A[np.arange(R), rows.kl - 1]
    C, t, u = rows.C, rows.t[:, None], rows.u[:, None]
    Cv = np.where(rows.valid, C + A, 0.0)
    running = EPS * np.cumsum(Cv, 1)
    tot = running[np.arange(R), rows.kl - 1][:, None]
    # the re-summation inside the located block of super_ groups
    blk = np.zeros_like(Cv)
    for j0 in range(0, K, super_):
        blk[:, j0:j0 + super_] = np.cumsum(Cv[:, j0:j0 + super_], 1)
    B = (A + running + EPS * blk + u * (At[:, None] + tot)
         + EPS * (t + At[:, None]))
    return _second_order(B, 2 * K)


def vs_scan_depth(K, block=256, coarse=64):
    """rounded adds on the longest path from a likelihood to C[x][k] in
    k_vs_scan_prepare (kernels_vs.h:1310-1356): 3 inside a thread's four,
    6 levels of __shfl_up, then before = carry + <= 3 wave sums + (run -
    l[3]) and + l[i]: 14 within a round of 4 * 256 entries; the carry of an
    earlier round passes 5 more per round.  +2: the subtraction run - l[3]
    counts the thread's own entries in two nodes."""
    kpad = (K + coarse - 1) // coarse * coarse
    rounds = (kpad + 4 * block - 1) // (4 * block)
    return 16 + 5 * (rounds - 1)


def band_vs_scan(rows, g, s_tab_g):
    """k_vs_scan_prepare / k_vs_scan_rows (kernels_vs.h:1236-1420): per value
    x the tabulated scores (the row's own slot g with the row included:
    s_tab_g), l_k = exp2(fma(s_k, L, fl(-M L))) with M their maximum, C[x]
    their inclusive scan (depth D, vs_scan_depth); for the row
    delta = fl(l_own - l_g), target = fl(fl(total + delta) u), the first k
    with fl(C[x][k] + (k >= g ? delta : 0)) >= target by binary search (first
    over the 64-entry block ends, then inside the block: either way the
    returned index satisfies the two conditions of `accepted`).

    fl(-M L) is common to every entry and to the target: it cancels.  Per
    entry rho_k = 1.25 eps |s_k - M| + eps + EXP2_REL (the fma's rounding
    and L's).  The tabulated l_g enters the prefixes and delta through the
    same operations (it cancels too); it is bounded here all the same, twice.
    Summation: D eps times the tabulated prefix (node values of the scan
    never exceed the prefix up to the thread's fourth entry), eps for the
    correction's add and for delta, u times the total's error, eps t."""
    R, K = rows.s32.shape
    r = np.arange(R)
    g = np.asarray(g, np.int64)
    D = vs_scan_depth(K)
    s_tab_g = np.asarray(s_tab_g, np.float64)
    M = np.maximum(rows.m, s_tab_g)
    # (scaled) tabulated likelihood of slot g, and the own one
    wtab = np.exp(s_tab_g - rows.m) * rows.scale
    wown = rows.w[r, g]
    gapM = np.where(rows.valid, M[:, None] - rows.s, 0.0)
    rho = 1.25 * EPS * gapM + EPS + EXP2_REL
    e = np.where(rows.valid, rho * rows.w + 2 * TINY * rows.scale[:, None], 0.0)
    rho_g = 1.25 * EPS * (M - s_tab_g) + EPS + EXP2_REL
    eg = 2 * rho_g * wtab
    ge = np.arange(K)[None, :] >= g[:, None]
    A = np.cumsum(e, 1) + ge * eg[:, None]
    At = A[r, rows.kl - 1]
    dabs = np.abs(wown - wtab)
    Ctab = rows.C + ge * (wtab - wown)[:, None]
    # node values: up to the thread's fourth entry
    k4 = np.minimum(np.arange(K) | 3, rows.kl[:, None] - 1)
    Cnode = np.take_along_axis(np.maximum(Ctab, 0.0), k4, 1) + A
    C, t, u = rows.C, rows.t[:, None], rows.u[:, None]
    Wtab = Ctab[r, rows.kl - 1] + At
    B = (A + D * EPS * Cnode + EPS * (C + A) + ge * EPS * dabs[:, None]
         + u * (At + D * EPS * Wtab + EPS * (1 + At) + EPS * dabs)[:, None]
         + EPS * (t + At[:, None]))
    return _second_order(B, D + 4)


def band_crude(rows):
    """the issue's yardstick: 2 (K + 3) eps W"""
    return np.full(rows.C.shape, 2.0 * (rows.K + 3) * EPS)


class Report(object):
    """what every checked case prints"""

    def __init__(self, name):
        self.name = name
        self.n = self.differ = self.inband = self.bad = 0
        self.worst = 0.0
        self.first_bad = None

    def add(self, rows, B, drawn, ids=None):
        ok, exc, near = accepted(rows, B, drawn)
        k64 = rows.index()
        self.n += len(ok)
        self.differ += int((np.asarray(drawn) != k64).sum())
        self.inband += int(near.sum())
        self.bad += int((~ok).sum())
        if (~ok).any() and self.first_bad is None:
            i = int(np.nonzero(~ok)[0][0])
            self.first_bad = (ids[i] if ids is not None else i,
                              int(np.asarray(drawn)[i]), int(k64[i]),
                              float(exc[i]))
        fin = exc[np.isfinite(exc)]
        if fin.size:
            self.worst = max(self.worst, float(fin.max()))
        if (~np.isfinite(exc)).any():
            self.worst = np.inf
        return ok

    def line(self):
        return ("%s: %d rows, %.4f %% differ from float64, %d inside a band, "
                "worst excursion %.3g of the band, %d outside%s"
                % (self.name, self.n, 100.0 * self.differ / max(self.n, 1),
                   self.inband, self.worst, self.bad,
                   "" if self.first_bad is None else
                   " (first: row %s drew %d, float64 %d, excursion %.3g)"
                   % self.first_bad))
