"""A float64 reference for the float statistics themselves -- NICH (count,
mean, count_times_variance) and GammaPoisson's log_prod -- and a band around
each derived from the operations that maintain them.

TEST INFRASTRUCTURE (imported by tests only).  Like f64_marginals it reads
nothing from the engine's or the oracle's statistics: everything is rebuilt
from the columns, the assignments and the history of assignments.

  truth           per global group id and float feature: n, the two-pass
                  float64 mean, sum (x - mean)^2, and sum log x! (gammaln)
  ordered paths   (the sorted replay, the additions-only replay of a load,
                  the sequential chain's stats_add / stats_remove: binary32
                  running updates, nich.hpp:125-165, gp.hpp:115,134) are held
                  to f64_scores.nich_welford_bounds and
                  f64_marginals.gp_log_prod_bounds as they are, the history
                  being the assignment after every SWEEP
  merged path     (option "float_stats" = 1: k_merge_float_moves / _reduce /
                  _apply / _export) is held to `merged_bounds`, the history
                  being the assignment after every SUB-SWEEP: its error is
                  per batch, not per event

The merged bound, per touched group and batch.  u = 2^-24, v = 2^-53.  The
group's true moments go (n0, mu0, C0) -> (n1, mu1, C1), Q = C + n mu^2 is the
true sum of squares, the stored binary32 (m0, c0) are within (em0, ec0) of
(mu0, C0).  In the kernels' order:

  k_merge_float_moves, k_merge_float_reduce
      dn exact (whole numbers).  dx, dxx: binary64 sums of +-x and +-x^2
      (x^2 of a binary32 x is exact in binary64) over the group's L moved
      rows, by LDS atomics in no fixed order, then over the workgroups'
      partial sums in order.  Any order of at most `ops` = L + workgroups
      additions is within g = ops v / (1 - ops v) times the sum of the
      magnitudes:  edx = g sum|x|,  edxx = g sum x^2.
  k_merge_float_apply
      p = n0 m0 is exact (24 x 24 bits).  s1 = fl(p + dx), mean1 =
      fl(s1 / n1):
        mean1 - mu1 = n0 (m0 - mu0) / n1 + eta,
        |eta| <= (edx + v |s1|) / n1 + v |mean1|            =: e_eta
        em1 = n0 em0 / n1 + e_eta + u |mean1|               (the narrowing)
      s2 = fl(fl(c0 + fl(p m0)) + dxx), z = fl(fl(n1 mean1) mean1),
      ctv1 = fl(s2 - z).  Writing d = m0 - mu0 and expanding both squares,
      the terms 2 n0 d mu0 of s2 and 2 n0 d mu1 of z meet:
        ctv1 - C1 = (c0 - C0) + 2 n0 d (mu0 - mu1) + n0 d^2 (1 - n0 / n1)
                    - 2 n0 d eta - n1 eta^2 - 2 mu1 n1 eta
                    + (dxx - DXX) + roundings
        ec1 = ec0 + 2 n0 em0 |mu0 - mu1| + n0 em0^2 |1 - n0 / n1|
              + 2 n0 em0 e_eta + n1 e_eta^2 + 2 |mu1| n1 e_eta + edxx
              + v (n0 m0^2 + |c0 + n0 m0^2| + |s2| + 2 |z| + |ctv1|)
              + u |ctv1|                                    (the narrowing)
      (the five v terms: fl(p m0), the two additions of s2, the two products
      of z -- |fl(n1 mean1)| |mean1| is |z| again --, the subtraction.)
      n1 < 2: ctv1 = 0 = C1, ec1 = 0.  n1 < 1: mean1 = 0, em1 = 0.  The clamp
      at 0 never increases the distance from a non-negative truth.  A group
      the kernel SKIPS because its three sums came out zero has a truth that
      moved by no more than edx / n and edxx + 2 |mu| edx, which the terms
      above contain.
  start = "import"  (import_float_moments_dev, reset = 1: n0 = 0) of an image
      the test sums exactly and rounds once (math.fsum): edx = v |S|,
      edxx = v Q.
  start = "load"    the load's binary32 additions in row order: the ordered
      bounds with history[:1].
  GammaPoisson  d = binary64 sum of +-(double) fast_log_factorial(x) over the
      moved rows: ed = g sum|lf|; log_prod1 = (float) fl(log_prod0 + d):
      (u + v) |log_prod1|; plus |fast_log_factorial(x) - log x!| -- from a
      load, over the CURRENT members (added when a row comes, taken back
      when it leaves, as gp_log_prod_bounds has it); from an import of true
      sums, over every row that has moved since (nothing to cancel against).

Magnitudes of computed values are bounded by the true value plus the error
bound so far; SLACK covers the second-order terms.  Nothing is fitted to
kernel, oracle or restatement output.

`Restated` is a plain numpy restatement of the three kernels (binary64 sums,
binary32 state, the skip of untouched groups, the n1 >= 1 / n1 >= 2 branches,
the clamp, reset, export).  It exists so that the band and the planted bugs
can be checked without a GPU; it is NOT the reference.  Planted bugs, mut=:
  sq_f32            x * x in binary32 before widening
  no_recentre       n0 mean0^2 left out of s2
  skip_n_unchanged  a group whose count did not change is skipped although
                    its members did
  stale_on_empty    mean and ctv kept when n1 == 0
  var_at_one        ctv computed at n1 == 1
  gp_sign           the removed rows' log x! added
Float64-side mutants (`truth(mut=)`), for every path:
  lost_add          one member of the largest group, the one at the median
                    |x - mean|, missing from the truth's sums
  lost_remove       a row that left in the last step is still in the sums of
                    the group it left (the largest such group)
  gp_factorial_off  log (x - 1)! for one member of the largest group
"""
import math

import numpy as np

import f64_marginals as fm
import f64_scores as fx
from f64_scores import EPS, GP, NICH

U = EPS              # binary32 unit roundoff
V = 2.0 ** -53       # binary64 unit roundoff
SLACK = 1.0 + 1e-6
KAPPLY_ROWS = 8192   # kApplyLdsRows: rows per workgroup of k_merge_float_moves

KERNEL_MUTANTS = ["sq_f32", "no_recentre", "skip_n_unchanged",
                  "stale_on_empty", "var_at_one", "gp_sign"]
TRUTH_MUTANTS = ["lost_add", "lost_remove", "gp_factorial_off"]


def float_features(shareds):
    """[(feature index, kind)] of the features with float statistics"""
    return [(f, int(s.kind)) for f, s in enumerate(shareds)
            if int(s.kind) in (NICH, GP)]


def _x64(col):
    return np.asarray(col).view(np.float32).astype(np.float64) \
        if np.asarray(col).dtype != np.float32 \
        else np.asarray(col, np.float32).astype(np.float64)


def _log_fact(col):
    """(float64 log x!, binary32 fast_log_factorial(x) widened)"""
    return fm._log_factorials(np.ascontiguousarray(col, np.uint32))


# ---------------------------------------------------------------------------
# the truth


def _moments(x):
    n = len(x)
    if not n:
        return 0, 0.0, 0.0
    mean = math.fsum(x) / n
    return n, mean, math.fsum((x - mean) ** 2)


def truth(cols, shareds, assign, mut=(), prev=None):
    """-> {feature: {global id: (n, mean, ctv)}} for NICH,
    {feature: {global id: (n, sum log x!)}} for GammaPoisson.  n is always
    the members' number; a planted bug (one of TRUTH_MUTANTS; lost_remove
    needs `prev`, the assignment before the last step) changes the sums of
    one group only."""
    assign = np.asarray(assign, np.int64)
    ids, inv, cnt = np.unique(assign, return_inverse=True, return_counts=True)
    order = np.argsort(inv, kind="stable")
    starts = np.r_[0, np.cumsum(cnt)]
    big = int(np.argmax(cnt)) if len(cnt) else -1
    if "lost_remove" in mut:
        # the largest group that a row left in the last step
        assert prev is not None, "lost_remove needs the previous assignment"
        prev = np.asarray(prev, np.int64)
        lost = set(prev[prev != assign].tolist())
        cand = [j for j, g in enumerate(ids.tolist()) if g in lost]
        big = max(cand, key=lambda j: cnt[j]) if cand else -1
    out = {}
    for f, kind in float_features(shareds):
        x = _x64(cols[f]) if kind == NICH else _log_fact(cols[f])[0]
        res = {}
        for j, gid in enumerate(ids.tolist()):
            rows = order[starts[j]:starts[j + 1]]
            xs = x[rows]
            if j == big and mut:
                xs = _mutated(mut, kind, cols[f], x, rows, assign, prev,
                              int(gid))
            n = len(rows)
            if kind == NICH:
                _, mean, ctv = _moments(xs)
                res[gid] = (n, mean, ctv)
            else:
                res[gid] = (n, math.fsum(xs))
        out[f] = res
    return out


def _mutated(mut, kind, col, x, rows, assign, prev, gid):
    xs = x[rows]
    if "lost_add" in mut and len(rows) > 1:
        v = _x64(col)[rows] if kind == NICH else np.asarray(
            col, np.float64)[rows]
        dev = np.abs(v - v.mean())
        drop = int(np.argsort(dev, kind="stable")[len(dev) // 2])
        xs = np.delete(xs, drop)
    if "lost_remove" in mut:
        left = np.nonzero((prev == gid) & (assign != gid))[0]
        if len(left):
            xs = np.r_[xs, x[left[0]]]
    if "gp_factorial_off" in mut and kind == GP:
        c = np.asarray(col, np.int64)[rows]
        at = np.nonzero(c >= 2)[0]
        if len(at):
            xs = xs.copy()
            xs[at[0]] -= math.log(float(c[at[0]]))
    return xs


def image_of(cols, shareds, assign):
    """the float64 image (n, sum x, sum x^2 | sum log x!) per global id that
    import_float_moments_dev installs: every sum exact, rounded once
    -> {feature: {global id: (n, S, Q)} or {global id: (lp,)}}"""
    assign = np.asarray(assign, np.int64)
    out = {}
    for f, kind in float_features(shareds):
        x = _x64(cols[f]) if kind == NICH else _log_fact(cols[f])[0]
        res = {}
        for gid in np.unique(assign).tolist():
            xs = x[assign == gid]
            if kind == NICH:
                res[gid] = (float(len(xs)), math.fsum(xs), math.fsum(xs * xs))
            else:
                res[gid] = (math.fsum(xs),)
        out[f] = res
    return out


# ---------------------------------------------------------------------------
# the merged path's bound


def _g(ops):
    return ops * V / (1.0 - ops * V)


def nich_merge_step(n0, mu0, C0, em0, ec0, n1, mu1, C1, edx, edxx):
    """(em1, ec1) after one k_merge_float_apply of a group (module
    docstring); edx, edxx bound the image's sums against the exact ones"""
    if n1 < 1:
        return 0.0, 0.0
    m0 = abs(mu0) + em0                        # |m0| at most
    S1 = abs(n1 * mu1) + n0 * em0 + edx        # |s1| at most (before fl)
    mean1 = abs(mu1) + (n0 * em0 + edx) / n1   # |mean1| at most (before fl)
    e_eta = ((edx + V * S1) / n1 + V * mean1) * SLACK
    em_d = n0 * em0 / n1 + e_eta
    em1 = (em_d + U * (abs(mu1) + em_d)) * SLACK
    if n1 < 2:
        return em1, 0.0
    Q1 = C1 + n1 * mu1 * mu1
    q = n0 * m0 * m0
    t = C0 + ec0 + q
    s2 = Q1 + ec0 + n0 * em0 * (2.0 * abs(mu0) + em0) + edxx
    z = n1 * (abs(mu1) + em_d) ** 2
    e_d = (ec0 + 2.0 * n0 * em0 * abs(mu0 - mu1)
           + n0 * em0 * em0 * abs(1.0 - n0 / n1)
           + 2.0 * n0 * em0 * e_eta + n1 * e_eta * e_eta
           + 2.0 * abs(mu1) * n1 * e_eta + edxx)
    e_d += V * (q + t + s2 + 2.0 * z + (C1 + e_d)) * SLACK
    ec1 = (e_d + U * (C1 + e_d)) * SLACK
    return em1, ec1


def export_bounds(n, mu, em, ec):
    """bounds on the exported (sum x, sum x^2) of k_merge_float_export --
    n mean32 (exact) and fl(ctv32 + fl(n mean32 mean32)) -- against the
    rows' sums:  n em  and  ec + 2 n |mu| em + n em^2  (+ two roundings)"""
    es = n * em
    q = n * (abs(mu) + em) ** 2
    return es, (ec + 2.0 * n * abs(mu) * em + n * em * em) * SLACK + 2.0 * V * q


def merged_bounds(cols, shareds, history, start, blocks=None):
    """history: the assignment (global ids) at the start and after every
    sub-sweep.  start: "load" or "import".  blocks: workgroups of
    k_merge_float_moves (default: what all rows at once would take, an upper
    bound for every batch).
    -> a list, one entry per entry of history, of
       {feature: {global id: (n, em, ec)} or {global id: (n, elp)}}"""
    assert start in ("load", "import")
    history = [np.asarray(h, np.int64) for h in history]
    N = len(history[0])
    if blocks is None:
        blocks = (N + KAPPLY_ROWS - 1) // KAPPLY_ROWS
    out = [dict() for _ in history]
    for f, kind in float_features(shareds):
        tr = [truth([cols[f]], [shareds[f]], h)[0] for h in history]
        if kind == NICH:
            x = _x64(cols[f])
            if start == "load":
                b0 = fx.nich_welford_bounds(
                    np.asarray(cols[f]).view(np.float32), history[:1])
                st = {g: (b[1], b[2]) for g, b in b0.items()}
            else:
                st = {}
                for g, (n, mu, C) in tr[0].items():
                    xs = x[history[0] == g]
                    S, Q = abs(math.fsum(xs)), math.fsum(xs * xs)
                    st[g] = nich_merge_step(0, 0.0, 0.0, 0.0, 0.0, n, mu, C,
                                            V * S, V * Q)
            out[0][f] = {g: (tr[0][g][0],) + st[g] for g in tr[0]}
            for t in range(1, len(history)):
                old, new = history[t - 1], history[t]
                moved = np.nonzero(old != new)[0]
                ax = np.abs(x[moved])
                touched = {}
                for side in (old, new):
                    for g, a in zip(side[moved].tolist(), ax.tolist()):
                        L, s, ss = touched.get(g, (0, 0.0, 0.0))
                        touched[g] = (L + 1, s + a, ss + a * a)
                nxt = {}
                for g, (n1, mu1, C1) in tr[t].items():
                    if g not in touched:
                        nxt[g] = st[g]
                        continue
                    L, s, ss = touched[g]
                    n0, mu0, C0 = tr[t - 1].get(g, (0, 0.0, 0.0))
                    em0, ec0 = st.get(g, (0.0, 0.0))
                    gg = _g(L + blocks)
                    nxt[g] = nich_merge_step(n0, mu0, C0, em0, ec0, n1, mu1,
                                             C1, gg * s * SLACK,
                                             gg * ss * SLACK)
                st = nxt
                out[t][f] = {g: (tr[t][g][0],) + st[g] for g in tr[t]}
        else:
            true, lf32 = _log_fact(cols[f])
            err = np.abs(lf32 - true)
            if start == "load":
                b0 = fm.gp_log_prod_bounds(cols[f], history[:1])
                st = {g: b[1] for g, b in b0.items()}
            else:
                st = {g: (U + 2.0 * V) * abs(lp) * SLACK
                      for g, (n, lp) in tr[0].items()}
            out[0][f] = {g: (tr[0][g][0], st[g]) for g in tr[0]}
            for t in range(1, len(history)):
                old, new = history[t - 1], history[t]
                moved = np.nonzero(old != new)[0]
                touched = {}
                for sign, side in ((-1.0, old), (1.0, new)):
                    for g, a, e in zip(side[moved].tolist(),
                                       lf32[moved].tolist(),
                                       err[moved].tolist()):
                        L, s, m = touched.get(g, (0, 0.0, 0.0))
                        touched[g] = (L + 1, s + abs(a),
                                      m + (sign * e if start == "load" else e))
                nxt = {}
                for g, (n1, lp1) in tr[t].items():
                    if g not in touched:
                        nxt[g] = st[g]
                        continue
                    L, s, m = touched[g]
                    e0 = st.get(g, 0.0)
                    e_d = e0 + _g(L + blocks) * s + m
                    nxt[g] = max(e_d + (U + V) * (abs(lp1) + e_d), 0.0) * SLACK
                st = nxt
                out[t][f] = {g: (tr[t][g][0], st[g]) for g in tr[t]}
    return out


# ---------------------------------------------------------------------------
# the kernels restated


def _f32(x):
    return float(np.float32(x))


class Restated(object):
    """k_merge_float_moves / _reduce / _apply / _export in numpy: binary64
    sums, binary32 state per global id.  NOT the reference."""

    def __init__(self, cols, shareds, mut=()):
        self.mut = tuple(mut)
        self.feats = float_features(shareds)
        self.x32 = {}
        self.lf = {}
        for f, kind in self.feats:
            if kind == NICH:
                self.x32[f] = np.asarray(cols[f]).view(np.float32) \
                    if np.asarray(cols[f]).dtype != np.float32 \
                    else np.asarray(cols[f], np.float32)
            else:
                self.lf[f] = _log_fact(cols[f])[1]
        self.st = {f: {} for f, _ in self.feats}
        # what an emptied group's slot still holds when the next new group
        # takes it (zeros, unless stale_on_empty)
        self.left_in_slot = {f: (0.0, 0.0) for f, _ in self.feats}

    # -- the load's additions, in row order, in binary32 --------------------
    def load(self, assign):
        f32 = np.float32
        for f, kind in self.feats:
            st = {}
            if kind == NICH:
                for g, x in zip(np.asarray(assign).tolist(), self.x32[f]):
                    n, m, c = st.get(g, (0, f32(0), f32(0)))
                    n += 1
                    delta = f32(x - m)
                    m = f32(m + f32(delta / f32(n)))
                    c = f32(c + f32(delta * f32(x - m)))
                    st[g] = (n, m, c)
                st = {g: (n, float(m), float(c)) for g, (n, m, c) in
                      st.items()}
            else:
                for g, a in zip(np.asarray(assign).tolist(),
                                self.lf[f].astype(f32)):
                    n, lp = st.get(g, (0, f32(0)))
                    st[g] = (n + 1, f32(lp + a))
                st = {g: (n, float(lp)) for g, (n, lp) in st.items()}
            self.st[f] = st

    # -- k_merge_float_apply ------------------------------------------------
    def _apply_nich(self, old, dn, dx, dxx, reset):
        mut = self.mut
        if not reset and dn == 0.0 and dx == 0.0 and dxx == 0.0:
            return old
        if not reset and dn == 0.0 and "skip_n_unchanged" in mut:
            return old
        n0, mean0, ctv0 = (0.0, 0.0, 0.0) if reset else (
            float(old[0]), old[1], old[2])
        n1 = n0 + dn
        s1 = n0 * mean0 + dx
        s2 = ctv0 + dxx if "no_recentre" in mut else (
            ctv0 + n0 * mean0 * mean0 + dxx)
        mean1, ctv1 = 0.0, 0.0
        if n1 >= 1.0:
            mean1 = s1 / n1
        if n1 >= (1.0 if "var_at_one" in mut else 2.0):
            ctv1 = s2 - n1 * mean1 * mean1
            if ctv1 < 0.0:
                ctv1 = 0.0
        if n1 < 1.0 and "stale_on_empty" in mut and not reset:
            mean1, ctv1 = mean0, ctv0
        return (int(n1), _f32(mean1), _f32(ctv1))

    def import_image(self, image):
        """reset = 1: the old statistics taken as zero"""
        for f, kind in self.feats:
            if kind == NICH:
                self.st[f] = {g: self._apply_nich(None, n, S, Q, True)
                              for g, (n, S, Q) in image[f].items()}
            else:
                # (the count is an integer statistic, not the image's)
                self.st[f] = {g: (self.st[f].get(g, (0,))[0], _f32(0.0 + lp))
                              for g, (lp,) in image[f].items()}

    def set_counts(self, assign):
        """GammaPoisson's count is an integer statistic: from the rows"""
        ids, cnt = np.unique(np.asarray(assign, np.int64), return_counts=True)
        for f, kind in self.feats:
            if kind == GP:
                self.st[f] = {int(g): (int(c), self.st[f].get(int(g),
                                                              (0, 0.0))[1])
                              for g, c in zip(ids, cnt)}

    def export_image(self):
        """k_merge_float_export"""
        out = {}
        for f, kind in self.feats:
            if kind == NICH:
                out[f] = {g: (float(n), float(n) * m, c + float(n) * m * m)
                          for g, (n, m, c) in self.st[f].items()}
            else:
                out[f] = {g: (lp,) for g, (n, lp) in self.st[f].items()}
        return out

    def batch(self, old, new, rng=None):
        """one sub-sweep's moves: old, new the assignments before and after.
        rng: the order in which the binary64 sums are taken (a permutation of
        the moved rows is drawn; default row order)"""
        old = np.asarray(old, np.int64)
        new = np.asarray(new, np.int64)
        moved = np.nonzero(old != new)[0]
        if rng is not None:
            moved = rng.permutation(moved)
        mut = self.mut
        for f, kind in self.feats:
            # (a group emptied by the batch before has left the group set;
            # its id is never reused by the engine, and what its slot holds
            # is what the next new group starts from)
            st = {}
            for g, s in self.st[f].items():
                if s[0] > 0:
                    st[g] = s
                elif kind == NICH:
                    self.left_in_slot[f] = s[1:]
            delta = {}
            if kind == NICH:
                x32 = self.x32[f][moved]
                x = x32.astype(np.float64)
                xx = (x32 * x32).astype(np.float64) if "sq_f32" in mut \
                    else x * x
                for go, gn, a, aa in zip(old[moved].tolist(),
                                         new[moved].tolist(), x.tolist(),
                                         xx.tolist()):
                    d = delta.setdefault(go, [0.0, 0.0, 0.0])
                    d[0] -= 1.0
                    d[1] -= a
                    d[2] -= aa
                    d = delta.setdefault(gn, [0.0, 0.0, 0.0])
                    d[0] += 1.0
                    d[1] += a
                    d[2] += aa
                for g, (dn, dx, dxx) in delta.items():
                    fresh = (0,) + self.left_in_slot[f]
                    st[g] = self._apply_nich(st.get(g, fresh), dn, dx, dxx,
                                             False)
            else:
                lf = self.lf[f][moved]
                for go, gn, a in zip(old[moved].tolist(), new[moved].tolist(),
                                     lf.tolist()):
                    d = delta.setdefault(go, [0.0, 0.0])
                    d[0] -= 1.0
                    d[1] += a if "gp_sign" in mut else -a
                    d = delta.setdefault(gn, [0.0, 0.0])
                    d[0] += 1.0
                    d[1] += a
                for g, (dn, d) in delta.items():
                    n, lp = st.get(g, (0, 0.0))
                    if d != 0.0:
                        lp = _f32(lp + d)
                    st[g] = (n + int(dn), lp)
            self.st[f] = st     # (emptied groups stay visible for one step)


def merged_restated(cols, shareds, history, start, mut=(), rng=None):
    """-> a list, one entry per entry of history, of
    {feature: {global id: (n, mean32, ctv32)} or {global id: (n, lp32)}}"""
    r = Restated(cols, shareds, mut)
    r.load(history[0])
    if start == "import":
        r.import_image(image_of(cols, shareds, history[0]))
    out = [{f: dict(s) for f, s in r.st.items()}]
    for old, new in zip(history[:-1], history[1:]):
        r.batch(old, new, rng)
        out.append({f: dict(s) for f, s in r.st.items()})
    return out


# ---------------------------------------------------------------------------
# comparing


def ordered_bounds(cols, shareds, history):
    """the ordered paths' bounds, the history per SWEEP
    -> {feature: {global id: (n, em, ec)} or {global id: (n, elp)}}"""
    out = {}
    for f, kind in float_features(shareds):
        if kind == NICH:
            out[f] = fx.nich_welford_bounds(
                np.asarray(cols[f]).view(np.float32), history)
        else:
            out[f] = fm.gp_log_prod_bounds(cols[f], history)
    return out


def _ratio(d, band):
    return 0.0 if d == 0.0 else d / max(band, 1e-300)


def excursions(got, want, bounds, shareds):
    """got: {feature: {id: (n, mean, ctv) | (n, log_prod)}} as read from the
    code under test; want: truth(); bounds: the matching entry of
    merged_bounds or ordered_bounds.
    -> (counts equal, {"mean" | "ctv" | "log_prod": worst |got - want| /
    band over the non-empty groups}); every statistic must be finite.  An
    EMPTY group's NICH mean and ctv must be exactly zero (nich.hpp:159-163;
    its ctv enters the score of joining it): "empty" is inf otherwise.
    (GammaPoisson's log_prod of an empty group may keep the roundings of its
    removals, gp.hpp:134, and nothing reads it.)"""
    worst = {}
    counts_ok = True
    for f, kind in float_features(shareds):
        live = {g: s for g, s in got[f].items() if s[0] > 0}
        if kind == NICH:
            for g, s in got[f].items():
                if s[0] == 0 and (s[1] != 0.0 or s[2] != 0.0):
                    worst["empty"] = float("inf")
        if set(live) != set(want[f]):
            counts_ok = False
        for g, w in want[f].items():
            s = live.get(g)
            if s is None:
                continue
            b = bounds[f][g]
            if s[0] != w[0] or b[0] != w[0]:
                counts_ok = False
            names = ("mean", "ctv") if kind == NICH else ("log_prod",)
            for j, name in enumerate(names):
                if not math.isfinite(s[1 + j]):
                    worst[name] = float("inf")
                    continue
                r = _ratio(abs(s[1 + j] - w[1 + j]), b[1 + j])
                worst[name] = max(worst.get(name, 0.0), r)
    return counts_ok, worst


def reimport_bounds(cols, shareds, assign, parts, part_bounds):
    """the band after import_float_moments_dev of the SUM of exported images:
    parts: one row-index array per exporting replica; part_bounds: per part
    the bounds its statistics had ({feature: {id: (n, em, ec) | (n, elp)}},
    against the truth of ITS rows).  The image's sums are then within the
    sum of export_bounds (plus one binary64 rounding per addition) of the
    rows' sums, and the import is one nich_merge_step from zero.
    -> as one entry of merged_bounds"""
    assign = np.asarray(assign, np.int64)
    whole = truth(cols, shareds, assign)
    out = {}
    for f, kind in float_features(shareds):
        acc = {}
        for rows, pb in zip(parts, part_bounds):
            sub = truth([np.asarray(cols[f])[rows]], [shareds[f]],
                        assign[rows])[0]
            for g, s in sub.items():
                b = pb[f][g]
                assert b[0] == s[0]
                if kind == NICH:
                    es, eq = export_bounds(s[0], s[1], b[1], b[2])
                    S = abs(s[0] * s[1]) + es
                    Q = s[2] + s[0] * s[1] * s[1] + eq
                    a = acc.get(g, (0.0, 0.0, 0.0, 0.0))
                    acc[g] = (a[0] + es, a[1] + eq, a[2] + S, a[3] + Q)
                else:
                    a = acc.get(g, (0.0, 0.0))
                    acc[g] = (a[0] + b[1], a[1] + abs(s[1]) + b[1])
        res = {}
        for g, w in whole[f].items():
            a = acc[g]
            if kind == NICH:
                k = len(parts) * V
                res[g] = (w[0],) + nich_merge_step(
                    0, 0.0, 0.0, 0.0, 0.0, w[0], w[1], w[2],
                    a[0] + k * a[2], a[1] + k * a[3])
            else:
                e = a[0] + len(parts) * V * a[1]
                res[g] = (w[0], (e + (U + V) * (abs(w[1]) + e)) * SLACK)
        out[f] = res
    return out
