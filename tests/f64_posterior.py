"""The posterior over set partitions in float64, and the exact law of the
sequential chain on that space.

TEST INFRASTRUCTURE (imported by tests only).

At n = 6 rows there are 203 set partitions (877 at n = 7), so everything the
exact chain is for can be written down completely:

  log_posterior        the closed form: log EPPF of PitmanYor(alpha, d)
                       (clustering.cc:144-183 is the same product) plus, per
                       block and feature, the log marginal likelihood as the
                       chain-rule sum of `f64_scores.float64_score`
  row_matrix           one row step as a 203 x 203 stochastic matrix: the row
                       is taken out (alone in its group, the group vanishes:
                       mixture.hpp:94-122), every remaining group and each of
                       the `empty` empty groups is scored -- the clustering
                       terms are `f64_scores.py_terms` / `le_terms`
                       (clustering.hpp:195-230, 267-292), the feature terms
                       `float64_score` of the group's members -- and the row
                       joins a slot with probability proportional to
                       exp(score) (mixture.hpp:73-92)
  sweep_matrix         rows 0 .. n-1 in order
  law_after            e_start @ P**T: what a histogram of chain states after
                       T sweeps is tested against; no burn-in argument
  stationarity_gap     max |pi P - pi|
  mixing_distance      max_s TV(P**T[s], pi)
  pooled_chi_square    Pearson's chi-square with the small cells pooled

Nothing here reads the oracle or the library; the two runners at the end
(`oracle_histogram`, and the helpers the GPU test shares) only drive them.

BNB: `float64_score` is the reference's Scorer, the beta-negative-binomial
pmf without C(x + r - 1, x).  That factor depends on the row alone, so it is
the same for every partition and cancels from the posterior; it is not added.

LowEntropy (clustering.hpp:245-331).  Finding, checked in float64 by
`test_low_entropy_stationary_law`: score_add_value IS an exact difference of
score_counts (clustering.cc:221-248) as far as the chain can tell.  For a
group of n <= 10000 rows, n log((n + 1) / n) + log(n + 1) = (n + 1) log(n + 1)
- n log n exactly (the "very_large" approximation starts above 10000).  A new
group scores the postpred correction at the sample size the row joins; every
row step scores at sample size N, so that is one constant c per new group,
and score_counts has the same c * (groups - 1), its remaining terms depending
on N alone.  So exp(score_counts) times the marginals is the stationary law
(gap below 1e-12, with and without dataset_size == N) and both it and
e_start @ P**T are used.
"""
import itertools
import math

import numpy as np
from scipy import stats

import f64_scores as fs

DD, BB, GP, NICH, DPD, BNB = fs.DD, fs.BB, fs.GP, fs.NICH, fs.DPD, fs.BNB

# the mutated REFERENCES of the power tests (the library is never mutated)
MUTANTS = (
    "ne_plus_one",      # the discount multiplied by K + 1 instead of K
    "log_n",            # the discount missing from the within-group factor
    "alpha_undivided",  # the new-group mass not shared between empty groups
    "own_kept",         # the row's own group not decremented before scoring
    "last_never",       # the last slot never drawn.  Slot order is not part
                        # of a partition: the mutant drops the last EMPTY slot
                        # (the fresh group every add appends is the last one),
                        # i.e. 2/3 of the new-group mass with 3 empty groups
)


def set_partitions(n):
    """restricted-growth strings of length n, in lexicographic order"""
    out = []

    def grow(prefix, top):
        if len(prefix) == n:
            out.append(tuple(prefix))
            return
        for b in range(top + 2):
            grow(prefix + [b], max(top, b))
    if n:
        grow([0], 0)
    return out


def canonical(assign):
    """the partition of a chain state: ids relabelled in order of first
    appearance"""
    seen = {}
    return tuple(seen.setdefault(int(a), len(seen)) for a in assign)


class Space(object):
    """the partitions of n rows and a vectorised index of chain states"""

    def __init__(self, n):
        self.n = n
        self.parts = set_partitions(n)
        self.index = {p: i for i, p in enumerate(self.parts)}
        self.pairs = list(itertools.combinations(range(n), 2))
        self._by_code = {}
        for i, p in enumerate(self.parts):
            self._by_code[self._code(np.array([p]))[0]] = i

    def _code(self, assign):
        a = np.asarray(assign, np.int64)
        code = np.zeros(len(a), np.int64)
        for bit, (i, j) in enumerate(self.pairs):
            code |= (a[:, i] == a[:, j]).astype(np.int64) << bit
        return code

    def indices(self, assign):
        """[M, n] group ids (any labels) -> [M] partition indices"""
        code = self._code(assign)
        return np.array([self._by_code[c] for c in code.tolist()], np.int64)

    def histogram(self, assign):
        return np.bincount(self.indices(assign), minlength=len(self.parts))


class Model(object):
    """rows, features and clustering prior of one configuration.

    shareds: the oracle's Shared structs (hyper-parameters as the binary32
    values the models hold, taken as exact); cols: one value list per feature
    (NICH: float32 values); prior: ("py", alpha, d) or ("le", dataset_size);
    empty: how many empty groups the mixture keeps."""

    def __init__(self, shareds, cols, prior, empty):
        self.feats = [fs.Feature(s) for s in shareds]
        self.cols = []
        for f, c in zip(self.feats, cols):
            if f.kind == NICH:
                self.cols.append([float(np.float32(x)) for x in c])
            else:
                self.cols.append([int(x) for x in c])
        self.n = len(self.cols[0])
        if prior[0] == "py":
            prior = ("py", float(np.float32(prior[1])),
                     float(np.float32(prior[2])))
        self.prior = prior
        self.empty = int(empty)
        self.space = Space(self.n)
        self._pred = {}

    def pred(self, members, row):
        """sum over the features of the log predictive of `row`'s values
        given the rows in `members` (a sorted tuple)"""
        key = (members, row)
        if key not in self._pred:
            self._pred[key] = sum(
                float(fs.float64_score(f.kind, f.kw(),
                                       [c[j] for j in members], c[row]))
                for f, c in zip(self.feats, self.cols))
        return self._pred[key]

    # -- the closed form ----------------------------------------------------
    def log_prior(self, sizes):
        N = sum(sizes)
        if self.prior[0] == "py":
            # Pitman's EPPF: prod_{j<k} (alpha + j d) / prod_{m<N} (alpha + m)
            # times prod_b prod_{m<n_b} (m - d)
            _, alpha, d = self.prior
            s = sum(math.log(alpha + j * d) for j in range(1, len(sizes)))
            s -= sum(math.log(alpha + m) for m in range(1, N))
            for nb in sizes:
                s += sum(math.log(m - d) for m in range(1, nb))
            return s
        # LowEntropy::score_counts (clustering.cc:221-248) up to terms that
        # depend on N alone
        D = float(self.prior[1])
        s = sum(nb * math.log(nb) for nb in sizes)
        if N != D:
            corr = math.log(D / N) * (0.45 - 0.1 / N - 0.1 / D)
            s += corr * (len(sizes) - 1)
        return s

    def log_posterior(self):
        """unnormalised log posterior of every partition"""
        out = np.zeros(len(self.space.parts))
        for i, p in enumerate(self.space.parts):
            blocks = _blocks(p)
            s = self.log_prior([len(b) for b in blocks])
            for b in blocks:
                for j, row in enumerate(b):
                    s += self.pred(b[:j], row)
            out[i] = s
        return out

    def posterior(self):
        lp = self.log_posterior()
        w = np.exp(lp - lp.max())
        return w / w.sum()

    # -- the chain ----------------------------------------------------------
    def step_law(self, part, row, mut=()):
        """one row step from partition `part`: [(partition, probability)]"""
        blocks = _blocks(part)
        own = [b for b in blocks if row in b][0]
        rest = [b for b in blocks if b is not own]
        left = tuple(r for r in own if r != row)
        slots = rest + ([left] if left else [])   # the groups the row sees
        scored = list(slots)
        if left and "own_kept" in mut:
            scored[-1] = own              # scored with the row still in it
        m = len(slots)
        E = self.empty
        sizes = np.array([len(b) for b in scored] + [0] * E, np.float64)
        N = self.n - 1                    # the sample size the row joins
        if self.prior[0] == "py":
            _, alpha, d = self.prior
            ne = m + (1 if "ne_plus_one" in mut else 0)
            score = fs.py_terms(sizes, np.full(m + E, float(ne)), E, N,
                                alpha, d, mut).v.copy()
        else:
            score = fs.le_terms(sizes, N, E, self.prior[1], mut).v.copy()
        for k, b in enumerate(scored):
            score[k] += self.pred(b, row)
        score[m:] += self.pred((), row)
        w = np.exp(score - score.max())
        if "last_never" in mut:
            w[-1] = 0.0
        w /= w.sum()
        out = []
        for k in range(m):
            joined = tuple(sorted(set(slots[k]) | {row}))
            others = [b for j, b in enumerate(slots) if j != k]
            out.append((_partition(others + [joined], self.n), w[k]))
        out.append((_partition(slots + [(row,)], self.n), w[m:].sum()))
        return out

    def row_matrix(self, row, mut=()):
        S = len(self.space.parts)
        P = np.zeros((S, S))
        for i, p in enumerate(self.space.parts):
            for q, w in self.step_law(p, row, mut):
                P[i, self.space.index[q]] += w
        return P

    def sweep_matrix(self, mut=()):
        P = np.eye(len(self.space.parts))
        for row in range(self.n):
            P = P @ self.row_matrix(row, mut)
        return P


def _blocks(part):
    """blocks of a restricted-growth string, as sorted tuples of rows"""
    out = [[] for _ in range(max(part) + 1)]
    for row, b in enumerate(part):
        out[b].append(row)
    return [tuple(b) for b in out]


def _partition(blocks, n):
    a = [0] * n
    for k, b in enumerate(blocks):
        for r in b:
            a[r] = k
    return canonical(a)


def start_state(space, start):
    """"one": all rows in one group; "alone": every row alone"""
    p = (0,) * space.n if start == "one" else tuple(range(space.n))
    e = np.zeros(len(space.parts))
    e[space.index[p]] = 1.0
    return e


def law_after(P, e_start, T):
    return e_start @ np.linalg.matrix_power(P, T)


def law_sum(P, e_start, T, samples):
    """sum_{j=1..samples} e_start @ P**(jT): expected share of each partition
    among the states of one chain taken every T sweeps (sums to `samples`)"""
    PT = np.linalg.matrix_power(P, T)
    v = e_start.copy()
    total = np.zeros_like(v)
    for _ in range(samples):
        v = v @ PT
        total += v
    return total


def stationarity_gap(P, pi):
    return float(np.abs(pi @ P - pi).max())


def mixing_distance(P, pi, T):
    PT = np.linalg.matrix_power(P, T)
    return float(0.5 * np.abs(PT - pi[None, :]).sum(1).max())


def mixing_time(P, pi, bound=1e-4, limit=4096):
    """the smallest T with max_s TV(P**T[s], pi) < bound"""
    PT = np.eye(len(pi))
    for T in range(1, limit + 1):
        PT = PT @ P
        if 0.5 * np.abs(PT - pi[None, :]).sum(1).max() < bound:
            return T
    raise AssertionError("the chain does not mix within %d sweeps" % limit)


def pooling(expected, floor=5.0):
    """-> (pooled [cells] bool, pooled share of the expected mass): cells with
    expectation below `floor` go, smallest first, into one cell; while that
    cell itself is below `floor` the next smallest joins it"""
    e = np.asarray(expected, np.float64)
    order = np.argsort(e, kind="stable")
    pooled = np.zeros(len(e), bool)
    acc = 0.0
    for i in order:
        if e[i] >= floor and (acc >= floor or acc == 0.0):
            break
        pooled[i] = True
        acc += e[i]
    return pooled, float(acc / e.sum())


def pooled_chi_square(hist, expected, floor=5.0):
    """Pearson's chi-square of a histogram against expected counts, small
    cells pooled (`pooling`) -> (chi2, degrees of freedom, p)"""
    h = np.asarray(hist, np.float64)
    e = np.asarray(expected, np.float64)
    assert abs(h.sum() - e.sum()) <= 1e-6 * e.sum()
    pooled, _ = pooling(e, floor)
    hh = np.r_[h[~pooled], h[pooled].sum()] if pooled.any() else h
    ee = np.r_[e[~pooled], e[pooled].sum()] if pooled.any() else e
    keep = ee > 0
    # a count in a cell of expectation zero is an outright rejection
    if hh[~keep].sum() > 0:
        return float("inf"), int(keep.sum()) - 1, 0.0
    chi2 = float((((hh - ee) ** 2)[keep] / ee[keep]).sum())
    dof = int(keep.sum()) - 1
    return chi2, dof, float(stats.chi2.sf(chi2, dof))


def report(name, expected, hist):
    """one line per test: partitions, cells after pooling, pooled mass, chi2,
    degrees of freedom, p"""
    pooled, mass = pooling(expected)
    chi2, dof, p = pooled_chi_square(hist, expected)
    cells = int((~pooled).sum()) + (1 if pooled.any() else 0)
    print("%-34s partitions %3d cells %3d pooled mass %.4f min expected %8.2f"
          " chi2 %9.1f dof %3d p %.3g" % (name, len(expected), cells, mass,
                                          float(np.min(expected)), chi2, dof,
                                          p))
    return chi2, dof, p, mass


# ---------------------------------------------------------------------------
# the configurations (rows and hyper-parameters chosen so that the float64
# law alone keeps the pooled mass under 5 %: checked by the tests)

ROWS = {
    "dd":  [[0, 1, 2, 0, 1, 0]],
    "bb":  [[1, 0, 1, 1, 0, 0]],
    "dpd": [[0, 1, 2, 0, 3, 1]],
    "bnb": [[0, 3, 1, 7, 2, 4]],
    "gp_nich": [[2, 7, 3, 6, 1, 8],
                [-0.75, 1.25, -0.5, 0.875, 0.25, 1.5]],
    "dd_bb_gp": [[0, 1, 2, 0, 1, 2], [1, 0, 1, 0, 0, 1], [2, 5, 3, 4, 1, 6]],
    "dd7": [[0, 1, 2, 0, 1, 0, 2]],
}


def shared_kw(config):
    """-> [(kind, hyper-parameters)] of a configuration's features"""
    dd = (DD, dict(alphas=[0.5, 1.0, 2.0]))
    bb = (BB, dict(alpha=0.75, beta=1.5))
    gp = (GP, dict(alpha=2.0, inv_beta=0.5))
    return {
        "dd": [dd],
        "dd7": [dd],
        "bb": [bb],
        "dpd": [(DPD, dict(alpha=1.5, betas=[0.3, 0.25, 0.2, 0.15],
                           beta0=0.1))],
        "bnb": [(BNB, dict(alpha=2.5, beta=1.5, r=2))],
        "gp_nich": [gp, (NICH, dict(mu=0.25, kappa=0.5, sigmasq=1.5,
                                    nu=2.0))],
        "dd_bb_gp": [dd, bb, gp],
    }[config]


PY = ("py", 1.2, 0.3)
# (configuration, clustering prior, empty groups)
CASES = [(c, PY, e) for c in ("dd", "bb", "dpd", "bnb", "gp_nich", "dd_bb_gp")
         for e in (1, 3)]
CASES += [("dd", ("le", 6), 2), ("gp_nich", ("le", 10), 2), ("dd7", PY, 2)]


# states taken from ONE engine by the single-engine legs of
# test_gpu_posterior.py; test_f64_posterior.py holds the mutants to this count
LEG_SAMPLES = 20000


def case_id(case):
    config, prior, empty = case
    tag = ("py" if prior[0] == "py" else "le%d" % prior[1])
    return "%s-%s-e%d" % (config, tag, empty)


_MODELS = {}


def model(case):
    """the float64 model of a case (cached: the matrices are reused)"""
    import oracle_lib as ol
    if case not in _MODELS:
        config, prior, empty = case
        shareds = [ol.make_shared(k, **kw) for k, kw in shared_kw(config)]
        _MODELS[case] = Model(shareds, ROWS[config], prior, empty)
    return _MODELS[case]


def start_assign(n, start):
    """-> (packed assignments, non-empty groups) of a start state"""
    if start == "one":
        return np.zeros(n, np.uint32), 1
    return np.arange(n, dtype=np.uint32), n


# ---------------------------------------------------------------------------
# runner: M independent oracle chains


def oracle_mixture(case):
    import ctypes
    import oracle_lib as ol
    config, prior, empty = case
    shareds = [ol.make_shared(k, **kw) for k, kw in shared_kw(config)]
    if prior[0] == "py":
        orc = ol.OracleMixture(prior[1], prior[2], shareds)
    else:
        orc = ol.OracleMixture(1.0, 0.0, shareds)
        orc.L.orc_mix_set_low_entropy.restype = None
        orc.L.orc_mix_set_low_entropy.argtypes = [ctypes.c_void_p,
                                                  ctypes.c_int]
        orc.L.orc_mix_set_low_entropy(orc.h, prior[1])
    vals = [np.asarray(c, np.float32 if k == NICH else np.uint32)
            for (k, _), c in zip(shared_kw(config), ROWS[config])]
    return orc, vals


def oracle_histogram(case, start, chains, sweeps, base):
    """`chains` independent OracleMixture.gibbs_sequential chains of `sweeps`
    sweeps from `start`, chain c seeded orc_rng_seed(base + c) -> histogram
    over the partitions"""
    import ctypes
    orc, vals = oracle_mixture(case)
    n = len(vals[0])
    assign0, nonempty = start_assign(n, start)
    empty = case[2]
    orc.init_from_assignments(vals, assign0, nonempty, empty)
    L, h, ptrs = orc.L, orc.h, orc._vals
    seed, init, gibbs = (L.orc_rng_seed, L.orc_mix_init_from_assignments,
                         L.orc_mix_gibbs_sequential)
    out = np.zeros((chains, n), np.uint32)
    st = ctypes.c_uint32(0)
    ref = ctypes.byref(st)
    for c in range(chains):
        a = out[c]
        init(h, n, ptrs, assign0, nonempty, empty, a)
        st.value = seed(base + c)
        for _ in range(sweeps):
            gibbs(h, 0, n, ptrs, a, ref)
    return model(case).space.histogram(out)
