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
  row_options          the same row step as a law over slots that keep their
                       identity for every row of a batch: a block of the
                       partition, or one of the empty groups
  batch_matrix         a batch of several rows: every row
                       draws from `row_options` of the state at batch entry,
                       independently; then all moves are applied
  batch_sweep_matrix   the tiles [0, B), [B, 2B), ... of the rows in order
  stationary           a matrix's stationary vector (power iteration): used
                       for the thinning T of the batch chain alone, whose law
                       is not the posterior
  mutant_power         how visible a planted bug is to the float64 law alone
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


# planted bugs of the BATCH law (`Model.batch_matrix`)
BATCH_MUTANTS = (
    "sequential",       # rows of a batch see the moves of the rows before
                        # them: the batch is `sweep_matrix`'s product
    "empties_merged",   # every empty slot is the same new group
    "empties_apart",    # two rows that pick the same empty slot found two
                        # groups
    "lone_keeps_own",   # a row alone in its group is offered that group (as
                        # one more empty slot) in addition to the empty ones
    "own_kept",         # as in MUTANTS
    "alpha_undivided",  # as in MUTANTS
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
        self._lut = None
        for i, p in enumerate(self.parts):
            self._by_code[self._code(np.array([p]))[0]] = i

    def _code(self, assign):
        a = np.asarray(assign, np.int64)
        code = np.zeros(len(a), np.int64)
        for bit, (i, j) in enumerate(self.pairs):
            code |= (a[:, i] == a[:, j]).astype(np.int64) << bit
        return code

    def lookup(self):
        """pair code -> partition index as an array (-1: no partition)"""
        if self._lut is None:
            self._lut = np.full(1 << len(self.pairs), -1, np.int64)
            for c, i in self._by_code.items():
                self._lut[c] = i
        return self._lut

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
    def row_options(self, part, row, mut=()):
        """the row step from partition `part` as a law over SLOTS that keep
        their identity for every row of a batch -> (labels, probabilities).
        A label below K = the number of blocks of `part` is that block (the
        row's own block only while it has other members, and scored without
        the row: a row alone has seen its group vanish); K + j is empty slot
        j, each with its own weight."""
        blocks = _blocks(part)
        K = len(blocks)
        own_k = part[row]
        own = blocks[own_k]
        rest = [b for b in blocks if b is not own]
        left = tuple(r for r in own if r != row)
        slots = rest + ([left] if left else [])   # the groups the row sees
        labels = [k for k in range(K) if k != own_k] + ([own_k] if left
                                                        else [])
        scored = list(slots)
        if left and "own_kept" in mut:
            scored[-1] = own              # scored with the row still in it
        m = len(slots)
        E = self.empty
        lone = (not left) and "lone_keeps_own" in mut
        if lone:
            E += 1                        # the vanished group, still a slot
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
        labels += ([own_k] if lone else []) + [K + j for j in
                                               range(self.empty)]
        return labels, w

    def step_law(self, part, row, mut=()):
        """one row step from partition `part`: [(partition, probability)]"""
        labels, w = self.row_options(part, row, mut)
        K = max(part) + 1
        m = sum(1 for k in labels if k < K)
        out = []
        for k, wk in zip(labels[:m], w[:m]):
            q = list(part)
            q[row] = k
            out.append((canonical(q), wk))
        q = list(part)
        q[row] = K
        out.append((canonical(q), w[m:].sum()))
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


    # -- batches of several rows --------------------------
    def batch_matrix(self, rows, mut=()):
        """one batch as a stochastic matrix: every row of `rows` draws,
        independently, from `row_options` of the partition at batch entry;
        then all moves are applied -- rows outside the batch stay, rows with
        the same label end up together, different empty slots are different
        new groups.  The outcomes of one state are a grid (one axis per row
        of the batch); their partitions are found through the pair code of
        `Space`."""
        rows = [int(r) for r in rows]
        assert len(set(rows)) == len(rows)
        if "sequential" in mut:           # the rows see each other's moves
            rest = tuple(x for x in mut if x != "sequential")
            P = np.eye(len(self.space.parts))
            for r in rows:
                P = P @ self.row_matrix(r, rest)
            return P
        space = self.space
        S = len(space.parts)
        lut = space.lookup()
        bit = {}
        for k, (i, j) in enumerate(space.pairs):
            bit[(i, j)] = bit[(j, i)] = np.int64(1) << k
        fixed = [j for j in range(self.n) if j not in rows]
        b = len(rows)
        P = np.zeros((S, S))
        for i, part in enumerate(space.parts):
            K = max(part) + 1
            code = np.zeros((1,) * b, np.int64)
            for x, y in itertools.combinations(fixed, 2):
                if part[x] == part[y]:
                    code = code + bit[(x, y)]
            wgt = np.ones((1,) * b)
            place = []
            for t, r in enumerate(rows):
                labels, w = self.row_options(part, r, mut)
                lab = np.array(labels, np.int64)
                if "empties_merged" in mut:
                    lab = np.minimum(lab, K)
                if "empties_apart" in mut:
                    lab = np.where(lab >= K, K + self.empty + t, lab)
                shape = [1] * b
                shape[t] = len(lab)
                c = np.zeros(len(lab), np.int64)
                for j in fixed:
                    c += (lab == part[j]) * bit[(r, j)]
                place.append(lab.reshape(shape))
                code = code + c.reshape(shape)
                wgt = wgt * w.reshape(shape)
            for t in range(b):
                for u in range(t + 1, b):
                    code = code + (place[t] == place[u]) * bit[(rows[t],
                                                                rows[u])]
            idx = lut[code.ravel()]
            assert idx.min() >= 0
            P[i] = np.bincount(idx, weights=wgt.ravel(), minlength=S)
        return P

    def batch_tiles(self, B):
        """the batches of one sweep: [0, B), [B, 2B), ..., the last ragged"""
        return [list(range(b, min(self.n, b + B)))
                for b in range(0, self.n, B)]

    def batch_sweep_matrix(self, B, mut=()):
        P = np.eye(len(self.space.parts))
        for tile in self.batch_tiles(B):
            P = P @ self.batch_matrix(tile, mut)
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


def stationary(P, tol=1e-15, limit=100000):
    """the stationary vector of a stochastic matrix by power iteration"""
    v = np.full(len(P), 1.0 / len(P))
    for _ in range(limit):
        nv = v @ P
        nv /= nv.sum()
        if np.abs(nv - v).max() < tol:
            return nv
        v = nv
    raise AssertionError("no stationary vector within %d steps" % limit)


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


# -- batches of several rows -------------------------------------------------
# (case, batch_rows): the sweep is the tiles [0, B), [B, 2B), ... of the rows
BATCH_LEGS = [
    (("dd", PY, 1), 6), (("dd", PY, 3), 3), (("dd", PY, 3), 6),
    (("bb", PY, 3), 4), (("dpd", PY, 1), 6), (("bnb", PY, 3), 3),
    (("gp_nich", PY, 3), 3), (("gp_nich", PY, 1), 6),
    (("dd_bb_gp", PY, 1), 6), (("dd", ("le", 6), 2), 6),
    (("gp_nich", ("le", 10), 2), 3), (("dd7", PY, 2), 4),
]
assert all(c in CASES for c, _ in BATCH_LEGS)
# legs that are also run from "every row alone"
BATCH_ALONE = ("dd-py-e3-B3", "gp_nich-py-e1-B6")
# states the runs take per leg where the derived count below is not larger
BATCH_RUN = 5000
POWER_LEVEL = 1e-12


def batch_id(leg):
    return "%s-B%d" % (case_id(leg[0]), leg[1])


def batch_seed(leg, start="one"):
    """the engine seed of a leg's chain (fixed before the first run)"""
    return 5200 + 2 * BATCH_LEGS.index(leg) + (1 if start == "alone" else 0)


# Derived, not chosen: per leg the smallest multiple of 1000 (at most
# LEG_SAMPLES) at which (a) the float64 law alone keeps the pooled mass at or
# under 5 % and (b) the oracle's histogram (start "one", the leg's seed)
# rejects every REQUIRED mutant at p < POWER_LEVEL.  Which mutants are
# required is fixed at the count the legs RUN, max(BATCH_RUN, the count of
# (a)), not at LEG_SAMPLES, so that the device legs stay at 5000 states: a
# mutant is required where counts distributed as the true law, tested against
# the mutant's, reach p < POWER_LEVEL with probability >= 0.999 under the
# non-central chi-square approximation (`mutant_power`; the threshold is this
# file's choice).  That is a statement about the run count, not about what
# the law can see: a mutant left out here may well be visible at 20000 states.
# test_f64_batch_posterior.py derives both tables again.  Met at the count:
#                       pooled mass   largest p of a required mutant
#   dd-py-e1-B6            0.0145      2e-83   (at 1000: mass 0.32)
#   dd-py-e3-B3            0.0306      7e-191  (at 3000: mass 0.057)
#   dd-py-e3-B6            0.0312      8e-45   (at 2000: mass 0.12)
#   bb-py-e3-B4            0.0233      7e-72   (at 3000: mass 0.057)
#   dpd-py-e1-B6           0.0353      5e-16   (at 1000: mass 0.31)
#   bnb-py-e3-B3           0.0420      1e-109  (at 2000: mass 0.12)
#   gp_nich-py-e3-B3       0.0444      1e-171  (at 3000: mass 0.067)
#   gp_nich-py-e1-B6       0.0243      6e-248  (at 1000: mass 0.45)
#   dd_bb_gp-py-e1-B6      0.0124      2e-16   (at 2000: lone_keeps_own 2e-9)
#   dd-le6-e2-B6           0.0432      0       (at 3000: mass 0.076)
#   gp_nich-le10-e2-B3     0.0360      0       (at 4000: mass 0.052)
#   dd7-py-e2-B4           0.0497      0       (at 12000: mass 0.057)
BATCH_SAMPLES = {
    "dd-py-e1-B6": 2000, "dd-py-e3-B3": 4000, "dd-py-e3-B6": 3000,
    "bb-py-e3-B4": 4000, "dpd-py-e1-B6": 2000, "bnb-py-e3-B3": 3000,
    "gp_nich-py-e3-B3": 4000, "gp_nich-py-e1-B6": 2000,
    "dd_bb_gp-py-e1-B6": 3000, "dd-le6-e2-B6": 4000,
    "gp_nich-le10-e2-B3": 5000, "dd7-py-e2-B4": 13000,
}
# Not required, with the float64 non-centrality at the count of the rule:
# empties_merged and alpha_undivided with ONE empty group (the identity: 0);
# the two empty-slot mutants under LowEntropy, where new groups are rare (7 to
# 34); lone_keeps_own wherever a row alone is rare -- 3 empty groups (4 to
# 15), LowEntropy (1 to 6), 7 rows (64).  lone_keeps_own on dd-py-e1-B6 (183:
# chance 0.58) and gp_nich-py-e1-B6 (152: 0.24) is left out ONLY because of
# the run count: at LEG_SAMPLES its non-centrality is 731 and 611 and the
# oracle's histogram rejects it at 4e-79 and 5e-77.  The event itself is held
# by dpd-py-e1-B6 and dd_bb_gp-py-e1-B6.  alpha_undivided is PitmanYor's.
_SEEN = ("sequential", "empties_apart", "own_kept")
_ALL3 = ("sequential", "empties_merged", "empties_apart", "own_kept",
         "alpha_undivided")
BATCH_REQUIRED = {
    "dd-py-e1-B6": _SEEN, "dd-py-e3-B3": _ALL3, "dd-py-e3-B6": _ALL3,
    "bb-py-e3-B4": _ALL3,
    "dpd-py-e1-B6": _SEEN + ("lone_keeps_own",), "bnb-py-e3-B3": _ALL3,
    "gp_nich-py-e3-B3": _ALL3, "gp_nich-py-e1-B6": _SEEN,
    "dd_bb_gp-py-e1-B6": _SEEN + ("lone_keeps_own",),
    "dd-le6-e2-B6": ("sequential", "own_kept"),
    "gp_nich-le10-e2-B3": ("sequential", "own_kept"),
    "dd7-py-e2-B4": _ALL3,
}


def batch_states(leg):
    return max(BATCH_RUN, BATCH_SAMPLES[batch_id(leg)])


def mutant_power(expected, mutated, level=POWER_LEVEL):
    """float64 only: counts distributed as `expected`, tested against the
    `mutated` expectation -> (non-centrality, degrees of freedom, chance of
    p < level under the non-central chi-square approximation).  A cell the
    mutant forbids and the law fills is an outright rejection."""
    e = np.asarray(expected, np.float64)
    q = np.asarray(mutated, np.float64)
    pooled, _ = pooling(q)
    ee = np.r_[e[~pooled], e[pooled].sum()] if pooled.any() else e
    qq = np.r_[q[~pooled], q[pooled].sum()] if pooled.any() else q
    keep = qq > 0
    dof = int(keep.sum()) - 1
    if ee[~keep].sum() > 1.0:
        return float("inf"), dof, 1.0
    nc = float((((ee - qq) ** 2)[keep] / qq[keep]).sum())
    if nc < 1e-9:
        return nc, dof, 0.0
    bar = stats.chi2.isf(level, dof)
    return nc, dof, float(stats.ncx2.sf(bar, dof, nc))


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


def oracle_batch_chain(leg, start, T, samples, tile_sweeps=0):
    """ONE OracleMixture chain of batches: sweep k is gibbs_batch over the
    leg's tiles with draw_base = k * n and the leg's seed -> (the state after
    every sweep [samples * T, n], the state after every tile of the first
    `tile_sweeps` sweeps [tile_sweeps * tiles, n])"""
    case, B = leg
    orc, vals = oracle_mixture(case)
    n = len(vals[0])
    assign0, nonempty = start_assign(n, start)
    orc.init_from_assignments(vals, assign0, nonempty, case[2])
    L, h, ptrs, a = orc.L, orc.h, orc._vals, orc.assign
    st = L.orc_rng_seed(batch_seed(leg, start))
    tiles = [(b, min(n, b + B)) for b in range(0, n, B)]
    out = np.zeros((samples * T, n), np.uint32)
    per_tile = []
    for k in range(samples * T):
        for b0, b1 in tiles:
            L.orc_mix_gibbs_batch(h, b0, b1, ptrs, a, st, k * n)
            if k < tile_sweeps:
                per_tile.append(a.copy())
        out[k] = a
    return out, np.array(per_tile, np.uint32).reshape(-1, n)
