"""Batches of several rows against their float64 law over partitions
(tests/f64_posterior.py, `Model.batch_matrix`).

DESIGN section 3 defines a batch as independent draws: every row draws from
its conditional given the state at batch entry minus itself, then all moves
are applied.  On the 203 partitions of 6 rows (877 of 7) that is a stochastic
matrix, and the law of the chain after t sweeps is e_start @ P**t exactly,
whatever P's stationary vector is (it is NOT the posterior: total variation
0.24 to 0.55 over the legs, printed and asserted above 0.02 -- otherwise this
file could not tell a batch from the sequential chain).

The law itself: a batch of one row is `sweep_matrix` to the bit; rows sum to
1; the order of the rows inside a batch does not matter; `step_law`, now
written through `row_options`, gives the matrices it gave before.

The oracle: ONE `OracleMixture` chain per leg and start, sweep k being
`gibbs_batch` over the tiles with draw_base = k * n, a state taken every T
sweeps (T: the smallest with max_s TV(P**T[s], stationary) < 1e-4, derived
again here), `fp.batch_states(leg)` states, against `law_sum`: pooled mass
<= 0.05, p > 1e-4.  Seeds (`fp.batch_seed`) were fixed before the first run.
Every sweep of the run, and every tile of its first 300 sweeps, must be a
transition the law allows.

Power: the same chain's first `fp.BATCH_SAMPLES[leg]` states reject every
mutant of `fp.BATCH_REQUIRED[leg]` at p < 1e-12; both tables are derived
again (the count is the smallest, the required mutants are those the float64
law alone can see at the number of states the legs run).

Measured (start "one"; T, states, pooled mass, p):
  dd-py-e1-B6 13 5000 0.0093 0.49      dd-py-e3-B3 10 5000 0.0158 0.15
  dd-py-e3-B6 16 5000 0.0119 0.034     bb-py-e3-B4 10 5000 0.0108 0.81
  dpd-py-e1-B6 8 5000 0.0096 0.22      bnb-py-e3-B3 11 5000 0.0136 0.26
  gp_nich-py-e3-B3 10 5000 0.0321 0.50 gp_nich-py-e1-B6 14 5000 0.0018 0.79
  dd_bb_gp-py-e1-B6 10 5000 0.0114 0.22 dd-le6-e2-B6 31 5000 0.0273 0.44
  gp_nich-le10-e2-B3 20 5000 0.0360 0.33 dd7-py-e2-B4 11 13000 0.0497 0.70
dd-py-e3-B6 carried on to 10000 and 20000 states: p = 0.28 and 0.41.
From "every row alone": dd-py-e3-B3 0.12, gp_nich-py-e1-B6 0.023.  The file
takes about 4 minutes (92 tests) on the CPU, a third of it the leg of 7 rows.
"""
import functools

import numpy as np
import pytest

import f64_posterior as fp
import f64_scores as fs

LEVEL = 1e-4
TILE_SWEEPS = 300

# sweeps between two states: the smallest T with max_s TV(P**T[s], pi_B) <
# 1e-4, pi_B the batch chain's own stationary vector
BATCH_T = {
    "dd-py-e1-B6": 13, "dd-py-e3-B3": 10, "dd-py-e3-B6": 16,
    "bb-py-e3-B4": 10, "dpd-py-e1-B6": 8, "bnb-py-e3-B3": 11,
    "gp_nich-py-e3-B3": 10, "gp_nich-py-e1-B6": 14,
    "dd_bb_gp-py-e1-B6": 10, "dd-le6-e2-B6": 31, "gp_nich-le10-e2-B3": 20,
    "dd7-py-e2-B4": 11,
}

LEGS = fp.BATCH_LEGS
RUNS = [(leg, "one") for leg in LEGS] + [
    (leg, "alone") for leg in LEGS if fp.batch_id(leg) in fp.BATCH_ALONE]


def run_id(run):
    return "%s-%s" % (fp.batch_id(run[0]), run[1])


@functools.lru_cache(maxsize=None)
def tile_matrices(leg, mut=()):
    m = fp.model(leg[0])
    return [m.batch_matrix(tile, mut) for tile in m.batch_tiles(leg[1])]


@functools.lru_cache(maxsize=None)
def sweep_matrix(leg, mut=()):
    P = np.eye(len(fp.model(leg[0]).space.parts))
    for Q in tile_matrices(leg, mut):
        P = P @ Q
    return P


@functools.lru_cache(maxsize=None)
def reference(leg):
    """-> (model, sweep matrix, its stationary vector, T)"""
    m = fp.model(leg[0])
    P = sweep_matrix(leg)
    pi = fp.stationary(P)
    assert fp.stationarity_gap(P, pi) < 1e-13
    T = fp.mixing_time(P, pi, 1e-4)
    assert T == BATCH_T[fp.batch_id(leg)]
    return m, P, pi, T


@functools.lru_cache(maxsize=None)
def chain(leg, start):
    """-> (partition index after every sweep, after every tile of the first
    TILE_SWEEPS sweeps)"""
    m, _, _, T = reference(leg)
    states, tiles = fp.oracle_batch_chain(leg, start, T, fp.batch_states(leg),
                                          TILE_SWEEPS)
    return m.space.indices(states), m.space.indices(tiles)


@functools.lru_cache(maxsize=None)
def expected(leg, start, samples, mut=()):
    m, _, _, T = reference(leg)
    return fp.law_sum(sweep_matrix(leg, mut), fp.start_state(m.space, start),
                      T, samples)


def histogram(leg, start, samples):
    m, _, _, T = reference(leg)
    idx = chain(leg, start)[0][T - 1::T][:samples]
    assert len(idx) == samples
    return np.bincount(idx, minlength=len(m.space.parts))


# ---------------------------------------------------------------------------
# the law itself


def step_law_before(self, part, row, mut=()):
    """`Model.step_law` as it stood before `row_options` (kept here as the
    yardstick of the refactoring).  It is a second statement of the row step:
    a change to what `py_terms` / `le_terms` or a mutant mean reaches it
    through those functions, but a new mutant or term written into
    `row_options` itself has to be written here too, or left out of the
    comparison below."""
    blocks = fp._blocks(part)
    own = [b for b in blocks if row in b][0]
    rest = [b for b in blocks if b is not own]
    left = tuple(r for r in own if r != row)
    slots = rest + ([left] if left else [])
    scored = list(slots)
    if left and "own_kept" in mut:
        scored[-1] = own
    m = len(slots)
    E = self.empty
    sizes = np.array([len(b) for b in scored] + [0] * E, np.float64)
    N = self.n - 1
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
        out.append((fp._partition(others + [joined], self.n), w[k]))
    out.append((fp._partition(slots + [(row,)], self.n), w[m:].sum()))
    return out


@pytest.mark.parametrize("case", [("dd", fp.PY, 3), ("gp_nich", fp.PY, 1),
                                  ("dd", ("le", 6), 2)], ids=fp.case_id)
def test_row_step_is_unchanged_to_the_bit(case):
    m = fp.model(case)
    muts = [()] + [(x,) for x in fp.MUTANTS
                   if case[1][0] == "py" or x in ("own_kept", "last_never")]
    for mut in muts:
        for row in (0, 3, m.n - 1):
            P = m.row_matrix(row, mut)
            Q = np.zeros_like(P)
            for i, p in enumerate(m.space.parts):
                law = step_law_before(m, p, row, mut)
                assert law == m.step_law(p, row, mut)
                for q, w in law:
                    Q[i, m.space.index[q]] += w
            assert np.array_equal(P, Q), (mut, row)


def test_row_options_keep_slot_identities():
    m = fp.model(("dd", fp.PY, 3))
    part = (0, 1, 0, 2, 1, 0)           # blocks {0,2,5} {1,4} {3}
    labels, w = m.row_options(part, 0)
    assert labels == [1, 2, 0, 3, 4, 5] and abs(w.sum() - 1) < 1e-15
    assert w[3] == w[4] == w[5]         # the empty slots share one mass
    labels, w = m.row_options(part, 3)  # alone: its group is no option
    assert labels == [0, 1, 3, 4, 5] and abs(w.sum() - 1) < 1e-15
    labels, w = m.row_options(part, 3, ("lone_keeps_own",))
    assert labels == [0, 1, 2, 3, 4, 5] and w[2] == w[3]


@pytest.mark.parametrize("case", sorted(set(c for c, _ in LEGS)),
                         ids=fp.case_id)
def test_batches_of_one_row_are_the_sequential_sweep(case):
    m = fp.model(case)
    diff = np.abs(m.batch_sweep_matrix(1) - m.sweep_matrix()).max()
    print("%s max difference %.1e" % (fp.case_id(case), diff))
    assert diff == 0.0


@pytest.mark.parametrize("leg", LEGS, ids=fp.batch_id)
def test_batch_matrices_are_stochastic(leg):
    m = fp.model(leg[0])
    assert len(tile_matrices(leg)) == -(-m.n // leg[1])
    for Q in tile_matrices(leg):
        assert np.all(Q >= 0)
        np.testing.assert_allclose(Q.sum(1), 1.0, atol=1e-12)
    np.testing.assert_allclose(sweep_matrix(leg).sum(1), 1.0, atol=1e-12)
    np.testing.assert_array_equal(sweep_matrix(leg),
                                  m.batch_sweep_matrix(leg[1]))


@pytest.mark.parametrize("case", [("dd", fp.PY, 3), ("gp_nich", fp.PY, 1)],
                         ids=fp.case_id)
def test_order_inside_a_batch_does_not_matter(case):
    m = fp.model(case)
    P = m.batch_matrix([0, 1, 2, 3])
    for rows in ([3, 2, 1, 0], [2, 0, 3, 1]):
        np.testing.assert_allclose(m.batch_matrix(rows), P, rtol=0,
                                   atol=1e-14)
    # and it is not the sequential product of the same rows
    assert np.abs(m.batch_matrix([0, 1, 2, 3], ("sequential",)) -
                  P).max() > 1e-3


@pytest.mark.parametrize("leg", LEGS, ids=fp.batch_id)
def test_batch_chain_is_not_the_posterior_chain(leg):
    m, P, pi, T = reference(leg)
    tv = 0.5 * np.abs(pi - m.posterior()).sum()
    print("%s T %d TV(stationary, posterior) %.3f" % (fp.batch_id(leg), T,
                                                      tv))
    assert tv > 0.02


# ---------------------------------------------------------------------------
# the oracle against the law


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_oracle_batches_have_the_exact_law(run):
    leg, start = run
    m, P, pi, T = reference(leg)
    samples = fp.batch_states(leg)
    want = expected(leg, start, samples)
    chi2, dof, p, mass = fp.report(
        "%s from %s T %d states %d" % (fp.batch_id(leg), start, T, samples),
        want, histogram(leg, start, samples))
    assert mass <= 0.05
    assert p > LEVEL, (chi2, dof, p)


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_no_transition_of_probability_zero(run):
    leg, start = run
    m, P, pi, T = reference(leg)
    sweeps, tiles = chain(leg, start)
    first = m.space.index[fp.canonical(fp.start_assign(m.n, start)[0])]
    path = np.r_[first, sweeps]
    assert np.all(P[path[:-1], path[1:]] > 0)
    mats = tile_matrices(leg)
    path = np.r_[first, tiles]
    assert len(tiles) == TILE_SWEEPS * len(mats)
    for k, Q in enumerate(mats):
        assert np.all(Q[path[k:-1:len(mats)], path[k + 1::len(mats)]] > 0), k
    assert any((Q == 0).any() for Q in mats)    # the check can fail


# ---------------------------------------------------------------------------
# power


def mutants_of(leg):
    return [x for x in fp.BATCH_MUTANTS
            if leg[0][1][0] == "py" or x != "alpha_undivided"]


@pytest.mark.parametrize("leg", LEGS, ids=fp.batch_id)
def test_required_mutants_are_rejected_at_the_derived_count(leg):
    """at fp.BATCH_SAMPLES[leg] states the pooled mass is within 5 % and
    every required mutant is rejected; 1000 states fewer, one of the two
    fails"""
    name = fp.batch_id(leg)
    floor = fp.BATCH_SAMPLES[name]
    assert floor % 1000 == 0 and floor <= fp.LEG_SAMPLES

    def holds(samples):
        _, mass = fp.pooling(expected(leg, "one", samples))
        worst = max(fp.pooled_chi_square(
            histogram(leg, "one", samples),
            expected(leg, "one", samples, (mut,)))[2]
            for mut in fp.BATCH_REQUIRED[name])
        print("%s states %d pooled mass %.4f largest mutant p %.3g" % (
            name, samples, mass, worst))
        return mass <= 0.05 and worst < fp.POWER_LEVEL

    assert holds(floor)
    assert floor == 1000 or not holds(floor - 1000)
    samples = fp.batch_states(leg)
    hist = histogram(leg, "one", samples)
    assert fp.pooled_chi_square(hist, expected(leg, "one", samples))[2] > LEVEL
    for mut in fp.BATCH_REQUIRED[name]:
        chi2, dof, p, _ = fp.report(
            "%s mutant %s" % (name, mut),
            expected(leg, "one", samples, (mut,)), hist)
        assert p < fp.POWER_LEVEL


@pytest.mark.parametrize("leg", LEGS, ids=fp.batch_id)
def test_required_mutants_are_those_the_law_can_see(leg):
    """float64 only: fp.BATCH_REQUIRED[leg] is the set of mutants whose law
    differs from the true one enough for p < 1e-12 with probability 0.999 at
    the number of states the leg runs"""
    name = fp.batch_id(leg)
    samples = 1000
    while fp.pooling(expected(leg, "one", samples))[1] > 0.05:
        samples += 1000
    samples = max(fp.BATCH_RUN, samples)
    want = expected(leg, "one", samples)
    seen = []
    for mut in mutants_of(leg):
        nc, dof, power = fp.mutant_power(want,
                                         expected(leg, "one", samples, (mut,)))
        print("%s %-16s non-centrality %9.1f dof %3d power %.3f" % (
            name, mut, nc, dof, power))
        if power >= 0.999:
            seen.append(mut)
    assert sorted(seen) == sorted(fp.BATCH_REQUIRED[name])
    assert "sequential" in seen
