"""The oracle's exact chain against the float64 posterior over partitions
(tests/f64_posterior.py), end to end: remove the row, score, sample, add back
-- groups vanishing with their last row, the last group moving into the freed
slot, empty groups filled and a fresh one appended, the new-group mass shared
between the empty groups -- must compose into a chain whose law after T
sweeps is e_start @ P**T, P being the float64 transition matrix on the 203
partitions of 6 rows (877 of 7).  The closed-form posterior is P's
stationary vector to 1e-12 (a check of the reference, not of the library).

M = 100 000 independent `OracleMixture.gibbs_sequential` chains per
histogram, seeds orc_rng_seed(base + chain), T = 4 sweeps from "all rows in
one group" and from "every row alone".  The reference is the exact T-sweep
law, so T needs no burn-in; 4 keeps the 30 histograms of the file (about 3 s
each) within its time and leaves every cell populated (the laws after 4
sweeps are within 2 % of the posterior cell by cell).  Seeds are fixed: the
outcome is deterministic.  The level 1e-4 is the one
test_oracle_models.py::test_scores_sampler_goodness_of_fit uses.

Power.  The same histograms reject mutated REFERENCES (the library is never
mutated); chi-squares measured here, dd-py-e3 / gp_nich-py-e3, M = 10^5, on
202 degrees of freedom:

  ne_plus_one      discount times K + 1, not K            3084 /   2614
  log_n            discount missing within the group      4909 /   5399
  alpha_undivided  empty-group mass not shared          401189 / 313103
  own_kept         own group not decremented             20775 /  48732
  last_never       the last (empty) slot never drawn     26326 /  23255

(gp_nich pools up to 7 cells: 196 to 202 degrees of freedom.)  A histogram
taken after 1 sweep is rejected by the 4-sweep law (chi2 57 854).  The first
three must reach p < 1e-12; the last two were first measured for this file,
so their bar is a chi-square half of the figure above.  At the 20 000 states
of the single-engine device legs (test_gpu_posterior.py) the weakest is
ne_plus_one on gp_nich: chi2 562 on 183 degrees of freedom, p = 4e-40.

Limit: this is a test of STRUCTURE.  When the test was designed (T = 12) a
10 % error in a hyper-parameter was barely visible at this sample size (DD
alphas x 1.1: p = 0.027; NICH kappa x 1.1: p = 0.41); per-model numerics are
tests/f64_scores.py's job.

Measured: the file takes 142 s (103 tests) on the CPU.
"""
import functools

import numpy as np
import pytest

import f64_posterior as fp

M = 100000
T = 4
LEVEL = 1e-4
STARTS = ("one", "alone")
BASE = {"one": 1000000, "alone": 5000000}

IDS = [fp.case_id(c) for c in fp.CASES]
PY_CASES = [c for c in fp.CASES if c[1][0] == "py"]
LE_CASES = [c for c in fp.CASES if c[1][0] == "le"]


@functools.lru_cache(maxsize=None)
def sweep_matrix(case, mut=()):
    return fp.model(case).sweep_matrix(mut)


@functools.lru_cache(maxsize=None)
def histogram(case, start, chains=M, sweeps=T):
    return fp.oracle_histogram(case, start, chains, sweeps, BASE[start])


def expected(case, start, chains=M, sweeps=T, mut=()):
    m = fp.model(case)
    return chains * fp.law_after(sweep_matrix(case, mut),
                                 fp.start_state(m.space, start), sweeps)


# ---------------------------------------------------------------------------
# the reference itself


def test_set_partitions_and_canonical():
    assert [len(fp.set_partitions(n)) for n in range(1, 8)] == [
        1, 2, 5, 15, 52, 203, 877]            # Bell numbers
    parts = fp.set_partitions(6)
    assert len(set(parts)) == 203
    assert all(fp.canonical(p) == p for p in parts)
    assert fp.canonical([7, 7, 2, 9, 2, 7]) == (0, 0, 1, 2, 1, 0)
    space = fp.Space(6)
    a = np.array([[7, 7, 2, 9, 2, 7], [5, 4, 3, 2, 1, 0], [3] * 6])
    assert [space.parts[i] for i in space.indices(a)] == [
        (0, 0, 1, 2, 1, 0), (0, 1, 2, 3, 4, 5), (0,) * 6]


def test_transition_matrices_are_stochastic():
    m = fp.model(fp.CASES[1])
    for row in range(m.n):
        P = m.row_matrix(row)
        assert np.all(P >= 0)
        np.testing.assert_allclose(P.sum(1), 1.0, atol=1e-14)
        # a row step is a projection on the other rows' partition: P P = P
        np.testing.assert_allclose(P @ P, P, atol=1e-14)


@pytest.mark.parametrize("case", PY_CASES, ids=fp.case_id)
def test_closed_form_is_stationary(case):
    """PitmanYor: the closed-form posterior is the sweep's stationary vector"""
    m = fp.model(case)
    gap = fp.stationarity_gap(sweep_matrix(case), m.posterior())
    print("%s stationarity gap %.2e" % (fp.case_id(case), gap))
    assert gap < 1e-12


@pytest.mark.parametrize("case", LE_CASES, ids=fp.case_id)
def test_low_entropy_stationary_law(case):
    """LowEntropy: exp(score_counts) times the marginals is stationary under
    score_add_value, with dataset_size == N (no postpred correction) and with
    dataset_size > N (one constant per new group): see f64_posterior's
    docstring"""
    m = fp.model(case)
    gap = fp.stationarity_gap(sweep_matrix(case), m.posterior())
    print("%s stationarity gap %.2e" % (fp.case_id(case), gap))
    assert gap < 1e-12


@pytest.mark.parametrize("case", [c for c in fp.CASES
                                  if c[2] > 1 and c[0] in ("dd", "gp_nich")],
                         ids=fp.case_id)
def test_mutants_are_not_stationary(case):
    """the self-check has teeth: every mutated matrix that differs from the
    true one moves the closed form by far more than 1e-12"""
    m = fp.model(case)
    pi = m.posterior()
    for mut in fp.MUTANTS:
        if case[1][0] == "le" and mut in ("ne_plus_one", "log_n",
                                          "alpha_undivided"):
            continue        # PitmanYor's terms
        gap = fp.stationarity_gap(sweep_matrix(case, (mut,)), pi)
        assert gap > 1e-4, (mut, gap)


def test_pooled_chi_square():
    rng = np.random.default_rng(5)
    p = np.r_[np.full(50, 0.0199), np.full(50, 0.0001)]
    e = 10000 * p                       # 50 cells of 199, 50 cells of 1
    pooled, mass = fp.pooling(e)
    assert pooled.sum() == 50 and abs(mass - 0.005) < 1e-12
    ps = []
    for _ in range(200):
        chi2, dof, pv = fp.pooled_chi_square(rng.multinomial(10000, p), e)
        assert dof == 50
        ps.append(pv)
    assert 0.35 < np.mean(ps) < 0.65    # uniform p-values under the truth
    # a lone small cell takes the next smallest with it
    pooled, mass = fp.pooling([3.0, 6.0, 50.0, 41.0])
    assert pooled.tolist() == [True, True, False, False]
    # a count where the reference allows none is a rejection
    assert fp.pooled_chi_square([1, 99, 0], [0.0, 90.0, 10.0])[2] == 0.0
    wrong = p[::-1]
    assert fp.pooled_chi_square(rng.multinomial(10000, wrong), e)[2] < 1e-12


# ---------------------------------------------------------------------------
# the oracle's chain against the exact law


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("case", fp.CASES, ids=fp.case_id)
def test_pooling_condition(case, start):
    """a condition on the float64 law alone: pooling absorbs at most 5 % of
    the expected mass"""
    _, mass = fp.pooling(expected(case, start))
    assert mass <= 0.05, mass


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("case", fp.CASES, ids=fp.case_id)
def test_oracle_chain_has_the_exact_law(case, start):
    hist = histogram(case, start)
    assert hist.sum() == M
    chi2, dof, p, mass = fp.report("%s from %s" % (fp.case_id(case), start),
                                   expected(case, start), hist)
    assert mass <= 0.05
    assert p > LEVEL, (chi2, dof, p)


def test_wrong_sweep_count_is_rejected():
    """not passing for lack of power: states after ONE sweep against the
    4-sweep law (chi2 measured: 57854 on 202 degrees of freedom)"""
    case = fp.CASES[1]
    hist = fp.oracle_histogram(case, "one", M, 1, BASE["one"])
    chi2, dof, p, _ = fp.report("one sweep against four",
                                expected(case, "one"), hist)
    assert p < 1e-12


# (mutant, chi2 measured on dd-py-e3, on gp_nich-py-e3) -- the bar of the
# last two is half the measured chi-square
MEASURED = {
    "ne_plus_one": (3084, 2614),
    "log_n": (4909, 5399),
    "alpha_undivided": (401189, 313103),
    "own_kept": (20775, 48732),
    "last_never": (26326, 23255),
}
MUTANT_CASES = [("dd", fp.PY, 3), ("gp_nich", fp.PY, 3)]


@pytest.mark.parametrize("which", [0, 1], ids=["dd", "gp_nich"])
@pytest.mark.parametrize("mut", fp.MUTANTS)
def test_mutated_reference_is_rejected(mut, which):
    """the histogram the true reference accepts rejects the mutated one"""
    case = MUTANT_CASES[which]
    hist = histogram(case, "one")
    assert fp.pooled_chi_square(hist, expected(case, "one"))[2] > LEVEL
    chi2, dof, p, _ = fp.report("%s mutant %s" % (fp.case_id(case), mut),
                                expected(case, "one", mut=(mut,)), hist)
    assert p < 1e-12
    if mut in ("own_kept", "last_never"):
        assert chi2 > MEASURED[mut][which] / 2.0


# the single-engine device legs (test_gpu_posterior.py) take fewer samples;
# the same mutants at that count, on oracle chains
LEG_SAMPLES = fp.LEG_SAMPLES


@pytest.mark.parametrize("which", [0, 1], ids=["dd", "gp_nich"])
@pytest.mark.parametrize("mut", fp.MUTANTS)
def test_mutants_rejected_at_the_single_engine_sample_count(mut, which):
    case = MUTANT_CASES[which]
    hist = histogram(case, "one", LEG_SAMPLES)
    assert fp.pooled_chi_square(
        hist, expected(case, "one", LEG_SAMPLES))[2] > LEVEL
    chi2, dof, p, _ = fp.report(
        "%s mutant %s at %d" % (fp.case_id(case), mut, LEG_SAMPLES),
        expected(case, "one", LEG_SAMPLES, mut=(mut,)), hist)
    assert p < 1e-12
