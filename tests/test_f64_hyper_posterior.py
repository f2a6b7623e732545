"""The composition "one sequential sweep, then one draw of the
hyper-parameters from a grid" against the float64 joint law of (partition,
grid index) (tests/f64_hyper_posterior.py), on the oracle alone: no GPU, and
nothing of the library.

- the closed-form joint posterior under a uniform prior on the grid is the
  stationary vector of the transition matrix (gap below 1e-12);
- oracle chains -- OracleMixture.gibbs_sequential, orc_mix_slave_score_data_grid
  or orc_py_score_counts, orc_sample_from_scores_overwrite, the state carried
  to the oracle of the chosen grid point by orc_mix_load_state -- pass the
  pooled chi-square against the exact law sum_j e_start @ T**(j T_mix) at the
  project's p > 1e-4;
- power: the same histograms reject the law of the mutant that draws h but
  keeps sweeping under the hyper-parameters it was created with, at the sample
  size the device test uses (f64_hyper_posterior.CHAINS x SAMPLES = 20 480
  states).  Expected chi-square of that rejection, from the two float64 laws
  alone: dd about 3 800 above its 484 degrees of freedom, gp_nich about 3 400
  above 447; the bar is p < 1e-12.

Seeds are fixed: the outcome is deterministic."""
import functools

import numpy as np
import pytest

import f64_hyper_posterior as hp
import f64_posterior as fp

LEVEL = 1e-4
BASE = 7000000
NAMES = sorted(hp.CONFIGS)
# mixing time of the joint chain (max_s TV(T**t[s], pi) < 1e-4), derived again
# by test_joint_posterior_is_stationary
T_MIX = {"dd": 9, "gp_nich": 19}


@functools.lru_cache(maxsize=None)
def matrices(name):
    J = hp.joint(name)
    return J, J.transition(), J.transition(mutant=True)


@functools.lru_cache(maxsize=None)
def histogram(name):
    return hp.oracle_histogram(name, hp.CHAINS, T_MIX[name], hp.SAMPLES, BASE)


def expected(name, mutant=False):
    J, T, Tmut = matrices(name)
    return hp.CHAINS * fp.law_sum(Tmut if mutant else T, J.start(),
                                  T_MIX[name], hp.SAMPLES)


@pytest.mark.parametrize("name", NAMES)
def test_joint_posterior_is_stationary(name):
    J, T, Tmut = matrices(name)
    assert J.H == 4 and len(J.joint) == 4 * 203
    np.testing.assert_allclose(T.sum(1), 1.0, atol=1e-13)
    gap = fp.stationarity_gap(T, J.joint)
    marginal = J.joint.reshape(J.H, J.S).sum(1)
    print(name, "stationarity gap %.2e" % gap, "grid marginal", marginal)
    assert gap < 1e-12
    assert marginal.min() > 0.05          # every grid point is visited
    assert fp.mixing_time(T, J.joint, 1e-4) == T_MIX[name]
    # the mutant's matrix does NOT keep the joint posterior
    assert fp.stationarity_gap(Tmut, J.joint) > 1e-3


@pytest.mark.parametrize("name", NAMES)
def test_pooling_condition(name):
    _, mass = fp.pooling(expected(name))
    assert mass <= 0.05, mass


@pytest.mark.parametrize("name", NAMES)
def test_oracle_chain_has_the_joint_law(name):
    hist = histogram(name)
    assert hist.sum() == hp.CHAINS * hp.SAMPLES
    chi2, dof, p, mass = fp.report(name + " sweep + grid draw", expected(name),
                                   hist)
    assert mass <= 0.05
    assert p > LEVEL, (chi2, dof, p)


@pytest.mark.parametrize("name", NAMES)
def test_stale_cache_mutant_is_rejected_at_the_device_sample_size(name):
    hist = histogram(name)
    assert fp.pooled_chi_square(hist, expected(name))[2] > LEVEL
    chi2, dof, p, _ = fp.report(name + " mutant: sweeps under the old caches",
                                expected(name, mutant=True), hist)
    assert p < 1e-12, (chi2, dof, p)
