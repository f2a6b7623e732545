"""The exact chain on the device against the float64 posterior over
partitions (tests/f64_posterior.py): 6 rows (203 partitions; one case of 7,
877), K between 2 and 8, structural steps at almost every row -- the shape
test_gpu_chains.py does not reach (its smallest is 400 rows in 150 groups).

k_chains.  1024 engines of one configuration (same rows, own entropy state;
512 start from "all rows in one group", 512 from "every row alone") are
stepped with sweep_sequential_many and one state per chain is taken every T
sweeps, T the smallest number of sweeps with max_s TV(P**T[s], pi) < 1e-4 in
the float64 matrix (T_MIX, derived again by the test).  A launch of 1024
chains costs about 50 ms, nearly all of it the host preparing and collecting
1024 engines, so 30 states per chain are taken, 30 720 per configuration (8 to
23 s each, 2.9 minutes for the 15; 100 states per chain would take 9).
Expected counts are sum_j e_start @ P**(jT); the bar is p > 1e-4 as in
test_f64_posterior.py, whose mutants are rejected at p < 1e-40 with 20 000
states already.  Measured p: dd 0.60 / 0.30 (1 / 3 empty groups), bb 0.039 /
0.00039, dpd 0.39 / 0.35, bnb 0.48 / 0.21, gp_nich 0.90 / 0.84, dd_bb_gp 0.11
/ 0.18, LowEntropy dd 0.029 and gp_nich 0.065, 7 rows 0.44.  bb with 3 empty
groups sits close to the bar: the oracle, run on the CPU with the same 1024
entropy states, gives the same chi-square to the digit (276.4 on 202), and
the same chains carried on to 150 states each give p = 0.39 -- a fluctuation
of these seeds, not a drift.  64 of the chains are followed by
OracleMixture.gibbs_sequential from the same entropy states: assignments (so
the partition) and the entropy state must be identical at every sampling
point.

The other ways to run one row -- debug.sequential_chain 1 and 0, and the
batched engine with batch_rows = 1 under value_sorted 0 and 2 -- are one
chain per engine and several launches per row, so they take
f64_posterior.LEG_SAMPLES states from one engine, T sweeps apart;
test_f64_posterior.py shows that the structural mutants are still rejected at
p < 1e-12 at that count.  Batches of more than one row score against a
snapshot and do not have the posterior as their stationary law: they are held
to their own float64 law in test_gpu_batch_posterior.py.
"""
import time

import numpy as np
import pytest

import f64_posterior as fp

pytestmark = pytest.mark.gpu

CHAINS = 1024
SAMPLES = 30
FOLLOWED = 64
LEVEL = 1e-4

# sweeps between two states of one chain: the smallest T with
# max_s TV(P**T[s], pi) < 1e-4 in the float64 sweep matrix
T_MIX = {
    "dd-py-e1": 7, "dd-py-e3": 7, "bb-py-e1": 6, "bb-py-e3": 6,
    "dpd-py-e1": 5, "dpd-py-e3": 5, "bnb-py-e1": 7, "bnb-py-e3": 7,
    "gp_nich-py-e1": 7, "gp_nich-py-e3": 7, "dd_bb_gp-py-e1": 6,
    "dd_bb_gp-py-e3": 6, "dd-le6-e2": 11, "gp_nich-le10-e2": 15,
    "dd7-py-e2": 8,
}

_SWEEP = {}


def reference(case):
    """-> (model, sweep matrix, posterior, T)"""
    if case not in _SWEEP:
        m = fp.model(case)
        P = m.sweep_matrix()
        pi = m.posterior()
        assert fp.stationarity_gap(P, pi) < 1e-12
        T = fp.mixing_time(P, pi, 1e-4)
        assert T == T_MIX[fp.case_id(case)]
        _SWEEP[case] = (m, P, pi, T)
    return _SWEEP[case]


def make_engine(case, start, options=()):
    from distributions_amd import engine
    config, prior, empty = case
    make = {fp.DD: lambda kw: engine.dd_shared(kw["alphas"]),
            fp.BB: lambda kw: engine.bb_shared(kw["alpha"], kw["beta"]),
            fp.GP: lambda kw: engine.gp_shared(kw["alpha"], kw["inv_beta"]),
            fp.NICH: lambda kw: engine.nich_shared(
                kw["mu"], kw["kappa"], kw["sigmasq"], kw["nu"]),
            fp.BNB: lambda kw: engine.bnb_shared(kw["alpha"], kw["beta"],
                                                 kw["r"]),
            fp.DPD: lambda kw: engine.dpd_shared(kw["alpha"], kw["betas"],
                                                 kw["beta0"])}
    kinds = fp.shared_kw(config)
    gsh = [make[k](kw) for k, kw in kinds]
    vals = [np.asarray(c, np.float32 if k == fp.NICH else np.uint32)
            for (k, _), c in zip(kinds, fp.ROWS[config])]
    if prior[0] == "py":
        gpu = engine.Gibbs(prior[1], prior[2], gsh)
    else:
        gpu = engine.Gibbs(0.0, 0.0, gsh, dataset_size=prior[1])
    for name, value in options:
        gpu.set_option(name, value)
    assign, nonempty = fp.start_assign(len(vals[0]), start)
    gpu.load_rows(vals, assign, nonempty, empty)
    return gpu


def expected_counts(case, chains_by_start, samples):
    m, P, _, T = reference(case)
    return sum(c * fp.law_sum(P, fp.start_state(m.space, s), T, samples)
               for s, c in chains_by_start.items())


@pytest.mark.parametrize("case", fp.CASES, ids=fp.case_id)
def test_many_chains_have_the_posterior_law(case):
    """k_chains, 1024 chains per launch: the histogram of their states
    against the exact law, and 64 of them equal to the oracle's chains"""
    from distributions_amd import _core
    m, P, pi, T = reference(case)
    n = m.n
    t0 = time.time()
    starts = ["one" if i % 2 == 0 else "alone" for i in range(CHAINS)]
    engines = [make_engine(case, s) for s in starts]
    cores = [g.core for g in engines]
    states = np.array([_core.rng_seed(77000 + i) for i in range(CHAINS)],
                      np.uint32)
    orcs = []
    for i in range(FOLLOWED):
        orc, vals = fp.oracle_mixture(case)
        assign, nonempty = fp.start_assign(n, starts[i])
        orc.init_from_assignments(vals, assign, nonempty, case[2])
        orcs.append(orc)
    out = np.zeros((SAMPLES, CHAINS, n), np.uint32)
    for s in range(SAMPLES):
        for _ in range(T):
            new = _core.sweep_sequential_many(cores, 0, n, states)
            for i, orc in enumerate(orcs):
                want = orc.gibbs_sequential(0, n, int(states[i]))
                assert int(new[i]) == want, (s, i)
            states = new
        for i, g in enumerate(engines):
            out[s, i] = g.assignments()
        for i, orc in enumerate(orcs):
            assert np.array_equal(out[s, i], orc.assign), (s, i)
            assert fp.canonical(out[s, i]) == fp.canonical(orc.assign)
    hist = m.space.histogram(out.reshape(-1, n))
    want = expected_counts(case, {"one": CHAINS // 2, "alone": CHAINS // 2},
                           SAMPLES)
    chi2, dof, p, mass = fp.report(
        "k_chains %s T %d (%.1f s)" % (fp.case_id(case), T,
                                        time.time() - t0), want, hist)
    assert mass <= 0.05
    assert p > LEVEL, (chi2, dof, p)
    assert len(set(int(x) for x in states)) == CHAINS
    for g in engines[::61] + engines[-1:]:
        assert g.validate()["code"] == 0
        assert 2 <= len(g) <= n + case[2]


LEG_CASE = ("dd", fp.PY, 3)
LEGS = {
    "chain_host_steps": (("debug.sequential_chain", 1),),
    "chain_batches_of_one": (("debug.sequential_chain", 0),),
    "batch_generic": (("value_sorted", 0),),
    "batch_value_sorted": (("value_sorted", 2),),
}


def run_leg(case, leg, samples, start="one"):
    from distributions_amd import _core
    m, P, pi, T = reference(case)
    n = m.n
    gpu = make_engine(case, start, LEGS[leg])
    out = np.zeros((samples, n), np.uint32)
    st = _core.rng_seed(4100)
    sweeps = 0
    for s in range(samples):
        for _ in range(T):
            if leg.startswith("chain"):
                st = gpu.sweep_sequential(0, n, st)
            else:   # row i of sweep k takes engine draw k * n + i
                gpu.sweep(0, n, 1, 4100, draw_base=sweeps * n)
            sweeps += 1
        out[s] = gpu.assignments()
    assert gpu.validate()["code"] == 0
    return gpu, m.space.histogram(out)


@pytest.mark.parametrize("leg", list(LEGS))
def test_single_engine_paths_have_the_posterior_law(leg):
    """one chain, one engine, fp.LEG_SAMPLES states T sweeps apart, through
    each of the other ways to run one row.  Measured: 49, 43, 40 and 27 s;
    the four paths take the same draws and gave the same histogram, chi2
    208.5 on 202 degrees of freedom, p = 0.36"""
    case = LEG_CASE
    t0 = time.time()
    gpu, hist = run_leg(case, leg, fp.LEG_SAMPLES)
    assert gpu.core.chain_launches() == 0      # k_chains took no part
    by_value, generic = gpu.path_counts()
    if leg == "batch_value_sorted":
        assert by_value > 0 and generic == 0
    else:
        assert by_value == 0 and generic > 0
    want = expected_counts(case, {"one": 1}, fp.LEG_SAMPLES)
    chi2, dof, p, mass = fp.report(
        "%s %s %d states (%.1f s)" % (leg, fp.case_id(case), fp.LEG_SAMPLES,
                                      time.time() - t0), want, hist)
    assert mass <= 0.05
    assert p > LEVEL, (chi2, dof, p)
