"""The engine's alternation -- sweep_sequential_many, then the hyper-parameter
draw per engine (sample_hypers / sample_clustering: grid, draw and install on
the device) -- against the float64 joint law of (partition, grid index)
(tests/f64_hyper_posterior.py; the oracle passes the same test on the CPU,
tests/test_f64_hyper_posterior.py, where the stale-cache mutant is shown to be
rejected at this sample size).

f64_hyper_posterior.CHAINS engines, SAMPLES states each, one state every T_MIX
transitions (T_MIX from mixing_time of the joint chain's float64 matrix,
derived again here); expected counts sum_j e_start @ T**(j T_MIX); pooled
chi-square at the project's p > 1e-4.  Chain c is seeded like the oracle's
chain c of the CPU test, and both take the sweep's and the draw's entropy from
the one engine state.  Seeds are fixed: the outcome is deterministic."""
import time

import numpy as np
import pytest

import f64_hyper_posterior as hp
import f64_posterior as fp

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

LEVEL = 1e-4
BASE = 7000000
T_MIX = {"dd": 9, "gp_nich": 19}


def engine_shareds(name):
    """per grid point the engine's SharedParams list"""
    from distributions_amd import engine
    make = {fp.DD: lambda kw: engine.dd_shared(kw["alphas"]),
            fp.GP: lambda kw: engine.gp_shared(kw["alpha"], kw["inv_beta"]),
            fp.NICH: lambda kw: engine.nich_shared(
                kw["mu"], kw["kappa"], kw["sigmasq"], kw["nu"])}
    config, what, grid = hp.CONFIGS[name]
    base = fp.shared_kw(config)
    out = []
    for point in grid:
        kinds = [(base[0][0], point)] + base[1:] if what == "shared" else base
        out.append([make[k](kw) for k, kw in kinds])
    return out


@pytest.mark.parametrize("name", sorted(hp.CONFIGS))
def test_sweep_and_grid_draw_have_the_joint_law(name):
    from distributions_amd import _core, engine
    J = hp.joint(name)
    Tm = J.transition()
    assert fp.stationarity_gap(Tm, J.joint) < 1e-12
    T = fp.mixing_time(Tm, J.joint, 1e-4)
    assert T == T_MIX[name]
    what = hp.CONFIGS[name][1]
    cands = hp.candidates(name)
    gsh = engine_shareds(name)
    vals = hp.values(name)
    n = len(vals[0])
    alphas = np.array([p[0] for _, p in cands], np.float32)
    ds = np.array([p[1] for _, p in cands], np.float32)
    t0 = time.time()
    engines = []
    for c in range(hp.CHAINS):
        g = engine.Gibbs(cands[0][1][0], cands[0][1][1], gsh[0])
        g.load_rows(vals, np.zeros(n, np.uint32), 1, hp.EMPTY)
        engines.append(g)
    states = np.array([_core.rng_seed(BASE + c) for c in range(hp.CHAINS)],
                      np.uint32)
    h = np.zeros(hp.CHAINS, np.int64)
    out_h = np.zeros((hp.SAMPLES, hp.CHAINS), np.int64)
    out_a = np.zeros((hp.SAMPLES, hp.CHAINS, n), np.uint32)
    for s in range(hp.SAMPLES):
        for _ in range(T):
            swept = engine.sweep_sequential_many(engines, 0, n, states)
            for c, g in enumerate(engines):
                if what == "shared":
                    h[c], states[c] = g.sample_hypers(0, [x[0] for x in gsh],
                                                      int(swept[c]))
                else:
                    h[c], states[c] = g.sample_clustering(alphas, ds,
                                                          int(swept[c]))
        for c, g in enumerate(engines):
            out_a[s, c] = g.assignments()
        out_h[s] = h
    hist = J.histogram(out_h.reshape(-1), out_a.reshape(-1, n))
    want = hp.CHAINS * fp.law_sum(Tm, J.start(), T, hp.SAMPLES)
    chi2, dof, p, mass = fp.report(
        "%s engines: sweep + grid draw (%.1f s)" % (name, time.time() - t0),
        want, hist)
    print("grid marginal", np.bincount(out_h.reshape(-1), minlength=J.H)
          / float(out_h.size), "expected", J.joint.reshape(J.H, J.S).sum(1))
    assert mass <= 0.05
    assert p > LEVEL, (chi2, dof, p)
    for g in engines[:4]:
        g.validate()
