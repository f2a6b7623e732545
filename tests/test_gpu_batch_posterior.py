"""Batches of several rows on the device against their float64 law over
partitions (`f64_posterior.Model.batch_matrix`; the law, its identities, the
oracle's chains and the planted bugs are in test_f64_batch_posterior.py).

One engine per leg (test_gpu_posterior.make_engine), 6 rows, started from
"all rows in one group": sweep k is gpu.sweep(0, n, B, seed, draw_base = k *
n), the engine cutting the rows into the tiles [0, B), [B, 2B), ...; a state
is taken every T sweeps, fp.batch_states(leg) states, and their histogram is
held to sum_j e_start @ P**(jT), P the float64 matrix of one sweep of batches:
pooled mass <= 0.05, p > 1e-4.  T, the number of states and the expected
counts come from the float64 matrices alone.

Kernels.  At 6 rows every batch that is not value-sorted is sampled by
k_rows_wave, the wave-per-row kernel (a batch of at most 2048 rows whose K
scores fit in LDS): the legs called "wave" below -- one small-domain feature
with value_sorted 0, the general rows (NICH, several features, BNB),
LowEntropy -- exercise that kernel's batch semantics and the apply /
normalise kernels behind it, NOT k_sweep_sample, k_sweep_program or
k_rows_scratch, which no batch of this size reaches (scratch_batches == 0 is
asserted).  value_sorted 2 forces the value-sorted kernels (path_counts()
asserted; rows they hand over go to k_rows_wave as at any size).  float_stats
1 applies the moves through the merged float statistics (merged_batches
asserted).  Scan sampling (sampling 1) is covered on the value-sorted path
alone (every batch counted in scan_batches): the scan claims the exact mode's
distribution at tolerance level, and this is a check of that claim that does
not go through the exact mode's indices.  NOT covered: the scan on general
rows (k_rows_scratch<scan>).  k_rows_wave does not read the option, so a
gp_nich leg with sampling 1 would be the exact leg run twice; nothing at 6
rows and K <= 9 reaches that kernel, and it stays held only by
tests/test_gpu_scan.py and tests/test_gpu_fullsize_modes.py.

The exact-mode legs are also followed: the oracle's chain of the same leg and
seed (fp.oracle_batch_chain, shared between the legs of one seed) must hold
the same assignments at every sampling point, which tells "engine != oracle"
from "both != the float64 law".  Every leg ends with validate().

Measured on one MI355X (seconds, p; the followed legs held the oracle's
assignments throughout, so their p is the oracle's):
  dd-py-e3-B3  value_sorted 0 / 2        8.1 / 4.0    0.15
  dd-py-e3-B6  value_sorted 0 / 2        5.5 / 3.4    0.034 (see below)
  dd-py-e3-B6  value_sorted 2, scan      4.5          0.034
  bb-py-e3-B4  value_sorted 0 / 2        5.9 / 3.8    0.81
  dd-py-e1-B6, dpd-py-e1-B6  (2)         2.8, 2.0     0.49, 0.22
  gp_nich-py-e3-B3  exact / merged       7.4 / 6.8    0.50
  gp_nich-py-e1-B6, dd_bb_gp-py-e1-B6    5.5, 5.4     0.79, 0.22
  bnb-py-e3-B3                           6.7          0.26
  dd-le6-e2-B6                           7.7          0.44
At 4 to 9 groups the value-sorted scan and the merged statistics led to the
exact mode's histogram.  dd-py-e3-B6: the oracle's same chain carried on to 10 000 and
20 000 states gives p = 0.28 and 0.41.  gp_nich-le10-e2-B3 took 12.8 s for
its 5 000 states, which is also its derived floor: it is left to the CPU
file, as is the leg of 7 rows.
"""
import functools
import time

import numpy as np
import pytest

import f64_posterior as fp
from test_f64_batch_posterior import BATCH_T, LEVEL
from test_gpu_posterior import make_engine

pytestmark = pytest.mark.gpu

VS, WAVE = "value_sorted", "wave"      # WAVE: k_rows_wave samples the batch
DD3, GN3 = ("dd", fp.PY, 3), ("gp_nich", fp.PY, 3)
# (case, B, options, the path every batch must take, followed by the oracle)
GPU_LEGS = [
    (DD3, 3, (("value_sorted", 0),), WAVE, True),
    (DD3, 3, (("value_sorted", 2),), VS, True),
    (DD3, 6, (("value_sorted", 0),), WAVE, True),
    (DD3, 6, (("value_sorted", 2),), VS, True),
    (DD3, 6, (("value_sorted", 2), ("sampling", 1)), VS, False),
    (("bb", fp.PY, 3), 4, (("value_sorted", 0),), WAVE, True),
    (("bb", fp.PY, 3), 4, (("value_sorted", 2),), VS, True),
    (("dd", fp.PY, 1), 6, (("value_sorted", 2),), VS, True),
    (("dpd", fp.PY, 1), 6, (("value_sorted", 2),), VS, True),
    (GN3, 3, (), WAVE, True),
    (GN3, 3, (("float_stats", 1),), WAVE, False),
    (("gp_nich", fp.PY, 1), 6, (), WAVE, True),
    (("dd_bb_gp", fp.PY, 1), 6, (), WAVE, True),
    (("bnb", fp.PY, 3), 3, (), WAVE, True),
    (("dd", ("le", 6), 2), 6, (), WAVE, True),
]
assert all((c, B) in fp.BATCH_LEGS for c, B, _, _, _ in GPU_LEGS)


def leg_id(g):
    case, B, options, _, _ = g
    return "-".join([fp.batch_id((case, B))] +
                    ["%s%d" % (k[:3] if k != "value_sorted" else "vs", v)
                     for k, v in options])


@functools.lru_cache(maxsize=None)
def reference(leg):
    """-> (model, T, expected counts of fp.batch_states(leg) states)"""
    m = fp.model(leg[0])
    P = m.batch_sweep_matrix(leg[1])
    T = fp.mixing_time(P, fp.stationary(P), 1e-4)
    assert T == BATCH_T[fp.batch_id(leg)]
    want = fp.law_sum(P, fp.start_state(m.space, "one"), T,
                      fp.batch_states(leg))
    want.setflags(write=False)
    return m, T, want


@functools.lru_cache(maxsize=None)
def oracle_states(leg):
    """the oracle's assignments at the sampling points of the leg"""
    _, T, _ = reference(leg)
    states, _ = fp.oracle_batch_chain(leg, "one", T, fp.batch_states(leg))
    states = states[T - 1::T]
    states.setflags(write=False)
    return states


@pytest.mark.parametrize("g", GPU_LEGS, ids=leg_id)
def test_batches_have_their_float64_law(g):
    case, B, options, path, followed = g
    leg = (case, B)
    m, T, want = reference(leg)
    n, samples, seed = m.n, fp.batch_states(leg), fp.batch_seed(leg)
    t0 = time.time()
    gpu = make_engine(case, "one", options)
    out = np.zeros((samples, n), np.uint32)
    sweeps = 0
    for s in range(samples):
        for _ in range(T):
            gpu.sweep(0, n, B, seed, draw_base=sweeps * n)
            sweeps += 1
        out[s] = gpu.assignments()
    seconds = time.time() - t0
    assert gpu.validate()["code"] == 0
    counts = gpu.core.debug_counts()
    assert counts["chain_launches"] == 0
    by_value, generic = gpu.path_counts()
    assert by_value + generic == sweeps * -(-n // B)
    if path == VS:
        assert by_value > 0 and generic == 0
    else:
        assert by_value == 0 and generic > 0
        assert counts["scratch_batches"] == 0      # k_rows_wave, see above
    opts = dict(options)
    assert counts["scan_batches"] == (by_value if opts.get("sampling") else 0)
    assert not opts.get("sampling") or path == VS  # the only scan in reach
    if opts.get("float_stats"):
        assert counts["merged_batches"] > 0
    chi2, dof, p, mass = fp.report(
        "%s T %d states %d (%.1f s)" % (leg_id(g), T, samples, seconds),
        want, m.space.histogram(out))
    if followed:
        theirs = oracle_states(leg)
        same = (out == theirs).all(1)
        assert same.all(), ("first sampling point that differs",
                            int(np.argmin(same)), out[np.argmin(same)],
                            theirs[np.argmin(same)])
    assert mass <= 0.05
    assert p > LEVEL, (chi2, dof, p)
