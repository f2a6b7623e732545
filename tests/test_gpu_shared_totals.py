"""debug.shared_totals: k_vs_tables folds every (value, group) cell's sampling
total once and the value tiles start their scan from it (1, the default:
where the library chooses; 2: whenever k_vs_tables runs), or each tile folds
the total per row as before (0).  The fold is the same float operations in
the same order, so every setting samples every row alike: two engines from
the same state and seed agree bit for bit, and both agree with the oracle."""
import numpy as np
import pytest

import oracle_lib as ol
import workloads
from test_gpu_sweep import assert_same_state

pytestmark = pytest.mark.gpu


def engines(config, n, k, alpha, d, empty, dim=None, modes=(0, 2)):
    """-> oracle, one engine per shared_totals mode, values; every engine on
    the fused value-sorted path (k_vs_tables, the 128-row tiles)"""
    from distributions_amd import engine
    osh, gsh, vals, assign = workloads.make(config, n, k, dim=dim)
    orc = ol.OracleMixture(alpha, d, osh)
    orc.init_from_assignments(vals, assign, k, empty)
    out = []
    for mode in modes:
        gpu = engine.Gibbs(alpha, d, gsh)
        gpu.set_option("value_sorted", 2)
        gpu.set_option("value_stream", 0)
        gpu.set_option("narrow_tiles", 0)
        gpu.set_option("device_normalise", 1)
        gpu.set_option("fused_tables", 1)
        gpu.set_option("debug.shared_totals", mode)
        gpu.load_rows(vals, assign, k, empty)
        out.append(gpu)
    return orc, out, vals


def assert_same_engines(a, b, what):
    np.testing.assert_array_equal(a.assignments(), b.assignments(),
                                  err_msg=what)
    np.testing.assert_array_equal(a.counts(), b.counts(), err_msg=what)


def run_sweeps(config, n, k, alpha, d, empty, batches, dim=None):
    orc, gpus, _ = engines(config, n, k, alpha, d, empty, dim=dim)
    seed = 7177
    st = ol.oracle().orc_rng_seed(seed)
    sizes = []
    for sweep, batch in enumerate(batches):
        for b in range(0, n, batch):
            orc.gibbs_batch(b, min(n, b + batch), st, sweep * n)
        sizes.append(len(orc))
        for gpu in gpus:
            gpu.sweep(0, n, batch, seed, draw_base=sweep * n)
        what = "%s sweep %d" % (config, sweep)
        assert_same_engines(gpus[0], gpus[1], what)
        for gpu in gpus:
            assert_same_state(orc, gpu, what)
    for gpu in gpus:
        assert gpu.core.debug_counts()["fused_batches"] > 0
    return sizes


@pytest.mark.parametrize("config,dim", [("dd", 16), ("dd_skew", 24),
                                        ("bb", None), ("dd", 256)])
@pytest.mark.parametrize("d", [0.6, 0.0])
def test_group_churn(config, dim, d):
    """Many small groups and a large alpha: groups are swap-removed (the
    tables' removal plan) and filled in nearly every batch, rows alone in
    their group are handed over, and tiles hold rows of their value's
    arg-max group next to others (both classes in one tile)."""
    sizes = run_sweeps(config, 6000, 900, 30.0, d, 4,
                       [1500, 1000, 6000, 700], dim=dim)
    assert len(set(sizes)) > 1


@pytest.mark.parametrize("k", [1100, 2100, 4200])
def test_group_counts_past_one_round(k):
    """Group counts past one group per thread of k_vs_tables (1024), past
    two, and past what one round of its waves folds (16 jobs of 256 groups):
    the strided layouts of the tables and the totals' second round."""
    run_sweeps("dd", 12000, k, 1.0, 0.2, 1, [4000, 12000], dim=16)


@pytest.mark.parametrize("config", ["dd", "dd_zipf"])
def test_full_batches_dd256(config):
    """DD-256, 10^6-row batches (the benchmark's shape, uniform and Zipf
    values): two whole sweeps through the default (totals shared) and
    through the per-row totals agree bit for bit; the oracle then adopts
    the state and follows the next sub-sweep of both."""
    n, k, batch = 2_000_000, 1024, 1_000_000
    alpha, d = 1.0, 0.2
    orc, gpus, vals = engines(config, n, k, alpha, d, 1, dim=256,
                              modes=(0, 1))
    seed = 20240601
    for sweep in range(2):
        for gpu in gpus:
            gpu.sweep(0, n, batch, seed, draw_base=sweep * n)
        assert_same_engines(gpus[0], gpus[1], "%s sweep %d" % (config, sweep))
    for gpu in gpus:
        assert gpu.core.debug_counts()["fused_batches"] > 0
    orc.adopt(gpus[0], vals)
    assert_same_state(orc, gpus[1], "%s adopted state" % config)
    st = ol.oracle().orc_rng_seed(seed)
    orc.gibbs_batch(0, batch, st, 2 * n)
    for gpu in gpus:
        gpu.sweep(0, batch, batch, seed, draw_base=2 * n)
        assert_same_state(orc, gpu, "%s sub-sweep after two sweeps" % config)
