"""The row set-up of k_vs_sample / k_vs_narrow issues both rows' loads in
stages (positions -> group and draw-table words -> own likelihood and total),
lanes without a row and rows the tile skips loading from clamped in-range
indices, and the value's words (K among them) come by scalar loads.  No float
operation of any row changes, so every case here is bit-exact against the
oracle after every sweep: tiles of 1, 2, odd and 128 rows, rows alone in their
group in either slot of a lane, mixed-class and band tiles, draw indices past
one and two 4 096-blocks of the power tables, every path of the set-up, and
the benchmark's shape (the 512-thread instantiation at full occupancy)."""
import numpy as np
import pytest

import oracle_lib as ol
import workloads
from test_gpu_sweep import assert_same_state

pytestmark = pytest.mark.gpu

FUSED = {"value_sorted": 2, "value_stream": 0, "narrow_tiles": 0,
         "device_normalise": 1, "fused_tables": 1}
# the same with what large launches get: a band tile per apply chunk for the
# rows of the value's arg-max group, the regular tiles skipping those rows
BANDED = dict(FUSED, **{"debug.running_sums_min_tiles": 0})


def make_engine(gsh, vals, assign, k, empty, alpha, d, options,
                row_offset=0):
    from distributions_amd import engine
    gpu = engine.Gibbs(alpha, d, gsh)
    for name, value in options.items():
        gpu.set_option(name, value)
    gpu.load_rows(vals, assign, k, empty, row_offset=row_offset)
    return gpu


def assert_same_engines(a, b, what):
    np.testing.assert_array_equal(a.assignments(), b.assignments(),
                                  err_msg=what)
    np.testing.assert_array_equal(a.counts(), b.counts(), err_msg=what)


def run_sweeps(config, dim, n, k, alpha, d, empty, batches, variants,
               seed=7177, row_offsets=None):
    """One oracle, one engine per entry of `variants` (option dicts); after
    every sweep each engine equals the oracle and the engines one another.
    -> group counts after each sweep, and whether a batch met a group of
    size 1 at its entry (the oracle's sizes)."""
    osh, gsh, vals, assign = workloads.make(config, n, k, dim=dim)
    row_offsets = row_offsets or [0] * len(variants)
    assert len(set(row_offsets)) == 1, "one oracle follows one draw sequence"
    offset = row_offsets[0]
    orc = ol.OracleMixture(alpha, d, osh)
    orc.init_from_assignments(vals, assign, k, empty)
    gpus = [make_engine(gsh, vals, assign, k, empty, alpha, d, opts, offset)
            for opts in variants]
    st = ol.oracle().orc_rng_seed(seed)
    sizes, met_single = [], False
    for sweep, batch in enumerate(batches):
        base = 1000 + sweep * n   # (never 0)
        for b in range(0, n, batch):
            met_single = met_single or bool(
                (np.asarray(orc.counts())[:len(orc)] == 1).any())
            # row i draws with engine step base + offset + i + 1
            orc.gibbs_batch(b, min(n, b + batch), st, base + offset)
        sizes.append(len(orc))
        for gpu in gpus:
            gpu.sweep(0, n, batch, seed, draw_base=base)
        what = "%s-%s d=%g sweep %d" % (config, dim, d, sweep)
        for gpu in gpus[1:]:
            assert_same_engines(gpus[0], gpu, what)
        for i, gpu in enumerate(gpus):
            assert_same_state(orc, gpu, "%s engine %d" % (what, i))
    return sizes, met_single, gpus


@pytest.mark.parametrize("config,dim", [("dd_skew", 24), ("dd", 16)])
@pytest.mark.parametrize("d", [0.6, 0.0])
def test_tile_shapes(config, dim, d):
    """Skewed values: tiles of 1, 2, odd and 128 rows (a lane's second row
    missing while its first is there), rows alone in their group in either
    slot of a lane, mixed-class tiles and -- on the second engine -- band
    tiles; the group count moves (swap-removals) in nearly every batch."""
    sizes, met_single, gpus = run_sweeps(
        config, dim, 6000, 900, 30.0, d, 4, [1500, 1000, 6000, 700],
        [FUSED, BANDED])
    assert len(set(sizes)) > 1
    assert met_single
    for gpu in gpus:
        assert gpu.core.debug_counts()["fused_batches"] > 0
    # (launches this small get band tiles -- and with them the tiles that
    # skip a band's rows -- only when asked to)
    assert gpus[0].core.debug_counts()["band_launches"] == 0
    assert gpus[1].core.debug_counts()["band_launches"] > 0


def test_draw_indices():
    """Batch ranges that begin off a multiple of 4 096 and run past it (the
    high power table's entries 1 and 2), a draw base that is not zero, and a
    second run whose rows sit at a global offset."""
    for offset in (0, 123457):
        _, _, gpus = run_sweeps("dd", 16, 12000, 1100, 1.0, 0.2, 1,
                                [5000, 12000], [FUSED],
                                row_offsets=[offset])
        assert gpus[0].core.debug_counts()["fused_batches"] > 0


def test_paths():
    """The first tile-shape case through every path of the set-up: totals
    per row (shared_totals 0) and shared whenever the tables run (2), the
    unfused ladder (fused_tables 0: counts and the own score per row), and
    the one-row-per-lane tiles (narrow_tiles 2)."""
    variants = [
        dict(FUSED, **{"debug.shared_totals": 0}),
        dict(FUSED, **{"debug.shared_totals": 2}),
        dict(FUSED, fused_tables=0),
        dict(FUSED, narrow_tiles=2),
    ]
    sizes, met_single, gpus = run_sweeps(
        "dd_skew", 24, 6000, 900, 30.0, 0.6, 4, [1500, 1000, 6000, 700],
        variants)
    assert len(set(sizes)) > 1
    assert met_single
    for i in (0, 1, 3):
        assert gpus[i].core.debug_counts()["fused_batches"] > 0
    assert gpus[2].core.debug_counts()["fused_batches"] == 0
    # (k_vs_narrow took every batch of the last engine, none of the others)
    counts = [gpu.core.debug_counts() for gpu in gpus]
    assert counts[3]["narrow_batches"] == counts[3]["value_sorted_batches"] > 0
    for i in (0, 1, 2):
        assert counts[i]["narrow_batches"] == 0


def test_benchmark_shape():
    """DD-256, 10^6-row batches: one sweep of 2 x 10^6 rows, then the oracle
    adopts the state and follows one sub-sweep."""
    n, k, batch = 2_000_000, 1024, 1_000_000
    alpha, d = 1.0, 0.2
    seed = 20240601
    osh, gsh, vals, assign = workloads.make("dd", n, k, dim=256)
    gpu = make_engine(gsh, vals, assign, k, 1, alpha, d, FUSED)
    gpu.sweep(0, n, batch, seed, draw_base=0)
    assert gpu.core.debug_counts()["fused_batches"] > 0
    orc = ol.OracleMixture(alpha, d, osh)
    orc.init_from_assignments(vals, assign, k, 1)
    orc.adopt(gpu, vals)
    st = ol.oracle().orc_rng_seed(seed)
    orc.gibbs_batch(0, batch, st, n)
    gpu.sweep(0, batch, batch, seed, draw_base=n)
    assert_same_state(orc, gpu, "sub-sweep after one sweep")
