"""The certified search: k_vs_search, in k_vs_sample's place, answers a row's
inverse CDF by binary search on its value's float64 prefix sums where the
bound of csrc/vs_certify.h proves the float chain gives the same index, and
runs the chain itself on the rows that are left over.  Exact either way:
engines with the search off (0), forced (2) and at the default agree bit for
bit with each other and with the oracle after every sweep -- with the bound as
it is (slack 0), widened so that a good part of these small shapes' rows is
left over, and widened until nothing is certified (200: every row goes
through the kernel's chain phase)."""
import numpy as np
import pytest

import oracle_lib as ol
import workloads
from test_gpu_sweep import assert_same_state

pytestmark = pytest.mark.gpu

# the fused path with the cells' totals built whenever k_vs_tables runs
FUSED = {"value_sorted": 2, "value_stream": 0, "narrow_tiles": 0,
         "device_normalise": 2, "fused_tables": 1, "debug.shared_totals": 2}
# At K = 40 to 100 the proof's window is some K^2 2^-24 = 1e-4 to 6e-4 of a
# row's interval; 2^10 of it leaves roughly a tenth to a half of the rows over
# (tests/test_certified_search_cpu.py: 0.12 at K = 64, flat, slack 9).
SLACKS = [0, 10, 200]
MODES = (0, 2, 1)


def same_engines(a, b, what):
    np.testing.assert_array_equal(a.assignments(), b.assignments(),
                                  err_msg=what)
    np.testing.assert_array_equal(a.counts(), b.counts(), err_msg=what)


def run(workload, k, alpha, d, empty, batches, slack, start=0, base0=0):
    """One oracle and an engine per mode; after every sweep of rows
    [start, n) all of them agree.  -> the engines' debug counts by mode and
    the group counts after every sweep."""
    from distributions_amd import engine
    osh, gsh, vals, assign = workload
    n = len(assign)
    orc = ol.OracleMixture(alpha, d, osh)
    orc.init_from_assignments(vals, assign, k, empty)
    gpus = []
    for mode in MODES:
        gpu = engine.Gibbs(alpha, d, gsh)
        for name, value in FUSED.items():
            gpu.set_option(name, value)
        gpu.core.set_certified_search(mode, slack)
        gpu.load_rows(vals, assign, k, empty)
        gpus.append(gpu)
    seed = 7177
    st = ol.oracle().orc_rng_seed(seed)
    sizes = [len(orc)]
    for sweep, batch in enumerate(batches):
        base = base0 + sweep * n
        for b in range(start, n, batch):
            orc.gibbs_batch(b, min(n, b + batch), st, base)
        sizes.append(len(orc))
        for mode, gpu in zip(MODES, gpus):
            gpu.sweep(start, n, batch, seed, draw_base=base)
            what = "certified_search=%d slack=%d sweep %d" % (mode, slack,
                                                               sweep)
            assert gpu.validate()["code"] == 0, what
            assert_same_state(orc, gpu, what)
        same_engines(gpus[0], gpus[1], "0 against 2, sweep %d" % sweep)
        same_engines(gpus[0], gpus[2], "0 against default, sweep %d" % sweep)
    counts = {mode: gpu.core.debug_counts() for mode, gpu in zip(MODES, gpus)}
    check_paths(counts, slack)
    return counts, sizes


def check_paths(counts, slack):
    off, forced, auto = counts[0], counts[2], counts[1]
    assert off["fused_batches"] > 0
    assert off["search_batches"] == 0
    assert off["rows_certified"] == off["rows_left_over"] == 0
    for c in (forced, auto):
        assert c["fused_batches"] > 0
        assert 0 < c["search_batches"] <= c["fused_batches"]
        rows = c["rows_certified"] + c["rows_left_over"]
        share = c["rows_left_over"] / max(rows, 1)
        print("slack %d: %d rows certified, %d left over (%.3f)"
              % (slack, c["rows_certified"], c["rows_left_over"], share))
        assert rows > 0
        if slack == 0:
            assert c["rows_certified"] > 0 and share < 0.05
        elif slack == 200:
            # (a row whose draw is exactly 0 needs no bound)
            assert c["rows_left_over"] > 0 and share > 0.999
        else:
            assert c["rows_certified"] > 0 and c["rows_left_over"] > 0
    assert forced["rows_certified"] == auto["rows_certified"]
    assert forced["rows_left_over"] == auto["rows_left_over"]


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("config,dim,d", [
    ("dd", 16, 0.6), ("dd", 256, 0.6), ("dd", 16, 0.0), ("bb", None, 0.6)])
def test_group_churn(config, dim, d, slack):
    """60 groups of a hundred rows and a large alpha: groups of one row are
    founded in nearly every batch (their rows are handed over), vanish again
    and are swap-removed; the group count is no multiple of 32 and crosses
    one.  DD-16 (some 375 rows per value: chunks of three tiles), DD-256 (23
    rows per value), BetaBernoulli (two values, the larger past one chunk's
    5 120 rows at 7 000 rows); d = 0 too."""
    n = 7000 if config == "bb" else 6000
    _, sizes = run(workloads.make(config, n, 60, dim=dim), 60, 30.0, d, 4,
                   [1500, 1000, n, 700], slack)
    assert len({s // 32 for s in sizes}) > 1, sizes
    assert any(s % 32 for s in sizes), sizes


@pytest.mark.parametrize("slack", SLACKS)
def test_value_of_several_chunks(slack):
    """Two values, 24 000 rows: each value's rows span three apply chunks,
    the last a partial one; 80 groups."""
    n = 24000
    run(workloads.make("dd", n, 80, dim=2, seed=11), 80, 25.0, 0.5, 2,
        [n, 12000], slack)


@pytest.mark.parametrize("slack", [10, 200])
def test_chunk_sizes_row_offset_and_draw_base(slack):
    """Chunks of 1, 2, 127, 128 and 129 rows (the chain phase's 64-row trips
    end inside a trip, at its end, and one row into the next) beside ordinary
    ones; the
    sweeps cover rows [1000, n) only and start from a draw base that is not
    zero, so positions, rows and draws are three different numbers."""
    n, k, dim = 7000, 50, 16
    osh, gsh, vals, assign = workloads.make("dd", n, k, dim=dim)
    v = vals[0].copy()
    rng = np.random.default_rng(3)
    swept = np.arange(1000, n)
    rng.shuffle(swept)
    v[swept] = 5 + (np.arange(len(swept)) % (dim - 5))
    at = 0
    for value, rows in enumerate([1, 2, 127, 128, 129]):
        v[swept[at:at + rows]] = value
        at += rows
    run((osh, gsh, [v.astype(np.uint32)], assign), k, 20.0, 0.4, 2,
        [n - 1000, 2500], slack, start=1000, base0=123457)
