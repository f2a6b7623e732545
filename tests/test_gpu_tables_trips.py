"""k_vs_tables lays its LDS out by the launch's own bound on the group count,
reads the logarithm's and the exponential's tables from copies in LDS where
they fit beside the strips (a launch bound of up to some 4 800 groups; the
global tables beyond), and leaves the band section to its last wave, beside
the fold.  Loads move and a table changes its place: no float operation
changes, so every case is bit-exact against the oracle after every sweep,
with validate() clean; the cases also walk k_vs_apply's sort and
k_vs_reduce's pass over values of several chunks, which follow it."""
import pytest

import oracle_lib as ol
import workloads
from test_gpu_sweep import assert_same_state

pytestmark = pytest.mark.gpu

# the fused path (k_vs_tables, k_vs_apply's sorting form, k_vs_reduce) with
# the totals folded whenever the tables run
FUSED = {"value_sorted": 2, "value_stream": 0, "narrow_tiles": 0,
         "device_normalise": 2, "fused_tables": 1, "debug.shared_totals": 2}
# ... and band tiles on launches this small
BANDED = dict(FUSED, **{"debug.running_sums_min_tiles": 0})


def group_ids(orc):
    """-> {global id of a group: its packed index}"""
    return {orc.packed_to_global(k): k for k in range(len(orc))}


def run_chain(config, dim, n, k, alpha, d, empty, batches, options,
              seed=7177, wl_seed=workloads.SEED, upto=None):
    """One oracle, one engine; after every sweep (of the first `upto` rows;
    None: of all) the engine validates and equals the oracle.  -> the engine's debug counts, and what the oracle's
    batches did to the group set: {"appended", "vanished", "moved"} (groups
    with a new id; ids that are gone; surviving groups under another packed
    index, as a swap-removal leaves them)."""
    from distributions_amd import engine
    osh, gsh, vals, assign = workloads.make(config, n, k, seed=wl_seed,
                                            dim=dim)
    orc = ol.OracleMixture(alpha, d, osh)
    orc.init_from_assignments(vals, assign, k, empty)
    gpu = engine.Gibbs(alpha, d, gsh)
    for name, value in options.items():
        gpu.set_option(name, value)
    gpu.load_rows(vals, assign, k, empty)
    st = ol.oracle().orc_rng_seed(seed)
    churn = set()
    end = upto or n
    for sweep, batch in enumerate(batches):
        base = 1000 + sweep * n
        for b in range(0, end, batch):
            before = group_ids(orc)
            orc.gibbs_batch(b, min(end, b + batch), st, base)
            after = group_ids(orc)
            if after.keys() - before.keys():
                churn.add("appended")
            if before.keys() - after.keys():
                churn.add("vanished")
            if any(after[g] != k for g, k in before.items() if g in after):
                churn.add("moved")
        gpu.sweep(0, end, batch, seed, draw_base=base)
        what = "%s-%s k=%d sweep %d" % (config, dim, k, sweep)
        assert gpu.validate()["code"] == 0, what
        assert_same_state(orc, gpu, what)
    return gpu.core.debug_counts(), churn


ALL_CHURN = {"appended", "vanished", "moved"}


@pytest.mark.parametrize("config,dim,k", [
    ("dd", 16, 48), ("dd", 256, 130), ("bb", None, 48), ("gp", None, 48),
    ("bnb", None, 48)])
def test_kinds(config, dim, k):
    """DD-16, DD-256 with more groups than one fold window (128) holds,
    and the scalar kinds: BetaBernoulli and BetaNegativeBinomial run
    k_vs_tables with a scorer_init that keeps to the global tables;
    GammaPoisson's batches never take the fused launch (below), so its case
    covers k_vs_reduce alone and no instance of k_vs_tables.  Sub-sweeps of
    4 000 of 20 000 rows, four sweeps.  A large alpha appends groups of one
    row in nearly every batch and they vanish again, most of them from the
    middle of the group set: the plan, src_of, and the own slots over the
    plan's counts."""
    counts, churn = run_chain(config, dim, 20000, k, 30.0, 0.6, 4,
                              [4000, 4000, 4000, 4000], FUSED)
    assert churn == ALL_CHURN
    # (GammaPoisson's log-product is a float statistic: its batches do not
    # take the fused launch, and come here through k_vs_reduce only)
    assert (counts["fused_batches"] > 0) == (config != "gp")


@pytest.mark.parametrize("config,dim", [("dd_skew", 24), ("dd", 16)])
@pytest.mark.parametrize("d", [0.6, 0.0])
def test_bands(config, dim, d):
    """Bands on small launches: the band section runs in every fused launch,
    and the group set moves (swap-removals) in nearly every batch, so a
    launch reads offsets that a sort left under an older epoch, through this
    batch's plan and the log of moves.  band_mode / band_tile decide which
    rows a band tile and which the regular tiles sample: a wrong band shows
    in the assignments."""
    counts, churn = run_chain(config, dim, 6000, 900, 30.0, d, 4,
                              [1500, 1000, 6000, 700], BANDED)
    assert churn == ALL_CHURN
    assert counts["fused_batches"] > 0
    assert counts["band_launches"] > 0


@pytest.mark.parametrize("k,first", [(900, 4000), (5400, 1500)])
def test_both_table_sources(k, first):
    """900 groups: the tables' copies fit behind the strips.  5 400 groups,
    two or three rows each: the launch's bound is past what leaves room for
    them (some 4 800 groups) and the same instantiation reads the global
    tables -- for the first six launches, the sixth with some 450 groups to
    swap-remove; then the group count has sunk below the bound and the chain
    goes on with the copies."""
    counts, churn = run_chain("dd", 16, 12000, k, 1.0, 0.2, 1,
                              [first, 12000], BANDED)
    assert churn == ALL_CHURN
    assert counts["fused_batches"] > 0


def test_global_tables_alone():
    """5 400 groups again, and only the first four batches of 1 500 rows:
    no group has lost all its rows yet, the group count is 5 401 to 5 404 at
    every launch, so every fused batch the counter reports had a bound past
    the 4 832 groups that leave room for the copies and read the global
    tables."""
    counts, _ = run_chain("dd", 16, 12000, 5400, 1.0, 0.2, 1, [1500],
                          BANDED, upto=6000)
    assert counts["fused_batches"] > 0


def test_value_of_several_chunks():
    """Two values, 30 000 rows: each value's rows span three apply chunks
    of 5 120 (the band section's loop over a value's chunks, the cells
    k_vs_apply leaves to k_vs_reduce's pass over such values)."""
    n = 30000
    counts, churn = run_chain("dd", 2, n, 700, 25.0, 0.5, 2, [n, 15000, n],
                              BANDED, seed=777, wl_seed=11)
    # (groups of forty rows do not vanish; the appended ones hold the rows
    # alone in their group, which the chunks are handed)
    assert "appended" in churn
    assert counts["fused_batches"] > 0
    assert counts["band_launches"] > 0


def test_last_wave_folds_after_the_bands():
    """2 100 groups: seventeen fold jobs, so the last wave has one of its
    own behind the band section."""
    counts, _ = run_chain("dd", 16, 12000, 2100, 1.0, 0.2, 1, [4000, 12000],
                          BANDED)
    assert counts["fused_batches"] > 0
    assert counts["band_launches"] > 0
