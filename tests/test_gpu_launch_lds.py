"""The host launch layer: every kernel instance that takes more than 64 KiB of
dynamic LDS opts in through one helper (launch_lds, dist_hip.hip), sized by
the kernel's own size function (kernels*.h), and dist_gibbs_set_option reads
one table.  The engines here sit at the group counts where a launch crosses
64 KiB or changes form, and are held to the oracle bit for bit.

The sizes, from the constants of kernels_vs.h / kernels_apply.h /
kernels_api.h (kVsApplyBlock 1024, kVsApplyRows 5120, the 144 KiB limit):

  vs_apply_sort_lds(k)  = (2 k + 1024 / 64 + 4 * 5120 + 4) * 4
                        = 8 k + 82 000 bytes: ABOVE 64 KiB at every k, so the
      sorting k_vs_apply opts in on its first launch whatever the group
      count, and again whenever a later engine has more groups.  It stops
      fitting the workgroup limit at the first k with 8 k + 82 000 >
      147 456, k = 8183: from there the plain form runs.
  vs_apply_plain_lds(k) = 4 k: past 64 KiB from k = 16 385.
  normalise_lds(k)      = 4 (k + 2) + 8 (k / 2 + 1): past 64 KiB from 8191.
  apply_moves_stage_lds = 4 bytes per statistic word, (3 + dim) words per
      group and feature list of one DD: dim = 4, past 64 KiB from k = 2341.
  cs_scatter_lds(keys)  = 5 * 4 * keys, keys = k + 1: past 64 KiB from
      k = 3276 (float statistics only: GammaPoisson here).
  vs_tables_lds(Kpad)   = (4 Kpad + 2) * 4: tests/test_gpu_shared_totals.py at
      k = 4200.
  merge_float_lds(words) = 8 bytes per word, one word per group of a
      GammaPoisson feature: past 64 KiB from K() = 8193.
  k_vs_apply_mixed takes vs_apply_plain_lds: past 64 KiB from k = 16 385.
  chains_lds(room)      = 8 bytes per slot, at most 64 KiB by chain_fits: the
      exact chain (k_chains) never passes 64 KiB of dynamic LDS; its launch
      keeps its own form, run by tests/test_gpu_chains.py.

The engine's group count K() is the k non-empty groups plus `empty`.
"""
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import workloads
from test_gpu_sweep import assert_same_state

pytestmark = pytest.mark.gpu

KIB = 1024
APPLY_BLOCK, APPLY_ROWS, WORKGROUP_LIMIT = 1024, 5120, 144 * KIB


def vs_apply_sort_lds(k):
    return (2 * k + APPLY_BLOCK // 64 + 4 * APPLY_ROWS + 4) * 4


def first_k(size, above):
    k = 0
    while size(k) <= above:
        k += 1
    return k


def one_sweep(config, k, options, rows_per_group=2, dim=4, empty=1):
    """One sub-sweep of all rows against the oracle -> the engine's counts"""
    from distributions_amd import engine
    n = rows_per_group * k
    osh, gsh, vals, assign = workloads.make(config, n, k, dim=dim)
    orc = ol.OracleMixture(1.0, 0.2, osh)
    orc.init_from_assignments(vals, assign, k, empty)
    gpu = engine.Gibbs(1.0, 0.2, gsh)
    for name, value in options.items():
        gpu.set_option(name, value)
    gpu.load_rows(vals, assign, k, empty)
    seed = 4242
    st = ol.oracle().orc_rng_seed(seed)
    orc.gibbs_batch(0, n, st, 0)
    gpu.sweep(0, n, n, seed, draw_base=0)
    what = "%s k=%d %r" % (config, k, options)
    assert len(gpu) == len(orc), what
    np.testing.assert_array_equal(gpu.assignments(), orc.assign, err_msg=what)
    np.testing.assert_array_equal(gpu.counts(), orc.counts(), err_msg=what)
    return gpu, orc, gpu.core.debug_counts()


def test_sizes_as_the_docstring_states_them():
    assert vs_apply_sort_lds(0) > 64 * KIB
    assert first_k(vs_apply_sort_lds, WORKGROUP_LIMIT) == 8183


@pytest.mark.parametrize("order", [("dd", "bb"), ("bb", "dd")])
def test_raise_only_per_instance(order):
    """Engines in ONE process through the sorting k_vs_apply with growing
    group counts -- every step asks for more LDS than the instance was raised
    to -- then a small one again (nothing is lowered: the larger ones still
    run after it).  The second kind's instance starts from nothing of its
    own: it must not inherit the first's.  (First in this file: no test
    before it here has raised either instance to its limit.)"""
    for config in order:
        for k in (64, 4000, 4400, 64, 4400):
            _, _, counts = one_sweep(config, k, {"value_sorted": 2})
            assert counts["value_sorted_batches"] >= 1


@pytest.mark.parametrize("k", [first_k(vs_apply_sort_lds, WORKGROUP_LIMIT) - 40,
                               first_k(vs_apply_sort_lds, WORKGROUP_LIMIT) + 8])
def test_sorting_apply_up_to_the_workgroup_limit_and_past_it(k):
    """The sorting k_vs_apply at the most LDS it ever takes (the engine's
    bound on the group count includes its empty groups: a few short of
    8183), and the plain form just past it."""
    _, _, counts = one_sweep("dd", k, {"value_sorted": 2})
    assert counts["value_sorted_batches"] >= 1
    assert counts["other_batches"] == 0


def test_plain_apply_and_normalise_past_64k():
    """16 400 groups: k_vs_apply's plain form (4 K bytes) and k_normalise of
    the device-normalised run both opt in."""
    k = first_k(lambda k: 4 * k, 64 * KIB) + 15
    _, _, counts = one_sweep("dd", k, {"value_sorted": 2,
                                       "device_normalise": 1})
    assert counts["value_sorted_batches"] >= 1
    assert counts["device_normalised"] >= 1


def test_staged_apply_past_64k():
    """General rows, the whole integer image in LDS (k_apply_moves_stage):
    7 words per group at dim = 4.  The staged form is taken when
    debug.apply_stage is set, the image fits 144 KiB, a feature is categorical
    and the batch has n >= 4 K() rows: five rows per group give
    n = 5 k >= 4 (k + 1).  (With fewer rows the batch would take
    k_apply_moves, whose result is the same.)"""
    k = first_k(lambda k: 4 * (7 * (k + 1)), 64 * KIB)
    rows_per_group, empty = 5, 1
    assert 4 * 7 * (k + empty) > 64 * KIB
    assert 4 * 7 * (k + empty) <= WORKGROUP_LIMIT
    assert rows_per_group * k >= 4 * (k + empty)
    _, _, counts = one_sweep("dd", k, {"value_sorted": 0,
                                       "debug.apply_stage": 1},
                             rows_per_group=rows_per_group, empty=empty)
    assert counts["value_sorted_batches"] == 0
    assert counts["other_batches"] >= 1


def test_merged_float_sums_past_64k():
    """float_stats = 1: k_merge_float_moves keeps one binary64 per group of a
    GammaPoisson feature in LDS, 8 K() bytes.  One sub-sweep from the
    oracle's state makes the oracle's moves; the merged log-products are
    held to binary32 rounding elsewhere (tests/test_gpu_scan.py)."""
    k = first_k(lambda k: 8 * (k + 1), 64 * KIB) + 7
    assert 8 * (k + 1) <= WORKGROUP_LIMIT
    _, _, counts = one_sweep("gp", k, {"value_sorted": 0, "float_stats": 1},
                             rows_per_group=4)
    assert counts["merged_batches"] == 1


def test_mixed_chunks_apply_past_64k():
    """k_vs_apply_mixed: with the table-free kernel forced (value_stream = 2)
    a categorical value with at most 5120 / 2 rows shares its apply chunk
    with its neighbours.  dim = 16 and two rows per group: 2 k / 16 = 2050
    rows per value, two values per chunk; the chunks' LDS is 4 K() bytes."""
    k = first_k(lambda k: 4 * (k + 1), 64 * KIB) + 16
    assert 2 * k // 16 <= APPLY_ROWS // 2
    _, _, counts = one_sweep("dd", k, {"value_sorted": 2, "value_stream": 2},
                             dim=16)
    assert counts["stream_batches"] >= 1
    assert counts["other_batches"] == 0


def test_counting_sort_scatter_past_64k():
    """GammaPoisson's ordered replay: k_cs_scatter keeps five rows of
    (groups + 1) counters."""
    k = first_k(lambda k: 20 * (k + 1), 64 * KIB) + 4
    gpu, orc, _ = one_sweep("gp", k, {"value_sorted": 0}, rows_per_group=4)
    for g in (0, 1, len(orc) - 1):
        np.testing.assert_array_equal(gpu.get_group(0, g), orc.get_group(0, g))


# ---- options ---------------------------------------------------------------
def documented_options():
    """-> [(name as the caller spells it)] from the header's comment"""
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include",
                             "distributions_hip.h")).read()
    block = text[text.index("/* Options."):
                 text.index("int dist_gibbs_set_option(")]
    return re.findall(r'^ \*  "([a-z_.]+)"', block, flags=re.M)


def table_options():
    """-> the names of the library's table (kGibbsOptions), hooks spelled
    with their prefix, read from the source"""
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "distributions_amd", "csrc",
                             "dist_hip.hip")).read()
    block = text[text.index("kGibbsOptions[] = {"):]
    block = block[:block.index("\n};")]
    rows = re.findall(r'\{"([a-z_]+)", (true|false),', block)
    return [("debug." if hook == "true" else "") + name
            for name, hook in rows]


# default, a value one step below the accepted ones, one step above
# (None: no such bound)
EXPECT = {
    "value_sorted": (1, -1, 3), "value_stream": (1, -1, 3),
    "narrow_tiles": (1, -1, 3), "device_normalise": (2, -1, 3),
    "sharded_device_normalise": (1, -1, 2), "fused_tables": (1, -1, 2),
    "kernel_timing": (1, -1, None), "phase_timing": (0, -1, 2),
    "float_stats": (0, -1, 2), "sampling": (0, -1, 2),
    "debug.sequential_chain": (2, -1, 3),
    "debug.running_sums_min_tiles": (2048, -1, None),
    "debug.narrow_read_ahead": (0, -1, 9), "debug.stream_scratch": (1, -1, 2),
    "debug.rows_scratch": (3, -1, 4), "debug.rows_scratch_lds_log": (1, -1, 2),
    "debug.rows_scratch_block": (512, 0, 1088), "debug.rows_fold": (1, -1, 3),
    "debug.apply_stage": (1, -1, 2), "debug.program_all": (1, -1, 2),
    "debug.sample_prio": (0x13210, -1, 0x20000),
    "debug.rows_prio": (0x13210, -1, 0x20000),
    "debug.apply_overlap": (1, -1, 2), "debug.run_batches_cap": (0, -1, None),
    "debug.shared_totals": (1, -1, 3), "debug.score_rows_chunk": (1 << 30, 0, None),
    "debug.predict_chunk": (1 << 22, 0, None),
}
# inside the range, outside the set
ODD = {"debug.narrow_read_ahead": (2, 6), "debug.rows_scratch": (1, 2),
       "debug.rows_scratch_block": (65, 500), "debug.sample_prio": (1, 0xffff),
       "debug.rows_prio": (1, 0xffff)}


def test_options_table_and_header_agree():
    from distributions_amd import engine
    names = documented_options()
    assert sorted(names) == sorted(table_options()), "header vs table"
    assert sorted(names) == sorted(EXPECT), "header comment vs this test"
    gpu = engine.Gibbs(1.0, 0.2, [engine.dd_shared([0.5] * 4)])

    def refused(name, value, word):
        with pytest.raises(Exception) as err:
            gpu.set_option(name, value)
        assert word in str(err.value), (name, value, str(err.value))

    for name in names:
        default, below, above = EXPECT[name]
        bare = name[6:] if name.startswith("debug.") else name
        gpu.set_option(name, default)
        refused(name, below, bare + ":")
        if above is not None:
            refused(name, above, bare + ":")
        for value in ODD.get(name, ()):
            refused(name, value, bare + ":")
        if name.startswith("debug."):
            refused(bare, default, "spell it debug." + bare)
        else:
            refused("debug." + name, default, "unknown option")
    refused("no_such_option", 0, "unknown option")
    refused("debug.no_such_option", 0, "unknown option")
