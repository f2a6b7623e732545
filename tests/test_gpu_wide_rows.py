"""General rows of four to eight features against the oracle, bit for bit
(tests/wide_rows.py builds the lists).  Only a list longer than three
features reaches these parts of the general-row kernels: a fold of three to
seven leading ops with ops left over (launch_rows_scratch moves the remaining
ops to the front and numbers their gtab slots afterwards; k_fold_codes /
k_rows_fold stride over every folded digit), each compile-time instance of
k_rows_scratch behind such a fold, the rolled generic instance with up to
five ops (the row's values picked from eight registers by the op index), and
a ScoreProgram of sixteen ops in k_sweep_program.  Every test asserts, from
the engine's diagnostics, which kernel, fold depth and instance it ran."""
import numpy as np
import pytest

import oracle_lib as ol
import wide_rows
from test_gpu_sweep import assert_same_state

pytestmark = pytest.mark.gpu

N = 6000
BATCH = 3000
SEED = 4242


def engine_for(name, n, k, options, alpha=1.0, d=0.2, empty=1,
               dataset_size=None):
    from distributions_amd import engine
    _, gsh, vals, assign = wide_rows.make(name, n, k)
    gpu = (engine.Gibbs(alpha, d, gsh) if dataset_size is None
           else engine.Gibbs(alpha, d, gsh, dataset_size=dataset_size))
    for key, value in options.items():
        gpu.set_option(key, value)
    gpu.load_rows(vals, assign, k, empty)
    return gpu


def assert_launch(counts, name, fold):
    """the diagnostics of the last k_rows_scratch launch against the table of
    wide_rows.EXPECT (fold 2) or an unfolded launch (fold 0)"""
    folded, instance, hands_over = wide_rows.EXPECT[name]
    if fold:
        assert counts["rows_folded_last"] == folded, counts
        assert counts["rows_instance_last"] == instance, counts
        assert counts["fold_batches"] == (
            counts["scratch_batches"] if folded else 0), counts
    else:
        assert counts["rows_folded_last"] == 0, counts
        assert counts["fold_batches"] == 0, counts
    # (the other lists hand a row over only where it is alone in its group)
    if hands_over:
        assert counts["handed_over_last"] > 0, counts


@pytest.mark.parametrize("name", wide_rows.NAMES)
@pytest.mark.parametrize("fold,lds_log,block", [(2, 1, 256), (2, 0, 64),
                                                (0, 1, 512)])
@pytest.mark.parametrize("k", [31, 40])
def test_wide_rows_scratch_kernel_bit_exact(name, fold, lds_log, block, k):
    """k_rows_scratch on every list, group counts on either side of the
    blocks of 8 groups and of kRowsSuper = 32: folded as deep as batches of
    3000 rows allow (every instance behind a fold of two ops or more, the
    generic one with 0, 3, 4 and 5 ops left) and unfolded (the generic
    instance with up to eight ops)."""
    gpu = engine_for(name, N, k, {
        "value_sorted": 0, "debug.rows_scratch": 3,
        "debug.rows_scratch_lds_log": lds_log,
        "debug.rows_scratch_block": block, "debug.rows_fold": fold})
    for sweep, orc in enumerate(wide_rows.oracle_sweeps(name, N, k, BATCH,
                                                        SEED)):
        gpu.sweep(0, N, BATCH, SEED, draw_base=sweep * N)
        assert_same_state(orc, gpu, "%s K=%d fold %d sweep %d" % (
            name, k, fold, sweep))
    counts = gpu.core.debug_counts()
    assert counts["scratch_batches"] == 4, counts
    assert_launch(counts, name, fold)


@pytest.mark.parametrize("name", wide_rows.NAMES)
def test_wide_rows_program_kernel_bit_exact(name):
    """k_sweep_program: a ScoreProgram of up to sixteen ops (cats8)"""
    k = 31
    gpu = engine_for(name, N, k, {"value_sorted": 0, "debug.rows_scratch": 0})
    for sweep, orc in enumerate(wide_rows.oracle_sweeps(name, N, k, BATCH,
                                                        SEED)):
        gpu.sweep(0, N, BATCH, SEED, draw_base=sweep * N)
        assert_same_state(orc, gpu, "%s program sweep %d" % (name, sweep))
    counts = gpu.core.debug_counts()
    assert counts["scratch_batches"] == 0, counts
    assert counts["fold_batches"] == 0, counts
    assert counts["rows_folded_last"] == 0, counts
    if wide_rows.EXPECT[name][2]:
        assert counts["handed_over_last"] > 0, counts


@pytest.mark.parametrize("name,n", [("defaults5", 8192), ("mixed5", 16384)])
def test_wide_rows_shipped_defaults(name, n):
    """No option set: one batch of n >= 8192 rows folds while the joint
    domain leaves 128 rows per code.  defaults5 (DD4, BB, DD8, GPs, NICH) at
    8192 rows: J = 4 * 2 * 8 = 64 fits exactly, 64 * 16 does not.  mixed5 at
    16 384: J = 16 * 4 * 2 = 128 fits exactly.  Either way three ops are
    folded and GammaPoisson + NormalInverseChiSq remain: instance GN."""
    k = 40
    gpu = engine_for(name, n, k, {})
    for sweep, orc in enumerate(wide_rows.oracle_sweeps(name, n, k, n, SEED)):
        gpu.sweep(0, n, n, SEED, draw_base=sweep * n)
        assert_same_state(orc, gpu, "%s defaults sweep %d" % (name, sweep))
    counts = gpu.core.debug_counts()
    assert counts["scratch_batches"] == 2, counts
    assert counts["fold_batches"] == 2, counts
    assert counts["rows_folded_last"] == 3, counts
    assert counts["rows_instance_last"] == 1, counts


@pytest.mark.parametrize("name", ["wide8", "planted6"])
def test_wide_rows_under_group_churn(name):
    """Two rows per group, a large alpha, three empty groups: in every batch
    groups die and empty ones fill while rows alone in their group (and
    wide8's rows beyond the GammaPoisson table) are handed over."""
    k, alpha, d, empty = 3000, 20.0, 0.5, 3
    gpu = engine_for(name, N, k, {
        "value_sorted": 0, "debug.rows_scratch": 3, "debug.rows_fold": 2},
        alpha, d, empty)
    states = wide_rows.oracle_sweeps(name, N, k, BATCH, SEED, 3, alpha, d,
                                     empty)
    for sweep, orc in enumerate(states):
        gpu.sweep(0, N, BATCH, SEED, draw_base=sweep * N)
        assert_same_state(orc, gpu, "%s churn sweep %d" % (name, sweep))
    assert len(set(len(s) for s in states)) > 1       # the group set changed
    counts = gpu.core.debug_counts()
    assert counts["scratch_batches"] == 6, counts
    assert counts["fold_batches"] == 6, counts
    assert counts["rows_folded_last"] == wide_rows.EXPECT[name][0], counts
    assert counts["rows_instance_last"] == wide_rows.EXPECT[name][1], counts
    assert counts["handed_over_last"] > 0, counts


def test_wide_rows_low_entropy():
    """Clustering::LowEntropy with dataset_size > n through the folded GN
    instance and the hand-over of the rows beyond the GammaPoisson table"""
    name, k, ds = "mixed5_big", 40, N + 1000
    gpu = engine_for(name, N, k, {
        "value_sorted": 0, "debug.rows_scratch": 3, "debug.rows_fold": 2},
        0.7, 0.3, 2, dataset_size=ds)
    states = wide_rows.oracle_sweeps(name, N, k, BATCH, SEED, 2, 0.7, 0.3, 2,
                                     ds)
    for sweep, orc in enumerate(states):
        gpu.sweep(0, N, BATCH, SEED, draw_base=sweep * N)
        assert_same_state(orc, gpu, "low entropy sweep %d" % sweep)
    counts = gpu.core.debug_counts()
    assert counts["scratch_batches"] == 4, counts
    assert_launch(counts, name, 2)


@pytest.mark.parametrize("name", ["wide8", "reals4"])
def test_wide_rows_exact_chains(name):
    """four concurrent exact chains (k_chains) over a long list: three or
    four order-dependent float features per row, groups founded and removed;
    every chain and its returned rng state against gibbs_sequential"""
    from distributions_amd import _core, engine
    m, n, k, empty = 4, 300, 40, 2
    chains = []
    for i in range(m):
        osh, gsh, vals, assign = wide_rows.make(name, n, k, seed=700 + i)
        orc = ol.OracleMixture(8.0, 0.4, osh)
        orc.init_from_assignments(vals, assign, k, empty)
        gpu = engine.Gibbs(8.0, 0.4, gsh)
        gpu.load_rows(vals, assign, k, empty)
        chains.append((orc, gpu))
    states = np.array([_core.rng_seed(31 + i) for i in range(m)], np.uint32)
    got = engine.sweep_sequential_many([g for _, g in chains], 0, n, states)
    for i, (orc, gpu) in enumerate(chains):
        assert int(got[i]) == orc.gibbs_sequential(0, n, int(states[i])), i
        assert_same_state(orc, gpu, "%s chain %d" % (name, i))
    assert sum(g.core.chain_launches() for _, g in chains) >= 1


@pytest.mark.parametrize("name", wide_rows.NAMES)
def test_wide_rows_row_scores_match_oracle(name):
    """the premise of every test above: the oracle and the engine score these
    lists alike, before any sampling is blamed"""
    from distributions_amd import engine
    k = 40
    osh, gsh, vals, assign = wide_rows.make(name, N, k)
    orc = ol.OracleMixture(1.0, 0.2, osh)
    orc.init_from_assignments(vals, assign, k, 1)
    gpu = engine.Gibbs(1.0, 0.2, gsh)
    gpu.load_rows(vals, assign, k, 1)
    for row in [0, 1, 17, 2999, N - 1]:
        g = int(ol.oracle().orc_mix_global_to_packed(orc.h,
                                                     int(orc.assign[row])))
        want = orc.row_scores(row, g)
        got = gpu.row_scores(row)
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (
            name, row, np.abs(got - want).max())
