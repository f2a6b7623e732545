"""The host arithmetic on a partition agreement (engine.rand_index,
adjusted_rand_index, binder_distance, variation_of_information, consensus),
fed with the matrices of the numpy restatement (tests/partition_expect.py):
against workloads.adjusted_rand_index, against brute force over the explicit
N x N matrices, and on constructed cases.  The restatement's own measures go
through the same assertions, and three planted bugs in it must each trip at
least one of them: the expectation the GPU tests hold the device to can tell
a wrong answer from a right one."""
import numpy as np
import pytest

import partition_expect as pe
import workloads
from distributions_amd import engine


def random_pairs():
    """ten pairs of label columns, N = 500, 1 to 40 labels, arbitrary names"""
    rng = np.random.default_rng(20240917)
    pairs = []
    for i in range(10):
        ka, kb = (1, 40) if i == 0 else rng.integers(1, 41, 2)
        a = rng.integers(0, ka, 500) * 3 + 7
        b = rng.integers(0, kb, 500)
        if i % 3 == 1:      # (related partitions, not only independent ones)
            b = np.where(rng.random(500) < 0.8, a % kb, b)
        pairs.append((a, b))
    return pairs


def check_ari(bug=None):
    """ARI = workloads.adjusted_rand_index to 1e-12 on the ten pairs"""
    for a, b in random_pairs():
        res, _ = pe.agreement([a, b], bug=bug)
        with np.errstate(invalid="ignore"):
            want = workloads.adjusted_rand_index(a, b)
        if not np.isfinite(want):       # (one group against one group)
            want = 1.0
        for got in (engine.adjusted_rand_index(res),
                    pe.adjusted_rand_index(res, bug)):
            assert got.shape == (2, 2)
            assert abs(got[0, 1] - want) <= 1e-12, (got[0, 1], want)
            assert got[0, 1] == got[1, 0]
            assert got[0, 0] == 1.0 and got[1, 1] == 1.0


def check_renamed(bug=None):
    """two equal partitions under different names"""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 9, 300)
    b = np.array([40, 3, 17, 5, 900, 1, 0, 8, 2])[a]
    res, _ = pe.agreement([a, b], bug=bug)
    for ari, rand, binder in (
            (engine.adjusted_rand_index(res), engine.rand_index(res),
             engine.binder_distance(res)),
            (pe.adjusted_rand_index(res, bug), pe.rand_index(res, bug),
             pe.binder_distance(res, bug))):
        assert ari[0, 1] == 1.0
        assert rand[0, 1] == 1.0
        assert binder[0, 1] == 0 and binder[1, 0] == 0
    for vi in (engine.variation_of_information(res),
               pe.variation_of_information(res)):
        assert abs(vi[0, 1]) <= 1e-12


def check_singletons_against_one_group(bug=None):
    n = 50
    res, _ = pe.agreement([np.arange(n), np.zeros(n, np.int64)], bug=bug)
    assert int(res.sq[0, 1]) == n                 # n cells of one row
    t = (res.sq.astype(np.int64) - n) // 2
    assert t[0, 1] == 0 and t[0, 0] == 0 and t[1, 1] == n * (n - 1) // 2
    for got in (engine.adjusted_rand_index(res),
                pe.adjusted_rand_index(res, bug)):
        assert got[0, 1] == 0.0
    # Rand: the pairs both separate (none) plus the pairs both join (none)
    for got in (engine.rand_index(res), pe.rand_index(res, bug)):
        assert got[0, 1] == 0.0
    # VI = H(singletons) + H(one group) - 2 I = log n
    for got in (engine.variation_of_information(res),
                pe.variation_of_information(res)):
        assert abs(got[0, 1] - np.log(n)) <= 1e-12


def brute_columns(m=7, n=60):
    rng = np.random.default_rng(77)
    base = rng.integers(0, 5, n)
    cols = []
    for i in range(m):
        c = base.copy()
        move = rng.random(n) < 0.05 + 0.07 * i
        c[move] = rng.integers(0, 7, int(move.sum()))
        cols.append(c)
    return cols


def check_binder_brute(bug=None):
    cols = brute_columns()
    res, _ = pe.agreement(cols, bug=bug)
    want = np.array([[pe.binder_brute(a, b) for b in cols] for a in cols])
    assert want.max() > 0
    for got in (engine.binder_distance(res), pe.binder_distance(res, bug)):
        assert got.dtype == np.int64
        assert np.array_equal(got, want)


def check_consensus_brute(bug=None):
    cols = brute_columns()
    res, _ = pe.agreement(cols, bug=bug)
    want, loss = pe.consensus_brute(cols)
    # (the minimum is a clear one: an exact tie is the next test's)
    assert np.sort(loss)[1] - np.sort(loss)[0] > 1e-6
    for index, total in (engine.consensus(res), pe.consensus(res, bug=bug)):
        assert index == want
        assert len(total) == 7
        # sum_b Binder(a, b) = M |delta_a - PSM|^2 + a constant of the set
        shift = total - len(cols) * loss
        assert np.abs(shift - shift[0]).max() <= 1e-6
    # among: a subset, and extras beside the samples
    sub = [1, 3, 4, 6]
    want_sub, _ = pe.consensus_brute([cols[i] for i in sub])
    assert engine.consensus(res, among=sub)[0] == sub[want_sub]
    truth = np.arange(60) % 5
    res_x, _ = pe.agreement(cols + [truth], m=7)
    assert engine.consensus(res_x)[0] == want     # (the extra does not vote)
    assert np.array_equal(engine.consensus(res_x)[1], engine.consensus(res)[1])


def test_ari_equals_the_contingency_form():
    check_ari()


def test_equal_partitions_under_other_names():
    check_renamed()


def test_singletons_against_one_group():
    check_singletons_against_one_group()


def test_binder_equals_brute_force():
    check_binder_brute()


def test_consensus_equals_least_squares_from_the_similarity_matrix():
    check_consensus_brute()


def test_consensus_takes_the_first_of_a_tie():
    """samples 1 and 2 are one partition under two names, sample 0 and 3 are
    each as far from them as from each other: 1 and 2 tie, 1 is named"""
    a = np.array([0, 0, 1, 1, 2, 2])
    cols = [np.array([0, 1, 2, 3, 4, 5]), a, a + 10, np.zeros(6, np.int64)]
    res, _ = pe.agreement(cols)
    index, total = engine.consensus(res)
    assert total[1] == total[2] == total.min()
    assert index == 1
    assert engine.consensus(res, among=[2, 1, 0])[0] == 2
    assert engine.consensus(res, among=[3])[0] == 3
    with pytest.raises(RuntimeError, match="no partition"):
        engine.consensus(res, among=[])


def test_fewer_than_two_rows():
    res, _ = pe.agreement([np.array([4]), np.array([0])])
    assert np.array_equal(engine.adjusted_rand_index(res), np.ones((2, 2)))
    assert np.array_equal(engine.rand_index(res), np.ones((2, 2)))
    assert np.array_equal(engine.binder_distance(res), np.zeros((2, 2)))
    assert np.array_equal(engine.variation_of_information(res),
                          np.zeros((2, 2)))


def test_variation_of_information_needs_nlogn():
    res, _ = pe.agreement([np.arange(4), np.arange(4)])
    res.nlogn = None
    with pytest.raises(RuntimeError, match="nlogn=False"):
        engine.variation_of_information(res)


ALL_CHECKS = [check_ari, check_renamed, check_singletons_against_one_group,
              check_binder_brute, check_consensus_brute]


@pytest.mark.parametrize("bug", ["sq_no_diagonal", "pairs_n2", "binder_half"])
def test_a_planted_bug_is_caught(bug):
    caught = []
    for check in ALL_CHECKS:
        try:
            check(bug)
        except AssertionError:
            caught.append(check.__name__)
    assert caught, "no assertion noticed %s" % bug
