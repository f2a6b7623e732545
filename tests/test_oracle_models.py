"""The parts of the oracle that cannot be compared with a compiled reference
here (random.hpp needs Eigen): pinned by the reference's OWN tests for this
path, restated, and by an independent float64 evaluation.

  test_mixture_score            distributions/tests/test_models.py:537-594
  test_mixture_runs             distributions/tests/test_models.py:498-534
  test_py_mixture_matches_...   distributions/tests/test_clustering.py:242-327
  test_sample_discrete_known    distributions/tests/test_random.py:224-247
  test_log_sum_exp              distributions/tests/test_random.py:213-221
  test_scores_sampler_gof       distributions/tests/test_random.py:201-210
EXAMPLES are the lp modules' (lp/models/dd.pyx:35-48, bb.pyx:35-44,
gp.pyx:35-40, nich.pyx:35-40, dpd.pyx:37-66; lp/clustering.pyx:211-217).
"""
import ctypes

import numpy as np
import pytest
from scipy import stats

import oracle_lib as ol
from f64_scores import float64_score

TOL = 1e-3   # distributions/tests/util.py:42


def assert_close(a, b, tol=TOL, msg=""):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert np.all(np.abs(a - b) <= tol * (1.0 + np.abs(a) + np.abs(b))), (
        msg, a, b)


EXAMPLES = [
    ("dd4", ol.DD, dict(alphas=[0.5, 0.5, 0.5, 0.5]), [0, 1, 0, 2, 0, 1, 0]),
    ("dd2", ol.DD, dict(alphas=[1.0, 4.0]), [0, 1, 1, 1, 1, 0, 1]),
    ("dd20", ol.DD, dict(alphas=[2.0 / n for n in range(1, 21)]),
     list(range(20))),
    ("bb", ol.BB, dict(alpha=0.5, beta=2.0), [False, False, True, False, True,
                                              True, False, False]),
    ("bb2", ol.BB, dict(alpha=10.5, beta=0.5), [False] * 9),
    ("gp", ol.GP, dict(alpha=1.0, inv_beta=1.0), [0, 1, 2, 3, 4, 5, 6, 7, 8]),
    ("gp2", ol.GP, dict(alpha=3.0, inv_beta=0.25), [2, 1, 0, 9, 70, 3]),
    ("nich", ol.NICH, dict(mu=0.0, kappa=1.0, sigmasq=1.0, nu=1.0),
     [-4.0, -2.0, 0.0, 1.0, 2.0, 3.0, 5.0]),
    ("nich2", ol.NICH, dict(mu=1.5, kappa=0.3, sigmasq=2.5, nu=4.0),
     [0.25, -1.5, 3.0, 3.25, 100.0]),
    ("dpd", ol.DPD, dict(alpha=0.5, betas=[0.25] * 4, beta0=0.0),
     [0, 1, 0, 2, 0, 1, 0, 3]),
]


def words(kind, value):
    return int(ol.value_words(kind, [value])[0])


@pytest.mark.parametrize("name,kind,kw,values", EXAMPLES)
def test_mixture_score(name, kind, kw, values):
    """Mixture.score_value (accumulating, vectorised caches) ==
    Group.score_value per group (Scorer) == float64, after init, after every
    add and every remove."""
    L = ol.oracle()
    sh = ol.make_shared(kind, **kw)
    m = ol.OracleMixture(1.0, 0.0, [sh])
    members = [[v] for v in values]
    for v in values:
        L.orc_mix_slave_append_empty(m.h, 0)
        L.orc_mix_slave_group_add_value(m.h, 0, len(m_groups(m)) - 1,
                                        words(kind, v))
    L.orc_mix_slave_init(m.h, 0)
    rng = np.random.default_rng(0)

    def check(value):
        k = L.orc_mix_slave_size(m.h, 0)
        expected = [L.orc_group_score_value(ctypes.byref(sh),
                                            m.get_group(0, g),
                                            words(kind, value))
                    for g in range(k)]
        noise = rng.normal(size=k).astype(np.float32)
        actual = noise.copy()
        L.orc_mix_slave_score_value(m.h, 0, words(kind, value), actual)
        actual = actual - noise
        assert_close(actual, expected, msg="score_value")
        another = [L.orc_mix_slave_score_value_group(m.h, 0, g,
                                                     words(kind, value))
                   for g in range(k)]
        assert_close(another, expected, msg="score_value_group")
        f64 = [float64_score(kind, kw, members[g], value) for g in range(k)]
        assert_close(expected, f64, tol=2e-3, msg="float64 " + name)
        return actual

    for v in values:
        check(v)
    placed = []
    for v in values:
        scores = check(v)
        p = np.exp(scores - scores.max())
        g = int(rng.choice(len(p), p=p / p.sum()))
        L.orc_mix_slave_add_value(m.h, 0, g, words(kind, v))
        members[g].append(v)
        placed.append(g)
    for v, g in zip(values, placed):
        L.orc_mix_slave_remove_value(m.h, 0, g, words(kind, v))
        members[g].remove(v)
        check(v)


def m_groups(m):
    return range(ol.oracle().orc_mix_slave_size(m.h, 0))


@pytest.mark.parametrize("name,kind,kw,values", EXAMPLES)
def test_mixture_runs(name, kind, kw, values):
    L = ol.oracle()
    sh = ol.make_shared(kind, **kw)
    m = ol.OracleMixture(1.0, 0.0, [sh])
    for v in values:
        L.orc_mix_slave_append_empty(m.h, 0)
        L.orc_mix_slave_group_add_value(m.h, 0, len(m_groups(m)) - 1,
                                        words(kind, v))
    L.orc_mix_slave_init(m.h, 0)
    st = ctypes.c_uint32(L.orc_rng_seed(0))
    placed = []
    for v in values:
        scores = np.zeros(len(m_groups(m)), np.float32)
        L.orc_mix_slave_score_value(m.h, 0, words(kind, v), scores)
        g = L.orc_sample_from_scores_overwrite(ctypes.byref(st), scores.size,
                                               scores)
        L.orc_mix_slave_add_value(m.h, 0, g, words(kind, v))
        placed.append(g)
    L.orc_mix_slave_add_group(m.h, 0)
    assert len(m_groups(m)) == len(values) + 1
    for v, g in zip(values, placed):
        L.orc_mix_slave_remove_value(m.h, 0, g, words(kind, v))
    L.orc_mix_slave_remove_group(m.h, 0, 0)
    L.orc_mix_slave_remove_group(m.h, 0, len(m_groups(m)) - 1)
    assert len(m_groups(m)) == len(values) - 1


PY_EXAMPLES = [(1.0, 0.0), (1.0, 0.1), (1.0, 0.9), (10.0, 0.1), (0.1, 0.1)]


@pytest.mark.parametrize("alpha,d", PY_EXAMPLES)
@pytest.mark.parametrize("empty_group_count", [1, 10])
def test_py_mixture_matches_score_add_value(alpha, d, empty_group_count):
    L = ol.oracle()
    rng = np.random.default_rng(5)
    nonempty = list(rng.integers(1, 30, 12))
    counts = nonempty + [0] * empty_group_count
    rng.shuffle(counts)
    counts = [int(c) for c in counts]
    m = ol.OracleMixture(alpha, d, [])
    L.orc_mix_driver_init(m.h, np.array(counts, np.int32), len(counts))
    L.orc_mix_tracker_init(m.h, len(counts))

    def check():
        assert L.orc_mix_empty_count(m.h) == empty_group_count
        assert list(m.counts()) == counts
        n = sum(counts)
        ne = len(counts) - empty_group_count
        expected = [L.orc_py_score_add_value(alpha, d, c, ne, n,
                                             empty_group_count)
                    for c in counts]
        actual = rng.normal(size=len(counts)).astype(np.float32)
        L.orc_mix_driver_score_value(m.h, actual)   # overwrites
        assert_close(actual, expected)
        # float64 Pitman-Yor predictive
        f64 = [np.log((c - d) / (n + alpha)) if c else
               np.log((alpha + d * ne) / ((n + alpha) * empty_group_count))
               for c in counts]
        assert_close(actual, f64, tol=2e-3)
        return actual

    check()
    placed = []
    for _ in range(200):
        scores = check()
        p = np.exp(scores - scores.max())
        g = int(rng.choice(len(p), p=p / p.sum()))
        expected_added = counts[g] == 0
        counts[g] += 1
        assert bool(L.orc_mix_driver_add_value(m.h, g)) == expected_added
        placed.append(L.orc_mix_packed_to_global(m.h, g))
        if expected_added:
            L.orc_mix_tracker_add_group(m.h)
            counts.append(0)
    for gl in placed:
        g = L.orc_mix_global_to_packed(m.h, gl)
        counts[g] -= 1
        expected_removed = counts[g] == 0
        assert bool(L.orc_mix_driver_remove_value(m.h, g)) == expected_removed
        if expected_removed:
            L.orc_mix_tracker_remove_group(m.h, g)
            back = counts.pop()
            if g < len(counts):
                counts[g] = back
        check()


def test_sample_discrete_known_answers():
    L = ol.oracle()
    st = ctypes.c_uint32(L.orc_rng_seed(0))
    for probs, want in [([.5], 0), ([1.], 0), ([1e-3], 0),
                        ([1 - 1e-3, 1e-3], 0), ([1e-3, 1 - 1e-3], 1)]:
        p = np.array(probs, np.float32)
        assert L.orc_sample_discrete(ctypes.byref(st), p.size, p) == want


def test_sample_from_scores_recorded_probe():
    """scores {-1,-2.5,.25,-.75,-3}, seed 1 -> 0 0 2 2 2 2 0 2
    (recorded from the compiled reference)"""
    L = ol.oracle()
    st = ctypes.c_uint32(L.orc_rng_seed(1))
    got = []
    for _ in range(8):
        s = np.array([-1, -2.5, .25, -.75, -3], np.float32)
        got.append(L.orc_sample_from_scores_overwrite(ctypes.byref(st), 5, s))
    assert got == [0, 0, 2, 2, 2, 2, 0, 2]


def test_log_sum_exp():
    L = ol.oracle()
    rng = np.random.default_rng(1)
    for size in range(20):
        s = rng.normal(size=size).astype(np.float32)
        want = np.logaddexp.reduce(s.astype(np.float64)) if size else 0.0
        assert_close(L.orc_log_sum_exp(size, np.ascontiguousarray(s)), want)


def test_scores_sampler_goodness_of_fit():
    L = ol.oracle()
    rng = np.random.default_rng(2)
    st = ctypes.c_uint32(L.orc_rng_seed(2))
    for size in [1, 2, 5, 30]:
        scores = rng.normal(size=size).astype(np.float32) * 2
        p = np.exp(scores.astype(np.float64) - scores.max())
        p /= p.sum()
        n = 20000
        hist = np.zeros(size)
        for _ in range(n):
            s = scores.copy()
            hist[L.orc_sample_from_scores_overwrite(ctypes.byref(st), size,
                                                    s)] += 1
        if size > 1:
            chi2 = ((hist - n * p) ** 2 / (n * p)).sum()
            assert stats.chi2.sf(chi2, size - 1) > 1e-4


def test_fast_exp_flushes_like_the_reference_build():
    """FTZ/DAZ: exp(-88) has a zero exponent field in fmath's scale factor,
    which the -ffast-math build treats as zero."""
    L = ol.oracle()
    assert L.orc_fast_exp(-88.0) == 0.0
    assert L.orc_fast_exp(-87.0) > 0.0
    s = np.array([0.0, -100.0, -88.0, -50.0], np.float32)
    total = L.orc_scores_to_likelihoods(4, s)
    assert s[0] == 1.0 and s[1] == 0.0 and s[2] == 0.0 and total >= 1.0


# ---------------------------------------------------------------------------
# score_data / score_counts

@pytest.mark.parametrize("name,kind,kw,values", EXAMPLES)
def test_score_data_chain_rule_and_float64(name, kind, kw, values):
    """distributions/tests/test_models.py:241-251: the sequential predictive
    scores of a group's values sum to its score_data; and both agree with the
    float64 marginal likelihood."""
    L = ol.oracle()
    sh = ol.make_shared(kind, **kw)
    m = ol.OracleMixture(1.0, 0.0, [sh])
    L.orc_mix_slave_append_empty(m.h, 0)
    L.orc_mix_slave_init(m.h, 0)
    chain = 0.0
    f64 = 0.0
    for i, v in enumerate(values):
        chain += L.orc_group_score_value(ctypes.byref(sh), m.get_group(0, 0),
                                         words(kind, v))
        f64 += float64_score(kind, kw, values[:i], v)
        L.orc_mix_slave_add_value(m.h, 0, 0, words(kind, v))
    total = L.orc_group_score_data(ctypes.byref(sh), m.get_group(0, 0))
    assert_close(total, chain, tol=2e-3, msg=name + " chain rule")
    assert_close(total, f64, tol=2e-3, msg=name + " float64")
    # Mixture.score_data == sum of Group.score_data (test_models.py:559-562)
    for v in values[:3]:
        L.orc_mix_slave_add_group(m.h, 0)
        L.orc_mix_slave_add_value(m.h, 0, L.orc_mix_slave_size(m.h, 0) - 1,
                                  words(kind, v))
    expected = sum(L.orc_group_score_data(ctypes.byref(sh), m.get_group(0, g))
                   for g in range(L.orc_mix_slave_size(m.h, 0)))
    assert_close(L.orc_mix_slave_score_data(m.h, 0), expected,
                 msg=name + " mixture score_data")


def test_score_counts_recorded_probe_and_consistency():
    """SURVEY 8c(5), recorded from the compiled reference:
    PitmanYor(alpha=1, d=.2).score_counts({5,3,1,0}) = -9.18923473; and
    test_clustering.py:201-239: score_add_value == difference of
    score_counts."""
    L = ol.oracle()
    got = L.orc_py_score_counts(1.0, 0.2, np.array([5, 3, 1, 0], np.int32), 4)
    assert abs(got - (-9.18923473)) < 5e-7
    rng = np.random.default_rng(8)
    for alpha, d in PY_EXAMPLES:
        counts = [int(c) for c in rng.integers(1, 20, 6)]
        base = L.orc_py_score_counts(alpha, d, np.array(counts, np.int32),
                                     len(counts))
        n = sum(counts)
        for g in range(len(counts) + 1):
            bumped = list(counts) + [0]
            bumped[g] += 1
            after = L.orc_py_score_counts(alpha, d,
                                          np.array(bumped, np.int32),
                                          len(bumped))
            size = counts[g] if g < len(counts) else 0
            add = L.orc_py_score_add_value(alpha, d, size, len(counts), n, 1)
            assert_close(after - base, add, tol=5e-3)


def test_sample_assignments_recorded_probe():
    """SURVEY 8c(5), recorded from the compiled reference: alpha=1, d=.2,
    n=20, default-seeded engine -> 0 0 0 1 0 0 0 0 0 0 2 0 0 2 0 0 0 0 0 0"""
    L = ol.oracle()
    st = ctypes.c_uint32(L.orc_rng_seed(1))
    out = np.zeros(20, np.int32)
    L.orc_py_sample_assignments(1.0, 0.2, 20, ctypes.byref(st), out)
    assert list(out) == [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 2, 0, 0, 2, 0, 0, 0, 0,
                         0, 0]


# ---------------------------------------------------------------------------
# Clustering<int>::LowEntropy (clustering.hpp:245-331, clustering.cc:186-283)

def _le_sigs():
    L = ol.oracle()
    i = ctypes.c_int
    L.orc_le_score_add_value.restype = ctypes.c_float
    L.orc_le_score_add_value.argtypes = [i, i, i, i, i]
    L.orc_le_score_remove_value.restype = ctypes.c_float
    L.orc_le_score_remove_value.argtypes = [i, i, i, i, i]
    L.orc_le_log_partition_function.restype = ctypes.c_float
    L.orc_le_log_partition_function.argtypes = [i]
    L.orc_le_score_counts.restype = ctypes.c_float
    L.orc_le_score_counts.argtypes = [i, ctypes.c_void_p, ctypes.c_size_t]
    return L


def _le_score_counts(L, dataset_size, counts):
    c = np.ascontiguousarray(counts, np.int32)
    return L.orc_le_score_counts(dataset_size, c.ctypes.data, c.size)


def _partitions(n, largest=None):
    """integer partitions of n as non-increasing tuples"""
    largest = n if largest is None else largest
    if n == 0:
        yield ()
        return
    for first in range(min(n, largest), 0, -1):
        for rest in _partitions(n - first, first):
            yield (first,) + rest


def _set_partition_count(shape):
    """number of set partitions of [sum(shape)] with these block sizes"""
    from math import factorial
    from collections import Counter
    n = sum(shape)
    ways = factorial(n)
    for size in shape:
        ways //= factorial(size)
    for mult in Counter(shape).values():
        ways //= factorial(mult)
    return ways


def test_low_entropy_partition_table_is_the_reference_table():
    """the table derived in tools/gen_le_table.py (exact recurrence) equals
    the one the reference ships, to the last bit of binary32"""
    import json
    import os
    L = _le_sigs()
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "low_entropy.json")) as f:
        ref = json.load(f)
    got = np.array([L.orc_le_log_partition_function(n) for n in range(48)],
                   np.float32)
    assert np.array_equal(got.view(np.uint32),
                          np.array(ref["float32_bits"], np.uint32))
    # beyond the table: the asymptotic form (clustering.cc:210-214)
    for n in [48, 100, 1000]:
        want = n * np.log(n) * (1 + 0.28269584 * n ** -0.75)
        assert abs(L.orc_le_log_partition_function(n) - want) < 1e-3 * want


def test_low_entropy_score_counts_is_normalised_at_full_size():
    """test_clustering.py:168-193: sum over all set partitions of
    exp(score_counts) is 1 when sample_size == dataset_size"""
    L = _le_sigs()
    for n in range(1, 11):
        total = 0.0
        for shape in _partitions(n):
            total += _set_partition_count(shape) * np.exp(
                _le_score_counts(L, n, list(shape)))
        assert abs(total - 1.0) < 1e-4, (n, total)


@pytest.mark.parametrize("dataset_size", [5, 10, 100, 1000])
def test_low_entropy_score_add_value_matches_score_counts(dataset_size):
    """test_clustering.py:201-238: probabilities from score_add_value agree
    with ratios of score_counts to 0.05"""
    L = _le_sigs()

    def probs(scores):
        scores = np.array(scores, np.float64)
        p = np.exp(scores - scores.max())
        return p / p.sum()

    for sample_size in range(2, min(10, dataset_size) + 1):
        for shape in _partitions(sample_size - 1):
            counts = list(shape)
            nonempty = len(counts)
            actual, expected = [], []
            for i, size in enumerate(counts):
                bumped = counts[:]
                bumped[i] += 1
                expected.append(_le_score_counts(L, dataset_size, bumped))
                actual.append(L.orc_le_score_add_value(
                    dataset_size, size, nonempty, sample_size - 1, 1))
            expected.append(_le_score_counts(L, dataset_size, counts + [1]))
            actual.append(L.orc_le_score_add_value(
                dataset_size, 0, nonempty, sample_size - 1, 1))
            np.testing.assert_allclose(probs(actual), probs(expected),
                                       atol=0.05)


def test_low_entropy_score_remove_value_is_minus_add_of_the_smaller_group():
    L = _le_sigs()
    for n in [1, 2, 7, 10001, 20000]:
        assert L.orc_le_score_remove_value(50000, n + 1, 3, 100, 1) == \
            -L.orc_le_score_add_value(50000, n, 3, 100, 1)
    # beyond very_large the closed form 1 + log(n + 1) (clustering.hpp:283-291)
    b = L.orc_le_score_add_value(10 ** 6, 10001, 1, 10, 1)
    assert abs(b - (1 + np.log(10002.0))) < 1e-3


def test_low_entropy_driver_scores_are_score_add_value():
    """MixtureDriver<LowEntropy>::score_value (mixture.hpp:124-141) through
    the oracle mixture's driver"""
    L = _le_sigs()
    L.orc_mix_set_low_entropy.restype = None
    L.orc_mix_set_low_entropy.argtypes = [ctypes.c_void_p, ctypes.c_int]
    m = ol.OracleMixture(1.0, 0.0, [ol.make_shared(ol.BB, alpha=1.0, beta=1.0)])
    L.orc_mix_set_low_entropy(m.h, 500)
    counts = np.array([5, 0, 3, 1, 0, 40], np.int32)
    L.orc_mix_driver_init(m.h, counts, len(counts))
    scores = np.zeros(len(counts), np.float32)
    L.orc_mix_driver_score_value(m.h, scores)
    for k, c in enumerate(counts):
        assert scores[k] == np.float32(L.orc_le_score_add_value(
            500, int(c), 4, int(counts.sum()), 2))
    assert L.orc_mix_driver_add_value(m.h, 1) == 1      # an empty group filled
    assert L.orc_mix_size(m.h) == len(counts) + 1


def test_low_entropy_sample_assignments_matches_score_counts():
    """test_clustering.py:139-165 (test_sample_matches_score_counts): the
    frequencies of sampled partitions follow exp(score_counts), at full size
    where score_counts is exactly normalised"""
    L = _le_sigs()
    L.orc_le_sample_assignments.restype = None
    L.orc_le_sample_assignments.argtypes = [
        ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    from collections import Counter
    size = 6
    state = ctypes.c_uint32(L.orc_rng_seed(123))
    n_samples = 20000
    seen = Counter()
    out = np.zeros(size, np.int32)
    for _ in range(n_samples):
        L.orc_le_sample_assignments(size, size, ctypes.byref(state),
                                    out.ctypes.data)
        # first-appearance labelling: group ids are 0..G-1 in order
        assert out[0] == 0 and all(
            out[i] <= out[:i].max() + 1 for i in range(1, size))
        seen[tuple(out.tolist())] += 1
    # every set partition of 6 elements (Bell(6) = 203) has probability
    # exp(score_counts(shape)); compare by shape
    by_shape = Counter()
    for labels, count in seen.items():
        shape = tuple(sorted(Counter(labels).values(), reverse=True))
        by_shape[shape] += count
    for shape in _partitions(size):
        p = _set_partition_count(shape) * np.exp(
            _le_score_counts(L, size, list(shape)))
        got = by_shape[shape] / n_samples
        assert abs(got - p) < 4 * np.sqrt(p * (1 - p) / n_samples) + 2e-3, (
            shape, got, p)


def test_low_entropy_table_headers_are_what_the_generator_writes():
    """le_table.h (product and oracle copies) == tools/gen_le_table.py's
    output: the table in the build is the independently derived one"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "gen_le_table", os.path.join(root, "tools", "gen_le_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    text = gen.render()
    for rel in ("distributions_amd/csrc/le_table.h", "oracle/le_table.h"):
        with open(os.path.join(root, rel)) as f:
            assert f.read() == text, rel
