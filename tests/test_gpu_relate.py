"""dist_gibbs_relate[_many] (sample_rows_many's draw, k_marginals_many,
k_ensemble_fold, k_relate_moments): the mutual information of every feature
pair and the entropies under an ensemble's predictive.

The rows behind relate_many(seed, member_seed, draw_base) are
sample_rows_many's, so the sums are recomputed on the host in float64 from
marginals_many on those rows and held to the float64 summation bound
n 2^-52 sum |d|; equal calls give equal bits; chunking moves the sums within
that bound; the matrix is symmetric bit for bit; and at n = 20 000 the (DD, BB)
cell and the two entropies of dd_bb_gp lie within 5 sigma / sqrt(n) of the law
tests/marginals_expect.py enumerates in float64 (tests/test_marginals_oracle.py
checks on the CPU that the oracle's composition does, for the same seed)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ensemble_expect as ee  # noqa: E402
import marginals_expect as mx  # noqa: E402

pytestmark = pytest.mark.gpu

# (tests/test_marginals_oracle.py checks the reference composition for these)
SEED, MEMBER_SEED, BASE, N_LAW = 7, 8, 1000, 20000
EPS64 = 2.0 ** -52
_STATE = {}


def ensemble():
    if "ens" not in _STATE:
        _STATE["ens"] = ee.Ensemble("dd_bb_gp", ee.SPECS3)
        _STATE["gpus"] = _STATE["ens"].engines()
    return _STATE["ens"], _STATE["gpus"]


def host_d(gpus, n, single=False, planes=None):
    """the rows sample_rows_many draws and, from marginals_many on them, d_q
    in float64 per cell -> d [F, F, n] (the upper triangle and the diagonal:
    -L_i); planes: the folded values to use in the place of marginals_many's
    """
    from distributions_amd import engine
    F = len(gpus[0].shareds)
    cols, _, _ = engine.sample_rows_many(gpus, n=n, seed=SEED,
                                         member_seed=MEMBER_SEED,
                                         draw_base=BASE)
    masks = mx.singles_and_pairs(F)
    if planes is not None:
        lp = planes(cols, masks)
    elif single:
        lp = gpus[0].marginals(cols, masks)
    else:
        lp = engine.marginals_many(gpus, cols, masks)[0]
    lp = lp.astype(np.float64)
    d = np.zeros((F, F, n))
    col = F
    for i in range(F):
        d[i, i] = -lp[:, i]
    for i in range(F):
        for j in range(i + 1, F):
            d[i, j] = lp[:, col] - lp[:, i] - lp[:, j]
            col += 1
    return d


def check_sums(moments, d, n, slack=1.0):
    """sum d and sum d^2 within the float64 summation bound of numpy's"""
    F = d.shape[0]
    for i in range(F):
        for j in range(i, F):
            x = d[i, j]
            for c, v in enumerate((x, x * x)):
                bound = slack * n * EPS64 * np.abs(v).sum()
                got = moments[i, j, c]
                assert abs(got - np.sum(v, dtype=np.float64)) <= bound, \
                    (i, j, c, got, np.sum(v, dtype=np.float64), bound)
                assert moments[j, i, c] == got


def test_the_sums_are_those_of_sample_rows_manys_rows():
    from distributions_amd import engine
    ens, gpus = ensemble()
    n = 1000
    d = host_d(gpus, n)
    mi, se, mo = engine.relate_many(gpus, n, seed=SEED,
                                    member_seed=MEMBER_SEED, draw_base=BASE,
                                    moments=True)
    check_sums(mo, d, n)
    F = d.shape[0]
    for i in range(F):
        for j in range(i, F):
            x = d[i, j]
            assert abs(n * mi[i, j] - np.sum(x, dtype=np.float64)) \
                <= n * EPS64 * np.abs(x).sum()
            want = np.sqrt(np.var(x, ddof=1) / n)
            print("cell (%d, %d): mi %.6g, stderr %.6g against numpy's %.6g"
                  % (i, j, mi[i, j], se[i, j], want))
            assert abs(se[i, j] - want) <= 1e-12 * want
    # symmetric in every bit
    assert np.array_equal(mi.view(np.uint64), mi.T.view(np.uint64))
    assert np.array_equal(se.view(np.uint64), se.T.copy().view(np.uint64))
    # the same call again: the same bits
    mi2, se2, mo2 = engine.relate_many(gpus, n, seed=SEED,
                                       member_seed=MEMBER_SEED,
                                       draw_base=BASE, moments=True)
    assert np.array_equal(mo.view(np.uint64), mo2.view(np.uint64))
    assert np.array_equal(mi.view(np.uint64), mi2.view(np.uint64))
    assert np.array_equal(se.view(np.uint64), se2.view(np.uint64))
    # default outputs, and the engines are as they were
    two = engine.relate_many(gpus, n, seed=SEED, member_seed=MEMBER_SEED,
                             draw_base=BASE)
    assert len(two) == 2 and np.array_equal(two[0], mi)
    for g, m in zip(gpus, ens.members):
        assert np.array_equal(g.assignments(), m.orc.assign)
        g.validate()


def test_chunks_move_the_sums_within_the_summation_band():
    from distributions_amd import engine
    _, gpus = ensemble()
    n = 1000
    d = host_d(gpus, n)
    one = engine.relate_many(gpus, n, seed=SEED, member_seed=MEMBER_SEED,
                             draw_base=BASE, moments=True)[2]
    try:
        gpus[0].set_option("debug.predict_chunk", 96)
        many = engine.relate_many(gpus, n, seed=SEED,
                                  member_seed=MEMBER_SEED, draw_base=BASE,
                                  moments=True)[2]
        again = engine.relate_many(gpus, n, seed=SEED,
                                   member_seed=MEMBER_SEED, draw_base=BASE,
                                   moments=True)[2]
    finally:
        gpus[0].set_option("debug.predict_chunk", 1 << 22)
    check_sums(many, d, n)
    assert np.array_equal(many.view(np.uint64), again.view(np.uint64))
    F = d.shape[0]
    for i in range(F):
        for j in range(i, F):
            for c, v in enumerate((d[i, j], d[i, j] ** 2)):
                assert abs(one[i, j, c] - many[i, j, c]) \
                    <= n * EPS64 * np.abs(v).sum()


def test_one_row_none_and_one_engine():
    from distributions_amd import engine
    _, gpus = ensemble()
    mi, se = engine.relate_many(gpus, 1, seed=SEED, member_seed=MEMBER_SEED,
                                draw_base=BASE)
    d = host_d(gpus, 1)
    for i in range(3):
        for j in range(i, 3):
            assert mi[i, j] == d[i, j, 0]
    assert np.all(np.isposinf(se))
    with pytest.raises(RuntimeError, match="no sample"):
        engine.relate_many(gpus, 0)
    # one engine: sample_rows' rows, marginals without the fold
    n = 500
    d1 = host_d(gpus[1:2], n, single=True)
    mo = gpus[1].relate(n, seed=SEED, member_seed=MEMBER_SEED, draw_base=BASE,
                        moments=True)[2]
    check_sums(mo, d1, n)


def test_the_estimate_is_the_enumerated_law_within_five_sigma():
    from distributions_amd import engine
    ens, gpus = ensemble()
    n = N_LAW
    law = mx.enumerate_pair([m.st for m in ens.members], 0, 1, False)
    mi, se = engine.relate_many(gpus, n, seed=SEED, member_seed=MEMBER_SEED,
                                draw_base=BASE)
    root = np.sqrt(n)
    print("n=%d: mi(DD, BB) %.6g +- %.3g against %.6g (sigma / sqrt n "
          "%.3g), H(DD) %.6g against %.6g, H(BB) %.6g against %.6g"
          % (n, mi[0, 1], se[0, 1], law["mi"], law["sigma"] / root, mi[0, 0],
             law["h_i"], mi[1, 1], law["h_j"]))
    assert abs(mi[0, 1] - law["mi"]) <= 5 * law["sigma"] / root
    assert abs(mi[0, 0] - law["h_i"]) <= 5 * law["sigma_i"] / root
    assert abs(mi[1, 1] - law["h_j"]) <= 5 * law["sigma_j"] / root
    assert abs(se[0, 1] / (law["sigma"] / root) - 1) <= 0.1


def test_two_copies_of_a_state_relate_as_the_fold_says():
    """An ensemble of two engines in the same state draws the one-engine rows
    (either member gives row q the same group and cells) and folds two equal
    planes: L2 = ensemble_expect.fold([w, w]), which is w plus whatever
    fast_log(fast_exp(0) + fast_exp(0)) - fast_log(2) leaves in float32 --
    computed here, not assumed to vanish.  The two-member sums are those of
    the folded planes, and the (DD, BB) cell differs from the one-engine cell
    by the mean of that residue's d."""
    from distributions_amd import engine
    ens, _ = ensemble()
    a, b = ens.members[1].engine(), ens.members[1].engine()
    n = 1000
    cols1 = engine.sample_rows_many([a], n=n, seed=SEED,
                                    member_seed=MEMBER_SEED,
                                    draw_base=BASE)[0]
    cols2 = engine.sample_rows_many([a, b], n=n, seed=SEED,
                                    member_seed=MEMBER_SEED,
                                    draw_base=BASE)[0]
    for c1, c2 in zip(cols1, cols2):
        assert np.array_equal(c1, c2)

    def folded(cols, masks):
        w = a.marginals(cols, masks)
        lp, _, _ = ee.fold(np.stack([w.ravel(), w.ravel()]), 1, 0)
        return lp.reshape(w.shape)

    d1 = host_d([a], n, single=True)
    d2 = host_d([a, b], n, planes=folded)
    assert np.array_equal(
        engine.marginals_many([a, b], cols2, mx.singles_and_pairs(3))[0]
        .view(np.uint32),
        folded(cols2, mx.singles_and_pairs(3)).view(np.uint32))
    mi1, _, mo1 = a.relate(n, seed=SEED, member_seed=MEMBER_SEED,
                           draw_base=BASE, moments=True)
    mi2, _, mo2 = engine.relate_many([a, b], n, seed=SEED,
                                     member_seed=MEMBER_SEED, draw_base=BASE,
                                     moments=True)
    check_sums(mo1, d1, n)
    check_sums(mo2, d2, n)
    residue = d2[0, 1] - d1[0, 1]
    print("two copies: mi(DD, BB) %.9g against one engine's %.9g; the fold's "
          "residue in d is at most %.3g, its mean %.3g"
          % (mi2[0, 1], mi1[0, 1], np.abs(residue).max(), residue.mean()))
    band = EPS64 * (np.abs(d1[0, 1]).sum() + np.abs(d2[0, 1]).sum())
    assert abs((mi2[0, 1] - mi1[0, 1]) - residue.mean()) <= band
