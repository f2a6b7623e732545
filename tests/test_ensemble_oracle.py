"""The expectation dist_gibbs_predict_many is held to (tests/ensemble_expect.py:
predict_expect.expect per member, orc_log_sum_exp over the members minus
orc_fast_log(M), orc_sample_from_scores_overwrite at the member stream's
engine step) must itself be right before the GPU is compared with it bit for
bit (tests/test_gpu_predict_many.py):

  * its logp lies inside the derived float64 band around
    log (1/M) sum_e p(x | member e), for every held-out row of every
    configuration of test_f64_scores.CONFIGS at M = 3 -- members that differ
    in rows, K (5, 20+, 43+), empty groups, alpha, d, sweeps and
    hyper-parameters -- and for LowEntropy dd and gp_nich at M = 3;
  * planted bugs -- the mean of the logs, the missing - log M, LowEntropy
    without the members' own normalisation -- lie more than ten bands away
    for at least 90 % of the held-out rows;
  * its member draws follow the float64 responsibilities exp(W_e - L) / M
    (chi-squared, 20 000 draws per configuration);
  * for M = 1 it is predict_expect.expect, bit for bit.
"""
import numpy as np
import pytest
from scipy import stats

import eight_expect as xe
import ensemble_expect as ee
import oracle_lib as ol
import predict_expect as pe
from test_f64_scores import CONFIGS

LE_SPECS3 = [dict(k=4, empty=1, alpha=1.0, d=0.0, sweeps=0),
             dict(k=17, empty=1, alpha=1.0, d=0.0, sweeps=0),
             dict(k=41, empty=1, alpha=1.0, d=0.0, sweeps=0)]

# the planted bugs' members: the mean of the logs differs from the log of the
# mean only where the members disagree, so these also differ in their row
# counts (100, 600, 1500) and sweep counts; checked with the oracle on the
# CPU before they were fixed (the fractions the test prints)
FAR_SPECS3 = [dict(k=4, empty=1, alpha=1.0, d=0.0, sweeps=0, n=100),
              dict(k=17, empty=3, alpha=20.0, d=0.5, sweeps=1),
              dict(k=41, empty=2, alpha=5.0, d=0.25, sweeps=3, n=1500)]
FAR_LE_SPECS3 = [dict(k=4, empty=1, alpha=1.0, d=0.0, sweeps=0, n=100),
                 dict(k=17, empty=1, alpha=1.0, d=0.0, sweeps=0),
                 dict(k=41, empty=1, alpha=1.0, d=0.0, sweeps=0, n=1500)]

_ENS = {}


def ensemble(name):
    if name not in _ENS:
        if name.startswith("farle_"):
            _ENS[name] = ee.Ensemble(name[6:], FAR_LE_SPECS3, le=3000)
        elif name.startswith("far_"):
            _ENS[name] = ee.Ensemble(name[4:], FAR_SPECS3)
        elif name.startswith("le_"):
            _ENS[name] = ee.Ensemble(name[3:], LE_SPECS3, le=2000)
        else:
            other = (1, 2) if name == "dpd_other" else ()
            _ENS[name] = ee.Ensemble(name, ee.SPECS3, other=other)
    return _ENS[name]


NAMES = list(CONFIGS) + ["le_dd", "le_gp_nich"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", NAMES)
def test_expectation_is_in_the_float64_band(name):
    ens = ensemble(name)
    e = ens.expect()
    assert e["w"].shape == (3, ens.nq)
    assert np.all(np.isfinite(e["logp"]))
    x = ee.excursion(e["logp"], ens)
    _, band, _ = ens.f64()
    print("%s: K = %s, %d held-out rows; worst excursion / band %.3f "
          "(band %.2e .. %.2e)" % (name, [m.K for m in ens.members], ens.nq,
                                   x.max(), band.min(), band.max()))
    assert x.max() <= 1.0, name


@pytest.mark.parametrize("name,variant", [
    ("far_dd", "mean_of_logs"), ("far_dd", "no_log_m"),
    ("far_gp_nich", "no_log_m"), ("far_dd_bb_gp", "no_log_m"),
    ("farle_dd", "unnormalised"), ("farle_gp_nich", "unnormalised"),
    ("farle_dd", "no_log_m")])
def test_planted_bug_leaves_the_band(name, variant):
    ens = ensemble(name)
    Lv, band, _ = ens.f64()
    wrong, _, _ = ee.law_f64([m.st for m in ens.members], ens.qvals,
                             ens.le is not None, variant)
    assert ee.excursion(ens.expect()["logp"], ens).max() <= 1.0
    far = np.abs(wrong - Lv) > 10.0 * band
    print("%s, %s: %.1f %% of the held-out rows more than ten bands away; "
          "median distance / band %.1f" % (
              name, variant, 100.0 * far.mean(),
              np.median(np.abs(wrong - Lv) / band)))
    assert far.mean() >= 0.9


@pytest.mark.parametrize("name", NAMES)
def test_member_draws_follow_the_float64_responsibilities(name):
    """one held-out row 20 000 times (the row whose least likely member is
    the most likely: every cell is populated); draw q uses engine step
    draw_base + q + 1 of the member stream, so the draws differ"""
    ens = ensemble(name)
    e = ens.expect()
    _, _, r = ens.f64()
    q = int(np.argmax(r.min(1)))
    n = 20000
    w = np.repeat(e["w"][:, q:q + 1], n, axis=1)
    _, draw, first = ee.fold(w, ol.oracle().orc_rng_seed(20240601), 0)
    expected = r[q] * n
    observed = np.bincount(draw, minlength=ens.M).astype(np.float64)
    small = expected < 50
    if small.any():          # cells of expected count >= 50: pool the rest
        keep = np.nonzero(~small)[0]
        pooled_e, pooled_o = expected[small].sum(), observed[small].sum()
        expected, observed = expected[keep], observed[keep]
        if pooled_e >= 50:
            expected = np.append(expected, pooled_e)
            observed = np.append(observed, pooled_o)
        else:
            i = int(np.argmin(expected))
            expected[i] += pooled_e
            observed[i] += pooled_o
    assert len(expected) >= 2, "a row one member owns tests nothing"
    chi2, pvalue = stats.chisquare(observed, expected)
    print("%s row %d: responsibilities %s, cells %s / %s, chi2 %.2f, p %.4f"
          % (name, q, np.round(r[q], 4), observed, np.round(expected, 1),
             chi2, pvalue))
    assert pvalue > 1e-4
    assert len(set(first.tolist())) == 1
    assert first[0] == int(np.argmax(r[q]))


@pytest.mark.parametrize("name", ["dd", "gp_nich", "le_dd"])
def test_one_member_is_predict_itself(name):
    ens = ensemble(name)
    L = ol.oracle()
    for m in ens.members:
        one = ee.expect_many([m.orc], ens.qvals, L.orc_rng_seed(ee.DRAW_SEED),
                             L.orc_rng_seed(ee.MEMBER_SEED), ee.DRAW_BASE,
                             ens.le is not None)
        p = pe.expect(m.orc, ens.qvals, L.orc_rng_seed(ee.DRAW_SEED),
                      ee.DRAW_BASE)
        want = p["logp"]
        if ens.le is not None:
            want = (want - p["prior_total"]).astype(np.float32)
        assert L.orc_fast_log(1.0) == 0.0 and L.orc_fast_exp(0.0) == 1.0
        assert np.array_equal(bits(one["logp"]), bits(want))
        assert np.all(one["member_draw"] == 0)
        assert np.all(one["member_map"] == 0)
        assert np.array_equal(one["group_draw"], p["draw"])
        assert np.array_equal(one["group_map"], p["map"])


# ---------------------------------------------------------------------------
# the eight-feature ensemble of tests/eight_expect.py


def test_eight3_expectation_is_in_the_float64_band():
    """every held-out row, none left out"""
    ens = xe.eight3()
    e = ens.expect()
    assert e["w"].shape == (3, ens.nq)
    assert np.all(np.isfinite(e["logp"]))
    assert len({m.K for m in ens.members}) == 3
    x = ee.excursion(e["logp"], ens)
    print("eight3: K = %s, %d held-out rows; worst excursion / band %.3f; "
          "member draws %s" % ([m.K for m in ens.members], ens.nq, x.max(),
                               np.bincount(e["member_draw"], minlength=3)))
    assert x.max() <= 1.0


@pytest.mark.parametrize("variant", ["drop", "wrap"])
def test_eight3_planted_variants_leave_the_band(variant):
    ens = xe.eight3()
    Lv, band, _ = ens.f64()
    planted = [xe.planted_state(m.st, ens.qvals, variant)
               for m in ens.members]
    wrong, _, _ = ee.law_f64([p[0] for p in planted], planted[0][1], False)
    out = np.abs(wrong - Lv) > band
    print("eight3, %s: %.0f %% of the held-out rows leave the band" % (
        variant, 100.0 * out.mean()))
    assert out.any()
