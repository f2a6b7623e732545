"""The expectation dist_gibbs_predict_feature is held to
(tests/feature_expect.py) must itself be right before the GPU is compared with
it bit for bit (tests/test_gpu_predict_feature.py):

  * joint of fully observed rows lies inside predict_expect.logp_f64's band
    around the float64 log-sum-exp of the float64 predictives of the
    COMPLETED rows;
  * the conditional sums to one: for a DD or BB target over its whole domain,
    base lies inside the band (logp_f64's over the feature list without the
    target) of the float64 log sum_c exp(L_c), L_c the float64 joints;
  * 20 000 draws of `choice` follow the float64 conditional (chi-squared,
    p > 1e-4, the project's threshold);
  * with nothing observed, base is orc_log_sum_exp of the driver's scores, bit
    for bit.
"""
import numpy as np
import pytest
from scipy import stats

import feature_expect as fe
import oracle_lib as ol
import predict_expect as pe

NROWS = 40      # fully observed held-out rows checked per case


def seed_state():
    return ol.oracle().orc_rng_seed(pe.DRAW_SEED)


def head(c, n=NROWS):
    return [q[:n] for q in c.qvals]


def joints_f64(c, qvals, target, cand):
    """float64 joint and band per candidate, rows completed with it"""
    kind = c.osh[target].kind
    Ls, bands = [], []
    for v in cand:
        Lv, band, _ = pe.logp_f64(c.st, fe.completed(qvals, target, v, kind))
        Ls.append(Lv)
        bands.append(band)
    return np.array(Ls).T, np.array(bands).T


@pytest.mark.parametrize("name,target", [
    ("dd_bb_gp", 0), ("dd_bb_gp_swept", 1), ("dd_bb_gp", 2),
    ("gp_nich_swept", 0), ("nich2", 1), ("le_gp_nich", 1),
    ("mixed4", 1), ("mixed4_swept", 3), ("mixed4", 2)])
def test_joint_of_observed_rows_is_in_the_float64_band(name, target):
    c = fe.case(name)
    q = head(c)
    sh = c.osh[target]
    cand = fe.candidates_for(sh)
    e = fe.expect(c.orc, q, None, target, cand, seed_state(), pe.DRAW_BASE)
    values = fe.default_candidates(sh) if cand is None else cand
    Lv, band = joints_f64(c, q, target, values)
    x = np.abs(e["joint"].astype(np.float64) - Lv) / band
    print("%s target %d: %d candidates, worst excursion / band %.3f" % (
        name, target, len(values), x.max()))
    assert x.max() <= 1.0


@pytest.mark.parametrize("name,target", [
    ("dd_bb_gp", 0), ("dd_bb_gp_swept", 1), ("mixed4", 0), ("mixed4", 1),
    ("mixed4_swept", 3)])
def test_base_is_the_marginal_the_conditional_sums_to_one(name, target):
    c = fe.case(name)
    q = head(c)
    sh = c.osh[target]
    e = fe.expect(c.orc, q, None, target, None, seed_state(), pe.DRAW_BASE)
    Lc, _ = joints_f64(c, q, target, fe.default_candidates(sh))
    m = Lc.max(1)
    total = np.log(np.exp(Lc - m[:, None]).sum(1)) + m
    Lb, band = fe.base_f64(c.st, q, target)
    # the float64 model itself: the target's predictive is normalised
    assert np.abs(total - Lb).max() < 1e-9
    x = np.abs(e["base"].astype(np.float64) - total) / band
    print("%s target %d: base worst excursion / band %.3f" % (name, target,
                                                              x.max()))
    assert x.max() <= 1.0


def test_choice_draws_follow_the_float64_conditional():
    c = fe.case("mixed4")
    n = 20000
    for row, target in ((3, 1), (7, 0)):
        sh = c.osh[target]
        q = [np.repeat(v[row:row + 1], n) for v in c.qvals]
        e = fe.expect(c.orc, q, None, target, None,
                      ol.oracle().orc_rng_seed(20240601), 0)
        Lc, _ = joints_f64(c, [v[:1] for v in q], target,
                           fe.default_candidates(sh))
        p = np.exp(Lc[0] - Lc[0].max())
        p /= p.sum()
        observed = np.bincount(e["draw"], minlength=len(p))
        assert observed.sum() == n
        chi2, pvalue = stats.chisquare(observed, p * n)
        print("row %d target %d: conditional %s, observed %s, chi2 %.2f, "
              "p %.4f" % (row, target, np.round(p, 4), observed, chi2,
                          pvalue))
        assert pvalue > 1e-4
        assert len(set(e["map"].tolist())) == 1
        assert e["map"][0] == int(np.argmax(p))


@pytest.mark.parametrize("name,target", [("dd_bb_gp", 1), ("le_gp_nich", 0),
                                         ("mixed4_swept", 2)])
def test_nothing_observed_gives_the_drivers_log_sum_exp(name, target):
    c = fe.case(name)
    q = head(c, 5)
    cand = fe.candidates_for(c.osh[target])
    e = fe.expect(c.orc, q, np.zeros(5, np.uint32), target, cand,
                  seed_state(), 0)
    K = len(c.orc)
    prior = np.zeros(K, np.float32)
    c.orc.L.orc_mix_driver_score_value(c.orc.h, prior)
    want = np.float32(c.orc.L.orc_log_sum_exp(K, prior))
    assert np.all(e["base"].view(np.uint32) == want.view(np.uint32))
    assert want.view(np.uint32) == np.float32(
        pe.expect(c.orc, q, seed_state(), 0)["prior_total"]).view(np.uint32)
    # and every row's joint is then the same
    assert np.all(e["joint"].view(np.uint32) == e["joint"][0].view(np.uint32))
