"""The expectation dist_gibbs_predict is held to (tests/predict_expect.py: the
oracle's driver and slave score_value with the query's values, orc_log_sum_exp,
orc_sample_from_scores_overwrite at the batch convention's engine step) must
itself be right before the GPU is compared with it bit for bit
(tests/test_gpu_predict.py):

  * its logp lies inside the derived float64 band around the float64
    log-sum-exp of the float64 predictives (tests/f64_scores.py), for every
    held-out row of every case;
  * under PitmanYor it is a normalised density: over all 16 values of one
    DirichletDiscrete feature exp(logp) sums to 1 within the summed band;
  * its draws follow the float64 responsibilities (chi-squared, 20 000 draws).

Worst excursion / band measured per case (printed by the test):
  dd (K=19) 0.778; dd_swept (K=66) 0.818; dd_zipf (K=19) 0.878;
  dd_zipf_swept (K=46) 0.858; dd_skew (K=19) 0.402;
  dd_skew_swept (K=78) 0.362; bb (K=19) 0.753; bb_swept (K=92) 0.809;
  gp (K=19) 0.119; gp_swept (K=56) 0.128; bnb (K=19) 0.167;
  bnb_swept (K=75) 0.176; nich (K=19) 0.950; nich_swept (K=62) 0.485;
  gp_nich (K=19) 0.653; gp_nich_swept (K=49) 0.645; nich2 (K=19) 0.951;
  nich2_swept (K=54) 0.338; dpd (K=19) 0.934; dpd_swept (K=83) 0.899;
  dpd_other (K=19) 0.934; dpd_other_swept (K=69) 0.917;
  dd_bb_gp (K=19) 0.181; dd_bb_gp_swept (K=60) 0.593; le_dd (K=17) 0.989;
  le_gp_nich (K=17) 0.388; only_empty_k1 (K=1) 0.514;
  only_empty_k3 (K=3) 0.966; k17 (K=17) 0.946; dd256_k1025 (K=1025) 0.749;
  dpd10000_k8193 (K=8193) 0.719
sum of exp(logp) - 1 = -1.8e-05 within a summed band of 3.3e-05; the draws'
chi-squared p-value is 0.31 (seed 20240601, the first one tried).
"""
import numpy as np
import pytest
from scipy import stats

import eight_expect as xe
import oracle_lib as ol
import predict_expect as pe
import workloads
from test_f64_scores import build


@pytest.mark.parametrize("name", list(pe.CASES))
def test_oracle_logp_is_in_the_float64_band(name):
    c = pe.case(name)
    e = c.expect()
    assert e["scores"].shape == (c.nq, c.K)
    assert np.all(np.isfinite(e["logp"]))
    x = pe.excursion(e["logp"], c)
    print("%s: K=%d, %d held-out rows; worst excursion / band %.3f "
          "(band %.2e .. %.2e)" % (name, c.K, c.nq, x.max(),
                                   c.f64()[1].min(), c.f64()[1].max()))
    assert x.max() <= 1.0, name


@pytest.mark.parametrize("name", ["dd", "dpd_other_swept", "le_gp_nich",
                                  "only_empty_k3"])
def test_expected_groups_are_live_global_ids(name):
    c = pe.case(name)
    e = c.expect()
    live = {c.orc.packed_to_global(k) for k in range(c.K)}
    assert set(e["draw"].tolist()) <= live
    assert set(e["map"].tolist()) <= live
    # the first maximum: no earlier slot scores as high
    g2p = {c.orc.packed_to_global(k): k for k in range(c.K)}
    for q in range(c.nq):
        k = g2p[int(e["map"][q])]
        s = e["scores"][q]
        assert s[k] == s.max() and np.all(s[:k] < s[k])


def test_pitman_yor_logp_is_a_normalised_density():
    """one DirichletDiscrete feature of dim 16: exp(logp) over its 16 values
    sums to 1 to within the bands' sum (needs no band model beyond that)"""
    osh, _, vals, assign = workloads.make("dd", 2000, 16)
    vals[0][vals[0] == 15] = 0          # a value with zero count everywhere
    orc, st = build(osh, vals, assign, 16, 3, 1.0, 0.5)
    q = [np.arange(16, dtype=np.uint32)]
    e = pe.expect(orc, q, ol.oracle().orc_rng_seed(1), 0)
    Lv, band, _ = pe.logp_f64(st, q)
    assert abs(np.exp(Lv).sum() - 1.0) < 1e-12, "the float64 density itself"
    total = np.exp(e["logp"].astype(np.float64)).sum()
    slack = (np.exp(Lv) * np.expm1(band)).sum()
    print("sum of exp(logp) - 1 = %.3e, summed band %.3e" % (total - 1.0,
                                                             slack))
    assert abs(total - 1.0) <= slack
    assert abs(float(e["prior_total"])) <= 1e-5   # the driver is normalised


def test_draws_follow_the_float64_responsibilities():
    """K = 5 (4 groups, 1 empty), one held-out row 20 000 times: row q draws
    with engine step draw_base + q + 1, so the draws differ; chi-squared
    against the float64 responsibilities"""
    osh, _, vals, assign = workloads.make("dd_bb_gp", 200, 4)
    orc, st = build(osh, vals, assign, 4, 1, 1.0, 0.5)
    assert len(orc) == 5
    n = 20000
    row = [np.uint32(3), np.uint32(1), np.uint32(4)]
    q = [np.full(n, v, np.uint32) for v in row]
    e = pe.expect(orc, q, ol.oracle().orc_rng_seed(20240601), 0)
    _, _, p = pe.logp_f64(st, [v[:1] for v in q])
    p2g = [orc.packed_to_global(k) for k in range(5)]
    observed = np.array([(e["draw"] == g).sum() for g in p2g])
    assert observed.sum() == n
    chi2, pvalue = stats.chisquare(observed, p[0] * n)
    print("responsibilities %s, observed %s, chi2 %.2f, p %.4f" % (
        np.round(p[0], 4), observed, chi2, pvalue))
    assert pvalue > 1e-4
    assert len(set(e["map"].tolist())) == 1
    assert e["map"][0] == p2g[int(np.argmax(p[0]))]


# ---------------------------------------------------------------------------
# five to eight features (tests/eight_expect.py)


@pytest.mark.parametrize("name", xe.NAMES)
def test_wide_oracle_logp_is_in_the_float64_band(name):
    """every held-out row, none left out"""
    c = xe.case(name)
    e = c.expect()
    assert e["scores"].shape == (c.nq, c.K)
    assert np.all(np.isfinite(e["logp"]))
    x = pe.excursion(e["logp"], c)
    _, _, p = c.f64()
    print("%s: F=%d, K=%d, %d held-out rows over %d drawn groups; worst "
          "excursion / band %.3f; median largest responsibility %.2f" % (
              name, len(c.osh), c.K, c.nq, len(set(e["draw"].tolist())),
              x.max(), np.median(p.max(1))))
    assert x.max() <= 1.0, name


@pytest.mark.parametrize("variant", ["drop", "wrap"])
@pytest.mark.parametrize("name", xe.NAMES)
def test_wide_planted_variants_leave_the_band(name, variant):
    """a law that leaves a feature >= 4 out, or reads feature f's words from
    feature f & 3, is outside the band the oracle is inside"""
    c = xe.case(name)
    Lv, band, _ = c.f64()
    st, q = xe.planted_state(c.st, c.qvals, variant)
    wrong, _, _ = pe.logp_f64(st, q)
    out = np.abs(wrong - Lv) > band
    print("%s, %s: %.0f %% of the held-out rows leave the band" % (
        name, variant, 100.0 * out.mean()))
    assert out.any()
