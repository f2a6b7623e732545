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

import eight_expect as xe
import feature_expect as fe
import feature_many_expect as fm
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


# ---------------------------------------------------------------------------
# five to eight features (tests/eight_expect.py), under per-row masks


def wide_law(c, q, masks, target, values):
    """feature_many_expect.law_f64 over the one member: the float64 joint and
    base of every row over the features its mask observes, and their bands
    (the fold over one member adds orc_fast_log(1) = 0 and one eps)"""
    return fm.law_f64([c.st], q, masks, target, values, False)


WIDE = [(name, t) for name in ("eight", "eight_swept")
        for t in xe.TARGETS8] + [("real_first", 0), ("real_first", 1),
                                 ("real_first", 4)]


@pytest.mark.parametrize("name,target", WIDE)
def test_wide_joint_and_base_are_in_the_float64_band(name, target):
    """every candidate on every one of the first n held-out rows (n = NROWS,
    15 for DD70's 70 candidates), under random masks and the fixed ones (only
    features >= 4, only features < 4, alternating)"""
    c = xe.case(name)
    F = len(c.osh)
    sh = c.osh[target]
    cand = fe.candidates_for(sh)
    # (DD70's 70 candidates on the rows of the fixed masks and three more)
    n = 15 if sh.kind == ol.DD and sh.dim > 30 else NROWS
    q = head(c, n)
    masks = xe.masks_for(n, F, 100 + target)
    e = fe.expect(c.orc, q, masks, target, cand, seed_state(), pe.DRAW_BASE)
    assert np.all(np.isfinite(e["joint"])) and np.all(np.isfinite(e["base"]))
    values = fm.candidate_values(sh, cand)
    law = wide_law(c, q, masks, target, values)
    xj = np.abs(e["joint"] - law["joint"]) / law["joint_band"]
    xb = np.abs(e["base"] - law["base"]) / law["base_band"]
    print("%s target %d: %d candidates, worst excursion / band: joint %.3f, "
          "base %.3f" % (name, target, len(values), xj.max(), xb.max()))
    assert xj.max() <= 1.0 and xb.max() <= 1.0
    # the planted variants leave the band the oracle is inside
    if not any(f >= 4 and f != target for f in range(F)):
        return              # (no feature >= 4 besides the target)
    for variant in xe.VARIANTS:
        drop = F - 2 if target == F - 1 else F - 1
        if variant == "drop" and drop < 4:
            continue        # (no feature >= 4 besides the target)
        st, qq = xe.planted_state(c.st, q, "wrap" if variant == "wrap"
                                  else "mask4")
        wrong = fm.law_f64([st], qq, xe.planted_mask(masks, variant, drop),
                           target, values, False)
        out = ((np.abs(wrong["joint"] - law["joint"])
                > law["joint_band"]).any(1)
               | (np.abs(wrong["base"] - law["base"]) > law["base_band"]))
        print("  %s: %.0f %% of the rows leave the band" % (
            variant, 100.0 * out.mean()))
        assert out.any(), variant


def test_wide_targets_cross_the_staging_tile():
    """the staged kernels' launch geometry, restated
    (eight_expect.staged_geometry): with NROWS query rows target 0 of the
    eight-feature list stages 11 planes of 32 rows, 1408 bytes a group and
    33 groups a tile -- two tiles at K = 43, three at K = 79; target 3
    eight planes and 47 groups a tile -- two tiles at K = 79; the
    ensemble's tile is taken from its largest K"""
    def geometry(kinds, sh, target, K):
        cand = fe.candidates_for(sh)
        C = len(fe.default_candidates(sh) if cand is None else cand)
        return xe.staged_geometry(kinds, target, C, K, NROWS)

    c, swept = xe.case("eight"), xe.case("eight_swept")
    kinds = [s.kind for s in c.osh]
    assert (c.K, swept.K) == (43, 79)
    g = geometry(kinds, c.osh[0], 0, c.K)
    assert (g["planes"], g["rows"], g["tile"]) == (11, 32, 33)
    assert xe.feature_lds(10, 0, 32) == 1408
    assert g["lds"] <= xe.FEATURE_LDS_BUDGET
    assert g["tiles"] >= 2
    assert geometry(kinds, c.osh[0], 0, swept.K)["tiles"] >= 3
    g = geometry(kinds, c.osh[3], 3, swept.K)
    assert (g["planes"], g["tile"], g["tiles"]) == (8, 47, 2)
    assert geometry(kinds, c.osh[7], 7, swept.K)["planes"] == 1
    ens = xe.eight3()
    ks = [m.K for m in ens.members]
    g = geometry(kinds, c.osh[0], 0, max(ks))
    assert g["tile"] == 33 and sorted(-(-k // g["tile"]) for k in ks) == [
        1, 2, 2]
