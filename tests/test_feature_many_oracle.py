"""The expectation dist_gibbs_predict_feature_many is held to
(tests/feature_many_expect.py: feature_expect.expect per member,
ensemble_expect.fold over the members, the choice from the FOLDED joint) must
itself be right before the GPU is compared with it bit for bit
(tests/test_gpu_predict_feature_many.py):

  * its joint and base lie inside the derived float64 bands around
    log (1/M) sum_e p(x_t, x_obs | e) and log (1/M) sum_e p(x_obs | e), at
    M = 3 under random per-row masks: a DD, a BB and a GP target on the mixed
    list dd_bb_gp, a NICH target on gp_nich, DD alone, DPD with OTHER among
    the candidates, LowEntropy dd;
  * the ensemble's conditional sums to one over a DD's or BB's whole domain;
  * planted bugs -- the mean of the members' conditionals, the mean of the
    logs, the missing - log M, LowEntropy without the members' own
    normalisation -- leave the band on every asserted row;
  * 20 000 draws of `choice` follow the float64 conditional of the folded
    law, 20 000 draws of `member` the responsibilities exp(B_e - base) / M
    (chi-squared, p > 1e-4);
  * for M = 1 it is feature_expect.expect, bit for bit (minus the prior total
    under LowEntropy).
"""
import numpy as np
import pytest
from scipy import stats

import eight_expect as xe
import ensemble_expect as ee
import feature_expect as fe
import feature_many_expect as fm
import oracle_lib as ol
from test_ensemble_oracle import FAR_LE_SPECS3, FAR_SPECS3, LE_SPECS3
# (the entry point this expectation describes: without it there is nothing
# to hold, and this module does not load)
from distributions_amd.engine import predict_feature_many  # noqa: F401

NQ = 80
MASK_SEED = 11

# name: config, target, LowEntropy dataset size, members, candidates
CASES = {
    "mixed_dd": ("dd_bb_gp", 0, None, ee.SPECS3, None),
    "mixed_bb": ("dd_bb_gp", 1, None, ee.SPECS3, None),
    "mixed_gp": ("dd_bb_gp", 2, None, ee.SPECS3, fe.COUNT_CANDIDATES),
    "gp_nich_nich": ("gp_nich", 1, None, ee.SPECS3, fe.REAL_CANDIDATES),
    "dd": ("dd", 0, None, ee.SPECS3, None),
    "dpd_other": ("dpd_other", 0, None, ee.SPECS3,
                  [0, 3, 49, fe.OTHER, 77]),     # 77: not in the table, OTHER
    "le_dd": ("dd", 0, 2000, LE_SPECS3, None),
    # the planted bugs' members, further apart (test_ensemble_oracle's)
    "far_mixed_dd": ("dd_bb_gp", 0, None, FAR_SPECS3, None),
    "far_mixed_gp": ("dd_bb_gp", 2, None, FAR_SPECS3, fe.COUNT_CANDIDATES),
    "far_gp_nich": ("gp_nich", 1, None, FAR_SPECS3, fe.REAL_CANDIDATES),
    "farle_mixed_dd": ("dd_bb_gp", 0, 3000, FAR_LE_SPECS3, None),
    "farle_gp_nich": ("gp_nich", 0, 3000, FAR_LE_SPECS3,
                      fe.COUNT_CANDIDATES),
}
_FENS = {}


def case(name):
    if name not in _FENS:
        config, target, le, specs, cand = CASES[name]
        other = (1, 2) if config == "dpd_other" else ()
        ens = ee.Ensemble(config, specs, nq=NQ, le=le, other=other)
        sh = ens.members[0].osh[target]
        if cand is not None:
            cand = np.array(cand, np.float32 if sh.kind == ol.NICH
                            else np.uint32)
        masks = fe.random_masks(NQ, len(ens.members[0].osh), MASK_SEED)
        _FENS[name] = fm.FeatureEnsemble(ens, target, cand, masks)
    return _FENS[name]


def observes_something(fens):
    """rows whose mask observes at least one feature besides the target"""
    ob = fens.observed.astype(np.int64) & ((1 << fens.F) - 1)
    return (ob & ~(1 << fens.target)) != 0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


BAND_NAMES = ["mixed_dd", "mixed_bb", "mixed_gp", "gp_nich_nich", "dd",
              "dpd_other", "le_dd"]


@pytest.mark.parametrize("name", BAND_NAMES)
def test_expectation_is_in_the_float64_band(name):
    fens = case(name)
    e, law = fens.expect(), fens.f64()
    assert e["wj"].shape == (3, NQ, fens.C) and e["wb"].shape == (3, NQ)
    assert np.all(np.isfinite(e["joint"])) and np.all(np.isfinite(e["base"]))
    xj = np.abs(e["joint"] - law["joint"]) / law["joint_band"]
    xb = np.abs(e["base"] - law["base"]) / law["base_band"]
    print("%s: K = %s, %d rows x %d candidates; worst excursion / band: "
          "joint %.3f, base %.3f (joint band %.2e .. %.2e)" % (
              name, [m.K for m in fens.ens.members], NQ, fens.C, xj.max(),
              xb.max(), law["joint_band"].min(), law["joint_band"].max()))
    assert xj.max() <= 1.0 and xb.max() <= 1.0, name


@pytest.mark.parametrize("name", ["mixed_dd", "mixed_bb", "dd", "le_dd"])
def test_the_ensemble_conditional_sums_to_one(name):
    """over the whole domain of a DD or BB target: logsumexp_c(joint) - base
    is within the summed bands of 0 (the log-sum-exp over the candidates moves
    by at most the largest of their bands)"""
    fens = case(name)
    assert fens.cand is None
    e, law = fens.expect(), fens.f64()

    def lse(x):
        m = x.max(1)
        return np.log(np.exp(x - m[:, None]).sum(1)) + m

    # the float64 law itself: every member's predictive is normalised
    assert np.abs(lse(law["joint"]) - law["base"]).max() < 1e-9
    got = lse(e["joint"].astype(np.float64)) - e["base"]
    band = law["joint_band"].max(1) + law["base_band"]
    print("%s: worst |logsumexp_c(joint) - base| / band %.3f" % (
        name, (np.abs(got) / band).max()))
    assert np.all(np.abs(got) <= band)


@pytest.mark.parametrize("name,variant", [
    ("far_mixed_dd", "mean_of_conditionals"),
    ("far_mixed_gp", "mean_of_conditionals"),
    ("farle_mixed_dd", "mean_of_conditionals"),
    ("far_mixed_dd", "mean_of_logs"), ("far_gp_nich", "mean_of_logs"),
    ("far_mixed_dd", "no_log_m"), ("far_gp_nich", "no_log_m"),
    ("farle_mixed_dd", "no_log_m"),
    ("farle_mixed_dd", "unnormalised"), ("farle_gp_nich", "unnormalised")])
def test_planted_bug_leaves_the_band(name, variant):
    """A row leaves the band when its farthest candidate does: the distance
    of a row is the largest over its candidates of |wrong - law| / band.

    mean_of_conditionals is held on the conditional joint - base (band: the
    two bands summed) and asserted on the rows whose mask observes at least
    one feature besides the target -- the rows where the members' weights
    p(e | x_obs) are in play, 61 and 62 of the 80 here.  The others are not
    asserted: with nothing observed the variant differs from the law only
    through the members' disagreement about the target's marginal, which is
    not what it is about.  no_log_m and unnormalised are held on joint and on
    base, every row asserted (- log M and the prior totals shift every
    value).  mean_of_logs is held on joint, every row asserted; on base it is
    only reported: where a mask observes nothing, or only cells the members
    agree on, the members' base values coincide and the mean of the logs IS
    the log of the mean (PitmanYor's prior total is 0 in every member)."""
    fens = case(name)
    law = fens.f64()
    e = fens.expect()
    assert (np.abs(e["joint"] - law["joint"]) / law["joint_band"]).max() <= 1
    wrong = fm.law_f64([m.st for m in fens.ens.members], fens.ens.qvals,
                       fens.observed, fens.target, fens.values, fens.le,
                       variant)
    if variant == "mean_of_conditionals":
        rows = observes_something(fens)
        assert rows.mean() >= 0.5
        x = (np.abs(wrong["cond"] - law["cond"]) / law["cond_band"]).max(1)
        print("%s, %s: %d of %d rows asserted; least distance / band %.1f, "
              "median %.1f" % (name, variant, rows.sum(), NQ, x[rows].min(),
                               np.median(x[rows])))
        assert np.all(x[rows] > 1.0)
        return
    xj = (np.abs(wrong["joint"] - law["joint"]) / law["joint_band"]).max(1)
    xb = np.abs(wrong["base"] - law["base"]) / law["base_band"]
    print("%s, %s: every row asserted; least distance / band: joint %.1f, "
          "base %.1f" % (name, variant, xj.min(), xb.min()))
    assert np.all(xj > 1.0)
    assert variant == "mean_of_logs" or np.all(xb > 1.0)


def chi_square(observed, expected):
    """over cells of expected count >= 50, the rest pooled (as
    test_ensemble_oracle does)"""
    observed = observed.astype(np.float64)
    small = expected < 50
    if small.any():
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
    assert len(expected) >= 2, "one cell tests nothing"
    return stats.chisquare(observed, expected) + (observed, expected)


@pytest.mark.parametrize("name", ["mixed_dd", "mixed_gp", "farle_mixed_dd"])
def test_choice_draws_follow_the_float64_conditional(name):
    """one row's folded joint 20 000 times: draw q uses engine step
    draw_base + q + 1, so the draws differ"""
    fens = case(name)
    e, law = fens.expect(), fens.f64()
    q = int(np.nonzero(observes_something(fens))[0][0])
    n = 20000
    joint = np.repeat(e["joint"][q:q + 1], n, axis=0)
    draw, first = fm.choice_of(joint, ol.oracle().orc_rng_seed(20240601), 0)
    p = np.exp(law["joint"][q] - law["joint"][q].max())
    p /= p.sum()
    chi2, pvalue, o, x = chi_square(np.bincount(draw, minlength=fens.C),
                                    p * n)
    print("%s row %d: conditional %s, cells %s / %s, chi2 %.2f, p %.4f" % (
        name, q, np.round(p, 4), o, np.round(x, 1), chi2, pvalue))
    assert pvalue > 1e-4
    assert len(set(first.tolist())) == 1 and first[0] == int(np.argmax(p))


@pytest.mark.parametrize("name", ["mixed_dd", "mixed_gp", "farle_mixed_dd"])
def test_member_draws_follow_the_float64_responsibilities(name):
    """among the rows that observe something (with nothing observed the
    members tie), the one whose least likely member is the most likely,
    20 000 times"""
    fens = case(name)
    e, law = fens.expect(), fens.f64()
    r = law["r"]
    q = int(np.argmax(np.where(observes_something(fens), r.min(1), -1.0)))
    n = 20000
    wb = np.repeat(e["wb"][:, q:q + 1], n, axis=1)
    _, draw, first = ee.fold(wb, ol.oracle().orc_rng_seed(20240601), 0)
    chi2, pvalue, o, x = chi_square(np.bincount(draw, minlength=fens.M),
                                    r[q] * n)
    print("%s row %d: responsibilities %s, cells %s / %s, chi2 %.2f, p %.4f"
          % (name, q, np.round(r[q], 4), o, np.round(x, 1), chi2, pvalue))
    assert pvalue > 1e-4
    assert len(set(first.tolist())) == 1 and first[0] == int(np.argmax(r[q]))


@pytest.mark.parametrize("name", ["mixed_dd", "gp_nich_nich", "le_dd"])
def test_one_member_is_predict_feature_itself(name):
    fens = case(name)
    L = ol.oracle()
    seed, mseed = L.orc_rng_seed(fm.DRAW_SEED), L.orc_rng_seed(fm.MEMBER_SEED)
    assert L.orc_fast_log(1.0) == 0.0 and L.orc_fast_exp(0.0) == 1.0
    for m in fens.ens.members:
        one = fm.expect_many([m.orc], fens.ens.qvals, fens.observed,
                             fens.target, fens.cand, seed, mseed,
                             fm.DRAW_BASE, fens.le)
        p = fe.expect(m.orc, fens.ens.qvals, fens.observed, fens.target,
                      fens.cand, seed, fm.DRAW_BASE)
        wj, wb = p["joint"], p["base"]
        if fens.le:
            total = fm.prior_total(m.orc)
            wj = (wj - total).astype(np.float32)
            wb = (wb - total).astype(np.float32)
            # the choice is then taken from the shifted values
            draw, first = fm.choice_of(wj, seed, fm.DRAW_BASE)
        else:
            draw, first = p["draw"], p["map"]
        assert np.array_equal(bits(one["joint"]), bits(wj))
        assert np.array_equal(bits(one["base"]), bits(wb))
        assert np.array_equal(one["choice_draw"], draw)
        assert np.array_equal(one["choice_map"], first)
        assert np.all(one["member_draw"] == 0)
        assert np.all(one["member_map"] == 0)


# ---------------------------------------------------------------------------
# the eight-feature ensemble of tests/eight_expect.py


def eight3_case(target, n):
    ens = xe.eight3()
    sh = ens.members[0].osh[target]
    cand = fe.candidates_for(sh)
    key = ("eight3", target, n)
    if key not in _FENS:
        f = fm.FeatureEnsemble(ens, target, cand,
                               xe.masks_for(n, 8, MASK_SEED + target))
        f.nq = n
        _FENS[key] = f
    return _FENS[key]


@pytest.mark.parametrize("target", xe.TARGETS8)
def test_eight3_joint_and_base_are_in_the_float64_band(target):
    """every candidate on every one of the first n held-out rows (n = 40;
    12 for DD70's 70 candidates, 20 for DPD's 21) under random and fixed
    masks; the GPU test holds all 100 rows of targets 0, 3 and 7; the planted
    variants (a feature >= 4 never observed, feature f's words from feature
    f & 3, the mask through & 0xF) leave the band"""
    # (DD70's 70 candidates on the rows of the fixed masks alone, DPD's 21
    # on half the rows)
    n = {4: 12, 6: 20}.get(target, 40)
    fens = eight3_case(target, n)
    ens = fens.ens
    q = [v[:n] for v in ens.qvals]
    L = ol.oracle()
    e = fm.expect_many([m.orc for m in ens.members], q, fens.observed,
                       target, fens.cand, L.orc_rng_seed(fm.DRAW_SEED),
                       L.orc_rng_seed(fm.MEMBER_SEED), fm.DRAW_BASE, False)
    states = [m.st for m in ens.members]
    law = fm.law_f64(states, q, fens.observed, target, fens.values, False)
    assert np.all(np.isfinite(e["joint"])) and np.all(np.isfinite(e["base"]))
    xj = np.abs(e["joint"] - law["joint"]) / law["joint_band"]
    xb = np.abs(e["base"] - law["base"]) / law["base_band"]
    print("eight3 target %d: %d rows x %d candidates; worst excursion / "
          "band: joint %.3f, base %.3f" % (target, n, fens.C, xj.max(),
                                           xb.max()))
    assert xj.max() <= 1.0 and xb.max() <= 1.0
    for variant in xe.VARIANTS:
        drop = 6 if target == 7 else 7
        qq = xe.planted_state(states[0], q, "wrap" if variant == "wrap"
                              else "mask4")[1]
        wrong = fm.law_f64(states, qq,
                           xe.planted_mask(fens.observed, variant, drop),
                           target, fens.values, False)
        out = ((np.abs(wrong["joint"] - law["joint"])
                > law["joint_band"]).any(1)
               | (np.abs(wrong["base"] - law["base"]) > law["base_band"]))
        print("  %s: %.0f %% of the rows leave the band" % (
            variant, 100.0 * out.mean()))
        assert out.any(), variant
