"""tests/marginals_expect.py against itself, without a GPU: the expectation
composed from the oracle lies inside the float64 bands, planted bugs leave
them, and the enumerated mutual information behaves as one; then the
composition dist_gibbs_relate_many is held to -- the oracle's marginals of
the oracle's own sample_rows_many rows -- is inside the bound the GPU test
uses, for the seed it uses."""
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
import oracle_lib as ol  # noqa: E402
import sample_many_expect as smx  # noqa: E402

LE2 = [dict(k=k, empty=1, alpha=1.0, d=0.0, sweeps=0) for k in (4, 17)]
# name: ensemble, masks
CASES = {
    "dd_bb_gp": (lambda: ee.Ensemble("dd_bb_gp", ee.SPECS3, nq=60),
                 lambda: mx.all_masks(3)),
    "gp_nich": (lambda: ee.Ensemble("gp_nich", ee.SPECS3, nq=60),
                lambda: mx.all_masks(2)),
    "le_m2": (lambda: ee.Ensemble("dd_bb_gp", LE2, le=2000, nq=60),
              lambda: mx.all_masks(3)),
    "eight": (lambda: mx.Ensemble8(nq=24), mx.eight_masks),
}
_DONE = {}

# the relate test's ensemble, seeds and sample size (tests/test_gpu_relate.py)
RELATE_SEED, RELATE_MEMBER_SEED, RELATE_BASE, RELATE_N = 7, 8, 1000, 20000


def case(name):
    """-> (ensemble, masks, expect_many, law, band)"""
    if name not in _DONE:
        ens = CASES[name][0]()
        masks = CASES[name][1]()
        le = ens.le is not None
        e = mx.expect_many([m.orc for m in ens.members], ens.qvals, masks, le)
        Lv, band = mx.law_f64([m.st for m in ens.members], ens.qvals, masks,
                              le)
        _DONE[name] = (ens, masks, e, Lv, band)
    return _DONE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_the_expectation_is_inside_the_float64_bands(name):
    ens, masks, e, Lv, band = case(name)
    finite = np.isfinite(Lv)
    exc = np.abs(e["logp"].astype(np.float64) - Lv)[finite] / band[finite]
    print("%s: M=%d, %d rows x %d masks: largest excursion %.3f of the band, "
          "band at most %.3g" % (name, ens.M, ens.nq, len(masks), exc.max(),
                                 band[finite].max()))
    assert finite.all()
    assert exc.max() <= 1.0


@pytest.mark.parametrize("name,variant", [
    ("dd_bb_gp", "mean_of_logs"), ("dd_bb_gp", "no_log_m"),
    ("le_m2", "unnormalised"), ("dd_bb_gp", "wrong_feature"),
    ("dd_bb_gp", "plus_zero_cat")])
def test_planted_bugs_leave_the_band(name, variant):
    ens, masks, e, Lv, band = case(name)
    bug, _ = mx.law_f64([m.st for m in ens.members], ens.qvals, masks,
                        ens.le is not None, variant)
    exc = np.abs(bug - Lv) / band
    print("%s / %s: the planted law is up to %.3g bands from the law"
          % (name, variant, exc.max()))
    assert exc.max() > 1.0


def test_mask_zero_is_the_prior_total_and_the_full_mask_is_predict():
    ens, masks, e, _, _ = case("dd_bb_gp")
    full = ens.expect()        # ensemble_expect's predict_many expectation
    s_full, s_zero = int(np.nonzero(masks == 7)[0][0]), \
        int(np.nonzero(masks == 0)[0][0])
    assert np.array_equal(e["w"][:, :, s_full].view(np.uint32),
                          full["w"].view(np.uint32))
    assert np.array_equal(e["logp"][:, s_full].view(np.uint32),
                          full["logp"].view(np.uint32))
    for i in range(ens.M):
        assert np.all(e["w"][i, :, s_zero].view(np.uint32)
                      == e["prior_totals"][i].view(np.uint32))


def test_the_enumerated_mutual_information_is_one():
    ens, _, _, _, _ = case("dd_bb_gp")
    states = [m.st for m in ens.members]
    law = mx.enumerate_pair(states, 0, 1, False)
    print("dd_bb_gp SPECS3, (DD, BB): mi %.6g, sigma %.6g, H(DD) %.6g, "
          "H(BB) %.6g, mass - 1 = %.3g" % (law["mi"], law["sigma"],
                                           law["h_i"], law["h_j"],
                                           law["mass"] - 1))
    assert abs(law["mass"] - 1) < 1e-9
    assert law["mi"] >= 0 and law["sigma"] > 0
    assert 0 < law["h_i"] <= np.log(8) and 0 < law["h_j"] <= np.log(2)
    for st in states:
        one = mx.enumerate_pair([st], 0, 1, False)
        assert one["mi"] >= 0
    # a member of one group is a product law
    alone = mx.enumerate_pair([mx.one_group_state()], 0, 1, False, slots=[0])
    assert abs(alone["mass"] - 1) < 1e-12
    assert abs(alone["mi"]) < 1e-12 and alone["sigma"] < 1e-6


def test_the_reference_composition_is_inside_the_relate_bound():
    """the oracle's marginals of the oracle's sample_rows_many rows, for the
    seed tests/test_gpu_relate.py fixes: (DD, BB) and the two entropies
    within 5 sigma / sqrt(n) of the enumerated law"""
    ens, _, _, _, _ = case("dd_bb_gp")
    L = ol.oracle()
    n = RELATE_N
    rows = smx.expect_many([m.orc for m in ens.members],
                           [m.gsh for m in ens.members], None, None,
                           L.orc_rng_seed(RELATE_SEED),
                           L.orc_rng_seed(RELATE_MEMBER_SEED), RELATE_BASE,
                           False, nq=n)["cols"]
    masks = np.array([1, 2, 3], np.uint32)
    e = mx.expect_many([m.orc for m in ens.members], [rows[0], rows[1], None],
                       masks, False, nq=n)
    lp = e["logp"].astype(np.float64)
    d = lp[:, 2] - lp[:, 0] - lp[:, 1]
    law = mx.enumerate_pair([m.st for m in ens.members], 0, 1, False)
    root = np.sqrt(n)
    print("n=%d: mi %.6g against %.6g (%.2f sigma), H(DD) %.6g against %.6g "
          "(%.2f), H(BB) %.6g against %.6g (%.2f); stderr %.4g against %.4g"
          % (n, d.mean(), law["mi"],
             (d.mean() - law["mi"]) / law["sigma"] * root,
             -lp[:, 0].mean(), law["h_i"],
             (-lp[:, 0].mean() - law["h_i"]) / law["sigma_i"] * root,
             -lp[:, 1].mean(), law["h_j"],
             (-lp[:, 1].mean() - law["h_j"]) / law["sigma_j"] * root,
             d.std(ddof=1) / root, law["sigma"] / root))
    assert abs(d.mean() - law["mi"]) <= 5 * law["sigma"] / root
    assert abs(-lp[:, 0].mean() - law["h_i"]) <= 5 * law["sigma_i"] / root
    assert abs(-lp[:, 1].mean() - law["h_j"]) <= 5 * law["sigma_j"] / root
    assert abs(d.std(ddof=1) / law["sigma"] - 1) <= 0.1
