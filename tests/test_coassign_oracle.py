"""The expectation dist_gibbs_coassign[_many] is held to
(tests/coassign_expect.py: oracle scores, scores_to_likelihoods, float32
responsibilities, libm's fmaf chain) against the float64 law
C64 = (1/M) sum_e p_e p_e^T within its derived band; planted bugs leave the
band; pairs of independent oracle draws agree with the law.  The GPU is held
to the expectation bit for bit (tests/test_gpu_coassign.py).

Largest |expectation - C64| / C64 over the specified cells, as printed by
test_expectation_is_within_the_band_of_the_law: see DESIGN.md 4.17.
"""
import ctypes

import numpy as np
import pytest

import coassign_expect as ce
import oracle_lib as ol


def excursion(got, sub, sym):
    C, band = sub.law(sym)
    mask = sub.mask(sym)
    with np.errstate(all="ignore"):
        return (np.abs(np.asarray(got, np.float64) - C) / band)[mask]


@pytest.mark.parametrize("name", ce.NAMES)
@pytest.mark.parametrize("sym", [True, False])
def test_expectation_is_within_the_band_of_the_law(name, sym):
    sub = ce.subject(name)
    want = sub.expect(sym)
    C, band = sub.law(sym)
    mask = sub.mask(sym)
    assert mask.any()
    assert np.isfinite(want[mask]).all() and np.isfinite(band[mask]).all()
    exc = excursion(want, sub, sym)
    rel = (np.abs(want.astype(np.float64) - C) / C)[mask]
    soft = mask & (want > 0) & (want < ce.UNDERFLOW)
    print("%s sym=%d: worst excursion %.3g of the band, largest relative "
          "distance %.3g, smallest cell %.3g, cells near underflow %d"
          % (name, sym, exc.max(), rel.max(), want[mask].min(), soft.sum()))
    assert exc.max() <= 1.0
    assert soft.sum() <= ce.UNDERFLOW_SHARE * mask.sum()


@pytest.mark.parametrize("name", ce.NAMES)
def test_symmetric_with_a_diagonal_in_0_1(name):
    sub = ce.subject(name)
    want = sub.expect(True)
    assert np.array_equal(want.view(np.uint32), want.T.view(np.uint32))
    diag = np.diag(want)[sub.specified(sub.rq)]
    assert (diag > 0).all() and (diag <= 1).all()
    # the rectangular call is not the square one's corner
    assert sub.expect(False).shape == (len(sub.rq), len(sub.rt))


def planted(sub, variant, sym=False):
    counts = [np.asarray(m.orc.counts()) for m in sub.members]
    C, _ = ce.law_f64([m.st for m in sub.members], sub.cols(sub.rq),
                      sub.cols(sub.rq if sym else sub.rt), variant, counts)
    return C


@pytest.mark.parametrize("name", ["dd", "gp_nich", "only_empty_k3",
                                  "ens3_dd_bb_gp", "ens3_gp_nich"])
def test_planted_bugs_leave_the_band(name):
    sub = ce.subject(name)
    variants = ["unnormalised", "hard"]
    # dropping the empty groups moves a cell by about the new-group mass,
    # alpha / (n + alpha) = 5e-4 at alpha = 1 and 2000 rows: visible against
    # DirichletDiscrete's band (relative 2e-5), not against the score bands
    # of GammaPoisson + NormalInverseChiSq (relative 5e-2), alone or in an
    # ensemble
    if "gp_nich" not in name:
        variants.append("no_empty")
    if sub.M > 1:
        variants.append("no_mean")
    for v in variants:
        exc = excursion(planted(sub, v), sub, False)
        assert exc.max() > 1.0, (name, v, exc.max())
    # the output of a rectangular call written transposed: the [n_t, n_q]
    # matrix read as [n_q, n_t] (with only empty groups every cell is 1 / K:
    # nothing tells a transpose there)
    if name == "only_empty_k3":
        return
    C, _ = sub.law(False)
    swapped = np.ascontiguousarray(C.T).reshape(C.shape)
    assert excursion(swapped, sub, False).max() > 1.0


@pytest.mark.parametrize("name", ["dd", "gp_nich_swept", "ens3_gp_nich"])
def test_another_order_of_the_exp_sum_stays_inside(name):
    sub = ce.subject(name)
    rows = np.concatenate([sub.rq, sub.rt])
    r = [ce.responsibilities(s[rows], reverse_sum=True) for s in sub.scores()]
    n = len(sub.rq)
    other = ce.chain([x[:n][:24] for x in r], [x[n:] for x in r], False)
    C, band = sub.law(False)
    mask = sub.mask(False)[:24]
    exc = (np.abs(other.astype(np.float64) - C[:24]) / band[:24])[mask]
    assert exc.max() <= 1.0


@pytest.mark.parametrize("name", ["dd", "gp_nich", "le_dd", "only_empty_k3",
                                  "ens3_dd_bb_gp"])
def test_pairs_of_independent_draws_agree_with_the_law(name):
    """20 000 pairs of orc_sample_from_scores_overwrite draws, the engine
    uniform, the two draws independent: the share of equal slots against C64
    at 4.5 binomial sigma"""
    sub = ce.subject(name)
    L = ol.oracle()
    C, _ = sub.law(False)
    scores = sub.scores()
    ok = np.argwhere(sub.mask(False))
    pick = np.random.default_rng(5)
    N = 20000
    for a, b in ok[pick.choice(len(ok), 3, replace=False)]:
        qa, qb = sub.rq[a], sub.rt[b]
        member = pick.integers(0, sub.M, N)
        st = ctypes.c_uint32(L.orc_rng_seed(1000 + int(a) * 131 + int(b)))
        hits = 0
        for e in range(sub.M):
            sa = np.ascontiguousarray(scores[e][qa], np.float32)
            sb = np.ascontiguousarray(scores[e][qb], np.float32)
            K = len(sa)
            for _ in range(int((member == e).sum())):
                ga = L.orc_sample_from_scores_overwrite(ctypes.byref(st), K,
                                                        sa.copy())
                gb = L.orc_sample_from_scores_overwrite(ctypes.byref(st), K,
                                                        sb.copy())
                hits += ga == gb
        # (engine uniform, then equal with that engine's probability: each
        # pair is one Bernoulli(C64) trial)
        p = float(C[a, b])
        sigma = np.sqrt(max(p * (1 - p), 1e-12) / N)
        assert abs(hits / N - p) <= 4.5 * sigma + 1e-9, (a, b, hits / N, p)


@pytest.mark.parametrize("variant", ["drop", "wrap"])
@pytest.mark.parametrize("name", ce.WIDE)
def test_wide_planted_variants_leave_the_band(name, variant):
    """eight features: a law without feature 7, or with feature f's words
    taken from feature f & 3, is outside the band on some cell"""
    import eight_expect as xe
    sub = ce.subject(name)
    planted = [xe.planted_state(m.st, sub.qvals, variant)
               for m in sub.members]
    cols = planted[0][1]
    C, _ = ce.law_f64([p[0] for p in planted],
                      [np.ascontiguousarray(c[sub.rq]) for c in cols],
                      [np.ascontiguousarray(c[sub.rt]) for c in cols])
    exc = excursion(C, sub, False)
    print("%s, %s: %.0f %% of the cells leave the band" % (
        name, variant, 100.0 * (exc > 1.0).mean()))
    assert exc.max() > 1.0
