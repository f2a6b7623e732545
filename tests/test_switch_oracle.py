"""The expectation the held-out readers are held to AFTER a hyper-parameter
step (tests/switch_expect.py: the case's oracle state adopted by an oracle
created with the new values) must itself be right, and must be able to tell a
reader that kept part of the old hyper-parameters from one that did not,
before the GPU is compared with it bit for bit
(tests/test_gpu_switch_readers.py).

a. Under every row of switch_expect.SWITCHES the existing expectations lie
   inside the existing derived float64 bands (condition <= 1.0, unchanged):
   predict_expect.expect's logp in predict_expect.logp_f64's; the chain of
   coassign_expect.responsibilities in coassign_expect.law_f64's (40 x 25
   rows, cells near underflow at most UNDERFLOW_SHARE); marginals_expect's
   in its law_f64's (60 rows, every subset of the features); and
   feature_expect.expect's base in base_f64's for the lists of more than one
   feature.
b. A stale reader is seen: on the same adopted state, the oracle that kept
   every old value, only the old clustering, or only feature f's old value
   gives a logp that differs in bits from the switched one in at least half
   of the rows where both are finite, and leaves the switched band in at
   least one row.  One stated exception: only_empty_k3 with the clustering
   old -- three empty groups score alike under either PitmanYor, the
   normalised prior keeps logp inside the band, and only the bits are
   asserted there.

Measured (printed by the tests), worst excursion / band:
  case              logp   coassign  marginals  base
  gp_nich_swept     0.393  0.029     0.570      0.583, 0.016
  bnb_swept         0.050  0.010     0.360      -
  bb_swept          0.789  0.011     0.481      -
  dd_bb_gp_swept    0.118  0.022     0.568      0.060, 0.082, 0.538
  dpd_other_swept   0.532  0.110     0.362      -
  dpd_swept         0.940  0.146     0.621      -
  le_gp_nich        0.409  0.006     0.707      0.688, 0.312
  only_empty_k3     0.443  0.000     0.277      0.396, 0.465
  dd256_k1025       0.414  0.041     0.311      -
(logp over all held-out rows; marginals over the first 60 rows and every
subset of the features, the empty one included; base per target over the
first 48 rows.)  Cells near underflow: 0 in every case.
Stale variants: every row differs in bits from the switched expectation, in
every variant of every case.  Rows outside the switched band, of 300 (256
for dd256_k1025):
  gp_nich_swept     all old 164; clustering old 2; feature 0 old 166;
                    feature 1 old 59
  bnb_swept         all old 300; clustering old 12; feature 0 old 300
  bb_swept          all old 300; clustering old 300; feature 0 old 300
  dd_bb_gp_swept    all old 231; clustering old 3; feature 0 old 196;
                    feature 1 old 53; feature 2 old 206
  dpd_other_swept   all old 300; clustering old 297; feature 0 old 300
  dpd_swept         all old 296; clustering old 295; feature 0 old 300
  le_gp_nich        all old 276; feature 0 old 244; feature 1 old 271
  only_empty_k3     all old 300; clustering old 0 (the exception);
                    feature 0 old 300; feature 1 old 300
  dd256_k1025       all old 256; clustering old 58; feature 0 old 256
(The bands of GammaPoisson and NormalInverseChiSq scores are wide, 5e-2
relative: an old clustering model alone moves few of their rows out.)
"""
import numpy as np
import pytest

import coassign_expect as ce
import feature_expect as fe
import marginals_expect as mx
import oracle_lib as ol
import predict_expect as pe
import switch_expect as sx

_SW = {}


def switched(name):
    if name not in _SW:
        _SW[name] = sx.switched(name)
    return _SW[name]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def seed_state():
    return ol.oracle().orc_rng_seed(pe.DRAW_SEED)


@pytest.mark.parametrize("name", list(sx.SWITCHES))
def test_the_switched_state_is_the_cases_under_other_values(name):
    sw = switched(name)
    c = sw.case
    assert sw.K == c.K
    assert np.array_equal(sw.orc.counts(), c.orc.counts())
    assert np.array_equal(sw.orc.assign, c.orc.assign)
    for k in range(c.K):
        assert sw.orc.packed_to_global(k) == c.orc.packed_to_global(k)
    for f in range(len(c.osh)):
        for k in sorted({0, c.K // 2, c.K - 1}):
            assert np.array_equal(sw.orc.get_group(f, k),
                                  c.orc.get_group(f, k))
    # adopting under the OLD values gives back the case's own expectation
    same = sx.Switched(c, list(zip(c.osh, c.gsh)), None)
    e = pe.expect(same.orc, c.qvals, seed_state(), pe.DRAW_BASE)
    assert np.array_equal(bits(e["logp"]), bits(c.expect()["logp"]))
    assert np.array_equal(e["draw"], c.expect()["draw"])


@pytest.mark.parametrize("name", list(sx.SWITCHES))
def test_switched_logp_is_in_the_float64_band(name):
    sw = switched(name)
    e = sw.expect()
    assert e["scores"].shape == (sw.nq, sw.K)
    assert np.all(np.isfinite(e["logp"]))
    x = pe.excursion(e["logp"], sw)
    print("%s: K=%d, %d held-out rows; logp worst excursion / band %.3f"
          % (name, sw.K, sw.nq, x.max()))
    assert x.max() <= 1.0, name


@pytest.mark.parametrize("name", list(sx.SWITCHES))
def test_switched_coassignment_is_in_the_band_of_the_law(name):
    sw = switched(name)
    rq, rt = np.arange(40), np.arange(100, 125)
    s = sw.expect()["scores"]
    r = ce.responsibilities(s[np.concatenate([rq, rt])])
    want = ce.chain([r[:40]], [r[40:]], False)
    cols = [np.ascontiguousarray(c[rq]) for c in sw.qvals]
    tcols = [np.ascontiguousarray(c[rt]) for c in sw.qvals]
    C, band = ce.law_f64([sw.st], cols, tcols)
    assert np.isfinite(want).all() and np.isfinite(band).all()
    exc = np.abs(want.astype(np.float64) - C) / band
    soft = (want > 0) & (want < ce.UNDERFLOW)
    print("%s: 40 x 25 cells; co-assignment worst excursion / band %.3f, "
          "cells near underflow %d" % (name, exc.max(), int(soft.sum())))
    assert exc.max() <= 1.0
    assert soft.sum() <= ce.UNDERFLOW_SHARE * want.size


@pytest.mark.parametrize("name", list(sx.SWITCHES))
def test_switched_marginals_are_in_the_band_of_the_law(name):
    sw = switched(name)
    q = [c[:60] for c in sw.qvals]
    masks = mx.all_masks(len(sw.osh))
    le = sw.le is not None
    e = mx.expect_many([sw.orc], q, masks, le)
    Lv, band = mx.law_f64([sw.st], q, masks, le)
    assert np.isfinite(Lv).all()
    exc = np.abs(e["logp"].astype(np.float64) - Lv) / band
    print("%s: 60 rows x %d masks; marginals worst excursion / band %.3f"
          % (name, len(masks), exc.max()))
    assert exc.max() <= 1.0


@pytest.mark.parametrize("name", [n for n in sx.SWITCHES
                                  if len(sx.SWITCHES[n][0]()) > 1])
def test_switched_base_is_in_the_band_of_the_marginal(name):
    sw = switched(name)
    q = [c[:48] for c in sw.qvals]
    worst = []
    for target, sh in enumerate(sw.osh):
        cand = fe.candidates_for(sh)
        e = fe.expect(sw.orc, q, None, target, cand, seed_state(),
                      pe.DRAW_BASE)
        Lb, band = fe.base_f64(sw.st, q, target)
        x = np.abs(e["base"].astype(np.float64) - Lb) / band
        worst.append(x.max())
        assert x.max() <= 1.0, (name, target)
    print("%s: base worst excursion / band per target %s"
          % (name, ", ".join("%.3f" % w for w in worst)))


@pytest.mark.parametrize("name", list(sx.SWITCHES))
def test_a_stale_reader_differs_in_bits_and_leaves_the_band(name):
    sw = switched(name)
    want = sw.expect()["logp"]
    Lv, band, _ = sw.f64()
    for what, orc in sx.stale_variants(sw).items():
        with np.errstate(all="ignore"):
            got = pe.expect(orc, sw.qvals, seed_state(),
                            pe.DRAW_BASE)["logp"]
            finite = np.isfinite(got) & np.isfinite(want)
            differ = int((bits(got) != bits(want))[finite].sum())
            outside = int((np.abs(got.astype(np.float64) - Lv)
                           > band)[finite].sum())
        print("%s, %s: of %d finite rows %d differ in bits, %d lie outside "
              "the switched band" % (name, what, int(finite.sum()), differ,
                                     outside))
        assert finite.sum() * 2 >= len(want), (name, what)
        assert differ * 2 >= finite.sum(), (name, what)
        if (name, what) != ("only_empty_k3", "clustering old"):
            assert outside >= 1, (name, what)
