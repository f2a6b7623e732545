"""The expectation dist_gibbs_sample_rows_many is held to
(tests/sample_many_expect.py: the members' `base` folds, ensemble_expect.fold
for the member, sample_expect's group draw and dist_group_sample_value's cells
on the chosen member) must itself be right before the GPU is compared with it
bit for bit (tests/test_gpu_sample_rows_many.py):

  * at M = 3, 10^5 composed draws of ONE query row under ONE mask follow the
    float64 law  sum_e p(e | x_obs) sum_k p(k | x_obs, e) prod_f p(x_f | k, e)
    of its unobserved cells (p > 1e-4): on the discrete list dd_bb_gp a
    chi-square over the joint cells (the count cut off and the cells merged to
    an expected count >= 50), on gp_nich Kolmogorov-Smirnov for the real;
  * the same histograms reject three planted laws (p < 1e-6): the member drawn
    uniformly whatever is observed, the member drawn once per call, the cells
    drawn from their per-cell marginals (the group redrawn per cell);
  * its wb, base and member are feature_many_expect's for a target no row
    observes;
  * for M = 1 it is sample_expect's expectation.

The members are ensemble_expect's FAR members (100, 600 and 1500 rows; K = 5,
20 and 43; alpha 1, 20 and 5; hyper-parameters scaled per member) on tables
shaped by sample_many_expect.shape_rows: on workloads.make's own columns every
member and every group predicts the same cells, and no planted law is another
law.  Whether each planted law IS another law for a row and a mask is checked
here, before anything is drawn, by the chi-square's noncentrality (or the
distance of the CDFs): see `LAWS`.
"""
import numpy as np
import pytest
from scipy import stats

import eight_expect as xe
import ensemble_expect as ee
import feature_expect as fe
import feature_many_expect as fm
import marginals_expect as mx
import oracle_lib as ol
import sample_expect as sx
import sample_many_expect as sm
from test_ensemble_oracle import FAR_SPECS3
# (the entry point this expectation describes: without it there is nothing
# to hold, and this module does not load)
from distributions_amd.engine import sample_rows_many  # noqa: F401

N = 100000
GP_CELLS = 24                        # counts 0 .. 23, then one cell beyond
NICH_EDGES = np.linspace(-7.0, 5.0, 25)
# the least noncentrality n sum (p - q)^2 / q a planted law q must have under
# the law p, over the merged cells, before its rejection is asserted: the
# statistic is then about df + 400 +- 2 sqrt(df + 800) against a 1e-6
# quantile of about df + 5 sqrt(2 df) + 25 -- beyond it for every df here
NCP_MIN = 400.0
# ... and the least distance of the CDFs for Kolmogorov-Smirnov: 1e-6 is at
# 0.0086 for 10^5 draws, whose own scatter is 0.004
KS_MIN = 0.02

# name: config, the query row, its mask, the planted laws that are another
# law there (asserted; the others are reported):
#   uniform  needs the members' p(e | x_obs) far from 1/3: something observed
#            that the members disagree about.  With nothing observed it IS the
#            law under PitmanYor (every member's prior total is 0)
#   once     the law of one member alone, for each of the three
#   percell  needs two unobserved cells that depend on each other through the
#            group; with one unobserved cell it IS the law
#            (the BB cell alone says little about the member, the members'
#            BB columns being alike: 38 against the 400 asked for, reported)
LAWS = {
    "mixed_bb_seen": ("dd_bb_gp", [0, 1, 0], 0b010, ("once", "percell")),
    "mixed_gp_seen": ("dd_bb_gp", [0, 0, 11], 0b100,
                      ("uniform", "once", "percell")),
    "mixed_dd_seen": ("dd_bb_gp", [5, 0, 0], 0b001,
                      ("uniform", "once", "percell")),
    "real_gp_seen": ("gp_nich", [11, 0.0], 0b01, ("uniform", "once")),
    "real_nich_seen": ("gp_nich", [0, -2.5], 0b10, ("uniform", "once")),
    "real_nothing_seen": ("gp_nich", [0, 0.0], 0b00, ("once", "percell")),
}
_ENS = {}
_DRAWS = {}


def ensemble(config):
    if config not in _ENS:
        _ENS[config] = sm.ShapedEnsemble(config, FAR_SPECS3)
    return _ENS[config]


def row_of(config, values, n):
    osh = ensemble(config).members[0].osh
    return [np.full(n, v, np.float32 if s.kind == ol.NICH else np.uint32)
            for s, v in zip(osh, values)]


class Case(object):
    """one row under one mask: the float64 law over the joint cells of its
    unobserved features and the planted laws"""

    def __init__(self, name):
        self.name = name
        self.config, self.values, self.ob, self.asserted = LAWS[name]
        self.ens = ensemble(self.config)
        osh = self.ens.members[0].osh
        self.law = sm.RowLaw(self.ens.members, row_of(self.config,
                                                      self.values, 1),
                             self.ob, False)
        self.unobs = self.law.unobs
        self.kinds = [osh[f].kind for f in self.unobs]
        M = self.ens.M
        self.tables, self.sizes = {}, []
        for f, kind in zip(self.unobs, self.kinds):
            if kind == ol.NICH:
                t = [self.law.cell_cdf_bins(e, f, NICH_EDGES)
                     for e in range(M)]
            else:
                vals = np.arange({ol.DD: osh[f].dim, ol.BB: 2}.get(kind,
                                                                   GP_CELLS))
                t = [self.law.cell_pmf(e, f, vals) for e in range(M)]
            self.tables[f] = t
            self.sizes.append(t[0].shape[1])
        self.pmf = self.law.joint(self.tables)
        self.planted = {"uniform": self.law.joint(self.tables,
                                                  r=np.full(M, 1.0 / M)),
                        "percell": self.law.joint(self.tables,
                                                  independent=True)}
        for e in range(M):
            self.planted["once%d" % e] = self.law.joint(
                self.tables, r=np.eye(M)[e])
        # the real alone: Kolmogorov-Smirnov on its CDF
        self.ks = self.kinds == [ol.NICH]

    def cells_of(self, cols):
        """the draws' joint cells (cols: the completed columns as words)"""
        idx = []
        for f, kind in zip(self.unobs, self.kinds):
            w = np.asarray(cols[f])
            if kind == ol.NICH:
                idx.append(np.searchsorted(NICH_EDGES, w.view(np.float32)
                                           .astype(np.float64), side="left"))
            elif kind == ol.GP:
                idx.append(np.minimum(w.astype(np.int64), GP_CELLS))
            else:
                idx.append(w.astype(np.int64))
        return sm.flatten(idx, self.sizes)

    def p_value(self, cols, which=None):
        """of the draws against the law, or a planted law"""
        if self.ks:
            f = self.unobs[0]
            r = None
            if which == "uniform":
                r = np.full(self.ens.M, 1.0 / self.ens.M)
            elif which is not None:
                r = np.eye(self.ens.M)[int(which[4:])]
            x = np.asarray(cols[f]).view(np.float32).astype(np.float64)
            return float(stats.kstest(
                x, lambda t: self.law.cell_cdf(f, t, r)).pvalue)
        pmf = self.pmf if which is None else self.planted[which]
        return sx.chi2_p(self.cells_of(cols), np.arange(len(pmf)), pmf)

    def apart(self, which):
        """how far the planted law is from the law, before anything is drawn
        -> (figure, the least figure its rejection is asserted at)"""
        if self.ks:
            f = self.unobs[0]
            r = (np.full(self.ens.M, 1.0 / self.ens.M) if which == "uniform"
                 else np.eye(self.ens.M)[int(which[4:])])
            t = np.linspace(-12.0, 10.0, 2201)
            return float(np.abs(self.law.cell_cdf(f, t)
                                - self.law.cell_cdf(f, t, r)).max()), KS_MIN
        p, q = self.pmf, self.planted[which]
        cp, cq, a, b = [], [], 0.0, 0.0
        for pi, qi in zip(p, q):          # (chi2_p's merging, under q)
            a, b = a + pi, b + qi
            if b * N >= 50.0:
                cp.append(a)
                cq.append(b)
                a = b = 0.0
        cp[-1] += a
        cq[-1] += b
        cp, cq = np.array(cp), np.array(cq)
        return float(N * ((cp - cq) ** 2 / cq).sum()), NCP_MIN


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def draws(name):
    """N composed draws of the case's row under its mask"""
    if name not in _DRAWS:
        c = case(name)
        L = ol.oracle()
        _DRAWS[name] = sm.expect_many(
            [m.orc for m in c.ens.members], [m.gsh for m in c.ens.members],
            row_of(c.config, c.values, N), np.full(N, c.ob, np.uint32),
            L.orc_rng_seed(20240601), L.orc_rng_seed(20240602), 0, False)
    return _DRAWS[name]


def which_laws(name):
    c = case(name)
    out = []
    for w in c.asserted:
        out += (["once%d" % e for e in range(c.ens.M)] if w == "once"
                else [w])
    return out


@pytest.mark.parametrize("name", sorted(LAWS))
def test_planted_laws_are_other_laws_for_these_rows_and_masks(name):
    """before anything is drawn: the members disagree about the observed
    cells, and every planted law that is asserted is far from the law"""
    c = case(name)
    print("%s: p(e | x_obs) = %s, %d joint cells" % (
        name, np.round(c.law.r, 4), len(c.pmf)))
    assert abs(c.pmf.sum() - 1.0) < 1e-6
    for w in ["uniform", "percell"] + ["once%d" % e for e in range(c.ens.M)]:
        if c.ks and w == "percell":
            continue
        figure, least = c.apart(w)
        print("  %-8s %s %.4g (asserted from %.4g)%s" % (
            w, "CDF distance" if c.ks else "noncentrality", figure, least,
            "" if w in which_laws(name) else "  -- not asserted"))
        if w in which_laws(name):
            assert figure >= least, (name, w)


@pytest.mark.parametrize("name", sorted(LAWS))
def test_composed_draws_follow_the_law_and_reject_the_planted_laws(name):
    c = case(name)
    d = draws(name)
    assert len(set(d["member"].tolist())) == c.ens.M
    # the member alone: p(e | x_obs)
    pm = sx.chi2_p(d["member"], np.arange(c.ens.M), c.law.r)
    p = c.p_value(d["cols"])
    print("%s: %d draws; members %s against %s, p = %.3g; cells p = %.3g" % (
        name, N, np.bincount(d["member"], minlength=c.ens.M),
        np.round(c.law.r, 4), pm, p))
    assert pm > 1e-4 and p > 1e-4
    # observed cells come back as given
    for f in range(len(c.values)):
        if (c.ob >> f) & 1:
            assert np.all(d["cols"][f] == ol.value_words(
                c.ens.members[0].osh[f].kind,
                row_of(c.config, c.values, 1)[f])[0])
    for w in which_laws(name):
        pw = c.p_value(d["cols"], w)
        print("  planted %-8s p = %.3g" % (w, pw))
        assert pw < 1e-6, (name, w)


# ---------------------------------------------------------------------------
# the pieces it is composed from


def small(config, le=None, nq=60):
    specs = ee.SPECS3 if le is None else [
        dict(k=k, empty=1, alpha=1.0, d=0.0, sweeps=0) for k in (4, 17, 41)]
    return ee.Ensemble(config, specs, nq=nq, le=le)


def expect_small(ens, observed, members=None):
    L = ol.oracle()
    ms = ens.members if members is None else members
    return sm.expect_many([m.orc for m in ms], [m.gsh for m in ms], ens.qvals,
                          observed, L.orc_rng_seed(sm.DRAW_SEED),
                          L.orc_rng_seed(sm.MEMBER_SEED), sm.DRAW_BASE,
                          ens.le is not None)


@pytest.mark.parametrize("config,le,target,cand", [
    ("dd_bb_gp", None, 0, None), ("dd_bb_gp", None, 2, fe.COUNT_CANDIDATES),
    ("gp_nich", None, 1, fe.REAL_CANDIDATES), ("dd_bb_gp", 2000, 1, None)])
def test_wb_base_and_member_are_predict_feature_manys(config, le, target,
                                                      cand):
    """for masks that leave the target unobserved the fold is
    feature_many_expect's `base` chain, bit for bit, and so are the ensemble's
    base and the member drawn from it"""
    ens = small(config, le)
    F = len(ens.members[0].osh)
    observed = fe.random_masks(ens.nq, F, 11) & ~np.uint32(1 << target)
    e = expect_small(ens, observed)
    L = ol.oracle()
    if cand is not None:
        kind = ens.members[0].osh[target].kind
        cand = np.array(cand, np.float32 if kind == ol.NICH else np.uint32)
    want = fm.expect_many([m.orc for m in ens.members], ens.qvals, observed,
                          target, cand, L.orc_rng_seed(sm.DRAW_SEED),
                          L.orc_rng_seed(sm.MEMBER_SEED), sm.DRAW_BASE,
                          le is not None)

    def bits(a):
        return np.ascontiguousarray(a, np.float32).view(np.uint32)

    assert np.array_equal(bits(e["wb"]), bits(want["wb"]))
    assert np.array_equal(bits(e["base"]), bits(want["base"]))
    assert np.array_equal(e["member"], want["member_draw"])
    assert len(set(e["member"].tolist())) > 1


@pytest.mark.parametrize("config,le", [("dd_bb_gp", None), ("gp_nich", None),
                                       ("dd_bb_gp", 2000)])
def test_one_member_is_sample_rows_itself(config, le):
    ens = small(config, le)
    F = len(ens.members[0].osh)
    L = ol.oracle()
    seed = L.orc_rng_seed(sm.DRAW_SEED)
    for observed in (fe.random_masks(ens.nq, F, 12), None):
        for m in ens.members:
            one = sm.expect_many([m.orc], [m.gsh], ens.qvals, observed, seed,
                                 L.orc_rng_seed(sm.MEMBER_SEED), sm.DRAW_BASE,
                                 le is not None, nq=ens.nq)
            want = sx.expect_groups(m.orc, ens.qvals, observed, seed,
                                    sm.DRAW_BASE, nq=ens.nq)
            assert np.all(one["member"] == 0)
            assert np.array_equal(one["group"], want)
            # the cells: sample_expect.cell_word on the drawn group's words
            # (the inexact kinds may part in a last place, see sample_expect)
            for f, osh in enumerate(m.osh):
                for q in range(0, ens.nq, 7):
                    if observed is not None and (int(observed[q]) >> f) & 1:
                        continue
                    w = sx.cell_word(osh, m.orc.get_group(
                        f, int(one["packed"][q])), seed, sm.DRAW_BASE + q, f)
                    if osh.kind in (ol.DD, ol.BB):
                        assert one["cols"][f][q] == w, (f, q)


# ---------------------------------------------------------------------------
# the eight-feature ensemble of tests/eight_expect.py

_EIGHT3 = {}


def eight3_draws():
    """sample_many_expect.expect_many of eight3's 100 rows under random and
    fixed masks, computed once"""
    if not _EIGHT3:
        ens = xe.eight3()
        L = ol.oracle()
        masks = xe.masks_for(ens.nq, 8, 41)
        _EIGHT3["masks"] = masks
        _EIGHT3["e"] = sm.expect_many(
            [m.orc for m in ens.members], [m.gsh for m in ens.members],
            ens.qvals, masks, L.orc_rng_seed(sm.DRAW_SEED),
            L.orc_rng_seed(sm.MEMBER_SEED), sm.DRAW_BASE, False)
    return _EIGHT3["e"], _EIGHT3["masks"]


def base_law(states, qvals, masks):
    """the float64 log of the mean over the members of the marginal density
    of every row's observed cells, and its band: marginals_expect.law_f64
    per distinct mask on the rows that carry it"""
    pat = np.asarray(masks, np.int64) & 0xFF
    Lv, band = np.zeros(len(pat)), np.zeros(len(pat))
    for p in np.unique(pat):
        idx = np.nonzero(pat == p)[0]
        a, b = mx.law_f64(states, [np.asarray(v)[idx] for v in qvals],
                          np.array([p], np.uint32), False)
        Lv[idx], band[idx] = a[:, 0], b[:, 0]
    return Lv, band


def test_eight3_base_is_in_the_float64_band_and_the_variants_are_not():
    """every row; then a law that never observes feature 7, one that takes
    feature f's words from feature f & 3, one that reads the mask through
    & 0xF"""
    ens = xe.eight3()
    e, masks = eight3_draws()
    states = [m.st for m in ens.members]
    assert np.all(np.isfinite(e["base"]))
    assert len(set(e["member"].tolist())) == 3
    Lv, band = base_law(states, ens.qvals, masks)
    x = np.abs(e["base"] - Lv) / band
    print("eight3: %d rows, worst excursion / band of base %.3f; members "
          "drawn %s" % (ens.nq, x.max(), np.bincount(e["member"])))
    assert x.max() <= 1.0
    for variant in xe.VARIANTS:
        qq = xe.planted_state(states[0], ens.qvals,
                              "wrap" if variant == "wrap" else "mask4")[1]
        wrong, _ = base_law(states, qq, xe.planted_mask(masks, variant, 7))
        out = np.abs(wrong - Lv) > band
        print("  %s: %.0f %% of the rows leave the band" % (
            variant, 100.0 * out.mean()))
        assert out.any(), variant


def test_eight3_wb_and_member_are_predict_feature_manys():
    """for the rows whose mask leaves the target unobserved"""
    ens = xe.eight3()
    e, masks = eight3_draws()
    L = ol.oracle()

    def bits(a):
        return np.ascontiguousarray(a, np.float32).view(np.uint32)

    for target in (0, 7):
        rows = np.nonzero(((masks >> target) & 1) == 0)[0]
        assert len(rows) >= 30
        want = fm.expect_many(
            [m.orc for m in ens.members], ens.qvals, masks, target, None,
            L.orc_rng_seed(sm.DRAW_SEED), L.orc_rng_seed(sm.MEMBER_SEED),
            sm.DRAW_BASE, False)
        assert np.array_equal(bits(e["wb"][:, rows]),
                              bits(want["wb"][:, rows]))
        assert np.array_equal(bits(e["base"][rows]), bits(want["base"][rows]))
        assert np.array_equal(e["member"][rows], want["member_draw"][rows])


def test_eight3_cells_are_drawn_with_their_own_feature_as_the_key():
    """every unobserved DD, BB and DPD cell is sample_expect.cell_word on the
    drawn member's drawn group with key f, for f up to 7 (the other kinds
    may part in a last place, see sample_expect)"""
    ens = xe.eight3()
    e, masks = eight3_draws()
    seed = ol.oracle().orc_rng_seed(sm.DRAW_SEED)
    cells = 0
    for q in range(ens.nq):
        m = ens.members[int(e["member"][q])]
        for f, osh in enumerate(m.osh):
            if (int(masks[q]) >> f) & 1 or osh.kind not in (ol.DD, ol.BB,
                                                            ol.DPD):
                continue
            w = sx.cell_word(osh, m.orc.get_group(f, int(e["packed"][q])),
                             seed, sm.DRAW_BASE + q, f)
            assert e["cols"][f][q] == w, (q, f)
            cells += 1
    assert cells > 150
