"""dist_group_sample_value, the host side of csrc/sample.h: held to the
float64 law of each kind, made to reject planted bugs at the same sample size,
and compared word for word with the Python restatement (sample_expect.py).
Needs no GPU."""
import numpy as np
import pytest

import f64_scores as fx
import oracle_lib as ol
import sample_expect as sx
from distributions_amd import engine

N_DRAWS = 100000
SEED_STATE = 0x2545F491
A5 = [0.5, 1.0, 0.25, 2.0, 0.75]
BETAS = [0.3, 0.2, 0.15, 0.1, 0.1, 0.05]       # + beta0 = 0.1

# name: (oracle Shared, engine Shared, member generator)
KINDS = {
    "dd5": (ol.make_shared(ol.DD, alphas=A5), engine.dd_shared(A5),
            lambda rng, n: rng.integers(0, 5, n)),
    "dd70": (ol.make_shared(ol.DD, alphas=[0.5] * 70),
             engine.dd_shared([0.5] * 70),
             lambda rng, n: rng.integers(0, 70, n) ** 2 // 70),
    "dpd": (ol.make_shared(ol.DPD, alpha=2.0, betas=BETAS, beta0=0.1),
            engine.dpd_shared(2.0, BETAS, 0.1),
            lambda rng, n: rng.integers(0, 6, n)),
    "bb": (ol.make_shared(ol.BB, alpha=0.5, beta=2.0),
           engine.bb_shared(0.5, 2.0),
           lambda rng, n: (rng.random(n) < 0.4).astype(np.int64)),
    "gp": (ol.make_shared(ol.GP, alpha=2.5, inv_beta=0.7),
           engine.gp_shared(2.5, 0.7), lambda rng, n: rng.poisson(6.0, n)),
    "bnb": (ol.make_shared(ol.BNB, alpha=2.5, beta=1.5, r=3),
            engine.bnb_shared(2.5, 1.5, 3),
            lambda rng, n: rng.poisson(4.0, n)),
    "nich": (ol.make_shared(ol.NICH, mu=0.0, kappa=1.0, sigmasq=1.0, nu=1.0),
             engine.nich_shared(0.0, 1.0, 1.0, 1.0),
             lambda rng, n: rng.normal(1.0, 2.0, n).astype(np.float32)),
}
SIZES = [0, 3, 400]
_DRAWS = {}


def members(name, size):
    rng = np.random.default_rng(1000 + size)
    return KINDS[name][2](rng, size)


def group_words(name, size):
    osh, gsh, _ = KINDS[name]
    g = gsh.group_init()
    for w in ol.value_words(osh.kind, members(name, size)):
        gsh.group_add_value(g, int(w))
    return g


def draws(name, size, feature=0, n=N_DRAWS):
    """the draws of one group, made once and shared"""
    key = (name, size, feature, n)
    if key not in _DRAWS:
        gsh = KINDS[name][1]
        _DRAWS[key] = gsh.group_sample_value(group_words(name, size),
                                             SEED_STATE, 7 * size, n, feature)
    return _DRAWS[key]


def law(name, size, **kw):
    osh = KINDS[name][0]
    return sx.law_pmf(osh.kind, fx.Feature(osh).kw(), members(name, size),
                      **kw)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ["dd5", "dd70", "dpd", "bb", "gp", "bnb"])
def test_law_discrete(name, size):
    values, pmf = law(name, size)
    p = sx.chi2_p(draws(name, size), values, pmf)
    print("%s, %d members: chi-square p = %.3g" % (name, size, p))
    assert p > 1e-4


@pytest.mark.parametrize("size", SIZES)
def test_law_nich(size):
    osh = KINDS["nich"][0]
    t = sx.nich_t(fx.Feature(osh).kw(), members("nich", size))
    x = draws("nich", size).view(np.float32).astype(np.float64)
    p = sx.stats.kstest(x, t.cdf).pvalue
    print("nich, %d members: KS p = %.3g" % (size, p))
    assert p > 1e-4


# ---- planted bugs: the same histograms reject each wrong law ---------------


def test_rejects_dd_without_alphas():
    # (held on the 3-member group, where the alphas are most of the weight;
    # against 400 counts DD(5)'s alphas, 4.5 in all, move the law by a
    # percent, which 10^5 draws cannot see)
    for name in ("dd5", "dd70"):
        dim = KINDS[name][0].dim
        pmf = np.bincount(members(name, 3), minlength=dim) / 3.0
        p = sx.chi2_p(draws(name, 3), np.arange(dim), pmf)
        print("%s weights without the alphas: p = %.3g" % (name, p))
        assert p < 1e-6


def test_rejects_gp_scale_without_n():
    osh = KINDS["gp"][0]
    kw = fx.Feature(osh).kw()
    for size in (3, 400):
        m = members("gp", size)
        # gamma(alpha + sum) / inv_beta: the negative binomial of a group
        # whose rate forgot its n
        a = kw["alpha"] + m.sum()
        ib = kw["inv_beta"]
        nb = sx.stats.nbinom(a, ib / (ib + 1.0))
        hi = int(nb.ppf(1 - 1e-13)) + 1
        xs = np.arange(hi)
        p = sx.chi2_p(draws("gp", size), xs, nb.pmf(xs))
        print("gp scale without n, %d members: p = %.3g" % (size, p))
        assert p < 1e-6


def test_rejects_nich_scale_without_kappa_term():
    osh = KINDS["nich"][0]
    for size in SIZES:
        t = sx.nich_t(fx.Feature(osh).kw(), members("nich", size),
                      scale_bug=True)
        x = draws("nich", size).view(np.float32).astype(np.float64)
        p = sx.stats.kstest(x, t.cdf).pvalue
        print("nich scale without (kn + 1) / kn, %d members: p = %.3g"
              % (size, p))
        if size < 400:
            assert p < 1e-6
    # at 400 members (kn + 1) / kn is 1.0025: the scale moves by 0.12 %, which
    # 10^5 draws cannot see; the two smaller groups carry this check


def test_rejects_bnb_without_binomial():
    for size in SIZES:
        values, pmf = law("bnb", size, bnb_binomial=False)
        p = sx.chi2_p(draws("bnb", size), values, pmf)
        print("bnb held to the bare score, %d members: p = %.3g" % (size, p))
        assert p < 1e-6


def test_pair_of_features_independent():
    """two features of one row draw from streams of their own; keyed without
    the feature index they would be the same draw"""
    for name in ("dd5", "bb"):
        a = draws(name, 3, feature=0)
        b = draws(name, 3, feature=1)
        p = sx.pair_p(a, b)
        print("%s, features 0 and 1 of the same rows: p = %.3g" % (name, p))
        assert p > 1e-4
        # the planted bug: both cells keyed as feature 0
        assert sx.pair_p(a, draws(name, 3, feature=0)) < 1e-6


# ---- the restatement --------------------------------------------------------

N_CELLS = 20000


@pytest.mark.parametrize("name", ["dd5", "dd70", "dpd", "bb", "gp", "bnb",
                                  "nich"])
def test_restatement(name):
    osh, gsh, _ = KINDS[name]
    exact = name not in ("gp", "bnb")
    excused = 0
    per = -(-N_CELLS // (2 * len(SIZES)))
    for size in SIZES:
        g = group_words(name, size)
        for feature in (0, 5):
            row0 = (1 << 33) + 1000 * size      # rows beyond 32 bits too
            got = gsh.group_sample_value(g, SEED_STATE, row0, per, feature)
            for i in range(per):
                streams = []
                want = sx.cell_word(osh, g, SEED_STATE, row0 + i, feature,
                                    streams)
                assert not streams[0].exhausted
                if int(got[i]) == want:
                    continue
                # only a PTRS acceptance that CPython's lgamma and the C
                # library's decide differently in the last place is excused,
                # and it is shown to be one
                margin = streams[0].ptrs_margin
                assert not exact and margin is not None and margin < 1e-14, (
                    name, size, feature, i, int(got[i]), want, margin)
                excused += 1
    print("%s: %d cells, %d excused" % (name, 2 * per * len(SIZES), excused))
    assert excused * 100000 <= 2 * per * len(SIZES)
