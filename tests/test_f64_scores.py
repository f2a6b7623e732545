"""The oracle's row scores held to float64 predictives (tests/f64_scores.py).

orc_mix_batch_row_scores (the batch-semantics composition every kernel is
pinned to bit for bit) and the oracle's sequential Mixture::score_value must
lie within the derived band of the float64 scores rebuilt from the groups'
members, for every slot of every checked row.  Planted bugs in the float64
scorer must fall outside it: the band is tight enough to see them."""
import ctypes

import numpy as np
import pytest

import f64_scores as fx
import oracle_lib as ol
import workloads

CONFIGS = ["dd", "dd_zipf", "dd_skew", "bb", "gp", "bnb", "nich", "gp_nich",
           "nich2", "dpd", "dpd_other", "dd_bb_gp"]
SEED = 5


def _le(orc, dataset_size):
    orc.L.orc_mix_set_low_entropy.restype = None
    orc.L.orc_mix_set_low_entropy.argtypes = [ctypes.c_void_p, ctypes.c_int]
    orc.L.orc_mix_set_low_entropy(orc.h, dataset_size)


def build(osh, vals, assign, k, empty, alpha=1.0, d=0.0, sweeps=0, le=None,
          batch=16):
    """an oracle state and its float64 restatement; `sweeps` passes of
    batches of `batch` rows at (alpha, d) make singletons and new groups"""
    orc = ol.OracleMixture(alpha, d, osh)
    if le is not None:
        _le(orc, le)
    orc.init_from_assignments(vals, assign, k, empty)
    n = len(assign)
    history = [orc.assign.copy()]
    st = ol.oracle().orc_rng_seed(SEED)
    for s in range(sweeps):
        for b in range(0, n, batch):
            orc.gibbs_batch(b, min(n, b + batch), st, s * n)
        history.append(orc.assign.copy())
    p2g = [orc.packed_to_global(i) for i in range(len(orc))]
    prior = ("py", float(np.float32(alpha)), float(np.float32(d))) \
        if le is None else ("le", le)
    return orc, fx.State(vals, osh, orc.assign, p2g, prior, history)


def workload_state(config, empty, d, sweeps, n=2000, k=16, dim=None):
    osh, _, vals, assign = workloads.make(config, n, k, dim=dim)
    alpha = 20.0 if sweeps else 1.0
    return build(osh, vals, assign, k, empty, alpha, d, sweeps)


def big_group_state():
    """LowEntropy with one group above very_large = 10000 rows (10241: its
    logs' arguments are whole numbers in [8192, 16384), bucket ends of the
    log table) and a few small ones, no features"""
    n = 10400
    assign = np.r_[np.zeros(10241), 1 + np.arange(n - 10241) % 40]
    orc, st = build([], [], assign.astype(np.uint32), 41, 1, le=n + 1000)
    return orc, st


def planted_state():
    _, osh, _, vals = workloads.planted(2000, k_true=16, n_cat=4, n_real=2)
    assign = (np.arange(2000) % 16).astype(np.uint32)
    return build(osh, vals, assign, 16, 1, 20.0, 0.5, sweeps=1)


def le_state(config, n, extra):
    osh, _, vals, assign = workloads.make(config, n, 16)
    return build(osh, vals, assign, 16, 1, le=n + extra)


def _cases():
    out = {}
    for config in CONFIGS:
        for d in (0.0, 0.5):
            for empty in (1, 3):
                for sweeps in (0, 2):
                    out["%s_d%g_e%d_s%d" % (config, d, empty, sweeps)] = (
                        lambda c=config, e=empty, dd=d, s=sweeps:
                        workload_state(c, e, dd, s))
    out["planted"] = planted_state
    out["dd256_k1024"] = lambda: workload_state("dd", 1, 0.5, 0, n=4096,
                                                k=1024, dim=256)
    out["le_dd_N"] = lambda: le_state("dd", 2000, 0)
    out["le_gp_nich_N1000"] = lambda: le_state("gp_nich", 2000, 1000)
    out["le_bb_small"] = lambda: le_state("bb", 200, 1000)
    out["le_big_group"] = big_group_state
    return out


CASES = _cases()
_STATES = {}


def state(name):
    if name not in _STATES:
        _STATES[name] = CASES[name]()
    return _STATES[name]


def oracle_row_scores(orc, st, rows):
    out = np.full((len(rows), st.K), np.nan)
    for i, r in enumerate(rows):
        s = orc.row_scores(int(r), int(st.slot[r]))
        out[i, :len(s)] = s
    return out


def oracle_sequential_scores(orc, st, rows):
    """MixtureDriver::score_value, then every slave's score_value"""
    out = np.zeros((len(rows), st.K), np.float32)
    words = orc.values
    for i, r in enumerate(rows):
        s = out[i]
        orc.L.orc_mix_driver_score_value(orc.h, s)
        for f in range(orc.F):
            orc.L.orc_mix_slave_score_value(orc.h, f, int(words[f][r]), s)
    return out.astype(np.float64)


def worst(got, want, band):
    x = fx.excursion(got, want, band)
    return float(x.max()) if x.size else 0.0


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_scores_are_in_the_float64_band(name):
    orc, st = state(name)
    rows = fx.checked_rows(st)
    v, b, kl = fx.row_scores_f64(st, rows)
    got = oracle_row_scores(orc, st, rows)
    assert np.array_equal(np.isnan(got), np.isnan(v)), "slot counts differ"
    w_batch = worst(got, v, b)
    v2, b2, _ = fx.score_rows_f64(st, rows)
    w_seq = worst(oracle_sequential_scores(orc, st, rows), v2, b2)
    print("%s: K=%d, %d rows, %d alone; worst excursion / band: "
          "row_scores %.3f, score_value %.3f" % (
              name, st.K, len(rows), int((kl != st.K).sum()), w_batch, w_seq))
    assert w_batch <= 1.0, name
    assert w_seq <= 1.0, name


# ---------------------------------------------------------------------------
# the float64 formulas are the textbook predictives


@pytest.mark.parametrize("config", CONFIGS)
def test_float64_scorer_is_the_predictive(config):
    """State's per-slot formulas (written in the kernels' order) agree with
    float64_score (scipy) to float64 accuracy, feature by feature"""
    orc, st = state("%s_d0.5_e3_s2" % config)
    rng = np.random.default_rng(1)
    rows = rng.choice(st.N, 6, replace=False)
    for fi, (f, col) in enumerate(zip(st.feats, st.cols)):
        one = fx.State([col], [orc.shareds[fi]], st.assign, st.p2g,
                       ("le", 10 ** 6))
        # the prior alone: the same state without the feature
        bare = fx.State([], [], st.assign, st.p2g, ("le", 10 ** 6))
        v, _, _ = fx.score_rows_f64(one, rows)
        p, _, _ = fx.score_rows_f64(bare, rows)
        for i, r in enumerate(rows):
            for k in range(st.K):
                members = col[st.slot == k]
                x = col[r]
                if f.kind in (fx.DD, fx.DPD, fx.BB, fx.GP, fx.BNB):
                    members, x = members.astype(np.int64), int(x)
                else:
                    members, x = members.astype(np.float64), float(x)
                want = fx.float64_score(f.kind, f.kw(), members, x)
                assert abs((v[i, k] - p[i, k]) - want) <= 1e-9 * (
                    1 + abs(want)), (config, fi, r, k)


def test_bnb_reference_score_drops_only_the_binomial_coefficient():
    """bnb.hpp:200-223: adding log C(x + r - 1, x) makes the score a
    normalised pmf over x; without it, it is not"""
    kw = dict(alpha=1.5, beta=0.75, r=3)
    members = [0, 4, 2, 7]
    x = np.arange(0, 20000)
    s = np.array([fx.float64_score(fx.BNB, kw, members, int(v)) for v in x])
    total = np.exp(s + fx.bnb_log_binomial(3.0, x)).sum()
    assert abs(total - 1.0) < 1e-3
    assert abs(np.exp(s).sum() - 1.0) > 0.1
    # and it is the oracle's group score (to float32 accuracy)
    L = ol.oracle()
    sh = ol.make_shared(ol.BNB, **kw)
    m = ol.OracleMixture(1.0, 0.0, [sh])
    L.orc_mix_slave_append_empty(m.h, 0)
    for v in members:
        L.orc_mix_slave_group_add_value(m.h, 0, 0, v)
    L.orc_mix_slave_init(m.h, 0)
    for v in (0, 1, 5, 30):
        got = L.orc_mix_slave_score_value_group(m.h, 0, 0, v)
        want = fx.float64_score(fx.BNB, kw, members, v)
        assert abs(got - want) < 1e-3 * (1 + abs(want))


def test_dpd_other_scores_alpha_beta0():
    """dpd.hpp:534-542: OTHER, never a row's value here, scores
    log(alpha * beta0 / (alpha + n)) in every group"""
    orc, st = state("dpd_other_d0.5_e1_s2")
    f = st.feats[0]
    for k in range(st.K):
        got = orc.L.orc_mix_slave_score_value_group(orc.h, 0, k, fx.OTHER)
        members = st.cols[0][st.slot == k].astype(np.int64)
        want = fx.float64_score(fx.DPD, f.kw(), members, fx.OTHER)
        S, H = fx.cat_terms(f, np.array([len(members)]), np.array([0]),
                            np.array([fx.OTHER], np.int64))
        assert abs(got - want) <= S.e[0] + H.e[0] + 2 * fx.EPS * abs(want)


# ---------------------------------------------------------------------------
# planted bugs

MUTANTS = ["own_prior", "own_feat", "own_both", "log_n", "vanish_nonempty",
           "alpha_undivided", "shift_N", "singleton_old", "le_corr_at_sample",
           "le_very_large", "dd_alpha_sum_row", "dpd_beta_unscaled",
           "bb_swapped", "gp_no_logfact", "bnb_r_count", "nich_kappa"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_planted_bug_leaves_the_band(mutant):
    """each mutated float64 scorer puts at least one checked (row, slot) of
    the cases above outside the band (the case that shows it is printed).
    The band stays the one of the operations the oracle performs."""
    for name in CASES:
        orc, st = state(name)
        rows = fx.checked_rows(st)
        got = oracle_row_scores(orc, st, rows)
        _, b, _ = fx.row_scores_f64(st, rows)
        v, _, _ = fx.row_scores_f64(st, rows, mut=(mutant,))
        w = worst(got, v, b)
        if w > 1.0:
            print("%s caught by %s: %.1f x the band" % (mutant, name, w))
            return
    pytest.fail("planted bug %s stays inside the band" % mutant)
