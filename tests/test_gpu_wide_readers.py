"""The held-out readers on five to eight features (tests/eight_expect.py):
k_predict, k_predict_feature and its recompute partner, k_sample_rows, bit for
bit against the expectations predict_expect, feature_expect and sample_expect
compose from the oracle (which tests/test_predict_oracle.py and
tests/test_predict_feature_oracle.py hold to float64 on the same subjects).

Every list of three or more features runs the scorers' run-time instance: the
loop over the features is not unrolled, the query words, log factorials and
the observed mask are indexed by a run-time f, and the staged
predict_feature numbers its LDS planes by walking the features after the
target.  What changes past four features is aimed at here: feature indices
4 .. 7 in the words, the mask, the bad-value report and the cell key; three
categorical features after a target; a target whose staging takes two and
three tiles of groups (asserted from the restated launch geometry).

The ensemble forms on the eight-feature ensemble are cases of
test_gpu_predict_many.py, test_gpu_predict_feature_many.py,
test_gpu_sample_rows_many.py, test_gpu_coassign.py, test_gpu_coassign_topk.py
and test_gpu_search_resident.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import eight_expect as xe  # noqa: E402
import feature_expect as fe  # noqa: E402
import oracle_lib as ol  # noqa: E402
import predict_expect as pe  # noqa: E402
import sample_expect as sx  # noqa: E402
from test_gpu_predict import (  # noqa: E402
    GROUP_SENTINEL, SENTINEL, bits, predict_dev, same, snapshot, word)
from test_gpu_predict_feature import check as check_feature  # noqa: E402
from test_gpu_sample_rows import (  # noqa: E402
    check_cells, rows_dev, words_of)

pytestmark = pytest.mark.gpu

NQ = 48            # held-out rows per (case, target)
FORMS = (True, False)     # staged, recompute
EIGHTS = ["eight", "eight_swept"]

_ENGINES = {}


def engine_of(name):
    """one engine per subject, shared: the readers leave it as it was"""
    if name not in _ENGINES:
        _ENGINES[name] = xe.case(name).engine()
    return _ENGINES[name]


def seed_state():
    return ol.oracle().orc_rng_seed(pe.DRAW_SEED)


# ---------------------------------------------------------------------------
# predict


@pytest.mark.parametrize("name", xe.NAMES)
def test_predict_is_the_oracles_bit_for_bit(name):
    c = xe.case(name)
    e = c.expect()
    gpu = engine_of(name)
    before = snapshot(gpu)
    logp, draw, total = gpu.predict(c.qvals, "sample", seed=pe.DRAW_SEED,
                                    draw_base=pe.DRAW_BASE)
    logp_m, first, total_m = gpu.predict(c.qvals, "map")
    logp_n, none, _ = gpu.predict(c.qvals, None)
    x = pe.excursion(logp, c)
    print("%s: F=%d, K=%d, %d held-out rows: logp bits differ in %d rows, "
          "draws in %d, maxima in %d; worst excursion / band %.3f" % (
              name, len(c.osh), c.K, c.nq,
              int((bits(logp) != bits(e["logp"])).sum()),
              int((draw != e["draw"]).sum()), int((first != e["map"]).sum()),
              x.max()))
    assert np.array_equal(bits(logp), bits(e["logp"]))
    assert np.array_equal(bits(logp_m), bits(e["logp"]))
    assert np.array_equal(bits(logp_n), bits(e["logp"]))
    assert none is None
    assert np.array_equal(draw, e["draw"])
    assert np.array_equal(first, e["map"])
    assert word(total) == word(e["prior_total"]) == word(total_m)
    if c.le is None:
        assert abs(float(total)) <= 1e-4
    assert x.max() <= 1.0
    assert same(before, snapshot(gpu))


@pytest.mark.parametrize("name", xe.NAMES)
def test_predict_chunks_of_64_around_the_wave(name):
    """debug.predict_chunk = 64 with 1, 63, 64, 65 and 129 rows (the held-out
    rows cycled): row q draws with engine step draw_base + q + 1 whatever the
    chunk, nothing is written past n"""
    c = xe.case(name)
    gpu = engine_of(name)
    rows = xe.repeat_rows(c.qvals, 129)
    e = pe.expect(c.orc, rows, seed_state(), pe.DRAW_BASE)
    assert np.array_equal(bits(e["logp"][:c.nq]), bits(c.expect()["logp"]))
    words = pe.query_words(c.orc, rows)
    gpu.set_option("debug.predict_chunk", 64)
    try:
        for n in (1, 63, 64, 65, 129):
            for mode, key in ((0, "draw"), (1, "map")):
                logp, group = predict_dev(gpu, words, n, mode)
                assert np.array_equal(bits(logp[:n]), bits(e["logp"][:n])), n
                assert np.array_equal(group[:n].view(np.uint32),
                                      e[key][:n]), (n, key)
                assert np.all(logp[n:] == SENTINEL), n
                assert np.all(group[n:] == GROUP_SENTINEL), n
    finally:
        gpu.set_option("debug.predict_chunk", 1 << 22)


def test_predict_many_of_one_engine_is_predict():
    from distributions_amd import engine
    c = xe.case("eight_swept")
    e = c.expect()
    gpu = engine_of("eight_swept")
    for flags in (0, engine.PREDICT_MANY_DRAW_ALL):
        logp, member, group, _, _ = engine.predict_many(
            [gpu], c.qvals, "sample", seed=pe.DRAW_SEED,
            draw_base=pe.DRAW_BASE, flags=flags)
        assert np.array_equal(bits(logp), bits(e["logp"]))
        assert np.all(member == 0)
        assert np.array_equal(group, e["draw"])
        _, _, first, _, _ = engine.predict_many([gpu], c.qvals, "map",
                                                flags=flags)
        assert np.array_equal(first, e["map"])


def test_predict_then_sweep_is_the_oracles_sweep():
    c = xe.case("eight")
    gpu = c.engine()          # (its own engine: the state moves)
    gpu.predict(c.qvals, "sample", seed=1)
    orc = ol.OracleMixture(c.alpha, c.d, c.osh)
    orc.init_from_assignments(c.vals, c.assign0, c.k, c.empty)
    st = ol.oracle().orc_rng_seed(11)
    for b in range(0, c.n, 500):
        orc.gibbs_batch(b, b + 500, st, 0)
    gpu.sweep(0, c.n, 500, 11)
    gpu.predict(c.qvals, "map")         # (closes a run the sweep left open)
    assert np.array_equal(gpu.assignments(), orc.assign)
    assert np.array_equal(gpu.counts(), orc.counts())
    gpu.validate()
    e = pe.expect(orc, c.qvals, ol.oracle().orc_rng_seed(1), 0)
    logp, draw, _ = gpu.predict(c.qvals, "sample", seed=1)
    assert np.array_equal(bits(logp), bits(e["logp"]))
    assert np.array_equal(draw, e["draw"])


@pytest.mark.parametrize("feature,value", [(4, 70), (7, 3)])
def test_a_bad_value_names_its_row_and_a_feature_past_the_fourth(feature,
                                                                 value):
    c = xe.case("eight")
    e = c.expect()
    gpu = engine_of("eight")
    gpu.set_option("debug.predict_chunk", 64)
    try:
        bad = [q.copy() for q in c.qvals]
        bad[feature][70] = value
        bad[feature][45] = value        # the first offending row is named
        bad[2][45] = 2 ** 31            # (GammaPoisson takes any count)
        bad[0][90] = 200                # (a later row, an earlier feature)
        with pytest.raises(RuntimeError,
                           match="row 45, feature %d" % feature):
            gpu.predict(bad, "sample")
        only = [q.copy() for q in c.qvals]
        only[feature][70] = value       # (in the second chunk)
        with pytest.raises(RuntimeError,
                           match="row 70, feature %d" % feature):
            gpu.predict(only, "map")
        # process and engine go on
        logp, first, _ = gpu.predict(c.qvals, "map")
        assert np.array_equal(bits(logp), bits(e["logp"]))
        assert np.array_equal(first, e["map"])
    finally:
        gpu.set_option("debug.predict_chunk", 1 << 22)


# ---------------------------------------------------------------------------
# predict_feature


def tiles(c, target, n_rows=NQ):
    sh = c.osh[target]
    cand = fe.candidates_for(sh)
    C = len(fe.default_candidates(sh) if cand is None else cand)
    return xe.staged_geometry([s.kind for s in c.osh], target, C, c.K,
                              n_rows)


# tiles of groups the staged form must take, by the restated host geometry
# (tests/test_predict_feature_oracle.py asserts the figures behind them)
LEAST_TILES = {("eight", 0): 2, ("eight_swept", 0): 3, ("eight_swept", 3): 2}


@pytest.mark.parametrize("target", xe.TARGETS8)
@pytest.mark.parametrize("name", EIGHTS)
def test_eight_features_targets_under_per_row_masks(name, target):
    """both forms, joint, base, the draw and the first maximum; random masks
    with junk above bit 8, and on three rows each: only features >= 4, only
    features < 4, alternating"""
    c = xe.case(name)
    gpu = engine_of(name)
    before = snapshot(gpu)
    q = [v[:NQ] for v in c.qvals]
    cand = fe.candidates_for(c.osh[target])
    masks = xe.masks_for(NQ, 8, 100 + target)
    assert [int(m) & 0xFF for m in masks[3:12:3]] == [0xF0, 0x0F, 0xAA]
    assert tiles(c, target)["tiles"] >= LEAST_TILES.get((name, target), 1)
    e = fe.expect(c.orc, q, masks, target, cand, seed_state(), pe.DRAW_BASE)
    assert np.all(np.isfinite(e["joint"]))
    check_feature(gpu, q, target, cand, masks, e,
                  "%s target %d (%d tiles)" % (name, target,
                                               tiles(c, target)["tiles"]))
    assert same(before, snapshot(gpu))


def test_real_first_every_target_under_per_row_masks():
    name = "real_first"
    c = xe.case(name)
    gpu = engine_of(name)
    q = [v[:NQ] for v in c.qvals]
    F = len(c.osh)
    for target in range(F):
        cand = fe.candidates_for(c.osh[target])
        masks = xe.masks_for(NQ, F, 100 + target)
        e = fe.expect(c.orc, q, masks, target, cand, seed_state(),
                      pe.DRAW_BASE)
        check_feature(gpu, q, target, cand, masks, e,
                      "%s target %d" % (name, target))


@pytest.mark.parametrize("target", [0, 3, 6])
def test_observed_joint_is_predicts_logp_and_mask_zero_its_prior_total(
        target):
    c = xe.case("eight")
    gpu = engine_of("eight")
    q = [v[:NQ] for v in c.qvals]
    sh = c.osh[target]
    cand = fe.candidates_for(sh)
    values = fe.default_candidates(sh) if cand is None else cand
    for staged in FORMS:
        joint, base, _ = gpu.predict_feature(q, target, cand, None, None,
                                             staged=staged)
        for i, v in enumerate(values):
            logp, _, total = gpu.predict(
                fe.completed(q, target, v, sh.kind), None)
            assert np.array_equal(bits(joint[:, i]), bits(logp)), (staged, i)
        _, base0, _ = gpu.predict_feature(q, target, cand,
                                          np.zeros(NQ, np.uint32), None,
                                          staged=staged)
        assert np.all(bits(base0) == word(total)), staged


@pytest.mark.parametrize("staged", FORMS)
def test_predict_feature_names_a_bad_value_past_the_fourth_feature(staged):
    c = xe.case("eight")
    gpu = engine_of("eight")
    bad = [v.copy() for v in c.qvals]
    bad[7][60] = 3
    bad[4][31] = 70                  # the first offending row is named
    bad[1][90] = 2                   # (a later row, an earlier feature)
    with pytest.raises(RuntimeError, match="row 31, feature 4"):
        gpu.predict_feature(bad, 0, staged=staged)
    # the same words in cells that are not observed are never read
    masks = np.full(c.nq, 0xFF, np.uint32)
    masks[31] = 0xEF
    masks[60] = 0x7F
    masks[90] = 0xFD
    ok = gpu.predict_feature(bad, 0, None, masks, staged=staged)
    clean = gpu.predict_feature(c.qvals, 0, None, masks, staged=staged)
    for a, b in zip(ok, clean):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------
# sample_rows


@pytest.mark.parametrize("name", EIGHTS)
def test_groups_and_cells_under_per_row_masks(name):
    c = xe.case(name)
    gpu = engine_of(name)
    before = snapshot(gpu)
    F = len(c.osh)
    q = [v[:NQ] for v in c.qvals]
    given = words_of(c, q)
    masks = xe.masks_for(NQ, F, 41)
    want = sx.expect_groups(c.orc, q, masks, seed_state(), pe.DRAW_BASE)
    cols, groups = gpu.sample_rows(values=q, observed=masks,
                                   seed=pe.DRAW_SEED, draw_base=pe.DRAW_BASE)
    print("%s: K=%d, groups differ in %d of %d rows" % (
        name, c.K, int((groups != want).sum()), NQ))
    assert np.array_equal(groups, want)
    cells, wrong = check_cells(c, gpu, cols, groups, masks, given,
                               pe.DRAW_BASE, name)
    # the cells of the exact kinds against sample_expect.cell_word itself:
    # feature f's cell is drawn from feature f's statistics with key f
    got = words_of(c, cols)
    g2p = {c.orc.packed_to_global(k): k for k in range(c.K)}
    exact = 0
    for f, osh in enumerate(c.osh):
        if osh.kind not in (ol.DD, ol.BB, ol.DPD):
            continue
        for r in range(NQ):
            if (int(masks[r]) >> f) & 1:
                continue
            w = sx.cell_word(osh, c.orc.get_group(f, g2p[int(groups[r])]),
                             seed_state(), pe.DRAW_BASE + r, f)
            assert got[f][r] == w, (name, r, f)
            exact += 1
    assert exact > 50
    # every feature observed: predict's draw; the cells are the query's
    full = np.full(NQ, (1 << F) - 1, np.uint32)
    cols_f, groups_f = gpu.sample_rows(values=q, observed=full,
                                       seed=pe.DRAW_SEED,
                                       draw_base=pe.DRAW_BASE)
    assert np.array_equal(groups_f, c.expect()["draw"][:NQ])
    for f in range(F):
        assert np.array_equal(words_of(c, cols_f)[f], given[f])
    # no mask (the nothing-observed instance) and a mask of zeros agree
    want0 = sx.expect_groups(c.orc, None, None, seed_state(), pe.DRAW_BASE,
                             nq=NQ)
    cols_u, groups_u = gpu.sample_rows(n=NQ, seed=pe.DRAW_SEED,
                                       draw_base=pe.DRAW_BASE)
    cols_g, groups_g = gpu.sample_rows(observed=np.zeros(NQ, np.uint32),
                                       seed=pe.DRAW_SEED,
                                       draw_base=pe.DRAW_BASE)
    assert np.array_equal(groups_u, want0)
    assert np.array_equal(groups_g, want0)
    for a, b in zip(words_of(c, cols_u), words_of(c, cols_g)):
        assert np.array_equal(a, b)
    c2, w2 = check_cells(c, gpu, cols_u, groups_u, None, None, pe.DRAW_BASE,
                         name + " unconditional")
    cells, wrong = cells + c2, wrong + w2
    print("%s: %d cells of GP / BNB / NICH compared, %d differ" % (
        name, cells, wrong))
    assert wrong * 100000 <= cells
    assert same(before, snapshot(gpu))
    assert gpu.validate()["code"] == 0


def test_completion_in_place_and_what_is_refused():
    name = "eight_swept"
    c = xe.case(name)
    gpu = engine_of(name)
    F = len(c.osh)
    n = 100
    given = words_of(c, c.qvals)
    masks = xe.masks_for(n, F, 78)
    masks &= ~np.uint32(1 << 5)          # no row observes feature 5
    base = 5
    ref_c, ref_g = rows_dev(gpu, c, n, given, masks, base, pad=0)
    want = sx.expect_groups(c.orc, c.qvals, masks, seed_state(), base)
    assert np.array_equal(ref_g, want)
    # unobserved cells filled with 0xFFFFFFFF are never read; completion in
    # place (the torch form's out[f] = values[f]) writes only those
    filled = []
    for f in range(F):
        w = given[f].copy()
        w[((masks >> f) & 1) == 0] = 0xFFFFFFFF
        filled.append(w)
    cols, grp = rows_dev(gpu, c, n, filled, masks, base, in_place=True,
                         pad=0)
    assert np.array_equal(grp, ref_g)
    for f in range(F):
        assert np.array_equal(cols[f], ref_c[f])
    # the same through the torch form, out[f] = values[f]
    import torch
    vals = [torch.from_numpy(w.view(np.int32).copy()).cuda() for w in filled]
    mk = torch.from_numpy(masks.view(np.int32).copy()).cuda()
    out, grp_t = gpu.sample_rows_torch(values=vals, observed=mk,
                                       seed=pe.DRAW_SEED, draw_base=base,
                                       out=vals)
    assert all(o is v for o, v in zip(out, vals))
    assert np.array_equal(grp_t.cpu().numpy().view(np.uint32), ref_g)
    for f in range(F):
        assert np.array_equal(vals[f].cpu().numpy().view(np.uint32),
                              ref_c[f])
    # an observed bit on a feature passed without a column, at feature 5
    holes = list(given)
    holes[5] = None
    cols, grp = rows_dev(gpu, c, n, holes, masks, base, pad=0)
    assert np.array_equal(grp, ref_g)
    masks_bad = masks.copy()
    masks_bad[17] |= 1 << 5
    with pytest.raises(RuntimeError, match="row 17, feature 5"):
        rows_dev(gpu, c, n, holes, masks_bad, base, pad=0)
    # an observed value outside its domain at feature 7
    gpu.set_option("debug.predict_chunk", 64)
    try:
        full = np.full(n, (1 << F) - 1, np.uint32)
        bad = [v.copy() for v in c.qvals]
        bad[7][80] = 3
        bad[7][66] = 3                   # the first offending row is named
        bad[0][90] = 200                 # (a later row, an earlier feature)
        with pytest.raises(RuntimeError, match="row 66, feature 7"):
            gpu.sample_rows(values=bad, observed=full, seed=1)
        # the same words in cells that are not observed are never read
        unread = full.copy()
        unread[[66, 80]] &= ~np.uint32(1 << 7)
        unread[90] &= ~np.uint32(1)
        a = gpu.sample_rows(values=bad, observed=unread, seed=1)
        b = gpu.sample_rows(values=c.qvals, observed=unread, seed=1)
        assert np.array_equal(a[1], b[1])
        for x, y in zip(words_of(c, a[0]), words_of(c, b[0])):
            assert np.array_equal(x, y)
    finally:
        gpu.set_option("debug.predict_chunk", 1 << 22)
