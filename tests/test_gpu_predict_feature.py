"""dist_gibbs_predict_feature (k_predict_feature, its recompute partner and
k_predict_feature_choice): one feature's predictive given the others, bit for
bit against the expectation tests/feature_expect.py composes from the oracle
(and tests/test_predict_feature_oracle.py holds to float64).

Both forms (staged, recompute), joint, base, the draw and the first maximum:
every feature of eight feature lists as the target under random per-row masks,
DD-256 at K = 1025 and DPD with 10 000 values at K = 8193, identities against
Gibbs.predict that need no oracle, launch geometry, and the reader rules."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import feature_expect as fe  # noqa: E402
import oracle_lib as ol  # noqa: E402
import predict_expect as pe  # noqa: E402
from test_gpu_predict import bits, same, snapshot, word  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
CHOICE_SENTINEL = -7
NQ = 48            # held-out rows per (case, target)
FORMS = (True, False)     # staged, recompute

_ENGINES = {}


def engine_of(name):
    """one engine per case, shared: predict_feature leaves it as it was"""
    if name not in _ENGINES:
        _ENGINES[name] = fe.case(name).engine()
    return _ENGINES[name]


def seed_state():
    return ol.oracle().orc_rng_seed(pe.DRAW_SEED)


def check(gpu, q, target, cand, masks, e, what):
    """both forms, both modes, against the expectation e"""
    for staged in FORMS:
        joint, base, draw = gpu.predict_feature(
            q, target, cand, masks, "sample", seed=pe.DRAW_SEED,
            draw_base=pe.DRAW_BASE, staged=staged)
        joint_m, base_m, first = gpu.predict_feature(
            q, target, cand, masks, "map", staged=staged)
        tag = (what, "staged" if staged else "recompute")
        print("%s %s: joint bits differ in %d of %d cells, base in %d rows, "
              "draws in %d, maxima in %d" % (
                  tag + (int((bits(joint) != bits(e["joint"])).sum()),
                         joint.size,
                         int((bits(base) != bits(e["base"])).sum()),
                         int((draw != e["draw"]).sum()),
                         int((first != e["map"]).sum()))))
        assert np.array_equal(bits(joint), bits(e["joint"])), tag
        assert np.array_equal(bits(base), bits(e["base"])), tag
        assert np.array_equal(bits(joint_m), bits(e["joint"])), tag
        assert np.array_equal(bits(base_m), bits(e["base"])), tag
        assert np.array_equal(draw, e["draw"]), tag
        assert np.array_equal(first, e["map"]), tag


@pytest.mark.parametrize("name", ["dd_bb_gp", "dd_bb_gp_swept",
                                  "gp_nich_swept", "nich2", "le_gp_nich",
                                  "only_empty_k3", "dpd_other", "bnb",
                                  "mixed4", "mixed4_swept"])
def test_every_feature_as_target_under_per_row_masks(name):
    c = fe.case(name)
    gpu = engine_of(name)
    before = snapshot(gpu)
    q = [v[:NQ] for v in c.qvals]
    F = len(c.osh)
    for target in range(F):
        cand = fe.candidates_for(c.osh[target])
        masks = fe.random_masks(NQ, F, 100 + target)
        e = fe.expect(c.orc, q, masks, target, cand, seed_state(),
                      pe.DRAW_BASE)
        check(gpu, q, target, cand, masks, e, "%s target %d" % (name, target))
    assert same(before, snapshot(gpu))


def test_dd256_k1025_all_candidates():
    """four strips of 64 candidates and the base slot; K is no multiple of
    any tile"""
    c = fe.case("dd256_k1025")
    gpu = engine_of("dd256_k1025")
    q = [v[:24] for v in c.qvals]
    e = fe.expect(c.orc, q, None, 0, None, seed_state(), pe.DRAW_BASE)
    assert e["joint"].shape == (24, 256)
    check(gpu, q, 0, None, None, e, "dd256_k1025")


def test_dpd10000_k8193_seventy_candidates():
    c = fe.case("dpd10000_k8193")
    gpu = engine_of("dpd10000_k8193")
    q = [v[:8] for v in c.qvals]
    cand = np.r_[np.arange(0, 6700, 100), 9999, 123456,
                 pe.OTHER].astype(np.uint32)
    assert len(cand) == 70
    e = fe.expect(c.orc, q, None, 0, cand, seed_state(), pe.DRAW_BASE)
    assert np.isfinite(e["joint"]).any(1).all()
    check(gpu, q, 0, cand, None, e, "dpd10000_k8193")


# ---------------------------------------------------------------------------
# identities that need no oracle


@pytest.mark.parametrize("name,target", [("dd_bb_gp_swept", 0),
                                         ("mixed4_swept", 1),
                                         ("gp_nich_swept", 1),
                                         ("le_gp_nich", 0)])
def test_observed_joint_is_predicts_logp_and_mask_zero_its_prior_total(name,
                                                                       target):
    c = fe.case(name)
    gpu = engine_of(name)
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


@pytest.mark.parametrize("name,target", [("mixed4", 1), ("dd_bb_gp_swept", 2)])
def test_permuting_queries_and_candidates_permutes_the_results(name, target):
    c = fe.case(name)
    gpu = engine_of(name)
    F = len(c.osh)
    q = [v[:NQ] for v in c.qvals]
    masks = fe.random_masks(NQ, F, 9)
    sh = c.osh[target]
    cand = fe.candidates_for(sh)
    values = fe.default_candidates(sh) if cand is None else cand
    rng = np.random.default_rng(3)
    perm = rng.permutation(NQ)
    cperm = rng.permutation(len(values))
    for staged in FORMS:
        joint, base, first = gpu.predict_feature(q, target, values, masks,
                                                 "map", staged=staged)
        joint_p, base_p, first_p = gpu.predict_feature(
            [v[perm] for v in q], target, values, masks[perm], "map",
            staged=staged)
        assert np.array_equal(bits(joint_p), bits(joint[perm]))
        assert np.array_equal(bits(base_p), bits(base[perm]))
        assert np.array_equal(first_p, first[perm])
        # the draw goes with its own step: row perm[i] drawn at step i
        for i in (0, 5, NQ - 1):
            _, _, d = gpu.predict_feature(
                [v[perm[i]:perm[i] + 1] for v in q], target, values,
                masks[perm[i]:perm[i] + 1], "sample", seed=4, draw_base=i,
                staged=staged)
            _, _, dp = gpu.predict_feature(
                [v[perm] for v in q], target, values, masks[perm], "sample",
                seed=4, staged=staged)
            assert d[0] == dp[i]
        joint_c, base_c, _ = gpu.predict_feature(q, target, values[cperm],
                                                 masks, None, staged=staged)
        assert np.array_equal(bits(joint_c), bits(joint[:, cperm]))
        assert np.array_equal(bits(base_c), bits(base))


# ---------------------------------------------------------------------------
# geometry


def feature_dev(gpu, words, masks, n, target, cand, mode, staged, want=(1, 1, 1),
                pad=64):
    """predict_feature_dev on the first n rows into sentinel-filled device
    buffers with padding -> (joint, base, choice) flat, padding included"""
    import torch
    from distributions_amd import _core
    C = len(gpu.core.feature_candidates(target, cand))
    cols = [torch.from_numpy(np.ascontiguousarray(w[:n]).view(np.int32)
                             .copy()).cuda() for w in words]
    mk = torch.from_numpy(masks[:n].view(np.int32).copy()).cuda()
    joint = torch.full((n * C + pad,), SENTINEL, dtype=torch.float32,
                       device="cuda")
    base = torch.full((n + pad,), SENTINEL, dtype=torch.float32,
                      device="cuda")
    choice = torch.full((n + pad,), CHOICE_SENTINEL, dtype=torch.int32,
                        device="cuda")
    torch.cuda.synchronize()
    gpu.core.predict_feature_dev(
        [int(t.data_ptr()) for t in cols], n, int(mk.data_ptr()), target,
        cand, int(joint.data_ptr()) if want[0] else 0,
        int(base.data_ptr()) if want[1] else 0,
        int(choice.data_ptr()) if want[2] else 0, mode, seed_state(),
        pe.DRAW_BASE, 0 if staged else _core.PREDICT_FEATURE_RECOMPUTE)
    torch.cuda.synchronize()
    return joint.cpu().numpy(), base.cpu().numpy(), choice.cpu().numpy()


@pytest.mark.parametrize("staged", FORMS)
def test_rows_chunks_and_optional_outputs(staged):
    """n around the wave and the chunk (100 rows), nothing written past n * C,
    n, n; each output alone, `choice` without `joint` through the scratch"""
    name, target, n_all = "mixed4", 1, 257
    c = fe.case(name)
    gpu = engine_of(name)
    F = len(c.osh)
    words = pe.query_words(c.orc, c.qvals)
    masks = fe.random_masks(n_all, F, 21)
    e = fe.expect(c.orc, [v[:n_all] for v in c.qvals], masks, target, None,
                  seed_state(), pe.DRAW_BASE)
    C = e["joint"].shape[1]
    gpu.set_option("debug.predict_chunk", 100)
    try:
        for n in (1, 63, 64, 65, 257):
            for mode, key in ((0, "draw"), (1, "map")):
                joint, base, choice = feature_dev(gpu, words, masks, n,
                                                  target, None, mode, staged)
                assert np.array_equal(bits(joint[:n * C]),
                                      bits(e["joint"][:n].ravel())), (n, mode)
                assert np.array_equal(bits(base[:n]), bits(e["base"][:n]))
                assert np.array_equal(choice[:n].view(np.uint32), e[key][:n])
                assert np.all(joint[n * C:] == SENTINEL)
                assert np.all(base[n:] == SENTINEL)
                assert np.all(choice[n:] == CHOICE_SENTINEL)
            for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
                joint, base, choice = feature_dev(gpu, words, masks, n,
                                                  target, None, 0, staged,
                                                  want)
                if want[0]:
                    assert np.array_equal(bits(joint[:n * C]),
                                          bits(e["joint"][:n].ravel()))
                    assert np.all(joint[n * C:] == SENTINEL)
                else:
                    assert np.all(joint == SENTINEL)
                if want[1]:
                    assert np.array_equal(bits(base[:n]), bits(e["base"][:n]))
                    assert np.all(base[n:] == SENTINEL)
                else:
                    assert np.all(base == SENTINEL)
                if want[2]:
                    assert np.array_equal(choice[:n].view(np.uint32),
                                          e["draw"][:n])
                    assert np.all(choice[n:] == CHOICE_SENTINEL)
                else:
                    assert np.all(choice == CHOICE_SENTINEL)
        # no rows: nothing happens
        joint, base, choice = feature_dev(gpu, words, masks, 0, target, None,
                                          0, staged)
        assert np.all(joint == SENTINEL) and np.all(base == SENTINEL)
        assert np.all(choice == CHOICE_SENTINEL)
    finally:
        gpu.set_option("debug.predict_chunk", 1 << 22)


@pytest.mark.parametrize("C", [1, 63, 64, 65])
def test_candidate_counts_around_the_wave(C):
    """C + 1 slots: rows share a wave, fill one, and spill into the next"""
    name, n = "mixed4_swept", 37
    c = fe.case(name)
    gpu = engine_of(name)
    q = [v[:n] for v in c.qvals]
    masks = fe.random_masks(n, len(c.osh), 5)
    cand = (np.arange(C) * 7 % 70).astype(np.uint32)      # DD(70), repeats
    e = fe.expect(c.orc, q, masks, 3, cand, seed_state(), pe.DRAW_BASE)
    check(gpu, q, 3, cand, masks, e, "C=%d" % C)
    reals = np.linspace(-3, 3, C).astype(np.float32)      # NICH in the middle
    e = fe.expect(c.orc, q, masks, 2, reals, seed_state(), pe.DRAW_BASE)
    check(gpu, q, 2, reals, masks, e, "C=%d reals" % C)


# ---------------------------------------------------------------------------
# rules


def test_refused_with_a_batch_open():
    c = fe.case("dd_bb_gp")
    gpu = c.engine()          # (its own engine: the state moves)
    q = [v[:NQ] for v in c.qvals]
    st = ol.oracle().orc_rng_seed(3)
    gpu.core.batch_sample(0, 1024, st, 0)
    with pytest.raises(RuntimeError, match="batch open"):
        gpu.predict_feature(q, 0)
    gpu.core.batch_apply_local()
    gpu.core.batch_finish()
    gpu.predict_feature(q, 0)


@pytest.mark.parametrize("staged", FORMS)
def test_bad_values_and_candidates(staged):
    name = "dd_bb_gp"
    c = fe.case(name)
    gpu = engine_of(name)
    n = 200
    q = [v[:n].copy() for v in c.qvals]
    e = fe.expect(c.orc, [v[:NQ] for v in q], None, 2,
                  fe.COUNT_CANDIDATES, seed_state(), pe.DRAW_BASE)
    gpu.set_option("debug.predict_chunk", 64)
    try:
        bad = [v.copy() for v in q]
        bad[1][150] = 2
        bad[1][130] = 2                  # the first offending row is named
        bad[0][170] = 200                # (a later row, an earlier feature)
        with pytest.raises(RuntimeError, match="row 130, feature 1"):
            gpu.predict_feature(bad, 2, fe.COUNT_CANDIDATES, staged=staged)
        # the same words in cells that are not observed are never read, and
        # the target's column may be missing altogether
        masks = np.full(n, 0b111, np.uint32)
        masks[[130, 150]] = 0b101
        masks[170] = 0b110
        ok = gpu.predict_feature(bad, 2, fe.COUNT_CANDIDATES, masks,
                                 staged=staged)
        clean = gpu.predict_feature([q[0], q[1], None], 2,
                                    fe.COUNT_CANDIDATES, masks,
                                    staged=staged)
        for a, b in zip(ok, clean):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # a bad word in the TARGET's column is not read either
        bad = [v.copy() for v in q]
        bad[0][:] = 99
        j0, b0, _ = gpu.predict_feature(bad, 0, None, None, None,
                                        staged=staged)
        j1, b1, _ = gpu.predict_feature([None, q[1], q[2]], 0, None, None,
                                        None, staged=staged)
        assert np.array_equal(bits(j0), bits(j1))
        assert np.array_equal(bits(b0), bits(b1))
        # candidates are validated on the host, by index
        with pytest.raises(RuntimeError, match="candidate 2 "):
            gpu.predict_feature(q, 0, [0, 7, 8, 1], staged=staged)
        with pytest.raises(RuntimeError, match="candidate 1 "):
            gpu.predict_feature(q, 1, [1, 2], staged=staged)
        with pytest.raises(RuntimeError, match="candidate list"):
            gpu.predict_feature(q, 2, staged=staged)
        # process and engine go on
        joint, base, first = gpu.predict_feature(
            [v[:NQ] for v in q], 2, fe.COUNT_CANDIDATES, staged=staged)
        assert np.array_equal(bits(joint), bits(e["joint"]))
        assert np.array_equal(bits(base), bits(e["base"]))
        assert np.array_equal(first, e["map"])
    finally:
        gpu.set_option("debug.predict_chunk", 1 << 22)


def test_predict_feature_torch_returns_device_tensors():
    import torch
    name, target = "mixed4", 1
    c = fe.case(name)
    gpu = engine_of(name)
    q = [v[:NQ] for v in c.qvals]
    masks = fe.random_masks(NQ, len(c.osh), 33)
    words = pe.query_words(c.orc, q)
    cols = [torch.from_numpy(w.view(np.int32).copy()).cuda() for w in words]
    cols[target] = None
    mk = torch.from_numpy(masks.view(np.int32).copy()).cuda()
    for mode in ("sample", "map", None):
        host = gpu.predict_feature(q, target, None, masks, mode,
                                   seed=pe.DRAW_SEED, draw_base=pe.DRAW_BASE)
        dev = gpu.predict_feature_torch(cols, target, None, mk, mode,
                                        seed=pe.DRAW_SEED,
                                        draw_base=pe.DRAW_BASE)
        assert dev[0].is_cuda and dev[1].is_cuda
        assert np.array_equal(bits(dev[0].cpu().numpy()), bits(host[0]))
        assert np.array_equal(bits(dev[1].cpu().numpy()), bits(host[1]))
        if mode is None:
            assert dev[2] is None and host[2] is None
        else:
            assert dev[2].is_cuda
            assert np.array_equal(dev[2].cpu().numpy().view(np.uint32),
                                  host[2])
