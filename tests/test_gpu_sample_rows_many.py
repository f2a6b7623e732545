"""dist_gibbs_sample_rows_many (k_sample_base_many, k_sample_prior_lik_many,
k_ensemble_fold, k_sample_rows_pick in both instances): whole rows and missing
cells drawn from an ensemble of M engines.

Bit for bit against the expectation tests/sample_many_expect.py composes from
the oracle (and tests/test_sample_many_oracle.py holds to the float64 law) --
base, member and group in every bit, the cells of DD, BB and DPD in every bit,
those of GP and NICH against dist_group_sample_value, whose double log /
lgamma may part from the device's in a last place (at most 1 cell in 10^5, as
tests/test_gpu_sample_rows.py has it) -- and against the two identities of the
definition, in every bit of every kind:
  member == predict_feature_many's member (for a target no row observes);
  row q  == row q of Gibbs.sample_rows on engine member[q], over all rows.
Then launch geometry (n around a wave and a workgroup's chunk at M = 2, K = 4
beside K = 1025, M = 66 in chunks of 37, each output alone, sentinels), no
mask against a zero mask, everything observed, completion in place, the error
word, the chains of sweep_sequential_many, the refusals, and the law of 2 *
10^5 rows on the device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ensemble_expect as ee  # noqa: E402
import feature_expect as fe  # noqa: E402
import oracle_lib as ol  # noqa: E402
import predict_expect as pe  # noqa: E402
import sample_expect as sx  # noqa: E402
import sample_many_expect as sm  # noqa: E402
from test_gpu_predict import same, snapshot  # noqa: E402
from test_gpu_predict_feature_many import (  # noqa: E402
    ENSEMBLES, K4_K1025, masks_of, same_bits)
# (without the entry point there is nothing to test: the module does not load)
from distributions_amd.engine import (  # noqa: E402,F401
    sample_rows_many, sample_rows_many_torch)

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
WORD_SENTINEL = 0x5EEDF00D
MASK_SEED = 23
INEXACT = (ol.GP, ol.BNB, ol.NICH)

OWN = dict(ENSEMBLES)
OWN.update({
    "dd": lambda: ee.Ensemble("dd", ee.SPECS3, nq=96),
    # chunks of predict_many_pick_rows(2) = 128 rows: 257 rows are three
    # workgroups per member, the last of one row
    "m2": lambda: ee.Ensemble("dd_bb_gp", ee.SPECS3[1:], nq=257),
    "k4_k1025": lambda: ee.Ensemble("dd_bb_gp", K4_K1025, nq=96),
})
_ENS = {}
_GPUS = {}


def ensemble(name):
    if name not in _ENS:
        _ENS[name] = OWN[name]()
    return _ENS[name]


def engines_of(name):
    """one set of engines per ensemble, shared: the reader leaves them as
    they were"""
    if name not in _GPUS:
        _GPUS[name] = ensemble(name).engines()
    return _GPUS[name]


def seeds():
    L = ol.oracle()
    return L.orc_rng_seed(sm.DRAW_SEED), L.orc_rng_seed(sm.MEMBER_SEED)


def expect(ens, observed, n=None, draw_base=sm.DRAW_BASE, qvals=None,
           members=None):
    ms = ens.members if members is None else members
    seed, mseed = seeds()
    return sm.expect_many([m.orc for m in ms], [m.gsh for m in ms],
                          ens.qvals if qvals is None else qvals, observed,
                          seed, mseed, draw_base, ens.le is not None, nq=n)


def words_of(ens, cols):
    return [ol.value_words(s.kind, v)
            for s, v in zip(ens.members[0].osh, cols)]


def host(gpus, ens, observed, n=None, draw_base=sm.DRAW_BASE, qvals=None):
    from distributions_amd import engine
    q = ens.qvals if qvals is None else qvals
    cols, groups, members, base = engine.sample_rows_many(
        gpus, n=n, values=None if observed is None else q, observed=observed,
        seed=sm.DRAW_SEED, draw_base=draw_base, base=True)
    return words_of(ens, cols), groups, members, base


def check_against(ens, got, e, what):
    """base, member, group in every bit; the cells of the exact kinds in
    every bit, those of the others counted -> (cells, mismatches)"""
    cols, groups, members, base = got
    assert same_bits(base, e["base"]), what
    assert np.array_equal(members, e["member"]), what
    assert np.array_equal(groups, e["group"]), what
    cells = wrong = 0
    for f, osh in enumerate(ens.members[0].osh):
        if osh.kind in INEXACT:
            cells += len(cols[f])
            wrong += int((cols[f] != e["cols"][f]).sum())
        else:
            assert np.array_equal(cols[f], e["cols"][f]), (what, f)
    return cells, wrong


def check_rows_are_the_members_own(ens, gpus, got, observed, n, draw_base,
                                   qvals=None):
    """row q == row q of Gibbs.sample_rows on engine member[q], run over all
    rows: every bit of every kind"""
    cols, groups, members, _ = got
    q = ens.qvals if qvals is None else qvals
    for i, g in enumerate(gpus):
        rows = members == i
        if not rows.any():
            continue
        c1, g1 = g.sample_rows(n=n, values=None if observed is None else q,
                               observed=observed, seed=sm.DRAW_SEED,
                               draw_base=draw_base)
        assert np.array_equal(groups[rows], g1[rows]), i
        for a, b in zip(cols, words_of(ens, c1)):
            assert np.array_equal(a[rows], b[rows]), i


# name: ensemble, a target no mask observes for the identity with
# predict_feature_many, its candidates
CASES = {
    "dd_bb_gp": ("dd_bb_gp", 0, None),
    "gp_nich": ("gp_nich", 0, fe.COUNT_CANDIDATES),
    "dd": ("dd", 0, None),
    "dpd_other_mixed": ("dpd_other_mixed", 0, None),
    "le_m1": ("le_m1", 1, None),
    "le_m2": ("le_m2", 0, None),
    "le_m5": ("le_m5", 1, None),
    "only_empty_member": ("only_empty_member", 1, None),
    "eight3": ("eight3", 7, None),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_sample_rows_many_is_the_expectation_bit_for_bit(name):
    from distributions_amd import engine
    ens_name, target, cand = CASES[name]
    ens, gpus = ensemble(ens_name), engines_of(ens_name)
    before = [snapshot(g) for g in gpus]
    F = len(ens.members[0].osh)
    n = min(ens.nq, 96)
    q = [v[:n] for v in ens.qvals]
    full = (1 << F) - 1
    masks = masks_of(n, F, MASK_SEED)
    cells = wrong = 0
    # per-row masks; a zero mask and no mask (both instances); everything
    # observed
    zero = np.zeros(n, np.uint32)
    for what, observed in (("masks", masks), ("zero", zero), ("none", None),
                           ("full", np.full(n, full, np.uint32))):
        e = expect(ens, observed, n, qvals=q)
        got = host(gpus, ens, observed, n, qvals=q)
        c, w = check_against(ens, got, e, (name, what))
        cells, wrong = cells + c, wrong + w
        check_rows_are_the_members_own(ens, gpus, got, observed, n,
                                       sm.DRAW_BASE, qvals=q)
        if what == "zero":
            at_zero = got
        if what == "none":
            assert same_bits(got[3], at_zero[3])
            assert np.array_equal(got[1], at_zero[1])
            assert np.array_equal(got[2], at_zero[2])
            for a, b in zip(got[0], at_zero[0]):
                assert np.array_equal(a, b)
        if what == "full":
            # nothing is drawn but the member and its group: predict_many's
            # planes are wb, and its group of the same member is the group
            given = words_of(ens, q)
            for a, b in zip(got[0], given):
                assert np.array_equal(a, b)
            if name != "dpd_other_mixed":     # (OTHER rows: -inf planes)
                lp, mem, grp, planes, _ = engine.predict_many(
                    gpus, q, "sample", seed=sm.DRAW_SEED,
                    draw_base=sm.DRAW_BASE, members=True)
                assert same_bits(planes, e["wb"])
                assert same_bits(lp, got[3])
                assert np.array_equal(mem, got[2])
                assert np.array_equal(grp, got[1])
    print("%s: M=%d, K=%s, %d rows x 4 calls; %d cells of GP / NICH compared "
          "with the host entry, %d differ" % (
              name, ens.M, [m.K for m in ens.members], n, cells, wrong))
    assert wrong * 100000 <= cells
    # member == predict_feature_many's member where no row observes the target
    hidden = masks & ~np.uint32(1 << target)
    kind = ens.members[0].osh[target].kind
    if cand is not None:
        cand = np.array(cand, np.float32 if kind == ol.NICH else np.uint32)
    got = host(gpus, ens, hidden, n, qvals=q)
    _, base, _, member, _, pb, _ = engine.predict_feature_many(
        gpus, q, target, cand, hidden, "sample", seed=sm.DRAW_SEED,
        draw_base=sm.DRAW_BASE, members=True)
    assert np.array_equal(got[2], member)
    assert same_bits(got[3], base)
    assert same_bits(expect(ens, hidden, n, qvals=q)["wb"], pb)
    for b, g in zip(before, gpus):
        assert same(b, snapshot(g))
        assert g.validate()["code"] == 0


def test_one_engine_is_sample_rows():
    ens, gpus = ensemble("gp_nich"), engines_of("gp_nich")
    n = 96
    q = [v[:n] for v in ens.qvals]
    masks = fe.random_masks(n, 2, MASK_SEED)
    for observed in (masks, None):
        for i, g in enumerate(gpus):
            cols, groups, members, base = host(gpus[i:i + 1], ens, observed,
                                               n, qvals=q)
            c1, g1 = g.sample_rows(n=n, values=None if observed is None
                                   else q, observed=observed,
                                   seed=sm.DRAW_SEED, draw_base=sm.DRAW_BASE)
            assert np.all(members == 0)
            assert np.array_equal(groups, g1)
            for a, b in zip(cols, words_of(ens, c1)):
                assert np.array_equal(a, b)


# ---------------------------------------------------------------------------
# geometry


def many_dev(gpus, words, n, observed, want="gmb", in_place=False, pad=8,
             draw_base=sm.DRAW_BASE, flags=0):
    """sample_rows_many_dev on the first n rows into sentinel-filled, padded
    device buffers -> dict of host copies (o: the columns as words, g: groups,
    m: members, b: base)"""
    import torch
    from distributions_amd import _core
    F = len(gpus[0].shareds)

    def ints(k):
        return torch.from_numpy(np.full(k + pad, WORD_SENTINEL, np.uint32)
                                .view(np.int32)).cuda()

    vals = None
    if words is not None:
        vals = [None if w is None else torch.from_numpy(
            np.ascontiguousarray(w[:n]).view(np.int32).copy()).cuda()
            for w in words]
    mask = None if observed is None else torch.from_numpy(
        np.ascontiguousarray(observed[:n]).view(np.int32).copy()).cuda()
    outs = vals if in_place else [ints(n) for _ in range(F)]
    buf = dict(g=ints(n), m=ints(n),
               b=torch.full((n + pad,), SENTINEL, dtype=torch.float32,
                            device="cuda"))
    torch.cuda.synchronize()
    seed, mseed = seeds()
    _core.sample_rows_many_dev(
        [None if g is None else g.core for g in gpus],
        None if vals is None
        else [0 if v is None else int(v.data_ptr()) for v in vals], n,
        0 if mask is None else int(mask.data_ptr()),
        [int(o.data_ptr()) for o in outs],
        int(buf["g"].data_ptr()) if "g" in want else 0,
        int(buf["m"].data_ptr()) if "m" in want else 0,
        int(buf["b"].data_ptr()) if "b" in want else 0,
        seed, mseed, draw_base, flags)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in buf.items()}
    out["g"] = out["g"].view(np.uint32)
    out["m"] = out["m"].view(np.uint32)
    out["o"] = [o.cpu().numpy().view(np.uint32) for o in outs]
    return out


def check_dev(out, ref, n, want="gmb", columns=True):
    """every asked output the reference's first n rows, everything else
    untouched (ref: host()'s tuple of a call over at least n rows)"""
    cols, groups, members, base = ref
    for key, r in (("g", groups), ("m", members)):
        if key in want:
            assert np.array_equal(out[key][:n], r[:n]), key
            assert np.all(out[key][n:] == WORD_SENTINEL), key
        else:
            assert np.all(out[key] == WORD_SENTINEL), key
    if "b" in want:
        assert same_bits(out["b"][:n], base[:n])
        assert np.all(out["b"][n:] == SENTINEL)
    else:
        assert np.all(out["b"] == SENTINEL)
    if columns:
        for a, b in zip(out["o"], cols):
            assert np.array_equal(a[:n], b[:n])
            assert np.all(a[n:] == WORD_SENTINEL)


def test_row_counts_around_a_wave_and_a_chunk_at_two_members():
    """n = 1, 63, 64, 65, 257 at M = 2: the pick kernel's chunk is 128 rows,
    so 257 rows are three workgroups per member with partial waves in their
    lists, and n = 1 leaves one member without a row; several launches
    (debug.predict_chunk = 100); each output alone; nothing written past n"""
    ens, gpus = ensemble("m2"), engines_of("m2")
    N = ens.nq
    given = words_of(ens, ens.qvals)
    masks = fe.random_masks(N, 3, MASK_SEED)
    ref = host(gpus, ens, masks)
    unc = host(gpus, ens, None, N)
    c, w = check_against(ens, ref, expect(ens, masks), "m2 masks")
    c2, w2 = check_against(ens, unc, expect(ens, None, N), "m2 none")
    assert (w + w2) * 100000 <= c + c2
    assert len(set(ref[2].tolist())) == 2 and len(set(unc[2].tolist())) == 2
    try:
        for chunk in (1 << 22, 100):
            gpus[0].set_option("debug.predict_chunk", chunk)
            for n in (1, 63, 64, 65, 257):
                check_dev(many_dev(gpus, given, n, masks), ref, n)
                check_dev(many_dev(gpus, None, n, None), unc, n)
        gpus[0].set_option("debug.predict_chunk", 100)
        for want in ("g", "m", "b", ""):
            check_dev(many_dev(gpus, given, N, masks, want), ref, N, want)
            check_dev(many_dev(gpus, None, N, None, want), unc, N, want)
        # one call against two with draw_base advanced
        a = many_dev(gpus, [g[:100] for g in given], 100, masks[:100], pad=0)
        b = many_dev(gpus, [g[100:] for g in given], 157, masks[100:], pad=0,
                     draw_base=sm.DRAW_BASE + 100)
        assert np.array_equal(np.r_[a["g"], b["g"]], ref[1])
        assert np.array_equal(np.r_[a["m"], b["m"]], ref[2])
        for f in range(3):
            assert np.array_equal(np.r_[a["o"][f], b["o"][f]], ref[0][f])
        # no rows: nothing happens
        out = many_dev(gpus, None, 0, None)
        check_dev(out, unc, 0, "")
    finally:
        gpus[0].set_option("debug.predict_chunk", 1 << 22)


def test_four_groups_beside_1025_in_one_call():
    ens, gpus = ensemble("k4_k1025"), engines_of("k4_k1025")
    assert [m.K for m in ens.members] == [4, 1025]
    masks = fe.random_masks(ens.nq, 3, MASK_SEED)
    cells = wrong = 0
    for observed in (masks, None):
        e = expect(ens, observed, ens.nq)
        got = host(gpus, ens, observed, ens.nq)
        c, w = check_against(ens, got, e, "k4_k1025")
        cells, wrong = cells + c, wrong + w
        assert len(set(got[2].tolist())) == 2
        check_rows_are_the_members_own(ens, gpus, got, observed, ens.nq,
                                       sm.DRAW_BASE)
    assert wrong * 100000 <= cells


def test_66_members_in_chunks_of_37_and_members_no_row_draws():
    ens, gpus = ensemble("small66"), engines_of("small66")
    assert ens.M == 66
    N = ens.nq
    given = words_of(ens, ens.qvals)
    masks = fe.random_masks(N, 3, MASK_SEED)
    e = expect(ens, masks)
    ref = host(gpus, ens, masks)
    c, w = check_against(ens, ref, e, "small66")
    assert w * 100000 <= c
    check_rows_are_the_members_own(ens, gpus, ref, masks, None, sm.DRAW_BASE)
    unc = host(gpus, ens, None, N)
    c, w = check_against(ens, unc, expect(ens, None, N), "small66 none")
    assert w * 100000 <= c
    try:
        gpus[0].set_option("debug.predict_chunk", 37)
        check_dev(many_dev(gpus, given, N, masks), ref, N)
        check_dev(many_dev(gpus, None, N, None), unc, N)
        # 37 rows cannot reach 66 members: at least 29 lists stay empty
        out = many_dev(gpus, given, 37, masks)
        check_dev(out, ref, 37)
        assert len(set(out["m"][:37].tolist())) < 66
    finally:
        gpus[0].set_option("debug.predict_chunk", 1 << 22)


def test_in_place_through_the_torch_form():
    import torch
    from distributions_amd import engine
    ens, gpus = ensemble("gp_nich"), engines_of("gp_nich")
    n = 130
    q = [np.resize(v, n) for v in ens.qvals]
    given = words_of(ens, q)
    masks = fe.random_masks(n, 2, MASK_SEED + 1)
    ref = host(gpus, ens, masks, qvals=q)
    # unobserved cells filled with 0xFFFFFFFF are never read; completion in
    # place writes only those
    filled = []
    for f in range(2):
        w = given[f].copy()
        w[((masks >> f) & 1) == 0] = 0xFFFFFFFF
        filled.append(w)
    vals = [torch.from_numpy(filled[0].view(np.int32).copy()).cuda(),
            torch.from_numpy(filled[1].view(np.float32).copy()).cuda()]
    mk = torch.from_numpy(masks.view(np.int32).copy()).cuda()
    cols, groups, members, base = engine.sample_rows_many_torch(
        gpus, values=vals, observed=mk, seed=sm.DRAW_SEED,
        draw_base=sm.DRAW_BASE, out=vals, base=True)
    assert cols[0] is vals[0] and cols[1] is vals[1]
    assert groups.is_cuda and members.is_cuda and base.is_cuda
    assert cols[1].dtype == torch.float32
    assert np.array_equal(groups.cpu().numpy().view(np.uint32), ref[1])
    assert np.array_equal(members.cpu().numpy().view(np.uint32), ref[2])
    assert same_bits(base.cpu().numpy(), ref[3])
    for f in range(2):
        assert np.array_equal(vals[f].cpu().numpy().view(np.uint32),
                              ref[0][f])
    # no mask: fresh tensors on the current device
    unc = host(gpus, ens, None, n)
    cols, groups, members = engine.sample_rows_many_torch(
        gpus, n=n, seed=sm.DRAW_SEED, draw_base=sm.DRAW_BASE)
    assert all(t.is_cuda for t in cols)
    assert np.array_equal(members.cpu().numpy().view(np.uint32), unc[2])
    for f in range(2):
        assert np.array_equal(cols[f].cpu().numpy().view(np.uint32),
                              unc[0][f])
    with pytest.raises(RuntimeError, match="observed mask"):
        engine.sample_rows_many(gpus, values=q)


def test_the_chains_of_sweep_sequential_many():
    """8 chains advanced in one launch, sampled from in one call, advanced
    again: the reader left every engine alone"""
    from distributions_amd import _core, engine
    from test_gpu_chains import assert_same, make_chain
    import workloads
    m, n, k = 8, 300, 20
    chains = [make_chain("dd_bb_gp", n, k + i, 4.0 + i, 0.3, 1 + i % 2,
                         60 + i) for i in range(m)]
    gpus = [g for _, g in chains]
    states = np.array([_core.rng_seed(500 + i) for i in range(m)], np.uint32)
    got = engine.sweep_sequential_many(gpus, 0, n, states)
    for i, (orc, _) in enumerate(chains):
        assert int(got[i]) == orc.gibbs_sequential(0, n, int(states[i]))
    _, _, q, _ = workloads.make("dd_bb_gp", 200, 1, seed=pe.QSEED)
    observed = fe.random_masks(200, 3, MASK_SEED)
    seed, mseed = seeds()
    e = sm.expect_many([o for o, _ in chains], [g.shareds for g in gpus], q,
                       observed, seed, mseed, 0, False)
    cols, groups, members, base = engine.sample_rows_many(
        gpus, values=q, observed=observed, seed=sm.DRAW_SEED, base=True)
    assert same_bits(base, e["base"])
    assert np.array_equal(members, e["member"])
    assert np.array_equal(groups, e["group"])
    assert len(set(members.tolist())) > 1
    for f in (0, 1):
        assert np.array_equal(cols[f], e["cols"][f])
    assert int((cols[2] != e["cols"][2]).sum()) * 100000 <= 200
    again = engine.sweep_sequential_many(gpus, 0, n, got)
    for i, (orc, gpu) in enumerate(chains):
        assert int(again[i]) == orc.gibbs_sequential(0, n, int(got[i]))
        assert_same(orc, gpu, "chain %d after sample_rows_many" % i)


# ---------------------------------------------------------------------------
# rules


def test_an_observed_value_out_of_its_domain_is_named():
    ens, gpus = ensemble("dd_bb_gp"), engines_of("dd_bb_gp")
    q = ens.qvals
    n = ens.nq
    full = np.full(n, 0b111, np.uint32)
    good = host(gpus, ens, full)
    gpus[0].set_option("debug.predict_chunk", 64)
    try:
        bad = [c.copy() for c in q]
        bad[1][211] = 2
        bad[1][130] = 2                 # the first offending row is named
        bad[0][250] = 200               # (a later row, an earlier feature)
        with pytest.raises(RuntimeError, match="row 130, feature 1"):
            host(gpus, ens, full, qvals=bad)
        # the same words in unobserved cells are never read
        hidden = full.copy()
        hidden[[130, 211]] = 0b101
        hidden[250] = 0b110
        a = host(gpus, ens, hidden, qvals=bad)
        b = host(gpus, ens, hidden)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        for f in range(3):
            seen = ((hidden >> f) & 1) == 1
            assert np.array_equal(a[0][f][~seen], b[0][f][~seen])
        # an observed cell of a column that was not given
        holes = list(q)
        holes[2] = None
        with pytest.raises(RuntimeError, match="row 0, feature 2"):
            host(gpus, ens, full, qvals=holes)
        # process and engines go on
        again = host(gpus, ens, full)
        assert np.array_equal(again[1], good[1])
        assert np.array_equal(again[2], good[2])
    finally:
        gpus[0].set_option("debug.predict_chunk", 1 << 22)


def test_an_open_batch_on_one_member_is_refused():
    ens = ensemble("dd_bb_gp")
    gpus = [m.engine() for m in ens.members]    # (their own: a state moves)
    gpus[1].core.batch_sample(0, 256, ol.oracle().orc_rng_seed(3), 0)
    with pytest.raises(RuntimeError, match="batch open"):
        host(gpus, ens, None, 4)
    gpus[1].core.batch_apply_local()
    gpus[1].core.batch_finish()
    host(gpus, ens, None, 4)


def test_refused_engine_lists_and_arguments():
    from distributions_amd import engine
    ens, gpus = ensemble("dd_bb_gp"), engines_of("dd_bb_gp")
    with pytest.raises(RuntimeError, match="one feature list"):
        host([gpus[0], engines_of("gp_nich")[0]], ens, None, 4)
    other_dim = engine.Gibbs(1.0, 0.0, [engine.dd_shared([0.5] * 12),
                                        engine.bb_shared(0.5, 2.0),
                                        engine.gp_shared(1.0, 1.0)])
    other_dim.load_rows_unassigned([np.zeros(4, np.uint32)] * 3, 1)
    with pytest.raises(RuntimeError, match="one feature list"):
        host([gpus[0], other_dim], ens, None, 4)
    with pytest.raises(RuntimeError, match="one clustering model"):
        host([gpus[0], engines_of("le_m1")[0]], ens, None, 4)
    with pytest.raises(RuntimeError, match="null engine"):
        host([gpus[0], None], ens, None, 4)
    with pytest.raises(RuntimeError, match="the same engine twice"):
        host([gpus[0], gpus[1], gpus[0]], ens, None, 4)
    with pytest.raises(RuntimeError, match="at most 65535 engines"):
        host([gpus[0]] * 65536, ens, None, 4)
    with pytest.raises(RuntimeError, match="no engine"):
        host([], ens, None, 4)
    with pytest.raises(RuntimeError, match="unknown flag"):
        many_dev(gpus, None, 4, None, flags=1)
    with pytest.raises(RuntimeError, match="neither n nor a mask"):
        engine.sample_rows_many(gpus)


# ---------------------------------------------------------------------------
# the law on the device


@pytest.mark.parametrize("name", ["mixed_gp_seen", "real_gp_seen",
                                  "real_nothing_seen"])
def test_law_of_rows_on_the_device(name):
    """2 * 10^5 draws of the CPU test's row under its mask, on the CPU test's
    members, against the float64 law of the unobserved cells (chi-square over
    the joint cells, Kolmogorov-Smirnov for the real alone) and of the member;
    real_nothing_seen goes without a mask, through the other instance"""
    import test_sample_many_oracle as tso
    from distributions_amd import engine
    c = tso.case(name)
    key = "law:" + c.config
    if key not in _GPUS:
        _GPUS[key] = c.ens.engines()
    gpus = _GPUS[key]
    n = 200000
    if c.ob:
        cols, groups, members = engine.sample_rows_many(
            gpus, values=tso.row_of(c.config, c.values, n),
            observed=np.full(n, c.ob, np.uint32), seed=11)
    else:
        cols, groups, members = engine.sample_rows_many(gpus, n=n, seed=11)
    words = [ol.value_words(s.kind, v)
             for s, v in zip(c.ens.members[0].osh, cols)]
    pm = sx.chi2_p(members, np.arange(c.ens.M), c.law.r)
    p = c.p_value(words)
    print("%s: members %s against %s, p = %.3g; cells p = %.3g" % (
        name, np.bincount(members, minlength=c.ens.M), np.round(c.law.r, 4),
        pm, p))
    assert pm > 1e-4 and p > 1e-4
