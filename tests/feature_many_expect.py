"""What dist_gibbs_predict_feature_many must return -- one feature's predictive
given the others, averaged over M engines -- composed from what exists
(tests/feature_expect.py per member, tests/ensemble_expect.py's fold over the
members), and the float64 law it is held to.

TEST INFRASTRUCTURE (imported by tests only).

The expectation (`expect_many`), per query row q, target t, candidates
cand[0..C) and mask observed[q]:
  wj[e][q][c]  feature_expect.expect's joint on member e; under LowEntropy
               minus that member's prior total, one float32 subtraction
  wb[e][q]     the same for base
  joint, base  ensemble_expect.fold over the members: orc_log_sum_exp minus
               orc_fast_log(M), in float32
  choice       orc_sample_from_scores_overwrite over a copy of the FOLDED
               joint[q] on a state positioned by orc_rng_jump(seed_state,
               draw_base + q); for "map" the first maximum
  member       ensemble_expect.fold's draw / first maximum over wb[.][q] on
               the member stream

The float64 law (`law_f64`): per member L_e(q, c), predict_expect.logp_f64 on
the rows completed with cand[c], and B_e(q), the same without the target --
each over the features the row's mask observes -- with their bands; under
LowEntropy minus the member's float64 prior total (its band and one eps
added).  Then ensemble_expect.lse_band over the members, - log M with the
fast_log(M) table term and one eps: exactly how ensemble_expect.law_f64 is
built.  The ensemble's conditional is joint - base, a ratio of averages;
nothing in the bands is fitted to oracle or kernel output.
"""
import ctypes
import math

import numpy as np

import ensemble_expect as ee
import f64_scores as fx
import feature_expect as fe
import oracle_lib as ol
import predict_expect as pe

DRAW_SEED = ee.DRAW_SEED
MEMBER_SEED = ee.MEMBER_SEED
DRAW_BASE = ee.DRAW_BASE


def prior_total(orc):
    """orc_log_sum_exp of the driver's scores alone, float32"""
    K = len(orc)
    prior = np.zeros(K, np.float32)
    orc.L.orc_mix_driver_score_value(orc.h, prior)
    return np.float32(orc.L.orc_log_sum_exp(K, prior))


def choice_of(joint, seed_state, draw_base):
    """-> (draw [nq], map [nq]) over the rows of joint [nq, C]"""
    L = ol.oracle()
    nq, C = joint.shape
    draw = np.zeros(nq, np.uint32)
    first = np.zeros(nq, np.uint32)
    with np.errstate(invalid="ignore"):
        for q in range(nq):
            j = np.ascontiguousarray(joint[q], np.float32)
            first[q] = ee.first_maximum(j)
            st = ctypes.c_uint32(L.orc_rng_jump(seed_state, draw_base + q))
            draw[q] = L.orc_sample_from_scores_overwrite(ctypes.byref(st), C,
                                                         j.copy())
    return draw, first


def expect_many(orcs, qvals, observed, target, cand, seed_state,
                member_seed_state, draw_base, le):
    """-> dict(wj [M, nq, C], wb [M, nq], prior_totals [M], joint [nq, C],
    base [nq], choice_draw, choice_map, member_draw, member_map, per_member:
    feature_expect.expect of each member)"""
    per = [fe.expect(o, qvals, observed, target, cand, seed_state, draw_base)
           for o in orcs]
    totals = np.array([prior_total(o) for o in orcs], np.float32)
    wj = np.stack([p["joint"] for p in per]).astype(np.float32)
    wb = np.stack([p["base"] for p in per]).astype(np.float32)
    if le:
        with np.errstate(invalid="ignore"):
            wj = (wj - totals[:, None, None]).astype(np.float32)
            wb = (wb - totals[:, None]).astype(np.float32)
    M, nq, C = wj.shape
    joint, _, _ = ee.fold(wj.reshape(M, nq * C), member_seed_state, 0)
    joint = joint.reshape(nq, C)
    base, mdraw, mmap = ee.fold(wb, member_seed_state, draw_base)
    cdraw, cmap = choice_of(joint, seed_state, draw_base)
    return dict(wj=wj, wb=wb, prior_totals=totals, joint=joint, base=base,
                choice_draw=cdraw, choice_map=cmap, member_draw=mdraw,
                member_map=mmap, per_member=per)


def candidate_values(shared, cand):
    """the candidates as values: the list given or the whole domain (a DPD
    value the table does not hold is OTHER, dpd.hpp:534-542)"""
    if cand is None:
        return fe.default_candidates(shared)
    v = np.array(cand)
    if shared.kind == ol.DPD:
        v[v >= shared.dim] = fe.OTHER
    return v


class FeatureEnsemble(object):
    """an ensemble_expect.Ensemble with a target, candidates and masks"""

    def __init__(self, ens, target, cand=None, observed=None):
        self.ens, self.target, self.cand = ens, target, cand
        self.observed = observed
        self.le = ens.le is not None
        self.M, self.nq = ens.M, ens.nq
        self.F = len(ens.members[0].osh)
        self.shared = ens.members[0].osh[target]
        self.values = candidate_values(self.shared, cand)
        self.C = len(self.values)
        self._expect = {}
        self._f64 = None

    def expect(self, draw_base=DRAW_BASE):
        if draw_base not in self._expect:
            L = ol.oracle()
            self._expect[draw_base] = expect_many(
                [m.orc for m in self.ens.members], self.ens.qvals,
                self.observed, self.target, self.cand,
                L.orc_rng_seed(DRAW_SEED), L.orc_rng_seed(MEMBER_SEED),
                draw_base, self.le)
        return self._expect[draw_base]

    def f64(self):
        if self._f64 is None:
            self._f64 = law_f64([m.st for m in self.ens.members],
                                self.ens.qvals, self.observed, self.target,
                                self.values, self.le)
        return self._f64


# ---------------------------------------------------------------------------
# float64


def member_f64(state, qvals, observed, target, values):
    """one member -> (Lj [nq, C], bj [nq, C], Lb [nq], bb [nq]): the float64
    joint per candidate and base of every query row over the features its
    mask observes, and the bands of their float32 values"""
    F = len(state.feats)
    nq = len(observed) if observed is not None else len(
        next(v for v in qvals if v is not None))
    full = (1 << F) - 1
    pat = np.full(nq, full, np.int64) if observed is None \
        else (np.asarray(observed, np.int64) & full)
    pat &= ~(1 << target)
    C = len(values)
    Lj, bj = np.zeros((nq, C)), np.zeros((nq, C))
    Lb, bb = np.zeros(nq), np.zeros(nq)
    for p in np.unique(pat):
        idx = np.nonzero(pat == p)[0]
        drop = {f for f in range(F) if f != target and not (p >> f) & 1}
        sj, keep = fe.without(state, drop)
        for c, v in enumerate(values):
            cols = [np.full(len(idx), v, np.asarray(values).dtype)
                    if f == target else np.asarray(qvals[f])[idx]
                    for f in keep]
            Lv, band, _ = pe.logp_f64(sj, cols)
            Lj[idx, c], bj[idx, c] = Lv, band
        sb, keepb = fe.without(state, drop | {target})
        if keepb:
            Lv, band, _ = pe.logp_f64(sb, [np.asarray(qvals[f])[idx]
                                           for f in keepb])
            Lb[idx], bb[idx] = Lv, band
        else:       # nothing observed: the driver's scores alone
            Lb[idx], bb[idx] = ee.prior_total_f64(state)
    return Lj, bj, Lb, bb


def members_f64(states, qvals, observed, target, values, le):
    """-> (Wj [nq, C, M], Bj, Wb [nq, M], Bb): every member's values and
    bands, under LowEntropy normalised by the member's prior total"""
    Wj, Bj, Wb, Bb = [], [], [], []
    for st in states:
        Lj, bj, Lb, bb = member_f64(st, qvals, observed, target, values)
        if le:
            Lp, bp = ee.prior_total_f64(st)
            Lj, Lb = Lj - Lp, Lb - Lp
            bj = bj + bp + fx.EPS * np.abs(Lj)
            bb = bb + bp + fx.EPS * np.abs(Lb)
        Wj.append(Lj)
        Bj.append(bj)
        Wb.append(Lb)
        Bb.append(bb)
    return (np.stack(Wj, 2), np.stack(Bj, 2), np.stack(Wb, 1),
            np.stack(Bb, 1))


def law_f64(states, qvals, observed, target, values, le, variant=None):
    """-> dict(joint [nq, C], joint_band, base [nq], base_band, cond [nq, C]
    = joint - base, cond_band = the two bands summed, r [nq, M]: the member
    responsibilities exp(Wb_e - base) / M).

    variant: a planted bug instead of the law (no bands then):
      "mean_of_conditionals"  cond = the mean over the members of their own
                              conditionals L_e - B_e (joint, base: the law's)
      "mean_of_logs"          the mean of the members' log values
      "no_log_m"              the log of the SUM over the members
      "unnormalised"          LowEntropy without the members' normalisation"""
    M = len(states)
    Wj, Bj, Wb, Bb = members_f64(states, qvals, observed, target, values,
                                 le and variant != "unnormalised")
    nq, C, _ = Wj.shape
    if variant == "mean_of_logs":
        j, b = Wj.mean(2), Wb.mean(1)
        return dict(joint=j, base=b, cond=j - b[:, None])
    Lj, bandj, _ = ee.lse_band(Wj.reshape(nq * C, M), Bj.reshape(nq * C, M))
    Lb, bandb, r = ee.lse_band(Wb, Bb)
    Lj, bandj = Lj.reshape(nq, C), bandj.reshape(nq, C)
    if variant == "no_log_m":
        return dict(joint=Lj, base=Lb, cond=Lj - Lb[:, None])
    log_m = math.log(M)
    Lj, Lb = Lj - log_m, Lb - log_m
    if variant == "mean_of_conditionals":
        return dict(joint=Lj, base=Lb, cond=(Wj - Wb[:, None, :]).mean(2))
    table = abs(float(np.float32(ol.oracle().orc_fast_log(float(M))))
                - log_m)
    bandj = bandj + table + fx.EPS * np.abs(Lj)
    bandb = bandb + table + fx.EPS * np.abs(Lb)
    return dict(joint=Lj, joint_band=bandj, base=Lb, base_band=bandb,
                cond=Lj - Lb[:, None], cond_band=bandj + bandb[:, None], r=r)
