"""What dist_gibbs_sample_rows_many must return -- whole rows and missing cells
drawn from an ensemble of M engines -- composed from what exists, and the
float64 law of a row's unobserved cells given its observed ones.

TEST INFRASTRUCTURE (imported by tests only).

The expectation (`expect_many`), per query row q with mask observed[q]:
  wb[e][q]   orc_log_sum_exp of orc_mix_driver_score_value folded, in feature
             order, with orc_mix_slave_score_value of every OBSERVED feature:
             feature_expect.expect's `base` for a target the row does not
             observe (feature_many_expect.expect_many's wb; the oracle test
             holds the two to each other), here for every mask, the full one
             included; under LowEntropy minus the member's prior total, one
             float32 subtraction
  base, member
             ensemble_expect.fold over the members: orc_log_sum_exp minus
             orc_fast_log(M), and orc_sample_from_scores_overwrite over
             wb[.][q] on the member stream at orc_rng_jump(member_seed_state,
             draw_base + q)
  group      sample_expect.expect_groups' draw of row q on member member[q]:
             the same scores, orc_sample_from_scores_overwrite at
             orc_rng_jump(seed_state, draw_base + q); that member's global id
  cells      dist_group_sample_value (which tests/test_sample_value_host.py
             holds to the float64 laws and to sample_expect.cell_word) on the
             drawn group's statistic words, keyed by (seed_state,
             draw_base + q, f); observed cells as given

Rows that repeat (the law tests draw ONE row 10^5 times) are scored once: the
scores depend on the mask and the observed words alone.

The float64 law (`RowLaw`) of one query row under one mask:
  p(x_unobs | x_obs) = sum_e p(e | x_obs) sum_k p(k | x_obs, e)
                       prod_{f unobserved} p(x_f | k, e)
with p(e | x_obs) proportional to p(x_obs | e) (predict_expect.logp_f64 over
the observed features; under LowEntropy over the member's normalised prior),
p(k | x_obs, e) that call's responsibilities, and p(x_f | k, e)
sample_expect.law_pmf / nich_t on the group's MEMBERS.  The planted laws
change one factor each.
"""
import copy
import ctypes

import numpy as np

import ensemble_expect as ee
import f64_scores as fx
import feature_expect as fe
import feature_many_expect as fm
import oracle_lib as ol
import predict_expect as pe
import sample_expect as sx

DRAW_SEED = ee.DRAW_SEED
MEMBER_SEED = ee.MEMBER_SEED
DRAW_BASE = ee.DRAW_BASE


def query_words(orc, qvals):
    """the query columns as the scorers take them (None stays None)"""
    words = []
    for s, v in zip(orc.shareds, qvals):
        if v is None:
            words.append(None)
            continue
        w = ol.value_words(s.kind, v).copy()
        if s.kind == ol.DPD:
            # dpd.hpp:534-542: a value the table does not hold is OTHER
            w[w >= s.dim] = sx.OTHER
        words.append(w)
    return words


class MemberScores(object):
    """one member's scores of query rows under masks, each distinct (mask,
    observed words) scored once"""

    def __init__(self, orc, qvals, observed):
        self.orc, self.L, self.K, self.F = orc, orc.L, len(orc), orc.F
        self.observed = observed
        self.words = None if qvals is None else query_words(orc, qvals)
        self.prior = np.zeros(self.K, np.float32)
        self.L.orc_mix_driver_score_value(orc.h, self.prior)
        self.p2g = np.array([orc.packed_to_global(k) for k in range(self.K)],
                            np.uint32)
        self._seen = {}

    def at(self, q):
        """-> (scores [K] float32, their orc_log_sum_exp)"""
        ob = 0 if self.observed is None else \
            int(self.observed[q]) & ((1 << self.F) - 1)
        key = (ob,) + tuple(int(self.words[f][q]) for f in range(self.F)
                            if (ob >> f) & 1)
        if key not in self._seen:
            s = self.prior.copy()
            for f in range(self.F):
                if (ob >> f) & 1:
                    self.L.orc_mix_slave_score_value(
                        self.orc.h, f, int(self.words[f][q]), s)
            self._seen[key] = (s, np.float32(self.L.orc_log_sum_exp(self.K,
                                                                    s)))
        return self._seen[key]

    def words_raw(self, qvals, f):
        """the query's words of feature f as GIVEN (an observed DPD value
        outside the table comes back as it was)"""
        return ol.value_words(self.orc.shareds[f].kind, qvals[f])


def expect_many(orcs, gshs, qvals, observed, seed_state, member_seed_state,
                draw_base, le, nq=None, cells=True):
    """orcs: the members' oracle states; gshs: ONE member's engine Shareds
    per member (list of lists) for the cell draws.
    -> dict(wb [M, nq] float32, base [nq], member [nq], group [nq] (the drawn
    member's global id), packed [nq], cols: F arrays of uint32 words or None)
    """
    L = ol.oracle()
    M = len(orcs)
    if observed is not None:
        nq = len(observed)
    F = orcs[0].F
    ms = [MemberScores(o, qvals, observed) for o in orcs]
    totals = np.array([fm.prior_total(o) for o in orcs], np.float32)
    wb = np.zeros((M, nq), np.float32)
    for e in range(M):
        for q in range(nq):
            wb[e, q] = ms[e].at(q)[1]
    if le:
        with np.errstate(invalid="ignore"):
            wb = (wb - totals[:, None]).astype(np.float32)
    base, member, _ = ee.fold(wb, member_seed_state, draw_base)
    packed = np.zeros(nq, np.int64)
    group = np.zeros(nq, np.uint32)
    for q in range(nq):
        m = ms[int(member[q])]
        st = ctypes.c_uint32(L.orc_rng_jump(seed_state, draw_base + q))
        packed[q] = L.orc_sample_from_scores_overwrite(
            ctypes.byref(st), m.K, m.at(q)[0].copy())
        group[q] = m.p2g[packed[q]]
    out = dict(wb=wb, base=base, member=member, group=group, packed=packed,
               prior_totals=totals, cols=None)
    if not cells:
        return out
    cols = []
    for f in range(F):
        col = np.zeros(nq, np.uint32)
        seen = np.zeros(nq, bool)
        if observed is not None:
            seen = ((np.asarray(observed, np.int64) >> f) & 1).astype(bool)
            if seen.any():
                col[seen] = ms[0].words_raw(qvals, f)[seen]
        for e in range(M):
            for k in np.unique(packed[(member == e) & ~seen]):
                rows = np.nonzero((member == e) & (packed == k) & ~seen)[0]
                stats = orcs[e].get_group(f, int(k))
                col[rows] = draw_cells(gshs[e][f], stats, seed_state,
                                       draw_base, rows, f)
        cols.append(col)
    out["cols"] = cols
    return out


def draw_cells(gsh, stats, seed_state, draw_base, rows, f):
    """dist_group_sample_value's words of cells (draw_base + rows, f), rows
    ascending: one call over their span, the rows picked"""
    rows = np.asarray(rows, np.int64)
    out = np.zeros(len(rows), np.uint32)
    if len(rows) == 0:
        return out
    span = int(rows[-1] - rows[0]) + 1
    w = gsh.group_sample_value(stats, seed_state, draw_base + int(rows[0]),
                               span, f)
    return w[rows - rows[0]]


# ---------------------------------------------------------------------------
# members that disagree, made of groups that differ


def shape_rows(config, vals, assign, e):
    """workloads.make's columns are independent of the member and of the
    group, so every member and every group predicts the same cells and no
    histogram could tell who drew them.  Member e's table is shaped instead:
    rows of odd groups (assign % 2 == 1) are of another type than rows of even
    groups, and the types sit elsewhere in every member.
      DD(8)  even: as drawn; odd: {2e, 2e + 1}
      BB     even: as drawn (half ones); odd: ones but for every fourth row
      GP     + 3 in odd groups, + 3e in every group
      NICH   + 2 in odd groups, - 1.5e in every group
    Observing a cell then says something about the member (p(e | x_obs) is far
    from uniform) and about the group's type (the unobserved cells of a row
    depend on each other through the group)."""
    t = (np.asarray(assign) % 2).astype(np.int64)
    rows = np.arange(len(t))
    out = []
    kinds = {"dd_bb_gp": (ol.DD, ol.BB, ol.GP), "gp_nich": (ol.GP, ol.NICH)}
    for kind, v in zip(kinds[config], vals):
        if kind == ol.DD:
            w = np.where(t == 1, v % 2 + 2 * e, v).astype(np.uint32)
        elif kind == ol.BB:
            w = np.where((t == 1) & (rows % 4 != 0), 1, v).astype(np.uint32)
        elif kind == ol.GP:
            w = (v + 3 * t + 3 * e).astype(np.uint32)
        else:
            w = (v + np.float32(2.0) * t.astype(np.float32)
                 - np.float32(1.5 * e)).astype(np.float32)
        out.append(w)
    return out


class ShapedMember(ee.Member):
    """ensemble_expect.Member on shape_rows' table"""

    def __init__(self, config, e, spec, n, le):
        from test_f64_scores import build
        import workloads
        self.__dict__.update(spec)
        self.n, self.le = n, le
        _, _, vals, assign = workloads.make(config, n, self.k,
                                            seed=workloads.SEED + 31 * e)
        vals = shape_rows(config, vals, assign, e)
        self.osh, self.gsh = ee.member_shareds(config, e)
        self.vals, self.assign0 = vals, assign
        self.orc, self.st = build(self.osh, vals, assign, self.k, self.empty,
                                  self.alpha, self.d, self.sweeps, le)
        self.K = len(self.orc)


class ShapedEnsemble(object):
    """an ensemble_expect.Ensemble of ShapedMembers (no query rows of its own:
    the law tests bring theirs)"""

    def __init__(self, config, specs, n=600, le=None):
        self.config, self.le = config, le
        self.members = [ShapedMember(config, e, s, s.get("n", n), le)
                        for e, s in enumerate(specs)]
        self.M = len(self.members)

    def engines(self):
        return [m.engine() for m in self.members]


# ---------------------------------------------------------------------------
# float64


def member_posterior_f64(state, row_vals, ob):
    """one member, one row, one mask -> (log p(x_obs | e), p(k | x_obs, e)
    [K]) in float64; nothing observed: the driver's scores alone"""
    F = len(state.feats)
    drop = {f for f in range(F) if not (ob >> f) & 1}
    if len(drop) == F:
        bare = copy.copy(state)
        bare.feats, bare.cols, bare.stats = [], [], []
        bare.slot = np.zeros(1, np.int64)
        v, _, _ = bare.scores(np.arange(1), remove=False)
        v = v[0]
        m = v.max()
        w = np.exp(v - m)
        return float(np.log(w.sum()) + m), w / w.sum()
    s, keep = fe.without(state, drop)
    Lv, _, p = pe.logp_f64(s, [np.asarray(row_vals[f])[:1] for f in keep])
    return float(Lv[0]), p[0]


class RowLaw(object):
    """the float64 law of ONE query row's unobserved cells under ONE mask, over
    the members' states: r [M] = p(e | x_obs), pk[e] [K_e] = p(k | x_obs, e),
    and per unobserved feature the per-(member, group) cell laws"""

    def __init__(self, members, row_vals, ob, le):
        self.members, self.ob = members, ob
        self.F = len(members[0].osh)
        self.unobs = [f for f in range(self.F) if not (ob >> f) & 1]
        Ls, self.pk = [], []
        for m in members:
            Lv, p = member_posterior_f64(m.st, row_vals, ob)
            if le:
                Lv -= ee.prior_total_f64(m.st)[0]
            Ls.append(Lv)
            self.pk.append(p)
        Ls = np.array(Ls)
        r = np.exp(Ls - Ls.max())
        self.r = r / r.sum()

    def group_members(self, e, f):
        st = self.members[e].st
        col = np.asarray(st.cols[f])
        return [col[st.slot == k] for k in range(len(self.pk[e]))]

    def cell_pmf(self, e, f, values):
        """-> [K_e, len(values) + 1]: p(x_f = v | k, e) for a discrete
        feature, the last column the mass beyond `values`"""
        osh = self.members[e].osh[f]
        feat = fx.Feature(osh)
        out = []
        for mem in self.group_members(e, f):
            xs, pm = sx.law_pmf(osh.kind, feat.kw(), mem)
            row = np.zeros(len(values) + 1)
            index = {int(x): i for i, x in enumerate(xs)}
            for j, v in enumerate(values):
                if int(v) in index:
                    row[j] = pm[index[int(v)]]
            row[-1] = max(0.0, 1.0 - row[:-1].sum())
            out.append(row)
        return np.array(out)

    def cell_cdf_bins(self, e, f, edges):
        """-> [K_e, len(edges) + 1]: the mass of a NICH cell's Student-t law
        in the bins the edges cut the line into"""
        osh = self.members[e].osh[f]
        feat = fx.Feature(osh)
        out = []
        for mem in self.group_members(e, f):
            law = sx.nich_t(feat.kw(), mem.view(np.float32))
            cdf = np.r_[0.0, law.cdf(edges), 1.0]
            out.append(np.diff(cdf))
        return np.array(out)

    def cell_cdf(self, f, t, r=None):
        """the marginal CDF of a NICH cell at t (array)"""
        r = self.r if r is None else r
        t = np.asarray(t, np.float64)
        out = np.zeros_like(t)
        for e, m in enumerate(self.members):
            if r[e] == 0.0:
                continue
            feat = fx.Feature(m.osh[f])
            for k, mem in enumerate(self.group_members(e, f)):
                if self.pk[e][k] < 1e-15:
                    continue
                law = sx.nich_t(feat.kw(), mem.view(np.float32))
                out += r[e] * self.pk[e][k] * law.cdf(t)
        return out

    def joint(self, tables, r=None, independent=False):
        """tables[f][e]: [K_e, n_f] per unobserved feature f (cell_pmf or
        cell_cdf_bins) -> the joint law over the product of the features'
        cells, flattened in feature order (the last feature fastest).
        r: other member weights (a planted law); independent: within the
        drawn member the product of the per-cell marginals (the group redrawn
        per cell)"""
        r = self.r if r is None else np.asarray(r, np.float64)
        fs = self.unobs
        if independent:
            total = 0.0
            for e in range(len(self.members)):
                cell = np.ones(1)
                for f in fs:
                    cell = np.multiply.outer(
                        cell, self.pk[e] @ tables[f][e]).ravel()
                total = total + r[e] * cell
            return total
        total = 0.0
        for e in range(len(self.members)):
            for k, pk in enumerate(self.pk[e]):
                if pk == 0.0 or r[e] == 0.0:
                    continue
                cell = np.ones(1)
                for f in fs:
                    cell = np.multiply.outer(cell, tables[f][e][k]).ravel()
                total = total + r[e] * pk * cell
        return total


def flatten(indices, sizes):
    """per-feature cell indices -> the joint's flattened cell (RowLaw.joint's
    order)"""
    out = np.zeros(len(indices[0]), np.int64)
    for idx, n in zip(indices, sizes):
        out = out * n + np.asarray(idx, np.int64)
    return out
