"""What the held-out readers must return AFTER a hyper-parameter step
(set_shared / set_clustering, sample_hypers / sample_clustering): the cases of
tests/predict_expect.py, tests/feature_expect.py and the members of
tests/ensemble_expect.py, under other hyper-parameters than the ones their
engine was constructed with.

TEST INFRASTRUCTURE (imported by tests only).  No expectation is composed
here: `Switched` exposes what those cases expose (.orc, .st, .qvals, .osh,
.gsh, .K, .engine) for the state after the switch, and the existing functions
of predict_expect, coassign_expect, feature_expect, marginals_expect,
sample_expect and their *_many forms run on it unchanged.

  .orc   a new OracleMixture(alpha', d', shareds') -- LowEntropy where the
         case is -- that adopts the case's oracle: the same groups, members,
         statistics, ids and assignments, other hyper-parameters (the pattern
         of tests/test_gpu_hypers.py's switch-then-sweep test)
  .st    the case's float64 state with the new features' hyper-parameters and
         the new prior.  f64_scores.State's statistics (counts, sums, the NICH
         bounds of the assignments' history) depend on the features' kind and
         dim alone, so they are the case's own: a shallow copy with `feats`
         and `prior` replaced is State(cols, shareds', assign, p2g, prior',
         history) without rebuilding them.
  .qvals the case's held-out rows by the case's own rule under the new values:
         a DPD feature whose beta0 becomes positive has OTHER in rows 1 and 2
  .engine(route)
         the case's engine, then the switch:
         "set"     set_shared per feature, then set_clustering
         "sample"  sample_hypers over a grid of three candidates per feature
                   (`hyper_grid`) and sample_clustering over three pairs
                   (`clustering_grid`); the object is then RE-INSTALLED under
                   the candidates the calls chose (.drawn has the indices), so
                   the expectation follows what the device drew
         Either way the core's own record (core.shared(f), core.clustering())
         must be what was installed: an engine whose Python side took the new
         values without handing them to the core fails here.

`SWITCHES`: the table of cases; each new value crosses a branch of the
kernels (gp_lut arguments below 2.5, NICH nu below 1/16, the small-lgamma
table, DPD's OTHER with d = 0, beta0 from 0 to > 0, LowEntropy, K = 3 without
statistics, K = 1025 at dim 256).
"""
import copy

import numpy as np

import coassign_expect as ce
import coassign_topk_expect as ct
import f64_scores as fx
import oracle_lib as ol
import predict_expect as pe
from test_f64_scores import _le
from test_gpu_hypers import dd, dpd, scalar, shared_equals

OTHER = pe.OTHER
SAMPLE_SEED = 4243          # the engine stream sample_* draw their index from


# -- (oracle Shared, engine SharedParams) pairs: tests/test_gpu_hypers.py's ---

def f32(x):
    return float(np.float32(x))


def bb(alpha, beta):
    return scalar("bb", alpha, beta)


def gp(alpha, inv_beta):
    return scalar("gp", alpha, inv_beta)


def nich(mu, kappa, sigmasq, nu):
    return scalar("nich", mu, kappa, sigmasq, nu)


def bnb(alpha, beta, r):
    return scalar("bnb", alpha, beta, int(r))


def _gp_nich():
    return [gp(0.3, 2.0), nich(-0.5, 2.0, 0.5, 0.03)]


# name (an existing case): new shareds, new (alpha, d) or None
SWITCHES = {
    "gp_nich_swept": (_gp_nich, (2.5, 0.45)),
    "bnb_swept": (lambda: [bnb(0.6, 2.0, 5)], (2.5, 0.45)),
    "bb_swept": (lambda: [bb(4.0, 0.25)], (2.5, 0.45)),
    "dd_bb_gp_swept": (lambda: [dd([2.0, 0.1, 0.1, 5.0, 1.0, 1.0, 0.3, 0.7]),
                                bb(3.0, 3.0), gp(9.0, 0.1)], (2.5, 0.45)),
    "dpd_other_swept": (lambda: [dpd(4.0, np.linspace(1, 3, 50) / 100.0 * 0.6,
                                     0.4)], (0.3, 0.0)),
    "dpd_swept": (lambda: [dpd(4.0, np.linspace(1, 3, 100) / 200.0 * 0.9,
                               0.1)], (2.5, 0.45)),
    "le_gp_nich": (lambda: [gp(6.0, 0.5), nich(0.5, 0.2, 3.0, 4.0)], None),
    "only_empty_k3": (_gp_nich, (2.5, 0.0)),
    "dd256_k1025": (lambda: [dd([0.05 + 0.01 * i for i in range(256)])],
                    (2.5, 0.45)),
}
# the rows that also go by route "sample"
SAMPLED = ["gp_nich_swept", "dd_bb_gp_swept", "dpd_swept"]


def hyper_grid(pair):
    """three candidates for sample_hypers: the table's new value and two more
    of its kind (a DPD's beta0 stays as it is: held-out rows carry OTHER)"""
    o = pair[0]
    p = [float(x) for x in o.p]
    if o.kind == ol.DD:
        a = np.array([o.alphas[i] for i in range(o.dim)], np.float64)
        return [pair, dd(a * 1.5 + 0.25), dd(a[::-1] * 0.5 + 0.125)]
    if o.kind == ol.BB:
        return [pair, bb(p[0] * 2, p[1] + 1), bb(p[0] * 0.25, p[1] * 0.5)]
    if o.kind == ol.GP:
        return [pair, gp(p[0] + 1, p[1] * 2), gp(p[0] * 0.5, p[1] * 0.5)]
    if o.kind == ol.NICH:
        return [pair, nich(p[0] + 1, p[1] * 2, p[2] * 2, p[3] + 1),
                nich(p[0] - 0.25, p[1] * 0.5, p[2] + 1, p[3] * 0.5)]
    if o.kind == ol.BNB:
        return [pair, bnb(p[0] + 1, p[1] + 1, p[2] + 1),
                bnb(p[0] * 0.5, p[1] * 0.5, max(1, int(p[2]) - 2))]
    betas = np.array([o.betas[i] for i in range(o.dim)], np.float32)
    return [pair, dpd(p[0] * 2, betas, p[1]), dpd(p[0] * 0.25, betas[::-1],
                                                   p[1])]


def clustering_grid(alpha, d):
    """three (alpha, d) pairs for sample_clustering, the table's first"""
    return [(alpha, d), (alpha * 2, d * 0.5), (alpha * 0.5, d * 0.5 + 0.25)]


def install(gpu, gsh, clustering):
    """route "set" on an engine: set_shared per feature, then set_clustering
    """
    for f, shared in enumerate(gsh):
        gpu.set_shared(f, shared)
    if clustering is not None:
        gpu.set_clustering(*clustering)


class Switched(object):
    """a case (predict_expect.Case, feature_expect's, ensemble_expect.Member)
    under the hyper-parameters `shareds` = [(oracle Shared, engine
    SharedParams)] per feature and `clustering` = (alpha, d), None: as it
    was"""

    def __init__(self, case, shareds, clustering=None):
        self.case = case
        self.name = getattr(case, "name", None)
        self.le = case.le
        self.n, self.vals = case.n, case.vals
        self.k, self.empty = case.k, case.empty
        self.nq = getattr(case, "nq", None)
        self.drawn = None
        self._install(list(shareds), clustering)

    def _install(self, pairs, clustering):
        case = self.case
        self.pairs = pairs
        self.clustering = None if clustering is None else (
            f32(clustering[0]), f32(clustering[1]))
        self.osh = [p[0] for p in pairs]
        self.gsh = [p[1] for p in pairs]
        self.alpha, self.d = (f32(case.alpha), f32(case.d)) \
            if clustering is None else self.clustering
        self.orc = self.oracle_under(self.osh, (self.alpha, self.d))
        self.K = len(self.orc)
        st = copy.copy(case.st)
        st.feats = [fx.Feature(s) for s in self.osh]
        st.prior = ("le", self.le) if self.le is not None else (
            "py", self.alpha, self.d)
        self.st = st
        if hasattr(case, "qvals"):
            self.qvals = [q.copy() for q in case.qvals]
            for f, sh in enumerate(self.osh):
                if sh.kind == ol.DPD and sh.p[1] > 0:
                    self.qvals[f][[1, 2]] = OTHER
        self._expect = None
        self._f64 = None
        self._subject = None

    def oracle_under(self, osh, clustering):
        """the case's oracle state adopted by a new oracle with these
        hyper-parameters (the switched ones, or a stale mix of old and new)"""
        orc = ol.OracleMixture(clustering[0], clustering[1], list(osh))
        if self.le is not None:
            _le(orc, self.le)
        orc.adopt(self.case.orc, self.case.vals)
        assert len(orc) == self.case.K
        return orc

    def engine(self, route="set"):
        gpu = self.case.engine()
        if route == "set":
            install(gpu, self.gsh, self.clustering)
        else:
            assert route == "sample", route
            state = ol.oracle().orc_rng_seed(SAMPLE_SEED)
            chosen, drawn = [], []
            for f, pair in enumerate(self.pairs):
                grid = hyper_grid(pair)
                index, state = gpu.sample_hypers(f, [c[1] for c in grid],
                                                 state)
                chosen.append(grid[index])
                drawn.append(index)
            clustering = None
            if self.clustering is not None:
                grid = clustering_grid(*self.clustering)
                index, state = gpu.sample_clustering(
                    np.array([a for a, _ in grid], np.float32),
                    np.array([d for _, d in grid], np.float32), state)
                clustering = grid[index]
                drawn.append(index)
            self._install(chosen, clustering)
            self.drawn = drawn
        self.check_installed(gpu)
        return gpu

    def check_installed(self, gpu):
        """the core's own record is what this object expects under"""
        for f, shared in enumerate(self.gsh):
            shared_equals(gpu.core.shared(f), shared)
            assert gpu.shareds[f] is shared
        if self.le is None:
            assert gpu.core.clustering() == (self.alpha, self.d)
            assert (f32(gpu.alpha), f32(gpu.d)) == (self.alpha, self.d)

    # -- what predict_expect.Case has ----------------------------------------
    def expect(self):
        if self._expect is None:
            self._expect = pe.expect(self.orc, self.qvals,
                                     ol.oracle().orc_rng_seed(pe.DRAW_SEED),
                                     pe.DRAW_BASE)
        return self._expect

    def f64(self):
        if self._f64 is None:
            self._f64 = pe.logp_f64(self.st, self.qvals)
        return self._f64

    def subject(self):
        if self._subject is None:
            self._subject = Subject(self)
        return self._subject


def switched(name):
    """SWITCHES[name] on its case"""
    import feature_expect as fe
    new, clustering = SWITCHES[name]
    return Switched(fe.case(name), new(), clustering)


def stale_variants(sw):
    """name -> an oracle on the same adopted state that kept some of the
    constructor's values: what a reader that missed part of the switch would
    compute.  (A switch that leaves the clustering alone has no
    clustering-stale variant.)"""
    case = sw.case
    old_c = (f32(case.alpha), f32(case.d))
    new_c = (sw.alpha, sw.d)
    out = {"all old": sw.oracle_under(case.osh, old_c)}
    if sw.clustering is not None:
        out["clustering old"] = sw.oracle_under(sw.osh, old_c)
    for f in range(len(sw.osh)):
        osh = list(sw.osh)
        osh[f] = case.osh[f]
        out["feature %d old" % f] = sw.oracle_under(osh, new_c)
    return out


# -- ensembles -------------------------------------------------------------

def switched_ensemble(ens, which, pairs, clustering):
    """ensemble_expect.Ensemble `ens` with member `which` switched: the
    expectation's orcs and states take the switched member in its place"""
    out = copy.copy(ens)
    out.members = list(ens.members)
    out.members[which] = Switched(ens.members[which], pairs, clustering)
    out._expect = {}
    out._f64 = None
    return out


# -- coassign_expect / coassign_topk_expect over a switched source ----------

class Subject(ce.Subject):
    """coassign_expect.Subject over a Switched case (M = 1) or a switched
    ensemble: the same rows, the same expectation and law, another source"""

    def __init__(self, src):
        self.src = src
        self.ensemble = hasattr(src, "members")
        self.name = "switched"
        self.members = src.members if self.ensemble else [src]
        self.M = len(self.members)
        self.qvals = src.qvals
        big = max(m.K for m in self.members) > 256
        self.rq = np.arange(40 if big else 70)
        self.rt = np.arange(100, 125 if big else 145)
        self._r = None
        self._expect = {}
        self._law = {}

    def scores(self):
        if self.ensemble:
            return [p["scores"] for p in self.src.expect()["per_member"]]
        return [self.src.expect()["scores"]]

    def logp(self):
        if self.ensemble:
            return [p["logp"] for p in self.src.expect()["per_member"]]
        return [self.src.expect()["logp"]]


class TopkCase(ct.Case):
    """coassign_topk_expect.Case over a Subject of this module"""

    def __init__(self, sub):
        self.sub = sub
        self.rq = sub.rq[sub.specified(sub.rq)]
        self.rt = sub.rt[sub.specified(sub.rt)]
        self._ok_q = np.flatnonzero(sub.specified(sub.rq))
        self._ok_t = np.flatnonzero(sub.specified(sub.rt))
