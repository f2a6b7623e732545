"""The joint law of (partition, hyper-parameter index) in float64, and the
exact law of the chain that alternates one sequential sweep with one draw of
the hyper-parameters from a grid.

TEST INFRASTRUCTURE (imported by tests only); builds on tests/f64_posterior.py.

At 6 rows and a grid of H candidates the state is (h, partition): H * 203
states.  Under a uniform prior on the grid the joint posterior is

    pi(h, p)  proportional to  exp(log_posterior_h(p))

with log_posterior_h the closed form of f64_posterior.Model under candidate h
(EPPF of PitmanYor plus the blocks' log marginal likelihoods: both complete,
hyper-parameter dependent normalisers included).  One transition is

    a sweep under h (f64_posterior's sweep_matrix of model h), then
    h' drawn with probability pi(h' | p'):  what score_data_grid /
    score_counts followed by sample_from_scores does,

so T[(h, p), (h', p')] = P_h[p, p'] * pi(h' | p'), and pi is T's stationary
vector: the sweep leaves pi(. | h) invariant, the draw leaves pi(. | p')
invariant.  `transition(mutant=True)` is the chain that draws h but keeps
sweeping under the hyper-parameters it was created with (caches never
rebuilt): P_0 in place of P_h.

Configurations: DirichletDiscrete with a 4-point grid of alpha vectors (a
feature's Shared is drawn), GammaPoisson + NormalInverseChiSq with a 4-point
grid of PitmanYor (alpha, d) (the clustering model is drawn).  Nothing here
reads the library; `oracle_histogram` drives the oracle alone."""
import ctypes

import numpy as np

import f64_posterior as fp

EMPTY = 3

# name -> (configuration of f64_posterior, "shared" | "py", the grid)
CONFIGS = {
    "dd": ("dd", "shared", [
        dict(alphas=[0.5, 1.0, 2.0]),
        dict(alphas=[0.125, 0.125, 0.125]),
        dict(alphas=[4.0, 4.0, 4.0]),
        dict(alphas=[3.0, 0.25, 0.75]),
    ]),
    # (a grid whose points are near enough for the chain to move between
    # them: with d = 0.8 among the candidates the joint chain needs 47
    # transitions to mix to 1e-4, with these 19)
    "gp_nich": ("gp_nich", "py", [(1.2, 0.3), (0.3, 0.1), (4.0, 0.2),
                                  (1.0, 0.6)]),
}


def candidates(name):
    """-> per grid point (oracle shareds, (alpha, d))"""
    import oracle_lib as ol
    config, what, grid = CONFIGS[name]
    base = fp.shared_kw(config)
    out = []
    for point in grid:
        if what == "shared":
            kinds = [(base[0][0], point)] + base[1:]
            prior = fp.PY[1:]
        else:
            kinds = base
            prior = point
        out.append(([ol.make_shared(k, **kw) for k, kw in kinds],
                    (float(prior[0]), float(prior[1]))))
    return out


class Joint(object):
    def __init__(self, name):
        config = CONFIGS[name][0]
        self.name = name
        self.models = [fp.Model(shareds, fp.ROWS[config],
                                ("py", prior[0], prior[1]), EMPTY)
                       for shareds, prior in candidates(name)]
        self.H = len(self.models)
        self.space = self.models[0].space
        self.S = len(self.space.parts)
        lp = np.stack([m.log_posterior() for m in self.models])   # [H, S]
        w = np.exp(lp - lp.max())
        self.joint = (w / w.sum()).reshape(-1)                   # h * S + p
        self.cond = w / w.sum(0, keepdims=True)                   # pi(h | p)
        self._sweeps = None

    def sweeps(self):
        if self._sweeps is None:
            self._sweeps = [m.sweep_matrix() for m in self.models]
        return self._sweeps

    def transition(self, mutant=False):
        H, S = self.H, self.S
        P = self.sweeps()
        T = np.zeros((H * S, H * S))
        for h in range(H):
            Ph = P[0] if mutant else P[h]
            for h2 in range(H):
                T[h * S:(h + 1) * S, h2 * S:(h2 + 1) * S] = (
                    Ph * self.cond[h2][None, :])
        return T

    def start(self):
        """all rows in one group, under grid point 0"""
        e = np.zeros(self.H * self.S)
        e[self.space.index[(0,) * self.space.n]] = 1.0
        return e

    def histogram(self, h, assign):
        """[M] grid indices, [M, n] group ids -> counts over the H * S states"""
        idx = np.asarray(h, np.int64) * self.S + self.space.indices(assign)
        return np.bincount(idx, minlength=self.H * self.S)


# the sample the device test takes (tests/test_gpu_hyper_posterior.py):
# CHAINS engines, SAMPLES states each, a mixing time apart.  20 480 states keep
# the pooled mass of both configurations under 5 %;
# tests/test_f64_hyper_posterior.py shows that the stale-cache mutant is
# rejected at this count.
CHAINS = 512
SAMPLES = 40

_JOINTS = {}


def joint(name):
    if name not in _JOINTS:
        _JOINTS[name] = Joint(name)
    return _JOINTS[name]


def values(name):
    config = CONFIGS[name][0]
    return [np.asarray(c, np.float32 if k == fp.NICH else np.uint32)
            for (k, _), c in zip(fp.shared_kw(config), fp.ROWS[config])]


# ---------------------------------------------------------------------------
# runner: independent oracle chains, one oracle mixture per grid point; the
# state moves between them through orc_mix_load_state


def oracle_histogram(name, chains, T, samples, base):
    """`chains` chains from Joint.start(), chain c seeded orc_rng_seed(base +
    c); per transition one sequential sweep and one grid draw, both from the
    chain's one engine state; a state is recorded every T transitions,
    `samples` per chain -> histogram over the H * S states"""
    import oracle_lib as ol
    what = CONFIGS[name][1]
    cands = candidates(name)
    H = len(cands)
    vals = values(name)
    n = len(vals[0])
    orcs = [ol.OracleMixture(prior[0], prior[1], shareds)
            for shareds, prior in cands]
    L = orcs[0].L
    L.orc_mix_slave_score_data_grid.restype = None
    L.orc_mix_slave_score_data_grid.argtypes = [
        ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ol.Shared),
        ctypes.c_size_t, ol.c_f32p]
    grid = (ol.Shared * H)(*[shareds[0] for shareds, _ in cands])
    assign0 = np.zeros(n, np.uint32)
    for o in orcs:
        o.init_from_assignments(vals, assign0, 1, EMPTY)
    F = len(cands[0][0])
    out_h = np.zeros(chains * samples, np.int64)
    out_a = np.zeros((chains * samples, n), np.uint32)
    scores = np.zeros(H, np.float32)
    st = ctypes.c_uint32(0)
    ref = ctypes.byref(st)
    at = 0
    for c in range(chains):
        h = 0
        o = orcs[0]
        a = np.zeros(n, np.uint32)
        L.orc_mix_init_from_assignments(o.h, n, o._vals, assign0, 1, EMPTY, a)
        st.value = L.orc_rng_seed(base + c)
        for step in range(T * samples):
            L.orc_mix_gibbs_sequential(o.h, 0, n, o._vals, a, ref)
            if what == "shared":
                L.orc_mix_slave_score_data_grid(o.h, 0, grid, H, scores)
            else:
                counts = o.counts()
                for j, (_, prior) in enumerate(cands):
                    scores[j] = L.orc_py_score_counts(prior[0], prior[1],
                                                      counts, counts.size)
            h2 = int(L.orc_sample_from_scores_overwrite(ref, H, scores))
            if h2 != h:
                K = len(o)
                blocks = [np.ascontiguousarray(np.concatenate(
                    [o.get_group(f, g) for g in range(K)]).astype(np.uint32))
                    for f in range(F)]
                p2g = np.array([o.packed_to_global(k) for k in range(K)],
                               np.uint32)
                L.orc_mix_load_state(orcs[h2].h, K, o.counts(),
                                     ol.ptr_array(blocks), p2g,
                                     int(o.global_size()))
                h, o = h2, orcs[h2]
            if (step + 1) % T == 0:
                out_h[at] = h
                out_a[at] = a
                at += 1
    return joint(name).histogram(out_h, out_a)
