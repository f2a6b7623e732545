"""The engine's hyper-parameter step (dist_gibbs_score_data, _score_data_grid,
_score_counts_grid, _set_shared, _set_clustering, _sample_hypers,
_sample_clustering, _hyper_stats) against the oracle.

The oracle mirrors the engine's state through orc_mix_load_state
(OracleMixture.adopt).  DirichletDiscrete and the scalar kinds: bit for bit;
DirichletProcessDiscrete: 1e-5 relative, the tolerance Slave::score_data_grid
documents (binary64 sums, the reference's iteration order is undefined).
score_counts: 1e-6 relative, as tests/test_gpu_lp.py holds
dist_py_score_counts."""
import ctypes

import numpy as np
import pytest

import oracle_lib as ol
import workloads

pytestmark = pytest.mark.gpu

SEED = 777


# -- candidates: (oracle Shared, engine SharedParams) pairs --------------------

def dd(alphas):
    from distributions_amd import engine
    alphas = [float(np.float32(a)) for a in alphas]
    return ol.make_shared(ol.DD, alphas=alphas), engine.dd_shared(alphas)


def scalar(kind, *p):
    from distributions_amd import engine
    p = [float(np.float32(x)) for x in p]
    if kind == "bb":
        return (ol.make_shared(ol.BB, alpha=p[0], beta=p[1]),
                engine.bb_shared(*p))
    if kind == "gp":
        return (ol.make_shared(ol.GP, alpha=p[0], inv_beta=p[1]),
                engine.gp_shared(*p))
    if kind == "bnb":
        return (ol.make_shared(ol.BNB, alpha=p[0], beta=p[1], r=p[2]),
                engine.bnb_shared(*p))
    return (ol.make_shared(ol.NICH, mu=p[0], kappa=p[1], sigmasq=p[2],
                           nu=p[3]), engine.nich_shared(*p))


def dpd(alpha, betas, beta0):
    from distributions_amd import engine
    betas = np.ascontiguousarray(betas, np.float32)
    return (ol.make_shared(ol.DPD, alpha=float(np.float32(alpha)), betas=betas,
                           beta0=float(np.float32(beta0))),
            engine.dpd_shared(float(np.float32(alpha)), betas,
                              float(np.float32(beta0))))


def dd_grids(dim, rng):
    """name -> list of alpha vectors"""
    base = rng.uniform(0.1, 3.0, dim)
    whole = [rng.uniform(0.05, 4.0, dim) for _ in range(5)]
    v = int(rng.integers(0, dim))
    coord = []
    for a in [0.1, 0.3, 0.9, 2.7, 8.1, 24.3]:
        x = base.copy()
        x[v] = a
        coord.append(x)
    w = (v + 1) % dim
    two = []
    for a, b in [(0.2, 0.4), (0.7, 0.4), (1.5, 2.5), (0.2, 2.5)]:
        x = base.copy()
        x[v], x[w] = a, b
        two.append(x)
    back = []
    for a in [0.5, 1.5, 0.5, 3.0, 1.5, 0.5]:
        x = base.copy()
        x[v] = a
        back.append(x)
    # small alphas: the arguments below 2.5 that go through libm's lgammaf
    small = [np.full(dim, a) for a in [0.01, 0.5, 1.0, 2.4]]
    return {"whole": whole, "coordinate": coord, "two": two, "back": back,
            "one": [base], "small": small}


def grids_for(osh, rng):
    """the candidate grids of one feature: name -> [(oracle, engine)]"""
    kind = osh.kind
    if kind == ol.DD:
        return {name: [dd(a) for a in grid]
                for name, grid in dd_grids(osh.dim, rng).items()}
    if kind == ol.BB:
        return {"grid": [scalar("bb", a, b) for a in (0.1, 0.5, 2.0, 7.5)
                         for b in (0.3, 1.0, 4.0)],
                "one": [scalar("bb", 0.5, 2.0)]}
    if kind == ol.GP:
        return {"grid": [scalar("gp", a, b) for a in (0.2, 1.0, 3.5, 12.0)
                         for b in (0.1, 1.0, 2.5)],
                "one": [scalar("gp", 1.0, 1.0)]}
    if kind == ol.BNB:
        return {"grid": [scalar("bnb", a, b, r) for a in (0.4, 1.5, 6.0)
                         for b in (0.25, 0.75, 3.0) for r in (1, 3, 7)],
                "one": [scalar("bnb", 1.5, 0.75, 3)]}
    if kind == ol.NICH:
        return {"grid": [scalar("nich", mu, k, s, nu) for mu in (-1.0, 0.0, 0.5)
                         for k in (0.1, 1.0) for s in (0.5, 2.0)
                         for nu in (0.03, 1.0, 4.0)],
                "one": [scalar("nich", 0.0, 1.0, 1.0, 1.0)]}
    dim = osh.dim
    out = []
    for alpha in (0.1, 0.5, 3.0):
        for beta0 in (0.02, 0.1, 0.3):
            b = rng.dirichlet(np.ones(dim)) * (1.0 - beta0)
            out.append(dpd(alpha, b, beta0))
    return {"grid": out, "one": out[:1]}


def oracle_grid(orc, f, cands):
    L = orc.L
    L.orc_mix_slave_score_data_grid.restype = None
    L.orc_mix_slave_score_data_grid.argtypes = [
        ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ol.Shared),
        ctypes.c_size_t, ol.c_f32p]
    arr = (ol.Shared * len(cands))(*[c[0] for c in cands])
    out = np.zeros(len(cands), np.float32)
    L.orc_mix_slave_score_data_grid(orc.h, f, arr, len(cands), out)
    return out


def assert_scores(kind, got, want, what):
    print(what, "max |diff|", float(np.abs(got - want).max()))
    if kind == ol.DPD:
        assert np.all(np.abs(got - want) <= 1e-5 * (1 + np.abs(want))), (
            what, got, want)
    else:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (
            what, got, want)


# (config, dim, n rows, groups, value_sorted mode: None default, 0 general rows)
ENGINES = [("dd", 16, 4096, 6, None), ("dd", 16, 4096, 6, 0),
           ("dd", 256, 60000, 1100, None), ("dd", 256, 6000, 5, 0),
           ("bb", None, 4096, 8, None), ("gp", None, 4096, 8, 0),
           ("nich", None, 4096, 8, None), ("bnb", None, 4096, 8, None),
           ("dpd_other", None, 4096, 7, None), ("gp_nich", None, 30000, 1100, None),
           ("dd_bb_gp", None, 4096, 9, None)]


def swept(config, dim, n, k, mode, alpha=1.0, d=0.2, sweeps=3, empty=3,
          dataset_size=None):
    """an engine after `sweeps` batched sweeps under churn (groups die and
    are founded), and an oracle that adopted its state"""
    from distributions_amd import engine
    osh, gsh, vals, assign = workloads.make(config, n, k, seed=SEED, dim=dim)
    gpu = engine.Gibbs(alpha, d, gsh, dataset_size=dataset_size)
    if mode is not None:
        gpu.set_option("value_sorted", mode)
    gpu.load_rows(vals, assign, k, empty)
    for s in range(sweeps):
        gpu.sweep(0, n, max(256, n // 4), SEED, draw_base=s * n)
    orc = ol.OracleMixture(alpha, d, osh)
    orc.adopt(gpu, vals)
    return orc, gpu, osh, gsh, vals


def mixture_from_groups(gpu, f, shared):
    from distributions_amd import _core
    mix = _core.SlaveMixture(shared)
    for g in range(len(gpu)):
        mix.append(np.ascontiguousarray(gpu.get_group(f, g), np.uint32))
    mix.init()
    return mix


# -- a. grids -----------------------------------------------------------------

@pytest.mark.parametrize("config,dim,n,k,mode", ENGINES)
def test_score_data_grid_matches_oracle(config, dim, n, k, mode):
    orc, gpu, osh, gsh, vals = swept(config, dim, n, k, mode)
    vs, generic = gpu.path_counts()
    if mode == 0:
        assert vs == 0 and generic > 0
    rng = np.random.default_rng(5)
    L = orc.L
    want_data, got_data = [], gpu.score_data()[0]
    for f, sh in enumerate(osh):
        want_data.append(L.orc_mix_slave_score_data(orc.h, f))
        mix = mixture_from_groups(gpu, f, gsh[f]) if len(gpu) <= 64 else None
        for name, cands in grids_for(sh, rng).items():
            want = oracle_grid(orc, f, cands)
            got = gpu.score_data_grid(f, [c[1] for c in cands])
            what = "%s f%d %s K=%d" % (config, f, name, len(gpu))
            assert got.dtype == np.float32 and got.shape == want.shape
            assert_scores(sh.kind, got, want, what)
            if mix is not None:
                assert_scores(sh.kind, got,
                              mix.score_data_grid([c[1] for c in cands]),
                              what + " against dist_mixture_score_data_grid")
    assert_scores(ol.DPD if config.startswith("dpd") else ol.DD, got_data,
                  np.array(want_data, np.float32), config + " score_data")
    gpu.validate()


def test_score_data_grid_large_k_against_the_mixture():
    """K ~ 1100, DD-256: the engine's chains == the stand-alone mixture's
    one-block-per-candidate kernel on the same groups"""
    orc, gpu, osh, gsh, vals = swept("dd", 256, 60000, 1100, None)
    assert len(gpu) > 1000
    mix = mixture_from_groups(gpu, 0, gsh[0])
    rng = np.random.default_rng(8)
    for name, cands in grids_for(osh[0], rng).items():
        got = gpu.score_data_grid(0, [c[1] for c in cands])
        assert_scores(ol.DD, got, mix.score_data_grid([c[1] for c in cands]),
                      name)


@pytest.mark.parametrize("config", ["dd", "gp_nich", "dpd_other"])
def test_grids_on_an_engine_whose_groups_are_all_empty(config):
    from distributions_amd import engine
    osh, gsh, vals, assign = workloads.make(config, 100, 1, seed=SEED)
    gpu = engine.Gibbs(1.0, 0.2, gsh)
    gpu.load_rows_unassigned(vals, 3)      # rows without a group yet
    orc = ol.OracleMixture(1.0, 0.2, osh)
    orc.init_empty(vals, 3)
    assert len(gpu) == 3 and not gpu.counts().any()
    rng = np.random.default_rng(6)
    for f, sh in enumerate(osh):
        for name, cands in grids_for(sh, rng).items():
            want = oracle_grid(orc, f, cands)
            got = gpu.score_data_grid(f, [c[1] for c in cands])
            assert_scores(sh.kind, got, want, config + " empty " + name)
            assert not got.any()
    data, clustering = gpu.score_data()
    assert not data.any() and clustering == 0.0


# -- b. the clustering model ---------------------------------------------------

PY_GRID = [(0.1, 0.0), (1.0, 0.0), (1.0, 0.2), (3.0, 0.5), (10.0, 0.9),
           (0.01, 0.99), (100.0, 0.1)]


@pytest.mark.parametrize("config,dim,n,k,mode",
                         [ENGINES[0], ENGINES[2], ENGINES[9]])
def test_score_counts_grid_matches_oracle(config, dim, n, k, mode):
    orc, gpu, osh, gsh, vals = swept(config, dim, n, k, mode)
    counts = np.ascontiguousarray(gpu.counts(), np.int32)
    alphas = np.array([a for a, _ in PY_GRID], np.float32)
    ds = np.array([d for _, d in PY_GRID], np.float32)
    got = gpu.score_counts_grid(alphas, ds)
    for c in range(len(PY_GRID)):
        want = orc.L.orc_py_score_counts(float(alphas[c]), float(ds[c]), counts,
                                         counts.size)
        print(config, PY_GRID[c], got[c], want)
        assert abs(got[c] - want) <= 1e-6 * (1 + abs(want)), (c, got[c], want)
    # one launch, equal statistics: the same bits again
    assert np.array_equal(got, gpu.score_counts_grid(alphas, ds))
    want = orc.L.orc_py_score_counts(1.0, float(np.float32(0.2)), counts,
                                     counts.size)
    got = gpu.score_data()[1]
    assert abs(got - want) <= 1e-6 * (1 + abs(want)), (got, want)
    assert len(gpu.score_counts_grid([], [])) == 0


def test_low_entropy_engine_scores_its_own_model_and_has_no_grid():
    N = 5000
    orc, gpu, osh, gsh, vals = swept("dd", 16, 4096, 12, None, dataset_size=N)
    L = orc.L
    L.orc_le_score_counts.restype = ctypes.c_float
    L.orc_le_score_counts.argtypes = [ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_size_t]
    counts = np.ascontiguousarray(gpu.counts(), np.int32)
    want = L.orc_le_score_counts(N, counts.ctypes.data, counts.size)
    data, got = gpu.score_data()
    assert abs(got - want) <= 1e-6 * (1 + abs(want)), (got, want)
    assert data[0] == np.float32(L.orc_mix_slave_score_data(orc.h, 0))
    with pytest.raises(RuntimeError, match="LowEntropy"):
        gpu.score_counts_grid([1.0], [0.1])
    with pytest.raises(RuntimeError, match="LowEntropy"):
        gpu.set_clustering(1.0, 0.1)
    with pytest.raises(RuntimeError, match="LowEntropy"):
        gpu.sample_clustering([1.0], [0.1], 5)
    gpu.sweep(0, 4096, 1024, SEED, draw_base=10 ** 6)   # still usable
    gpu.validate()


# -- c. set_shared / set_clustering -------------------------------------------

def id_maps(x):
    return (np.array([x.core.packed_to_global(k) for k in range(len(x))]),
            int(x.core.global_size()))


def assert_same_engine_state(orc, gpu, what):
    assert len(gpu) == len(orc), what
    np.testing.assert_array_equal(gpu.counts(), orc.counts(), err_msg=what)
    np.testing.assert_array_equal(gpu.assignments(), orc.assign, err_msg=what)
    for f in range(orc.F):
        for g in range(len(orc)):
            np.testing.assert_array_equal(
                gpu.get_group(f, g), orc.get_group(f, g),
                err_msg="%s feature %d group %d" % (what, f, g))
    p2g, size = id_maps(gpu)
    p2g_o, size_o = id_maps(orc)
    np.testing.assert_array_equal(p2g, p2g_o, err_msg=what + " id map")
    assert size == size_o, what
    gpu.validate()


NEW_SHARED = {
    "dd": lambda: [dd([0.05 + 0.3 * i for i in range(16)])],
    "dd_skew": lambda: [dd([3.0] * 16)],
    "bb": lambda: [scalar("bb", 4.0, 0.25)],
    "gp": lambda: [scalar("gp", 6.0, 0.5)],
    "bnb": lambda: [scalar("bnb", 0.6, 2.0, 5)],
    "nich": lambda: [scalar("nich", 0.5, 0.2, 3.0, 0.03)],
    "gp_nich": lambda: [scalar("gp", 0.3, 2.0),
                        scalar("nich", -0.5, 2.0, 0.5, 4.0)],
    "dpd_other": lambda: [dpd(4.0, np.linspace(1, 3, 50) / 100.0 * 0.6, 0.4)],
    "dd_bb_gp": lambda: [dd([2.0, 0.1, 0.1, 5.0, 1.0, 1.0, 0.3, 0.7]),
                         scalar("bb", 3.0, 3.0), scalar("gp", 9.0, 0.1)],
}


@pytest.mark.parametrize("config", sorted(NEW_SHARED))
@pytest.mark.parametrize("mode", [None, 0])
def test_switch_then_sweep_equals_an_oracle_created_with_the_new_values(
        config, mode):
    n, k = 4096, 24
    _, gpu, osh, gsh, vals = swept(config, None, n, k, mode, sweeps=2)
    new = NEW_SHARED[config]()
    for f, (_, shared) in enumerate(new):
        gpu.set_shared(f, shared)
    gpu.set_clustering(2.5, 0.45)
    assert (gpu.alpha, gpu.d) == (2.5, float(np.float32(0.45)))
    orc = ol.OracleMixture(2.5, 0.45, [c[0] for c in new])
    orc.adopt(gpu, vals)            # the state at the switch
    st = ol.oracle().orc_rng_seed(SEED + 1)
    for s in range(2):
        base = (5 + s) * n
        for b in range(0, n, 1024):
            orc.gibbs_batch(b, b + 1024, st, base)
        gpu.sweep(0, n, 1024, SEED + 1, draw_base=base)
        assert_same_engine_state(orc, gpu, "%s batched %d" % (config, s))
    rng_g = gpu.sweep_sequential(0, 1500, 4711)
    rng_o = orc.gibbs_sequential(0, 1500, 4711)
    assert rng_g == rng_o
    assert_same_engine_state(orc, gpu, config + " sequential")
    # ... and back again, between a sequential and a batched pass
    for f, shared in enumerate(gsh):
        gpu.set_shared(f, shared)
    gpu.set_clustering(1.0, 0.2)
    orc = ol.OracleMixture(1.0, 0.2, osh)
    orc.adopt(gpu, vals)
    for b in range(0, n, 1024):
        orc.gibbs_batch(b, b + 1024, st, 9 * n)
    gpu.sweep(0, n, 1024, SEED + 1, draw_base=9 * n)
    assert_same_engine_state(orc, gpu, config + " back")


@pytest.mark.parametrize("config,normalise", [("dd", 2), ("dd", 0),
                                              ("dd_skew", 2), ("gp_nich", 2)])
def test_installing_the_values_in_force_changes_nothing(config, normalise):
    """with a device-normalised run open (normalise = 2, one integer feature)
    and with the value-sorted cache's assignments not yet written back"""
    from distributions_amd import engine
    n, k = 8192, 16
    osh, gsh, vals, assign = workloads.make(config, n, k, seed=SEED)
    pair = []
    for _ in range(2):
        g = engine.Gibbs(1.0, 0.2, gsh)
        g.set_option("device_normalise", normalise)
        if config.startswith("dd"):
            g.set_option("value_sorted", 2)    # (auto leaves so few rows alone)
        g.load_rows(vals, assign, k, 2)
        pair.append(g)
    a, b = pair
    for s in range(4):
        for g in pair:
            g.sweep(0, n, 2048, SEED, draw_base=s * n)
        for f, shared in enumerate(gsh):       # a alone; nothing else is asked
            a.set_shared(f, shared)            # of it in between
        a.set_clustering(1.0, 0.2)
    if config.startswith("dd"):
        assert a.path_counts()[0] > 0
        runs = b.core.debug_counts()["device_normalised"]
        print(config, normalise, "device-normalised batches", runs)
        assert (runs > 0) == (normalise == 2)
    np.testing.assert_array_equal(a.assignments(), b.assignments())
    np.testing.assert_array_equal(a.counts(), b.counts())
    for f in range(len(gsh)):
        for g in range(len(a)):
            np.testing.assert_array_equal(a.get_group(f, g), b.get_group(f, g))
    assert id_maps(a)[1] == id_maps(b)[1]
    np.testing.assert_array_equal(id_maps(a)[0], id_maps(b)[0])
    a.validate()


def test_a_refused_candidate_leaves_the_engine_usable():
    orc, gpu, osh, gsh, vals = swept("dd_bb_gp", None, 4096, 9, None, sweeps=1)
    with pytest.raises(RuntimeError, match="model mismatch"):
        gpu.set_shared(0, scalar("bb", 1.0, 1.0)[1])
    with pytest.raises(RuntimeError, match="dim mismatch"):
        gpu.set_shared(0, dd([1.0] * 9)[1])
    with pytest.raises(RuntimeError, match="bad feature"):
        gpu.set_shared(3, dd([1.0] * 8)[1])
    with pytest.raises(RuntimeError, match="alpha > 0"):
        gpu.set_clustering(0.0, 0.5)
    with pytest.raises(RuntimeError, match="alpha > 0"):
        gpu.set_clustering(1.0, 1.0)
    with pytest.raises(RuntimeError, match="mismatch"):
        gpu.score_data_grid(1, [dd([1.0] * 8)[1]])
    with pytest.raises(RuntimeError, match="mismatch"):
        gpu.sample_hypers(0, [dd([1.0] * 8)[1], dd([1.0] * 7)[1]], 9)
    # nothing was installed: the oracle under the ORIGINAL values follows
    assert gpu.core.shared(0).alphas == [0.5] * 8
    assert gpu.core.clustering() == (1.0, float(np.float32(0.2)))
    st = ol.oracle().orc_rng_seed(3)
    for b in range(0, 4096, 1024):
        orc.gibbs_batch(b, b + 1024, st, 10 ** 6)
    gpu.sweep(0, 4096, 1024, 3, draw_base=10 ** 6)
    assert_same_engine_state(orc, gpu, "after refused candidates")


def test_set_shared_on_one_engine_of_a_sweep_sequential_many_set():
    from distributions_amd import engine
    n, k, m = 600, 5, 3
    engines, oracles = [], []
    for i in range(m):
        osh, gsh, vals, assign = workloads.make("gp_nich", n, k, seed=SEED + i)
        g = engine.Gibbs(1.0, 0.2, gsh)
        g.load_rows(vals, assign, k, 1)
        engines.append(g)
        oracles.append((osh, vals))
    states = np.array([11, 22, 33], np.uint32)
    states = engine.sweep_sequential_many(engines, 0, n, states)
    new = NEW_SHARED["gp_nich"]()
    for f, (_, shared) in enumerate(new):
        engines[1].set_shared(f, shared)
    engines[1].set_clustering(0.3, 0.7)
    orcs = []
    for i, (osh, vals) in enumerate(oracles):
        o = (ol.OracleMixture(0.3, 0.7, [c[0] for c in new]) if i == 1
             else ol.OracleMixture(1.0, 0.2, osh))
        o.adopt(engines[i], vals)
        orcs.append(o)
    after = engine.sweep_sequential_many(engines, 0, n, states)
    for i in range(m):
        assert orcs[i].gibbs_sequential(0, n, int(states[i])) == int(after[i])
        assert_same_engine_state(orcs[i], engines[i], "chain %d" % i)


# -- d. sample_* -----------------------------------------------------------------

def shared_equals(got, want):
    assert got.kind == want.kind and got.dim == want.dim
    assert got.p == want.p
    if got.kind == ol.DD:
        assert got.alphas == want.alphas
    if got.kind == ol.DPD:
        np.testing.assert_array_equal(got.betas, want.betas)


@pytest.mark.parametrize("config,dim,n,k,mode",
                         [ENGINES[0], ENGINES[3], ENGINES[4], ENGINES[6],
                          ENGINES[8], ENGINES[9]])
def test_sample_hypers_draws_the_oracles_index(config, dim, n, k, mode):
    orc, gpu, osh, gsh, vals = swept(config, dim, n, k, mode, sweeps=2)
    L = orc.L
    rng = np.random.default_rng(17)
    state = L.orc_rng_seed(99)
    seen = set()
    for f, sh in enumerate(osh):
        for name, cands in grids_for(sh, rng).items():
            for _ in range(4):
                scores = oracle_grid(orc, f, cands)
                st = ctypes.c_uint32(state)
                want = L.orc_sample_from_scores_overwrite(
                    ctypes.byref(st), len(cands), scores)
                index, new_state = gpu.sample_hypers(
                    f, [c[1] for c in cands], state)
                assert (index, new_state) == (want, st.value), (config, name)
                state = new_state
                seen.add((name, index))
                shared_equals(gpu.core.shared(f), cands[index][1])
                assert gpu.shareds[f] is cands[index][1]
        # the engine now runs under the last choice: restore for the oracle
        gpu.set_shared(f, gsh[f])
    print(config, "drawn", sorted(seen))
    # a sweep under what was installed last equals the oracle's
    st = L.orc_rng_seed(5)
    for b in range(0, n, 1024):
        orc.gibbs_batch(b, min(n, b + 1024), st, 10 ** 7)
    gpu.sweep(0, n, 1024, 5, draw_base=10 ** 7)
    np.testing.assert_array_equal(gpu.assignments(), orc.assign)


def test_sample_clustering_draws_the_oracles_index():
    orc, gpu, osh, gsh, vals = swept("dd", 16, 4096, 6, None)
    L = orc.L
    counts = np.ascontiguousarray(gpu.counts(), np.int32)
    alphas = np.array([a for a, _ in PY_GRID[:5]], np.float32)
    ds = np.array([d for _, d in PY_GRID[:5]], np.float32)
    scores = np.array([L.orc_py_score_counts(float(a), float(d), counts,
                                             counts.size)
                       for a, d in zip(alphas, ds)], np.float32)
    got_scores = gpu.score_counts_grid(alphas, ds)
    state = L.orc_rng_seed(31)
    picks = set()
    for _ in range(12):
        # (the draw is held to the oracle's on the ENGINE's scores where the
        # two differ in the last place, which 1e-6 allows)
        st = ctypes.c_uint32(state)
        want = L.orc_sample_from_scores_overwrite(ctypes.byref(st), 5,
                                                  got_scores.copy())
        st2 = ctypes.c_uint32(state)
        want_o = L.orc_sample_from_scores_overwrite(ctypes.byref(st2), 5,
                                                    scores.copy())
        index, new_state = gpu.sample_clustering(alphas, ds, state)
        assert (index, new_state) == (want, st.value)
        assert index == want_o and new_state == st2.value
        assert gpu.core.clustering() == (float(alphas[index]),
                                         float(ds[index]))
        assert (gpu.alpha, gpu.d) == gpu.core.clustering()
        picks.add(index)
        state = new_state
    print("drawn", sorted(picks))


# -- e. work follows what changed ------------------------------------------------

@pytest.mark.parametrize("dim", [16, 256])
def test_chains_follow_what_changed(dim):
    orc, gpu, osh, gsh, vals = swept("dd", dim, 6000, 12, None, sweeps=1)
    rng = np.random.default_rng(4)
    grids = dd_grids(dim, rng)
    for name in ["coordinate", "two", "back", "one"]:
        grid = grids[name]
        changed = sum(int((np.float32(grid[c]) != np.float32(grid[c - 1])).sum())
                      for c in range(1, len(grid)))
        before = gpu.hyper_stats()
        gpu.score_data_grid(0, [dd(a)[1] for a in grid])
        after = gpu.hyper_stats()
        chains = after[0] - before[0]
        print(name, "chains", chains, "bound", dim + 1 + 2 * changed)
        assert 0 < chains <= (dim + 1) + 2 * changed, (name, chains, changed)
        assert after[1] - before[1] == len(grid)
        assert after[2] - before[2] == 2 and after[3] - before[3] == 1
    # a coordinate returning to an earlier value costs nothing new
    before = gpu.hyper_stats()[0]
    gpu.score_data_grid(0, [dd(a)[1] for a in grids["back"]])
    assert gpu.hyper_stats()[0] - before == (dim + 1) + 2 * 2
    # ... and sample_hypers is the same grid, one launch more
    before = gpu.hyper_stats()
    gpu.sample_hypers(0, [dd(a)[1] for a in grids["coordinate"]], 7)
    after = gpu.hyper_stats()
    assert after[0] - before[0] == (dim + 1) + 2 * 5
    assert after[2] - before[2] == 3
