"""A whole DirichletDiscrete coordinate pass in one call
(dist_gibbs_sample_hypers_pass, _pass_many) against the loop of
dist_gibbs_sample_hypers calls that defines it, and against the oracle.

Everything is bit for bit: the chosen indices, the advanced rng state, the
Shared in force afterwards and what the engine then computes under it.  A
"twin" is a second engine built by the same swept(...) call and taken through
the explicit loop.  dist_gibbs_hyper_stats tells which path ran: the device
pass is LAUNCHES launches whatever the shape, the loop 3 per step.

The small shapes' grids lie in [0.9, 4]; their smallest value is 1.5 at dim 2
and 1.0 at dim 3, because the device runs the pass only where dim times the
smallest value a coordinate can hold is 3 or more (every reachable alpha_sum
then stays on fast_lgamma's polynomial)."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib as ol
import workloads
from test_gpu_hypers import (SEED, assert_same_engine_state, dd, oracle_grid,
                             swept)

pytestmark = pytest.mark.gpu

LAUNCHES = 2      # of a device pass, stated in include/distributions_hip.h
STATE = 20250117


def f32(x):
    return np.ascontiguousarray(x, np.float32)


def loop(gpu, f, grids, state, coords=None):
    """the definition: sample_hypers per step over a coordinate grid"""
    from distributions_amd import engine
    alphas = list(gpu.core.shared(f).alphas)
    grids = f32(grids)
    coords = range(len(alphas)) if coords is None else coords
    chosen = []
    for i, v in enumerate(coords):
        row = grids[i] if grids.ndim == 2 else grids
        cands = []
        for a in row:
            x = list(alphas)
            x[v] = float(a)
            cands.append(engine.dd_shared(x))
        index, state = gpu.sample_hypers(f, cands, state)
        chosen.append(index)
        alphas[v] = float(row[index])
    return np.array(chosen, np.uint32), state, alphas


def oracle_pass(orc, f, alphas, grids, state, coords=None):
    """oracle_grid, then orc_sample_from_scores_overwrite, per step"""
    alphas = [float(np.float32(a)) for a in alphas]
    grids = f32(grids)
    coords = range(len(alphas)) if coords is None else coords
    chosen = []
    for i, v in enumerate(coords):
        row = grids[i] if grids.ndim == 2 else grids
        cands = []
        for a in row:
            x = list(alphas)
            x[v] = float(a)
            cands.append(dd(x))
        scores = oracle_grid(orc, f, cands)
        st = ctypes.c_uint32(state)
        index = orc.L.orc_sample_from_scores_overwrite(
            ctypes.byref(st), len(cands), scores)
        state = st.value
        chosen.append(index)
        alphas[v] = float(row[index])
    return np.array(chosen, np.uint32), state, alphas


def delta(gpu, before):
    return tuple(int(a) - int(b) for a, b in zip(gpu.hyper_stats(), before))


def assert_device_pass(gpu, before, n_coords, G):
    chains, cands, launches, calls = delta(gpu, before)
    assert calls == 1 and launches == LAUNCHES, (launches, calls)
    assert cands == n_coords * G
    assert chains >= n_coords * G


def assert_loop(gpu, before, n_coords):
    chains, cands, launches, calls = delta(gpu, before)
    assert launches == 3 * n_coords and calls == n_coords, (launches, calls)


@functools.lru_cache(maxsize=None)
def small(dim):
    """4096 rows, 6 to 12 groups after the churn, 3 of them empty at first"""
    orc, gpu, osh, gsh, vals = swept("dd", dim, 4096, 4, None, sweeps=1,
                                     empty=3)
    print("dim", dim, "groups", len(gpu))
    assert 6 <= len(gpu) <= 12
    return orc, gpu, vals


def small_grid(dim, G):
    """in [0.9, 4]; 1.5 is the value in force, 2.25 comes twice"""
    lo = max(0.9, 3.0 / dim)
    return f32({1: [2.0], 2: [2.25, 2.0],
                7: [lo, 1.5, 2.25, 4.0, 2.25, 3.125, 1.75]}[G])


# -- 1. against the oracle, small shapes ---------------------------------------

@pytest.mark.parametrize("G", [1, 2, 7])
@pytest.mark.parametrize("dim", [2, 3, 5, 16])
def test_small_passes_draw_the_oracles_sequence(dim, G):
    orc, gpu, vals = small(dim)
    gpu.set_shared(0, dd([1.5] * dim)[1])
    grid = small_grid(dim, G)
    want, want_state, want_alphas = oracle_pass(orc, 0, [1.5] * dim, grid,
                                                STATE + dim)
    before = gpu.hyper_stats()
    got, state = gpu.sample_hypers_pass(0, grid, STATE + dim)
    print(dim, G, "drawn", got.tolist())
    assert_device_pass(gpu, before, dim, G)
    assert got.dtype == np.uint32 and got.tolist() == want.tolist()
    assert state == want_state
    assert gpu.core.shared(0).alphas == want_alphas
    assert gpu.shareds[0].alphas == want_alphas
    # no coordinate at all: nothing changes
    got, same = gpu.sample_hypers_pass(0, grid, state, coords=[])
    assert len(got) == 0 and same == state
    assert gpu.core.shared(0).alphas == want_alphas


# -- 2. order and repeats ------------------------------------------------------

def test_coordinates_in_any_order_see_their_earlier_draws():
    coords = [5, 5, 0, 15, 5, 3]
    rng = np.random.default_rng(2)
    grids = f32(rng.uniform(0.9, 4.0, (len(coords), 5)))
    grids[1, 2] = grids[0, 0]           # (a value the first visit may draw)
    _, gpu, _ = small(16)
    _, twin, _, _, _ = swept("dd", 16, 4096, 4, None, sweeps=1, empty=3)
    for g in (gpu, twin):
        g.set_shared(0, dd([1.5] * 16)[1])
    want, want_state, want_alphas = loop(twin, 0, grids, STATE, coords)
    before = gpu.hyper_stats()
    got, state = gpu.sample_hypers_pass(0, grids, STATE, coords=coords)
    assert_device_pass(gpu, before, len(coords), 5)
    assert got.tolist() == want.tolist() and state == want_state
    assert gpu.core.shared(0).alphas == want_alphas
    assert gpu.core.shared(0).alphas == twin.core.shared(0).alphas
    # the third visit of coordinate 5 decides what stays
    assert want_alphas[5] == float(grids[4, want[4]])


# -- 3. DD-256 at the benchmark's group count -----------------------------------

def test_dd256_pass_equals_the_loop_and_installs_everything():
    n = 60000
    _, gpu, _, _, vals = swept("dd", 256, n, 1100, None)
    _, twin, _, _, _ = swept("dd", 256, n, 1100, None)
    assert len(gpu) > 1000
    grid = f32(np.geomspace(0.05, 5, 32))
    want, want_state, want_alphas = loop(twin, 0, grid, STATE)
    before = gpu.hyper_stats()
    got, state = gpu.sample_hypers_pass(0, grid, STATE)
    assert_device_pass(gpu, before, 256, 32)
    print("drawn", sorted(set(got.tolist())))
    assert got.tolist() == want.tolist() and state == want_state
    assert gpu.core.shared(0).alphas == want_alphas
    # the install is complete: what follows is the same on both
    for g in (gpu, twin):
        g.sweep(0, n, n // 4, SEED + 3, draw_base=10 ** 7)
    np.testing.assert_array_equal(gpu.assignments(), twin.assignments())
    np.testing.assert_array_equal(gpu.counts(), twin.counts())
    held_out = [np.random.default_rng(9).integers(0, 256, 64)
                .astype(np.uint32)]
    a, b = gpu.predict(held_out, seed=4), twin.predict(held_out, seed=4)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    np.testing.assert_array_equal(a[1], b[1])
    gpu.validate()


# -- 4. the loop cases ---------------------------------------------------------

def test_a_reachable_alpha_sum_below_the_polynomial_takes_the_loop():
    """glibc's lgammaf values decide: against the oracle as well"""
    dim = 4
    orc, gpu, osh, gsh, vals = swept("dd", dim, 4096, 8, None, empty=3)
    _, twin, _, _, _ = swept("dd", dim, 4096, 8, None, empty=3)
    for g in (gpu, twin):
        g.set_shared(0, dd([0.1] * dim)[1])
    grid = f32([0.05, 0.1, 0.4, 0.4, 1.2, 0.075])
    want_o, state_o, alphas_o = oracle_pass(orc, 0, [0.1] * dim, grid, STATE)
    want, want_state, want_alphas = loop(twin, 0, grid, STATE)
    before = gpu.hyper_stats()
    got, state = gpu.sample_hypers_pass(0, grid, STATE)
    assert_loop(gpu, before, dim)
    assert got.tolist() == want.tolist() == want_o.tolist()
    assert state == want_state == state_o
    assert gpu.core.shared(0).alphas == want_alphas == alphas_o


def test_an_engine_without_members_takes_the_loop():
    from distributions_amd import engine
    osh, gsh, vals, assign = workloads.make("dd", 100, 1, seed=SEED)
    pair = []
    for _ in range(2):
        g = engine.Gibbs(1.0, 0.2, gsh)
        g.load_rows_unassigned(vals, 3)
        g.set_shared(0, dd([1.5] * 16)[1])
        pair.append(g)
    gpu, twin = pair
    assert len(gpu) == 3 and not gpu.counts().any()
    grid = small_grid(16, 7)
    want, want_state, want_alphas = loop(twin, 0, grid, STATE)
    before = gpu.hyper_stats()
    got, state = gpu.sample_hypers_pass(0, grid, STATE)
    assert_loop(gpu, before, 16)
    assert got.tolist() == want.tolist() and state == want_state
    assert gpu.core.shared(0).alphas == want_alphas


def test_more_small_arguments_than_the_table_holds_take_the_loop():
    """256 coordinates x 24 distinct values below 0.5 x (value + 0, 1, 2) =
    18 432 arguments below 2.5, the table holds 16 384"""
    _, gpu, _, _, _ = swept("dd", 256, 6000, 12, None, sweeps=1)
    _, twin, _, _, _ = swept("dd", 256, 6000, 12, None, sweeps=1)
    grids = f32(np.linspace(0.05, 0.49, 256 * 24)).reshape(256, 24)
    assert len(set(grids.ravel().tolist())) == 256 * 24
    want, want_state, want_alphas = loop(twin, 0, grids, STATE)
    before = gpu.hyper_stats()
    got, state = gpu.sample_hypers_pass(0, grids, STATE)
    assert_loop(gpu, before, 256)
    assert got.tolist() == want.tolist() and state == want_state
    assert gpu.core.shared(0).alphas == want_alphas


# -- 5. refusals ---------------------------------------------------------------

def test_a_refused_pass_leaves_the_engine_as_it_was():
    orc, gpu, osh, gsh, vals = swept("dd_bb_gp", None, 4096, 9, None, sweeps=1)
    good = f32([0.5, 1.0, 2.0])
    with pytest.raises(RuntimeError, match="BetaBernoulli"):
        gpu.sample_hypers_pass(1, good, 9, coords=[0])
    with pytest.raises(RuntimeError, match="bad feature"):
        gpu.sample_hypers_pass(3, good, 9, coords=[0])
    with pytest.raises(RuntimeError, match="coordinate out of bounds: 8"):
        gpu.sample_hypers_pass(0, good, 9, coords=[0, 8])
    with pytest.raises(RuntimeError, match="grid value > 0"):
        gpu.sample_hypers_pass(0, f32([0.5, 0.0, 2.0]), 9)
    with pytest.raises(RuntimeError, match="grid value > 0"):
        gpu.sample_hypers_pass(0, f32([0.5, np.nan]), 9)
    with pytest.raises(RuntimeError, match="grid_size"):
        gpu.sample_hypers_pass(0, f32([]), 9)
    from distributions_amd import _core
    gpu.core.batch_sample(0, 1024, _core.rng_seed(3), 10 ** 6)
    with pytest.raises(RuntimeError, match="a batch is open"):
        gpu.sample_hypers_pass(0, good, 9)
    gpu.core.batch_apply_local()
    gpu.core.batch_finish()
    # nothing was installed: the oracle under the ORIGINAL values follows
    assert gpu.core.shared(0).alphas == [0.5] * 8
    assert gpu.shareds[0].alphas == [0.5] * 8
    st = ol.oracle().orc_rng_seed(3)
    orc.gibbs_batch(0, 1024, st, 10 ** 6)
    for b in range(1024, 4096, 1024):
        orc.gibbs_batch(b, b + 1024, st, 10 ** 6)
        gpu.sweep(b, b + 1024, 1024, 3, draw_base=10 ** 6)
    assert_same_engine_state(orc, gpu, "after refused passes")


# -- 6. M engines --------------------------------------------------------------

def test_many_engines_in_the_same_launches():
    from distributions_amd import engine
    dim = 16
    shapes = [(600, 1, [1.5] * dim), (4096, 12, [1.5] * dim),
              (30000, 1100, [1.5] * dim), (4096, 12, [0.1] * dim)]

    def build():
        out = []
        for i, (n, k, alphas) in enumerate(shapes):
            osh, gsh, vals, assign = workloads.make("dd", n, k, seed=SEED + i,
                                                    dim=dim)
            g = engine.Gibbs(1.0, 0.2, gsh)
            g.load_rows(vals, assign, k, 1)
            if k > 1:                # (the first keeps its one group)
                g.sweep(0, n, max(256, n // 4), SEED, draw_base=0)
            g.set_shared(0, dd(alphas)[1])
            out.append((g, vals, n))
        return out

    set_a, twins = build(), build()
    engines = [g for g, _, _ in set_a]
    print("groups", [len(g) for g in engines])
    grids = f32(np.random.default_rng(6).uniform(0.9, 4.0, (dim, 7)))
    grids[:, 3] = 1.5
    states = np.array([11, 22, 33, 44], np.uint32)
    # the same engine twice: refused, nothing changes
    with pytest.raises(RuntimeError, match="the same engine twice"):
        engine.sample_hypers_pass_many(engines + engines[:1], 0, grids,
                                       list(states) + [55])
    for g, (_, _, alphas) in zip(engines, shapes):
        assert g.core.shared(0).alphas == [float(np.float32(a))
                                           for a in alphas]
    before = [g.hyper_stats() for g in engines]
    indices, after = engine.sample_hypers_pass_many(engines, 0, grids, states)
    assert indices.shape == (4, dim) and indices.dtype == np.uint32
    assert after.dtype == np.uint32 and after.shape == (4,)
    for i, (twin, _, _) in enumerate(twins):
        want, want_state = twin.sample_hypers_pass(0, grids, int(states[i]))
        assert indices[i].tolist() == want.tolist(), i
        assert int(after[i]) == want_state, i
        assert engines[i].core.shared(0).alphas == twin.core.shared(0).alphas
        assert engines[i].shareds[0].alphas == twin.core.shared(0).alphas
    for i in range(3):
        assert_device_pass(engines[i], before[i], dim, 7)
    assert_loop(engines[3], before[3], dim)
    # the chains after the pass equal oracles created with the drawn alphas
    orcs = []
    for g, vals, n in set_a:
        o = ol.OracleMixture(1.0, 0.2, [dd(g.core.shared(0).alphas)[0]])
        o.adopt(g, vals)
        orcs.append(o)
    rows = 500
    later = engine.sweep_sequential_many(engines, 0, rows, after)
    for i, o in enumerate(orcs):
        assert o.gibbs_sequential(0, rows, int(after[i])) == int(later[i])
        assert_same_engine_state(o, engines[i], "chain %d" % i)
