"""Who frees what: an engine's pinned host buffers and events are taken lazily,
by the first call that needs them, and released when the engine goes.  Every
case here takes some of them, lets an engine go (or a buffer grow) and ends, as
smoke() does, with assignments and group sizes bit-equal to the oracle's batched
sweep -- at smoke()'s shape: DirichletDiscrete dim 16, 4096 rows, 32 groups,
batches of 1024."""
import gc
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

N, K, DIM, BATCH, SEED = 4096, 32, 16, 1024, 12345


def data(k=K):
    rng = np.random.default_rng(20240601)
    values = rng.integers(0, DIM, N).astype(np.uint32)
    assign = (np.arange(N) % k).astype(np.uint32)
    return values, assign


def make_oracle(alpha=1.0, k=K, empty=1):
    import oracle_lib as ol
    values, assign = data(k)
    orc = ol.OracleMixture(alpha, 0.2, [ol.make_shared(ol.DD,
                                                       alphas=[0.5] * DIM)])
    orc.init_from_assignments([values], assign, k, empty)
    return orc


def make_engine(alpha=1.0, k=K, empty=1, **options):
    from distributions_amd import engine
    values, assign = data(k)
    gpu = engine.Gibbs(alpha=alpha, d=0.2,
                       shareds=[engine.dd_shared([0.5] * DIM)])
    for name, value in options.items():
        gpu.set_option(name, value)
    gpu.load_rows([values], assign, nonempty_groups=k, empty_groups=empty)
    return gpu


def oracle_sweep(orc, draw_base=0):
    import oracle_lib as ol
    seed_state = ol.oracle().orc_rng_seed(SEED)
    for b in range(0, N, BATCH):
        orc.gibbs_batch(b, b + BATCH, seed_state, draw_base)


def assert_same(gpu, orc):
    assert np.array_equal(gpu.assignments(), orc.assign)
    assert np.array_equal(gpu.counts(), orc.counts())


@pytest.fixture(scope="module")
def smoke_oracle():
    """smoke()'s sweep in the oracle, computed once and left as it is"""
    orc = make_oracle()
    oracle_sweep(orc)
    return orc


def fresh_engine_equals(smoke_oracle):
    gpu = make_engine()
    gpu.sweep(0, N, BATCH, SEED)
    assert_same(gpu, smoke_oracle)


def test_engine_that_took_every_lazy_resource_goes_and_another_comes(
        smoke_oracle):
    """One engine takes, in turn, the value-sorted batch's and the
    device-normalised run's buffers, the hyper-parameter draw's, the exact
    chain's and the sharded sweep's (one rank, host transport), following the
    oracle all the way; it is destroyed, and a second engine of the same
    process repeats smoke()."""
    from distributions_amd import _core
    gpu = make_engine(value_sorted=2, device_normalise=1)
    orc = make_oracle()
    gpu.sweep(0, N, BATCH, SEED)
    oracle_sweep(orc)
    assert_same(gpu, orc)
    seen = gpu.core.debug_counts()
    assert seen["value_sorted_batches"] > 0 and seen["device_normalised"] > 0
    # the draw among candidates that all are the values in place: the pinned
    # draw is taken, the model stays the oracle's
    index, _ = gpu.sample_clustering([1.0] * 3, [0.2] * 3, _core.rng_seed(7))
    assert 0 <= index < 3
    assert gpu.hyper_stats()[3] > 0
    want = orc.gibbs_sequential(0, 512, 777)
    assert gpu.sweep_sequential(0, 512, 777) == want
    assert gpu.core.chain_launches() > 0
    assert_same(gpu, orc)
    comm = _core.Comm(_core.comm_unique_id_host(), 0, 1)
    assert comm.size() == (0, 1)
    gpu.core.sweep_sharded(comm, N // BATCH, BATCH, _core.rng_seed(SEED), N)
    oracle_sweep(orc, N)
    assert_same(gpu, orc)
    assert gpu.validate()["code"] == 0
    del gpu, comm
    gc.collect()
    fresh_engine_equals(smoke_oracle)


def test_engine_goes_with_its_run_still_open(smoke_oracle):
    """A sweep is queued and nothing reads the engine afterwards: the run is
    open (and a look at its state may be in flight) when the engine goes.
    That the run IS open cannot be asked of this engine -- any question,
    debug_counts included, settles it -- so the case relies on the test
    above, where the same options at the same shape are seen to take the
    device-normalised path."""
    gpu = make_engine(value_sorted=2, device_normalise=1)
    gpu.sweep(0, N, BATCH, SEED)
    del gpu
    gc.collect()
    fresh_engine_equals(smoke_oracle)


@pytest.mark.parametrize("value_sorted", [0, 2])
def test_group_sizes_outgrow_their_pinned_buffer(value_sorted):
    """The host reads the group sizes of a host-normalised batch from pinned
    memory whose capacity is a power of two, 64 at the least.  60 groups and
    4 empty ones fill 64 slots exactly; alpha = 50 founds groups in every
    batch, so the next batch's sizes need the next capacity."""
    k, empty, alpha = 60, 4, 50.0
    gpu = make_engine(alpha, k, empty, value_sorted=value_sorted,
                      device_normalise=0)
    orc = make_oracle(alpha, k, empty)
    assert len(gpu) == 64
    gpu.sweep(0, N, BATCH, SEED)
    oracle_sweep(orc)
    assert len(orc) > 64
    assert len(gpu) == len(orc)
    assert_same(gpu, orc)
    batches = gpu.core.debug_counts()
    assert batches["device_normalised"] == 0
    assert (batches["value_sorted_batches"] > 0) == (value_sorted == 2)
