"""A whole coordinate pass between passes of dist_gibbs_sweep_sharded: 2
processes over the library's host transport, value-partitioned
DirichletDiscrete, in the manner of tests/test_gpu_hypers_ranks.py.

- after a sharded pass the cells of the other rank's values are stale: the
  pass fails and says so, until the wrapper has gathered them;
- both ranks, calling ShardedGibbs.sample_hypers_pass with equal rng_state,
  return the same indices -- the sequence the oracle draws, step by step, from
  its scores of the same state -- on the device path (2 launches);
- the passes after the install equal one process with the same batch
  composition, bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_gpu_native_ranks import K, SEED, free_port, place  # noqa: E402
from test_gpu_hypers_ranks import (AFTER, BEFORE, DIM, DRAW_STATE,  # noqa: E402
                                   N, PER, WORLD, oracle_passes)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

GRID = np.array([0.5, 0.25, 1.0, 2.0], np.float32)


def worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("DIST_COMM_TIMEOUT_S", "120")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import oracle_lib as ol
    from distributions_amd import _core, engine
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    osh, gsh, vals, assign, bounds = place("dd", N, world, "value", DIM, K)
    lo, hi = bounds[rank]
    cols = [torch.from_numpy(ol.value_words(s.kind, v[lo:hi]).view(np.int32)
                             .copy()).to(dev) for s, v in zip(osh, vals)]
    packed = torch.from_numpy(assign[lo:hi].view(np.int32).copy()).to(dev)
    gpu = engine.Gibbs(1.0, 0.2, gsh)
    gpu.set_option("value_sorted", 2)
    gpu.set_option("device_normalise", 1)
    gpu.load_rows_torch(cols, packed.clone(), K, 2, row_offset=lo)
    sharded = engine.ShardedGibbs(gpu.core, hi - lo, lo, device=dev,
                                  columns=cols, assign_packed=packed)
    sharded.sync_initial_stats()
    assert sharded.use_native_comm()
    sharded.partition_by_value()
    for s in range(BEFORE):
        sharded.sweep(PER, _core.rng_seed(SEED), draw_base=s * N)
    try:
        gpu.sample_hypers_pass(0, GRID, DRAW_STATE)
        note = "sampled on stale cells"
    except RuntimeError as e:
        note = str(e)
    # the wrapper gathers the cells first (collective: every rank alike)
    before = gpu.hyper_stats()
    indices, state = sharded.sample_hypers_pass(0, GRID, DRAW_STATE)
    launches = gpu.hyper_stats()[2] - before[2]
    shared = gpu.core.shared(0)
    for s in range(BEFORE, BEFORE + AFTER):
        sharded.sweep(PER, _core.rng_seed(SEED), draw_base=s * N)
    sharded.gather_cells()
    with open(os.path.join(out, "note_%d.txt" % rank), "w") as f:
        f.write(note)
    np.save(os.path.join(out, "draw_%d.npy" % rank),
            np.array(list(indices) + [state, launches], np.int64))
    np.save(os.path.join(out, "alphas_%d.npy" % rank),
            np.array(shared.alphas, np.float32))
    np.save(os.path.join(out, "assign_%d.npy" % rank), gpu.assignments())
    np.save(os.path.join(out, "counts_%d.npy" % rank), gpu.counts())
    np.save(os.path.join(out, "groups_%d.npy" % rank), np.stack(
        [gpu.get_group(0, g) for g in range(len(gpu))]))
    dist.destroy_process_group()


def test_two_ranks_pass_alike_and_go_on_as_one_process(tmp_path):
    import oracle_lib as ol
    from test_gpu_hyper_pass import LAUNCHES, oracle_pass
    mp.spawn(worker, args=(WORLD, free_port(), str(tmp_path)), nprocs=WORLD,
             join=True)
    osh, gsh, vals, assign, bounds = place("dd", N, WORLD, "value", DIM, K)
    m = ol.OracleMixture(1.0, 0.2, osh)
    m.init_from_assignments(vals, assign, K, 2)
    oracle_passes(m, bounds, range(BEFORE))
    want, want_state, want_alphas = oracle_pass(m, 0, [0.5] * DIM, GRID,
                                                DRAW_STATE)
    print("drawn", want.tolist())
    after = ol.OracleMixture(1.0, 0.2,
                             [ol.make_shared(ol.DD, alphas=want_alphas)])
    after.adopt(m, vals)
    oracle_passes(after, bounds, range(BEFORE, BEFORE + AFTER))
    for r in range(WORLD):
        note = open(tmp_path / ("note_%d.txt" % r)).read()
        assert "stale on a value-partitioned rank" in note, note
        draw = np.load(tmp_path / ("draw_%d.npy" % r))
        assert draw[:DIM].tolist() == want.tolist(), r
        assert draw[DIM] == want_state and draw[DIM + 1] == LAUNCHES, r
        np.testing.assert_array_equal(
            np.load(tmp_path / ("alphas_%d.npy" % r)),
            np.array(want_alphas, np.float32))
    counts = [np.load(tmp_path / ("counts_%d.npy" % r)) for r in range(WORLD)]
    groups = [np.load(tmp_path / ("groups_%d.npy" % r)) for r in range(WORLD)]
    assert np.array_equal(counts[0], counts[1])
    assert np.array_equal(groups[0], groups[1])
    assert np.array_equal(after.counts(), counts[0])
    got = np.concatenate([np.load(tmp_path / ("assign_%d.npy" % r))
                          for r in range(WORLD)])
    assert np.array_equal(got, after.assign)
    want_groups = np.stack([after.get_group(0, g) for g in range(len(after))])
    assert np.array_equal(want_groups, groups[0])
