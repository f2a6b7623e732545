"""The hyper-parameter step between passes of dist_gibbs_sweep_sharded: 2
processes over the library's host transport (as tests/test_gpu_native_ranks.py
runs them), value-partitioned DirichletDiscrete.

- after a sharded pass the cells of the other rank's values are stale:
  scoring fails and says so, until dist_gibbs_gather_cells;
- then both ranks, calling sample_hypers with equal rng_state, choose the same
  index -- the one the oracle draws from its scores of the same state;
- the passes after the install equal one process with the same batch
  composition: the oracle created with the chosen values and loaded with the
  state at the switch, bit for bit."""
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

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

WORLD, N, PER, DIM = 2, 9001, 750, 16
BEFORE, AFTER = 2, 3            # passes before and after the switch
DRAW_STATE = 424243
GRID = [[0.5] * DIM, [0.05] * DIM, [4.0] * DIM,
        [0.1 + 0.2 * i for i in range(DIM)]]


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
    cands = [engine.dd_shared(a) for a in GRID]
    notes = []
    for s in range(BEFORE):
        sharded.sweep(PER, _core.rng_seed(SEED), draw_base=s * N)
    try:
        gpu.score_data_grid(0, cands)
        notes.append("scored on stale cells")
    except RuntimeError as e:
        notes.append(str(e))
    try:
        gpu.sample_hypers(0, cands, DRAW_STATE)
        notes.append("sampled on stale cells")
    except RuntimeError as e:
        notes.append(str(e))
    # the wrapper gathers the cells first (collective: every rank alike)
    index, state = sharded.sample_hypers(0, cands, DRAW_STATE)
    shared = gpu.core.shared(0)
    for s in range(BEFORE, BEFORE + AFTER):
        sharded.sweep(PER, _core.rng_seed(SEED), draw_base=s * N)
    sharded.gather_cells()
    with open(os.path.join(out, "notes_%d.txt" % rank), "w") as f:
        f.write("\n".join(notes))
    np.save(os.path.join(out, "draw_%d.npy" % rank),
            np.array([index, state], np.int64))
    np.save(os.path.join(out, "alphas_%d.npy" % rank),
            np.array(shared.alphas, np.float32))
    np.save(os.path.join(out, "assign_%d.npy" % rank), gpu.assignments())
    np.save(os.path.join(out, "counts_%d.npy" % rank), gpu.counts())
    np.save(os.path.join(out, "groups_%d.npy" % rank), np.stack(
        [gpu.get_group(0, g) for g in range(len(gpu))]))
    # (no validate() here: it recounts from the rows of THIS rank, and a
    # replica's group sizes count every rank's)
    dist.destroy_process_group()


def oracle_passes(m, bounds, sweeps):
    """one process, the ranks' batch composition (test_gpu_native_ranks)"""
    import oracle_lib as ol
    L = ol.oracle()
    ol._phase_sigs(L)
    st = L.orc_rng_seed(SEED)
    longest = max(hi - lo for lo, hi in bounds)
    for s in sweeps:
        for b in range(0, longest, PER):
            snap = m.counts().copy()
            moves = []
            for lo, hi in bounds:
                r0, r1 = min(hi, lo + b), min(hi, lo + b + PER)
                old = np.zeros(r1 - r0 + 1, np.uint32)
                new = np.zeros(r1 - r0 + 1, np.uint32)
                L.orc_mix_batch_sample(m.h, r0, r1, m._vals, m.assign, st,
                                       s * N, 0, old, new)
                moves.append((r0, r1, old, new))
            for r0, r1, old, new in moves:
                L.orc_mix_apply_moves(m.h, r0, r1, m._vals, m.assign, old, new)
            L.orc_mix_batch_finish(m.h, np.ascontiguousarray(snap, np.int32))


def test_two_ranks_draw_alike_and_go_on_as_one_process(tmp_path):
    import oracle_lib as ol
    mp.spawn(worker, args=(WORLD, free_port(), str(tmp_path)), nprocs=WORLD,
             join=True)
    osh, gsh, vals, assign, bounds = place("dd", N, WORLD, "value", DIM, K)
    m = ol.OracleMixture(1.0, 0.2, osh)
    m.init_from_assignments(vals, assign, K, 2)
    oracle_passes(m, bounds, range(BEFORE))
    L = m.L
    L.orc_mix_slave_score_data_grid.restype = None
    L.orc_mix_slave_score_data_grid.argtypes = [
        ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ol.Shared),
        ctypes.c_size_t, ol.c_f32p]
    shareds = [ol.make_shared(ol.DD, alphas=a) for a in GRID]
    scores = np.zeros(len(GRID), np.float32)
    L.orc_mix_slave_score_data_grid(m.h, 0, (ol.Shared * len(GRID))(*shareds),
                                    len(GRID), scores)
    st = ctypes.c_uint32(DRAW_STATE)
    want = L.orc_sample_from_scores_overwrite(ctypes.byref(st), len(GRID),
                                              scores)
    after = ol.OracleMixture(1.0, 0.2, [shareds[want]])
    after.adopt(m, vals)
    oracle_passes(after, bounds, range(BEFORE, BEFORE + AFTER))
    for r in range(WORLD):
        notes = open(tmp_path / ("notes_%d.txt" % r)).read().split("\n")
        assert len(notes) == 2
        for note in notes:
            assert "stale on a value-partitioned rank" in note, note
        index, state = np.load(tmp_path / ("draw_%d.npy" % r))
        assert (index, state) == (want, st.value), r
        np.testing.assert_array_equal(
            np.load(tmp_path / ("alphas_%d.npy" % r)),
            np.array(GRID[want], np.float32))
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
