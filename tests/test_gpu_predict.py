"""dist_gibbs_predict (k_predict): held-out rows' log predictive density and
group, bit for bit against the expectation tests/predict_expect.py composes
from the oracle (and tests/test_predict_oracle.py holds to float64).

Every case of predict_expect.CASES: the 12 feature lists at K = 16 + 3 empty,
the same after 2 sweeps at batch 16 (singletons, vanished groups, another K),
LowEntropy with the returned prior_total, engines that hold only empty groups
(K = 1, K = 3), K = 17, DD-256 at K = 1025, DPD with 10 000 values at
K = 8193.  Then launch geometry, equivariance under a permutation of the
queries, and the reader rules."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle_lib as ol  # noqa: E402
import predict_expect as pe  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
GROUP_SENTINEL = -7


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def word(x):
    return int(np.float32(x).view(np.uint32))


_ENGINES = {}


def engine_of(name):
    """one engine per case, shared: predict leaves it as it was"""
    if name not in _ENGINES:
        _ENGINES[name] = pe.case(name).engine()
    return _ENGINES[name]


def snapshot(gpu):
    K = len(gpu)
    groups = [gpu.get_group(f, k) for f in range(len(gpu.shareds))
              for k in sorted({0, K // 2, K - 1})]
    return (gpu.counts().copy(), gpu.assignments().copy(),
            [gpu.core.packed_to_global(k) for k in range(K)],
            np.concatenate(groups) if groups else np.zeros(0))


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(pe.CASES))
def test_predict_is_the_oracles_bit_for_bit(name):
    c = pe.case(name)
    e = c.expect()
    gpu = engine_of(name)
    before = snapshot(gpu)
    logp, draw, total = gpu.predict(c.qvals, "sample", seed=pe.DRAW_SEED,
                                    draw_base=pe.DRAW_BASE)
    logp_m, first, total_m = gpu.predict(c.qvals, "map")
    logp_n, none, _ = gpu.predict(c.qvals, None)
    x = pe.excursion(logp, c)
    print("%s: K=%d, %d held-out rows: logp bits differ in %d rows, draws in "
          "%d, maxima in %d; worst excursion / band %.3f" % (
              name, c.K, c.nq, int((bits(logp) != bits(e["logp"])).sum()),
              int((draw != e["draw"]).sum()), int((first != e["map"]).sum()),
              x.max()))
    assert np.array_equal(bits(logp), bits(e["logp"]))
    assert np.array_equal(bits(logp_m), bits(e["logp"]))
    assert np.array_equal(bits(logp_n), bits(e["logp"]))
    assert none is None
    assert np.array_equal(draw, e["draw"])
    assert np.array_equal(first, e["map"])
    # log_sum_exp of the clustering model's scores alone: what a LowEntropy
    # caller subtracts (PitmanYor's are normalised: zero up to rounding)
    assert word(total) == word(e["prior_total"]) == word(total_m)
    if c.le is None:
        assert abs(float(total)) <= 1e-4
    # the band a tolerance-level variant would be held to
    assert x.max() <= 1.0
    # a pure reader
    assert same(before, snapshot(gpu))


def predict_dev(gpu, qvals, n, mode, want_logp=True, want_group=True,
                pad=64):
    """predict_dev on the first n held-out rows into sentinel-filled device
    buffers -> (logp or None, group or None), padding included"""
    import torch
    cols = [torch.from_numpy(np.ascontiguousarray(w[:n]).view(np.int32)
                             .copy()).cuda() for w in qvals]
    logp = torch.full((n + pad,), SENTINEL, dtype=torch.float32,
                      device="cuda")
    group = torch.full((n + pad,), GROUP_SENTINEL, dtype=torch.int32,
                       device="cuda")
    torch.cuda.synchronize()
    gpu.core.predict_dev([int(t.data_ptr()) for t in cols], n,
                         int(logp.data_ptr()) if want_logp else 0,
                         int(group.data_ptr()) if want_group else 0, mode,
                         ol.oracle().orc_rng_seed(pe.DRAW_SEED),
                         pe.DRAW_BASE)
    torch.cuda.synchronize()
    return logp.cpu().numpy(), group.cpu().numpy()


@pytest.mark.parametrize("name", ["dd", "gp_nich_swept", "dd_bb_gp"])
def test_launch_geometry_chunks_and_optional_outputs(name):
    """whole and partial waves, chunk boundaries that are no multiple of 64
    (the draw of row q is engine step draw_base + q + 1 whatever the chunk),
    nothing written past n, either output alone"""
    c = pe.case(name)
    e = c.expect()
    gpu = engine_of(name)
    words = pe.query_words(c.orc, c.qvals)
    try:
        for chunk in (1 << 22, 100, 37, 1):
            gpu.set_option("debug.predict_chunk", chunk)
            for n in (1, 63, 64, 65, 300):
                if chunk == 1 and n > 65:
                    continue
                for mode, key in ((0, "draw"), (1, "map")):
                    logp, group = predict_dev(gpu, words, n, mode)
                    assert np.array_equal(bits(logp[:n]),
                                          bits(e["logp"][:n])), (chunk, n)
                    assert np.array_equal(group[:n].view(np.uint32),
                                          e[key][:n]), (chunk, n, key)
                    assert np.all(logp[n:] == SENTINEL), (chunk, n)
                    assert np.all(group[n:] == GROUP_SENTINEL), (chunk, n)
                logp, group = predict_dev(gpu, words, n, 0, want_group=False)
                assert np.array_equal(bits(logp[:n]), bits(e["logp"][:n]))
                assert np.all(group == GROUP_SENTINEL)
                logp, group = predict_dev(gpu, words, n, 0, want_logp=False)
                assert np.all(logp == SENTINEL)
                assert np.array_equal(group[:n].view(np.uint32),
                                      e["draw"][:n])
        # no rows: nothing happens
        logp, group = predict_dev(gpu, words, 0, 0)
        assert np.all(logp == SENTINEL) and np.all(group == GROUP_SENTINEL)
        with pytest.raises(RuntimeError, match="predict_chunk"):
            gpu.set_option("debug.predict_chunk", 0)
    finally:
        gpu.set_option("debug.predict_chunk", 1 << 22)


def test_predict_torch_returns_device_tensors():
    import torch
    c = pe.case("gp_nich")
    e = c.expect()
    gpu = engine_of("gp_nich")
    words = pe.query_words(c.orc, c.qvals)
    cols = [torch.from_numpy(w.view(np.int32).copy()).cuda() for w in words]
    logp, group, total = gpu.predict_torch(cols, "sample", seed=pe.DRAW_SEED,
                                           draw_base=pe.DRAW_BASE)
    assert logp.is_cuda and group.is_cuda
    assert np.array_equal(bits(logp.cpu().numpy()), bits(e["logp"]))
    assert np.array_equal(group.cpu().numpy().view(np.uint32), e["draw"])
    assert word(total) == word(e["prior_total"])
    logp, group, _ = gpu.predict_torch(cols, None)
    assert group is None
    assert np.array_equal(bits(logp.cpu().numpy()), bits(e["logp"]))


@pytest.mark.parametrize("name", ["dd_zipf", "dd_bb_gp_swept"])
def test_permuting_the_queries_permutes_the_results(name):
    c = pe.case(name)
    gpu = engine_of(name)
    logp, first, _ = gpu.predict(c.qvals, "map")
    perm = np.random.default_rng(3).permutation(c.nq)
    logp_p, first_p, _ = gpu.predict([q[perm] for q in c.qvals], "map")
    assert np.array_equal(bits(logp_p), bits(logp[perm]))
    assert np.array_equal(first_p, first[perm])


# ---------------------------------------------------------------------------
# reader rules


def test_predict_refuses_an_open_batch_and_sees_the_state_after_it():
    c = pe.case("dd")
    gpu = c.engine()          # (its own engine: the state moves)
    before, _, _ = gpu.predict(c.qvals, None)
    st = ol.oracle().orc_rng_seed(3)
    gpu.core.batch_sample(0, 1024, st, 0)
    with pytest.raises(RuntimeError, match="batch open"):
        gpu.predict(c.qvals, "map")
    gpu.core.batch_apply_local()
    gpu.core.batch_finish()
    orc = ol.OracleMixture(c.alpha, c.d, c.osh)
    orc.init_from_assignments(c.vals, c.assign0, c.k, c.empty)
    orc.gibbs_batch(0, 1024, st, 0)
    assert np.array_equal(gpu.assignments(), orc.assign)
    e = pe.expect(orc, c.qvals, ol.oracle().orc_rng_seed(pe.DRAW_SEED), 0)
    logp, draw, _ = gpu.predict(c.qvals, "sample", seed=pe.DRAW_SEED)
    assert np.array_equal(bits(logp), bits(e["logp"]))
    assert np.array_equal(draw, e["draw"])
    assert not np.array_equal(bits(logp), bits(before))


@pytest.mark.parametrize("name,feature,value,what", [
    ("dd", 0, 16, "feature 0"), ("dd_bb_gp", 1, 2, "feature 1"),
    ("bb", 0, 7, "feature 0")])
def test_a_value_outside_its_domain_fails_and_names_the_row(name, feature,
                                                            value, what):
    c = pe.case(name)
    e = c.expect()
    gpu = engine_of(name)
    gpu.set_option("debug.predict_chunk", 64)
    try:
        bad = [q.copy() for q in c.qvals]
        bad[feature][211] = value
        bad[feature][130] = value       # the first offending row is named
        if name == "dd_bb_gp":
            bad[2][130] = 2 ** 31       # (GammaPoisson takes any count)
            bad[0][250] = 200           # (a later row, an earlier feature)
        with pytest.raises(RuntimeError, match="row 130, " + what):
            gpu.predict(bad, "sample")
        # process and engine go on
        logp, first, _ = gpu.predict(c.qvals, "map")
        assert np.array_equal(bits(logp), bits(e["logp"]))
        assert np.array_equal(first, e["map"])
    finally:
        gpu.set_option("debug.predict_chunk", 1 << 22)


def test_a_dpd_value_beyond_the_table_scores_as_other():
    c = pe.case("dpd_other")
    gpu = engine_of("dpd_other")
    other = np.nonzero(c.qvals[0] == pe.OTHER)[0]
    assert len(other) == 2
    q = [c.qvals[0].copy()]
    q[0][other] = [50, 123456]          # (the table holds values 0 .. 49)
    logp, first, _ = gpu.predict(q, "map")
    assert np.array_equal(bits(logp), bits(c.expect()["logp"]))
    assert np.array_equal(first, c.expect()["map"])


@pytest.mark.parametrize("name", ["dd", "gp_nich"])
def test_predict_then_sweep_is_the_oracles_sweep(name):
    c = pe.case(name)
    gpu = c.engine()
    gpu.predict(c.qvals, "sample", seed=1)
    orc = ol.OracleMixture(c.alpha, c.d, c.osh)
    orc.init_from_assignments(c.vals, c.assign0, c.k, c.empty)
    st = ol.oracle().orc_rng_seed(11)
    for b in range(0, c.n, 500):
        orc.gibbs_batch(b, b + 500, st, 0)
    gpu.sweep(0, c.n, 500, 11)
    gpu.predict(c.qvals, "map")         # (closes a run the sweep left open)
    assert np.array_equal(gpu.assignments(), orc.assign)
    assert np.array_equal(gpu.counts(), orc.counts())
    gpu.validate()
    e = pe.expect(orc, c.qvals, ol.oracle().orc_rng_seed(1), 0)
    logp, draw, _ = gpu.predict(c.qvals, "sample", seed=1)
    assert np.array_equal(bits(logp), bits(e["logp"]))
    assert np.array_equal(draw, e["draw"])


# ---------------------------------------------------------------------------
# two value-partitioned ranks on one GPU (the library's host transport, as
# tests/test_gpu_hypers_ranks.py runs them)

WORLD, N, PER, DIM = 2, 3001, 750, 16
NQ = 150


def rank_queries(rank):
    rng = np.random.default_rng(500 + rank)
    return [rng.integers(0, DIM, NQ).astype(np.uint32)]


def worker(rank, world, port, out):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("DIST_COMM_TIMEOUT_S", "120")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from distributions_amd import _core, engine
    from test_gpu_native_ranks import K, SEED, place
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
    sharded.sweep(PER, _core.rng_seed(SEED), draw_base=0)
    q = rank_queries(rank)
    try:
        gpu.predict(q, "map")
        note = "predicted on stale cells"
    except RuntimeError as e:
        note = str(e)
    # the wrapper gathers the cells first (collective: every rank alike)
    logp, draw, total = sharded.predict(q, "sample",
                                        _core.rng_seed(pe.DRAW_SEED), 17)
    _, first, _ = sharded.predict(q, "map")
    with open(os.path.join(out, "note_%d.txt" % rank), "w") as f:
        f.write(note)
    np.save(os.path.join(out, "logp_%d.npy" % rank), logp)
    np.save(os.path.join(out, "draw_%d.npy" % rank), draw)
    np.save(os.path.join(out, "map_%d.npy" % rank), first)
    dist.destroy_process_group()


def test_value_partitioned_ranks_gather_their_cells_first(tmp_path):
    import torch.multiprocessing as mp
    from test_gpu_native_ranks import K, SEED, free_port, place
    mp.spawn(worker, args=(WORLD, free_port(), str(tmp_path)), nprocs=WORLD,
             join=True)
    osh, gsh, vals, assign, bounds = place("dd", N, WORLD, "value", DIM, K)
    m = ol.OracleMixture(1.0, 0.2, osh)
    m.init_from_assignments(vals, assign, K, 2)
    L = ol.oracle()
    ol._phase_sigs(L)
    st = L.orc_rng_seed(SEED)
    longest = max(hi - lo for lo, hi in bounds)
    for b in range(0, longest, PER):   # one pass, the ranks' composition
        snap = m.counts().copy()
        moves = []
        for lo, hi in bounds:
            r0, r1 = min(hi, lo + b), min(hi, lo + b + PER)
            old = np.zeros(r1 - r0 + 1, np.uint32)
            new = np.zeros(r1 - r0 + 1, np.uint32)
            L.orc_mix_batch_sample(m.h, r0, r1, m._vals, m.assign, st, 0, 0,
                                   old, new)
            moves.append((r0, r1, old, new))
        for r0, r1, old, new in moves:
            L.orc_mix_apply_moves(m.h, r0, r1, m._vals, m.assign, old, new)
        L.orc_mix_batch_finish(m.h, np.ascontiguousarray(snap, np.int32))
    for r in range(WORLD):
        note = open(tmp_path / ("note_%d.txt" % r)).read()
        assert "predict: the cells of other ranks' values are stale" in note
        e = pe.expect(m, rank_queries(r), L.orc_rng_seed(pe.DRAW_SEED), 17)
        assert np.array_equal(bits(np.load(tmp_path / ("logp_%d.npy" % r))),
                              bits(e["logp"])), r
        assert np.array_equal(np.load(tmp_path / ("draw_%d.npy" % r)),
                              e["draw"]), r
        assert np.array_equal(np.load(tmp_path / ("map_%d.npy" % r)),
                              e["map"]), r
