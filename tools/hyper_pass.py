#!/usr/bin/env python3
"""Times one DirichletDiscrete coordinate pass of the hyper-parameter step at
the benchmark's shape (DD-256, K ~ 1024 groups): for every coordinate v a grid
of G candidate values for alphas[v], scored against the groups, one drawn and
installed -- 256 grids of G candidates per pass.

Three routes, alternated run by run on the same engine state:

  engine   dist_gibbs_sample_hypers per coordinate (grid, draw and install on
           the device; kernels_hyper.h)
  pass     dist_gibbs_sample_hypers_pass: the whole pass in one call, two
           launches and one install
  parent   what was possible before those entry points: dist_gibbs_get_group
           for every group once, a stand-alone mixture built from them,
           dist_mixture_score_data_grid per coordinate, the draw on the host.
           (Installing the result would ALSO mean a new engine and reloading
           the rows; that is not timed, the comparison is of the scoring
           alone plus the one-off pull of the groups.)

and next to them the time of one assignment sweep of the same engine.
--many M: also M engines of --many-rows rows each, one
dist_gibbs_sample_hypers_pass_many call against M single passes.  Prints one
JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000000)
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--many", type=int, default=0)
    ap.add_argument("--many-rows", type=int, default=20000)
    args = ap.parse_args()
    from distributions_amd import _core, engine

    rng = np.random.default_rng(1)
    n, k, dim = args.rows, args.groups, args.dim
    values = rng.integers(0, dim, n).astype(np.uint32)
    assign = (np.arange(n) % k).astype(np.uint32)
    gpu = engine.Gibbs(1.0, 0.2, [engine.dd_shared([0.5] * dim)])
    gpu.load_rows([values], assign, k, 1)
    for s in range(2):          # churn, and every shape warmed up
        gpu.sweep(0, n, args.batch, 7, draw_base=s * n)
    len(gpu)
    grid_values = np.geomspace(0.05, 5.0, args.grid).astype(np.float32)

    def candidates(alphas, v):
        out = []
        for a in grid_values:
            x = list(alphas)
            x[v] = float(a)
            out.append(engine.dd_shared(x))
        return out

    def engine_pass(state):
        alphas = list(gpu.core.shared(0).alphas)
        for v in range(dim):
            index, state = gpu.sample_hypers(0, candidates(alphas, v), state)
            alphas[v] = float(grid_values[index])
        return state

    def whole_pass(state):
        return gpu.sample_hypers_pass(0, grid_values, state)[1]

    def parent_pass(state):
        t0 = time.perf_counter()
        alphas = list(gpu.core.shared(0).alphas)
        mix = _core.SlaveMixture(engine.dd_shared(alphas))
        for g in range(len(gpu)):
            mix.append(np.ascontiguousarray(gpu.get_group(0, g), np.uint32))
        mix.init()
        pulled = time.perf_counter() - t0
        for v in range(dim):
            scores = mix.score_data_grid(candidates(alphas, v))
            index, state = _core.sample_from_scores_overwrite(state, scores)
            alphas[v] = float(grid_values[index])
        return state, pulled

    def timed(fn, *a):
        _core.synchronize()
        t0 = time.perf_counter()
        out = fn(*a)
        _core.synchronize()
        return time.perf_counter() - t0, out

    # the host's share of either route: building 256 x G candidate structs
    t_build, _ = timed(lambda: [candidates([0.5] * dim, v)
                                for v in range(dim)])
    def stats_of(fn, *a):
        before = gpu.hyper_stats()
        fn(*a)
        after = gpu.hyper_stats()
        gpu.set_shared(0, engine.dd_shared([0.5] * dim))
        return dict(zip(["chains", "candidates", "launches", "calls"],
                        [int(y - x) for x, y in zip(before, after)]))

    stats_engine = stats_of(engine_pass, 11)   # (warm-up of every route too)
    stats_pass = stats_of(whole_pass, 11)
    parent_pass(11)
    t_engine, t_pass, t_parent, t_pull, t_sweep = [], [], [], [], []
    for r in range(args.repeats):
        t, state_engine = timed(engine_pass, 100 + r)
        t_engine.append(t)
        gpu.set_shared(0, engine.dd_shared([0.5] * dim))
        t, state_pass = timed(whole_pass, 100 + r)
        t_pass.append(t)
        assert state_pass == state_engine, "the pass left the loop's result"
        gpu.set_shared(0, engine.dd_shared([0.5] * dim))
        t, (_, pulled) = timed(parent_pass, 100 + r)
        t_parent.append(t)
        t_pull.append(pulled)
        t, _ = timed(gpu.sweep, 0, n, args.batch, 7, (5 + r) * n)
        len(gpu)
        t_sweep.append(t)
    many = None
    if args.many:
        engines = []
        for i in range(args.many):
            r = np.random.default_rng(100 + i)
            g = engine.Gibbs(1.0, 0.2, [engine.dd_shared([0.5] * dim)])
            g.load_rows([r.integers(0, dim, args.many_rows).astype(np.uint32)],
                        (np.arange(args.many_rows) % 64).astype(np.uint32),
                        64, 1)
            g.sweep(0, args.many_rows, args.many_rows, 7)
            len(g)
            engines.append(g)
        states = np.arange(1, args.many + 1, dtype=np.uint32)

        def reset():
            for g in engines:
                g.set_shared(0, engine.dd_shared([0.5] * dim))

        def singles():
            return [g.sample_hypers_pass(0, grid_values, int(s))[1]
                    for g, s in zip(engines, states)]

        def together():
            return engine.sample_hypers_pass_many(engines, 0, grid_values,
                                                  states)[1]

        singles()
        reset()
        together()
        reset()
        t_one, t_many = [], []
        for r in range(args.repeats):
            t, a = timed(singles)
            t_one.append(t)
            reset()
            t, b = timed(together)
            t_many.append(t)
            reset()
            assert list(a) == list(b)
        many = {"engines": args.many, "rows": args.many_rows,
                "groups": [len(engines[0]), len(engines[-1])],
                "single_passes_ms": [round(1e3 * t, 3) for t in t_one],
                "pass_many_ms": [round(1e3 * t, 3) for t in t_many]}
    chains, cands, launches, calls = gpu.hyper_stats()
    print(json.dumps({
        "shape": {"rows": n, "groups": len(gpu), "dim": dim,
                  "grid": args.grid, "batch": args.batch},
        "engine_pass_ms": [round(1e3 * t, 3) for t in t_engine],
        "pass_ms": [round(1e3 * t, 3) for t in t_pass],
        "hyper_stats_engine_pass": stats_engine,
        "hyper_stats_pass": stats_pass,
        "many": many,
        "parent_pass_ms": [round(1e3 * t, 3) for t in t_parent],
        "parent_pull_groups_ms": [round(1e3 * t, 3) for t in t_pull],
        "candidate_structs_ms": round(1e3 * t_build, 3),
        "sweep_ms": [round(1e3 * t, 3) for t in t_sweep],
        "hyper_stats": {"chains": chains, "candidates": cands,
                        "launches": launches, "calls": calls}}))


if __name__ == "__main__":
    main()
