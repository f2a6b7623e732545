#!/usr/bin/env python3
"""Held-out rows against M engines: dist_gibbs_predict_many_dev against the
only route there was before it, on one MI355X.  A tool, not part of bench.py.

Shapes (every member PitmanYor(1, 0.2), K = 1024 + 1 empty, its own rows
generated on the device from its own seed, initial assignment i mod K):
  i    M = 8,   10^6 queries,   DirichletDiscrete dim 256
  ii   M = 512, 4096 queries,   DirichletDiscrete dim 256, 20 000 rows per
       member: the shape of bench.py's exact chains
  iii  M = 64,  65 536 queries, GammaPoisson + NormalInverseChiSq

  A           M calls of Gibbs.predict_torch (logp only), torch.stack, then
              torch.logsumexp(dim=0) - log M
  B           predict_many_torch, logp only
  B_draw      predict_many_torch, logp, member and group: the group drawn in
              the chosen member only (the default)
  B_draw_all  the same with PREDICT_MANY_DRAW_ALL: every member draws, the
              fold selects

Each repetition times the routes in turn (alternating, one process, one box)
with a host clock around calls that end in a device synchronise; all routes
are warmed first.  Medians, spread (min .. max) and the ratio A / B are
printed, one JSON line per shape last.  A's logsumexp does not keep the
reference's float order; the largest |A - B| is reported beside the times.

    python tools/predict_many_rate.py [--shapes i,ii,iii] [--reps 7]
    rocprofv3 --kernel-trace --stats -d DIR -- python \\
        tools/predict_many_rate.py --reps 1 --shapes ii   # kernel times and
                                        # launch counts, in a run of its own
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"i": ("dd", 8, 1000000), "ii": ("dd", 512, 4096),
          "iii": ("gp_nich", 64, 65536)}


def columns(kind, n, seed, dev, torch):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    if kind == "dd":
        return [torch.randint(0, 256, (n,), generator=gen, device=dev,
                              dtype=torch.int32)]
    rate = torch.full((n,), 5.0, device=dev)
    return [torch.poisson(rate, generator=gen).to(torch.int32),
            torch.randn((n,), generator=gen, device=dev)]


def member(kind, n, k, seed, dev, torch, engine):
    if kind == "dd":
        shareds = [engine.dd_shared([0.5] * 256)]
    else:
        shareds = [engine.gp_shared(1.0, 1.0),
                   engine.nich_shared(0.0, 1.0, 1.0, 1.0)]
    assign = (torch.arange(n, device=dev, dtype=torch.int64) % k).to(
        torch.int32)
    gpu = engine.Gibbs(1.0, 0.2, shareds)
    gpu.load_rows_torch(columns(kind, n, seed, dev, torch), assign, k, 1)
    return gpu


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="i,ii,iii")
    ap.add_argument("--rows", type=int, default=20000,
                    help="resident rows per member")
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("predict_many_rate.py: no GPU; nothing is "
                         "measured\n")
        return 2
    from distributions_amd import engine
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        kind, M, nq = SHAPES[shape]
        gpus = [member(kind, args.rows, args.groups, 1000 + e, dev, torch,
                       engine) for e in range(M)]
        cols = columns(kind, nq, 7, dev, torch)
        torch.cuda.synchronize()
        out = {}

        def route_a():
            planes = torch.stack([g.predict_torch(cols, None)[0]
                                  for g in gpus])
            out["A"] = torch.logsumexp(planes, dim=0) - math.log(M)
            torch.cuda.synchronize()

        def route_b():
            out["B"] = engine.predict_many_torch(gpus, cols, None)[0]

        def route_b_draw():
            out["B_draw"] = engine.predict_many_torch(gpus, cols, "sample",
                                                      seed=1)

        def route_b_draw_all():
            out["B_draw_all"] = engine.predict_many_torch(
                gpus, cols, "sample", seed=1,
                flags=engine.PREDICT_MANY_DRAW_ALL)

        routes = [("A", route_a), ("B", route_b), ("B_draw", route_b_draw),
                  ("B_draw_all", route_b_draw_all)]
        for _, fn in routes:        # warm: code objects, allocator, tables
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in routes}
        for _ in range(args.reps):
            for name, fn in routes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[name].append(time.perf_counter() - t0)
        diff = float((out["A"] - out["B"]).abs().max().item())
        same = all(bool(torch.equal(a, b)) for a, b in
                   zip(out["B_draw"][:3], out["B_draw_all"][:3]))
        res = dict(shape=shape, kind=kind, M=M, K=len(gpus[0]), queries=nq,
                   max_abs_A_minus_B=diff, draw_forms_equal=same)
        for name, _ in routes:
            t = times[name]
            med = statistics.median(t)
            res[name] = dict(ms_median=1e3 * med, ms_min=1e3 * min(t),
                             ms_max=1e3 * max(t))
            print("%-3s %-10s %9.3f ms (min %.3f .. max %.3f)" % (
                shape, name, 1e3 * med, 1e3 * min(t), 1e3 * max(t)))
        res["A_over_B"] = res["A"]["ms_median"] / res["B"]["ms_median"]
        res["draw_all_over_draw"] = (res["B_draw_all"]["ms_median"]
                                     / res["B_draw"]["ms_median"])
        print("%s time A / time B = %.3f (B %s); max |A - B| = %.2e; "
              "time B_draw_all / time B_draw = %.3f; the draw forms' bits %s"
              % (shape, res["A_over_B"],
                 "not slower" if res["A_over_B"] >= 1.0 else "SLOWER", diff,
                 res["draw_all_over_draw"],
                 "are equal" if same else "DIFFER"))
        print(json.dumps(res))
        del gpus, out
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
