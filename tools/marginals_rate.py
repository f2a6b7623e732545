#!/usr/bin/env python3
"""Log marginals of feature subsets over M engines:
dist_gibbs_marginals_many_dev against the only route there was before it, on
one MI355X.  A tool, not part of bench.py.

Shapes (every member PitmanYor(1, 0.2), K = 1024 + 1 empty, its own rows
generated on the device from its own seed, initial assignment i mod K; M = 8,
10^5 query rows):
  i    the bench's mixed rows DD(16) + DD(4) + BetaBernoulli + GammaPoisson +
       NormalInverseChiSq; the masks are the 5 singles and the 10 pairs
  ii   DirichletDiscrete dim 256 alone; the single mask (staging saves nothing
       there)

  A    one predict_feature_many_torch(..., mode=None) call per mask with the
       mask as every row's `observed` and a target outside it, taking `base`;
       predict_many_torch where no target is free
  B    one marginals_many_torch

A's columns are first held to B's bit for bit.  Then each repetition times the
routes in turn (alternating, one process, one box) with a host clock around
calls that end in a device synchronise; both routes are warmed first.
Medians, spread (min .. max) and the ratio A / B are printed, one JSON line
per shape last.

    python tools/marginals_rate.py [--shapes i,ii] [--reps 7]
    rocprofv3 --kernel-trace --stats -d DIR -- python \\
        tools/marginals_rate.py --reps 1 --shapes i   # kernel times and
                                      # launch counts, in a run of its own
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# kind, M, queries
SHAPES = {"i": ("mixed", 8, 100000), "ii": ("dd", 8, 100000)}


def columns(kind, n, seed, dev, torch):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)

    def categorical(dim):
        return torch.randint(0, dim, (n,), generator=gen, device=dev,
                             dtype=torch.int32)

    if kind == "dd":
        return [categorical(256)]
    rate = torch.full((n,), 5.0, device=dev)
    return [categorical(16), categorical(4),
            (torch.rand((n,), generator=gen, device=dev) < 0.3).to(
                torch.int32),
            torch.poisson(rate, generator=gen).to(torch.int32),
            torch.randn((n,), generator=gen, device=dev)]


def member(kind, n, k, seed, dev, torch, engine):
    if kind == "dd":
        shareds = [engine.dd_shared([0.5] * 256)]
    else:
        shareds = [engine.dd_shared([0.5] * 16), engine.dd_shared([0.5] * 4),
                   engine.bb_shared(0.5, 2.0), engine.gp_shared(1.0, 1.0),
                   engine.nich_shared(0.0, 1.0, 1.0, 1.0)]
    assign = (torch.arange(n, device=dev, dtype=torch.int64) % k).to(
        torch.int32)
    gpu = engine.Gibbs(1.0, 0.2, shareds)
    gpu.load_rows_torch(columns(kind, n, seed, dev, torch), assign, k, 1)
    return gpu


def singles_and_pairs(F):
    m = [1 << i for i in range(F)]
    m += [(1 << i) | (1 << j) for i in range(F) for j in range(i + 1, F)]
    return m


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="i,ii")
    ap.add_argument("--rows", type=int, default=20000,
                    help="resident rows per member")
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--queries", type=int, default=0,
                    help="query rows (0: the shape's)")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("marginals_rate.py: no GPU; nothing is measured\n")
        return 2
    from distributions_amd import engine
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        kind, M, nq = SHAPES[shape]
        nq = args.queries or nq
        gpus = [member(kind, args.rows, args.groups, 1000 + e, dev, torch,
                       engine) for e in range(M)]
        cols = columns(kind, nq, 7, dev, torch)
        F = len(cols)
        masks = singles_and_pairs(F)
        full = (1 << F) - 1
        # one candidate of the target, which `base` leaves out anyway
        observed = {m: torch.full((nq,), m, dtype=torch.int32, device=dev)
                    for m in masks}
        torch.cuda.synchronize()
        out = {}

        def route_a():
            per = []
            for m in masks:
                if m == full:
                    per.append(engine.predict_many_torch(gpus, cols, None)[0])
                    continue
                target = next(t for t in range(F) if not (m >> t) & 1)
                per.append(engine.predict_feature_many_torch(
                    gpus, cols, target, [0], observed[m], None)[1])
            out["A"] = torch.stack(per, dim=1)
            torch.cuda.synchronize()

        def route_b():
            out["B"] = engine.marginals_many_torch(gpus, cols, masks)[0]

        routes = [("A", route_a), ("B", route_b)]
        for _, fn in routes:        # warm: code objects, allocator, tables
            fn()
            fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(out["A"].view(torch.int32),
                                out["B"].view(torch.int32)))
        if not same:
            sys.stderr.write("marginals_rate.py: shape %s: A's columns are "
                             "not B's bits; nothing is timed\n" % shape)
            return 1
        times = {name: [] for name, _ in routes}
        for _ in range(args.reps):
            for name, fn in routes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[name].append(time.perf_counter() - t0)
        res = dict(shape=shape, kind=kind, M=M, K=len(gpus[0]), queries=nq,
                   masks=len(masks), columns_equal=same)
        for name, _ in routes:
            t = times[name]
            med = statistics.median(t)
            res[name] = dict(ms_median=1e3 * med, ms_min=1e3 * min(t),
                             ms_max=1e3 * max(t))
            print("%-3s %-3s %9.3f ms (min %.3f .. max %.3f)" % (
                shape, name, 1e3 * med, 1e3 * min(t), 1e3 * max(t)))
        res["A_over_B"] = res["A"]["ms_median"] / res["B"]["ms_median"]
        # B is ahead (behind) only when the two spreads do not overlap
        if res["B"]["ms_max"] < res["A"]["ms_min"]:
            verdict = "B ahead beyond the spread"
        elif res["A"]["ms_max"] < res["B"]["ms_min"]:
            verdict = "B BEHIND beyond the spread"
        else:
            verdict = "within the spread"
        res["verdict"] = verdict
        print("%s time A / time B = %.3f (%s); %d masks, the columns' bits "
              "are equal" % (shape, res["A_over_B"], verdict, len(masks)))
        print(json.dumps(res))
        del gpus, out
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
