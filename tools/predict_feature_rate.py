#!/usr/bin/env python3
"""(row, candidate) pairs per second of dist_gibbs_predict_feature_dev against
the only route there was before it, on one MI355X.  A tool, not part of
bench.py.

Shapes: PitmanYor(1, 0.2), K = 1024 + 1 empty, rows generated on the device
from a seed, initial assignment i mod K; the queries are the first --queries
resident rows' own values, everything but the target observed.
  mixed   the bench's mixed rows DD(16) + DD(4) + BetaBernoulli + GammaPoisson
          + NormalInverseChiSq, target the DD(16) column, its 16 values
  c2      DirichletDiscrete dim 256 alone, target that column, 256 values

  A       one predict_torch call per candidate on the rows completed with it
          (C calls; no `base`)
  B       predict_feature_dev, joint and base, the staged kernel
  B2      the same with DIST_PREDICT_FEATURE_RECOMPUTE

Each repetition times A, B and B2 in turn (alternating, one process, one box)
with a host clock around calls that end in a device synchronise; all routes
are warmed first.  Medians, spread (min .. max) and the ratios are printed, one
JSON line per shape last.  A's column c and B's joint[:, c] are compared bit
for bit.

    python tools/predict_feature_rate.py [--reps 7] [--shapes mixed,c2]
    rocprofv3 --kernel-trace --stats -d DIR -- \\
        python tools/predict_feature_rate.py --reps 1    # kernel times, in a
                                                         # run of its own
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(shape, n, k, dev, torch, engine):
    gen = torch.Generator(device=dev)
    gen.manual_seed(20240601)

    def categorical(dim):
        return torch.randint(0, dim, (n,), generator=gen, device=dev,
                             dtype=torch.int32)

    if shape == "c2":
        cols = [categorical(256)]
        shareds = [engine.dd_shared([0.5] * 256)]
        dim = 256
    else:
        rate = torch.full((n,), 5.0, device=dev)
        cols = [categorical(16), categorical(4),
                (torch.rand((n,), generator=gen, device=dev) < 0.3).to(
                    torch.int32),
                torch.poisson(rate, generator=gen).to(torch.int32),
                torch.randn((n,), generator=gen, device=dev)]
        shareds = [engine.dd_shared([0.5] * 16), engine.dd_shared([0.5] * 4),
                   engine.bb_shared(0.5, 2.0), engine.gp_shared(1.0, 1.0),
                   engine.nich_shared(0.0, 1.0, 1.0, 1.0)]
        dim = 16
    assign = (torch.arange(n, device=dev, dtype=torch.int64) % k).to(
        torch.int32)
    gpu = engine.Gibbs(1.0, 0.2, shareds)
    gpu.load_rows_torch(cols, assign, k, 1)
    return gpu, cols, dim


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--queries-mixed", type=int, default=100000)
    ap.add_argument("--queries-c2", type=int, default=10000)
    ap.add_argument("--rows", type=int, default=2000000,
                    help="resident rows (the statistics the groups hold)")
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="mixed,c2")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("predict_feature_rate.py: no GPU; nothing is "
                         "measured\n")
        return 2
    from distributions_amd import _core, engine
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        gpu, cols, C = make(shape, args.rows, args.groups, dev, torch, engine)
        nq = min(args.queries_c2 if shape == "c2" else args.queries_mixed,
                 args.rows)
        K = len(gpu)
        q = [c[:nq].contiguous() for c in cols]
        filled = [torch.full((nq,), v, dtype=torch.int32, device=dev)
                  for v in range(C)]
        out_a = torch.empty((C, nq), dtype=torch.float32, device=dev)
        joint = torch.empty((nq, C), dtype=torch.float32, device=dev)
        base = torch.empty(nq, dtype=torch.float32, device=dev)
        ptrs = [0] + [int(c.data_ptr()) for c in q[1:]]
        torch.cuda.synchronize()

        def route_a():
            for v in range(C):
                logp, _, _ = gpu.predict_torch([filled[v]] + q[1:], None)
                out_a[v] = logp
            torch.cuda.synchronize()

        def feature(flags):
            gpu.core.predict_feature_dev(ptrs, nq, 0, 0, None,
                                         int(joint.data_ptr()),
                                         int(base.data_ptr()), 0, 1, 1, 0,
                                         flags)

        def route_b():
            feature(0)

        def route_b2():
            feature(_core.PREDICT_FEATURE_RECOMPUTE)

        routes = [("A", route_a), ("B", route_b), ("B2", route_b2)]
        same = {}
        for name, fn in routes:     # warm: code objects, allocator, tables
            fn()
            fn()
            torch.cuda.synchronize()
            if name != "A":
                same[name] = bool(torch.equal(
                    joint.view(torch.int32), out_a.t().view(torch.int32)))
                joint.zero_()
        times = {name: [] for name, _ in routes}
        for _ in range(args.reps):
            for name, fn in routes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[name].append(time.perf_counter() - t0)
        res = dict(shape=shape, K=K, queries=nq, candidates=C,
                   joint_bits_equal_A=same)
        pairs = nq * C
        for name, _ in routes:
            t = times[name]
            med = statistics.median(t)
            res[name] = dict(ms_median=1e3 * med, ms_min=1e3 * min(t),
                             ms_max=1e3 * max(t), pairs_per_s=pairs / med)
            print("%s %-3s %9.3f ms (min %.3f .. max %.3f)  %.3e pairs/s" % (
                shape, name, 1e3 * med, 1e3 * min(t), 1e3 * max(t),
                pairs / med))
        res["A_over_B"] = res["A"]["ms_median"] / res["B"]["ms_median"]
        res["B2_over_B"] = res["B2"]["ms_median"] / res["B"]["ms_median"]
        print("%s time A / time B = %.3f, time B2 / time B = %.3f; joint bits "
              "equal to A's: %s" % (shape, res["A_over_B"], res["B2_over_B"],
                                    same))
        print(json.dumps(res))
        del gpu
    return 0


if __name__ == "__main__":
    sys.exit(main())
