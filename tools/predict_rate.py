#!/usr/bin/env python3
"""Held-out rows per second: dist_gibbs_predict_dev against the only route
there was before it, on one MI355X.  A tool, not part of bench.py.

Shapes (BASELINE): C2 = DirichletDiscrete dim 256, K = 1024 + 1 empty;
C3 = GammaPoisson + NormalInverseChiSq, K = 1024 + 1 empty; PitmanYor(1, 0.2),
rows generated on the device from a seed, initial assignment i mod K.  The
queries are the first --queries resident rows' own values, so every route does
the same arithmetic.

  A       dist_gibbs_score_rows_dev into the largest chunk of whole rows whose
          chunk x K float matrix fits a fixed 1 GiB buffer, then
          torch.logsumexp(dim=1) per chunk
  B       dist_gibbs_predict_dev, logp only
  B_draw  dist_gibbs_predict_dev, logp and the drawn group

Each repetition times A, B and B_draw in turn (alternating, one process, one
box) with a host clock around calls that end in a device synchronise; all
routes are warmed first.  Medians, spread (min .. max) and the ratio A / B are
printed, one JSON line per shape last.  A's logsumexp does not keep the
reference's float order; the largest |A - B| is reported beside the rates.

    python tools/predict_rate.py [--queries 1000000] [--reps 7]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/predict_rate.py \\
        --reps 1 --shapes c2           # kernel times, in a run of its own
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
    if shape == "c2":
        cols = [torch.randint(0, 256, (n,), generator=gen, device=dev,
                              dtype=torch.int32)]
        shareds = [engine.dd_shared([0.5] * 256)]
    else:
        rate = torch.full((n,), 5.0, device=dev)
        cols = [torch.poisson(rate, generator=gen).to(torch.int32),
                torch.randn((n,), generator=gen, device=dev)]
        shareds = [engine.gp_shared(1.0, 1.0),
                   engine.nich_shared(0.0, 1.0, 1.0, 1.0)]
    assign = (torch.arange(n, device=dev, dtype=torch.int64) % k).to(
        torch.int32)
    gpu = engine.Gibbs(1.0, 0.2, shareds)
    gpu.load_rows_torch(cols, assign, k, 1)
    return gpu, cols


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--queries", type=int, default=1000000)
    ap.add_argument("--rows", type=int, default=2000000,
                    help="resident rows (the statistics the groups hold)")
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--buffer-bytes", type=int, default=1 << 30)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("predict_rate.py: no GPU; nothing is measured\n")
        return 2
    from distributions_amd import engine
    dev = torch.device("cuda", 0)
    nq = min(args.queries, args.rows)
    for shape in args.shapes.split(","):
        gpu, cols = make(shape, args.rows, args.groups, dev, torch, engine)
        K = len(gpu)
        chunk = max(1, args.buffer_bytes // (4 * K))
        buf = torch.empty((min(chunk, nq), K), dtype=torch.float32, device=dev)
        out_a = torch.empty(nq, dtype=torch.float32, device=dev)
        out_b = torch.empty(nq, dtype=torch.float32, device=dev)
        group = torch.empty(nq, dtype=torch.int32, device=dev)
        ptrs = [int(c.data_ptr()) for c in cols]

        def route_a():
            for r0 in range(0, nq, chunk):
                r1 = min(nq, r0 + chunk)
                gpu.core.score_rows_dev(r0, r1, int(buf.data_ptr()), K)
                torch.logsumexp(buf[:r1 - r0], dim=1, out=out_a[r0:r1])
                # (the library writes the next chunk on its own stream)
                torch.cuda.synchronize()

        def route_b():
            gpu.core.predict_dev(ptrs, nq, int(out_b.data_ptr()), 0, 0, 1, 0)

        def route_b_draw():
            gpu.core.predict_dev(ptrs, nq, int(out_b.data_ptr()),
                                 int(group.data_ptr()), 0, 1, 0)

        routes = [("A", route_a), ("B", route_b), ("B_draw", route_b_draw)]
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
        diff = float((out_a - out_b).abs().max().item())
        res = dict(shape=shape, K=K, queries=nq, rows_per_chunk_A=chunk,
                   max_abs_A_minus_B=diff)
        for name, _ in routes:
            t = times[name]
            med = statistics.median(t)
            res[name] = dict(ms_median=1e3 * med, ms_min=1e3 * min(t),
                             ms_max=1e3 * max(t), rows_per_s=nq / med)
            print("%s %-6s %9.3f ms (min %.3f .. max %.3f)  %.3e rows/s" % (
                shape, name, 1e3 * med, 1e3 * min(t), 1e3 * max(t), nq / med))
        res["A_over_B"] = res["A"]["ms_median"] / res["B"]["ms_median"]
        print("%s time A / time B = %.3f (B %s); max |A - B| = %.2e" % (
            shape, res["A_over_B"],
            "not slower" if res["A_over_B"] >= 1.0 else "SLOWER", diff))
        print(json.dumps(res))
        del gpu, buf
    return 0


if __name__ == "__main__":
    sys.exit(main())
