#!/usr/bin/env python3
"""One feature's predictive averaged over M engines:
dist_gibbs_predict_feature_many_dev against the only route there was before
it, on one MI355X.  A tool, not part of bench.py.

Shapes (every member PitmanYor(1, 0.2), K = 1024 + 1 empty, its own rows
generated on the device from its own seed, initial assignment i mod K;
everything but the target observed):
  i    M = 8,   10^5 queries, the bench's mixed rows DD(16) + DD(4) +
       BetaBernoulli + GammaPoisson + NormalInverseChiSq, target the DD(16)
       column, its 16 values
  ii   M = 512, 256 queries x 256 candidates, DirichletDiscrete dim 256 alone
  iii  M = 64,  65 536 queries, GammaPoisson + NormalInverseChiSq, target the
       GammaPoisson column, the counts 0, 1, 2, 5, 9, 40, 300

  A    M calls of Gibbs.predict_feature_torch (joint and base), torch.stack,
       then torch.logsumexp(dim=0) - log M on joint and on base
  B    predict_feature_many_torch, joint and base (B_members: with the planes,
       timed apart, for the comparison of the members' bits)

Each repetition times the routes in turn (alternating, one process, one box)
with a host clock around calls that end in a device synchronise; all routes
are warmed first.  Medians, spread (min .. max) and the ratio A / B are
printed, one JSON line per shape last.  A's members' joints and B's
members_joint are compared bit for bit; A's logsumexp does not keep the
reference's float order, and the largest |A - B| on the folded values is
reported beside the times.

    python tools/predict_feature_many_rate.py [--shapes i,ii,iii] [--reps 7]
    rocprofv3 --kernel-trace --stats -d DIR -- python \\
        tools/predict_feature_many_rate.py --reps 1 --shapes ii   # kernel
                              # times and launch counts, in a run of its own
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

COUNT_CANDIDATES = [0, 1, 2, 5, 9, 40, 300]
# kind, M, queries, candidates (None: the target's whole domain)
SHAPES = {"i": ("mixed", 8, 100000, None), "ii": ("dd", 512, 256, None),
          "iii": ("gp_nich", 64, 65536, COUNT_CANDIDATES)}


def columns(kind, n, seed, dev, torch):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)

    def categorical(dim):
        return torch.randint(0, dim, (n,), generator=gen, device=dev,
                             dtype=torch.int32)

    if kind == "dd":
        return [categorical(256)]
    rate = torch.full((n,), 5.0, device=dev)
    if kind == "gp_nich":
        return [torch.poisson(rate, generator=gen).to(torch.int32),
                torch.randn((n,), generator=gen, device=dev)]
    return [categorical(16), categorical(4),
            (torch.rand((n,), generator=gen, device=dev) < 0.3).to(
                torch.int32),
            torch.poisson(rate, generator=gen).to(torch.int32),
            torch.randn((n,), generator=gen, device=dev)]


def member(kind, n, k, seed, dev, torch, engine):
    if kind == "dd":
        shareds = [engine.dd_shared([0.5] * 256)]
    elif kind == "gp_nich":
        shareds = [engine.gp_shared(1.0, 1.0),
                   engine.nich_shared(0.0, 1.0, 1.0, 1.0)]
    else:
        shareds = [engine.dd_shared([0.5] * 16), engine.dd_shared([0.5] * 4),
                   engine.bb_shared(0.5, 2.0), engine.gp_shared(1.0, 1.0),
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
        sys.stderr.write("predict_feature_many_rate.py: no GPU; nothing is "
                         "measured\n")
        return 2
    from distributions_amd import engine
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        kind, M, nq, cand = SHAPES[shape]
        gpus = [member(kind, args.rows, args.groups, 1000 + e, dev, torch,
                       engine) for e in range(M)]
        cols = columns(kind, nq, 7, dev, torch)
        if len(cols) > 1:
            cols[0] = None      # the target's column is not read
        torch.cuda.synchronize()
        out = {}

        def route_a():
            per = [g.predict_feature_torch(cols, 0, cand, None, None)
                   for g in gpus]
            pj = torch.stack([p[0] for p in per])
            pb = torch.stack([p[1] for p in per])
            out["A"] = (torch.logsumexp(pj, dim=0) - math.log(M),
                        torch.logsumexp(pb, dim=0) - math.log(M), pj)
            torch.cuda.synchronize()

        def route_b():
            out["B"] = engine.predict_feature_many_torch(gpus, cols, 0, cand,
                                                         None, None)

        def route_b_members():
            out["B_members"] = engine.predict_feature_many_torch(
                gpus, cols, 0, cand, None, None, members=True)

        routes = [("A", route_a), ("B", route_b),
                  ("B_members", route_b_members)]
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
        diff_j = float((out["A"][0] - out["B"][0]).abs().max().item())
        diff_b = float((out["A"][1] - out["B"][1]).abs().max().item())
        same = bool(torch.equal(out["A"][2].view(torch.int32),
                                out["B_members"][4].view(torch.int32)))
        C = int(out["B"][0].shape[1])
        res = dict(shape=shape, kind=kind, M=M, K=len(gpus[0]), queries=nq,
                   candidates=C, max_abs_A_minus_B_joint=diff_j,
                   max_abs_A_minus_B_base=diff_b, members_joint_equal=same)
        for name, _ in routes:
            t = times[name]
            med = statistics.median(t)
            res[name] = dict(ms_median=1e3 * med, ms_min=1e3 * min(t),
                             ms_max=1e3 * max(t))
            print("%-3s %-10s %9.3f ms (min %.3f .. max %.3f)" % (
                shape, name, 1e3 * med, 1e3 * min(t), 1e3 * max(t)))
        res["A_over_B"] = res["A"]["ms_median"] / res["B"]["ms_median"]
        print("%s time A / time B = %.3f (B %s); max |A - B| = %.2e (joint), "
              "%.2e (base); the members' joint bits %s" % (
                  shape, res["A_over_B"],
                  "not slower" if res["A_over_B"] >= 1.0 else "SLOWER",
                  diff_j, diff_b, "are equal" if same else "DIFFER"))
        print(json.dumps(res))
        del gpus, out
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
