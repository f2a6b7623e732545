#!/usr/bin/env python3
"""Co-assignment of row pairs over M engines: dist_gibbs_coassign_many_dev
against what could be composed before it, on one MI355X.  A tool, not part of
bench.py.

Shapes (every member PitmanYor(1, 0.2), K = 1024 + 1 empty, the SAME 20 000
rows in every member -- route A can only score rows that are resident --,
initial assignment (i + 37 e) mod K in member e), n = 8192 rows against
themselves, M = 1 and M = 8:
  dd       DirichletDiscrete dim 256
  gp_nich  GammaPoisson + NormalInverseChiSq

  A   per engine: score_rows_dev of the resident rows [0, n) into an n x K
      matrix, torch.softmax over K, W @ W.T; then the mean over the engines
      (eight n x K matrices through HBM and 3 launches per engine at M = 8)
  B   coassign_many_torch on the same rows' values

Each repetition times the routes in turn (alternating, one process, one box)
with a host clock around calls that end in a device synchronise; both routes
are warmed first.  Medians and spread (min .. max) of --reps repetitions, the
largest |A - B| (A has other bits: score_rows scores rows that are IN the
table, and the softmax and the product keep no float order), and whether B's
median is within A's median plus A's own spread.
One JSON line per shape and M; everything is also written to --out.

    python tools/coassign_rate.py [--shapes dd,gp_nich] [--members 1,8]
    rocprofv3 --kernel-trace --stats -d DIR -- python \\
        tools/coassign_rate.py --reps 1 --shapes dd --members 8 --out none
                        # k_coassign_gemm's time, in a run of its own: its
                        # rate is 2 n^2 sum_e K2_e FLOP over that time
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def columns(kind, n, seed, dev, torch):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    if kind == "dd":
        return [torch.randint(0, 256, (n,), generator=gen, device=dev,
                              dtype=torch.int32)]
    rate = torch.full((n,), 5.0, device=dev)
    return [torch.poisson(rate, generator=gen).to(torch.int32),
            torch.randn((n,), generator=gen, device=dev)]


def member(kind, cols, k, e, dev, torch, engine):
    if kind == "dd":
        shareds = [engine.dd_shared([0.5] * 256)]
    else:
        shareds = [engine.gp_shared(1.0, 1.0),
                   engine.nich_shared(0.0, 1.0, 1.0, 1.0)]
    n = int(cols[0].numel())
    assign = ((torch.arange(n, device=dev, dtype=torch.int64) + 37 * e)
              % k).to(torch.int32)
    gpu = engine.Gibbs(1.0, 0.2, shareds)
    gpu.load_rows_torch([c.clone() for c in cols], assign, k, 1)
    return gpu


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="dd,gp_nich")
    ap.add_argument("--members", default="1,8")
    ap.add_argument("--rows", type=int, default=20000,
                    help="resident rows per member")
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "coassign_rate.txt"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("coassign_rate.py: no GPU; nothing is measured\n")
        return 2
    from distributions_amd import engine
    dev = torch.device("cuda", 0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    n = args.n
    for kind in args.shapes.split(","):
        cols = columns(kind, args.rows, 1000, dev, torch)
        most = max(int(m) for m in args.members.split(","))
        every = [member(kind, cols, args.groups, e, dev, torch, engine)
                 for e in range(most)]
        query = [c[:n].contiguous() for c in cols]
        for M in (int(m) for m in args.members.split(",")):
            gpus = every[:M]
            K = len(gpus[0])
            scores = torch.empty((n, K), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            out = {}

            def route_a():
                acc = None
                for g in gpus:
                    g.core.score_rows_dev(0, n, int(scores.data_ptr()), K)
                    w = torch.softmax(scores, dim=1)
                    c = w @ w.T
                    acc = c if acc is None else acc + c
                out["A"] = acc / M
                torch.cuda.synchronize()

            def route_b():
                out["B"] = engine.coassign_many_torch(gpus, query)

            routes = [("A", route_a), ("B", route_b)]
            for _, fn in routes:    # warm: code objects, allocator, tables
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
            sym = bool(torch.equal(out["B"], out["B"].T))
            k2 = sum((len(g) + 1) // 2 * 2 for g in gpus)
            res = dict(kind=kind, M=M, K=K, n=n, max_abs_A_minus_B=diff,
                       B_symmetric=sym, gemm_flop=2.0 * n * n * k2)
            for name, _ in routes:
                t = times[name]
                med = statistics.median(t)
                res[name] = dict(ms_median=1e3 * med, ms_min=1e3 * min(t),
                                 ms_max=1e3 * max(t))
                say("%-7s M=%d %s %9.3f ms (min %.3f .. max %.3f)" % (
                    kind, M, name, 1e3 * med, 1e3 * min(t), 1e3 * max(t)))
            a, b = res["A"], res["B"]
            res["A_over_B"] = a["ms_median"] / b["ms_median"]
            res["B_within_A_plus_spread"] = (
                b["ms_median"] <= a["ms_median"] + a["ms_max"] - a["ms_min"])
            say("%-7s M=%d time A / time B = %.3f; B's median %s A's median "
                "plus A's spread; max |A - B| = %.2e; B %s its transpose"
                % (kind, M, res["A_over_B"],
                   "is within" if res["B_within_A_plus_spread"]
                   else "is NOT within", diff,
                   "equals" if sym else "DIFFERS FROM"))
            say(json.dumps(res))
            del out, scores
            torch.cuda.empty_cache()
        del every
        torch.cuda.empty_cache()
    if args.out != "none":
        with open(args.out, "w") as f:
            f.write("tools/coassign_rate.py --shapes %s --members %s --n %d "
                    "--rows %d --groups %d --reps %d\n"
                    % (args.shapes, args.members, args.n, args.rows,
                       args.groups, args.reps))
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
