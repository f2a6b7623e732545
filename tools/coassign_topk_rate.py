#!/usr/bin/env python3
"""Per query the k most co-assigned targets over M engines:
dist_gibbs_coassign_topk_many_dev against what could be composed before it, on
one MI355X.  A tool, not part of bench.py.

Members as tools/coassign_rate.py's (PitmanYor(1, 0.2), K = 1024 + 1 empty,
20 000 rows; dd: DirichletDiscrete dim 256, gp_nich: GammaPoisson +
NormalInverseChiSq), M = 1 and M = 8, k = 16:
  self    n = 8192 rows against themselves, self excluded
  search  256 queries against all 20 000 rows

  A   coassign_many_torch, the diagonal set to -1 where self is excluded,
      torch.topk(k) on the matrix (4 n_q n_t bytes of result)
  B   coassign_topk_many_torch (8 k n_q bytes of running keys and the
      candidate keys of one launch, 8 k n_q ceil(n_t / 128) bytes; the
      shapes here take one launch)

Each repetition times the routes in turn (alternating, one process, one box)
with a host clock around calls that end in a device synchronise; both routes
are warmed first.  Medians and spread (min .. max) of --reps repetitions, and
whether B's median is within A's median plus A's own spread.  Checked: the
sorted values of A and B are bit-equal, and B's targets hold B's values in A's
matrix (the indices may differ at ties only: torch.topk's tie order is
unspecified).
One JSON line per shape, members and M; everything is also written to --out.

    python tools/coassign_topk_rate.py [--shapes dd,gp_nich] [--members 1,8]
    rocprofv3 --kernel-trace --stats -d DIR -- python \\
        tools/coassign_topk_rate.py --reps 1 --members 1 --out none
                        # k_coassign_topk, k_coassign_topk_merge and
                        # k_coassign_gemm's times, in a run of its own
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from coassign_rate import columns, member  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="dd,gp_nich")
    ap.add_argument("--cases", default="self,search")
    ap.add_argument("--members", default="1,8")
    ap.add_argument("--rows", type=int, default=20000,
                    help="resident rows per member, and the search's targets")
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("-k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "coassign_topk_rate.txt"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("coassign_topk_rate.py: no GPU; nothing is "
                         "measured\n")
        return 2
    from distributions_amd import engine
    dev = torch.device("cuda", 0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    k = args.k
    for kind in args.shapes.split(","):
        cols = columns(kind, args.rows, 1000, dev, torch)
        most = max(int(m) for m in args.members.split(","))
        every = [member(kind, cols, args.groups, e, dev, torch, engine)
                 for e in range(most)]
        for case in args.cases.split(","):
            if case == "self":
                query = [c[:args.n].contiguous() for c in cols]
                other, n_q, n_t = None, args.n, args.n
            else:
                query = [c[:args.queries].contiguous() for c in cols]
                other, n_q, n_t = cols, args.queries, args.rows
            tiles = (n_t + 127) // 128
            bytes_a = 4 * n_q * n_t
            bytes_b = 8 * k * n_q + 8 * k * n_q * tiles
            for M in (int(m) for m in args.members.split(",")):
                gpus = every[:M]
                out = {}

                def route_a():
                    c = engine.coassign_many_torch(gpus, query, other)
                    out["matrix"] = c
                    if other is None:
                        c = c.clone()
                        c.fill_diagonal_(-1.0)
                    out["A"] = torch.topk(c, k, dim=1)
                    torch.cuda.synchronize()

                def route_b():
                    out["B"] = engine.coassign_topk_many_torch(
                        gpus, query, other, k)

                routes = [("A", route_a), ("B", route_b)]
                for _, fn in routes:    # warm: code objects, allocator
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
                index_b, prob_b = out["B"]
                values_equal = bool(torch.equal(
                    out["A"].values.view(torch.int32),
                    prob_b.view(torch.int32)))
                held = torch.gather(out["matrix"], 1, index_b.long())
                targets_hold = bool(torch.equal(held.view(torch.int32),
                                                prob_b.view(torch.int32)))
                index_differs = int(
                    (out["A"].indices != index_b.long()).sum().item())
                res = dict(kind=kind, case=case, M=M, n_q=n_q, n_t=n_t, k=k,
                           values_bit_equal=values_equal,
                           B_targets_hold_B_values=targets_hold,
                           indices_that_differ=index_differs,
                           result_bytes_A=bytes_a, result_bytes_B=bytes_b)
                what = "%-7s %-6s M=%d" % (kind, case, M)
                for name, _ in routes:
                    t = times[name]
                    med = statistics.median(t)
                    res[name] = dict(ms_median=1e3 * med, ms_min=1e3 * min(t),
                                     ms_max=1e3 * max(t))
                    say("%s %s %9.3f ms (min %.3f .. max %.3f)" % (
                        what, name, 1e3 * med, 1e3 * min(t), 1e3 * max(t)))
                a, b = res["A"], res["B"]
                res["A_over_B"] = a["ms_median"] / b["ms_median"]
                res["B_within_A_plus_spread"] = (
                    b["ms_median"]
                    <= a["ms_median"] + a["ms_max"] - a["ms_min"])
                say("%s time A / time B = %.3f; B's median %s A's median plus "
                    "A's spread; values %s; B's targets %s; %d indices differ "
                    "(ties); result bytes A %d, B %d"
                    % (what, res["A_over_B"],
                       "is within" if res["B_within_A_plus_spread"]
                       else "is NOT within",
                       "bit-equal" if values_equal else "DIFFER",
                       "hold their values" if targets_hold
                       else "DO NOT HOLD THEIR VALUES", index_differs,
                       bytes_a, bytes_b))
                say(json.dumps(res))
                del out
                torch.cuda.empty_cache()
        del every
        torch.cuda.empty_cache()
    if args.out != "none":
        with open(args.out, "w") as f:
            f.write("tools/coassign_topk_rate.py --shapes %s --cases %s "
                    "--members %s --n %d --queries %d --rows %d --groups %d "
                    "-k %d --reps %d\n"
                    % (args.shapes, args.cases, args.members, args.n,
                       args.queries, args.rows, args.groups, args.k,
                       args.reps))
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
