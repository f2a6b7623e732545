#!/usr/bin/env python3
"""Per query the k most co-assigned RESIDENT rows over M engines:
dist_gibbs_search_resident_many_dev and
dist_gibbs_coassign_resident_topk_many_dev against what could be composed
before them, on one MI355X.  A tool, not part of bench.py.

Members as tools/coassign_topk_rate.py builds them (PitmanYor(1, 0.2),
K = 1024 + 1 empty; dd: DirichletDiscrete dim 256, gp_nich: GammaPoisson +
NormalInverseChiSq) at N = 10^6 resident rows, M = 1 and M = 8, 256 queries,
k = 16:
  held_out  256 rows that are not in the table against all N resident rows
  resident  256 rows of the table against all N, self excluded

  A   held_out: responsibilities_torch per engine, an index-select of its
      [K, n_q] plane by the engine's translated labels, the sum over the
      engines, / M, torch.topk (4 n_q N bytes per engine and for the sum)
      resident: coassign_resident_many_torch against arange(N) in chunks of
      --chunk columns, the self cell set to -1, torch.topk per chunk and a
      final topk over the chunks' winners (4 n_q N bytes of cells)
  B   search_resident_many_torch / coassign_resident_topk_many_torch (8 k n_q
      bytes of running keys and 8 k n_q candidate keys per slice)

Each repetition times the routes in turn (alternating, one process, one box)
with a host clock around calls that end in a device synchronise; both routes
are warmed first.  Medians and spread (min .. max) of --reps repetitions, and
whether B's median is within A's median plus A's own spread.  Checked: the
sorted values of A and B are bit-equal in every row, and B's targets hold B's
values in A's cells (the indices may differ at ties only: torch.topk's tie
order is unspecified).
One JSON line per shape, case and M; everything is also written to --out.

    python tools/search_resident_rate.py [--shapes dd,gp_nich] [--members 1,8]
    rocprofv3 --kernel-trace --stats -d DIR -- python \\
        tools/search_resident_rate.py --reps 1 --members 8 --out none
                        # k_resident_topk's time, in a run of its own
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
    ap.add_argument("--cases", default="held_out,resident")
    ap.add_argument("--members", default="1,8")
    ap.add_argument("--rows", type=int, default=1000000,
                    help="resident rows per member: the targets")
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=1 << 18,
                    help="columns per chunk of route A's resident matrix")
    ap.add_argument("-k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "search_resident_rate.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("search_resident_rate.py: no GPU; nothing is "
                         "measured\n")
        return 2
    from distributions_amd import engine
    dev = torch.device("cuda", 0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    k, n, n_q = args.k, args.rows, args.queries
    for kind in args.shapes.split(","):
        cols = columns(kind, n, 1000, dev, torch)
        held = [c[:n_q].contiguous() for c in columns(kind, n_q, 977, dev,
                                                      torch)]
        most = max(int(m) for m in args.members.split(","))
        every = [member(kind, cols, args.groups, e, dev, torch, engine)
                 for e in range(most)]
        # the engines' labels as packed indices (set-up, not timed)
        slots = []
        for g in every:
            ids = g.assignments().astype(np.int64)
            g2p = np.full(int(ids.max()) + 1, -1, np.int64)
            for gid in np.unique(ids):
                g2p[gid] = g.core.global_to_packed(int(gid))
            slots.append(torch.from_numpy(g2p[ids]).to(dev))
        rows = torch.randint(0, n, (n_q,), device=dev, dtype=torch.int32,
                             generator=torch.Generator(device=dev)
                             .manual_seed(5))
        every_row = torch.arange(n, device=dev, dtype=torch.int32)
        for case in args.cases.split(","):
            for M in (int(m) for m in args.members.split(",")):
                gpus = every[:M]
                out = {}

                def route_a_held_out():
                    acc = None
                    for g, s in zip(gpus, slots):
                        plane = g.responsibilities_torch(held).t()
                        part = plane.index_select(0, s)        # [N, n_q]
                        acc = part if acc is None else acc + part
                    out["cells"] = acc / float(M)
                    top = torch.topk(out["cells"], k, dim=0)
                    out["A"] = top.values.t().contiguous()
                    torch.cuda.synchronize()

                def route_a_resident():
                    best = []
                    at = torch.arange(n_q, device=dev)
                    for c0 in range(0, n, args.chunk):
                        c1 = min(n, c0 + args.chunk)
                        cells = engine.coassign_resident_many_torch(
                            gpus, rows, every_row[c0:c1])
                        inside = (rows >= c0) & (rows < c1)
                        cells[at[inside], (rows[inside] - c0).long()] = -1.0
                        best.append(torch.topk(cells, min(k, c1 - c0),
                                               dim=1).values)
                    out["A"] = torch.topk(torch.cat(best, 1), k, dim=1).values
                    torch.cuda.synchronize()

                def route_b_held_out():
                    out["B"] = engine.search_resident_many_torch(gpus, held,
                                                                 k)

                def route_b_resident():
                    out["B"] = engine.coassign_resident_topk_many_torch(
                        gpus, rows, k, True)

                routes = ([("A", route_a_held_out), ("B", route_b_held_out)]
                          if case == "held_out" else
                          [("A", route_a_resident), ("B", route_b_resident)])
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
                    out["A"].view(torch.int32), prob_b.view(torch.int32)))
                if case == "held_out":
                    holds = torch.gather(out["cells"], 0, index_b.long().t()).t()
                    bytes_a = 4 * n_q * n * (M + 1)
                else:
                    pair = engine.coassign_resident_many_torch(
                        gpus, rows, index_b.reshape(-1))
                    holds = pair.reshape(n_q, n_q, k)[
                        torch.arange(n_q, device=dev),
                        torch.arange(n_q, device=dev)]
                    bytes_a = 4 * n_q * n
                targets_hold = bool(torch.equal(
                    holds.contiguous().view(torch.int32),
                    prob_b.view(torch.int32)))
                no_self = bool((index_b != rows[:, None]).all()) \
                    if case == "resident" else True
                bytes_b = 8 * k * n_q * 2
                res = dict(kind=kind, case=case, M=M, n_q=n_q, n_t=n, k=k,
                           values_bit_equal=values_equal,
                           B_targets_hold_B_values=targets_hold,
                           B_leaves_self_out=no_self,
                           bytes_written_A=bytes_a,
                           bytes_written_B_per_slice=bytes_b)
                what = "%-7s %-8s M=%d" % (kind, case, M)
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
                    "A's spread; values %s; B's targets %s; bytes written A "
                    "%d, B %d per slice"
                    % (what, res["A_over_B"],
                       "is within" if res["B_within_A_plus_spread"]
                       else "is NOT within",
                       "bit-equal" if values_equal else "DIFFER",
                       "hold their values" if targets_hold
                       else "DO NOT HOLD THEIR VALUES", bytes_a, bytes_b))
                say(json.dumps(res))
                del out
                torch.cuda.empty_cache()
        del every, slots
        torch.cuda.empty_cache()
    if args.out != "none":
        with open(args.out, "w") as f:
            f.write("tools/search_resident_rate.py --shapes %s --cases %s "
                    "--members %s --rows %d --queries %d --groups %d "
                    "--chunk %d -k %d --reps %d\n"
                    % (args.shapes, args.cases, args.members, args.rows,
                       args.queries, args.groups, args.chunk, args.k,
                       args.reps))
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
