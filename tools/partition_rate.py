#!/usr/bin/env python3
"""Agreement of P partitions of the same N rows: dist_partition_agreement_dev
against what there was before it, on one MI355X.  A tool, not part of
bench.py.

Shapes (synthetic label columns, no engines: one random partition of about
1 100 labels, and per column 10 % of the rows reassigned at random):
  i    P = 8, N = 10^7       (the bench's table, eight chains)
  ii   P = 1024, N = 20 000  (the exact chains' shape)

  A     what the device allowed before: per pair a <= b one
        torch.bincount(label_a * K + label_b), squared and summed, all pairs
        of the columns; at shape ii the P^2 / 2 launches are impractical, so A
        runs on the first 64 columns and B is timed on those 64 as well
        ("B64")
  B     engine.partition_agreement_labels on the same tensors, sq alone
        (nlogn=False), all P columns
  B+nl  the same with nlogn
  host  for the record, the route the tests took: np.unique and np.add.at on
        downloaded columns, the contingency of workloads.adjusted_rand_index,
        for --host-pairs pairs; the time per pair is printed

B's sq is first held to A's, entry by entry, where A has one.  Then each
repetition times the routes in turn (alternating, one process, one box) with
a host clock around calls that end in a device synchronise; every route is
warmed first.  Medians, spread (min .. max) and the ratio A / B are printed,
one JSON line per shape last.

    python tools/partition_rate.py [--shapes i,ii] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# P, N, the columns A runs on
SHAPES = {"i": (8, 10 ** 7, 8), "ii": (1024, 20000, 64)}
LABELS = 1100


def columns(p, n, dev, torch):
    gen = torch.Generator(device=dev)
    gen.manual_seed(20240917)
    base = torch.randint(0, LABELS, (n,), generator=gen, device=dev,
                         dtype=torch.int32)
    cols = []
    for _ in range(p):
        move = torch.rand((n,), generator=gen, device=dev) < 0.1
        other = torch.randint(0, LABELS, (n,), generator=gen, device=dev,
                              dtype=torch.int32)
        cols.append(torch.where(move, other, base).contiguous())
    return cols


def host_pair(a, b, np):
    ua, ia = np.unique(a, return_inverse=True)
    ub, ib = np.unique(b, return_inverse=True)
    c = np.zeros((ua.size, ub.size), np.int64)
    np.add.at(c, (ia, ib), 1)
    return int((c * c).sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="i,ii")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-pairs", type=int, default=2)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("partition_rate.py: no GPU; nothing is measured\n")
        return 2
    from distributions_amd import engine
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        p, n, pa = SHAPES[shape]
        cols = columns(p, n, dev, torch)
        wide = [c.to(torch.int64) for c in cols[:pa]]
        torch.cuda.synchronize()
        out = {}

        def route_a():
            sq = torch.zeros((pa, pa), dtype=torch.int64, device=dev)
            for a in range(pa):
                for b in range(a, pa):
                    cells = torch.bincount(wide[a] * LABELS + wide[b],
                                           minlength=LABELS * LABELS)
                    sq[a, b] = sq[b, a] = (cells * cells).sum()
            out["A"] = sq.cpu().numpy()

        def route_b():
            out["B"] = engine.partition_agreement_labels(cols, LABELS,
                                                         nlogn=False)

        def route_b_nl():
            out["B+nl"] = engine.partition_agreement_labels(cols, LABELS)

        def route_b_sub():
            out["B64"] = engine.partition_agreement_labels(cols[:pa], LABELS,
                                                           nlogn=False)

        routes = [("A", route_a), ("B", route_b), ("B+nl", route_b_nl)]
        if pa < p:
            routes.append(("B64", route_b_sub))
        for _, fn in routes:        # warm: code objects, allocator
            fn()
            fn()
        torch.cuda.synchronize()
        same = bool(np.array_equal(out["A"].astype(np.uint64),
                                   out["B"].sq[:pa, :pa])
                    and np.array_equal(out["B"].sq, out["B+nl"].sq))
        if not same:
            sys.stderr.write("partition_rate.py: shape %s: B's sq is not "
                             "A's; nothing is timed\n" % shape)
            return 1
        times = {name: [] for name, _ in routes}
        for _ in range(args.reps):
            for name, fn in routes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[name].append(time.perf_counter() - t0)
        res = dict(shape=shape, P=p, N=n, labels=LABELS, A_columns=pa,
                   sq_equal=same)
        for name, _ in routes:
            t = times[name]
            med = statistics.median(t)
            res[name] = dict(ms_median=1e3 * med, ms_min=1e3 * min(t),
                             ms_max=1e3 * max(t))
            print("%-3s %-5s %10.3f ms (min %.3f .. max %.3f)" % (
                shape, name, 1e3 * med, 1e3 * min(t), 1e3 * max(t)))
        # the host's route, per pair
        if args.host_pairs > 0:
            t0 = time.perf_counter()
            got = []
            for j in range(args.host_pairs):
                a, b = cols[0].cpu().numpy(), cols[j % pa].cpu().numpy()
                got.append(host_pair(a, b, np) == int(out["A"][0, j % pa]))
            per = (time.perf_counter() - t0) / args.host_pairs
            res["host_ms_per_pair"] = 1e3 * per
            res["host_equal"] = all(got)
            print("%-3s host  %10.3f ms per pair, download included (%d "
                  "pairs; all %d pairs of A's columns would take %.1f s)" % (
                      shape, 1e3 * per, args.host_pairs, pa * (pa + 1) // 2,
                      per * pa * (pa + 1) // 2))
        ref = "B64" if pa < p else "B"
        res["A_over_B"] = res["A"]["ms_median"] / res[ref]["ms_median"]
        # B is ahead (behind) only when the two spreads do not overlap
        if res[ref]["ms_max"] < res["A"]["ms_min"]:
            verdict = "B ahead beyond the spread"
        elif res["A"]["ms_max"] < res[ref]["ms_min"]:
            verdict = "B BEHIND beyond the spread"
        else:
            verdict = "within the spread"
        res["verdict"] = verdict
        print("%s time A / time %s = %.3f on %d columns (%s); sq equal" % (
            shape, ref, res["A_over_B"], pa, verdict))
        print(json.dumps(res))
        del cols, wide, out
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
