#!/usr/bin/env python3
"""Rows drawn from an ensemble of M engines: dist_gibbs_sample_rows_many_dev
against the only route there was before it, on one MI355X.  A tool, not part
of bench.py.

Shapes (every member PitmanYor(1, 0.2), K = 1024 + 1 empty, its own rows
generated on the device from its own seed, initial assignment i mod K):
  1    M = 8,   10^6 rows, DirichletDiscrete dim 256 alone, nothing observed
  2    M = 512, 4 096 rows, the bench's mixed rows DD(16) + DD(4) +
       BetaBernoulli + GammaPoisson + NormalInverseChiSq, half the cells
       observed
  3    M = 64,  65 536 rows, GammaPoisson + NormalInverseChiSq, half observed
  4    M = 512, 4 096 rows, DD(256) alone, nothing observed (not one of the
       three: the likelihood kernels' A/B under rocprofv3)
"Half observed": feature 0 is observed by no row -- it is the target route A
has to name, and the member it draws is then B's -- and each other feature by
a row with probability F / (2 (F - 1)).

  A    predict_feature_many_dev asked for the member alone, the members to
       the host, the rows bucketed by member, M Gibbs.sample_rows_torch calls
       on the gathered subsets (a member no row drew is skipped), the scatter
       back
  B    sample_rows_many_torch

Each repetition times the routes in turn (alternating, one process, one box)
with a host clock around calls that end in a device synchronise; both routes
are warmed first.  Medians, spread (min .. max) and the ratio A / B are
printed, one JSON line per shape last.  The members of A and B are compared
(they must be equal); groups and cells are not: a subset call numbers its rows
anew, so A's engine steps and cell keys are not the query's own.

    python tools/sample_rows_many_rate.py [--shapes 1,2,3] [--reps 7]
    rocprofv3 --kernel-trace --stats -d DIR -- python \\
        tools/sample_rows_many_rate.py --reps 1 --shapes 1   # kernel times
                              # and launch counts, in a run of its own
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# kind, M, rows, something observed
SHAPES = {"1": ("dd", 8, 1000000, False), "2": ("mixed", 512, 4096, True),
          "3": ("gp_nich", 64, 65536, True), "4": ("dd", 512, 4096, False)}


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


def half_masks(F, n, dev, torch):
    """feature 0 never, every other feature with probability F / (2 (F - 1))"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    masks = torch.zeros(n, dtype=torch.int32, device=dev)
    p = F / (2.0 * (F - 1))
    for f in range(1, F):
        on = torch.rand((n,), generator=gen, device=dev) < p
        masks |= on.to(torch.int32) << f
    return masks


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="1,2,3")
    ap.add_argument("--rows", type=int, default=20000,
                    help="resident rows per member")
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("sample_rows_many_rate.py: no GPU; nothing is "
                         "measured\n")
        return 2
    from distributions_amd import _core, engine
    dev = torch.device("cuda", 0)
    seed_state = _core.rng_seed(args.seed)
    member_state = _core.rng_seed(args.seed + 1)
    for shape in args.shapes.split(","):
        kind, M, n, seen = SHAPES[shape]
        gpus = [member(kind, args.rows, args.groups, 1000 + e, dev, torch,
                       engine) for e in range(M)]
        cores = [g.core for g in gpus]
        F = len(gpus[0].shareds)
        cols = columns(kind, n, 7, dev, torch) if seen else None
        masks = half_masks(F, n, dev, torch) if seen else None
        dtypes = [torch.float32 if s.kind == _core.KIND_NICH else torch.int32
                  for s in gpus[0].shareds]
        torch.cuda.synchronize()
        out = {}

        def route_a():
            chosen = torch.empty(n, dtype=torch.int32, device=dev)
            _core.predict_feature_many_dev(
                cores, [0] * F if cols is None else
                [0] + [int(c.data_ptr()) for c in cols[1:]], n,
                0 if masks is None else int(masks.data_ptr()), 0,
                None if kind != "gp_nich" else [0], 0, 0, 0,
                int(chosen.data_ptr()), 0, seed_state, member_state, 0,
                prior_totals=False)
            host = chosen.cpu()                      # the trip to the host
            order = torch.argsort(host, stable=True)
            counts = torch.bincount(host, minlength=M).tolist()
            order = order.to(dev)
            done = [torch.empty(n, dtype=t, device=dev) for t in dtypes]
            groups = torch.empty(n, dtype=torch.int32, device=dev)
            at = 0
            for e in range(M):
                c = counts[e]
                if c == 0:
                    continue
                idx = order[at:at + c]
                at += c
                if cols is None:
                    sub, g = gpus[e].sample_rows_torch(n=c, seed=args.seed)
                else:
                    sub, g = gpus[e].sample_rows_torch(
                        values=[v[idx] for v in cols], observed=masks[idx],
                        seed=args.seed)
                for f in range(F):
                    done[f][idx] = sub[f]
                groups[idx] = g
            torch.cuda.synchronize()
            out["A"] = (done, groups, chosen)

        def route_b():
            out["B"] = engine.sample_rows_many_torch(
                gpus, n=n, values=cols, observed=masks, seed=args.seed)

        routes = [("A", route_a), ("B", route_b)]
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
        same = bool(torch.equal(out["A"][2], out["B"][2]))
        drawn = int(torch.unique(out["B"][2]).numel())
        res = dict(shape=shape, kind=kind, M=M, K=len(gpus[0]), rows=n,
                   observed="half" if seen else "nothing",
                   members_equal=same, members_drawn=drawn)
        for name, _ in routes:
            t = times[name]
            med = statistics.median(t)
            res[name] = dict(ms_median=1e3 * med, ms_min=1e3 * min(t),
                             ms_max=1e3 * max(t))
            print("%-2s %-2s %9.3f ms (min %.3f .. max %.3f)" % (
                shape, name, 1e3 * med, 1e3 * min(t), 1e3 * max(t)))
        res["A_over_B"] = res["A"]["ms_median"] / res["B"]["ms_median"]
        print("%s time A / time B = %.3f (B %s); %d of %d members drawn; the "
              "members of A and B %s" % (
                  shape, res["A_over_B"],
                  "not slower" if res["A_over_B"] >= 1.0 else "SLOWER",
                  drawn, M, "are equal" if same else "DIFFER"))
        print(json.dumps(res))
        del gpus, cores, out
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
