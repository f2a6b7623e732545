#!/usr/bin/env python3
"""Drawn rows per second: dist_gibbs_sample_rows_dev against the only route
there was before it, on one MI355X.  A tool, not part of bench.py.

Shapes, all at K = 1024 + 1 empty, PitmanYor(1, 0.2), resident rows generated
on the device from a seed, initial assignment i mod K:
  i    DirichletDiscrete dim 256 alone, nothing observed
  ii   DD16 + DD4 + BetaBernoulli + GammaPoisson + NormalInverseChiSq,
       nothing observed
  iii  shape ii with half the cells observed at random (the observed values
       are resident rows' own)

  host     the route that existed: counts() and every group through
           get_group, then numpy on one core -- the group from the
           clustering model's weights (iii: times the observed cells'
           predictive, a [rows, K] matrix in chunks), then every missing cell
           vectorised per drawn group.  Its draws are numpy's, not the
           engine's streams: the same law, other numbers.  --host-rows rows
           are drawn (iii: --host-rows-iii) and the rate is per row.
  device   dist_gibbs_sample_rows_dev into preallocated device columns
  generic  (shape i) the same call with a mask of zeros, which takes the
           generic instance instead of the nothing-observed one: their A/B

Each repetition times the routes in turn (alternating, one process, one box)
with a host clock around calls that end in a device synchronise; all routes
are warmed first.  Medians, spread (min .. max) and the ratios are printed,
one JSON line per shape last.

    python tools/sample_rows_rate.py [--rows 1000000] [--reps 7]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python \\
        tools/sample_rows_rate.py --reps 1 --no-host   # kernel times, in a
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

ALPHA, D = 1.0, 0.2


def make(shape, n, k, dev, torch, engine):
    gen = torch.Generator(device=dev)
    gen.manual_seed(20240601)

    def ints(hi):
        return torch.randint(0, hi, (n,), generator=gen, device=dev,
                             dtype=torch.int32)

    if shape == "i":
        cols = [ints(256)]
        shareds = [engine.dd_shared([0.5] * 256)]
    else:
        rate = torch.full((n,), 5.0, device=dev)
        cols = [ints(16), ints(4), ints(2),
                torch.poisson(rate, generator=gen).to(torch.int32),
                torch.randn((n,), generator=gen, device=dev)]
        shareds = [engine.dd_shared([0.5] * 16), engine.dd_shared([0.5] * 4),
                   engine.bb_shared(0.5, 2.0), engine.gp_shared(1.0, 1.0),
                   engine.nich_shared(0.0, 1.0, 1.0, 1.0)]
    assign = (torch.arange(n, device=dev, dtype=torch.int64) % k).to(
        torch.int32)
    gpu = engine.Gibbs(ALPHA, D, shareds)
    gpu.load_rows_torch(cols, assign, k, 1)
    return gpu, cols


def host_route(gpu, n, values, masks, np, special):
    """n rows drawn on the host from what the engine hands out.  values /
    masks: host arrays of the observed cells, or None.  -> columns"""
    rng = np.random.default_rng(1)
    counts = gpu.counts().astype(np.float64)
    K = len(counts)
    F = len(gpu.shareds)
    groups = [[gpu.get_group(f, k) for k in range(K)] for f in range(F)]
    # PitmanYor score_value as weights (clustering.hpp:195-208)
    N = counts.sum()
    empty = counts == 0
    nonempty = K - empty.sum()
    w = np.where(empty, (ALPHA + D * nonempty) / max(empty.sum(), 1),
                 counts - D) / (N + ALPHA)
    logw = np.log(w)
    kinds = [s.kind for s in gpu.shareds]
    from distributions_amd import _core
    post = []
    for f, s in enumerate(gpu.shareds):
        g = np.stack(groups[f]).view(np.int32).astype(np.float64)
        p = [float(x) for x in s.p]
        if kinds[f] == _core.KIND_DD:
            a = 0.5 + g[:, 1:]
            post.append(a / a.sum(1, keepdims=True))
        elif kinds[f] == _core.KIND_BB:
            a, b = p[0] + g[:, 0], p[1] + g[:, 1]
            post.append(a / (a + b))
        elif kinds[f] == _core.KIND_GP:
            post.append((p[0] + g[:, 1], p[1] + g[:, 0]))
        else:
            raw = np.stack(groups[f])
            cnt = g[:, 0]
            mean = raw[:, 1].copy().view(np.float32).astype(np.float64)
            ctv = raw[:, 2].copy().view(np.float32).astype(np.float64)
            mu, kappa, sigmasq, nu = p
            kn = kappa + cnt
            mun = (kappa * mu + mean * cnt) / kn
            nun = nu + cnt
            sn = (nu * sigmasq + ctv + cnt * kappa * (mu - mean) ** 2 / kn) \
                / nun
            post.append((nun, mun, np.sqrt(sn * (kn + 1.0) / kn)))
    if masks is None:
        pick = rng.choice(K, size=n, p=w / w.sum())
    else:
        pick = np.empty(n, np.int64)
        for r0 in range(0, n, 4096):
            r1 = min(n, r0 + 4096)
            s = np.broadcast_to(logw, (r1 - r0, K)).copy()
            for f in range(F):
                on = ((masks[r0:r1] >> f) & 1).astype(bool)
                if not on.any():
                    continue
                x = values[f][r0:r1][on]
                if kinds[f] == _core.KIND_DD:
                    s[on] += np.log(post[f][:, x]).T
                elif kinds[f] == _core.KIND_BB:
                    pk = post[f][None, :]
                    s[on] += np.log(np.where(x[:, None] != 0, pk, 1.0 - pk))
                elif kinds[f] == _core.KIND_GP:
                    a, ib = post[f]
                    xv = x.astype(np.float64)[:, None]
                    s[on] += (special.gammaln(a[None, :] + xv)
                              - special.gammaln(a)[None, :]
                              - special.gammaln(xv + 1.0)
                              + (a * np.log(ib / (ib + 1.0)))[None, :]
                              - xv * np.log(ib + 1.0)[None, :])
                else:
                    nun, mun, scale = post[f]
                    z = (x.view(np.float32).astype(np.float64)[:, None]
                         - mun[None, :]) / scale[None, :]
                    s[on] += ((special.gammaln((nun + 1) / 2)
                               - special.gammaln(nun / 2)
                               - 0.5 * np.log(nun * np.pi)
                               - np.log(scale))[None, :]
                              - (nun[None, :] + 1) / 2
                              * np.log1p(z * z / nun[None, :]))
            s -= s.max(1, keepdims=True)
            c = np.cumsum(np.exp(s), 1)
            u = rng.random(r1 - r0) * c[:, -1]
            pick[r0:r1] = np.minimum((c < u[:, None]).sum(1), K - 1)
    order = np.argsort(pick, kind="stable")
    bounds = np.searchsorted(pick[order], np.arange(K + 1))
    cols = []
    for f in range(F):
        out = (np.empty(n, np.float32) if kinds[f] == _core.KIND_NICH
               else np.empty(n, np.uint32))
        for k in range(K):
            rows = order[bounds[k]:bounds[k + 1]]
            m = len(rows)
            if m == 0:
                continue
            if kinds[f] == _core.KIND_DD:
                out[rows] = rng.choice(post[f].shape[1], size=m, p=post[f][k])
            elif kinds[f] == _core.KIND_BB:
                out[rows] = rng.random(m) < post[f][k]
            elif kinds[f] == _core.KIND_GP:
                a, ib = post[f]
                out[rows] = rng.poisson(rng.gamma(a[k], 1.0 / ib[k], m))
            else:
                nun, mun, scale = post[f]
                out[rows] = mun[k] + scale[k] * rng.standard_t(nun[k], m)
        if masks is not None:
            on = ((masks >> f) & 1).astype(bool)
            out.view(np.uint32)[on] = values[f][on]
        cols.append(out)
    return cols


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=1000000, help="rows drawn")
    ap.add_argument("--resident", type=int, default=1000000,
                    help="resident rows (the statistics the groups hold)")
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="i,ii,iii")
    ap.add_argument("--host-rows", type=int, default=1000000)
    ap.add_argument("--host-rows-iii", type=int, default=50000)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    from scipy import special
    if not torch.cuda.is_available():
        sys.stderr.write("sample_rows_rate.py: no GPU; nothing is measured\n")
        return 2
    torch.set_num_threads(1)
    from distributions_amd import engine
    dev = torch.device("cuda", 0)
    n = args.rows
    for shape in args.shapes.split(","):
        gpu, cols = make("i" if shape == "i" else "ii", args.resident,
                         args.groups, dev, torch, engine)
        K = len(gpu)
        F = len(cols)
        outs = [torch.empty(n, dtype=torch.int32, device=dev)
                for _ in range(F)]
        group = torch.empty(n, dtype=torch.int32, device=dev)
        out_ptrs = [int(o.data_ptr()) for o in outs]
        vals = mk = None
        h_vals = h_mask = None
        if shape == "iii":
            gen = torch.Generator(device=dev)
            gen.manual_seed(7)
            idx = torch.arange(n, device=dev) % args.resident
            vals = [c[idx].contiguous().view(torch.int32) for c in cols]
            mk = torch.randint(0, 1 << F, (n,), generator=gen, device=dev,
                               dtype=torch.int32)
            nh = min(n, args.host_rows_iii)
            h_vals = [v[:nh].cpu().numpy().view(np.uint32) for v in vals]
            h_mask = mk[:nh].cpu().numpy().view(np.uint32)
        else:
            nh = min(n, args.host_rows)
        zeros = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def route_device():
            gpu.core.sample_rows_dev(
                None if vals is None else [int(v.data_ptr()) for v in vals],
                n, 0 if mk is None else int(mk.data_ptr()), out_ptrs,
                int(group.data_ptr()), 12345, 0)

        def route_generic():
            gpu.core.sample_rows_dev(None, n, int(zeros.data_ptr()), out_ptrs,
                                     int(group.data_ptr()), 12345, 0)

        def route_host():
            host_route(gpu, nh, h_vals, h_mask, np, special)

        routes = [("device", route_device, n)]
        if shape == "i":
            routes.append(("generic", route_generic, n))
        if not args.no_host:
            routes.append(("host", route_host, nh))
        for name, fn, _ in routes:   # warm: code objects, allocator, tables
            fn()
            if name != "host":
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in routes}
        for _ in range(args.reps):
            for name, fn, _ in routes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[name].append(time.perf_counter() - t0)
        res = dict(shape=shape, K=K, rows=n, features=F)
        for name, _, rows in routes:
            t = times[name]
            med = statistics.median(t)
            res[name] = dict(rows=rows, ms_median=1e3 * med,
                             ms_min=1e3 * min(t), ms_max=1e3 * max(t),
                             rows_per_s=rows / med)
            print("%-3s %-7s %8d rows %10.3f ms (min %.3f .. max %.3f)  "
                  "%.3e rows/s" % (shape, name, rows, 1e3 * med,
                                   1e3 * min(t), 1e3 * max(t), rows / med))
        if "host" in res:
            r = res["device"]["rows_per_s"] / res["host"]["rows_per_s"]
            res["device_over_host"] = r
            print("%-3s device / host rows per second = %.1f (device %s)" % (
                shape, r, "faster" if r > 1.0 else "NOT FASTER"))
        if "generic" in res:
            r = res["generic"]["ms_median"] / res["device"]["ms_median"]
            res["generic_over_uncond"] = r
            print("%-3s time generic / time nothing-observed = %.3f" % (
                shape, r))
        print(json.dumps(res))
        del gpu, outs, group
    return 0


if __name__ == "__main__":
    sys.exit(main())
