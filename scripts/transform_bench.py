#!/usr/bin/env python3
"""Timing of the transform (embedding new points into a fitted map) on one
MI355X: a synthetic n-point GMM map (--components 2 or 3) at theta = 0.5, m
new points for each m of --m.  Reports, per m: ms per transform iteration, the setup time (tree
build + query sort), and the cross kNN against tsne_dev_knn for the same
number of query rows; beside them two yardsticks on the same map: the member
path tsne_dev_repulsion per query, and oracle_tree_query on the CPU.

Host clock around work that ends in a context synchronise; every timed shape
is warmed first; --repeats windows, median and spread reported.  One JSON
line on stdout (and in --out).

The new points' rows of P are synthetic: the map's rows are sorted along a
Morton-like order, a new point hides next to a map row and takes the k rows
around it as neighbours (local, like real kNN rows; exact kNN on the map is
not what is timed), P from tsne_dev_pairwise_affinities on their distances.

--components 3 adds, on the same map: one iteration of the 3-D fit over the n
map points (tsne_dev_opt_step past early exaggeration; k local neighbours per
row with uniform P, learning rate 1 so that the map keeps its extent), and the
walk's stack pops per wave (option transform_stats) for the new points'
start and final positions."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "tsne-flink_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000, help="map points")
    ap.add_argument("--m", default="10000,100000,1000000", help="new points, comma-separated")
    ap.add_argument("--k", type=int, default=30, help="neighbours per new point")
    ap.add_argument("--dim", type=int, default=128, help="input dimension of the cross-kNN leg")
    ap.add_argument("--theta", type=float, default=0.5)
    ap.add_argument("--scale", type=float, default=1.0,
                    help="map scale: 1 = extent ~150 (a finished fit; short walks), 0.05 = extent ~8 (the fit's mid "
                         "phase; long walks)")
    ap.add_argument("--extent", type=float, default=0.0,
                    help="scale the map to this extent instead of --scale (C4: 7.5 when finished, 1.7 at t = 150)")
    ap.add_argument("--components", type=int, default=2, choices=(2, 3), help="the map's dimension")
    ap.add_argument("--lr", type=float, default=1.0,
                    help="the transform's learning rate (tsne_amd.transform's default 1.0 suits a finished map's extent; "
                         "on a small map the new points drift outwards and the walks shorten while they are timed)")
    ap.add_argument("--steps", type=int, default=40, help="iterations per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-sample", type=int, default=4096, help="queries of the oracle_tree_query yardstick (0: skip)")
    ap.add_argument("--resort", default="10", help="re-sort intervals to time (option transform_resort), comma-separated")
    ap.add_argument("--no-knn", action="store_true", help="skip the cross-kNN leg")
    ap.add_argument("--out", default="")
    return ap.parse_args()


def med_spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def gmm_map(n, seed, dev, c=2):
    """n x c GMM, rows ordered by a coarse Morton-like key (cluster cell, then x)."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    centres = torch.randn(64, c, generator=g, device=dev, dtype=torch.float64) * 25.0
    lab = torch.randint(0, 64, (n,), generator=g, device=dev)
    Y = centres[lab] + torch.randn(n, c, generator=g, device=dev, dtype=torch.float64) * 2.0
    Y -= Y.mean(dim=0)
    cell = torch.floor((Y - Y.min(dim=0).values) / 0.5).to(torch.int64)
    key = cell[:, 1] * (1 << 20) + cell[:, 0]
    if c == 3:
        key = cell[:, 2] * (1 << 40) + key
    order = torch.argsort(key, stable=True)
    return Y[order].contiguous()


def fit_step_ms(ctx, a, Yr, timed):
    """ms per tsne_dev_opt_step on the map itself: tree build, the member walk
    with its shortcuts, attraction, update."""
    import torch
    from tsne_amd.api import default_params
    dev, n, k = Yr.device, Yr.shape[0], a.k
    off = torch.cat([torch.arange(-(k // 2), 0, device=dev), torch.arange(1, k - k // 2 + 1, device=dev)])
    col = ((torch.arange(n, device=dev)[:, None] + off[None, :]) % n).to(torch.int32).contiguous().view(-1)
    rp = torch.arange(0, n * k + 1, k, device=dev, dtype=torch.int64)
    P = torch.full((n * k,), 1.0 / (n * k), device=dev, dtype=torch.float64)
    prm = default_params(n_components=Yr.shape[1], iterations=100000, theta=a.theta, learning_rate=1.0)
    Y, upd, gains = Yr.clone(), torch.zeros_like(Yr), torch.ones_like(Yr)
    torch.cuda.synchronize()
    ctx.set_option("graph_order", 0)   # the rows are in Morton-like order already (and a ring graph has no clusters to find)
    ctx.dev_opt_setup(prm, rp, col, P, n, Y, upd, gains)
    ctx.set_option("graph_order", 1)
    t = 200  # past early exaggeration: the late near-exact tolerance, as at the end of a fit
    for _ in range(a.warmup):
        ctx.dev_opt_step(t)
        t += 1
    ctx.dev_opt_sync()
    wins = []
    for _ in range(a.repeats):
        def window():
            nonlocal t
            for _ in range(a.steps):
                if t % 10 == 0:
                    t += 1   # a loss iteration costs extra: not what is compared
                ctx.dev_opt_step(t)
                t += 1
            ctx.dev_opt_sync()
        wins.append(timed(window) / a.steps)
    ext = float((Y.max(dim=0).values - Y.min(dim=0).values).max().item())
    return med_spread(wins), ext


def main():
    a = parse()
    import torch
    import tsne_amd as T
    from tsne_amd.api import default_params
    dev = "cuda:0"
    c = a.components
    res = {"n": a.n, "components": c, "scale": a.scale, "lr": a.lr, "k": a.k, "theta": a.theta, "steps": a.steps, "warmup": a.warmup,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "sizes": {}}
    Yr = gmm_map(a.n, 1, dev, c)
    if a.extent > 0.0:
        a.scale = a.extent / float((Yr.max(dim=0).values - Yr.min(dim=0).values).max().item())
        res["scale"] = a.scale
    Yr = (Yr * a.scale).contiguous()
    res["extent"] = float((Yr.max(dim=0).values - Yr.min(dim=0).values).max().item())
    g = torch.Generator(device=dev).manual_seed(2)
    with T.Context(0) as ctx:
        def timed(fn):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3

        # yardstick: the member path over the whole map, per query
        dF, dz = torch.zeros_like(Yr), torch.zeros(a.n, device=dev, dtype=torch.float64)
        torch.cuda.synchronize()
        ctx.dev_repulsion(Yr, a.theta, dF, dz)
        ms = [timed(lambda: ctx.dev_repulsion(Yr, a.theta, dF, dz)) for _ in range(a.repeats)]
        res["member_repulsion_ms"] = med_spread(ms)
        res["member_repulsion_ns_per_query"] = med_spread(ms)["median"] * 1e6 / a.n

        for m in [int(x) for x in a.m.split(",")]:
            r = {}
            home = torch.randint(a.k, a.n - a.k, (m,), generator=g, device=dev)
            Q0 = Yr[home] + torch.randn(m, c, generator=g, device=dev, dtype=torch.float64) * (0.7 * a.scale)
            col = (home[:, None] + torch.arange(-(a.k // 2), a.k - a.k // 2, device=dev)[None, :]).to(torch.int32)
            dist = ((Q0[:, None, :] - Yr[col.long()]) ** 2).sum(dim=2).contiguous()
            rp = torch.arange(0, m * a.k + 1, a.k, device=dev, dtype=torch.int64)
            P = torch.zeros(m * a.k, device=dev, dtype=torch.float64)
            torch.cuda.synchronize()
            ctx.dev_affinities(rp, dist.view(-1), m, 10.0, P)
            ctx.synchronize()
            Yinit = (P.view(m, a.k, 1) * Yr[col.long()]).sum(dim=1).contiguous()
            col = col.contiguous().view(-1)
            prm = default_params(n_components=c, iterations=1000, theta=a.theta, learning_rate=a.lr)
            Y, upd, gains = Yinit.clone(), torch.zeros_like(Yinit), torch.ones_like(Yinit)
            torch.cuda.synchronize()

            def setup():
                ctx.dev_transform_setup(prm, Yr, rp, col, P, Y, upd, gains)
            setup()   # warm (allocations, the first build's sort)
            r["setup_ms"] = med_spread([timed(setup) for _ in range(a.repeats)])
            # ms per iteration for each re-sort interval (option transform_resort), each from the same start
            r["iter_ms_by_resort"] = {}
            forms = [(int(x), 0) for x in a.resort.split(",")] + [(10, 1)]   # (re-sort interval, split form)
            for R, split in forms:
                ctx.set_option("transform_resort", R)
                ctx.set_option("transform_split", split)
                Y.copy_(Yinit); upd.zero_(); gains.fill_(1.0)
                torch.cuda.synchronize()
                setup()
                t = 1
                for _ in range(a.warmup):
                    ctx.dev_transform_step(t)
                    t += 1
                wins = []
                for _ in range(a.repeats):
                    def window():
                        nonlocal t
                        for _ in range(a.steps):
                            ctx.dev_transform_step(t)
                            t += 1
                    wins.append(timed(window) / a.steps)
                ctx.dev_transform_sync()
                if split:
                    r["iter_ms_split_launches"] = med_spread(wins)
                else:
                    r["iter_ms_by_resort"][str(R)] = med_spread(wins)
            ctx.set_option("transform_resort", 10)
            ctx.set_option("transform_split", 0)
            r["iter_ms"] = r["iter_ms_by_resort"].get("10", med_spread(wins))
            r["iter_ns_per_point"] = r["iter_ms"]["median"] * 1e6 / m
            r["finite"] = bool(torch.isfinite(Y).all().item())
            # the walk alone: tsne_dev_repulsion_queries (tree build + sort + walk) minus the setup
            qF, qz = torch.zeros_like(Y), torch.zeros(m, device=dev, dtype=torch.float64)
            ctx.dev_repulsion_queries(Yr, a.theta, Y, qF, qz)
            r["repulsion_queries_call_ms"] = med_spread(
                [timed(lambda: ctx.dev_repulsion_queries(Yr, a.theta, Y, qF, qz)) for _ in range(a.repeats)])
            if c == 3:   # the walk's pops per wave where the new points start and where the timed steps left them
                ctx.set_option("transform_stats", 1)
                for name, where in (("pops_per_wave_start", Yinit), ("pops_per_wave_end", Y)):
                    ctx.dev_repulsion_queries(Yr, a.theta, where, qF, qz)
                    r[name] = ctx.counter("xform3.pops") / ((m + 63) // 64)
                ctx.set_option("transform_stats", 0)
                r["max_abs_y_start"] = float(Yinit.abs().max().item())
                r["max_abs_y_end"] = float(Y.abs().max().item())
            res["sizes"][str(m)] = r

        if c == 3:   # yardstick: one iteration of the fit on the same map
            res["fit_step_ms"], res["fit_extent_after"] = fit_step_ms(ctx, a, Yr, timed)

        if not a.no_knn:
            X = torch.randn(32, a.dim, generator=g, device=dev, dtype=torch.float64)[
                torch.randint(0, 32, (a.n,), generator=g, device=dev)] * 3.0
            X += torch.randn(a.n, a.dim, generator=g, device=dev, dtype=torch.float64)
            kk = 90
            for m in [int(x) for x in a.m.split(",")]:
                m = min(m, a.n)
                Xq = (X[torch.randint(0, a.n, (m,), generator=g, device=dev)]
                      + 0.5 * torch.randn(m, a.dim, generator=g, device=dev, dtype=torch.float64)).contiguous()
                idx = torch.zeros(m, kk, device=dev, dtype=torch.int32)
                dd = torch.zeros(m, kk, device=dev, dtype=torch.float64)
                torch.cuda.synchronize()
                ctx.dev_knn_cross(X, Xq, kk, "sqeuclidean", idx, dd)
                cross = [timed(lambda: ctx.dev_knn_cross(X, Xq, kk, "sqeuclidean", idx, dd)) for _ in range(a.repeats)]
                ctx.dev_knn(X, kk, "sqeuclidean", 0, m, idx, dd)
                own = [timed(lambda: ctx.dev_knn(X, kk, "sqeuclidean", 0, m, idx, dd)) for _ in range(a.repeats)]
                res["sizes"].setdefault(str(m), {}).update(
                    {"knn_cross_ms": med_spread(cross), "dev_knn_same_rows_ms": med_spread(own), "knn_k": kk,
                     "knn_dim": a.dim})
                del Xq, idx, dd
            del X

    if a.cpu_sample > 0:   # yardstick: the CPU oracle's foreign-query walk on the same map
        import oracle_ctypes as O
        Yh = Yr.cpu().numpy()
        rng = np.random.default_rng(3)
        Qh = Yh[rng.integers(0, a.n, a.cpu_sample)] + rng.normal(size=(a.cpu_sample, c)) * (0.7 * a.scale)
    if a.cpu_sample > 0 and c == 3:   # the octree restatement builds its tree inside the call
        t0 = time.perf_counter()
        O.repulsion3_queries(Yh, a.theta, Qh, threads=16)
        res["oracle_repulsion3_queries_16thr_s"] = time.perf_counter() - t0
    elif a.cpu_sample > 0:
        t0 = time.perf_counter()
        tree = O.Tree(Yh)
        res["oracle_tree_build_s"] = time.perf_counter() - t0
        tree.query(a.theta, Qh[:64], threads=16)
        t0 = time.perf_counter()
        tree.query(a.theta, Qh, threads=16)
        dt = time.perf_counter() - t0
        res["oracle_tree_query_16thr_us_per_query"] = dt * 1e6 / a.cpu_sample
        tree.close()

    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
