#!/usr/bin/env python
"""Times of the map scores on the device at C3's shape, one JSON line (also
written to --out, default profiles/quality_bench.json).

The run: C3's rows (1M x 128 GMM, tests/configs.py c3_torch) -> kNN (k = 90,
timed: the yardstick the scores are set beside) -> affinities -> joint -> the
fit (--iterations, theta 0.5) -> the map Y.  Then
  * tsne_dev_embedding_quality on `--sample` strided rows (quality_rows), k =
    `--quality-k`: the whole call by the host clock around a synchronised call
    (median of --repeats after one warm-up), and inside it the rank scan on X
    and on Y from the library's stage timer "ranks.scan" (HIP events around the
    scan kernel: interval 0 is rank_X over the N_Y lists, 1 is rank_Y over N_X);
  * once, every row on the map side only: rank_Y of the kNN lists of X
    (tsne_dev_neighbor_ranks on Y, m = k), n^2 pairs in 2-D.
Beside every scan time its fp64 VALU issue bound: 3 rounded operations (sub,
mul, add; 2 for cosine) per coordinate per pair at the vector fp64 rate --
AMD's MI355X data sheet gives 78.6 TFLOP/s counting an FMA as two, so 39.3e12
single rounded operations a second (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz).

    python scripts/quality_bench.py [--repeats 3] [--small] [--out PATH]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tsne-flink_amd"))
sys.path.insert(0, str(ROOT / "tests"))

FP64_VALU_OPS = 39.3e12   # rounded fp64 vector operations a second (half the data sheet's FMA-counted 78.6 TFLOP/s)


def scan(ms, s, n, d):
    bound = 1e3 * 3.0 * d * s * n / FP64_VALU_OPS
    return {"ms": ms, "pairs": s * n, "d": d, "fp64_valu_bound_ms": bound, "share_of_bound": bound / ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample", type=int, default=10000)
    ap.add_argument("--quality-k", type=int, default=90)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--small", action="store_true", help="1/50 of the rows (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "quality_bench.json"))
    a = ap.parse_args()
    import torch

    import configs
    import tsne_amd as T
    from tsne_amd.api import default_params
    if not torch.cuda.is_available():
        raise SystemExit("quality_bench.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    n, d, k, kq = (20_000 if a.small else 1_000_000), 128, 90, a.quality_k
    s = min(a.sample, n)
    out = {"bench": "quality", "n": n, "d": d, "knn_k": k, "quality_k": kq, "sample": s, "iterations": a.iterations,
           "repeats": a.repeats, "fp64_valu_ops_per_s": FP64_VALU_OPS}
    with T.Context(0) as ctx:
        X = configs.c3_torch(n, d, 2, dev)
        torch.cuda.synchronize()
        idx = torch.empty((n, k), dtype=torch.int32, device=dev)
        dist = torch.empty((n, k), dtype=torch.float64, device=dev)
        t0 = time.perf_counter()
        ctx.dev_knn(X, k, "sqeuclidean", 0, n, idx, dist)
        ctx.synchronize()
        out["knn_s"] = time.perf_counter() - t0
        rp = torch.arange(0, n * k + 1, k, dtype=torch.int64, device=dev)
        p = torch.empty_like(dist)
        ctx.dev_affinities(rp, dist, n, 30.0, p)
        cap = 2 * n * k
        orp = torch.empty(n + 1, dtype=torch.int64, device=dev)
        oc = torch.empty(cap, dtype=torch.int32, device=dev)
        ov = torch.empty(cap, dtype=torch.float64, device=dev)
        ctx.dev_joint(rp, idx, p, n, cap, orp, oc, ov)
        ctx.synchronize()
        del dist, p
        Y0, U0, G0 = ctx.initWorkingSet(n, 2, seed=0)
        Y, U, G = (torch.from_numpy(v).to(dev) for v in (Y0, U0, G0))
        t0 = time.perf_counter()
        ctx.dev_opt_setup(default_params(iterations=a.iterations, theta=0.5), orp, oc, ov, n, Y, U, G)
        for t in range(1, a.iterations + 1):
            ctx.dev_opt_step(t)
        ctx.dev_opt_sync()
        ctx.synchronize()
        out["fit_s"] = time.perf_counter() - t0

        rows = torch.from_numpy(T.quality_rows(n, s)).to(dev)
        calls, sx, sy, lx, ly, q = [], [], [], [], [], None
        for r in range(1 + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q = ctx.dev_embedding_quality(X, Y, kq, d_rows=rows)
            if r:
                calls.append(time.perf_counter() - t0)
                ms = ctx.stage_ms("ranks.scan")
                sx.append(ms[0])
                sy.append(ms[1])
                lx.append(ctx.stage_ms("quality.lists_x")[-1])
                ly.append(ctx.stage_ms("quality.lists_y")[-1])
        med = statistics.median
        out["sampled"] = {"call_s": med(calls), "call_s_all": calls, "call_over_knn": med(calls) / out["knn_s"],
                          "lists_x_ms": med(lx), "lists_y_ms": med(ly),
                          "lists_x_fallback_queries": ctx.counter("quality.fallback_x"),
                          "lists_y_fallback_queries": ctx.counter("quality.fallback_y"),
                          "rank_scan_x": scan(med(sx), s, n, d), "rank_scan_y": scan(med(sy), s, n, 2),
                          "trustworthiness": q.trustworthiness, "continuity": q.continuity,
                          "knn_recall": q.knn_recall, "sums": [int(v) for v in q.sums]}
        # every row, the map side only: rank_Y of the kNN lists of X
        cand = idx[:, :kq].contiguous() if kq <= k else idx
        rank = torch.empty(cand.shape, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.dev_neighbor_ranks(Y, cand, rank)
        ctx.synchronize()
        wall = time.perf_counter() - t0
        m = cand.shape[1]
        s_c = int(torch.clamp(rank.to(torch.int64) - m, min=0).sum().item())
        out["all_rows_map_side"] = {"call_s": wall, "m": m, "rank_scan_y": scan(ctx.stage_ms("ranks.scan")[-1], n, n, 2),
                                    "continuity": 1.0 - 2.0 * s_c / (n * m * (2 * n - 3 * m - 1))}
    line = json.dumps(out)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
