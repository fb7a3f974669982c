#!/usr/bin/env python
"""Times of the PCA operators on the device, one JSON line.

Two shapes: C3's rows (1M x 128) and C4's (500k x 300, c_out = 50).  Per shape:
  * tsne_dev_pca_covariance: HIP events around `--repeats` calls after
    `--warmup` calls (torch events on the context's stream), and its kernels
    (pca_colmean, pca_gram, pca_gram_reduce) from the library's stage timers
    (HIP events around each kernel; the median over the repeats);
  * the host eigen-solve (tsne_sym_eig on the covariance), host clock;
  * pca_project from its stage timer inside tsne_dev_pca.
Beside every kernel time its two lower bounds: the bytes it must move (X read
once, 8 n d; the scores written, 8 n c_out) at the roofline's 8 TB/s
("Attraction roofline"), and its fp64 operations at the card's peak -- for pca_gram
2 n d_pad^2 / 2 (the upper triangle) at the 78.6 TFLOP/s fp64 matrix peak of
AMD's MI355X data sheet, for pca_project 2 n d c_out at the same figure for
vector fp64.  `x_reads` is pca_gram's own byte count over 8 n d: how often it
reads a row of X (one per panel pair; 1 for d <= 128).

    python scripts/pca_bench.py [--repeats 5] [--warmup 2] [--small]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tsne-flink_amd"))

HBM_BYTES_PER_S = 8e12          # the project's roofline rate
FP64_MATRIX_FLOPS = 78.6e12     # AMD Instinct MI355X data sheet: peak FP64 matrix, also its FP64 vector peak


def bounds(bytes_, flops):
    return {"hbm_ms": 1e3 * bytes_ / HBM_BYTES_PER_S, "fp64_ms": 1e3 * flops / FP64_MATRIX_FLOPS}


def fractions(ms, b):
    return {"ms": ms, **b, "hbm_frac": b["hbm_ms"] / ms, "fp64_frac": b["fp64_ms"] / ms}


def run_shape(ctx, T, torch, name, n, d, c_out, repeats, warmup):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    # planted spectrum with an offset, as in the tests
    X = torch.randn(n, d, generator=g, device=dev, dtype=torch.float64) * (1.6 ** -torch.arange(d, device=dev).clamp(max=40))
    X += 50.0
    mean = torch.zeros(d, dtype=torch.float64, device=dev)
    cov = torch.zeros(d, d, dtype=torch.float64, device=dev)
    scores = torch.zeros(n, c_out, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)       # the context enqueues on it, and so do the events below
    ctx.set_stream(stream.cuda_stream)
    kern = {"pca.colmean": [], "pca.gram": [], "pca.reduce": []}
    for _ in range(warmup):
        ctx.dev_pca_covariance(X, mean, cov)
    ctx.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call_ms = []
    for _ in range(repeats):
        e0.record(stream)
        ctx.dev_pca_covariance(X, mean, cov)
        e1.record(stream)
        e1.synchronize()
        call_ms.append(e0.elapsed_time(e1))
        for k in kern:
            kern[k].append(ctx.stage_ms(k)[-1])
    C = cov.cpu().numpy()
    t0 = time.perf_counter()
    T.sym_eig(C)
    eig_s = time.perf_counter() - t0
    proj = []
    for _ in range(warmup + repeats):
        ctx.dev_pca(X, c_out, None, None, None, scores)
        proj.append(ctx.stage_ms("pca.project")[-1])
    proj = proj[warmup:]
    d_pad = -(-d // 16) * 16
    npanels = -(-d_pad // 128)
    pairs = npanels * (npanels + 1) // 2
    # pca_gram's own reads of X: a diagonal pair stages its panel once, an off-diagonal pair both of its panels
    cols_read = sum((min(128, d - 128 * i) if i == j else min(128, d - 128 * i) + min(128, d - 128 * j))
                    for i in range(npanels) for j in range(i, npanels))
    med = statistics.median
    return {
        "shape": name, "n": n, "d": d, "d_pad": d_pad, "c_out": c_out, "panel_pairs": pairs,
        "x_reads": cols_read / d,
        "covariance_call_ms": med(call_ms), "covariance_call_ms_all": call_ms,
        "pca_colmean": fractions(med(kern["pca.colmean"]), bounds(8 * n * d, n * d)),
        "pca_gram": fractions(med(kern["pca.gram"]), bounds(8 * n * d, n * d_pad * d_pad)),
        "pca_gram_reduce_ms": med(kern["pca.reduce"]),
        "host_eig_s": eig_s,
        "pca_project": fractions(med(proj), bounds(8 * n * d + 8 * n * c_out, 2 * n * d * c_out)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="1/50 of the rows (a rehearsal, not a measurement)")
    a = ap.parse_args()
    import torch

    import tsne_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("pca_bench.py needs the GPU: nothing is measured without one")
    s = 50 if a.small else 1
    out = {"bench": "pca", "repeats": a.repeats, "warmup": a.warmup, "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "fp64_matrix_flops": FP64_MATRIX_FLOPS, "shapes": []}
    with T.Context(0) as ctx:
        for name, n, d, c in (("c3", 1_000_000 // s, 128, 2), ("c4", 500_000 // s, 300, 50)):
            out["shapes"].append(run_shape(ctx, T, torch, name, n, d, c, a.repeats, a.warmup))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
