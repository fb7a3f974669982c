// pca.hip -- column means, centred Gram matrix (fp64 MFMA), projection onto the
// leading eigenvectors, and the PCA initialisation of the working set.  The
// definitions, the tile mapping and the chunk rule are in pca.hpp.
#include "pca.hpp"

#include <cmath>
#include <vector>

namespace tsne {

namespace {

constexpr int MEAN_ROWS = 1024;    // rows per partial column sum
constexpr int GRAM_PANEL = 128;    // columns per panel (8 tiles of 16)
constexpr int GRAM_SLAB = 32;      // rows staged in LDS at a time (8 MFMA k-steps)
constexpr int GRAM_THREADS = 512;  // 8 waves
constexpr int GRAM_WAVES = GRAM_THREADS / 64;
// LDS row stride in doubles: two panels + 16, so the four rows a k-step reads
// (128 B each) alternate between the two halves of the 64 banks
constexpr int GRAM_LDW = 2 * GRAM_PANEL + 16;
constexpr int PROJ_ROWS = 64;      // rows per pca_project workgroup (one per lane)
constexpr int PROJ_SLICE = 32;     // columns of X and V staged per step

typedef double v4d __attribute__((ext_vector_type(4)));

// p[i * stride] summed over i = first, first + step, ... < count (count >= 1), in
// that order.  The loads go out in batches of 8 from clamped (always valid)
// addresses, so that none waits for the sum; a term past the end adds 0.0.
__device__ __forceinline__ double strided_sum(const double *__restrict__ p, int64_t stride, int64_t first, int64_t step,
                                              int64_t count) {
    double s = 0.0;
    for (int64_t i = first; i < count; i += 8 * step) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t ik = i + k * step;
            v[k] = p[(ik < count ? ik : count - 1) * stride];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) s += i + k * step < count ? v[k] : 0.0;
    }
    return s;
}

// grid (chunks, ceil(d / 64)), 256 threads: lane = column, 4 row lanes (rows ty, ty + 4, ...).
__global__ __launch_bounds__(256) void pca_colmean_partial(const double *__restrict__ X, int64_t n, int d,
                                                           double *__restrict__ part) {
    __shared__ double sh[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int col = blockIdx.y * 64 + tx, cl = col < d ? col : d - 1;
    const int64_t r0 = (int64_t)blockIdx.x * MEAN_ROWS;
    const int64_t r1 = r0 + MEAN_ROWS < n ? r0 + MEAN_ROWS : n;
    sh[ty][tx] = strided_sum(X + r0 * d + cl, d, ty, 4, r1 - r0);
    __syncthreads();
    if (ty == 0 && col < d) part[(int64_t)blockIdx.x * d + col] = ((sh[0][tx] + sh[1][tx]) + sh[2][tx]) + sh[3][tx];
}

// grid ceil(d / 64), 1024 threads: lane = column, 16 chunk lanes (chunks ty, ty + 16, ...),
// combined in lane order.
__global__ __launch_bounds__(1024) void pca_colmean_final(const double *__restrict__ part, int64_t chunks, int64_t n,
                                                          int d, double *__restrict__ mean) {
    __shared__ double sh[16][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + tx, cl = col < d ? col : d - 1;
    sh[ty][tx] = strided_sum(part + cl, d, ty, 16, chunks);
    __syncthreads();
    if (ty != 0 || col >= d) return;
    double s = sh[0][tx];
#pragma unroll
    for (int l = 1; l < 16; ++l) s += sh[l][tx];
    mean[col] = s / (double)n;
}

// One workgroup's slabs for a panel pair whose waves own PER tiles each (the
// last wave may own fewer: its spare accumulators repeat tile 0 and are dropped).
// Staging: the pair's columns side by side (one panel when DIAG); a thread keeps
// one column and takes every (512 / width)-th row of the slab.  The loads are
// unconditional, from clamped addresses, and nothing depends on them until the
// next slab's LDS store (which centres them and zeroes what lies past the
// chunk or past d), so they stay in flight across the MFMAs of the current slab.
template <int PER, bool DIAG>
__device__ __forceinline__ void gram_body(const double *__restrict__ X, const double *__restrict__ mu, int64_t d,
                                          int64_t r0, int64_t r1, int ntiles, const int *tile_ij, double *xs, int pi,
                                          int pj, int d_pad, double *__restrict__ out) {
    constexpr int LW = DIAG ? 7 : 8, WIDTH = 1 << LW, RSTEP = GRAM_THREADS >> LW, NPRE = GRAM_SLAB / RSTEP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = tid & (WIDTH - 1), rfirst = tid >> LW;
    const int gc = c < GRAM_PANEL ? pi * GRAM_PANEL + c : pj * GRAM_PANEL + (c - GRAM_PANEL);
    const bool col_ok = gc < d;
    const int64_t gcl = col_ok ? gc : d - 1;
    const double muc = mu[gcl];
    const int nslab = (int)((r1 - r0 + GRAM_SLAB - 1) / GRAM_SLAB);
    double pre[NPRE];
    auto load = [&](int s) {
        const int64_t rb = r0 + (int64_t)s * GRAM_SLAB + rfirst;
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int64_t r = rb + i * RSTEP;
            pre[i] = X[(r < r1 ? r : r1 - 1) * d + gcl];
        }
    };
    load(0);
    const int first = wave * PER;
    int offA[PER], offB[PER];
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int ij = tile_ij[first + t < ntiles ? first + t : 0];
        offA[t] = (ij >> 8) * 16;
        offB[t] = (DIAG ? 0 : GRAM_PANEL) + (ij & 255) * 16;
    }
    v4d acc[PER];
#pragma unroll
    for (int t = 0; t < PER; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
    const int kr = lane >> 4, cc = lane & 15;

    for (int s = 0; s < nslab; ++s) {
        const int64_t rb = r0 + (int64_t)s * GRAM_SLAB + rfirst;
#pragma unroll
        for (int i = 0; i < NPRE; ++i)
            xs[(rfirst + i * RSTEP) * GRAM_LDW + c] = (col_ok && rb + i * RSTEP < r1) ? pre[i] - muc : 0.0;
        __syncthreads();
        if (s + 1 < nslab) load(s + 1);
#pragma unroll
        for (int k = 0; k < GRAM_SLAB / 4; ++k) {
            const double *row = xs + (k * 4 + kr) * GRAM_LDW + cc;
            double a[PER], b[PER];
#pragma unroll
            for (int t = 0; t < PER; ++t) {
                a[t] = row[offA[t]];
                b[t] = row[offB[t]];
            }
#pragma unroll
            for (int t = 0; t < PER; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b[t], acc[t], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        if (first + t >= ntiles) continue;
        const int row0 = pi * GRAM_PANEL + offA[t] + kr;
        const int col = pj * GRAM_PANEL + (offB[t] - (DIAG ? 0 : GRAM_PANEL)) + cc;
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(int64_t)(row0 + 4 * r) * d_pad + col] = acc[t][r];
    }
}

// grid (chunks, panel pairs), 512 threads.  ws: [chunk][d_pad][d_pad], upper tiles only.
__global__ __launch_bounds__(GRAM_THREADS) void pca_gram(const double *__restrict__ X, const double *__restrict__ mu,
                                                         int64_t n, int d, int d_pad, int64_t chunk_rows, int npanels,
                                                         double *__restrict__ ws) {
    __shared__ double xs[GRAM_SLAB * GRAM_LDW];
    __shared__ int tile_ij[64];
    int pi = 0, rem = blockIdx.y;
    while (rem >= npanels - pi) {
        rem -= npanels - pi;
        ++pi;
    }
    const int pj = pi + rem;
    const bool diag = pi == pj;
    const int tI = min(8, (d_pad - pi * GRAM_PANEL) / 16), tJ = min(8, (d_pad - pj * GRAM_PANEL) / 16);
    const int ntiles = diag ? tI * (tI + 1) / 2 : tI * tJ;
    if (threadIdx.x == 0) {
        int t = 0;
        for (int I = 0; I < tI; ++I)
            for (int J = diag ? I : 0; J < tJ; ++J) tile_ij[t++] = I << 8 | J;
    }
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * chunk_rows;
    const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
    double *out = ws + (int64_t)blockIdx.x * d_pad * d_pad;
    const int per = (ntiles + GRAM_WAVES - 1) / GRAM_WAVES;   // tiles per wave, uniform over the workgroup
#define TSNE_GRAM_CASE(P, DG)                                                               \
    case P:                                                                                 \
        gram_body<P, DG>(X, mu, d, r0, r1, ntiles, tile_ij, xs, pi, pj, d_pad, out);        \
        break;
    if (diag) {   // at most 36 tiles: 5 per wave
        switch (per) {
            TSNE_GRAM_CASE(1, true) TSNE_GRAM_CASE(2, true) TSNE_GRAM_CASE(3, true) TSNE_GRAM_CASE(4, true)
            TSNE_GRAM_CASE(5, true)
        }
    } else {
        switch (per) {
            TSNE_GRAM_CASE(1, false) TSNE_GRAM_CASE(2, false) TSNE_GRAM_CASE(3, false) TSNE_GRAM_CASE(4, false)
            TSNE_GRAM_CASE(5, false) TSNE_GRAM_CASE(6, false) TSNE_GRAM_CASE(7, false) TSNE_GRAM_CASE(8, false)
        }
    }
#undef TSNE_GRAM_CASE
}

// grid (ceil(d / 16), ceil(d / 16)), 16 x 16 threads; (a, b) with a <= b.
__global__ __launch_bounds__(256) void pca_gram_reduce(const double *__restrict__ ws, int64_t chunks, int64_t n, int d,
                                                       int d_pad, double *__restrict__ C) {
    const int b = blockIdx.x * 16 + (threadIdx.x & 15), a = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (a > b || b >= d) return;
    const int64_t stride = (int64_t)d_pad * d_pad;
    const double *p = ws + (int64_t)a * d_pad + b;
    const double v = strided_sum(p, stride, 0, 1, chunks) / (double)n;
    C[(int64_t)a * d + b] = v;
    C[(int64_t)b * d + a] = v;
}

// grid ceil(n / 64), 256 threads: lane = row, wave g takes components g, g + 4, ...,
// QN of them (the rows of vs past c_out are zero).  The next slice of X, V and
// mu is loaded into registers (unconditionally, from clamped addresses) while
// the current one is summed.  init: the scores times `scale` go to out
// (n x c_out) with upd = 0, gains = 1.
template <int QN>
__global__ __launch_bounds__(256) void pca_project(const double *__restrict__ X, const double *__restrict__ mu,
                                                   const double *__restrict__ V, int64_t n, int d, int c_out,
                                                   double scale, int init, double *__restrict__ out,
                                                   double *__restrict__ upd, double *__restrict__ gains) {
    constexpr int NST = PROJ_ROWS / 8;   // staged elements of X (and of V) per thread and slice
    __shared__ double xs[PROJ_ROWS][PROJ_SLICE + 1];
    __shared__ double vs[PCA_MAX_OUT][PROJ_SLICE];
    const int tid = threadIdx.x, r = tid & 63, g = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * PROJ_ROWS;
    const int sc = tid & (PROJ_SLICE - 1), sr = tid >> 5;   // staging: column, first row
    double acc[QN];
#pragma unroll
    for (int q = 0; q < QN; ++q) acc[q] = 0.0;
    double xv[NST], vv[NST], mv;
    auto load = [&](int j0) {
        const int64_t jl = j0 + sc < d ? j0 + sc : d - 1;
        mv = mu[jl];
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int64_t row = row0 + sr + i * 8;
            const int a = sr + i * 8;
            xv[i] = X[(row < n ? row : n - 1) * d + jl];
            vv[i] = V[(int64_t)(a < c_out ? a : c_out - 1) * d + jl];
        }
    };
    load(0);
    for (int j0 = 0; j0 < d; j0 += PROJ_SLICE) {
        const bool ok = j0 + sc < d;
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            xs[sr + i * 8][sc] = (ok && row0 + sr + i * 8 < n) ? xv[i] - mv : 0.0;
            vs[sr + i * 8][sc] = (ok && sr + i * 8 < c_out) ? vv[i] : 0.0;
        }
        __syncthreads();
        if (j0 + PROJ_SLICE < d) load(j0 + PROJ_SLICE);
        const int jn = min(PROJ_SLICE, d - j0);
        for (int jj = 0; jj < jn; ++jj) {
            const double x = xs[r][jj];
#pragma unroll
            for (int q = 0; q < QN; ++q) acc[q] = __dadd_rn(acc[q], __dmul_rn(x, vs[g + 4 * q][jj]));
        }
        __syncthreads();
    }
    const int64_t row = row0 + r;
    if (row >= n) return;
#pragma unroll
    for (int q = 0; q < QN; ++q) {
        const int a = g + 4 * q;
        if (a >= c_out) continue;
        const int64_t o = row * c_out + a;
        out[o] = init ? __dmul_rn(acc[q], scale) : acc[q];
        if (init) {
            upd[o] = 0.0;
            gains[o] = 1.0;
        }
    }
}

void check_input(const double *dX, int64_t n, int32_t d) {
    TSNE_REQUIRE(dX != nullptr, "NULL buffer");
    TSNE_REQUIRE(n >= 2, "PCA needs at least two rows");
    TSNE_REQUIRE(d >= 1, "PCA needs at least one column");
}

void check_dim(int32_t d) {
    if (d > PCA_MAX_D) fail(TSNE_ERR_UNSUPPORTED, "PCA supports at most " + std::to_string(PCA_MAX_D) + " columns");
}

void project(tsne_ctx *ctx, const double *dX, int64_t n, int32_t d, int32_t c_out, const double *d_mean,
             const double *d_comp, double scale, int init, double *d_out, double *d_upd, double *d_gains) {
    ctx->timers.reset("pca.project");
    ctx->timers.begin("pca.project", ctx->stream);
    const dim3 grid((unsigned)ceil_div(n, PROJ_ROWS)), block(256);
    const int per_wave = (c_out + 3) / 4;   // components per wave, rounded up to a power of two
#define TSNE_PROJ_CASE(Q)                                                                                             \
    pca_project<Q><<<grid, block, 0, ctx->stream>>>(dX, d_mean, d_comp, n, d, c_out, scale, init, d_out, d_upd, d_gains)
    if (per_wave <= 1) TSNE_PROJ_CASE(1);
    else if (per_wave <= 2) TSNE_PROJ_CASE(2);
    else if (per_wave <= 4) TSNE_PROJ_CASE(4);
    else if (per_wave <= 8) TSNE_PROJ_CASE(8);
    else TSNE_PROJ_CASE(16);
#undef TSNE_PROJ_CASE
    TSNE_LAUNCH_CHECK();
    ctx->timers.end("pca.project", ctx->stream);
}

// mean, covariance, host eigen-solve, the leading c_out pairs back on the
// device; the scores or (c_init > 0) the initial working set.  Returns lambda_1.
void pca_core(tsne_ctx *ctx, const double *dX, int64_t n, int32_t d, int32_t c_out, double *d_mean, double *d_comp,
              double *d_eig, double *d_scores, bool init, double *d_upd, double *d_gains) {
    double *mean = d_mean ? d_mean : ctx->ws.get<double>("pca.mean", (size_t)d);
    double *cov = ctx->ws.get<double>("pca.cov", (size_t)d * d);
    pca_covariance_device(ctx, dX, n, d, mean, cov);
    std::vector<double> hC((size_t)d * d), w((size_t)d), Vh((size_t)d * d);
    TSNE_HIP(hipMemcpyAsync(hC.data(), cov, sizeof(double) * hC.size(), hipMemcpyDeviceToHost, ctx->stream));
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
    const int rc = sym_eig(hC.data(), d, w.data(), Vh.data());
    if (rc == 1) fail(TSNE_ERR_ARG, "the covariance of the input is not finite");
    if (rc != 0) fail(TSNE_ERR_HIP, "the eigen-solver did not converge");
    if (init && !(w[0] > 0.0)) fail(TSNE_ERR_ARG, "PCA initialisation of constant data (lambda_1 <= 0)");
    double *comp = d_comp ? d_comp : ctx->ws.get<double>("pca.comp", (size_t)c_out * d);
    TSNE_HIP(hipMemcpyAsync(comp, Vh.data(), sizeof(double) * (size_t)c_out * d, hipMemcpyHostToDevice, ctx->stream));
    if (d_eig) TSNE_HIP(hipMemcpyAsync(d_eig, w.data(), sizeof(double) * (size_t)c_out, hipMemcpyHostToDevice, ctx->stream));
    if (d_scores) {
        const double scale = init ? 1e-4 / std::sqrt(w[0]) : 1.0;
        project(ctx, dX, n, d, c_out, mean, comp, scale, init ? 1 : 0, d_scores, d_upd, d_gains);
    }
    TSNE_HIP(hipStreamSynchronize(ctx->stream));   // the uploads read this call's host vectors
}

}  // namespace

int64_t pca_gram_chunk_rows(int64_t n, int32_t d) {
    const int64_t d_pad = round_up(d, 16);
    int64_t rows = PCA_GRAM_ROWS;
    while (ceil_div(n, rows) * d_pad * d_pad * (int64_t)sizeof(double) > PCA_GRAM_WS_BYTES) rows *= 2;
    return rows;
}

void pca_covariance_device(tsne_ctx *ctx, const double *dX, int64_t n, int32_t d, double *d_mean, double *d_cov) {
    check_input(dX, n, d);
    check_dim(d);
    TSNE_REQUIRE(d_mean && d_cov, "NULL buffer");
    // stage timers (tsne_ctx_stage_ms): the last call's kernels, one interval each
    StageTimers &tm = ctx->timers;
    for (const char *name : {"pca.colmean", "pca.gram", "pca.reduce"}) tm.reset(name);
    const int64_t mchunks = ceil_div(n, MEAN_ROWS);
    double *part = ctx->ws.get<double>("pca.mean_part", (size_t)(mchunks * d));
    const int d_pad = (int)round_up(d, 16);
    const int npanels = (int)ceil_div(d_pad, GRAM_PANEL);
    const int64_t rows = pca_gram_chunk_rows(n, d), chunks = ceil_div(n, rows);
    double *gws = ctx->ws.get<double>("pca.gram", (size_t)(chunks * d_pad * d_pad));
    tm.begin("pca.colmean", ctx->stream);
    pca_colmean_partial<<<dim3((unsigned)mchunks, (unsigned)ceil_div(d, 64)), dim3(256), 0, ctx->stream>>>(dX, n, d, part);
    TSNE_LAUNCH_CHECK();
    pca_colmean_final<<<dim3((unsigned)ceil_div(d, 64)), dim3(1024), 0, ctx->stream>>>(part, mchunks, n, d, d_mean);
    TSNE_LAUNCH_CHECK();
    tm.end("pca.colmean", ctx->stream);
    tm.begin("pca.gram", ctx->stream);
    pca_gram<<<dim3((unsigned)chunks, (unsigned)(npanels * (npanels + 1) / 2)), dim3(GRAM_THREADS), 0, ctx->stream>>>(
        dX, d_mean, n, d, d_pad, rows, npanels, gws);
    TSNE_LAUNCH_CHECK();
    tm.end("pca.gram", ctx->stream);
    const unsigned tb = (unsigned)ceil_div(d, 16);
    tm.begin("pca.reduce", ctx->stream);
    pca_gram_reduce<<<dim3(tb, tb), dim3(256), 0, ctx->stream>>>(gws, chunks, n, d, d_pad, d_cov);
    TSNE_LAUNCH_CHECK();
    tm.end("pca.reduce", ctx->stream);
}

void pca_device(tsne_ctx *ctx, const double *dX, int64_t n, int32_t d, int32_t c_out, double *d_mean, double *d_comp,
                double *d_eig, double *d_scores) {
    check_input(dX, n, d);
    TSNE_REQUIRE(c_out >= 1 && c_out <= std::min<int32_t>(d, PCA_MAX_OUT), "c_out must be in [1, min(d, 64)]");
    check_dim(d);
    pca_core(ctx, dX, n, d, c_out, d_mean, d_comp, d_eig, d_scores, false, nullptr, nullptr);
}

void pca_init_device(tsne_ctx *ctx, const double *dX, int64_t n, int32_t d, int32_t c, double *dY, double *dupd,
                     double *dgains) {
    if (c != 2 && c != 3) fail(TSNE_ERR_UNSUPPORTED, "n_components must be 2 or 3");
    check_input(dX, n, d);
    TSNE_REQUIRE(c <= d, "n_components exceeds the input's columns");
    check_dim(d);
    TSNE_REQUIRE(dY && dupd && dgains, "NULL buffer");
    pca_core(ctx, dX, n, d, c, nullptr, nullptr, nullptr, dY, true, dupd, dgains);
}

}  // namespace tsne
