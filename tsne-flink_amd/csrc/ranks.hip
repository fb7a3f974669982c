// ranks.hip -- exact neighbour ranks by a brute-force fp64 scan, and the
// rank-based scores of a map on top of them (trustworthiness, continuity,
// kNN recall; include/tsne_hip.h "scoring a map").
//
// rank_A(i, j) = 1 + #{ l != i : (dkey(D(i,l)), l) < (dkey(D(i,j)), j) }, D the
// exact breeze metric of metric.hpp -- the position of j in row i of
// tsne_knn(A, k = n - 1).  For s scored rows with m candidates each:
//   1. thresholds: one wave per row computes (dkey(D(i,j)), j) of its m
//      candidates with exact_metric, bitonic-sorts them in LDS and keeps the
//      permutation back to the caller's order (the row itself sorts first,
//      below every real pair: nothing counts for it).
//   2. scan: all s x n pairs on the fp64 VALU (no MFMA: the sum over the
//      coordinates must be exact_metric's sequential sub, mul, add).  A
//      256-thread workgroup takes RQ = 64 scored rows and a chunk of the n
//      rows in tiles of RR = 128; both sides are staged through LDS in slices
//      of RS = 16 coordinates, coordinate-major, and each lane owns a 4 x 8
//      (query x row) tile of accumulators that the coordinates pass through in
//      index order.  A finished pair is compared with its query's largest
//      threshold (as doubles: a superset test); the few that pass take the
//      exact (key, index) binary search over the query's sorted thresholds
//      and bump one bucket of the query's histogram.
//      Histogram rule: m <= RHIST_MAX = 384 keeps the 64 x m int32 buckets
//      in LDS (<= 96 KB beside the 26.5 KB of staging) and adds the non-zero
//      ones to the global buckets at the end of the chunk; a larger m (up to
//      RANKS_MAX_M) bumps the global buckets directly.  The thresholds
//      themselves stay in global memory (L2): only passing pairs read them.
//   3. finish: one wave per row prefix-sums its buckets and writes
//      1 + count through the permutation (0 for the row itself).
// The counts are integers, so a rank does not depend on the tile shape, the
// launch order or the other rows of the call.
#include <algorithm>

#include "common.hpp"
#include "metric.hpp"
#include "ranks.hpp"

namespace tsne {
namespace {

constexpr int RQ = 64;     // scored rows per workgroup
constexpr int RR = 128;    // scanned rows per tile
constexpr int RS = 16;     // coordinates per LDS slice
constexpr int RHIST_MAX = 384;   // m up to which the histograms live in LDS
// staging + per-query state: Qs, Rs, nq, nr (two tiles), tmax, qid
constexpr size_t SCAN_LDS = sizeof(double) * (RS * RQ + RS * RR + RQ + 2 * RR + RQ) + sizeof(int64_t) * RQ;

__device__ __forceinline__ double dkey_inv(uint64_t k) {
    const uint64_t u = (k & 0x8000000000000000ull) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __longlong_as_double((long long)u);
}

// breeze norm() of every row (the cosine metric; prep_rows' norm64)
__global__ void ranks_norms(const double *__restrict__ A, int64_t n, int32_t d, double *__restrict__ norm) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) norm[i] = exact_norm(A + i * d, d);
}

// One wave per scored row: sorted (key, j) thresholds, the permutation, and
// the largest threshold's distance for the scan's first test.
__global__ __launch_bounds__(64) void ranks_thresholds(
    const double *__restrict__ A, int32_t d, int32_t metric, const double *__restrict__ norm,
    const int64_t *__restrict__ rows, const int32_t *__restrict__ cand, int32_t m, uint64_t *__restrict__ tkey,
    int32_t *__restrict__ tj, int32_t *__restrict__ perm, double *__restrict__ tmax) {
    __shared__ uint64_t ks[RANKS_MAX_M];
    __shared__ int32_t js[RANKS_MAX_M];
    __shared__ int32_t es[RANKS_MAX_M];
    const int lane = threadIdx.x;
    const int64_t a = blockIdx.x;
    const int64_t i = rows ? rows[a] : a;
    const bool cosine = metric == TSNE_METRIC_COSINE;
    int P = 64;
    while (P < m) P <<= 1;
    const double *xq = A + i * d;
    const double nqv = cosine ? norm[i] : 0.0;
    for (int e = lane; e < P; e += 64) {
        if (e < m) {
            const int32_t j = cand[a * m + e];
            if (j == i) {   // below every real pair: its count stays 0
                ks[e] = 0;
                js[e] = -1;
            } else {
                ks[e] = dkey(exact_metric(xq, A + (int64_t)j * d, d, metric, nqv, cosine ? norm[j] : 0.0));
                js[e] = j;
            }
            es[e] = e;
        } else {
            ks[e] = ~0ull;
            js[e] = 0x7FFFFFFF;
            es[e] = 0;
        }
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int e = lane; e < P / 2; e += 64) {
                const int lo = 2 * e - (e & (stride - 1));
                const int hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const uint64_t ka = ks[lo], kb = ks[hi];
                const int32_t ja = js[lo], jb = js[hi];
                const bool gt = (ka > kb) || (ka == kb && ja > jb);
                if (gt == up) {
                    ks[lo] = kb; ks[hi] = ka;
                    js[lo] = jb; js[hi] = ja;
                    const int32_t t = es[lo]; es[lo] = es[hi]; es[hi] = t;
                }
            }
            __syncthreads();
        }
    }
    for (int t = lane; t < m; t += 64) {
        tkey[a * m + t] = ks[t];
        tj[a * m + t] = js[t];
        perm[a * m + t] = es[t];
    }
    if (lane == 0) tmax[a] = js[m - 1] < 0 ? -__builtin_inf() : dkey_inv(ks[m - 1]);
}

// The scan (header).  Block b: query tile b % qtiles, row chunk b / qtiles
// (neighbouring blocks stream the same rows through L2).  METRIC is the
// tsne metric id; LHIST: the histograms in LDS.
template <int METRIC, bool LHIST>
__global__ __launch_bounds__(256) void ranks_scan(
    const double *__restrict__ A, int64_t n, int32_t d, const double *__restrict__ norm,
    const int64_t *__restrict__ rows, int64_t s, int32_t m, const uint64_t *__restrict__ tkey,
    const int32_t *__restrict__ tj, const double *__restrict__ tmax, int64_t qtiles, int64_t ntiles,
    int64_t tiles_per_chunk, int32_t *__restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *Qs = reinterpret_cast<double *>(smem);   // [RS][RQ]
    double *Rs = Qs + RS * RQ;                       // [RS][RR]
    double *nq_s = Rs + RS * RR;                     // [RQ]
    double *nr_s = nq_s + RQ;                        // [2][RR]: by tile parity
    double *tmax_s = nr_s + 2 * RR;                  // [RQ]
    int64_t *qid_s = reinterpret_cast<int64_t *>(tmax_s + RQ);   // [RQ], -1: no such row
    int32_t *hist_s = reinterpret_cast<int32_t *>(qid_s + RQ);   // [RQ][m] (LHIST)
    constexpr bool COS = METRIC == TSNE_METRIC_COSINE;

    const int tid = threadIdx.x;
    const int tq = tid >> 4, tr = tid & 15;   // the lane's queries 4 tq + a, rows 32 u + 2 tr + h
    const int64_t qt = blockIdx.x % qtiles, ch = blockIdx.x / qtiles;
    const int64_t qbase = qt * RQ;
    if (tid < RQ) {
        const int64_t a = qbase + tid;
        const bool valid = a < s;
        const int64_t id = valid ? (rows ? rows[a] : a) : -1;
        qid_s[tid] = id;
        tmax_s[tid] = valid ? tmax[a] : -__builtin_inf();
        nq_s[tid] = (COS && valid) ? norm[id] : 1.0;
    }
    if (LHIST)
        for (int e = tid; e < RQ * m; e += 256) hist_s[e] = 0;
    __syncthreads();

    const int64_t it0 = ch * tiles_per_chunk, it1 = min(ntiles, it0 + tiles_per_chunk);
    const bool qconst = d <= RS;   // one slice: the queries are staged once
    // staging shares: Q element e of 4 is (query tid & 63, coordinate (tid >> 6) + 4 e),
    // R element e of 8 is (row tid & 127, coordinate (tid >> 7) + 2 e)
    const int sq = tid & 63, sqc = tid >> 6, sr = tid & 127, src = tid >> 7;
    const int64_t myq = qid_s[sq];
    for (int64_t it = it0; it < it1; ++it) {
        const int64_t r0 = it * RR;
        const int64_t myr = r0 + sr;
        double *nr = nr_s + (it & 1) * RR;
        if (COS && tid < RR) nr[tid] = (r0 + tid) < n ? norm[r0 + tid] : 1.0;
        double acc[4][8];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) acc[a][b] = 0.0;
        const bool stage_q = !qconst || it == it0;
        double pq[4], pr[8];
        auto fetch = [&](int32_t c0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int32_t c = c0 + sqc + 4 * e;
                pq[e] = (stage_q && myq >= 0 && c < d) ? A[myq * d + c] : 0.0;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int32_t c = c0 + src + 2 * e;
                pr[e] = (myr < n && c < d) ? A[myr * d + c] : 0.0;
            }
        };
        fetch(0);
        for (int32_t c0 = 0; c0 < d; c0 += RS) {
            if (stage_q) {
#pragma unroll
                for (int e = 0; e < 4; ++e) Qs[(sqc + 4 * e) * RQ + sq] = pq[e];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) Rs[(src + 2 * e) * RR + sr] = pr[e];
            __syncthreads();
            if (c0 + RS < d) fetch(c0 + RS);
            const int cn = min(RS, d - c0);
            for (int c = 0; c < cn; ++c) {
                double q[4], r[8];
#pragma unroll
                for (int a = 0; a < 4; ++a) q[a] = Qs[c * RQ + 4 * tq + a];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    r[2 * u] = Rs[c * RR + 32 * u + 2 * tr];
                    r[2 * u + 1] = Rs[c * RR + 32 * u + 2 * tr + 1];
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 8; ++b) {
                        if (COS) {
                            acc[a][b] = __dadd_rn(acc[a][b], __dmul_rn(q[a], r[b]));
                        } else {
                            const double df = __dsub_rn(q[a], r[b]);
                            acc[a][b] = __dadd_rn(acc[a][b], __dmul_rn(df, df));
                        }
                    }
            }
            __syncthreads();
        }
        // count the tile's pairs
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int ql = 4 * tq + a;
            const double tm = tmax_s[ql];
            const double nqv = nq_s[ql];
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int rl = 32 * (b >> 1) + 2 * tr + (b & 1);
                const double v = metric_finish(acc[a][b], METRIC, nqv, COS ? nr[rl] : 1.0);
                if (v > tm) continue;   // above the largest threshold (NaN on either side: the exact test)
                const int64_t l = r0 + rl, i = qid_s[ql];
                if (l >= n || i < 0 || l == i) continue;
                const uint64_t K = dkey(v);
                const int64_t ag = qbase + ql;
                const uint64_t *tk = tkey + ag * m;
                const int32_t *tjj = tj + ag * m;
                int lo = 0, hi = m;   // lo -> the number of thresholds <= (K, l)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const uint64_t kk = tk[mid];
                    if (kk < K || (kk == K && (int64_t)tjj[mid] <= l)) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < m) {
                    if (LHIST) atomicAdd(&hist_s[ql * m + lo], 1);
                    else atomicAdd(&hist[ag * m + lo], 1);
                }
            }
        }
    }
    if (LHIST) {
        __syncthreads();
        for (int e = tid; e < RQ * m; e += 256) {
            const int32_t v = hist_s[e];
            if (v) atomicAdd(&hist[(qbase + e / m) * m + e % m], v);   // only rows < s were bumped
        }
    }
}

// One wave per scored row: inclusive prefix sum of its buckets, written
// through the permutation.
__global__ __launch_bounds__(64) void ranks_finish(const int32_t *__restrict__ hist, const int32_t *__restrict__ tj,
                                                   const int32_t *__restrict__ perm, int32_t m,
                                                   int32_t *__restrict__ rank) {
    const int lane = threadIdx.x;
    const int64_t a = blockIdx.x;
    int32_t carry = 0;
    for (int base = 0; base < m; base += 64) {
        const int t = base + lane;
        int32_t incl = t < m ? hist[a * m + t] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        incl += carry;
        if (t < m) rank[a * m + perm[a * m + t]] = tj[a * m + t] < 0 ? 0 : 1 + incl;
        carry = __shfl(incl, 63, 64);
    }
}

template <int METRIC>
void launch_scan(tsne_ctx *ctx, bool lhist, int64_t blocks, size_t lds, const double *dA, int64_t n, int32_t d,
                 const double *norm, const int64_t *d_rows, int64_t s, int32_t m, const uint64_t *tkey,
                 const int32_t *tj, const double *tmax, int64_t qtiles, int64_t ntiles, int64_t tpc, int32_t *hist) {
    if (lhist) {
        TSNE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&ranks_scan<METRIC, true>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((ranks_scan<METRIC, true>), dim3((unsigned)blocks), dim3(256), lds, ctx->stream, dA, n, d,
                           norm, d_rows, s, m, tkey, tj, tmax, qtiles, ntiles, tpc, hist);
    } else {
        hipLaunchKernelGGL((ranks_scan<METRIC, false>), dim3((unsigned)blocks), dim3(256), lds, ctx->stream, dA, n, d,
                           norm, d_rows, s, m, tkey, tj, tmax, qtiles, ntiles, tpc, hist);
    }
    TSNE_LAUNCH_CHECK();
}

// ------------------------------------------------------------- the scores
__global__ void quality_gather(const double *__restrict__ X, int32_t d, const int64_t *__restrict__ rows, int64_t s,
                               double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < s * d) out[e] = X[rows[e / d] * d + e % d];
}

// A cross-kNN row of k + 1 entries (the point itself among the candidates)
// -> the point's tsne_knn row: its own id dropped, or the last entry when it
// is not among them.
__global__ void quality_drop_self(const int32_t *__restrict__ idx1, const int64_t *__restrict__ rows, int64_t s,
                                  int32_t k, int32_t *__restrict__ out) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= s) return;
    const int64_t i = rows[a];
    const int32_t *in = idx1 + a * (k + 1);
    int32_t w = 0;
    for (int32_t t = 0; t <= k && w < k; ++t)
        if (in[t] != i) out[a * k + w++] = in[t];
}

// One wave per scored row: its three sums.  The ids of a list are distinct,
// so the k x k compare counts the intersection.
__global__ __launch_bounds__(64) void quality_rows(const int32_t *__restrict__ NX, const int32_t *__restrict__ NY,
                                                   const int32_t *__restrict__ RX, const int32_t *__restrict__ RY,
                                                   int32_t k, int64_t *__restrict__ row_sums) {
    const int lane = threadIdx.x;
    const int64_t a = blockIdx.x;
    long long st = 0, sc = 0, sr = 0;
    for (int t = lane; t < k; t += 64) {
        st += max(0, RX[a * k + t] - k);
        sc += max(0, RY[a * k + t] - k);
        const int32_t j = NY[a * k + t];
        for (int u = 0; u < k; ++u) sr += NX[a * k + u] == j;
    }
    st = wave_sum(st);
    sc = wave_sum(sc);
    sr = wave_sum(sr);
    if (lane == 0) {
        row_sums[a * 3] = st;
        row_sums[a * 3 + 1] = sc;
        row_sums[a * 3 + 2] = sr;
    }
}

// One workgroup: thread t sums rows t, t + 256, ..., then a tree over the threads.
__global__ __launch_bounds__(256) void quality_reduce(const int64_t *__restrict__ row_sums, int64_t s,
                                                      int64_t *__restrict__ sums) {
    __shared__ long long part[3][256];
    const int tid = threadIdx.x;
    long long v[3] = {0, 0, 0};
    for (int64_t a = tid; a < s; a += 256)
        for (int c = 0; c < 3; ++c) v[c] += row_sums[a * 3 + c];
    for (int c = 0; c < 3; ++c) part[c][tid] = v[c];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o)
            for (int c = 0; c < 3; ++c) part[c][tid] += part[c][tid + o];
        __syncthreads();
    }
    if (tid < 3) sums[tid] = part[tid][0];
}

}  // namespace

void ranks_device(tsne_ctx *ctx, const double *dA, int64_t n, int32_t d, int32_t metric, const int64_t *d_rows,
                  int64_t s, const int32_t *d_cand, int32_t m, int32_t *d_rank, bool reset_timer) {
    TSNE_REQUIRE(n >= 1 && n < (int64_t)INT32_MAX, "n must be in [1, 2^31 - 1)");
    TSNE_REQUIRE(d >= 1, "dimension must be positive");
    TSNE_REQUIRE(metric >= 0 && metric <= 2, "unknown metric");
    TSNE_REQUIRE(s >= 0 && s < (int64_t)INT32_MAX, "bad number of rows");
    TSNE_REQUIRE(d_rows != nullptr || s <= n, "rows is NULL: at most n rows");
    TSNE_REQUIRE(m >= 1, "m must be positive");
    if (m > RANKS_MAX_M) fail(TSNE_ERR_UNSUPPORTED, "at most 1024 candidates per row");
    if (reset_timer) ctx->timers.reset("ranks.scan");
    if (s == 0) return;
    TSNE_REQUIRE(dA != nullptr && d_cand != nullptr && d_rank != nullptr, "NULL buffer");
    hipStream_t st = ctx->stream;
    Workspace &ws = ctx->ws;
    double *norm = nullptr;
    if (metric == TSNE_METRIC_COSINE) {
        norm = ws.get<double>("ranks.norm", (size_t)n);
        hipLaunchKernelGGL(ranks_norms, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, dA, n, d, norm);
        TSNE_LAUNCH_CHECK();
    }
    const size_t sm = (size_t)s * (size_t)m;
    uint64_t *tkey = ws.get<uint64_t>("ranks.tkey", sm);
    int32_t *tj = ws.get<int32_t>("ranks.tj", sm);
    int32_t *perm = ws.get<int32_t>("ranks.perm", sm);
    int32_t *hist = ws.get<int32_t>("ranks.hist", sm);
    double *tmax = ws.get<double>("ranks.tmax", (size_t)s);
    TSNE_HIP(hipMemsetAsync(hist, 0, sizeof(int32_t) * sm, st));
    hipLaunchKernelGGL(ranks_thresholds, dim3((unsigned)s), dim3(64), 0, st, dA, d, metric, norm, d_rows, d_cand, m,
                       tkey, tj, perm, tmax);
    TSNE_LAUNCH_CHECK();
    // row chunks: about 8 workgroups per CU in all, a chunk at least one tile
    const int64_t qtiles = ceil_div(s, RQ), ntiles = ceil_div(n, RR);
    int64_t chunks = std::min<int64_t>(ntiles, std::max<int64_t>(1, ceil_div((int64_t)ctx->cu_count * 8, qtiles)));
    const int64_t tpc = ceil_div(ntiles, chunks);
    chunks = ceil_div(ntiles, tpc);
    const bool lhist = m <= RHIST_MAX;
    const size_t lds = SCAN_LDS + (lhist ? sizeof(int32_t) * (size_t)RQ * m : 0);
    const int64_t blocks = qtiles * chunks;
    ctx->timers.begin("ranks.scan", st);
    if (metric == TSNE_METRIC_SQEUCLIDEAN)
        launch_scan<TSNE_METRIC_SQEUCLIDEAN>(ctx, lhist, blocks, lds, dA, n, d, norm, d_rows, s, m, tkey, tj, tmax,
                                             qtiles, ntiles, tpc, hist);
    else if (metric == TSNE_METRIC_EUCLIDEAN)
        launch_scan<TSNE_METRIC_EUCLIDEAN>(ctx, lhist, blocks, lds, dA, n, d, norm, d_rows, s, m, tkey, tj, tmax,
                                           qtiles, ntiles, tpc, hist);
    else
        launch_scan<TSNE_METRIC_COSINE>(ctx, lhist, blocks, lds, dA, n, d, norm, d_rows, s, m, tkey, tj, tmax, qtiles,
                                        ntiles, tpc, hist);
    ctx->timers.end("ranks.scan", st);
    hipLaunchKernelGGL(ranks_finish, dim3((unsigned)s), dim3(64), 0, st, hist, tj, perm, m, d_rank);
    TSNE_LAUNCH_CHECK();
}

void quality_device(tsne_ctx *ctx, const double *dX, int64_t n, int32_t d, int32_t metric, const double *dY, int32_t c,
                    int32_t k, const int64_t *d_rows, int64_t s, int64_t *d_row_sums, int64_t sums_out[3]) {
    TSNE_REQUIRE(dX != nullptr && dY != nullptr && sums_out != nullptr, "NULL buffer");
    TSNE_REQUIRE(n >= 2 && n < (int64_t)INT32_MAX, "n must be in [2, 2^31 - 1)");
    TSNE_REQUIRE(d >= 1 && c >= 1, "dimensions must be positive");
    TSNE_REQUIRE(metric >= 0 && metric <= 2, "unknown metric");
    TSNE_REQUIRE(k >= 1, "k must be positive");
    TSNE_REQUIRE(2 * n - 3 * (int64_t)k - 1 > 0, "the scores need 2 n - 3 k - 1 > 0");
    TSNE_REQUIRE(s >= 1, "no rows to score");
    TSNE_REQUIRE(d_rows != nullptr || s == n, "rows is NULL: s must equal n");
    if (k > 896) fail(TSNE_ERR_UNSUPPORTED, "k too large (max 896)");   // tsne_knn's limit
    hipStream_t st = ctx->stream;
    Workspace &ws = ctx->ws;
    const size_t sk = (size_t)s * (size_t)k;
    int32_t *NX = ws.get<int32_t>("quality.nx", sk), *NY = ws.get<int32_t>("quality.ny", sk);
    // the neighbour lists: tsne_knn's rows of the scored points in X and in Y
    auto lists = [&](const double *A, int32_t da, int32_t mt, int32_t *out) {
        if (!d_rows) {
            double *dist = ws.get<double>("quality.dist", sk);
            knn_device(ctx, A, n, da, mt, k, 0, n, out, dist);
            return;
        }
        const size_t sk1 = (size_t)s * (size_t)(k + 1);   // k + 1 <= n: 2 n > 3 k + 1
        double *Aq = ws.get<double>("quality.rows", (size_t)s * da);
        int32_t *idx1 = ws.get<int32_t>("quality.idx1", sk1);
        double *dist = ws.get<double>("quality.dist", sk1);
        hipLaunchKernelGGL(quality_gather, dim3((unsigned)ceil_div(s * da, 256)), dim3(256), 0, st, A, da, d_rows, s, Aq);
        TSNE_LAUNCH_CHECK();
        knn_cross_device(ctx, A, n, Aq, s, da, mt, k + 1, idx1, dist);
        hipLaunchKernelGGL(quality_drop_self, dim3((unsigned)ceil_div(s, 256)), dim3(256), 0, st, idx1, d_rows, s, k, out);
        TSNE_LAUNCH_CHECK();
    };
    // stage timers "quality.lists_x" / "quality.lists_y": the two neighbour-list
    // stages (host waits inside the kNN included); their exact-scan fallbacks
    // are the counters "quality.fallback_x" / "quality.fallback_y"
    auto timed = [&](const char *name, const double *A, int32_t da, int32_t mt, int32_t *out, int64_t *fallbacks) {
        ctx->timers.reset(name);
        ctx->timers.begin(name, st);
        lists(A, da, mt, out);
        ctx->timers.end(name, st);
        *fallbacks = ctx->knn_fallback_queries;
    };
    timed("quality.lists_x", dX, d, metric, NX, &ctx->quality_fallbacks[0]);
    timed("quality.lists_y", dY, c, TSNE_METRIC_SQEUCLIDEAN, NY, &ctx->quality_fallbacks[1]);
    int32_t *RX = ws.get<int32_t>("quality.rx", sk), *RY = ws.get<int32_t>("quality.ry", sk);
    ranks_device(ctx, dX, n, d, metric, d_rows, s, NY, k, RX, true);                      // "ranks.scan" [0]: on X
    ranks_device(ctx, dY, n, c, TSNE_METRIC_SQEUCLIDEAN, d_rows, s, NX, k, RY, false);    // [1]: on Y
    int64_t *rs = d_row_sums ? d_row_sums : ws.get<int64_t>("quality.row_sums", (size_t)s * 3);
    int64_t *sums = ws.get<int64_t>("quality.sums", 3);
    hipLaunchKernelGGL(quality_rows, dim3((unsigned)s), dim3(64), 0, st, NX, NY, RX, RY, k, rs);
    hipLaunchKernelGGL(quality_reduce, dim3(1), dim3(256), 0, st, rs, s, sums);
    TSNE_LAUNCH_CHECK();
    TSNE_HIP(hipMemcpyAsync(sums_out, sums, sizeof(int64_t) * 3, hipMemcpyDeviceToHost, st));
    TSNE_HIP(hipStreamSynchronize(st));
}

}  // namespace tsne
