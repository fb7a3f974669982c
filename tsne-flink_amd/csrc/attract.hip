// attract.hip -- the attraction of the gradient on gfx950 (TsneHelpers.scala:
// 269-306): attr_i = sum_j ex P_ij q_ij (y_i - y_j) over a rank's rows of P,
// with the KL terms in loss launches.  attract_rows / attract3 gather Y_j over
// the CSR rows; attract_tiles (its pipe and stream forms, attract_tiles3) read
// Y_j from LDS over the tiled layout that attract_layout_build makes of the
// same rows.  optimize.hip calls attract_launch_2d / attract_launch_3d.
#include <hipcub/hipcub.hpp>

#include "attract.hpp"

namespace tsne {
namespace {

// q = 1 / (1 + metric(y_i, y_j)) with the input metric on 2-D points
// (TsneHelpers.scala:293), metric fixed at compile time; v_rcp_f64 + two
// Newton steps.
template <int MET>
__device__ __forceinline__ double qterm_t(double ax, double ay, double bx, double by, double &x) {
    double m;
    if (MET == TSNE_METRIC_COSINE) {
        const double dt = __dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by));
        const double na = sqrt(__dadd_rn(__dmul_rn(ax, ax), __dmul_rn(ay, ay)));
        const double nb = sqrt(__dadd_rn(__dmul_rn(bx, bx), __dmul_rn(by, by)));
        m = 1.0 - dt / (na * nb);
    } else {
        const double dx = __dsub_rn(ax, bx), dy = __dsub_rn(ay, by);
        const double s2 = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
        m = MET == TSNE_METRIC_EUCLIDEAN ? sqrt(s2) : s2;
    }
    x = 1.0 + m;
    double r = __builtin_amdgcn_rcp(x);
    r = __fma_rn(r, __fma_rn(-x, r, 1.0), r);
    r = __fma_rn(r, __fma_rn(-x, r, 1.0), r);
    return r;
}
// The tiled attraction's q (attract_tiles), given d = a - b: the sqeuclidean
// 1 + |d|^2 as an FMA chain and v_rcp_f64 + one Newton step (within 11 ulp,
// as recip_bh) -- 4 fp64 operations fewer per entry than qterm_t; x = 1 + metric.
template <int MET>
__device__ __forceinline__ double qforce_t(double ax, double ay, double bx, double by, double dx, double dy,
                                           double &x) {
    if (MET == TSNE_METRIC_COSINE) {
        const double dt = __dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by));
        const double na = sqrt(__dadd_rn(__dmul_rn(ax, ax), __dmul_rn(ay, ay)));
        const double nb = sqrt(__dadd_rn(__dmul_rn(bx, bx), __dmul_rn(by, by)));
        x = 1.0 + (1.0 - dt / (na * nb));
    } else if (MET == TSNE_METRIC_EUCLIDEAN) {
        x = 1.0 + sqrt(__fma_rn(dx, dx, dy * dy));
    } else {
        x = __fma_rn(dx, dx, __fma_rn(dy, dy, 1.0));
    }
    const double r = __builtin_amdgcn_rcp(x);
    return __fma_rn(r, __fma_rn(-x, r, 1.0), r);
}
template <int MET>
__device__ __forceinline__ double qterm_t(double ax, double ay, double bx, double by) {
    double x;
    return qterm_t<MET>(ax, ay, bx, by, x);
}

// ln x in fp64 for the KL terms (the loss), ~4x fewer instructions than the
// libm log: x = 2^e m with m in [1/sqrt2, sqrt2), ln m = 2 atanh(s),
// s = (m - 1) / (m + 1) (|s| <= 0.1716, v_rcp_f64 + two Newton steps), the
// odd series to s^21 (remainder < 3e-17 relative), e ln2 in two parts
// (fdlibm's split).  Within a few ulp of log(); zero, negative, infinite
// and NaN arguments take log() itself (0 ln 0 stays NaN).
__device__ __forceinline__ double log_kl(double x) {
    if (!(x >= 0x1p-1022 && x < INFINITY)) return log(x);
    const long long b = __double_as_longlong(x);
    int e = (int)((b >> 52) & 0x7ff) - 1023;
    double m = __longlong_as_double((b & 0x000fffffffffffffll) | 0x3ff0000000000000ll);
    if (m > 1.4142135623730951) { m *= 0.5; ++e; }
    const double f = m - 1.0;   // exact
    const double d = 2.0 + f;
    double r = __builtin_amdgcn_rcp(d);
    r = __fma_rn(r, __fma_rn(-d, r, 1.0), r);
    r = __fma_rn(r, __fma_rn(-d, r, 1.0), r);
    const double s = f * r, s2 = s * s;
    double p = 2.0 / 21.0;
    p = __fma_rn(p, s2, 2.0 / 19.0);
    p = __fma_rn(p, s2, 2.0 / 17.0);
    p = __fma_rn(p, s2, 2.0 / 15.0);
    p = __fma_rn(p, s2, 2.0 / 13.0);
    p = __fma_rn(p, s2, 2.0 / 11.0);
    p = __fma_rn(p, s2, 2.0 / 9.0);
    p = __fma_rn(p, s2, 2.0 / 7.0);
    p = __fma_rn(p, s2, 2.0 / 5.0);
    p = __fma_rn(p, s2, 2.0 / 3.0);
    const double lnm = __fma_rn(s * s2, p, 2.0 * s);
    const double de = (double)e;
    return __fma_rn(de, 6.93147180369123816490e-01, __fma_rn(de, 1.90821492927058770002e-10, lnm));
}

// Attraction over the CSR rows [r0, r1) (TsneHelpers.scala:269-306):
// attr_i = sum_j ex P_ij q_ij (y_i - y_j), and with LOSS the KL terms
// ex P_ij ln(ex P_ij / (q_ij / Z)).  LPR lanes per row, 64/LPR rows per wave
// step; each lane issues U (col, val) loads and then U dependent Y_j gathers
// before any arithmetic, so a row of <= LPR*U entries costs two memory round
// trips.  Tail slots gather Y_i with P = 0 (exact no-ops in the sums).
// Persistent, XCD-partitioned grid (gridDim.x a multiple of 8): the blocks
// the dispatcher places on XCD x (blockIdx % 8 == x) stride over the x-th
// contiguous eighth of the Morton-ordered rows, so that XCD's L2 holds the
// spatially local Y_j of its rows, and waves stay resident across rows (PMC:
// one-row-per-wave launches kept only ~3.7 waves per SIMD in flight).
template <int LPR, int U, bool LOSS, int MET>
__global__ __launch_bounds__(256) void attract_rows(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
    int64_t r0, int64_t r1, const double *__restrict__ Y, const double *__restrict__ scal, double ex,
    double2 *__restrict__ attr, double *__restrict__ lpart) {
    __shared__ double sl[4];
    constexpr int RPW = 64 / LPR;   // rows per wave step
    const int sub = threadIdx.x & (LPR - 1);
    const int x = blockIdx.x % NUM_XCD;
    const int64_t bpx = gridDim.x / NUM_XCD;                   // blocks per XCD
    const int64_t nrows = r1 - r0;
    const int64_t q0 = r0 + nrows * x / NUM_XCD, q1 = r0 + nrows * (x + 1) / NUM_XCD;
    const int64_t wv = (int64_t)(blockIdx.x / NUM_XCD) * 4 + (threadIdx.x >> 6);
    const int64_t nwv = bpx * 4;
    const int rsub = (threadIdx.x & 63) / LPR;
    const double Z = LOSS ? scal[0] : 1.0;
    double lsum = 0.0;
    for (int64_t i = q0 + wv * RPW + rsub; i - rsub < q1; i += nwv * RPW) {
        const bool live = i < q1;
        double fx = 0.0, fy = 0.0;
        double yx = 0.0, yy = 0.0;
        if (live) {
            const double2 yi = *reinterpret_cast<const double2 *>(Y + 2 * i);
            yx = yi.x; yy = yi.y;
            const int64_t e1 = row_ptr[i + 1];
            for (int64_t e = row_ptr[i] + sub; e < e1; e += LPR * U) {
                int32_t j[U];
                double pv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t o = e + LPR * u;
                    const bool in = o < e1;
                    j[u] = in ? col[o] : (int32_t)i;
                    pv[u] = in ? val[o] : 0.0;
                }
                double jx[U], jy[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const double2 yj = *reinterpret_cast<const double2 *>(Y + 2 * (int64_t)j[u]);
                    jx[u] = yj.x; jy[u] = yj.y;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const double pij = __dmul_rn(pv[u], ex);
                    const double q = qterm_t<MET>(yx, yy, jx[u], jy[u]);
                    const double sc = __dmul_rn(pij, q);
                    fx = __dadd_rn(fx, __dmul_rn(sc, __dsub_rn(yx, jx[u])));
                    fy = __dadd_rn(fy, __dmul_rn(sc, __dsub_rn(yy, jy[u])));
                    if (LOSS && e + LPR * u < e1) lsum += pij * log(pij / (q / Z));
                }
            }
        }
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) {
            fx += __shfl_xor(fx, o, LPR);
            fy += __shfl_xor(fy, o, LPR);
        }
        if (live && sub == 0) attr[i - r0] = make_double2(fx, fy);
    }
    if (LOSS) {
        lsum = wave_sum(lsum);
        if (lane_id() == 0) sl[threadIdx.x >> 6] = lsum;
        __syncthreads();
        if (threadIdx.x == 0) lpart[blockIdx.x] = (sl[0] + sl[1]) + (sl[2] + sl[3]);
    }
}

// ---- Tiled attraction (the optimizer's own rows of P, rebuilt with the labels)
// attract_rows is bound by its Y_j gathers: 16 B from a random line of a
// 1.6 MB blob of Y per entry, each an L1 miss served by the L2, at the CU's
// outstanding-miss limit (~0.11 misses/cycle/CU) -- 0.17 of the HBM roofline.
// Here the owned rows are cut into row blocks of RB rows and their entries
// regrouped by column window of W labels.  A "tile" (row block, window) is
// processed by one workgroup: it copies the window's Y into LDS (coalesced
// 16-byte loads, from L2), then sums the tile's entries with Y_j from LDS.
// Within a tile each row is one lane of a 64-row slice, the tile's rows sorted
// by their entry count (descending), and a slice is stored in jagged-diagonal
// order: step k holds the k-th entry of every lane whose row has more than k,
// contiguously (those lanes are a prefix, as the counts descend) -- the
// loads of a step are coalesced and no slot is padding.  Per entry only the
// bytes of a CSR pair cross HBM: a 16-bit column offset within the window and
// the value (10 B instead of 12).  A lane sums its row's entries of the tile
// in the row's own order and adds the sum to the row's LDS accumulator; every
// row has exactly one lane per tile, so nothing is shared and every sum runs
// in one fixed order (bit-reproducible).
template <int RB_, int W_, int NT_>
struct ATCfg {
    static constexpr int RB = RB_, W = W_, NT = NT_, WAVES = NT_ / 64;
    static constexpr int ROWBITS = __builtin_ctz(RB_);
    static_assert((RB_ & (RB_ - 1)) == 0 && RB_ <= 4096 && W_ <= 65536, "tile packing");
};
// Measured at C3 (window loss launch / non-loss launch): 4096 x 5888 1.12 /
// 0.77 ms, 4096 x 5632 1.45 / 0.79 (before the division-free loss), 2048 x
// 3840 1.59 / 1.14, 1024 x 3840 (2 workgroups per CU) 2.28 / 1.13: fewer,
// longer row segments per tile win over occupancy.
// The row block shrinks with the owned rows (a rank of a multi-GPU run) so
// that the grid still covers the CUs: the largest of 4096 / 2048 / 1024 / 512
// rows giving at least one workgroup per CU.
using ATCfg0 = ATCfg<512, 5888, 1024>;    // 102 KB LDS
using ATCfg1 = ATCfg<1024, 5888, 1024>;   // 110 KB
using ATCfg2 = ATCfg<2048, 5888, 1024>;   // 126 KB
using ATCfg3 = ATCfg<4096, 5888, 1024>;   // 156 KB
// 3-D (attract_tiles3): 24-byte points, so a smaller window
using ATCfg3D = ATCfg<2048, 4096, 1024>;   // 96 KB window + 48 KB accumulators
using ATCfg3Ds = ATCfg<512, 4096, 1024>;   // 96 + 12 KB: a rank's share of the rows
#ifndef AT_DIAG
#define AT_DIAG 0   // 1 / 2 / 3: diagnostic builds of attract_tiles (timing only; see DESIGN.md 6, rounds 5 and 6)
#endif
#ifndef AT_UNROLL
#define AT_UNROLL 12
#endif
constexpr int AT_U = AT_UNROLL;   // jagged steps whose loads are issued together
#ifndef AT_NT
#define AT_NT 1   // attract_tiles' entry loads nontemporal (round 6)
#endif
constexpr int AT_LENBITS = 20;    // slice lane word: local row << 20 | entries in the tile

constexpr uint32_t AT_OOB = 0x80000000u;   // >= the descriptors' range: reads 0

__device__ __forceinline__ __amdgpu_buffer_rsrc_t at_rsrc(const void *p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), (short)0, 0x7ffffff0, 0x00020000);
}
// the tile window into LDS: all loads before the first store, every store
// unconditional (indices past the window clamped onto its last point, whose
// writers all hold the same value), so no load can sink into a branch
template <int WN, int NT>
__device__ __forceinline__ void at_window_regs(double2 (&yv)[(WN + NT - 1) / NT], const double2 *src, int wn, int tid) {
#pragma unroll
    for (int k = 0; k < (WN + NT - 1) / NT; ++k) yv[k] = src[min(tid + k * NT, wn - 1)];
}
template <int WN, int NT>
__device__ __forceinline__ void at_window_store(double2 *win, const double2 (&yv)[(WN + NT - 1) / NT], int tid) {
#pragma unroll
    for (int k = 0; k < (WN + NT - 1) / NT; ++k) win[min(tid + k * NT, WN - 1)] = yv[k];
}

// A wave's next slice of the current tile: an LDS counter per tile parity
// (lane 0's atomic, broadcast)
__device__ __forceinline__ int at_claim(int *c) {
    int v = 0;
    if (lane_id() == 0) v = atomicAdd(c, 1);
    return __builtin_amdgcn_readfirstlane(v);
}

// One workgroup per row block (owned rows [b0, b0 + RB) of [0, rows), label
// r0 + local row); XCD-chunked block order.  attr / lpart as attract_rows.
// DYN (Options::attract_dyn, round 6): a tile's slices are claimed by the
// waves from a counter instead of dealt round-robin.  The slices come sorted
// by descending width, so round-robin gives wave 0 the widest of every 16 and
// the other waves wait for it at the tile's barrier (PMC: waves wait 58 % of
// their lifetime, 22 % on their own loads).  Every row has one slice per tile
// and the tiles keep their order, so each accumulator receives the same terms
// in the same order: the sums are bit-identical either way.  (Not for the
// loss: a wave's partial would sum whichever slices it claimed, so loss
// launches keep the round-robin deal.)
template <class CF, bool LOSS, int MET, bool DYN = false>
__global__ __launch_bounds__(CF::NT) void attract_tiles(
    const ATile *__restrict__ tiles, const int32_t *__restrict__ rbt, const ASlice *__restrict__ slices,
    const uint32_t *__restrict__ srow, int64_t rows, int64_t r0, int64_t n, const uint16_t *__restrict__ pk,
    const double *__restrict__ pv, const double *__restrict__ Y, const double *__restrict__ scal, double ex,
    int64_t xcd_chunk, double2 *__restrict__ attr, double *__restrict__ lpart, int64_t rbs) {
    constexpr int RB = CF::RB, W = CF::W, NT = CF::NT, WAVES = CF::WAVES;
    __shared__ double2 win[W];
    __shared__ double2 acc[RB];
    __shared__ double sl[WAVES];
    __shared__ int claim[2];
    const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const int64_t rb = xcd_chunk > 0 ? xcd_block_chunked(blockIdx.x, gridDim.x, xcd_chunk) : (int64_t)blockIdx.x;
    const int64_t b0 = rb * rbs;   // rbs <= RB rows per block (attract_layout_build)
    const int nr = (int)min(rbs, rows - b0);
    const double2 *Y2 = reinterpret_cast<const double2 *>(Y);
    const double2 *Yrow = Y2 + r0 + b0;
    for (int i = tid; i < nr; i += NT) acc[i] = make_double2(0.0, 0.0);
    if (DYN && tid < 2) claim[tid] = 0;
    const double Z = LOSS ? scal[0] : 1.0;
    double lsum = 0.0;
    constexpr int WL = (W + NT - 1) / NT;
    const int t0 = rbt[rb], t1 = rbt[rb + 1];
    for (int t = t0; t < t1; ++t) {
        const ATile tl = tiles[t];
#if AT_DIAG != 3
        {   // the tile's window: all of a thread's loads in flight before its LDS stores
            // (round 6: unconditional stores; with `if (i < wn)` the compiler sank each
            // load into its store's branch and the copy took WL dependent round trips)
            const int64_t base = (int64_t)tl.cb * W;
            double2 yv[WL];
            at_window_regs<W, NT>(yv, Y2 + base, (int)min((int64_t)W, n - base), tid);
            at_window_store<W, NT>(win, yv, tid);
        }
#endif
        __syncthreads();
        const int s0 = tl.s0, send = tl.s0 + tl.ns;
        // the wave's slices s0 + w, s0 + w + WAVES, ... (DYN: claimed); the next
        // slice's record and lane word are fetched during the current one
        if (DYN && tid == 0) claim[(t + 1) & 1] = 0;   // the next tile's counter: its last claim was before this barrier
        int s = DYN ? s0 + at_claim(&claim[t & 1]) : s0 + w;
        ASlice sd{};
        uint32_t rl = 0;
        if (s < send) {
            sd = slices[s];
            rl = srow[(int64_t)s * 64 + lane];
        }
        while (s < send) {
            const int len = (int)(rl & ((1u << AT_LENBITS) - 1)), lrow = (int)(rl >> AT_LENBITS);
            double2 yi = make_double2(0.0, 0.0);
#if AT_DIAG != 3
            if (len > 0) yi = Yrow[lrow];
#endif
            const int sn = DYN ? s0 + at_claim(&claim[t & 1]) : s + WAVES;
            ASlice sdn{};
            uint32_t rln = 0;
            double fx = 0.0, fy = 0.0;
            int64_t off = sd.base;   // wave-uniform: the current step's first entry
            for (int k0 = 0; k0 < sd.width; k0 += AT_U) {
                uint32_t cu[AT_U];   // one register each: a packed 16-bit array would wait on every load
                double vu[AT_U];
#pragma unroll
                for (int u = 0; u < AT_U; ++u) {
                    const int k = k0 + u;
                    cu[u] = 0;
                    vu[u] = 0.0;
#if AT_DIAG == 2   // diagnostic build: no entry loads
                    if (k < len) { cu[u] = (uint32_t)((lane * 97 + k * 31) % W); vu[u] = 1e-9; }
#elif AT_NT   // entries read once per launch (1.6 GB at C3, past the Infinity Cache): nontemporal
                    if (k < len) {
                        cu[u] = __builtin_nontemporal_load(pk + off + lane);
                        vu[u] = __builtin_nontemporal_load(pv + off + lane);
                    }
#else
                    if (k < len) { cu[u] = pk[off + lane]; vu[u] = pv[off + lane]; }
#endif
                    off += __popcll(__ballot(len > k));   // the step's active lanes (a prefix)
                }
                if (k0 == 0 && sn < send) {
                    sdn = slices[sn];
                    rln = srow[(int64_t)sn * 64 + lane];
                }
#pragma unroll
                for (int u = 0; u < AT_U; ++u) {
#if AT_DIAG == 1 || AT_DIAG == 3   // diagnostic builds: loads only, no window reads or pair terms
                                    // (3: no window copy or Y_i either -- the entry stream's own rate)
                    if (k0 + u < len) { fx += vu[u]; fy += (double)cu[u]; }
                    continue;
#endif
                    if (k0 + u < len) {
                        // P q d with P's exaggeration applied to the row's total
                        // (attr below), the q d terms accumulated by FMA
                        const double2 yj = win[cu[u]];
                        const double dx = __dsub_rn(yi.x, yj.x), dy = __dsub_rn(yi.y, yj.y);
                        double x1m;   // 1 + metric = 1 / q
                        const double q = qforce_t<MET>(yi.x, yi.y, yj.x, yj.y, dx, dy, x1m);
                        const double sc = __dmul_rn(vu[u], q);
                        fx = __fma_rn(sc, dx, fx);
                        fy = __fma_rn(sc, dy, fy);
                        // P ln(P / (q / Z)) = P ln(P Z (1 + metric)): no divisions
                        // (0 ln 0 = NaN for an underflowed P, as the reference)
                        if (LOSS) {
                            const double pij = __dmul_rn(vu[u], ex);
                            lsum += pij * log_kl(pij * Z * x1m);
                        }
                    }
                }
            }
            if (sd.wide) {   // one row over the 64 lanes: a fixed-order tree
                fx = wave_sum(fx);
                fy = wave_sum(fy);
                if (lane == 0) {
                    const double2 o = acc[lrow];
                    acc[lrow] = make_double2(__dadd_rn(o.x, fx), __dadd_rn(o.y, fy));
                }
            } else if (len > 0) {
                const double2 o = acc[lrow];
                acc[lrow] = make_double2(__dadd_rn(o.x, fx), __dadd_rn(o.y, fy));
            }
            s = sn;
            sd = sdn;
            rl = rln;
        }
        __syncthreads();
    }
    for (int i = tid; i < nr; i += NT) attr[b0 + i] = make_double2(acc[i].x * ex, acc[i].y * ex);
    if (LOSS) {
        lsum = wave_sum(lsum);
        if (lane == 0) sl[w] = lsum;
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int k = 0; k < WAVES; ++k) s += sl[k];
            lpart[blockIdx.x] = s;
        }
    }
}

// ---- attract_tiles, pipelined (Options::attract_pipe, round 6)
// attract_tiles' ISA waits once per slice for ALL of that slice's loads (its
// entries and the next slice's prefetched record alike: the entry loads sit in
// exec-masked branches, so the compiler's wait counts fall back to vmcnt(0)),
// and nothing is in flight while the slice is summed; each tile's window
// copy also ran as WL dependent load -> wait -> store round trips (the loads
// were sunk into the stores' branches).  Here a wave has the entries of its
// next D slices in flight while it sums the current one, the slice records
// 2D ahead, and the next tile's window is loaded into registers during the
// current tile (WPF).  Every slice issues the same instructions: the entry
// loads are buffer loads whose lanes past their row's entries address out of
// range (0, no memory request), so the compiler's wait counts stay exact.
// A slice wider than U steps loads and sums its remaining steps in place.
// Each lane sums its row's entries in the same order as attract_tiles, so the
// results are bit-identical.
// The wave's cursor over the row block's tiles (tile t, slice s < send;
// t == t1: none)
struct ATCur {
    int t, s, send;
};
// ring R (records and lane words, 2D + 1 slices ahead) and ring E (entries
// of the first U steps and y_i, D slices ahead)
struct ATRSlot {
    uint32_t lo;   // the slice record as loaded (every lane the same address):
    int2 wd;       // first entry (< 2^31: attract_layout_build), width, wide
    uint32_t rl;   // lane word: local row << AT_LENBITS | entries
    ATCur c;
};
template <int U>
struct ATESlot {
    uint16_t cu[U];   // widened where summed: a widening here waits for the load
    double vu[U];
    double2 yi;
    int base, width, wide, rU;   // wave-uniform; rU: entries of the first U steps
};
constexpr int AT_RU = 4;   // steps past U: loaded and summed 4 at a time

// the wave's first slice in tiles t.. (scalar loads: every value wave-uniform)
__device__ __forceinline__ ATCur atp_first(const ATile *__restrict__ tiles, int t, int t1, int w) {
    ATCur c{__builtin_amdgcn_readfirstlane(t), 0, 0};
    for (; c.t < t1; c.t = __builtin_amdgcn_readfirstlane(c.t + 1)) {
        const int s0 = __builtin_amdgcn_readfirstlane(tiles[c.t].s0);
        const int ns = __builtin_amdgcn_readfirstlane(tiles[c.t].ns);
        c.s = s0 + w;
        c.send = s0 + ns;
        if (c.s < c.send) break;
    }
    return c;
}
template <int WAVES>
__device__ __forceinline__ ATCur atp_next(const ATile *__restrict__ tiles, const ATCur &c, int t1, int w) {
    if (c.t >= t1) return c;
    ATCur d = c;
    d.s += WAVES;
    return d.s < d.send ? d : atp_first(tiles, c.t + 1, t1, w);
}
// ring R's loads: unconditional, so that every step issues the same
// instructions (past the wave's last slice a dummy slice's, whose entries are
// loaded but never summed); nothing consumes them until the entries' issue
// (a select on the lane word here would wait for it at once).  The record
// goes through buffer loads: vector memory, counted in order with the rest
// (scalar loads share their counter with the LDS reads of the sums).
__device__ __forceinline__ void atp_issue_rec(ATRSlot &x, const ASlice *__restrict__ slices,
                                              const uint32_t *__restrict__ srow, int t1, int sdummy, int lane) {
    const int s = x.c.t < t1 ? x.c.s : sdummy;
    const __amdgpu_buffer_rsrc_t rr = at_rsrc(slices + s);
    x.lo = __builtin_amdgcn_raw_buffer_load_b32(rr, 0u, 0, 0);   // base (low word)
    typedef uint32_t u2v __attribute__((ext_vector_type(2)));
    const u2v wd = __builtin_amdgcn_raw_buffer_load_b64(rr, 8u, 0, 0);
    x.wd = make_int2((int)wd.x, (int)wd.y);
    x.rl = srow[(int64_t)s * 64 + lane];
}
template <int U>
__device__ __forceinline__ void atp_issue_entries(const ATRSlot &x, ATESlot<U> &e, const uint16_t *__restrict__ pk,
                                                  const double *__restrict__ pv, const double2 *__restrict__ Yrow,
                                                  int lane) {
    e.base = __builtin_amdgcn_readfirstlane((int)x.lo);
    e.width = __builtin_amdgcn_readfirstlane(x.wd.x);
    e.wide = __builtin_amdgcn_readfirstlane(x.wd.y);
    const int len = (int)(x.rl & ((1u << AT_LENBITS) - 1)), lrow = (int)(x.rl >> AT_LENBITS);
    const __amdgpu_buffer_rsrc_t rk = at_rsrc(pk + e.base), rv = at_rsrc(pv + e.base);
    int r = 0;   // wave-uniform: the step's first entry, relative to base
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool act = len > u;
        const uint32_t o = (uint32_t)(r + lane);
        e.cu[u] = __builtin_amdgcn_raw_buffer_load_b16(rk, act ? 2u * o : AT_OOB, 0, 0);
        typedef uint32_t u2v __attribute__((ext_vector_type(2)));
        const u2v v = __builtin_amdgcn_raw_buffer_load_b64(rv, act ? 8u * o : AT_OOB, 0, 0);
        e.vu[u] = __longlong_as_double((long long)(((uint64_t)v.y << 32) | v.x));
        r += __popcll(__ballot(act));
    }
    e.rU = r;
    e.yi = Yrow[lrow];   // lrow = 0 for a lane without a row: a valid point
}
template <bool LOSS, int MET>
__device__ __forceinline__ void atp_term(const double2 *win, double2 yi, uint32_t c, double v, double ex, double Z,
                                         double &fx, double &fy, double &lsum) {
    const double2 yj = win[c];
    const double dx = __dsub_rn(yi.x, yj.x), dy = __dsub_rn(yi.y, yj.y);
    double x1m;
    const double q = qforce_t<MET>(yi.x, yi.y, yj.x, yj.y, dx, dy, x1m);
    const double sc = __dmul_rn(v, q);
    fx = __fma_rn(sc, dx, fx);
    fy = __fma_rn(sc, dy, fy);
    if (LOSS) {
        const double pij = __dmul_rn(v, ex);
        lsum += pij * log_kl(pij * Z * x1m);
    }
}
// a slice's sums into its rows' accumulators (steps past U loaded in place)
template <int U, bool LOSS, int MET>
__device__ __forceinline__ void atp_sum(const ATRSlot &x, const ATESlot<U> &e, const double2 *win, double2 *acc,
                                        const uint16_t *__restrict__ pk, const double *__restrict__ pv, double ex,
                                        double Z, int lane, double &lsum) {
    const int len = (int)(x.rl & ((1u << AT_LENBITS) - 1)), lrow = (int)(x.rl >> AT_LENBITS);
    double fx = 0.0, fy = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (u < len) atp_term<LOSS, MET>(win, e.yi, e.cu[u], e.vu[u], ex, Z, fx, fy, lsum);
    if (e.width > U) {
        int64_t off = (int64_t)e.base + e.rU;
        for (int k0 = U; k0 < e.width; k0 += AT_RU) {
            uint32_t cu[AT_RU];
            double vu[AT_RU];
#pragma unroll
            for (int u = 0; u < AT_RU; ++u) {
                const int k = k0 + u;
                cu[u] = 0;
                vu[u] = 0.0;
                if (k < len) { cu[u] = pk[off + lane]; vu[u] = pv[off + lane]; }
                off += __popcll(__ballot(len > k));
            }
#pragma unroll
            for (int u = 0; u < AT_RU; ++u)
                if (k0 + u < len) atp_term<LOSS, MET>(win, e.yi, cu[u], vu[u], ex, Z, fx, fy, lsum);
        }
        // vmcnt(0): the remainder's loads are consumed in exec-masked branches,
        // so past this block the compiler would count them as outstanding and
        // make every later step wait for nearly everything in flight
        __builtin_amdgcn_s_waitcnt(0x0F70);
    }
    if (e.wide) {   // one row over the 64 lanes: a fixed-order tree
        fx = wave_sum(fx);
        fy = wave_sum(fy);
        if (lane == 0) {
            const double2 o = acc[lrow];
            acc[lrow] = make_double2(__dadd_rn(o.x, fx), __dadd_rn(o.y, fy));
        }
    } else if (len > 0) {
        const double2 o = acc[lrow];
        acc[lrow] = make_double2(__dadd_rn(o.x, fx), __dadd_rn(o.y, fy));
    }
}
// tile t's window into LDS, then the barrier (every wave has left the previous one)
template <int W, int NT>
__device__ __forceinline__ void atp_tile_begin(double2 *win, const ATile *__restrict__ tiles, const double2 *Y2,
                                               int64_t n, int t, int tid) {
    const int64_t nb = (int64_t)__builtin_amdgcn_readfirstlane(tiles[t].cb) * W;
    double2 yv[(W + NT - 1) / NT];
    at_window_regs<W, NT>(yv, Y2 + nb, (int)min((int64_t)W, n - nb), tid);
    at_window_store<W, NT>(win, yv, tid);
    __syncthreads();
}

template <class CF, int D, int U, bool LOSS, int MET>
__global__ __launch_bounds__(CF::NT) void attract_tiles_pipe(
    const ATile *__restrict__ tiles, const int32_t *__restrict__ rbt, const ASlice *__restrict__ slices,
    const uint32_t *__restrict__ srow, int64_t rows, int64_t r0, int64_t n, const uint16_t *__restrict__ pk,
    const double *__restrict__ pv, const double *__restrict__ Y, const double *__restrict__ scal, double ex,
    int64_t xcd_chunk, double2 *__restrict__ attr, double *__restrict__ lpart, int64_t rbs) {
    constexpr int RB = CF::RB, W = CF::W, NT = CF::NT, WAVES = CF::WAVES;
    constexpr int NE = D + 1, NR = 2 * (D + 1);   // the step loop is unrolled over NR
    static_assert(D >= 1 && D <= 3 && U >= 1, "pipeline shape");
    __shared__ double2 win[W];
    __shared__ double2 acc[RB];
    __shared__ double sl[WAVES];
    const int tid = threadIdx.x, lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform for the compiler
    const int64_t rb = xcd_chunk > 0 ? xcd_block_chunked(blockIdx.x, gridDim.x, xcd_chunk) : (int64_t)blockIdx.x;
    const int64_t b0 = rb * rbs;
    const int nr = (int)min(rbs, rows - b0);
    const double2 *Y2 = reinterpret_cast<const double2 *>(Y);
    const double2 *Yrow = Y2 + r0 + b0;
    for (int i = tid; i < nr; i += NT) acc[i] = make_double2(0.0, 0.0);
    const double Z = LOSS ? scal[0] : 1.0;
    double lsum = 0.0;
    const int t0 = __builtin_amdgcn_readfirstlane(rbt[rb]), t1 = __builtin_amdgcn_readfirstlane(rbt[rb + 1]);
    if (t0 < t1) {
        const int sdummy = __builtin_amdgcn_readfirstlane(tiles[t0].s0);   // a valid slice for "no slice"
        ATRSlot R[NR];
        ATESlot<U> E[NE];
        // prologue: slices 0 .. 2D: records; 0 .. D-1: entries, issued in the
        // steps' own order (entries of j, then the record of j + D + 1), so
        // that the compiler's outstanding-load counts agree at the loop head
        R[0].c = atp_first(tiles, t0, t1, w);
#pragma unroll
        for (int j = 1; j <= 2 * D; ++j) R[j].c = atp_next<WAVES>(tiles, R[j - 1].c, t1, w);
#pragma unroll
        for (int j = 0; j <= D; ++j) atp_issue_rec(R[j], slices, srow, t1, sdummy, lane);
#pragma unroll
        for (int j = 0; j < D; ++j) {
            atp_issue_entries<U>(R[j], E[j], pk, pv, Yrow, lane);
            atp_issue_rec(R[j + D + 1], slices, srow, t1, sdummy, lane);
        }
        int tcur = t0;
        atp_tile_begin<W, NT>(win, tiles, Y2, n, t0, tid);
        // Rounds of NR steps; every step issues its loads whether or not its
        // slice exists (past the wave's last slice: dummies), only the sum is
        // conditional -- a step skipped as a whole would make the compiler
        // count fewer loads after each outstanding one and wait for nearly all
        do {
#pragma unroll
            for (int r = 0; r < NR; ++r) {   // the step of slice i, r = i mod NR
                const bool live = R[r].c.t < t1;
                while (live && tcur != R[r].c.t) {   // the wave's next slice is in a later tile
                    __syncthreads();
                    tcur = __builtin_amdgcn_readfirstlane(tcur + 1);
                    atp_tile_begin<W, NT>(win, tiles, Y2, n, tcur, tid);
                }
                atp_issue_entries<U>(R[(r + D) % NR], E[(r + D) % NE], pk, pv, Yrow, lane);   // slice i + D
                if (live) atp_sum<U, LOSS, MET>(R[r], E[r % NE], win, acc, pk, pv, ex, Z, lane, lsum);
                // slice i - 1's record slot is free: slice i + 2D + 1
                R[(r + NR - 1) % NR].c = atp_next<WAVES>(tiles, R[(r + 2 * D) % NR].c, t1, w);
                atp_issue_rec(R[(r + NR - 1) % NR], slices, srow, t1, sdummy, lane);
            }
        } while (R[0].c.t < t1);
        while (tcur + 1 < t1) {   // the barriers of the tiles this wave has no slice in
            __syncthreads();
            tcur = __builtin_amdgcn_readfirstlane(tcur + 1);
            atp_tile_begin<W, NT>(win, tiles, Y2, n, tcur, tid);
        }
        __syncthreads();
    }
    for (int i = tid; i < nr; i += NT) attr[b0 + i] = make_double2(acc[i].x * ex, acc[i].y * ex);
    if (LOSS) {
        lsum = wave_sum(lsum);
        if (lane == 0) sl[tid >> 6] = lsum;
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int k = 0; k < WAVES; ++k) s += sl[k];
            lpart[blockIdx.x] = s;
        }
    }
}

// ---- attract_tiles over the stream layout (Options::attract_stream, round 10)
// attract_tiles moves 290 B per vector-memory instruction (2-byte and 8-byte
// loads, exec-masked by the lane's row length, each step's base a ballot
// chain) and has nothing in flight while it sums a slice.  The stream layout
// stores the same tiles, slices, lanes and per-row entry order a second time,
// arranged for the fetch: a tile's slices are dealt to the 16 waves when the
// layout is built (by total width), and all the steps a wave runs in a row
// block -- slice after slice, tile after tile -- form one contiguous stream.
// Every step holds all 64 lanes: a lane past its row's end gets the value +0.0
// and the column of the lane's first entry in the slice (no row: column 0), so
// its term adds +-0 to a sum that is never -0, from a point the row has read
// already.  The steps go in groups of four (ATS_GBYTES per group: lane l's
// values of steps 0-1 at 16 l, of steps 2-3 at 1024 + 16 l, its four 16-bit
// columns at 2048 + 8 l); groups run across slices and tiles, so only the end
// of a wave's stream is padded to a group.  A wave reads its stream through a
// ring of ATS_D groups of registers: three unconditional buffer loads per
// group, the descriptor covering the wave's own stream and the offset advanced
// by a constant, on every path, so the compiler counts the loads in flight and
// the ring keeps issuing through slice switches and tile barriers.  A slice
// switch takes the lane word (from the dealt list, two slices ahead) and y_i
// (one slice ahead; see ats_wait_but), and adds the finished slice's sums to
// the rows' accumulators as attract_tiles does.  Each (row, tile) sum and each accumulator receives
// the same operations in the same order as in attract_tiles: bit-identical.
constexpr int ATS_GBYTES = 64 * (4 * 8 + 4 * 2);   // a group: four steps of 64 lanes
constexpr int ATS_D = 4;                           // groups in flight per wave (10 KB; 40 VGPRs)
typedef uint32_t ats_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t ats_u2 __attribute__((ext_vector_type(2)));
struct ATSGroup {
    ats_u4 a, b;   // values: steps 0-1, 2-3
    ats_u2 c;      // columns: four steps
};
#ifndef ATS_DEFECT
#define ATS_DEFECT 0   // 1, 3, 4: seeded defects for tests/test_gpu_attract_stream.py (never in a product build)
#endif
// a group's three loads; `goff` (the group's byte offset) goes into the range-checked
// vector offset, so that a group past the wave's stream reads zeros and moves nothing
__device__ __forceinline__ void ats_issue(ATSGroup &r, __amdgpu_buffer_rsrc_t rs, int lane, uint32_t goff) {
    // read once per launch: nontemporal (aux bit 1)
    r.a = __builtin_amdgcn_raw_buffer_load_b128(rs, goff + (uint32_t)lane * 16u, 0, 2);
    r.b = __builtin_amdgcn_raw_buffer_load_b128(rs, goff + (uint32_t)lane * 16u + 1024u, 0, 2);
    r.c = __builtin_amdgcn_raw_buffer_load_b64(rs, goff + (uint32_t)lane * 8u + 2048u, 0, 2);
}
template <int U>
__device__ __forceinline__ double ats_val(const ATSGroup &r) {
    return U == 0 ? __hiloint2double((int)r.a.y, (int)r.a.x) : U == 1 ? __hiloint2double((int)r.a.w, (int)r.a.z)
         : U == 2 ? __hiloint2double((int)r.b.y, (int)r.b.x) : __hiloint2double((int)r.b.w, (int)r.b.z);
}
template <int U>
__device__ __forceinline__ uint32_t ats_col(const ATSGroup &r) {
    return U == 0 ? (r.c.x & 0xffffu) : U == 1 ? (r.c.x >> 16) : U == 2 ? (r.c.y & 0xffffu) : (r.c.y >> 16);
}

// The slice pipeline's own loads (a lane word two slices ahead, y_i one slice
// ahead) are consumed at the next slice switch, and the compiler, which must
// assume the shortest path between two switches (no group issued), would wait
// there for every load in flight: the whole ring, once per slice (measured:
// 0.61 ms per launch against 0.67 for attract_tiles).  So these loads go
// through registers the compiler does not manage (accumulation registers a0 ..
// a5, written by the loads, read after the wait) and the wave counts the ring
// loads it has issued since: loads return in order, so leaving that many in
// flight is enough.  The compiler's own counts are unaware of these loads and
// therefore wait for at most two loads more than they need.
template <int P>
__device__ __forceinline__ void ats_lword_load(const uint32_t *p) {
    if (P == 0) asm volatile("global_load_dword a0, %0, off" : : "v"(p) : "a0", "memory");
    else asm volatile("global_load_dword a1, %0, off" : : "v"(p) : "a1", "memory");
}
template <int P>
__device__ __forceinline__ uint32_t ats_lword_read() {
    uint32_t v;
    if (P == 0) asm volatile("v_accvgpr_read_b32 %0, a0" : "=v"(v) : : "memory");
    else asm volatile("v_accvgpr_read_b32 %0, a1" : "=v"(v) : : "memory");
    return v;
}
__device__ __forceinline__ void ats_yi_load(const double2 *p) {
    asm volatile("global_load_dwordx4 a[2:5], %0, off" : : "v"(p) : "a2", "a3", "a4", "a5", "memory");
}
__device__ __forceinline__ double2 ats_yi_read() {
    uint32_t x0, x1, y0, y1;
    asm volatile("v_accvgpr_read_b32 %0, a2\n\tv_accvgpr_read_b32 %1, a3\n\t"
                 "v_accvgpr_read_b32 %2, a4\n\tv_accvgpr_read_b32 %3, a5"
                 : "=v"(x0), "=v"(x1), "=v"(y0), "=v"(y1) : : "memory");
    return make_double2(__hiloint2double((int)x1, (int)x0), __hiloint2double((int)y1, (int)y0));
}
// everything but the last `c` loads (c: ring loads issued since the loads waited for)
__device__ __forceinline__ void ats_wait_but(int c) {
    if (c >= 9) asm volatile("s_waitcnt vmcnt(9)" : : : "memory");
    else if (c >= 6) asm volatile("s_waitcnt vmcnt(6)" : : : "memory");
    else if (c >= 3) asm volatile("s_waitcnt vmcnt(3)" : : : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
}

template <class CF, int MET>
__global__ __launch_bounds__(CF::NT) void attract_tiles_stream(
    const ATile *__restrict__ tiles, const int32_t *__restrict__ rbt, const AWave *__restrict__ waves,
    const int2 *__restrict__ recs, const uint32_t *__restrict__ lword, const uint8_t *__restrict__ stream,
    int64_t rows, int64_t r0, int64_t n, const double *__restrict__ Y, double ex, int64_t xcd_chunk,
    double2 *__restrict__ attr, int64_t rbs) {
    constexpr int RB = CF::RB, W = CF::W, NT = CF::NT, WAVES = CF::WAVES, D = ATS_D;
    __shared__ double2 win[W];
    __shared__ double2 acc[RB];
    const int tid = threadIdx.x, lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t rb = xcd_chunk > 0 ? xcd_block_chunked(blockIdx.x, gridDim.x, xcd_chunk) : (int64_t)blockIdx.x;
    const int64_t b0 = rb * rbs;
    const int nr = (int)min(rbs, rows - b0);
    const double2 *Y2 = reinterpret_cast<const double2 *>(Y);
    const double2 *Yrow = Y2 + r0 + b0;
    for (int i = tid; i < nr; i += NT) acc[i] = make_double2(0.0, 0.0);
    const int t0 = __builtin_amdgcn_readfirstlane(rbt[rb]), t1 = __builtin_amdgcn_readfirstlane(rbt[rb + 1]);
    if (t0 < t1) {
        const AWave *wv = waves + rb * WAVES + w;
        const int q0 = __builtin_amdgcn_readfirstlane(wv->q0), cnt = __builtin_amdgcn_readfirstlane(wv->cnt);
#if ATS_DEFECT == 3
        const int steps = max(0, ((__builtin_amdgcn_readfirstlane(wv->steps) + 3) >> 2) - 1) << 2;
#else
        const int steps = __builtin_amdgcn_readfirstlane(wv->steps);
#endif
        const int64_t g0 = __builtin_amdgcn_readfirstlane(wv->g0);
        const int ng = (steps + 3) >> 2;
        // the descriptor covers the wave's own stream (all of P's entries can exceed 4 GB).
        // Every group slot issues its loads, past the stream's end too (out of range: zeros,
        // never summed): a conditional issue would leave the compiler no load count to wait by
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t *>(stream + g0 * ATS_GBYTES), (short)0, ng * ATS_GBYTES, 0x00020000);
        // the slice pipeline: slice i + 2's lane word and slice i + 1's y_i in flight
        // (list slots past the wave's slices hold other waves' words or the slack:
        // the row is clamped, the point never used)
        const uint32_t *lw = lword + (int64_t)q0 * 64 + lane;
        // (the lane words of even slices in a0, of odd ones in a1, y_i in a2 .. a5)
        ats_lword_load<0>(lw);
        ats_lword_load<1>(lw + 64);
        ats_wait_but(0);
        ats_yi_load(Yrow + min((int)(ats_lword_read<0>() >> AT_LENBITS), nr - 1));
        ATSGroup R[D];
        uint32_t soff = 0;
        int since = 0;   // ring loads issued since the slice pipeline's last loads
#pragma unroll
        for (int j = 0; j < D; ++j) {
            ats_issue(R[j], rs, lane, soff);
            soff += ATS_GBYTES;
            since += 3;
        }
        int2 rec1 = make_int2(0, t1);   // the next slice: width | wide << 31, tile
        if (cnt > 0) {
            rec1.x = __builtin_amdgcn_readfirstlane(recs[q0].x);
            rec1.y = __builtin_amdgcn_readfirstlane(recs[q0].y);
        }
        int i = 0, tcur = t0, rem = 0, wide = 0, len = 0, lrow = 0;
        double2 yi = make_double2(0.0, 0.0);
        double fx = 0.0, fy = 0.0, lnone = 0.0;
        atp_tile_begin<W, NT>(win, tiles, Y2, n, t0, tid);
        // the finished slice's sums into its rows' accumulators (as attract_tiles)
        auto flush = [&]() {
            if (wide) {   // one row over the 64 lanes: a fixed-order tree (lanes without entries add 0)
                fx = wave_sum(len > 0 ? fx : 0.0);
                fy = wave_sum(len > 0 ? fy : 0.0);
                if (lane == 0) {
                    const double2 o = acc[lrow];
                    acc[lrow] = make_double2(__dadd_rn(o.x, fx), __dadd_rn(o.y, fy));
                }
            } else if (len > 0) {
                const double2 o = acc[lrow];
                acc[lrow] = make_double2(__dadd_rn(o.x, fx), __dadd_rn(o.y, fy));
#if ATS_DEFECT == 4   // as if wave 1's slices had been dealt to a second wave as well
                if (w == 1) acc[lrow] = make_double2(__dadd_rn(acc[lrow].x, fx), __dadd_rn(acc[lrow].y, fy));
#endif
            }
        };
        // the barriers and window copies up to tile `to` (t1: past the last tile)
        auto advance = [&](int to) {
            while (tcur < to) {
                __syncthreads();
                tcur = __builtin_amdgcn_readfirstlane(tcur + 1);
                if (tcur == t1) break;
                atp_tile_begin<W, NT>(win, tiles, Y2, n, tcur, tid);
            }
        };
        auto next_slice = [&](auto par) {   // the parity of slice i
            constexpr int P = decltype(par)::value;
            flush();
            advance(rec1.y);
            ats_wait_but(since);
            const uint32_t rl1 = ats_lword_read<P>(), rl2 = ats_lword_read<1 - P>();
            rem = rec1.x & 0x7fffffff;
            wide = (int)((uint32_t)rec1.x >> 31);
            len = (int)(rl1 & ((1u << AT_LENBITS) - 1));
            lrow = (int)(rl1 >> AT_LENBITS);
            yi = ats_yi_read();
            fx = 0.0;
            fy = 0.0;
            i = __builtin_amdgcn_readfirstlane(i + 1);
            rec1 = make_int2(0, t1);
            if (i < cnt) {
                rec1.x = __builtin_amdgcn_readfirstlane(recs[q0 + i].x);
                rec1.y = __builtin_amdgcn_readfirstlane(recs[q0 + i].y);
            }
            ats_yi_load(Yrow + min((int)(rl2 >> AT_LENBITS), nr - 1));
            ats_lword_load<P>(lw + (int64_t)(i + 1) * 64);
            since = 0;
        };
#define TSNE_ATS_STEP(J, U)                                                                               \
    if (((g + J) << 2) + U < steps) {                                                                     \
        if (rem == 0) {                                                                                   \
            if (i & 1) next_slice(std::integral_constant<int, 1>{});                                      \
            else next_slice(std::integral_constant<int, 0>{});                                            \
        }                                                                                                 \
        atp_term<false, MET>(win, yi, ats_col<U>(R[J]), ats_val<U>(R[J]), ex, 1.0, fx, fy, lnone);       \
        --rem;                                                                                            \
    }
        for (int g = 0; g < ng; g += D) {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                if (g + j < ng) {
                    TSNE_ATS_STEP(j, 0)
                    TSNE_ATS_STEP(j, 1)
                    TSNE_ATS_STEP(j, 2)
                    TSNE_ATS_STEP(j, 3)
                }
                ats_issue(R[j], rs, lane, soff);   // group g + j + D
                soff += ATS_GBYTES;
                since += 3;
            }
        }
#undef TSNE_ATS_STEP
        ats_wait_but(0);   // the pipeline's last loads, of slices past the wave's
        flush();
        advance(t1);
    }
    for (int i = tid; i < nr; i += NT) attr[b0 + i] = make_double2(acc[i].x * ex, acc[i].y * ex);
}

// ---- tile layout build (at every relabel; see attract_layout_build)
// 1. key (row block * ncb + window) << rowbits | local row of every owned
//    entry (wave per row), for a stable radix sort
__global__ void at_keys(const int64_t *__restrict__ rpw, const int32_t *__restrict__ colw, int64_t rows, int64_t ncb,
                        int rowbits, int64_t rbs, int64_t W, uint64_t *__restrict__ key, int32_t *__restrict__ idx) {
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int64_t rb = r / rbs;   // row block of rbs (<= 2^rowbits) rows
    const uint64_t hi = (uint64_t)(rb * ncb);
    const uint64_t lr = (uint64_t)(r - rb * rbs);
    for (int64_t e = rpw[r] + lane_id(); e < rpw[r + 1]; e += 64) {
        key[e] = ((hi + (uint64_t)(colw[e] / W)) << rowbits) | lr;
        idx[e] = (int32_t)e;
    }
}

// 2. sorted position p <- entry perm[p]: column offset in the window, value,
//    and the start flag of each (tile, row) segment
__global__ void at_gather(const uint64_t *__restrict__ ks, const int32_t *__restrict__ perm, int64_t m, int64_t ncb,
                          int rowbits, int64_t W, const int32_t *__restrict__ colw, const double *__restrict__ valw,
                          uint16_t *__restrict__ cs, double *__restrict__ vs, int32_t *__restrict__ flag) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const int64_t e = perm[p];
    const uint64_t k = ks[p];
    const int64_t cb = (int64_t)((k >> rowbits) % (uint64_t)ncb);
    cs[p] = (uint16_t)(colw[e] - cb * W);
    vs[p] = valw[e];
    flag[p] = (p == 0 || ks[p - 1] != k) ? 1 : 0;
}

// 3. segments: start, key; then (next kernel) length and the sort key
//    (tile << 20 | ~length) that orders a tile's rows by descending count
__global__ void at_segs(const uint64_t *__restrict__ ks, const int32_t *__restrict__ flag,
                        const int32_t *__restrict__ sid, int64_t m, int32_t *__restrict__ sstart,
                        uint64_t *__restrict__ skey) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m || !flag[p]) return;
    sstart[sid[p]] = (int32_t)p;
    skey[sid[p]] = ks[p];
}
__global__ void at_seglen(const int32_t *__restrict__ sstart, const uint64_t *__restrict__ skey, int32_t ns, int64_t m,
                          int rowbits, int32_t *__restrict__ slen, uint64_t *__restrict__ okey,
                          int32_t *__restrict__ oval) {
    const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ns) return;
    const int32_t len = (int32_t)((g + 1 < ns ? (int64_t)sstart[g + 1] : m) - sstart[g]);
    slen[g] = len;
    okey[g] = ((skey[g] >> rowbits) << AT_LENBITS) | (uint64_t)((1u << AT_LENBITS) - 1 - (uint32_t)len);
    oval[g] = g;
}

// 4. over the sorted segments j: lengths in sorted order and tile-start flags
__global__ void at_sorted(const uint64_t *__restrict__ okey, const int32_t *__restrict__ og,
                          const int32_t *__restrict__ slen, int32_t ns, int64_t *__restrict__ lenj,
                          int32_t *__restrict__ tflag) {
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ns) return;
    lenj[j] = slen[og[j]];
    tflag[j] = (j == 0 || (okey[j - 1] >> AT_LENBITS) != (okey[j] >> AT_LENBITS)) ? 1 : 0;
}
// 5. tiles: first sorted segment, segment count -> slices (count / 64, scanned)
__global__ void at_tilefirst(const uint64_t *__restrict__ okey, const int32_t *__restrict__ tflag,
                             const int32_t *__restrict__ tix, int32_t ns, int64_t ncb, int32_t *__restrict__ tfirst,
                             ATile *__restrict__ tiles) {
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ns || !tflag[j]) return;
    const uint64_t tile = okey[j] >> AT_LENBITS;
    const int32_t t = tix[j];
    tfirst[t] = j;
    tiles[t].cb = (int32_t)(tile % (uint64_t)ncb);
    tiles[t].rb = (int32_t)(tile / (uint64_t)ncb);
}
// A row with more than AT_WIDE_MIN entries in a tile gets a slice of its own:
// the row cut into 64 consecutive pieces, one per lane, summed by a wave
// reduction -- a hub row would otherwise keep one wave busy while the
// workgroup waits for it at the tile's barrier.  (Measured at C3: wide above
// 48 entries 1.11 ms per loss launch; wide only above max(64, twice the
// slice's 64th row) 1.31 ms -- balanced lanes beat fewer slices.)
constexpr int AT_WIDE_MIN = 48;
__global__ void at_tilecount(const int32_t *__restrict__ tfirst, const int64_t *__restrict__ lenj, int32_t nt,
                             int32_t ns, int32_t *__restrict__ tns, int32_t *__restrict__ twide) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const int32_t j0 = tfirst[t], cnt = (t + 1 < nt ? tfirst[t + 1] : ns) - j0;
    int32_t nw = 0;   // segments sorted by descending length
    while (nw < cnt && lenj[j0 + nw] > AT_WIDE_MIN) ++nw;
    twide[t] = nw;
    tns[t] = nw + (cnt - nw + 63) / 64;
}
// 6. slice records (one thread per tile writes its slices)
__global__ void at_slices(const int32_t *__restrict__ tfirst, const int32_t *__restrict__ tns,
                          const int32_t *__restrict__ twide, const int32_t *__restrict__ ts0,
                          const int64_t *__restrict__ lenj, const int64_t *__restrict__ ebase, int32_t nt, int32_t ns,
                          ATile *__restrict__ tiles, ASlice *__restrict__ slices) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    tiles[t].s0 = ts0[t];
    tiles[t].ns = tns[t];
    const int32_t j0 = tfirst[t], jend = t + 1 < nt ? tfirst[t + 1] : ns, nw = twide[t];
    for (int32_t q = 0; q < tns[t]; ++q) {
        ASlice sd;
        if (q < nw) {
            sd.j0 = j0 + q;
            sd.cnt = 1;
            sd.wide = 1;
            sd.width = (int32_t)((lenj[sd.j0] + 63) / 64);
        } else {
            sd.j0 = j0 + nw + 64 * (q - nw);
            sd.cnt = min(64, jend - sd.j0);
            sd.wide = 0;
            sd.width = (int32_t)lenj[sd.j0];
        }
        sd.base = ebase[sd.j0];
        slices[ts0[t] + q] = sd;
    }
}
// 7. one wave per slice: lane words and the jagged-diagonal scatter of the
//    lanes' rows (step k: the k-th entry of each row longer than k)
__global__ void at_fill(const ASlice *__restrict__ slices, int32_t nsl, const int32_t *__restrict__ og,
                        const int32_t *__restrict__ sstart, const uint64_t *__restrict__ skey,
                        const int64_t *__restrict__ lenj, int rowbits, const uint16_t *__restrict__ cs,
                        const double *__restrict__ vs, uint32_t *__restrict__ srow, uint16_t *__restrict__ pk,
                        double *__restrict__ pv) {
    const int64_t s = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (s >= nsl) return;
    const int lane = lane_id();
    const ASlice sd = slices[s];
    int len = 0, lrow = 0;
    int64_t src = 0;
    if (sd.wide) {   // piece `lane` of the row: entries [lane * width, ...)
        const int32_t g = og[sd.j0];
        const int64_t L = lenj[sd.j0];
        len = (int)max((int64_t)0, min((int64_t)sd.width, L - (int64_t)lane * sd.width));
        lrow = (int)(skey[g] & ((1u << rowbits) - 1));
        src = sstart[g] + (int64_t)lane * sd.width;
    } else if (lane < sd.cnt) {
        const int32_t g = og[sd.j0 + lane];
        len = (int)lenj[sd.j0 + lane];
        lrow = (int)(skey[g] & ((1u << rowbits) - 1));
        src = sstart[g];
    }
    srow[s * 64 + lane] = ((uint32_t)lrow << AT_LENBITS) | (uint32_t)len;
    int64_t off = sd.base;
    for (int k = 0; k < sd.width; ++k) {
        if (k < len) {
            pk[off + lane] = cs[src + k];
            pv[off + lane] = vs[src + k];
        }
        off += __popcll(__ballot(k < len));
    }
}

// 8. the row blocks' tile ranges: rbt[rb] = first tile of a row block >= rb
__global__ void at_ranges(const ATile *__restrict__ tiles, int32_t nt, int64_t nrb, int32_t *__restrict__ rbt) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > nt) return;
    const int64_t lo = t == 0 ? 0 : (int64_t)tiles[t - 1].rb + 1;
    const int64_t hi = t < nt ? (int64_t)tiles[t].rb : nrb;
    for (int64_t r = lo; r <= hi; ++r) rbt[r] = (int32_t)t;
}

// ---- stream layout build (attract_tiles_stream), from the tiled layout
// The (tile, wave) regions are numbered in stream order: row block, wave,
// tile -- region (t, w) of a row block with tiles [t0, t1) is
// WAVES t0 + w (t1 - t0) + (t - t0).
__device__ __forceinline__ int64_t ats_region(int32_t t0, int32_t t1, int32_t t, int w, int waves) {
    return (int64_t)waves * t0 + (int64_t)w * (t1 - t0) + (t - t0);
}
// 9. one thread per tile deals its slices to the waves: each slice, in the
//    tile's order (wide slices, then descending row length), to the wave with
//    the fewest steps so far (the first of equals).  Per slice its wave, its
//    rank and first step within the region; per region its slices and steps.
template <int WAVES>
__global__ void ats_deal(const ATile *__restrict__ tiles, int32_t nt, const ASlice *__restrict__ slices,
                         const int32_t *__restrict__ rbt, int4 *__restrict__ deal, int32_t *__restrict__ rcnt,
                         int32_t *__restrict__ rsteps) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const ATile tl = tiles[t];
    const int32_t t0 = rbt[tl.rb], t1 = rbt[tl.rb + 1];
    int32_t load[WAVES], num[WAVES];
    for (int w = 0; w < WAVES; ++w) load[w] = num[w] = 0;
    for (int32_t q = 0; q < tl.ns; ++q) {
        const int32_t s = tl.s0 + q;
        int best = 0;
        for (int w = 1; w < WAVES; ++w)
            if (load[w] < load[best]) best = w;
        deal[s] = make_int4(t, best, num[best], load[best]);
        load[best] += slices[s].width;
        num[best] += 1;
    }
    for (int w = 0; w < WAVES; ++w) {
        const int64_t r = ats_region(t0, t1, t, w, WAVES);
        rcnt[r] = num[w];
        rsteps[r] = load[w];
    }
}
// 10. one thread per (row block, wave): its slices, steps and groups
//     (rq / rso: exclusive prefixes of the regions' slices / steps, with the totals at the end)
template <int WAVES>
__global__ void ats_waves(const int32_t *__restrict__ rbt, int64_t nrb, const int32_t *__restrict__ rq,
                          const int32_t *__restrict__ rso, AWave *__restrict__ waves, int32_t *__restrict__ wgroups) {
    const int64_t bw = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (bw >= nrb * WAVES) return;
    const int64_t rb = bw / WAVES;
    const int w = (int)(bw % WAVES);
    const int32_t t0 = rbt[rb], t1 = rbt[rb + 1];
    const int64_t a = ats_region(t0, t1, t0, w, WAVES), b = a + (t1 - t0);
    AWave x;
    x.q0 = rq[a];
    x.cnt = rq[b] - rq[a];
    x.steps = rso[b] - rso[a];
    x.g0 = 0;
    waves[bw] = x;
    wgroups[bw] = (x.steps + 3) >> 2;
}
__global__ void ats_wave_g0(AWave *__restrict__ waves, const int32_t *__restrict__ wg0, int64_t nw) {
    const int64_t bw = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (bw < nw) waves[bw].g0 = wg0[bw];
}
// 11. one wave per slice: its list record and lane words, and its steps into
//     the wave's stream, every step for all 64 lanes (see attract_tiles_stream)
template <int WAVES>
__global__ void ats_fill(const ASlice *__restrict__ slices, int32_t nsl, const ATile *__restrict__ tiles,
                         const int32_t *__restrict__ rbt, const int4 *__restrict__ deal,
                         const int32_t *__restrict__ rq, const int32_t *__restrict__ rso,
                         const AWave *__restrict__ waves, const uint32_t *__restrict__ srow,
                         const uint16_t *__restrict__ pk, const double *__restrict__ pv, int2 *__restrict__ recs,
                         uint32_t *__restrict__ lword, uint8_t *__restrict__ stream) {
    const int64_t s = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (s >= nsl) return;
    const int lane = lane_id();
    const ASlice sd = slices[s];
    const int4 dl = deal[s];   // tile, wave, rank, first step in the region
    const int32_t rb = tiles[dl.x].rb, t0 = rbt[rb], t1 = rbt[rb + 1];
    const int64_t ra = ats_region(t0, t1, t0, dl.y, WAVES), r = ats_region(t0, t1, dl.x, dl.y, WAVES);
    const int64_t q = (int64_t)rq[r] + dl.z;
    const int64_t step0 = (int64_t)(rso[r] - rso[ra]) + dl.w;
    const int64_t g0 = waves[(int64_t)rb * WAVES + dl.y].g0;
    const uint32_t rl = srow[s * 64 + lane];
    const int len = (int)(rl & ((1u << AT_LENBITS) - 1));
    lword[q * 64 + lane] = rl;
    if (lane == 0) recs[q] = make_int2((int)((uint32_t)sd.width | ((uint32_t)sd.wide << 31)), dl.x);
    int64_t off = sd.base;
    // the lanes with entries are a prefix, so step 0's entry of this lane is at base + lane
    const uint16_t c0 = len > 0 ? pk[off + lane] : (uint16_t)0;
    for (int k = 0; k < sd.width; ++k) {
        uint16_t c = c0;
        double v = ATS_DEFECT == 1 ? 1e-7 : 0.0;
        if (k < len) {
            c = pk[off + lane];
            v = pv[off + lane];
        }
        off += __popcll(__ballot(k < len));
        const int64_t st = step0 + k;
        const int u = (int)(st & 3);
        uint8_t *gp = stream + (g0 + (st >> 2)) * ATS_GBYTES;
        *reinterpret_cast<double *>(gp + (u >> 1) * 1024 + lane * 16 + (u & 1) * 8) = v;
        *reinterpret_cast<uint16_t *>(gp + 2048 + lane * 8 + u * 2) = c;
    }
}

// ---- 3-D (nComponents = 3) attraction kernels
// q = 1 / (1 + metric(y_i, y_j)) on 3-D points (TsneHelpers.scala:293)
template <int MET>
__device__ __forceinline__ double qterm3(const double *a, const double *b) {
    double m;
    if (MET == TSNE_METRIC_COSINE) {
        double dt = 0.0, na = 0.0, nb = 0.0;
        for (int k = 0; k < 3; ++k) {
            dt = __dadd_rn(dt, __dmul_rn(a[k], b[k]));
            na = __dadd_rn(na, __dmul_rn(a[k], a[k]));
            nb = __dadd_rn(nb, __dmul_rn(b[k], b[k]));
        }
        m = 1.0 - dt / (sqrt(na) * sqrt(nb));
    } else {
        double s2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double d = __dsub_rn(a[k], b[k]);
            s2 = __dadd_rn(s2, __dmul_rn(d, d));
        }
        m = MET == TSNE_METRIC_EUCLIDEAN ? sqrt(s2) : s2;
    }
    const double x = 1.0 + m;
    double r = __builtin_amdgcn_rcp(x);
    r = __fma_rn(r, __fma_rn(-x, r, 1.0), r);
    r = __fma_rn(r, __fma_rn(-x, r, 1.0), r);
    return r;
}

// qterm3's q with x = 1 + metric returned too (the tiled 3-D attraction's
// loss terms P ln(P Z x) need no division); the same arithmetic as qterm3.
template <int MET>
__device__ __forceinline__ double qforce3_t(const double *a, const double *b, double &x) {
    double m;
    if (MET == TSNE_METRIC_COSINE) {
        double dt = 0.0, na = 0.0, nb = 0.0;
        for (int k = 0; k < 3; ++k) {
            dt = __dadd_rn(dt, __dmul_rn(a[k], b[k]));
            na = __dadd_rn(na, __dmul_rn(a[k], a[k]));
            nb = __dadd_rn(nb, __dmul_rn(b[k], b[k]));
        }
        m = 1.0 - dt / (sqrt(na) * sqrt(nb));
    } else {
        double s2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double d = __dsub_rn(a[k], b[k]);
            s2 = __dadd_rn(s2, __dmul_rn(d, d));
        }
        m = MET == TSNE_METRIC_EUCLIDEAN ? sqrt(s2) : s2;
    }
    x = 1.0 + m;
    double r = __builtin_amdgcn_rcp(x);
    r = __fma_rn(r, __fma_rn(-x, r, 1.0), r);
    r = __fma_rn(r, __fma_rn(-x, r, 1.0), r);
    return r;
}

// The tiled attraction in 3-D (round 6; the 2-D kernel attract_tiles above,
// same layout and loop): per tile the window's W points (24 B each, copied
// from Y as 16-byte pieces) and the row block's RB accumulators sit in LDS;
// each row of a 64-row slice is one lane, summing its entries of the tile in
// its own order with attract3's pair term (qterm3), then adding the sum to
// its accumulator -- one fixed order per row, no atomics.  Replaces
// attract3's Y_j gathers (24 B from a random line per entry: 0.03 of the
// HBM roofline in the C4 loop) by LDS reads.
template <class CF, bool LOSS, int MET>
__global__ __launch_bounds__(CF::NT) void attract_tiles3(
    const ATile *__restrict__ tiles, const int32_t *__restrict__ rbt, const ASlice *__restrict__ slices,
    const uint32_t *__restrict__ srow, int64_t rows, int64_t r0, int64_t n, const uint16_t *__restrict__ pk,
    const double *__restrict__ pv, const double *__restrict__ Y, const double *__restrict__ scal, double ex,
    int64_t xcd_chunk, double *__restrict__ attr, double *__restrict__ lpart, int64_t rbs) {
    constexpr int RB = CF::RB, W = CF::W, NT = CF::NT, WAVES = CF::WAVES;
    static_assert(W % 2 == 0, "window as 16-byte pieces (aligned)");
    __shared__ double2 win2[3 * W / 2];
    __shared__ double acc[3 * RB];
    __shared__ double sl[WAVES];
    const double *win = reinterpret_cast<const double *>(win2);
    const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const int64_t rb = xcd_chunk > 0 ? xcd_block_chunked(blockIdx.x, gridDim.x, xcd_chunk) : (int64_t)blockIdx.x;
    const int64_t b0 = rb * rbs;   // rbs <= RB rows per block (attract_layout_build)
    const int nr = (int)min(rbs, rows - b0);
    const double *Yrow = Y + 3 * (r0 + b0);
    for (int i = tid; i < 3 * nr; i += NT) acc[i] = 0.0;
    const double Z = LOSS ? scal[0] : 1.0;
    double lsum = 0.0;
    constexpr int WL = (3 * W / 2 + NT - 1) / NT;
    const int t0 = rbt[rb], t1 = rbt[rb + 1];
    for (int t = t0; t < t1; ++t) {
        const ATile tl = tiles[t];
        {   // the window's 3 wn doubles: 16-byte pieces (the odd last double of the last window alone)
            const int64_t base = (int64_t)tl.cb * W;
            const int wn = (int)min((int64_t)W, n - base);
            const int np = 3 * wn / 2;
            const double2 *src = reinterpret_cast<const double2 *>(Y + 3 * base);
            double2 yv[WL];
#pragma unroll
            for (int k = 0; k < WL; ++k) yv[k] = src[min(tid + k * NT, np - 1)];
#pragma unroll
            for (int k = 0; k < WL; ++k) {
                const int i = tid + k * NT;
                if (i < np) win2[i] = yv[k];
            }
            if ((3 * wn) & 1) {
                if (tid == 0) reinterpret_cast<double *>(win2)[3 * wn - 1] = Y[3 * (base + wn) - 1];
            }
        }
        __syncthreads();
        const int s0 = tl.s0, send = tl.s0 + tl.ns;
        int s = s0 + w;
        ASlice sd{};
        uint32_t rl = 0;
        if (s < send) {
            sd = slices[s];
            rl = srow[(int64_t)s * 64 + lane];
        }
        while (s < send) {
            const int len = (int)(rl & ((1u << AT_LENBITS) - 1)), lrow = (int)(rl >> AT_LENBITS);
            double yi[3] = {0.0, 0.0, 0.0};
            if (len > 0) { yi[0] = Yrow[3 * lrow]; yi[1] = Yrow[3 * lrow + 1]; yi[2] = Yrow[3 * lrow + 2]; }
            const int sn = s + WAVES;
            ASlice sdn{};
            uint32_t rln = 0;
            double f0 = 0.0, f1 = 0.0, f2 = 0.0;
            int64_t off = sd.base;
            for (int k0 = 0; k0 < sd.width; k0 += AT_U) {
                uint32_t cu[AT_U];
                double vu[AT_U];
#pragma unroll
                for (int u = 0; u < AT_U; ++u) {
                    const int k = k0 + u;
                    cu[u] = 0;
                    vu[u] = 0.0;
                    if (k < len) { cu[u] = pk[off + lane]; vu[u] = pv[off + lane]; }
                    off += __popcll(__ballot(len > k));
                }
                if (k0 == 0 && sn < send) {
                    sdn = slices[sn];
                    rln = srow[(int64_t)sn * 64 + lane];
                }
#pragma unroll
                for (int u = 0; u < AT_U; ++u) {
                    if (k0 + u < len) {
                        const double yj[3] = {win[3 * cu[u]], win[3 * cu[u] + 1], win[3 * cu[u] + 2]};
                        double x1m;
                        const double q = qforce3_t<MET>(yi, yj, x1m);
                        const double sc = __dmul_rn(vu[u], q);
                        f0 = __fma_rn(sc, __dsub_rn(yi[0], yj[0]), f0);
                        f1 = __fma_rn(sc, __dsub_rn(yi[1], yj[1]), f1);
                        f2 = __fma_rn(sc, __dsub_rn(yi[2], yj[2]), f2);
                        if (LOSS) {
                            const double pij = __dmul_rn(vu[u], ex);
                            lsum += pij * log_kl(pij * Z * x1m);
                        }
                    }
                }
            }
            if (sd.wide) {   // one row over the 64 lanes: a fixed-order tree
                f0 = wave_sum(f0);
                f1 = wave_sum(f1);
                f2 = wave_sum(f2);
                if (lane == 0) {
                    acc[3 * lrow] = __dadd_rn(acc[3 * lrow], f0);
                    acc[3 * lrow + 1] = __dadd_rn(acc[3 * lrow + 1], f1);
                    acc[3 * lrow + 2] = __dadd_rn(acc[3 * lrow + 2], f2);
                }
            } else if (len > 0) {
                acc[3 * lrow] = __dadd_rn(acc[3 * lrow], f0);
                acc[3 * lrow + 1] = __dadd_rn(acc[3 * lrow + 1], f1);
                acc[3 * lrow + 2] = __dadd_rn(acc[3 * lrow + 2], f2);
            }
            s = sn;
            sd = sdn;
            rl = rln;
        }
        __syncthreads();
    }
    for (int i = tid; i < 3 * nr; i += NT) attr[3 * b0 + i] = acc[i] * ex;
    if (LOSS) {
        lsum = wave_sum(lsum);
        if (lane == 0) sl[w] = lsum;
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int k = 0; k < WAVES; ++k) s += sl[k];
            lpart[blockIdx.x] = s;
        }
    }
}

// One wave per row (grid-stride), lanes over the row's entries, then a
// wave reduction: attr_i = sum_j ex P_ij q_ij (y_i - y_j); LOSS adds the KL
// terms into one partial per block (TsneHelpers.scala:269-306).  A lane's
// entries e, e + 64, ... are taken ATTR3_U at a time: their column and value
// loads, then their Y_j gathers, are all in flight before the first term is
// summed (C4: ~163 entries per row, one round); the sums keep the lane's
// entry order, so the result is the same to the bit.
constexpr int ATTR3_U = 4;
template <bool LOSS, int MET>
__global__ __launch_bounds__(256) void attract3(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                const double *__restrict__ val, int64_t r0, int64_t r1,
                                                const double *__restrict__ Y, const double *__restrict__ scal,
                                                double ex, double *__restrict__ attr, double *__restrict__ lpart) {
    __shared__ double sl[4];
    const int lane = lane_id();
    const double Z = LOSS ? scal[0] : 1.0;
    double lsum = 0.0;
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t i = r0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < r1; i += nw) {
        const double yi[3] = {Y[3 * i], Y[3 * i + 1], Y[3 * i + 2]};
        double f[3] = {0.0, 0.0, 0.0};
        const int64_t e1 = row_ptr[i + 1];
        for (int64_t eb = row_ptr[i] + lane; eb < e1; eb += 64 * ATTR3_U) {
            int64_t j[ATTR3_U];
            double pv[ATTR3_U];
#pragma unroll
            for (int u = 0; u < ATTR3_U; ++u) {
                const int64_t e = eb + 64 * u;
                j[u] = e < e1 ? (int64_t)col[e] : i;
                pv[u] = e < e1 ? val[e] : 0.0;
            }
            double yj[ATTR3_U][3];
#pragma unroll
            for (int u = 0; u < ATTR3_U; ++u)
#pragma unroll
                for (int k = 0; k < 3; ++k) yj[u][k] = Y[3 * j[u] + k];
#pragma unroll
            for (int u = 0; u < ATTR3_U; ++u) {
                if (eb + 64 * u >= e1) break;
                const double pij = __dmul_rn(pv[u], ex);
                const double q = qterm3<MET>(yi, yj[u]);
                const double sc = __dmul_rn(pij, q);
                for (int k = 0; k < 3; ++k) f[k] = __dadd_rn(f[k], __dmul_rn(sc, __dsub_rn(yi[k], yj[u][k])));
                if (LOSS) lsum += pij * log(pij / (q / Z));
            }
        }
        for (int k = 0; k < 3; ++k) {
            const double v = wave_sum(f[k]);
            if (lane == 0) attr[3 * (i - r0) + k] = v;
        }
    }
    if (LOSS) {
        lsum = wave_sum(lsum);
        if (lane == 0) sl[threadIdx.x >> 6] = lsum;
        __syncthreads();
        if (threadIdx.x == 0) lpart[blockIdx.x] = (sl[0] + sl[1]) + (sl[2] + sl[3]);
    }
}
}  // namespace

int64_t attract3_blocks(int64_t rows) { return std::max<int64_t>(1, std::min<int64_t>(8192, ceil_div(rows, 4))); }

// Upper bound of attract_launch's block count for rows rows.
// (rounded up to the XCD count like attract_grid's launch)
int64_t attract_max_blocks(int64_t rows) {
    return round_up(std::max<int64_t>(1, ceil_div(rows * 64, 256)), NUM_XCD);
}

namespace {

// attract_tiles3 over the tiled layout of the owned rows (3-D); returns the
// workgroups (the loss partials)
template <class CF, bool LOSS, int MET>
static void attract_tiles3_c(hipStream_t st, const AttractLayout &l, const AttractArgs &a, double *attr) {
    const int64_t nb = l.at_nrb;
    hipLaunchKernelGGL((attract_tiles3<CF, LOSS, MET>), dim3(nb), dim3(CF::NT), 0, st, l.at_tiles, l.at_rbt,
                       l.at_slices, l.at_srow, a.r1 - a.r0, a.r0, a.n, l.at_pk, l.at_pv, a.Y, a.scal, a.ex,
                       nb / NUM_XCD, attr, a.lpart, l.at_rbs);
}
template <bool LOSS, int MET>
static void attract_tiles3_m(hipStream_t st, const AttractLayout &l, const AttractArgs &a, double *attr) {
    if (l.at_cfg == 4) attract_tiles3_c<ATCfg3D, LOSS, MET>(st, l, a, attr);
    else attract_tiles3_c<ATCfg3Ds, LOSS, MET>(st, l, a, attr);
}
static int64_t attract_tiles3_launch(hipStream_t st, const AttractLayout &l, const AttractArgs &a, double *attr,
                                     bool loss) {
    const int metric = a.metric;
#define TSNE_AT3(L, M) attract_tiles3_m<L, M>(st, l, a, attr)
    if (metric == TSNE_METRIC_EUCLIDEAN) { if (loss) TSNE_AT3(true, TSNE_METRIC_EUCLIDEAN); else TSNE_AT3(false, TSNE_METRIC_EUCLIDEAN); }
    else if (metric == TSNE_METRIC_COSINE) { if (loss) TSNE_AT3(true, TSNE_METRIC_COSINE); else TSNE_AT3(false, TSNE_METRIC_COSINE); }
    else { if (loss) TSNE_AT3(true, TSNE_METRIC_SQEUCLIDEAN); else TSNE_AT3(false, TSNE_METRIC_SQEUCLIDEAN); }
#undef TSNE_AT3
    TSNE_LAUNCH_CHECK();
    return l.at_nrb;
}

static int64_t attract3_launch(hipStream_t st, const AttractArgs &a, double *attr, bool loss) {
    const int64_t blocks = attract3_blocks(a.r1 - a.r0);
    if (a.r1 <= a.r0) return 0;
    const int metric = a.metric;
#define TSNE_A3(L, M)                                                                                              \
    hipLaunchKernelGGL((attract3<L, M>), dim3(blocks), dim3(256), 0, st, a.rp, a.col, a.val, a.r0, a.r1, a.Y, a.scal, \
                       a.ex, attr, a.lpart)
    if (metric == TSNE_METRIC_EUCLIDEAN) { if (loss) TSNE_A3(true, TSNE_METRIC_EUCLIDEAN); else TSNE_A3(false, TSNE_METRIC_EUCLIDEAN); }
    else if (metric == TSNE_METRIC_COSINE) { if (loss) TSNE_A3(true, TSNE_METRIC_COSINE); else TSNE_A3(false, TSNE_METRIC_COSINE); }
    else { if (loss) TSNE_A3(true, TSNE_METRIC_SQEUCLIDEAN); else TSNE_A3(false, TSNE_METRIC_SQEUCLIDEAN); }
#undef TSNE_A3
    return blocks;
}

// persistent grid: bpc 256-thread blocks per CU (8: every wave slot), a
// multiple of the XCD count.  The gathers are bound by the CU's outstanding
// misses, not its waves: 3-4 blocks per CU run as fast as 8 and leave slots
// to a concurrent tree build.
static int64_t attract_grid(int64_t rows, int lpr, int bpc_req) {
    static const int cus = [] {
        int dev = 0, c = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev);
        return c;
    }();
    const int bpc = bpc_req > 0 ? std::min(bpc_req, 8) : 8;
    const int64_t full = round_up(cus * bpc, NUM_XCD);
    const int64_t need = round_up(std::max<int64_t>(1, ceil_div(rows * lpr, 256)), NUM_XCD);
    return std::min(full, need);
}

template <int LPR, int U, int MET>
static int64_t attract_launch_m(hipStream_t st, const AttractArgs &a, bool loss) {
    const int64_t rows = a.r1 - a.r0;
    const int64_t blocks = attract_grid(rows, LPR, a.bpc);
    if (loss)
        hipLaunchKernelGGL((attract_rows<LPR, U, true, MET>), dim3(blocks), dim3(256), 0, st, a.rp, a.col, a.val,
                           a.r0, a.r1, a.Y, a.scal, a.ex, a.attr, a.lpart);
    else
        hipLaunchKernelGGL((attract_rows<LPR, U, false, MET>), dim3(blocks), dim3(256), 0, st, a.rp, a.col, a.val,
                           a.r0, a.r1, a.Y, a.scal, a.ex, a.attr, a.lpart);
    return blocks;
}

template <int LPR, int U>
static int64_t attract_launch_v(hipStream_t st, const AttractArgs &a, bool loss) {
    switch (a.metric) {
        case TSNE_METRIC_EUCLIDEAN: return attract_launch_m<LPR, U, TSNE_METRIC_EUCLIDEAN>(st, a, loss);
        case TSNE_METRIC_COSINE: return attract_launch_m<LPR, U, TSNE_METRIC_COSINE>(st, a, loss);
        default: return attract_launch_m<LPR, U, TSNE_METRIC_SQEUCLIDEAN>(st, a, loss);
    }
}

// attract_rows: 64 lanes per row, 4 (col, val) loads then 4 Y_j gathers in
// flight per lane (16/32 lanes, 8/12 in flight measured slower, round 1)
static int64_t attract_launch(hipStream_t st, const AttractArgs &a, bool loss) {
    return attract_launch_v<64, 4>(st, a, loss);
}

// The optimizer's attraction: attract_tiles over the tiled layout when it was
// built, else attract_rows over the owned CSR rows.  Returns the blocks (loss
// partials) written.
template <class CF, bool LOSS, int MET>
static void attract_tiles_launch_c(hipStream_t st, const AttractLayout &l, const AttractArgs &a) {
    const int64_t nb = l.at_nrb;
#define TSNE_ATP(K)                                                                                            \
    hipLaunchKernelGGL(K, dim3(nb), dim3(CF::NT), 0, st, l.at_tiles, l.at_rbt, l.at_slices, l.at_srow,    \
                       a.r1 - a.r0, a.r0, a.n, l.at_pk, l.at_pv, a.Y, a.scal, a.ex, nb / NUM_XCD, a.attr, \
                       a.lpart, l.at_rbs)
    if constexpr (!LOSS) {
        if (l.at_stream) {   // built only with attract_pipe 0
            hipLaunchKernelGGL((attract_tiles_stream<CF, MET>), dim3(nb), dim3(CF::NT), 0, st, l.at_tiles, l.at_rbt,
                               l.ats_waves, l.ats_recs, l.ats_lword, l.ats_stream, a.r1 - a.r0, a.r0, a.n, a.Y,
                               a.ex, nb / NUM_XCD, a.attr, l.at_rbs);
            return;
        }
    }
    if constexpr (CF::RB == 4096 && !LOSS) {
        switch (l.at_pipe) {
            case 1: TSNE_ATP((attract_tiles_pipe<CF, 1, 6, LOSS, MET>)); return;
            case 2: TSNE_ATP((attract_tiles_pipe<CF, 1, 8, LOSS, MET>)); return;
            case 3: TSNE_ATP((attract_tiles_pipe<CF, 2, 4, LOSS, MET>)); return;
            case 4: TSNE_ATP((attract_tiles_pipe<CF, 2, 6, LOSS, MET>)); return;
            case 5: TSNE_ATP((attract_tiles_pipe<CF, 3, 4, LOSS, MET>)); return;
            default: break;
        }
    }
    // loss launches deal the slices round-robin: a wave's loss partial sums the
    // slices it ran, so claimed slices would make the loss's rounding vary
    if (l.at_dyn && !LOSS) TSNE_ATP((attract_tiles<CF, LOSS, MET, true>));
    else TSNE_ATP((attract_tiles<CF, LOSS, MET, false>));
#undef TSNE_ATP
}
template <bool LOSS, int MET>
static void attract_tiles_launch_m(hipStream_t st, const AttractLayout &l, const AttractArgs &a) {
    switch (l.at_cfg) {
        case 0: attract_tiles_launch_c<ATCfg0, LOSS, MET>(st, l, a); break;
        case 1: attract_tiles_launch_c<ATCfg1, LOSS, MET>(st, l, a); break;
        case 3: attract_tiles_launch_c<ATCfg3, LOSS, MET>(st, l, a); break;
        default: attract_tiles_launch_c<ATCfg2, LOSS, MET>(st, l, a); break;
    }
}
template <bool LOSS>
static void attract_tiles_launch_l(hipStream_t st, const AttractLayout &l, const AttractArgs &a) {
    switch (a.metric) {
        case TSNE_METRIC_EUCLIDEAN: attract_tiles_launch_m<LOSS, TSNE_METRIC_EUCLIDEAN>(st, l, a); break;
        case TSNE_METRIC_COSINE: attract_tiles_launch_m<LOSS, TSNE_METRIC_COSINE>(st, l, a); break;
        default: attract_tiles_launch_m<LOSS, TSNE_METRIC_SQEUCLIDEAN>(st, l, a); break;
    }
}

// Tile configuration for `rows` owned rows (Options::attract_cfg 0..3 forces one);
// 3-D: 4 (ATCfg3D) when its row blocks cover the CUs, else 5 (ATCfg3Ds)
static int at_cfg(tsne_ctx *ctx, int64_t rows, int C = 2) {
    if (C == 3) return ceil_div(rows, (int64_t)ATCfg3D::RB) >= ctx->cu_count - ctx->cu_count / 16 ? 4 : 5;
    if (ctx->opts.attract_cfg >= 0) return ctx->opts.attract_cfg;
    for (int c = 3; c > 0; --c)
        if (ceil_div(rows, (int64_t)512 << c) >= ctx->cu_count - ctx->cu_count / 16) return c;
    return 0;
}
}  // namespace

// The tiled layout of the owned rows (attract_tiles): a stable radix sort of
// the entries by (row block, column window, local row) -- within a row the
// entries keep their order -- then per tile its rows sorted by entry count
// (a second radix sort of the (tile, row) segments), 64-row slices, and the
// jagged-diagonal scatter of the column offsets and values.
// Skipped (attract_rows runs) for dense rows over a small embedding (C5: all
// of Y sits in one L2), for >= 2^31 owned entries, or with Options::attract_tiles = 0.
void attract_layout_build(tsne_ctx *ctx, AttractLayout &l, const int64_t *rpw, const int32_t *colw, const double *valw,
                          int64_t rows, int64_t n, int64_t nnz, int C, bool morton_labels) {
    const bool on = ctx->opts.attract_tiles != 0;
    hipStream_t st = ctx->stream;
    Workspace &ws = ctx->ws;
    l.at_on = false;
    // Only while the labels are P's graph order: once they follow the
    // embedding's Morton order, a row's Y_j are spatially local and
    // attract_rows' gathers hit the L2 (C3 loss launches: attract_rows 1.58
    // ms, attract_tiles 2.4 ms over t = 300..1000; in graph order 1.45 vs 1.11).
    // 3-D only with Options::attract_tiles3 (measured slower than attract3 at C4)
    if (!on || rows <= 0 || morton_labels || (C == 3 && !ctx->opts.attract_tiles3)) return;
    if (nnz / std::max<int64_t>(1, n) > 1024 && n * 16 <= (2 << 20)) return;
    int64_t m = 0;
    TSNE_HIP(hipMemcpyAsync(&m, rpw + rows, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    TSNE_HIP(hipStreamSynchronize(st));
    if (m <= 0 || m >= (int64_t)INT32_MAX) return;
    const int cfg = at_cfg(ctx, rows, C);
    const int rowbits = cfg == 0 ? ATCfg0::ROWBITS : cfg == 1 ? ATCfg1::ROWBITS : cfg == 2 ? ATCfg2::ROWBITS
                      : cfg == 3 ? ATCfg3::ROWBITS : cfg == 4 ? ATCfg3D::ROWBITS : ATCfg3Ds::ROWBITS;
    const int64_t W = cfg == 0 ? ATCfg0::W : cfg == 1 ? ATCfg1::W : cfg == 2 ? ATCfg2::W : cfg == 3 ? ATCfg3::W
                    : cfg == 4 ? ATCfg3D::W : ATCfg3Ds::W;
    // rows per block: the config's 2^rowbits, or fewer (a multiple of 64) so
    // that the row blocks cover every CU (C3: 3968 rows, 253 blocks, instead
    // of 245 blocks of 4096)
    const int64_t rbs = std::min<int64_t>((int64_t)1 << rowbits, round_up(ceil_div(rows, (int64_t)ctx->cu_count), 64));
    const int64_t nrb = ceil_div(rows, rbs), ncb = ceil_div(n, W);
    int bits = rowbits;
    for (uint64_t v = (uint64_t)(nrb * ncb - 1); v; v >>= 1) ++bits;
    uint64_t *key = ws.get<uint64_t>("opt.at.key", m), *key2 = ws.get<uint64_t>("opt.at.key2", m);
    int32_t *idx = ws.get<int32_t>("opt.at.idx", m), *idx2 = ws.get<int32_t>("opt.at.idx2", m);
    auto scan_i32 = [&](const int32_t *in, int32_t *out, int64_t cnt) {
        size_t b = 0;
        TSNE_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b, in, out, (int)cnt, st));
        TSNE_HIP(hipcub::DeviceScan::ExclusiveSum(ws.get<uint8_t>("opt.at.stmp", b), b, in, out, (int)cnt, st));
    };
    auto total = [&](const int32_t *excl, const int32_t *in, int64_t cnt) {   // excl[cnt-1] + in[cnt-1]
        int32_t h[2] = {0, 0};
        TSNE_HIP(hipMemcpyAsync(h, excl + cnt - 1, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        TSNE_HIP(hipMemcpyAsync(h + 1, in + cnt - 1, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        TSNE_HIP(hipStreamSynchronize(st));
        return h[0] + h[1];
    };
    // 1-2: entries sorted by (tile, local row), row order kept within a row
    hipLaunchKernelGGL(at_keys, dim3(ceil_div(rows, 4)), dim3(256), 0, st, rpw, colw, rows, ncb, rowbits, rbs, W,
                       key, idx);
    size_t tb = 0;
    TSNE_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, key, key2, idx, idx2, (int)m, 0, bits, st));
    TSNE_HIP(hipcub::DeviceRadixSort::SortPairs(ws.get<uint8_t>("opt.at.tmp", tb), tb, key, key2, idx, idx2, (int)m, 0,
                                                bits, st));
    uint16_t *cs = ws.get<uint16_t>("opt.at.cs", m);
    double *vs = ws.get<double>("opt.at.vs", m);
    int32_t *flag = ws.get<int32_t>("opt.at.flag", m), *sid = ws.get<int32_t>("opt.at.sid", m);
    hipLaunchKernelGGL(at_gather, dim3(ceil_div(m, 256)), dim3(256), 0, st, key2, idx2, m, ncb, rowbits, W, colw,
                       valw, cs, vs, flag);
    // 3: (tile, row) segments, sorted by tile and descending length
    scan_i32(flag, sid, m);
    const int32_t ns = total(sid, flag, m);
    int32_t *sstart = ws.get<int32_t>("opt.at.sstart", ns), *slen = ws.get<int32_t>("opt.at.slen", ns);
    uint64_t *skey = ws.get<uint64_t>("opt.at.skey", ns);
    uint64_t *okey = ws.get<uint64_t>("opt.at.okey", ns), *okey2 = ws.get<uint64_t>("opt.at.okey2", ns);
    int32_t *oval = ws.get<int32_t>("opt.at.oval", ns), *og = ws.get<int32_t>("opt.at.og", ns);
    hipLaunchKernelGGL(at_segs, dim3(ceil_div(m, 256)), dim3(256), 0, st, key2, flag, sid, m, sstart, skey);
    hipLaunchKernelGGL(at_seglen, dim3(ceil_div(ns, 256)), dim3(256), 0, st, sstart, skey, ns, m, rowbits, slen, okey,
                       oval);
    const int obits = bits - rowbits + AT_LENBITS;
    tb = 0;
    TSNE_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, okey, okey2, oval, og, (int)ns, 0, obits, st));
    TSNE_HIP(hipcub::DeviceRadixSort::SortPairs(ws.get<uint8_t>("opt.at.tmp", tb), tb, okey, okey2, oval, og, (int)ns,
                                                0, obits, st));
    // 4-5: tiles, their slices, slice bases (prefix of the sorted lengths)
    int64_t *lenj = ws.get<int64_t>("opt.at.lenj", ns), *ebase = ws.get<int64_t>("opt.at.ebase", ns);
    int32_t *tflag = ws.get<int32_t>("opt.at.tflag", ns), *tix = ws.get<int32_t>("opt.at.tix", ns);
    hipLaunchKernelGGL(at_sorted, dim3(ceil_div(ns, 256)), dim3(256), 0, st, okey2, og, slen, ns, lenj, tflag);
    {
        size_t b = 0;
        TSNE_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b, lenj, ebase, (int)ns, st));
        TSNE_HIP(hipcub::DeviceScan::ExclusiveSum(ws.get<uint8_t>("opt.at.stmp", b), b, lenj, ebase, (int)ns, st));
    }
    scan_i32(tflag, tix, ns);
    const int32_t nt = total(tix, tflag, ns);
    int32_t *tfirst = ws.get<int32_t>("opt.at.tfirst", nt), *tns = ws.get<int32_t>("opt.at.tns", nt);
    int32_t *ts0 = ws.get<int32_t>("opt.at.ts0", nt), *twide = ws.get<int32_t>("opt.at.twide", nt);
    l.at_tiles = ws.get<ATile>("opt.at.tiles", nt);
    hipLaunchKernelGGL(at_tilefirst, dim3(ceil_div(ns, 256)), dim3(256), 0, st, okey2, tflag, tix, ns, ncb, tfirst,
                       l.at_tiles);
    hipLaunchKernelGGL(at_tilecount, dim3(ceil_div(nt, 256)), dim3(256), 0, st, tfirst, lenj, nt, ns, tns, twide);
    scan_i32(tns, ts0, nt);
    const int32_t nsl = total(ts0, tns, nt);
    l.at_slices = ws.get<ASlice>("opt.at.slices", nsl);
    hipLaunchKernelGGL(at_slices, dim3(ceil_div(nt, 256)), dim3(256), 0, st, tfirst, tns, twide, ts0, lenj, ebase, nt,
                       ns, l.at_tiles, l.at_slices);
    // 6-7: the jagged-diagonal entries and the lane words
    l.at_srow = ws.get<uint32_t>("opt.at.srow", (size_t)nsl * 64);
    l.at_pk = ws.get<uint16_t>("opt.at.pk", m);
    l.at_pv = ws.get<double>("opt.at.pv", m);
    hipLaunchKernelGGL(at_fill, dim3(ceil_div(nsl, 4)), dim3(256), 0, st, l.at_slices, nsl, og, sstart, skey, lenj,
                       rowbits, cs, vs, l.at_srow, l.at_pk, l.at_pv);
    l.at_rbt = ws.get<int32_t>("opt.at.rbt", nrb + 1);
    hipLaunchKernelGGL(at_ranges, dim3(ceil_div(nt + 1, 256)), dim3(256), 0, st, l.at_tiles, nt, nrb, l.at_rbt);
    TSNE_LAUNCH_CHECK();
    if (debug_tiles()) {   // layout statistics: tiles, segments, slices, slice widths
        std::vector<ASlice> hs(nsl);
        TSNE_HIP(hipMemcpyAsync(hs.data(), l.at_slices, sizeof(ASlice) * nsl, hipMemcpyDeviceToHost, st));
        TSNE_HIP(hipStreamSynchronize(st));
        int64_t wsum = 0, wmax = 0;
        for (const ASlice &x : hs) { wsum += x.width; wmax = std::max<int64_t>(wmax, x.width); }

        fprintf(stderr, "[attract tiles] cfg=%d rows=%lld m=%lld nrb=%lld ncb=%lld tiles=%d segments=%d slices=%d "
                "width avg=%.2f max=%lld entries/slice=%.1f\n", cfg, (long long)rows, (long long)m, (long long)nrb,
                (long long)ncb, nt, ns, nsl, nsl ? (double)wsum / nsl : 0.0, (long long)wmax,
                nsl ? (double)m / nsl : 0.0);
    }
    // the stream layout (attract_tiles_stream): the 2-D non-loss launches'
    // storage of the same slices -- the arrays above stay, for the loss launches
    l.at_stream = false;
    l.at_pad_ppm = 0;
    if (ctx->opts.attract_stream && C == 2 && ctx->opts.attract_pipe == 0) {
        constexpr int WV = ATCfg3::WAVES;
        static_assert(ATCfg0::WAVES == WV && ATCfg1::WAVES == WV && ATCfg2::WAVES == WV, "one deal for every shape");
        const int64_t nreg = (int64_t)nt * WV, nwv = nrb * WV;
        int4 *deal = ws.get<int4>("opt.ats.deal", nsl);
        int32_t *rcnt = ws.get<int32_t>("opt.ats.rcnt", nreg + 1), *rsteps = ws.get<int32_t>("opt.ats.rsteps", nreg + 1);
        int32_t *rq = ws.get<int32_t>("opt.ats.rq", nreg + 1), *rso = ws.get<int32_t>("opt.ats.rso", nreg + 1);
        TSNE_HIP(hipMemsetAsync(rcnt + nreg, 0, sizeof(int32_t), st));
        TSNE_HIP(hipMemsetAsync(rsteps + nreg, 0, sizeof(int32_t), st));
        hipLaunchKernelGGL(ats_deal<WV>, dim3(ceil_div(nt, 64)), dim3(64), 0, st, l.at_tiles, nt, l.at_slices,
                           l.at_rbt, deal, rcnt, rsteps);
        scan_i32(rcnt, rq, nreg + 1);
        scan_i32(rsteps, rso, nreg + 1);
        l.ats_waves = ws.get<AWave>("opt.ats.waves", nwv);
        int32_t *wgroups = ws.get<int32_t>("opt.ats.wgroups", nwv), *wg0 = ws.get<int32_t>("opt.ats.wg0", nwv);
        hipLaunchKernelGGL(ats_waves<WV>, dim3(ceil_div(nwv, 256)), dim3(256), 0, st, l.at_rbt, nrb, rq, rso,
                           l.ats_waves, wgroups);
        scan_i32(wgroups, wg0, nwv);
        hipLaunchKernelGGL(ats_wave_g0, dim3(ceil_div(nwv, 256)), dim3(256), 0, st, l.ats_waves, wg0, nwv);
        const int64_t groups = total(wg0, wgroups, nwv);
        int32_t tsteps = 0;
        TSNE_HIP(hipMemcpyAsync(&tsteps, rso + nreg, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        TSNE_HIP(hipStreamSynchronize(st));
        // the lane words are read two list slots ahead: slack
        l.ats_stream = ws.get<uint8_t>("opt.ats.stream", (size_t)std::max<int64_t>(groups, 1) * ATS_GBYTES);
        l.ats_recs = ws.get<int2>("opt.ats.recs", (size_t)nsl + 2);
        l.ats_lword = ws.get<uint32_t>("opt.ats.lword", ((size_t)nsl + 2) * 64);
        TSNE_HIP(hipMemsetAsync(l.ats_lword + (size_t)nsl * 64, 0, 2 * 64 * sizeof(uint32_t), st));
        hipLaunchKernelGGL(ats_fill<WV>, dim3(ceil_div(nsl, 4)), dim3(256), 0, st, l.at_slices, nsl, l.at_tiles,
                           l.at_rbt, deal, rq, rso, l.ats_waves, l.at_srow, l.at_pk, l.at_pv, l.ats_recs,
                           l.ats_lword, l.ats_stream);
        TSNE_LAUNCH_CHECK();
        l.at_pad_ppm = (int64_t)tsteps * 64 * 1000000 / m;   // stored slots per real entry
        l.at_stream = true;
        if (debug_tiles())
            fprintf(stderr, "[attract stream] steps=%d groups=%lld stream=%.1f MB padding=%.4f (64 lanes a step; "
                    "%.4f with the streams' last groups)\n", tsteps, (long long)groups,
                    (double)groups * ATS_GBYTES / 1e6, (double)tsteps * 64 / (double)m,
                    (double)groups * 256 / (double)m);
    }
    l.at_nrb = nrb;
    l.at_ncb = ncb;
    l.at_rbs = rbs;
    l.at_cfg = cfg;
    l.at_pipe = ctx->opts.attract_pipe;
    l.at_dyn = ctx->opts.attract_dyn;
    l.at_on = true;
}

// attract_tiles only while the tree build takes the root-tile path: beside
// the BH traversal of the later phases its 156 KB of LDS per CU keeps the
// traversal's workgroups off those CUs (t = 180..300 at C3: 5.4 ms per
// concurrent launch vs 3.1 for attract_rows), and there the attraction is
// hidden behind the traversal anyway.
int64_t attract_launch_2d(hipStream_t st, const AttractLayout &l, const AttractArgs &a, bool loss) {
    // tiles in every phase while the labels are P's graph order (only in the
    // root-tile phase, attract_rows after it: whole C3 schedule 5.94 -> 6.40 s)
    if (!l.at_on) return attract_launch(st, a, loss);
    if (loss) attract_tiles_launch_l<true>(st, l, a);
    else attract_tiles_launch_l<false>(st, l, a);
    return l.at_nrb;
}

int64_t attract_launch_3d(hipStream_t st, const AttractLayout &l, const AttractArgs &a, double *attr3, bool loss) {
    return l.at_on ? attract_tiles3_launch(st, l, a, attr3, loss) : attract3_launch(st, a, attr3, loss);
}

}  // namespace tsne
