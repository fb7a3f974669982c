// csort.hpp -- the trees' Morton sort, using the previous build's order.
//
// Every optimizer iteration sorts all n points by their Morton key (bhtree /
// octree builds).  rocPRIM's radix sort of 64-bit keys takes ~190 us at
// n = 1M (its merge-sort path: ~20 launches), a quarter of the 2-D build.
// The embedding moves little between iterations, so the previous build's
// sorted order nearly sorts the new keys: P splitters taken from it at equal
// steps (oversampled 4x) cut the key range into buckets of ~1024 points, the points are
// scattered to their buckets (in the previous order: a workgroup's points
// fall into a few adjacent buckets), and each bucket is sorted in LDS.
// Output: keys ascending, ties by point index -- exactly the stable radix
// sort of (keys[i], i), whatever the previous order was (it only sets the
// bucket sizes; a bucket beyond the LDS capacity is sorted in global memory
// by its workgroup, correct and slower).
#pragma once
#include "common.hpp"

namespace tsne {

constexpr int MORTON2_LEVELS = 31;                  // 62 key bits
constexpr uint64_t MORTON2_OUT_KEY = 1ull << 63;    // outside the root cell: sorts last

// Morton key by replaying the reference cell arithmetic (no FMA contraction).
// Fast path: away from cell boundaries the replay's digits are those of the
// exact quantisation X = (p + W) / (2W) * 2^31 (every coarser boundary is
// also a level-31 boundary, and the reference's rounded cell centres sit
// within a few ulps of the exact ones), so a point whose fixed-point
// coordinates are more than 1e-4 of a level-31 cell away from every boundary
// takes the quantised digits; the rest (a fraction ~4e-4) and every
// out-of-range case replay the reference arithmetic.
__device__ __forceinline__ bool quant_digits(double p, double W, uint32_t &q) {
    const double t = (p + W) / (2.0 * W) * 2147483648.0;   // in [0, 2^31] for in-root points
    if (!(t >= 0.0 && t < 2147483648.0)) return false;
    const double f = floor(t);
    const double fr = t - f;
    // t carries <= ~3 ulp(2^31) = 1.4e-6 of rounding, the reference's cell
    // centres <= 31 roundings = 7.4e-6 (both in level-31 cell units): a band
    // of 1e-4 is far outside both
    if (fr < 1e-4 || fr > 1.0 - 1e-4) return false;          // near a boundary: replay
    q = (uint32_t)f;
    return true;
}

// The 2-D tree's key of point (px, py) in the root cell (0, 0, W): one device
// function for morton_keys (bhtree_build.hip) and the fused sort front end
// (csort_run_fused2), so both chains sort the same keys.
__device__ __forceinline__ uint64_t morton2_key(double px, double py, double W) {
    double x = 0.0, y = 0.0, hw = W, hh = W;
    const bool in = (__dsub_rn(x, hw) <= px) && (__dadd_rn(x, hw) >= px) && (__dsub_rn(y, hh) <= py) &&
                    (__dadd_rn(y, hh) >= py);
    uint64_t key = 0;
    uint32_t qx, qy;
    if (in && W > 0.0 && quant_digits(px, W, qx) && quant_digits(py, W, qy)) {
        // digit l: (west/east from x, north/south from y): q = 2 * south + east,
        // south = y below the centre = high bit of qy clear
        uint64_t k = 0;
        for (int l = 30; l >= 0; --l) {
            const uint32_t east = (qx >> l) & 1u, south = 1u - ((qy >> l) & 1u);
            k = (k << 2) | (uint64_t)(2u * south + east);
        }
        key = k;
    } else if (in) {
        for (int l = 0; l < MORTON2_LEVELS; ++l) {
            const double nw = __dmul_rn(0.5, hw), nh = __dmul_rn(0.5, hw);
            const double xw = __dsub_rn(x, nw), xe = __dadd_rn(x, nw);
            const double yn = __dadd_rn(y, nh), ys = __dsub_rn(y, nh);
            const bool inW = (__dsub_rn(xw, nw) <= px) && (__dadd_rn(xw, nw) >= px);
            const bool inE = (__dsub_rn(xe, nw) <= px) && (__dadd_rn(xe, nw) >= px);
            const bool inN = (__dsub_rn(yn, nh) <= py) && (__dadd_rn(yn, nh) >= py);
            const bool inS = (__dsub_rn(ys, nh) <= py) && (__dadd_rn(ys, nh) >= py);
            int q;
            if (inN && inW) q = 0;        // NW
            else if (inN && inE) q = 1;   // NE
            else if (inS && inW) q = 2;   // SW
            else q = 3;                   // SE (or a rounding gap: see header)
            x = (q & 1) ? xe : xw;
            y = (q & 2) ? ys : yn;
            hw = nw;
            hh = nh;
            key = (key << 2) | (uint64_t)q;
        }
    } else {
        key = MORTON2_OUT_KEY;
    }
    return key;
}

struct CoherentSort {
    int64_t n = 0;
    int32_t P = 0;                  // buckets
    uint64_t *split = nullptr;      // P sorted splitters (bucket b holds keys in [split[b], split[b + 1]))
    uint64_t *runs = nullptr;       // the sorted sample runs the splitters are merged from
    int32_t *cnt = nullptr;         // P bucket sizes
    int32_t *off = nullptr;         // P + 1 bucket offsets
    int32_t *cur = nullptr;         // P scatter cursors
    int32_t *bkt = nullptr;         // n: bucket of element j (the previous order's j-th point)
    uint64_t *kb = nullptr;         // 3n: bucketed keys [0, n), then the oversized buckets' scratch
                                    // (bucket at offset o: [n + 2 o, n + 2 o + 2 m), power-of-two padded)
    int32_t *vb = nullptr;          // 3n: bucketed point indices, the same layout
    int32_t *stat = nullptr;        // [0] oversized buckets of the last sort, [1] their running total (diagnostics)
    uint64_t *kst = nullptr;        // n: element j's key, staged by cs_count for cs_scatter (the fused 2-D chain)
};

// What the 2-D tree build takes from the sorted order, written by the fused
// chain's bucket workgroups instead of by count_in_root, gather_sorted and
// dup_count (bhtree_build.hip; the same values).
struct Csort2Out {
    double2 *pos;       // pos[s] = Y[idx_sorted[s]]
    int32_t *inv;       // inv[idx_sorted[s]] = s
    int32_t *meta;      // meta[0] += the bucket's in-root keys (zero before the sort; the sum: count_in_root's m)
    int32_t *dupc;      // dup_count's three outputs
    int32_t *vid;
    int32_t *dflag;
};

// Buffers for n points (ctx workspace, names pre + field).  n outside
// [CSORT_MIN_N, CSORT_MAX_N]: nothing (the callers keep rocPRIM's sort).
constexpr int64_t CSORT_MIN_N = 16384;
// Above 1024 x 1.2k points the mean bucket outgrows the LDS sort's 4k capacity
// at the measured 3.3x bucket skew (cs_split_runs) and whole buckets would take the
// slow global-memory bitonic path: rocPRIM's sort there.
constexpr int64_t CSORT_MAX_N = 1250000;
void csort_alloc(tsne_ctx *ctx, CoherentSort &cs, int64_t n, const std::string &pre);
// keys[p] for points p < n -> keys_sorted / idx_sorted ascending by (key, p).
// prev_idx_sorted: the previous sort's idx_sorted (a permutation of [0, n));
// it may be the same buffer as idx_sorted (read before it is written).
void csort_run(tsne_ctx *ctx, CoherentSort &cs, const uint64_t *keys, const int32_t *prev_idx_sorted,
               uint64_t *keys_sorted, int32_t *idx_sorted, hipStream_t st);
// The 2-D build's fused chain (Options::build_fuse): the same keys_sorted /
// idx_sorted from Y (n x 2) and the root half-width *W directly -- the keys
// are computed where they are first needed (morton2_key), the cursor fill and
// the offset scan ride in cs_split_rank and cs_scatter, and the bucket
// workgroups also write out (5 launches for 11).
void csort_run_fused2(tsne_ctx *ctx, CoherentSort &cs, const double *Y, const double *W,
                      const int32_t *prev_idx_sorted, uint64_t *keys_sorted, int32_t *idx_sorted,
                      const Csort2Out &out, hipStream_t st);
// Oversized buckets of the last csort_run, or (total) of every run since the
// allocation (synchronises the context's stream; 0 if none ran).
int64_t csort_oversized(tsne_ctx *ctx, const CoherentSort &cs, bool total = false);

}  // namespace tsne
