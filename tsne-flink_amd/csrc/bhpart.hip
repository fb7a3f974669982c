// bhpart.hip -- the quadtree's helpers for several ranks: cost-balanced query
// slices (bh_balance) and the tree partition's cuts (part_align, part_recut,
// part_cost; see "Tree partition" in bhtree.hip).  They share REF_FORCED and
// PART_LEVEL (bhtree_impl.hpp) with the traversal, and nothing else.
#include "bhtree_impl.hpp"

namespace tsne {

// Cost-balanced query slices for the next iteration: one 1024-thread block
// scans the (all-reduced, so identical on every rank) 256-query bucket costs
// and cuts the sorted order into world pieces of equal cost.
__global__ __launch_bounds__(1024) void balance_slices(const unsigned long long *__restrict__ bcost, int64_t nb,
                                                       int64_t n, int world, int64_t *__restrict__ bounds) {
    __shared__ unsigned long long part[1024];
    __shared__ unsigned long long total;
    const int t = threadIdx.x;
    const int64_t per = (nb + 1023) / 1024, b0 = t * per, b1 = min(nb, b0 + per);
    unsigned long long acc = 0;
    for (int64_t b = b0; b < b1; ++b) acc += bcost[b];
    part[t] = acc;
    __syncthreads();
    if (t == 0) {
        unsigned long long run = 0;
        for (int k = 0; k < 1024; ++k) { const unsigned long long v = part[k]; part[k] = run; run += v; }
        total = run;
        bounds[0] = 0;
        bounds[world] = n;
        for (int r = 1; r < world; ++r)   // a zero target cuts at 0; the scan sets the others
            bounds[r] = (run / world * r + (run % world) * r / world) == 0 ? 0 : n;
    }
    __syncthreads();
    // thread t owns buckets [b0, b1) with exclusive prefix part[t]
    unsigned long long run = part[t];
    for (int64_t b = b0; b < b1; ++b) {
        const unsigned long long nxt = run + bcost[b];
        for (int r = 1; r < world; ++r) {
            const unsigned long long target = total / world * r + (total % world) * r / world;
            if (run < target && nxt >= target) bounds[r] = min(n, (b + 1) << 8);
        }
        run = nxt;
    }
    __syncthreads();
    if (t == 0) {   // all-zero costs: equal counts; keep the cuts monotone
        for (int r = 1; r < world; ++r) {
            if (total == 0) bounds[r] = n * r / world;
            if (bounds[r] < bounds[r - 1]) bounds[r] = bounds[r - 1];
        }
    }
}

void bh_balance(tsne_ctx *ctx, const unsigned long long *bcost, int64_t n, int world, int64_t *bounds) {
    hipLaunchKernelGGL(balance_slices, dim3(1), dim3(1024), 0, ctx->stream, bcost, ceil_div(n, 256), n, world, bounds);
    TSNE_LAUNCH_CHECK();
}

// ---- tree partition (several ranks; see REF_FORCED)
// One wave: cut r (1 <= r < world) moved forward to the first sorted position p
// with p == m or a level-PART_LEVEL cell boundary between keys p - 1 and p.
__global__ void part_align_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ meta,
                                  const int64_t *__restrict__ cuts, int world, int rank, int32_t *__restrict__ plim) {
    const int lane = lane_id();
    const int64_t m = meta[0];
    constexpr int SH = 62 - 2 * PART_LEVEL;
    auto align = [&](int r) -> int64_t {
        if (r <= 0) return 0;
        if (r >= world) return INT32_MAX;
        int64_t c = min(max(cuts[r], (int64_t)0), m);
        if (c <= 0 || c >= m) return c;
        for (int64_t b = c; b < m; b += 64) {
            const int64_t p = b + lane;
            const bool hit = p >= m || (keys[p - 1] >> SH) != (keys[p] >> SH);
            const uint64_t bl = __ballot(hit);
            if (bl) return b + __ffsll((long long)bl) - 1;
        }
        return m;
    };
    const int64_t lo = align(rank), hi = align(rank + 1);
    if (lane == 0) {
        plim[0] = (int32_t)lo;
        plim[1] = (int32_t)max(lo, hi);
    }
}

// One thread: equal-cost cuts of the cumulative cost, linear inside each
// rank's current range, moved half way from the current cuts.
__global__ void part_recut_kernel(const unsigned long long *__restrict__ cost, int world, int64_t n,
                                  int64_t *__restrict__ cuts) {
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int r = 0; r < world; ++r) total += (double)cost[r];
    if (!(total > 0.0)) return;
    double nc[64];
    int r = 0;
    double cum = 0.0;
    for (int k = 1; k < world && k < 64; ++k) {
        const double T = total * k / world;
        while (r < world - 1 && cum + (double)cost[r] <= T) cum += (double)cost[r++];
        const double x0 = (double)cuts[r], x1 = (double)(r + 1 < world ? cuts[r + 1] : n);
        const double f = cost[r] > 0 ? (T - cum) / (double)cost[r] : 0.5;
        nc[k] = x0 + f * (x1 - x0);
    }
    for (int k = 1; k < world && k < 64; ++k) {
        int64_t v = (int64_t)(0.5 * ((double)cuts[k] + nc[k]));
        v = max(v, cuts[k - 1]);
        cuts[k] = min(v, n);
    }
}

// Sum of the traversal waves' costs (pops + tile points / 64).
__global__ __launch_bounds__(1024) void part_cost_kernel(const int32_t *__restrict__ wcost, int64_t waves,
                                                         unsigned long long *__restrict__ out) {
    __shared__ unsigned long long red[16];
    unsigned long long a = 0;
    for (int64_t i = threadIdx.x; i < waves; i += 1024) a += (unsigned long long)max(wcost[i], 0);
    a = wave_sum(a);
    if (lane_id() == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int k = 0; k < 16; ++k) t += red[k];
        *out = t;
    }
}

void part_align(tsne_ctx *ctx, BHTree &t, const int64_t *cuts, int world, int rank, int32_t *plim) {
    TSNE_REQUIRE(world <= 64, "tree partition: at most 64 ranks");
    TSNE_REQUIRE(2 * t.n < (int64_t)REF_FORCED, "tree partition: too many points for the record flags");
    hipLaunchKernelGGL(part_align_kernel, dim3(1), dim3(64), 0, ctx->stream, t.keys_sorted, t.meta, cuts, world, rank,
                       plim);
    TSNE_LAUNCH_CHECK();
}

void part_recut(tsne_ctx *ctx, const unsigned long long *cost, int world, int64_t n, int64_t *cuts) {
    hipLaunchKernelGGL(part_recut_kernel, dim3(1), dim3(64), 0, ctx->stream, cost, world, n, cuts);
    TSNE_LAUNCH_CHECK();
}

void part_cost(tsne_ctx *ctx, BHTree &t, int64_t waves, unsigned long long *out) {
    hipLaunchKernelGGL(part_cost_kernel, dim3(1), dim3(1024), 0, ctx->stream, t.wcost, waves, out);
    TSNE_LAUNCH_CHECK();
}

}  // namespace tsne
