// bhtree.hip -- Barnes-Hut repulsion over a built quadtree (TsneHelpers.scala:227-264,
// QuadTree.scala:128-142) on gfx950: the traversal, the leaf tiles and moment
// evaluations it records, and the options around them ("Narrow layout",
// "Spill", "Tile streaming").  The build is bhtree_build.hip; what the two
// share is bhtree_impl.hpp.
//
// What bh_repulsion expects of the tree bh_build left (BHTree, bhtree.hpp):
//  * pos: the points in sorted (Morton) order; idx_sorted / inv between
//    sorted positions and rows; dupc: the exact copies of each sorted point;
//  * meta[0] = m, the in-root points (sorted positions [0, m)), meta[1] the
//    root ref; nodes[0, m - 1): the binary nodes with counts, centres of mass,
//    boxes, hmin and rball; qrec: the quad record of every real node (and the
//    virtual chain tops at [n, 2n)), built for this theta and near_dmax;
//  * mom / mom_flag: the subtree moments about the box centres -- or
//    mom_deferred, and bh_repulsion launches them (bh_moments) itself;
//  * root_tile: no tree at all, only nodes[0]'s box and count, the root's
//    polynomial coefficients rcoef and root_pos (the points in label order).
#include <hipcub/hipcub.hpp>

#include "bhtree_impl.hpp"

namespace tsne {
namespace {

constexpr int STACK = 320;                 // batch pops (<= 8 cells) while <= STACK/2 entries, then
                                           // depth-first (+3 per level, <= 35 levels): never overflows
constexpr int QREC_V4 = sizeof(QRec) / 16; // 16-byte pieces of a record
constexpr int MOM_TASKS = 128;  // moment evaluations recorded per query; more -> dense tiles
__host__ __device__ constexpr double fact(int k) { return k <= 1 ? 1.0 : k * fact(k - 1); }
__host__ __device__ constexpr double binom(int k, int i) { return fact(k) / (fact(i) * fact(k - i)); }

// 1/x for the BH terms: v_rcp_f64 + one Newton step, within 11 ulp of the
// IEEE quotient over the whole range (scripts/rcp_accuracy.hip: rcp alone
// 2.5e8 ulp, one step 11, two steps 0) -- ~2e-15 relative per term, far
// below the 1e-6 near-exact and 1e-4 gradient bars, two fp64 ops per term
// cheaper than the correctly rounded pair of steps.
__device__ __forceinline__ double recip_bh(double x) {
    const double r = __builtin_amdgcn_rcp(x);
    return __fma_rn(r, __fma_rn(-x, r, 1.0), r);
}

// Direct interaction of one lane's query with one leaf point (QuadTree.scala:
// 128-142 at a leaf: cumSize 1, com = the point; zero if equal to the query).
__device__ __forceinline__ void leaf_force(double qx, double qy, double px, double py, double &fx,
                                           double &fy, double &zs) {
    if (px == qx && py == qy) return;
    const double dx = qx - px, dy = qy - py;
    const double D = __fma_rn(dx, dx, dy * dy);
    const double r = recip_bh(1.0 + D);
    const double sc = r * r;
    fx = __fma_rn(sc, dx, fx);
    fy = __fma_rn(sc, dy, fy);
    zs += r;
}

// Masked forms for the traversal's child loop: every lane evaluates, `take`
// selects whether the term is added (a zero term leaves the sums bit-equal).
// Branch-free, so the accumulators are updated in place -- the branchy forms
// made the compiler copy fx, fy, zs at every merge of the divergent paths.
__device__ __forceinline__ void leaf_force_m(bool take, double qx, double qy, double px, double py, double &fx,
                                             double &fy, double &zs) {
    take = take && !(px == qx && py == qy);
    const double dx = qx - px, dy = qy - py;
    const double D = __fma_rn(dx, dx, dy * dy);
    const double r = recip_bh(1.0 + D);
    const double sc = r * r;
    fx = __fma_rn(take ? sc : 0.0, dx, fx);
    fy = __fma_rn(take ? sc : 0.0, dy, fy);
    zs += take ? r : 0.0;
}

// Pair term for dense tiles, without the equality test (see the caller):
// r = 1/(1 + dx^2 + dy^2) with the 1 folded into the FMA chain.
__device__ __forceinline__ void pair_force(double qx, double qy, double px, double py, double &fx,
                                           double &fy, double &zs) {
    const double dx = qx - px, dy = qy - py;
    const double r = recip_bh(__fma_rn(dx, dx, __fma_rn(dy, dy, 1.0)));
    const double sc = r * r;
    fx = __fma_rn(sc, dx, fx);
    fy = __fma_rn(sc, dy, fy);
    zs += r;
}
// pair_force's term added only with `take` (else + 0: the sums bit-equal)
__device__ __forceinline__ void pair_force_m(bool take, double qx, double qy, double px, double py, double &fx,
                                             double &fy, double &zs) {
    const double dx = qx - px, dy = qy - py;
    const double r = recip_bh(__fma_rn(dx, dx, __fma_rn(dy, dy, 1.0)));
    const double sc = r * r;
    fx = __fma_rn(take ? sc : 0.0, dx, fx);
    fy = __fma_rn(take ? sc : 0.0, dy, fy);
    zs += take ? r : 0.0;
}
// pair_force_m with the mask on r alone: without `take` r = 0, so sc = 0 * 0 = 0
// and every sum takes the same + 0 (the bits of pair_force_m, two selects fewer)
__device__ __forceinline__ void pair_force_r(bool take, double qx, double qy, double px, double py, double &fx,
                                             double &fy, double &zs) {
    const double dx = qx - px, dy = qy - py;
    const double r0 = recip_bh(__fma_rn(dx, dx, __fma_rn(dy, dy, 1.0)));
    const double r = take ? r0 : 0.0;
    const double sc = r * r;
    fx = __fma_rn(sc, dx, fx);
    fy = __fma_rn(sc, dy, fy);
    zs += r;
}

// omega_i (z) and phi_i (F) weights of S_i = sum D^i, Sx_i = sum D^i w, for
// A = |v|^2.
__device__ __forceinline__ void moment_weights(double A, double *om, double *ph) {
    const double B = 1.0 / (1.0 + A);
    {
        double Ap[MOM_ORDER + 1], Bp[MOM_ORDER + 3];
        Ap[0] = 1.0; Bp[0] = 1.0;
#pragma unroll
        for (int k = 1; k <= MOM_ORDER; ++k) Ap[k] = Ap[k - 1] * A;
#pragma unroll
        for (int k = 1; k <= MOM_ORDER + 2; ++k) Bp[k] = Bp[k - 1] * B;
#pragma unroll
        for (int i = 0; i <= MOM_ORDER; ++i) {
            double so = 0.0, sp = 0.0;
#pragma unroll
            for (int k = 0; k <= MOM_ORDER; ++k) {
                if (k < i) continue;
                so += binom(k, i) * Ap[k - i] * Bp[k + 1];
                sp += (k + 1) * binom(k, i) * Ap[k - i] * Bp[k + 2];
            }
            om[i] = (i & 1) ? -so : so;
            ph[i] = (i & 1) ? sp : -sp;
        }
    }
}

// Subtree sums for one lane's query from the node's moments (see the header).
// Returns z += sum 1/(1+D), (fx, fy) += sum (q - y)/(1+D)^2 over the subtree's
// points, the query itself and its exact duplicates included (D = 0: they add
// 1 to z and 0 to F; the traversal subtracts them).
__device__ __forceinline__ void moment_eval(const double *mu, double vx, double vy, double &fx, double &fy,
                                            double &zs) {
    double om[MOM_ORDER + 1], ph[MOM_ORDER + 1];
    moment_weights(vx * vx + vy * vy, om, ph);
    // shift to the query: w = u - v; X[e] = (-v_x)^e / e!
    double X[MOM_DEG + 1], Yv[MOM_DEG + 1];
    X[0] = 1.0; Yv[0] = 1.0;
#pragma unroll
    for (int e = 1; e <= MOM_DEG; ++e) {
        X[e] = X[e - 1] * (-vx) * (1.0 / e);
        Yv[e] = Yv[e - 1] * (-vy) * (1.0 / e);
    }
    double z = 0.0, gx = 0.0, gy = 0.0;
#pragma unroll
    for (int a = 0; a <= MOM_DEG; ++a) {
        double lam[MOM_DEG + 1];         // lam[b'] = sum_a' mu(a', b') X[a - a']
#pragma unroll
        for (int b1 = 0; b1 <= MOM_DEG; ++b1) {
            if (a + b1 > MOM_DEG) continue;
            double t = 0.0;
#pragma unroll
            for (int a1 = 0; a1 <= MOM_DEG; ++a1)
                if (a1 <= a) t = __fma_rn(mu[midx(a1, b1)], X[a - a1], t);
            lam[b1] = t;
        }
#pragma unroll
        for (int b = 0; b <= MOM_DEG; ++b) {
            if (a + b > MOM_DEG) continue;
            if ((a & 1) && (b & 1)) continue;
            if (!(a & 1) && !(b & 1) && a + b > 2 * MOM_ORDER) continue;
            double nu = 0.0;   // nu(a, b) / (a! b!) = sum_j w_x^a w_y^b / (a! b!)
#pragma unroll
            for (int b1 = 0; b1 <= MOM_DEG; ++b1)
                if (b1 <= b) nu = __fma_rn(lam[b1], Yv[b - b1], nu);
            if (!(a & 1) && !(b & 1)) {
                const int i = (a + b) / 2;
                z = __fma_rn(om[i] * (binom(i, a / 2) * fact(a) * fact(b)), nu, z);
            } else if (a & 1) {
                const int i = (a + b - 1) / 2;
                gx = __fma_rn(ph[i] * (binom(i, (a - 1) / 2) * fact(a) * fact(b)), nu, gx);
            } else {
                const int i = (a + b - 1) / 2;
                gy = __fma_rn(ph[i] * (binom(i, a / 2) * fact(a) * fact(b)), nu, gy);
            }
        }
    }
    zs += z;
    fx += gx;
    fy += gy;
}

template <int D>
__device__ __forceinline__ double poly_eval(const double *__restrict__ c, double vx, double vy) {
    double acc = 0.0;
#pragma unroll
    for (int p = D; p >= 0; --p) {
        const int o = p * (D + 1) - p * (p - 1) / 2;
        double r = c[o + D - p];
#pragma unroll
        for (int q = D - p - 1; q >= 0; --q) r = __fma_rn(r, vy, c[o + q]);
        acc = p == D ? r : __fma_rn(acc, vx, r);
    }
    return acc;
}

template <int I>
__device__ __forceinline__ void poly_terms(const double *__restrict__ c, double vx, double vy, const double *om,
                                           const double *ph, double &z, double &gx, double &gy) {
    if constexpr (I <= MOM_ORDER) {
        z = __fma_rn(om[I], poly_eval<2 * I>(c + poly_off_z(I), vx, vy), z);
        gx = __fma_rn(ph[I], poly_eval<2 * I + 1>(c + poly_off_x(I), vx, vy), gx);
        gy = __fma_rn(ph[I], poly_eval<2 * I + 1>(c + poly_off_y(I), vx, vy), gy);
        poly_terms<I + 1>(c, vx, vy, om, ph, z, gx, gy);
    }
}

// moment_eval from the subtree's polynomial coefficients (poly_coef).
__device__ __forceinline__ void poly_moment_eval(const double *__restrict__ coef, double vx, double vy, double &fx,
                                                 double &fy, double &zs) {
    double om[MOM_ORDER + 1], ph[MOM_ORDER + 1];
    moment_weights(vx * vx + vy * vy, om, ph);
    double z = 0.0, gx = 0.0, gy = 0.0;
    poly_terms<0>(coef, vx, vy, om, ph, z, gx, gy);
    zs += z;
    fx += gx;
    fy += gy;
}

// Truncation test of the moment path for query q and a subtree's bounding box.
__device__ __forceinline__ bool moment_ok(double bx0, double bx1, double by0, double by1, double qx, double qy,
                                          double tol) {
    double cx, cy, R;
    box_centre(bx0, bx1, by0, by1, cx, cy, R);
    const double vx = qx - cx, vy = qy - cy;
    const double A = vx * vx + vy * vy;
    const double rho = (R * R + 2.0 * sqrt(A) * R) / (1.0 + A) * (1.0 + 1e-12);
    if (!(rho < 0.25)) return false;
    double rp = rho;
#pragma unroll
    for (int k = 0; k < MOM_ORDER; ++k) rp *= rho;
    return (MOM_ORDER + 2) * rp <= tol * (1.0 - rho) * (1.0 - rho);
}

// Moment tasks of each query (query slots [g0, g1): sorted positions, or
// qlist[slot] when a rank computes a list of them), in traversal order, added
// to the traversal's F and z.
// Tile chunks (TSNE_TILE_CHUNK=0: off): a traversal wave whose tile cost
// (points + 16 per task) exceeds 2x the mean (and 4096) has its tile list cut
// into C contiguous index ranges, each a tile_apply wave of its own.  Chunk
// slots write partial sums (Fp, Zp) and moment lists per slot lane;
// chunk_combine adds them to F, Z in chunk order: deterministic.
struct ChunkView {
    const int32_t *slot_w = nullptr, *slot_c = nullptr, *nslots = nullptr;
    double2 *Fp = nullptr;
    double *Zp = nullptr;
};
constexpr int CHUNK_MAX = 32;
constexpr int CHUNK_MIN = 4096;
__global__ void chunk_total(const int32_t *__restrict__ tcost, int64_t waves, unsigned long long *__restrict__ total) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long c = w < waves ? (unsigned long long)max(tcost[w], 0) : 0ull;
    const unsigned long long ws = wave_sum(c);
    if (lane_id() == 0 && ws) atomicAdd(total, ws);
}
__global__ void chunk_parts(const int32_t *__restrict__ tcost, const unsigned long long *__restrict__ total,
                            int64_t waves, int32_t *__restrict__ Cw, const int32_t *__restrict__ claims, int32_t gen,
                            int32_t *__restrict__ wout, double frac) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w > waves) return;
    if (w == waves) { Cw[w] = 0; return; }
    // ceil(2 total / waves): the extra chunks sum to <= total / target <= waves / 2,
    // inside the slot capacity (waves + waves / 2 + 64, bh_alloc)
    const unsigned long long W = (unsigned long long)max<int64_t>(waves, 1);
    const long long target = max((long long)CHUNK_MIN, (long long)((2 * (*total) + W - 1) / W));
    if (wout && w == 0) *wout = (int32_t)min(2.0e9, frac * (double)target);
    // (tile streaming: a handed-over list is one chunk, whichever path sums it)
    Cw[w] = claims && (claims[w] >> 2) == gen ? 1
                                              : 1 + (int32_t)min((long long)(CHUNK_MAX - 1),
                                                                 (long long)max(tcost[w], 0) / target);
}
__global__ void chunk_fill(int32_t *__restrict__ Cw, int32_t *__restrict__ slot0,
                           const int32_t *__restrict__ tcost, int64_t waves, int32_t *__restrict__ slot_w,
                           int32_t *__restrict__ slot_c, int32_t *__restrict__ scost, int64_t slots_max,
                           int32_t *__restrict__ nslots) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // the plan fits by construction (chunk_parts); should it not, every wave
    // falls back to one slot (C = 1) rather than a chunk being dropped
    const bool fits = slot0[waves] <= slots_max;
    if (w == waves) *nslots = fits ? slot0[waves] : (int32_t)waves;
    if (w < waves && !fits) {
        Cw[w] = 1;
        slot0[w] = (int32_t)w;
        slot_w[w] = (int32_t)w;
        slot_c[w] = 1 << 16;
        scost[w] = tcost[w];
    } else if (w < waves) {
        const int C = Cw[w];
        for (int j = 0; j < C; ++j) {
            slot_w[slot0[w] + j] = (int32_t)w;
            slot_c[slot0[w] + j] = j | (C << 16);
            scost[slot0[w] + j] = tcost[w] / C;
        }
    }
    // slots past the plan: no work, lowest cost
    for (int64_t k = (fits ? slot0[waves] : waves) + w; w <= waves && k < slots_max; k += waves + 1) scost[k] = 0;
}
// The whole chunk plan and the longest-first tile_apply block order in ONE
// workgroup (replacing chunk_total / chunk_parts / a scan / chunk_fill and
// the block sort: ~13 launches of a few us each at 1M).  Same chunk counts,
// slots and fallback as those kernels; the block order is by cost bucket
// (4 per doubling, descending; the order within a bucket is unspecified --
// tile_apply's sums do not depend on the order its blocks run in).
constexpr int PLAN_WAVES_MAX = 16384;    // traversal waves whose costs the plan stages in LDS
constexpr int PLAN_BLOCKS_MAX = (PLAN_WAVES_MAX + PLAN_WAVES_MAX / 2 + 64 + 3) / 4;   // tile_apply blocks (4 slots each)
constexpr int PLAN_BUCKETS = 128;
__device__ __forceinline__ int plan_bucket(int32_t c) {
    return c <= 0 ? 0 : min(PLAN_BUCKETS - 1, 1 + (int)(4.0f * __log2f((float)c)));
}
// hist[key] += 1 for every active lane of the wave, one LDS atomic per
// distinct key (per-lane atomics serialise on the few cost buckets most
// entries share -- late in the schedule nearly all in bucket 0); returns the
// lane's slot (old value + its rank among the wave's lanes of that key).
__device__ __forceinline__ int32_t wave_bucket_add(int32_t *hist, int key, bool act) {
    const int lane = lane_id();
    int32_t res = 0;
    uint64_t rem = __ballot(act);
    while (rem) {
        const int leader = __builtin_ctzll(rem);
        const int kb = __shfl(key, leader, 64);
        const bool mine = act && key == kb;
        const uint64_t m = __ballot(mine);
        int32_t b0 = 0;
        if (lane == leader) b0 = atomicAdd(&hist[kb], (int32_t)__popcll(m));
        b0 = __shfl(b0, leader, 64);
        if (mine) res = b0 + (int32_t)__popcll(m & lanemask_lt());
        rem &= ~m;
    }
    return res;
}
__global__ __launch_bounds__(1024) void tile_plan(const int32_t *__restrict__ tcost, int64_t waves, int64_t slots_max,
                                                  int32_t *__restrict__ Cw, int32_t *__restrict__ slot0,
                                                  int32_t *__restrict__ slot_w, int32_t *__restrict__ slot_c,
                                                  int32_t *__restrict__ nslots, int32_t *__restrict__ torder,
                                                  const int32_t *__restrict__ claims, int32_t gen,
                                                  int32_t *__restrict__ wout, double frac) {
    __shared__ int32_t bc[PLAN_BLOCKS_MAX];
    __shared__ int32_t tc[PLAN_WAVES_MAX];
    __shared__ unsigned long long red[16];
    __shared__ int32_t wtot[16];
    __shared__ int32_t hist[PLAN_BUCKETS];
    __shared__ int32_t sfits;
    const int t = threadIdx.x, lane = lane_id(), w = t >> 6;
    const int64_t tblocks = (slots_max + 3) / 4;
    // total tile cost
    unsigned long long acc = 0;
    for (int64_t v = t; v < waves; v += 1024) {
        const int32_t c = max(tcost[v], 0);
        tc[v] = c;
        acc += (unsigned long long)c;
    }
    acc = wave_sum(acc);
    if (lane == 0) red[w] = acc;
    for (int64_t b = t; b < tblocks; b += 1024) bc[b] = 0;
    if (t < PLAN_BUCKETS) hist[t] = 0;
    __syncthreads();
    unsigned long long total = 0;
    for (int k = 0; k < 16; ++k) total += red[k];
    // ceil(2 total / waves): the extra chunks sum to <= waves / 2 (bh_alloc's slot capacity)
    const unsigned long long Wd = (unsigned long long)max<int64_t>(waves, 1);
    const long long target = max((long long)CHUNK_MIN, (long long)((2 * total + Wd - 1) / Wd));
    // (tile streaming: a handed-over list is one chunk, whichever path sums it)
    auto chunks = [&](int64_t v) {
        if (claims && (claims[v] >> 2) == gen) return 1;
        return 1 + (int32_t)min((long long)(CHUNK_MAX - 1), (long long)tc[v] / target);
    };
    if (wout && t == 0) *wout = (int32_t)min(2.0e9, frac * (double)target);
    // this thread's contiguous run of waves and its slot count
    const int64_t per = (waves + 1023) / 1024, v0 = min(waves, t * per), v1 = min(waves, v0 + per);
    int32_t loc = 0;
    for (int64_t v = v0; v < v1; ++v) loc += chunks(v);
    int32_t inc = loc;   // exclusive scan over the 1024 threads: waves, then wave totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t x = __shfl_up(inc, o, 64);
        if (lane >= o) inc += x;
    }
    if (lane == 63) wtot[w] = inc;
    __syncthreads();
    int32_t base = inc - loc, S = 0;
    for (int k = 0; k < 16; ++k) {
        if (k < w) base += wtot[k];
        S += wtot[k];
    }
    if (t == 0) sfits = S <= slots_max;
    __syncthreads();
    const bool fits = sfits != 0;   // else every wave one slot, rather than a chunk dropped
    int32_t run = base;
    for (int64_t v = v0; v < v1; ++v) {
        const int32_t c = fits ? chunks(v) : 1;
        const int32_t s0 = fits ? run : (int32_t)v;
        Cw[v] = c;
        slot0[v] = s0;
        const int32_t sc = tc[v] / c;
        for (int j = 0; j < c; ++j) {
            slot_w[s0 + j] = (int32_t)v;
            slot_c[s0 + j] = j | (c << 16);
            if (torder) atomicMax(&bc[(s0 + j) >> 2], sc);
        }
        run += c;
    }
    if (t == 0) {
        Cw[waves] = 0;
        slot0[waves] = fits ? S : (int32_t)waves;
        *nslots = fits ? S : (int32_t)waves;
    }
    if (!torder) return;
    __syncthreads();
    // the blocks' cost buckets (wave_bucket_add); the order within a bucket is free
    for (int64_t b0 = (int64_t)w * 64; b0 < tblocks; b0 += 1024) {
        const int64_t b = b0 + lane;
        (void)wave_bucket_add(hist, b < tblocks ? plan_bucket(bc[b]) : 0, b < tblocks);
    }
    __syncthreads();
    if (t == 0) {   // descending bucket starts
        int32_t r = 0;
        for (int k = PLAN_BUCKETS - 1; k >= 0; --k) { const int32_t c = hist[k]; hist[k] = r; r += c; }
    }
    __syncthreads();
    for (int64_t b0 = (int64_t)w * 64; b0 < tblocks; b0 += 1024) {
        const int64_t b = b0 + lane;
        const int32_t pos = wave_bucket_add(hist, b < tblocks ? plan_bucket(bc[b]) : 0, b < tblocks);
        if (b < tblocks) torder[pos] = (int32_t)b;
    }
}

// F, Z of each query += its chunks' partial sums, in chunk order
__global__ void chunk_combine(const double2 *__restrict__ Fp, const double *__restrict__ Zp,
                              const int32_t *__restrict__ Cw, const int32_t *__restrict__ slot0, int64_t g0, int64_t g1,
                              const int32_t *__restrict__ qlist, double2 *__restrict__ F, double *__restrict__ Z,
                              int32_t *__restrict__ pcost, const int32_t *__restrict__ idx_sorted,
                              const int32_t *__restrict__ wcost, const int32_t *__restrict__ nflag) {
    const int64_t k = g0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= g1) return;
    if (pcost) {   // option trav_front_cur: the point's wave cost (a narrow group's: heavy)
        const int64_t wq = (k - g0) >> 6;
        pcost[idx_sorted[k]] = nflag && nflag[wq] ? (1 << 29) : wcost[wq];
    }
    const int64_t w = (k - g0) >> 6, lane = (k - g0) & 63;
    const int64_t s = qlist ? (int64_t)qlist[k] : k;
    const int64_t b = (int64_t)slot0[w] * 64 + lane;
    double fx = 0.0, fy = 0.0, z = 0.0;
    for (int j = 0; j < Cw[w]; ++j) {
        const double2 g = Fp[b + 64 * j];
        fx += g.x; fy += g.y;
        z += Zp[b + 64 * j];
    }
    if (fx != 0.0 || fy != 0.0 || z != 0.0) {
        const double2 f = F[s];
        F[s] = make_double2(f.x + fx, f.y + fy);
        Z[s] = Z[s] + z;
    }
}

__global__ __launch_bounds__(256) void moment_apply(const double2 *__restrict__ pos,
                                                    const BHNode *__restrict__ nodes,
                                                    const double *__restrict__ mom,
                                                    const int32_t *__restrict__ mtask,
                                                    const int32_t *__restrict__ mtask_n, int64_t g0,
                                                    int64_t g1, const int32_t *__restrict__ qlist,
                                                    double2 *__restrict__ F, double *__restrict__ Z,
                                                    ChunkView cv) {
    // entry = query slot, or (tile chunks) chunk slot lane with partial sums Fp / Zp
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t k = g0 + i;
    if (cv.slot_w) {
        if ((i >> 6) >= *cv.nslots) return;
        k = g0 + (int64_t)cv.slot_w[i >> 6] * 64 + (i & 63);
    }
    if (k >= g1) return;
    const int64_t s = qlist ? (int64_t)qlist[k] : k;
    const int64_t e = cv.slot_w ? i : s;
    const int nt = mtask_n[e];
    if (nt == 0) return;
    const double2 q = pos[s];
    double fx = 0.0, fy = 0.0, zs = 0.0;
    for (int t = 0; t < nt; ++t) {
        const int node = mtask[e * MOM_TASKS + t];
        double cx, cy, R;
        box_centre(nodes[node], cx, cy, R);
        moment_eval(mom + (int64_t)node * MOM_K, q.x - cx, q.y - cy, fx, fy, zs);
    }
    double2 *Fo = cv.slot_w ? cv.Fp : F;
    double *Zo = cv.slot_w ? cv.Zp : Z;
    const double2 f = Fo[e];
    Fo[e] = make_double2(f.x + fx, f.y + fy);
    Zo[e] = Zo[e] + zs;
}

// Moment tasks of the narrow groups' queries (their own lists, entry = heavy
// slot x 64 + query), added to F, Z after the narrow traversal's sums.
__global__ __launch_bounds__(256) void narrow_moment_apply(const double2 *__restrict__ pos,
                                                           const BHNode *__restrict__ nodes,
                                                           const double *__restrict__ mom,
                                                           const int32_t *__restrict__ hlist,
                                                           const int32_t *__restrict__ hcount,
                                                           const int32_t *__restrict__ mtask,
                                                           const int32_t *__restrict__ mtask_n, int64_t g0, int64_t g1,
                                                           const int32_t *__restrict__ qlist, double2 *__restrict__ F,
                                                           double *__restrict__ Z) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ((e >> 6) >= (int64_t)*hcount) return;
    const int64_t k = g0 + (int64_t)hlist[e >> 6] * 64 + (e & 63);
    if (k >= g1) return;
    const int nt = mtask_n[e];
    if (nt == 0) return;
    const int64_t s = qlist ? (int64_t)qlist[k] : k;
    const double2 q = pos[s];
    double fx = 0.0, fy = 0.0, zs = 0.0;
    for (int t = 0; t < nt; ++t) {
        const int node = mtask[e * MOM_TASKS + t];
        double cx, cy, R;
        box_centre(nodes[node], cx, cy, R);
        moment_eval(mom + (int64_t)node * MOM_K, q.x - cx, q.y - cy, fx, fy, zs);
    }
    const double2 f = F[s];
    F[s] = make_double2(f.x + fx, f.y + fy);
    Z[s] = Z[s] + zs;
}

// fl(h / D) < theta -- the reference's max(hHeigth, hWidth) / D < theta with
// an IEEE division -- decided by comparing h with theta * D outside a 1e-14
// relative band (where the rounded quotient cannot cross theta), and by the
// exact division inside it.  Df may be the FMA-evaluated D (within 1 ulp of
// the reference's dx*dx + dy*dy); the exact path recomputes the latter.
// D = 0 or denormal gives h > theta D: opened, as h / 0 = inf is not < theta.
__device__ __forceinline__ bool summarise(double h, double Df, double dx, double dy, double th_lo, double th_hi,
                                          double theta) {
    if (h < th_lo * Df) return true;
    if (h > th_hi * Df) return false;
    const double D = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
    return h / D < theta;
}

// One summarised cell (QuadTree.scala:134-142): Q = 1/(1+D), m = n Q.
__device__ __forceinline__ void cell_force(double dx, double dy, double D, int32_t n, double &fx, double &fy,
                                           double &zs) {
    const double Q = recip_bh(1.0 + D);
    const double mult = (double)n * Q;
    const double sc = mult * Q;
    fx = __fma_rn(sc, dx, fx);
    fy = __fma_rn(sc, dy, fy);
    zs += mult;
}

// Traversal: one wave = 64 consecutive sorted queries sharing an LDS stack of
// (cell, lane mask) entries, one per cell that some lane OPENS.  Popping a
// cell loads its quad record once; every lane that opened it then takes its
// own reference decision for each quad child from the record (a leaf
// interacts; a cell is summarised when max(hW,hH)/D < theta, else pushed with
// the mask of the lanes that open it).  Fast path on pop: if for a lane EVERY
// real cell of the subtree would be opened, the reference would reach every
// leaf of it, so the lane sums the subtree's leaves directly (moment task or
// dense tile over the contiguous range of sorted points).  That is the
// near-exact regime of a small embedding.
// Two conservative all-open tests, either suffices (rounding margins kept):
//  * ball: |q - com|^2 <= rball^2, where ball(com, rball) lies inside every
//    descendant cell's "opened" disc |q - c_u|^2 <= h_u / theta (bottom_up);
//  * box: max squared distance from q to the subtree's bounding box
//    <= hmin / theta (hmin = smallest real cell half-width inside).
// A third test admits subtrees whose reference sum provably equals the exact
// leaf sum to BH_NEAR_TOL relative: a cell c is summarised only when
// h_c < theta D, and replacing its n_c points by their centre of mass changes
// sum 1/(1+D) by at most (8 + 32 D) h_c^2 n_c (second-order Taylor; the first
// order vanishes at the centre of mass) and sum (q-y)/(1+D)^2 by at most
// ~24 sqrt(D) h_c^2 n_c.  With every point of the subtree within
// D <= near_dmax of q (box corners), the relative deviation is below
// ~48 theta^2 near_dmax^2 <= BH_NEAR_TOL (bh_near_dmax).  In the tiny-embedding
// phase (extent ~1e-3) the root passes for every query: one moment task each.
// Dense leaf tiles are not run inside the traversal: the wave appends (leaf
// range, lane mask) to its own task list (DENSE_CAP entries; when full, the
// lanes simply keep traversing the subtree -- the reference's own path) and
// dense_apply sums the tiles afterwards.  This keeps the traversal at <= 64
// VGPRs (8 waves per SIMD to hide the record fetches) instead of ~100.

// ---- Narrow layout for heavy 64-query groups.
// A wave's BH work is the depth-first walk of its shared stack; its span is
// the serial chain pop -> record fetch -> child tests -> push.  In dense
// clusters a few 64-query groups carry 10-20x the mean work (DESIGN.md 6,
// "BH mid phase") and that chain alone sets the grid's span.  Such groups
// (previous traversal cost >= Options::narrow x the mean, narrow_select) run
// as NPARTS waves of NQ queries each, with the lanes laid out as (record k,
// query q, child c): one pass takes NKP stack entries at once and evaluates
// the 4 children of each for NQ queries in ONE sweep of the lanes, where the
// 64-query layout spends 4 sweeps (one per child) per entry with most lanes
// masked off.  The stack entries carry NQ-bit query masks.  All-open /
// near-exact tiles are summed inline (the 4 child lanes of a query split the
// subtree's points) or become moment tasks on the group's own lists
// (narrow_moment_apply).  Each lane keeps its own partial sums; the NKP x 4
// lanes of a query are added by a fixed xor butterfly at the end, so the
// result does not depend on timing (it differs from the 64-query layout's
// association only at rounding level: the same cells are summarised, the
// same leaves and tiles summed).
constexpr int NQ_LOG = 2;
constexpr int NQ = 1 << NQ_LOG;    // queries per narrow wave
constexpr int NKP = 16 / NQ;       // stack entries per narrow pass
constexpr int NPARTS = 64 / NQ;    // narrow waves per 64-query group (NPARTS / 4 workgroups)
static_assert(NKP * NQ * 4 == 64 && NPARTS % 4 == 0 && STACK / 2 + 4 * NKP + 3 * 32 <= STACK, "narrow lane layout, stack bound");

// bits {4 i : i < NQ} of x (one query per 4 lanes) -> bits {i}
__device__ __forceinline__ uint32_t narrow_compress(uint64_t x) {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < NQ; ++i) m |= (uint32_t)((x >> (4 * i)) & 1ull) << i;
    return m;
}
// lanes (k, q, c = 0) for every record slot k: query q's first lane in each
__host__ __device__ constexpr uint64_t narrow_qcol0() {
    uint64_t m = 0;
    for (int k = 0; k < NKP; ++k) m |= 1ull << (k * 4 * NQ);
    return m;
}

struct NarrowView {
    const int32_t *hlist = nullptr;    // heavy slot -> 64-query group
    const int32_t *hcount = nullptr;   // [0] heavy groups this traversal
    int32_t *ncost = nullptr;          // per heavy slot x part: the narrow wave's cost (next selection)
    int32_t *mtask = nullptr;          // per heavy slot x 64 queries: moment tasks (MOM_TASKS each)
    int32_t *mtask_n = nullptr;
    const int32_t *nflag = nullptr;    // per group: heavy slot + 1, or 0 (the 64-query layout)
    int32_t nbn = 0;                   // workgroups of the narrow part of the grid (hmax x NPARTS / 4)
    unsigned long long *wlog = nullptr;   // STATS + option wave_log: per-wave timeline (wave_log_put)
};

// Option wave_log (counting calls only): every traversal / narrow / tile wave
// appends (start, end << 2 | kind) in 100 MHz wall ticks; wlog[0] counts.
constexpr int64_t WAVE_LOG_CAP = 1 << 17;
__device__ __forceinline__ void wave_log_put(unsigned long long *wlog, unsigned long long t0, unsigned long long t1,
                                             int kind) {
    if (!wlog) return;
    const unsigned long long k = atomicAdd(wlog, 1ull);
    if (k < (unsigned long long)WAVE_LOG_CAP) {
        wlog[1 + 2 * k] = t0;
        wlog[2 + 2 * k] = (t1 << 2) | (unsigned long long)kind;
    }
}

// Tree partition (several ranks, bh_repulsion with `plim`): rank r owns the
// sorted positions [lo, hi) and walks every query over the cells that hold
// points of its own.  The cuts sit on boundaries of level-PART_LEVEL cells
// (part_align), so at most PART_LEVEL levels of records straddle a cut.  A
// record inside [lo, hi) takes the normal path; a straddling ("shared") one
// the slow path of bh_traverse<., true>: a child without points of mine is
// skipped, an opened one pushed, and a child's term (summarised cell, leaf,
// duplicate leaf or key-tie group) is taken only by the rank owning the
// child's first point -- so over the ranks every term of the reference's sum
// is taken exactly once.  A shared record that passes the all-open /
// near-exact test for a lane is an exact leaf sum for it: its children are
// pushed with REF_FORCED (lanes in exact-sum mode); a forced record of mine
// becomes one tile task (the exact leaf sum over its range), a forced shared
// one is expanded again.  The sum over the ranks of these parts is the
// record's exact leaf sum, up to rounding and the moments' 1e-12 truncation.
// (REF_FORCED, PART_LEVEL: bhtree_impl.hpp, shared with part_align in bhpart.hip)

// The traversal kernels' state (LDS per WPB-wave block): KB records per batch
// (4 in the 64-query layout, NKP in the narrow one).
template <int KB, int WPB = 4>
struct TravLDS_T {
    QRec srec[WPB][KB];          // first: the record fields' LDS offsets fit the ds_read2 immediates
    int32_t sref[WPB][STACK];
    uint64_t smask[WPB][STACK];
    int32_t bref[WPB][KB];       // the batch's refs (its masks ride in the records' lmask)
};
using TravLDS = TravLDS_T<4, TRAV_WPB>;
using NarrowLDS = TravLDS_T<(NKP > 4 ? NKP : 4)>;

// The LDS copy of a popped record under option trav_burst: QRec's 8-byte
// pieces regrouped so that what one step of a pop needs lies in whole 16-byte
// pieces -- the four words and {ex, lmask} the pop starts from, and per child
// {ccx, ccy} and {cb, ca} -- read with one ds_read_b128 each (RecHead,
// RecChild).  QRec itself (HBM; build_qrec, the narrow kernel, transform.hip)
// is unchanged: stage_records<., true> permutes while staging.
struct __attribute__((aligned(16))) QRecB {
    double cx, cy, rball, hmin, bx0, bx1, by0, by1;
    int32_t first, last, cnt, nch;
    double ex;
    uint64_t lmask;
    struct { double ccx, ccy, cb, ca; } ch[4];
    int32_t cref[4], ccnt[4];
};
static_assert(sizeof(QRecB) == sizeof(QRec) && offsetof(QRecB, first) == offsetof(QRec, first) &&
              offsetof(QRecB, ch) == 96 && offsetof(QRecB, cref) == 224, "QRecB: a permutation of QRec's pieces");

// Stage the records of stack entries [sp, sp + k) of wave w into LDS (one
// round of coalesced 16-byte loads; their latencies overlap), each with its
// entry's lane mask in the copy's lmask slot (read with the record's other
// fields from one LDS address).  BURST: in QRecB's order (each lane's two
// 8-byte halves to their places).
template <class LDS, bool BURST = false>
__device__ __forceinline__ void stage_records(LDS &L, int w, int lane, int sp, int k,
                                              const QRec *__restrict__ qrec) {
    // (BURST: the lane's addresses are recomputed per batch, a few VALU, instead of
    // living in ~10 VGPRs across the pop loop, which needs them for the bursts)
    if (BURST) asm volatile("" : "+v"(lane));
    static_assert(offsetof(QRec, lmask) == 16 * (QREC_V4 - 1) + 8, "lmask: the upper half of the last 16 bytes");
    static_assert(!BURST || (QREC_V4 == 16 && offsetof(QRec, ccx) == 80 && offsetof(QRec, cref) == 208 &&
                             offsetof(QRec, ex) == 240), "the permutation below is QRec's layout");
    if (lane < k) L.bref[w][lane] = L.sref[w][sp + lane];
    for (int e = lane; e < QREC_V4 * k; e += 64) {
        const int rr = e / QREC_V4, part = e - rr * QREC_V4;
        const int rf = L.sref[w][sp + rr] & ~REF_FORCED;
        uint4 v = reinterpret_cast<const uint4 *>(qrec + rf)[part];
        if (part == QREC_V4 - 1) {
            const uint64_t m = L.smask[w][sp + rr];
            v.z = (uint32_t)m;
            v.w = (uint32_t)(m >> 32);
        }
        if (BURST) {
            // halves 2 part, 2 part + 1 of QRec -> halves d0, d1 of QRecB
            int d0 = 2 * part, d1 = d0 + 1;                   // the tile fields, first .. nch: in place
            if (part >= 5 && part < 13) {                     // ccx, ccy, cb, ca [c, c + 1] -> ch[c], ch[c + 1]
                const int j = 2 * part - 10;
                d0 = 12 + 4 * (j & 3) + (j >> 2);
                d1 = d0 + 4;
            } else if (part >= 13) {                          // cref, ccnt: one piece on; {ex, lmask}: piece 5
                d0 = part == 15 ? 10 : 2 * part + 2;
                d1 = d0 + 1;
            }
            uint64_t *dst = reinterpret_cast<uint64_t *>(&L.srec[w][rr]);
            dst[d0] = ((uint64_t)v.y << 32) | v.x;
            dst[d1] = ((uint64_t)v.w << 32) | v.z;
        } else {
            reinterpret_cast<uint4 *>(&L.srec[w][rr])[part] = v;
        }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);   // vmcnt = lgkmcnt = 0: batch staged in LDS
    __builtin_amdgcn_wave_barrier();
}

// The fields of a popped record as the 64-query pop loop reads them (option
// trav_burst).  <false>: in place, each at its first use (the compiler waits
// for every LDS round trip where its value is needed: a chain of ~10 per
// pop).  <true>: fetch() issues all reads of a step at once, from the QRecB
// copy, in the order their values are needed; LDS returns in order, so the
// waits the compiler places are partial counts and one round trip covers the
// step.  The loads are volatile so that they stay where they are issued; the
// values, and everything computed from them, are the same.
typedef double f64x2_t __attribute__((ext_vector_type(2)));
typedef int32_t i32x4_t __attribute__((ext_vector_type(4)));
typedef uint64_t u64x2_t __attribute__((ext_vector_type(2)));
template <class T> __device__ __forceinline__ T lds_fetch(const void *p) {
    typedef const volatile __attribute__((address_space(3))) T *lds_ptr;
    return *(lds_ptr)(const __attribute__((address_space(3))) void *)p;
}
// Two points of the sorted positions fetched ahead (option tile_prefetch): the
// 16 bytes at each of two 32-bit byte offsets from the wave-uniform base (the
// loads' scalar-base form: no 64-bit address per lane).  The loads are issued
// where pos_issue2 stands and nothing waits for them there; pos_wait2 on the
// same pair, with exactly one later pos_issue2 in between, waits until all
// but that later pair have landed (loads return in order); pos_drain waits
// for every one.  A pair must not be read, copied or assigned between its
// issue and its wait: the compiler takes the values for present at the issue.
__device__ __forceinline__ void pos_issue2(const double2 *base, uint32_t o0, uint32_t o1, f64x2_t &x0, f64x2_t &x1) {
    asm volatile("global_load_dwordx4 %0, %2, %4\n\tglobal_load_dwordx4 %1, %3, %4"
                 : "=&v"(x0), "=&v"(x1) : "v"(o0), "v"(o1), "s"(base) : "memory");
}
__device__ __forceinline__ void pos_wait2(f64x2_t &x0, f64x2_t &x1) {
    asm volatile("s_waitcnt vmcnt(2)" : "+v"(x0), "+v"(x1) : : "memory");
}
__device__ __forceinline__ void pos_drain(f64x2_t &x0, f64x2_t &x1, f64x2_t &y0, f64x2_t &y1) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(x0), "+v"(x1), "+v"(y0), "+v"(y1) : : "memory");
}
template <bool BURST> struct RecHead;
template <> struct RecHead<false> {
    const QRec *nd;
    const int32_t *br;
    __device__ __forceinline__ void fetch(const QRec *rec, const int32_t *bref) { nd = rec; br = bref; }
    __device__ __forceinline__ int32_t ref() const { return *br; }
    __device__ __forceinline__ uint64_t lmask() const { return nd->lmask; }
    __device__ __forceinline__ int32_t nch() const { return nd->nch; }
    __device__ __forceinline__ int32_t first() const { return nd->first; }
    __device__ __forceinline__ int32_t last() const { return nd->last; }
    __device__ __forceinline__ int32_t cnt() const { return nd->cnt; }
    __device__ __forceinline__ double cx() const { return nd->cx; }
    __device__ __forceinline__ double cy() const { return nd->cy; }
    __device__ __forceinline__ double rball() const { return nd->rball; }
    __device__ __forceinline__ double hmin() const { return nd->hmin; }
    __device__ __forceinline__ double bx0() const { return nd->bx0; }
    __device__ __forceinline__ double bx1() const { return nd->bx1; }
    __device__ __forceinline__ double by0() const { return nd->by0; }
    __device__ __forceinline__ double by1() const { return nd->by1; }
    __device__ __forceinline__ double ex() const { return nd->ex; }
};
template <> struct RecHead<true> {
    i32x4_t ids;     // first, last, cnt, nch
    u64x2_t em;      // ex (bits), lmask
    int32_t rf;
    f64x2_t c, rh, bx, by;
    // the three words the pop's scalar state comes from first, then the tile test's
    __device__ __forceinline__ void fetch(const QRec *rec, const int32_t *bref) {
        const QRecB *b = reinterpret_cast<const QRecB *>(rec);
        ids = lds_fetch<i32x4_t>(&b->first);
        em = lds_fetch<u64x2_t>(&b->ex);
        rf = lds_fetch<int32_t>(bref);
        c = lds_fetch<f64x2_t>(&b->cx);
        rh = lds_fetch<f64x2_t>(&b->rball);
        bx = lds_fetch<f64x2_t>(&b->bx0);
        by = lds_fetch<f64x2_t>(&b->by0);
    }
    __device__ __forceinline__ int32_t ref() const { return rf; }
    __device__ __forceinline__ uint64_t lmask() const { return em.y; }
    __device__ __forceinline__ int32_t nch() const { return ids.w; }
    __device__ __forceinline__ int32_t first() const { return ids.x; }
    __device__ __forceinline__ int32_t last() const { return ids.y; }
    __device__ __forceinline__ int32_t cnt() const { return ids.z; }
    __device__ __forceinline__ double cx() const { return c.x; }
    __device__ __forceinline__ double cy() const { return c.y; }
    __device__ __forceinline__ double rball() const { return rh.x; }
    __device__ __forceinline__ double hmin() const { return rh.y; }
    __device__ __forceinline__ double bx0() const { return bx.x; }
    __device__ __forceinline__ double bx1() const { return bx.y; }
    __device__ __forceinline__ double by0() const { return by.x; }
    __device__ __forceinline__ double by1() const { return by.y; }
    __device__ __forceinline__ double ex() const { return __longlong_as_double((long long)em.x); }
};
// Child c's fields: <true> its bundle in one burst (fetched while the child
// before it is evaluated); at(): in place, for the rare kinds' loop.
template <bool BURST> struct RecChild;
template <> struct RecChild<false> {
    const QRec *nd;
    int c;
    __device__ __forceinline__ void fetch(const QRec *rec, int cc) { nd = rec; c = cc; }
    __device__ __forceinline__ double ccx() const { return nd->ccx[c]; }
    __device__ __forceinline__ double ccy() const { return nd->ccy[c]; }
    __device__ __forceinline__ double cb() const { return nd->cb[c]; }
    __device__ __forceinline__ double ca() const { return nd->ca[c]; }
    __device__ __forceinline__ int32_t ccnt() const { return nd->ccnt[c]; }
    __device__ __forceinline__ int32_t cref() const { return nd->cref[c]; }
};
// (in place in either layout: the rare kinds' loop)
template <bool BURST> struct RecChildAt {
    const QRec *nd;
    int c;
    __device__ __forceinline__ const QRecB *b() const { return reinterpret_cast<const QRecB *>(nd); }
    __device__ __forceinline__ double ccx() const { return BURST ? b()->ch[c].ccx : nd->ccx[c]; }
    __device__ __forceinline__ double ccy() const { return BURST ? b()->ch[c].ccy : nd->ccy[c]; }
    __device__ __forceinline__ int32_t ccnt() const { return BURST ? b()->ccnt[c] : nd->ccnt[c]; }
    __device__ __forceinline__ int32_t cref() const { return BURST ? b()->cref[c] : nd->cref[c]; }
};
template <> struct RecChild<true> {
    f64x2_t p, ba;
    int32_t n, rf;
    __device__ __forceinline__ void fetch(const QRec *rec, int cc) {
        const QRecB *b = reinterpret_cast<const QRecB *>(rec);
        p = lds_fetch<f64x2_t>(&b->ch[cc].ccx);
        ba = lds_fetch<f64x2_t>(&b->ch[cc].cb);
        n = lds_fetch<int32_t>(&b->ccnt[cc]);
        rf = lds_fetch<int32_t>(&b->cref[cc]);
    }
    __device__ __forceinline__ double ccx() const { return p.x; }
    __device__ __forceinline__ double ccy() const { return p.y; }
    __device__ __forceinline__ double cb() const { return ba.x; }
    __device__ __forceinline__ double ca() const { return ba.y; }
    __device__ __forceinline__ int32_t ccnt() const { return n; }
    __device__ __forceinline__ int32_t cref() const { return rf; }
};

// The half width of cell child `cref` of record `ref` (flags stripped), for
// the exact-quotient band (QACC_BAND): a real node's own h, or for the
// virtual chain top of a duplicate group (cref >= virt) half its parent's
// (build_qrec_reg).  A virtual record's only child is a real node.
__device__ __forceinline__ double qrec_child_h(const BHNode *__restrict__ nodes, int32_t ref, int32_t cref,
                                               int32_t virt) {
    return cref < virt ? nodes[cref].h : 0.5 * nodes[ref & ~REF_FORCED].h;
}

// The reference's summarise decision for a cell child from D1 = 1 + D (see
// QACC_BAND): the two record bounds, the exact IEEE quotient in between.
__device__ __forceinline__ bool qrec_accept(const QRec &nd, int c, double D1, double dx, double dy, double theta,
                                            const BHNode *__restrict__ nodes, int32_t ref, int32_t virt) {
    if (D1 > nd.ca[c]) return true;
    if (D1 < nd.cb[c]) return false;
    return qrec_child_h(nodes, ref, nd.cref[c], virt) / __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)) < theta;
}

// All-open / near-exact test of one (query, record) pair (see the comment above
// bh_traverse): the subtree's exact leaf sum replaces its walk.
// (The record carries the box's part of the rounding margin and the bound
// with its 1 + 1e-12 factor folded in: 5 fp64 operations fewer per lane.)
__device__ __forceinline__ bool tile_test(const QRec &nd, double qx, double qy, double qmag) {
    const double cdx = qx - nd.cx, cdy = qy - nd.cy;
    const double dc = cdx * cdx + cdy * cdy;
    bool tile = dc <= nd.rball;   // rball^2 (1 - 1e-9)
    if (!tile) {
        const double ex = __fma_rn(1e-15, qmag, nd.ex);   // 1e-15 (|q| + |box|)
        const double dxm = fmax(fabs(qx - nd.bx0), fabs(qx - nd.bx1)) + ex;
        const double dym = fmax(fabs(qy - nd.by0), fabs(qy - nd.by1)) + ex;
        tile = dxm * dxm + dym * dym <= nd.hmin;   // max(hmin / theta (1 - 1e-12), near_dmax) / (1 + 1e-12), rounded down
    }
    return tile;
}

// The root: a single point, a key-tie group, or a cell tested like any child.
// Lanes with `eval` take its term for their query (qx, qy); returns the lanes
// that open it (the caller pushes the root record) and its record ref.
template <bool STATS>
__device__ __forceinline__ uint64_t root_step(const double2 *__restrict__ pos, const BHNode *__restrict__ nodes,
                                              const QRec *__restrict__ qrec, const int32_t *__restrict__ meta,
                                              int32_t virt, bool eval, double qx, double qy, double theta,
                                              double th_lo, double th_hi, double &fx, double &fy, double &zs,
                                              unsigned long long &nvis, int32_t &rpush, bool own0 = true) {
    const int root = meta[1];
    rpush = root;
    if (root == ~0) {
        if (eval && own0) { if (STATS) ++nvis; const double2 p = pos[0]; leaf_force(qx, qy, p.x, p.y, fx, fy, zs); }
        return 0;
    }
    if (root < 0) return 0;
    const BHNode &rt = nodes[root];
    if (rt.delta >= 62) {
        for (int p = rt.first; p <= rt.last; ++p) {
            const double2 pp = pos[p];
            if (eval && own0) { if (STATS) ++nvis; leaf_force(qx, qy, pp.x, pp.y, fx, fy, zs); }
        }
        return 0;
    }
    // the root cell; with duplicates whose copies the reference root counts
    // differently from the cells below it: its virtual record (h = W, every
    // copy), opened into the real root node
    double rh = rt.h, rcx = rt.cx, rcy = rt.cy;
    int32_t rcnt = rt.cnt;
    if (meta[3]) {
        const QRec &vq = qrec[virt + root];
        rh = ldexp(rt.h, rt.delta >> 1);
        rcx = vq.cx; rcy = vq.cy; rcnt = vq.cnt; rpush = virt + root;
    }
    bool open = false;
    if (eval) {
        if (STATS) ++nvis;
        const double dx = qx - rcx, dy = qy - rcy;
        const double D = __fma_rn(dx, dx, dy * dy);
        if (summarise(rh, D, dx, dy, th_lo, th_hi, theta)) { if (own0) cell_force(dx, dy, D, rcnt, fx, fy, zs); }
        else open = true;
    }
    return __ballot(open);
}

// One narrow wave: part `part` (queries part*NQ .. +NQ-1) of heavy group `grp`
// (heavy slot h).  See "Narrow layout" above.
template <int MODE>
__device__ void narrow_wave(NarrowLDS &L, const double2 *__restrict__ pos, const int32_t *__restrict__ dupc,
                            const BHNode *__restrict__ nodes, const QRec *__restrict__ qrec,
                            const int32_t *__restrict__ meta, const double *__restrict__ unused_mom, bool mom_on,
                            double mom_tol, double theta, int64_t g0, int64_t g1, const int32_t *__restrict__ qlist,
                            int32_t virt, double2 *__restrict__ F, double *__restrict__ Z,
                            unsigned long long *__restrict__ visits, unsigned long long *__restrict__ bcost,
                            const int32_t *__restrict__ cost_lab, int32_t *__restrict__ ttask_n,
                            int32_t *__restrict__ tcost, int32_t *__restrict__ mom_flag, const NarrowView &nv,
                            int64_t h, int part, int w) {
    constexpr bool STATS = MODE == 2, COST = MODE >= 1;
    (void)unused_mom;
    const int lane = lane_id();
    const int c = lane & 3, q = (lane >> 2) & (NQ - 1), k = lane >> (2 + NQ_LOG);
    const int64_t grp = nv.hlist[h];
    const double th_lo = theta * (1.0 - 1e-14), th_hi = theta * (1.0 + 1e-14);
    const int64_t kq = g0 + grp * 64 + part * NQ + q;
    const bool valid = kq < g1;
    const int32_t s = valid ? (qlist ? qlist[kq] : (int32_t)kq) : -1;   // sorted position (< 2^31)
    // (the group's empty tile list and cost are the 64-query kernel's: tile_apply
    // need not wait for this kernel)
    const long long t_start = COST ? clock64() : 0;
    const unsigned long long w_start = STATS ? wall_clock64() : 0;
    double qx = 0.0, qy = 0.0;
    if (valid) { const double2 qq = pos[s]; qx = qq.x; qy = qq.y; }
    double fx = 0.0, fy = 0.0, zs = 0.0;
    unsigned long long nvis = 0;
    int32_t npops = 0, ntilepts = 0, ntask = 0, nwant = 0;
    int sp = 0;
    {
        int32_t rpush;
        const uint64_t om = root_step<STATS>(pos, nodes, qrec, meta, virt, valid && k == 0 && c == 0, qx, qy, theta,
                                             th_lo, th_hi, fx, fy, zs, nvis, rpush);
        const uint32_t qm = narrow_compress(om);
        if (qm) {
            if (lane == 0) { L.sref[w][0] = rpush; L.smask[w][0] = qm; }
            sp = 1;
        }
    }
    while (sp > 0) {
        const int kn = sp > STACK / 2 ? 1 : (sp < NKP ? sp : NKP);
        sp -= kn;
        stage_records(L, w, lane, sp, kn, qrec);
        npops += kn;
        const bool kin = k < kn;
        const int kk = kin ? k : 0;
        const QRec &nd = L.srec[w][kk];
        const uint32_t msk = (uint32_t)nd.lmask;
        bool act = kin && valid && ((msk >> q) & 1u);
        const int nflags = nd.nch;
        bool tile = false;
        if ((nflags & QNCH_TILE) && act) tile = tile_test(nd, qx, qy, fabs(qx) + fabs(qy));
        if (__ballot(tile)) {
            const int a = nd.first, b = nd.last, cnt = nd.cnt;
            // moment path: decided once per (record, query) by its child-0 lane,
            // tasks appended per query in record order (capped at MOM_TASKS)
            const bool mw = tile && c == 0 && cnt >= MOM_MIN_POINTS && moment_ok(nd.bx0, nd.bx1, nd.by0, nd.by1, qx, qy, mom_tol);
            nwant += mw ? 1 : 0;
            const uint64_t U = __ballot(mw && mom_on);
            // same-query lanes of earlier records: the task order within a pass
            const uint64_t qcol = narrow_qcol0() << (4 * q);
            const int before = __popcll(U & qcol & lanemask_lt());
            const bool usem = mw && mom_on && ntask + before < MOM_TASKS;
            if (usem) nv.mtask[(h * 64 + part * NQ + q) * MOM_TASKS + ntask + before] = L.bref[w][kk];
            ntask = min(MOM_TASKS, ntask + (int)__popcll(U & qcol));
            const uint64_t UM = __ballot(usem);
            const bool dense = tile && !((UM >> (lane & ~3)) & 1ull);
            // the range holds whole equal-key runs: the query's duplicates (itself
            // included) add exactly 1 each to z in the leaf sum, taken off here
            if (tile && c == 0 && s >= a && s <= b) zs -= (double)dupc[s];
            if (STATS && tile && c == 0) nvis += (unsigned long long)(b - a + 1);
            // dense: the query's 4 lanes split the subtree's points, summed
            // apart and added once (accumulating into fx / fy / zs inside the
            // divergent loop made the compiler copy them at every merge)
            // (a divergent do-while: lanes leave it one by one, no merge per point)
            double ux = 0.0, uy = 0.0, uq = 0.0;
            if (dense && a + c <= b) {
                int p = a + c;
                do {
                    const double2 pp = pos[p];
                    pair_force(qx, qy, pp.x, pp.y, ux, uy, uq);
                    p += 4;
                } while (p <= b);
            }
            if (dense) { fx += ux; fy += uy; zs += uq; }
            const uint64_t tm = __ballot(tile && c == 0);
            for (uint64_t r = tm; r; r &= r - 1) {   // cost: points per (record, query), as the 64-query layout's
                const int l = __ffsll((long long)r) - 1;
                ntilepts += __shfl(b - a + 1, l, 64);
            }
            act = act && !tile;
        }
        if (__ballot(act) == 0) continue;
        // child c of record k for query q
        const int nch = nflags & 0xff;
        const int kind = (nflags >> (QNCH_KIND + 2 * c)) & 3;
        const bool has = act && c < nch;
        const double dx = qx - nd.ccx[c], dy = qy - nd.ccy[c];
        const double D1 = __fma_rn(dx, dx, __fma_rn(dy, dy, 1.0));   // 1 + D (QACC_BAND)
        const bool isleaf = has && kind == QK_LEAF, iscell = has && kind == QK_CELL;
        bool acc = D1 > nd.ca[c];
        if (iscell && !acc && !(D1 < nd.cb[c]))
            acc = qrec_child_h(nodes, L.bref[w][kk], nd.cref[c], virt) / __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)) <
                  theta;
        const bool takel = isleaf && !(dx == 0.0 && dy == 0.0);
        const bool takec = iscell && acc;
        const double wm = takel ? 1.0 : (takec ? (double)nd.ccnt[c] : 0.0);
        if (STATS && (isleaf || iscell)) ++nvis;
        const double Qv = recip_bh(D1);
        const double mult = wm * Qv;
        const double sc = mult * Qv;
        fx = __fma_rn(sc, dx, fx);
        fy = __fma_rn(sc, dy, fy);
        zs += mult;
        // duplicate kinds (rare)
        const bool dupk = has && (kind == QK_MULTI || kind == QK_TIE);
        if (__builtin_expect(__ballot(dupk) != 0, 0)) {
            if (dupk && kind == QK_MULTI) {   // a leaf of ccnt copies: 0 if it is the query's point
                if (!(nd.ccx[c] == qx && nd.ccy[c] == qy)) {
                    if (STATS) ++nvis;
                    cell_force(dx, dy, __fma_rn(dx, dx, dy * dy), nd.ccnt[c], fx, fy, zs);
                }
            } else if (dupk) {                // a key-tie group: every point directly
                const BHNode &tn = nodes[nd.cref[c]];
                for (int p = tn.first; p <= tn.last; ++p) {
                    const double2 pp = pos[p];
                    if (STATS) ++nvis;
                    leaf_force(qx, qy, pp.x, pp.y, fx, fy, zs);
                }
            }
        }
        // pushes: one entry per (record, child) that some query opens, in lane order
        const uint64_t O = __ballot(iscell && !acc);
        const bool pl = q == 0 && kin;
        const uint32_t m = pl ? narrow_compress(O >> (k * 4 * NQ + c)) : 0u;
        const uint64_t P = __ballot(m != 0u);
        if (m) {
            const int at = sp + (int)__popcll(P & lanemask_lt());
            L.sref[w][at] = nd.cref[c];
            L.smask[w][at] = m;
        }
        sp += (int)__popcll(P);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the pushes landed before the next pop
        __builtin_amdgcn_wave_barrier();
    }
    // the query's NKP x 4 lanes, in a fixed xor butterfly (every lane the same bits)
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
        fx += __shfl_xor(fx, o, 64); fy += __shfl_xor(fy, o, 64); zs += __shfl_xor(zs, o, 64);
    }
#pragma unroll
    for (int o = 4 * NQ; o < 64; o <<= 1) {
        fx += __shfl_xor(fx, o, 64); fy += __shfl_xor(fy, o, 64); zs += __shfl_xor(zs, o, 64);
    }
    if (k == 0 && c == 0 && valid) {
        F[s] = make_double2(fx, fy);
        Z[s] = zs;
    }
    if (k == 0 && c == 0) nv.mtask_n[h * 64 + part * NQ + q] = valid ? ntask : 0;
    const int wwant = wave_sum(nwant);
    if (lane == 0) {
        nv.ncost[h * NPARTS + part] = npops + (ntilepts >> 6);
        if (wwant && __hip_atomic_load(&mom_flag[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mom_flag[2])
            atomicAdd(&mom_flag[1], wwant);
    }
    // this wave's run time into its queries' buckets (multi-GPU balancing); a
    // wave of the last, partial group may hold no query at all: nothing to add
    if (COST && bcost && __ballot(valid)) {
        const unsigned long long cc = ((unsigned long long)(clock64() - t_start) >> 6) + 1;
        if (cost_lab) {
            if (valid && k == 0 && c == 0) atomicAdd(&bcost[cost_lab[s] >> 8], (cc + NQ - 1) / NQ);
        } else {
            const int64_t sf = wave_min(valid ? s : ((int64_t)1 << 62));
            if (lane == 0) atomicAdd(&bcost[sf >> 8], cc);
        }
    }
    if (STATS && visits) {
        const unsigned long long tv = wave_sum(nvis);
        const unsigned long long tn = wave_sum((unsigned long long)(k == 0 && c == 0 && valid ? ntask : 0));
        if (lane == 0) {
            atomicAdd(visits, tv);
            atomicAdd(visits + 3, (unsigned long long)npops);
            atomicAdd(visits + 4, (unsigned long long)ntilepts);
            atomicMax(visits + 8, (unsigned long long)npops);
            atomicAdd(visits + 30, 1ull);   // narrow waves run
            atomicAdd(visits + 46, tn);     // their queries' moment tasks (narrow_moment_apply's)
            const unsigned long long w_end = wall_clock64();
            atomicMax(visits + 15, w_end - w_start);
            atomicMax(visits + 16, ~0ull - w_start);
            atomicMax(visits + 17, w_end);
            atomicAdd(visits + 18, w_end - w_start);
            atomicAdd(visits + 37, (unsigned long long)(clock64() - t_start));   // shader cycles (wave_mhz)
            atomicMax(visits + 31, w_end - w_start);   // longest narrow wave
            wave_log_put(nv.wlog, w_start, w_end, 1);
        }
    }
}

// The narrow waves of the heavy groups: 4 per workgroup, idle beyond the
// heavy count.  A kernel of its own (its ~78 VGPRs would cost the 64-query
// layout's 8 waves per SIMD), launched on a second stream beside bh_traverse.
template <int MODE>
#ifdef NARROW_WPE   // A/B builds: the narrow waves' occupancy bound (waves per SIMD)
#define NARROW_ATTR __attribute__((amdgpu_waves_per_eu(NARROW_WPE)))
#else
#define NARROW_ATTR
#endif
__global__ __launch_bounds__(256) NARROW_ATTR void bh_traverse_narrow(
    const double2 *__restrict__ pos, const int32_t *__restrict__ dupc, const BHNode *__restrict__ nodes,
    const QRec *__restrict__ qrec, int32_t *__restrict__ ttask_n, const int32_t *__restrict__ meta,
    int32_t *__restrict__ mom_flag, double mom_tol, double theta, int64_t g0, int64_t g1,
    const int32_t *__restrict__ qlist, int32_t virt, double2 *__restrict__ F, double *__restrict__ Z,
    unsigned long long *__restrict__ visits, unsigned long long *__restrict__ bcost, int32_t *__restrict__ tcost,
    const int32_t *__restrict__ cost_lab, NarrowView nv) {
    __shared__ NarrowLDS L;
    const int w = threadIdx.x >> 6;
    const int64_t slot = (int64_t)blockIdx.x * 4 + w;   // heavy slot x part
    const int64_t h = slot / NPARTS;
    if (h >= (int64_t)*nv.hcount) return;
    narrow_wave<MODE>(L, pos, dupc, nodes, qrec, meta, nullptr, mom_flag[0] != 0, mom_tol, theta, g0, g1, qlist, virt,
                      F, Z, visits, bcost, cost_lab, ttask_n, tcost, mom_flag, nv, h, (int)(slot % NPARTS), w);
}

// ---- Spill: splitting long walks over the chip (Options::spill; round 6).
// A walk -- a wave's own 64-query group, or a task -- that has popped its
// budget of records stops at the next batch boundary and hands its LDS stack
// (the rest of the walk: (cell record, lane mask) entries) to the task list of
// the next level, cut into tasks of consecutive entries (1, 1, 2, 4, 8, 16, 16,
// ... from the bottom of the stack, whose entries are the largest subtrees).
// Level l's tasks are taken by the l-th drain launch after the traversal: one
// atomic add per claim on the level's head, no waiting (the list is complete
// when the launch starts, as its producers ran in the previous launch); the
// task's entries become the wave's stack, the walk is the same loop -- the
// reference's opened / summarised cells (QuadTree.scala:123-152: a cell's
// decision depends on the query and the cell only, not on who walks it) --
// and splits again into level l + 1 (the last level never splits).  The split
// points depend on the pop counts of the walks alone (the tree and the
// queries), not on timing; the tasks' sums go to per-query fixed-point
// accumulators (2^-64 units in two carry-free words, fxp_add), whose integer
// adds are associative, so the result does not depend on which wave took which
// task.
// Tiles a task records go to 64-tile pages (tile_apply<true>), added the same
// way.  The heavy waves of the mid phase are one LDS stack walked serially
// (DESIGN 5, 6): this spreads their walks over the chip.
constexpr int SP_LMAX = 4;     // task levels (drain launches) at most
constexpr int SP_PAGES = 0, SP_B0 = 1, SP_B1 = 2, SP_OVF = 3, SP_TASKS = 4;
__host__ __device__ constexpr int sp_head(int l) { return 8 + 3 * (l - 1); }    // level l's next task to take
__host__ __device__ constexpr int sp_ttail(int l) { return 9 + 3 * (l - 1); }   // level l's tasks
__host__ __device__ constexpr int sp_etail(int l) { return 10 + 3 * (l - 1); }  // level l's stack entries
constexpr int SP_NCTL = 8 + 3 * SP_LMAX;
constexpr int SP_FRAC = 64;    // fixed-point fraction bits: |value| < 2^31, resolution 2^-64
constexpr int SP_PAGE = 64;    // tiles per task tile page
constexpr int SP_CHUNK = 16;   // stack entries per task at most (<= 64: one lane each)
struct SpillView {
    int32_t *ctl = nullptr;               // SP_* / sp_*(l) words
    int4 *task = nullptr;                 // level l's at [(l - 1) cap, l cap): {group, first entry, entries, 0}
    uint4 *ent = nullptr;                 // level l's at [(l - 1) cap, l cap): {ref, 0, mask lo, mask hi}
    int32_t *gflag = nullptr;             // group -> gen when it spilled
    unsigned long long *acc = nullptr;    // sorted position -> fx, fy, z as (lo, hi)
    TileTask *pg_tiles = nullptr;
    int32_t *pg_grp = nullptr, *pg_n = nullptr;
    int32_t cap = 0, pg_cap = 0, gen = 0;
    int32_t lin = 0;    // TASK launches: the level whose tasks they take
    int32_t lout = 0;   // the level a walk past its budget splits into (0: none, the last level)
    int32_t force = 0;  // > 0: both budgets this many pops
};

// ---- Tile streaming (option tile_stream, round 6)
// The 64-query traversal's tail -- its last, heavy waves finishing one by one
// -- leaves wave slots idle, while tile_apply's work waits for the whole grid.
// With streaming, a traversal wave whose list is short enough (st_streamed:
// tile cost <= maxcost, so the slot path would not chunk it) hands it over
// when it ends: its list stored, an agent-scope release, then the item
// gen << 32 | wave at items[tail++].  tile_apply<2>, a persistent grid of
// tile_stream workgroups per CU on a stream of its own, dispatched once every
// traversal block has started (hipStreamWaitValue32 on ST_STARTED, which the
// blocks count; tile_stream_gate 0: at once), takes items in order (head++);
// it waits a bounded while for a claimed item to appear and otherwise leaves.
// A list goes to whichever path claims its wave first (claims[wave]: gen << 2
// | 1 the slot path, | 2 a consumer; compare-and-swap), so a list published
// after the consumers left is summed by the slot path.  A consumer sums a list
// as the slot path does a one-chunk wave -- D (the dense terms, the same
// loops) into per-item partials and the moment list -- and stream_finish,
// after the traversal's launch and the consumers, adds M (the moment terms in
// list order, from 0) and then F += D + M, as moment_apply and chunk_combine
// would: the same bits, whichever path took a list and when.  Handed-over
// words are read through the vector path after the acquire (it does not
// invalidate the scalar cache).  Nothing waits on a later launch, so no
// consumer can hold resources another stream's kernel needs to finish.
constexpr int ST_STARTED = 0, ST_TAIL = 1, ST_HEAD = 2, ST_CUM = 9, ST_W = 10;
constexpr int ST_RESET = 8;     // words [0, 8) zeroed after every call (ST_CUM accumulates;
                                // ST_W: the streaming threshold the last tile plan set)
constexpr int ST_Q0 = 16;       // the claims (one word per wave slot) from word 16 on, then the items (8 B each)

#ifndef TSNE_ST_TRAV
#define TSNE_ST_TRAV 1   // 0: the traversal's hand-over hooks compiled out (A/B of their cost only)
#endif
struct StreamView {
    int32_t *ctl = nullptr;             // ST_* words, then the claims, then the items
    int32_t gen = 0;                    // this call's generation (never 0)
    int32_t maxcost = 0;                // > 0: streamed when the tile cost (points + 16 per task) <= maxcost;
                                        // 0: <= ctl[ST_W] (the previous plan's chunk unit x tile_stream_frac)
    int32_t cap = 0;                    // wave slots the claims and items have room for
    int32_t total = 0;                  // traversal wave slots of this call (blocks x TRAV_WPB)
    int32_t prio = 0;                   // the 64-query traversal waves' issue priority (s_setprio; option trav_prio)
    int32_t wait = 48;                  // polls (s_sleep 16 each, ~0.4 us) a consumer waits for a claimed item
    unsigned long long *wlog = nullptr; // the wave timeline (tile_apply's waves; see NarrowView::wlog)
    const int32_t *border = nullptr;    // the 64-query traversal's workgroup order (trav_front), or identity
};
__device__ __forceinline__ int32_t *st_claims(int32_t *ctl) { return ctl + ST_Q0; }
__device__ __forceinline__ unsigned long long *st_items(int32_t *ctl, int32_t cap) {
    return reinterpret_cast<unsigned long long *>(ctl + ST_Q0 + ((cap + 1) & ~1));
}
// A wave's claim word: gen << 2 when its list was handed over this call,
// | 1 once the slot path, | 2 once a consumer took it.  Claim for `who`: the
// owner (`who` itself for a list that was not handed over: the slot path's).
__device__ __forceinline__ int32_t st_claim(int32_t *claims, int64_t w, int32_t gen, int32_t who) {
    int32_t v = __hip_atomic_load(&claims[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        if ((v >> 2) != gen) return who;
        if (v & 3) return v & 3;
        if (__hip_atomic_compare_exchange_strong(&claims[w], &v, (gen << 2) | who, __ATOMIC_RELAXED,
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return who;
    }
}

// A load through the vector path: handed-over bytes read after the acquire
// must not come from the scalar cache, which the acquire does not invalidate
// (a wave-uniform address would otherwise make it an s_load).
template <class T> __device__ __forceinline__ T vec_load(const T *p) {
    asm volatile("" : "+v"(p));
    return *p;
}

// a += v as fixed point: X = v 2^64 truncated toward zero (|v| < 2^31), kept
// as two words that add without carries, so both atomics are independent
// (no returned value to wait for): a[0] += the low 32 bits of X (unsigned,
// < 2^32 per add), a[1] += X >> 32 (signed).  The value is a[1] 2^-32 +
// a[0] 2^-64, exact as a 128-bit integer; resolution 2^-64 absolute.
__device__ __forceinline__ void fxp_add(unsigned long long *a, double v) {
    if (v == 0.0) return;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    const int ex = (int)((bits >> 52) & 0x7ff);
    const unsigned long long M = (bits & 0xFFFFFFFFFFFFFull) | (ex ? (1ull << 52) : 0ull);
    const int sh = (ex ? ex : 1) - 1075 + SP_FRAC;   // |v| 2^64 = M 2^sh
    unsigned long long lo, hi;                       // |X| = hi 2^32 + lo, lo < 2^32
    if (sh >= 32) { lo = (M << sh) & 0xFFFFFFFFull; hi = M << (sh - 32); }
    else if (sh >= 0) { const unsigned long long m = M << sh; lo = m & 0xFFFFFFFFull; hi = sh ? (M >> (32 - sh)) : (M >> 32); }
    else if (sh > -64) { const unsigned long long m = M >> (-sh); lo = m & 0xFFFFFFFFull; hi = m >> 32; }
    else { lo = 0; hi = 0; }
    if (bits >> 63) {   // X = -|X|: lo' = (2^32 - lo) mod 2^32, hi' = -hi - (lo != 0)
        hi = ~hi + (lo ? 0ull : 1ull);
        lo = (0x100000000ull - lo) & 0xFFFFFFFFull;
    }
    atomicAdd(a, lo);
    atomicAdd(a + 1, hi);
}
__device__ __forceinline__ double fxp_value(unsigned long long lo, unsigned long long hi) {
    return ldexp((double)(long long)hi, 32 - SP_FRAC) + ldexp((double)lo, -SP_FRAC);
}

// task k of a split: its first entry and size (1, 1, 2, 4, 8, 16, 16, ...)
__device__ __forceinline__ int sp_size(int k) { return k < 2 ? 1 : min(1 << (k - 1), SP_CHUNK); }
__device__ __forceinline__ int sp_start(int k) {
    int s = 0;
    for (int j = 0; j < k; ++j) s += sp_size(j);
    return s;
}
__device__ __forceinline__ int sp_ntasks(int n) {
    int k = 0;
    for (int c = 0; c < n; ++k) c += sp_size(k);
    return k;
}

// The next task of level sv.lin (wave-uniform; false when the level's list is
// taken): its group, and its entries pushed onto wave w's stack (sp).
template <class LDS>
__device__ __forceinline__ bool sp_next(const SpillView &sv, LDS &L, int w, int64_t &grp, int &sp) {
    int h = -1;
    if (lane_id() == 0) {
        h = atomicAdd(&sv.ctl[sp_head(sv.lin)], 1);
        if (h >= sv.ctl[sp_ttail(sv.lin)]) h = -1;
    }
    h = __builtin_amdgcn_readfirstlane(h);
    if (h < 0) return false;
    const int4 tk = sv.task[(int64_t)(sv.lin - 1) * sv.cap + h];
    grp = __builtin_amdgcn_readfirstlane(tk.x);
    const int e0 = __builtin_amdgcn_readfirstlane(tk.y), n = __builtin_amdgcn_readfirstlane(tk.z);
    if (lane_id() < n) {
        const uint4 v = sv.ent[(int64_t)(sv.lin - 1) * sv.cap + e0 + lane_id()];
        L.sref[w][lane_id()] = (int32_t)v.x;
        L.smask[w][lane_id()] = ((uint64_t)v.w << 32) | v.z;
    }
    sp = n;
    return true;
}

// Room for n stack entries (and their tasks) in level sv.lout's lists: the
// first entry and the first task (wave-uniform), or e = -1 when the entries
// do not fit (the walk goes on: nothing is lost).  Only the allocation runs
// inside the walk's loop (few registers); sp_write fills the slots after it.
__device__ __forceinline__ int sp_alloc(const SpillView &sv, int n, int &t) {
    int e = -1, tt = 0;
    if (lane_id() == 0) {
        int c = __hip_atomic_load(&sv.ctl[sp_etail(sv.lout)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int tries = 0; tries < 100000; ++tries) {
            if (c + n > sv.cap) break;
            if (__hip_atomic_compare_exchange_strong(&sv.ctl[sp_etail(sv.lout)], &c, c + n, __ATOMIC_RELAXED,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                e = c;
                break;
            }
        }
        if (e < 0) {
            atomicOr(&sv.ctl[SP_OVF], 1);
        } else {   // tasks <= entries <= cap: always room
            const int nt = sp_ntasks(n);
            tt = atomicAdd(&sv.ctl[sp_ttail(sv.lout)], nt);
            atomicAdd(&sv.ctl[SP_TASKS], nt);
        }
    }
    t = __builtin_amdgcn_readfirstlane(tt);
    return __builtin_amdgcn_readfirstlane(e);
}
// Stack entries [0, n) of wave w -> level sv.lout's entries [e, e + n) and
// tasks [t, t + ntasks(n)) of group grp (read by the next launch).
template <class LDS>
__device__ __forceinline__ void sp_write(const SpillView &sv, LDS &L, int w, int e, int t, int n, int32_t grp) {
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the stack's last pushes landed
    __builtin_amdgcn_wave_barrier();
    if (lane_id() == 0) sv.gflag[grp] = sv.gen;
    const int64_t lb = (int64_t)(sv.lout - 1) * sv.cap;
    for (int i = lane_id(); i < n; i += 64) {
        const uint64_t m = L.smask[w][i];
        sv.ent[lb + e + i] = make_uint4((uint32_t)L.sref[w][i], 0u, (uint32_t)m, (uint32_t)(m >> 32));
    }
    const int nt = sp_ntasks(n);
    for (int k = lane_id(); k < nt; k += 64) {
        const int a = sp_start(k);
        sv.task[lb + t + k] = make_int4(grp, e + a, min(sp_size(k), n - a), 0);
    }
}

// Traversal kernel (see the comment above), one 64-query group per wave;
// groups the narrow waves take (nv.nflag) return at once.  MODE 0 plain; 1
// wave run times into the multi-GPU cost buckets; 2 every counter (profiling).
// With spill (sv.mode, never with a tree partition) a walk past its budget
// hands the rest to the task queue; TASK: the drain launches' instantiation,
// whose waves take tasks while the queue has any (see "Spill" above) -- a
// kernel of its own, so that the 64-query walk keeps its registers.
// BURST (option trav_burst): a popped record's fields are read in bursts
// (RecHead, RecChild) instead of one by one; the tree partition's
// instantiations keep the reads in place (their slow path reads QRec's layout).
template <int MODE, bool PART, bool TASK, bool BURST = false>
__global__ __launch_bounds__(64 * TRAV_WPB) __attribute__((amdgpu_waves_per_eu(8))) void bh_traverse(
    const double2 *__restrict__ pos, const int32_t *__restrict__ dupc, const BHNode *__restrict__ nodes,
    const QRec *__restrict__ qrec, TileTask *__restrict__ ttask, int32_t *__restrict__ ttask_n,
    const int32_t *__restrict__ meta, int32_t *__restrict__ mom_flag, double mom_tol, double theta, int64_t g0,
    int64_t g1, const int32_t *__restrict__ qlist, int32_t virt, double2 *__restrict__ F, double *__restrict__ Z,
    unsigned long long *__restrict__ visits, unsigned long long *__restrict__ bcost, int32_t *__restrict__ wcost,
    int32_t *__restrict__ tcost, const int32_t *__restrict__ cost_lab, NarrowView nv, int32_t *__restrict__ plim,
    SpillView sv, StreamView stv) {
    constexpr bool STATS = MODE == 2, COST = MODE >= 1;
    static_assert(!(PART && BURST), "the tree partition's slow path reads QRec's own layout");
    if (!PART && !TASK && stv.prio > 0) {   // issue priority over the waves beside it (option trav_prio)
        if (stv.prio == 1) __builtin_amdgcn_s_setprio(1);
        else if (stv.prio == 2) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(3);
    }
    // tile streaming (see "Tile streaming"): every block counts its start
    if (TSNE_ST_TRAV && !PART && !TASK && stv.ctl && threadIdx.x == 0) atomicAdd(&stv.ctl[ST_STARTED], 1);
    // tree partition: this rank's sorted positions [plo, phi) (plim[2]: stack overflow flag)
    const int32_t plo = PART ? plim[0] : 0, phi = PART ? plim[1] : INT32_MAX;
    __shared__ TravLDS L;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const double th_lo = theta * (1.0 - 1e-14), th_hi = theta * (1.0 + 1e-14);
    // (option trav_front: the previous traversal's heavy workgroups first)
    const int64_t blk = !PART && !TASK && stv.border ? (int64_t)stv.border[blockIdx.x] : (int64_t)blockIdx.x;
    const int64_t wid = blk * TRAV_WPB + w;   // query slots g0 + 64 wid .. + 63, tile list wid
    const bool spill_on = !PART && sv.lout != 0;
    int32_t bud = 0;   // pops after which a walk splits (0: never)
    if (spill_on) bud = sv.force > 0 ? sv.force : sv.ctl[TASK ? SP_B1 : SP_B0];
    // the wave's first item: its own group, or (TASK) a task
    int64_t grp = wid;
    constexpr bool task = TASK;
    int tsp = 0;   // TASK: the task's entries on the stack
    if (TASK) {
        if (!sp_next(sv, L, w, grp, tsp)) return;
    } else {
        if (g0 + wid * 64 >= g1) return;
        if (lane == 0) { ttask_n[wid] = 0; wcost[wid] = 0; tcost[wid] = 0; }
        if (nv.nflag && nv.nflag[wid]) return;   // a heavy group: the narrow waves take it (no tiles here)
    }
    for (;;) {
    // query slot k -> sorted position s (the identity, or this rank's list of
    // its own queries in sorted order: the waves stay Morton-coherent)
    const int64_t k = g0 + grp * 64 + lane;
    const bool valid = k < g1;
    const int64_t s = valid ? (qlist ? (int64_t)qlist[k] : k) : -1;
    const long long t_start = COST ? clock64() : 0;
    const unsigned long long w_start = STATS ? wall_clock64() : 0;
    int32_t npops = 0, ntilepts = 0;   // wave-uniform: this walk's cost for the next selection
    double qx = 0.0, qy = 0.0;
    if (valid) { double2 q = pos[s]; qx = q.x; qy = q.y; }
    const double qmag = fabs(qx) + fabs(qy);
    const int ndup = valid ? dupc[s] : 0;   // exact duplicates of the query (itself included)
    double fx = 0.0, fy = 0.0, zs = 0.0;
    unsigned long long nvis = 0, nevals = 0, wpops = 0, wtile = 0, wslots = 0;   // STATS only
    unsigned long long wtie = 0;                                               // STATS: key-tie points walked
    unsigned long long wfull = 0, wpart = 0;                                   // STATS only
    int sp = 0;
    int ntt = 0;
    // tile sink: a group's own list (TILE_CAP), or a task's current page
    TileTask *const mytt = ttask + wid * TILE_CAP;
    TileTask *tdst = task ? nullptr : mytt;
    int tcap = task ? 0 : TILE_CAP;
    int32_t page = -1;
    if (!task) {
        int32_t rpush;
        const uint64_t om = root_step<STATS>(pos, nodes, qrec, meta, virt, valid, qx, qy, theta, th_lo, th_hi, fx, fy,
                                             zs, nvis, rpush, plo <= 0 && phi > 0);
        if (om) {
            if (lane == 0) { L.sref[w][0] = rpush; L.smask[w][0] = om; }
            sp = 1;
        }
    } else {
        sp = tsp;   // (sp_next staged its entries)
    }
    // Pop up to 4 cells at a time (one while the stack is over half full: the
    // depth stays bounded): their records are fetched with one round of
    // coalesced 16-byte vector loads, then processed one by one from LDS
    // broadcasts.  (A software pipeline -- the next batch's records in flight
    // in registers while one is processed -- measured no gain: C3 loop 5.645
    // vs 5.643 s, BH snapshots within noise; removed.)
    int spe = -1, spt = 0;   // past the budget: where the rest of the walk goes (entries, tasks)
    int32_t wbud = bud;
    while (sp > 0) {
        if (!PART && wbud > 0 && npops >= wbud && sp >= 2) {
            spe = sp_alloc(sv, sp, spt);
            if (spe >= 0) break;
            wbud = 0;   // no room: walk on
        }
        const int kb = sp > STACK / 2 ? 1 : (sp < 4 ? sp : 4);
        sp -= kb;
        stage_records<TravLDS, BURST>(L, w, lane, sp, kb, qrec);
        const QRec *brec = L.srec[w];
        const int32_t *bref_c = L.bref[w];
        npops += kb;
        for (int r = 0; r < kb; ++r) {
            if (STATS) ++wpops;
            // the record's head fields; BURST: with child 0's, in one burst
            RecHead<BURST> hd;
            RecChild<BURST> chs[4];   // (one per unrolled child slot: registers, no copies)
            hd.fetch(brec + r, bref_c + r);
            if (BURST) {
                chs[0].fetch(brec + r, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            const int ref = __builtin_amdgcn_readfirstlane(hd.ref());
            const uint64_t msk = hd.lmask();
            const uint64_t msk_s = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(msk >> 32)) << 32) |
                                   (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)msk);   // the wave's (scalar)
            bool act = __builtin_amdgcn_inverse_ballot_w64(msk_s);   // the mask's own SGPRs: no VALU
            const QRec &nd = brec[r];
            if (PART) {   // a shared or forced record: the tree partition's slow path (see REF_FORCED)
                const int rf = __builtin_amdgcn_readfirstlane(nd.first), rl = __builtin_amdgcn_readfirstlane(nd.last);
                const bool forced = (ref & REF_FORCED) != 0, mine_rec = rf >= plo && rl < phi;
                if (forced || !mine_rec) {
                    auto push = [&](int32_t pref, uint64_t pm) {
                        if (sp >= STACK) {   // the cut alignment bounds the depth: never expected
                            if (lane == 0) plim[2] = 1;
                            return;
                        }
                        if (lane == 0) { L.sref[w][sp] = pref; L.smask[w][sp] = pm; }
                        ++sp;
                    };
                    const int rref = ref & ~REF_FORCED;
                    const int nflags = __builtin_amdgcn_readfirstlane(nd.nch);
                    bool fm = forced && act, an = !forced && act;
                    if (forced && mine_rec && ntt < TILE_CAP) {   // exact sum over a subtree of mine: one tile
                        const uint64_t tm = __ballot(fm);
                        if (lane == 0) {
                            TileTask tt; tt.ref = rref; tt.first = rf; tt.last = rl; tt.pad = nd.cnt; tt.mask = tm;
                            mytt[ntt] = tt;
                        }
                        ++ntt;
                        ntilepts += rl - rf + 1;
                        if (STATS) wtile += (unsigned long long)(rl - rf + 1);
                        if (fm) {
                            if (STATS) nvis += (unsigned long long)(rl - rf + 1);
                            if (s >= rf && s <= rl) zs -= (double)ndup;
                        }
                        continue;
                    }
                    if (!forced && (nflags & QNCH_TILE) && an && tile_test(nd, qx, qy, qmag)) { fm = true; an = false; }
                    if (__ballot(an || fm) == 0) continue;
                    const int nch = nflags & 0xff;
                    for (int c = 0; c < nch; ++c) {
                        const int kind = (nflags >> (QNCH_KIND + 2 * c)) & 3;
                        const int32_t cref = __builtin_amdgcn_readfirstlane(nd.cref[c]);
                        int32_t c0, c1;   // the child's sorted range
                        if (kind == QK_LEAF) {
                            c0 = c1 = ~cref;
                        } else {
                            const BHNode &cn = nodes[cref >= virt ? cref - virt : cref];
                            c0 = __builtin_amdgcn_readfirstlane(cn.first);
                            c1 = __builtin_amdgcn_readfirstlane(cn.last);
                        }
                        if (c1 < plo || c0 >= phi) continue;         // no point of mine below
                        const bool own = c0 >= plo && c0 < phi;      // the term's owner: its first point's rank
                        const double dx = qx - nd.ccx[c], dy = qy - nd.ccy[c];
                        const double D1 = __fma_rn(dx, dx, __fma_rn(dy, dy, 1.0));   // 1 + D (QACC_BAND)
                        if (kind == QK_LEAF || kind == QK_CELL) {
                            bool take, acc = false;
                            if (kind == QK_LEAF) {
                                take = own && (an || fm) && !(dx == 0.0 && dy == 0.0);
                            } else {
                                if (an) acc = qrec_accept(nd, c, D1, dx, dy, theta, nodes, rref, virt);
                                take = own && an && acc;
                                const uint64_t om = __ballot(an && !acc), fmm = __ballot(fm);
                                if (om) push(cref, om);
                                if (fmm) push(cref | REF_FORCED, fmm);
                            }
                            if (STATS && (an || fm)) ++nvis;
                            const double wm = take ? (kind == QK_LEAF ? 1.0 : (double)nd.ccnt[c]) : 0.0;
                            const double Q = recip_bh(D1);
                            const double mult = wm * Q;
                            const double sc = mult * Q;
                            fx = __fma_rn(sc, dx, fx);
                            fy = __fma_rn(sc, dy, fy);
                            zs += mult;
                        } else if (kind == QK_MULTI) {   // a leaf of ccnt copies: 0 if it is the query's point
                            if (own && (an || fm) && !(nd.ccx[c] == qx && nd.ccy[c] == qy)) {
                                if (STATS) ++nvis;
                                cell_force(dx, dy, __fma_rn(dx, dx, dy * dy), nd.ccnt[c], fx, fy, zs);
                            }
                        } else if (own) {                // a key-tie group: every point directly
                            for (int p = c0; p <= c1; ++p) {
                                const double2 pp = pos[p];
                                if (an || fm) { if (STATS) ++nvis; leaf_force(qx, qy, pp.x, pp.y, fx, fy, zs); }
                            }
                        }
                    }
                    continue;
                }
            }
            // all-open / near-exact tests (per lane) -> the subtree's exact leaf sum;
            // both tests on every lane, their masks straight from the compares
            // (tile_test's branch and a ballot of the combined bool cost more).
            // Lane state is kept as scalar masks (amask: lanes that go on to the
            // children), turned into lane predicates by inverse ballots, which
            // read the mask's SGPRs directly: no VALU per conversion.
            uint64_t tm = 0;
            uint64_t amask = msk_s;
            const int nflags = __builtin_amdgcn_readfirstlane(hd.nch());   // the record is the wave's
            if (nflags & QNCH_TILE) {
                const double cdx = qx - hd.cx(), cdy = qy - hd.cy();
                const double ex = __fma_rn(1e-15, qmag, hd.ex());
                const double dxm = fmax(fabs(qx - hd.bx0()), fabs(qx - hd.bx1())) + ex;
                const double dym = fmax(fabs(qy - hd.by0()), fabs(qy - hd.by1())) + ex;
                // (FMA forms: the bounds carry 1e-9 / 1.1e-12 relative margins)
                tm = msk_s & (__builtin_amdgcn_ballot_w64(__fma_rn(cdx, cdx, cdy * cdy) <= hd.rball()) |
                              __builtin_amdgcn_ballot_w64(__fma_rn(dxm, dxm, dym * dym) <= hd.hmin()));
            }
            if (!PART && tm && task && ntt == tcap) {   // a task's tile page is full (or none yet): the next one
                if (page >= 0 && lane == 0) { sv.pg_n[page] = ntt; sv.pg_grp[page] = (int32_t)grp; }
                int p = 0;
                if (lane == 0) p = atomicAdd(&sv.ctl[SP_PAGES], 1);
                p = __builtin_amdgcn_readfirstlane(p);
                ntt = 0;
                if (p < sv.pg_cap) {
                    page = p;
                    tdst = sv.pg_tiles + (int64_t)p * SP_PAGE;
                    tcap = SP_PAGE;
                } else {   // no page left: the lanes keep traversing (the reference's path; flagged)
                    page = -1;
                    tcap = 0;
                    if (lane == 0) atomicOr(&sv.ctl[SP_OVF], 2);
                }
            }
            if (tm && ntt < tcap) {
                // The wave records (subtree, lanes) for tile_apply, or, when its
                // list is full, the lanes keep traversing (the reference's path).
                // The range holds whole equal-key runs, so either all of the
                // query's exact duplicates (itself included) are in it or none
                // is; they add exactly 1 each to z in the leaf sum: taken off here.
                const int a = __builtin_amdgcn_readfirstlane(hd.first()), b = __builtin_amdgcn_readfirstlane(hd.last());
                if (lane == 0) {
                    TileTask tt; tt.ref = ref; tt.first = a; tt.last = b; tt.pad = hd.cnt(); tt.mask = tm;
                    tdst[ntt] = tt;
                }
                ++ntt;
                ntilepts += b - a + 1;
                if (STATS) wtile += (unsigned long long)(b - a + 1);
                if (__builtin_amdgcn_inverse_ballot_w64(tm)) {
                    if (STATS) nvis += (unsigned long long)(b - a + 1);
                    if (s >= a && s <= b) zs -= (double)ndup;
                }
                amask = msk_s & ~tm;
            }
            if (amask == 0) continue;
            act = __builtin_amdgcn_inverse_ballot_w64(amask);
            // the opened cell's quad children, from its record
            const int nch = nflags & 0xff;
            if (STATS) { wslots += (unsigned long long)nch; if (act) nevals += (unsigned long long)nch; }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c >= nch) break;
                const int kind = (nflags >> (QNCH_KIND + 2 * c)) & 3;   // uniform: scalar branches
                // BURST: this child's bundle was fetched while the one before it was
                // evaluated (child 0's with the head); the next slot's goes out now,
                // ahead of this child's arithmetic.  It goes out whether or not the
                // record has a child there (a read inside the record, never used):
                // under `c + 1 < nch` the compiler kept all four bundles live as
                // partly defined values and spilled them (172 bytes of scratch).
                if (BURST) {
                    if (c + 1 < 4) chs[c + 1 < 4 ? c + 1 : 3].fetch(brec + r, c + 1);
                    __builtin_amdgcn_sched_barrier(0);
                } else {
                    chs[c].fetch(brec + r, c);
                }
                const RecChild<BURST> &ch = chs[c];
                if (kind == QK_CELL || kind == QK_LEAF) {
                    // A leaf (cumSize 1, com = the point) always interacts, zero if
                    // it is the query's own point (x - y == 0 iff x == y).  A cell is
                    // summarised when ch / D < theta (QACC_BAND: two compares of
                    // D1 = 1 + D against the record's bounds, the exact quotient only
                    // inside the band; at D = 0 never).  wm = the term's multiplicity
                    // where taken, else 0: a zero term leaves the sums bit-equal.
                    // Only wm is computed per kind (uniform branch), so the
                    // accumulators stay in place.
                    if (STATS && act) ++nvis;
                    const double dx = qx - ch.ccx(), dy = qy - ch.ccy();
                    const double D1 = __fma_rn(dx, dx, __fma_rn(dy, dy, 1.0));   // 1 + D, the term's denominator
                    uint64_t takem;
                    double wm;
                    if (kind == QK_LEAF) {
                        takem = amask & ~(__builtin_amdgcn_ballot_w64(dx == 0.0) & __builtin_amdgcn_ballot_w64(dy == 0.0));
                        wm = __builtin_amdgcn_inverse_ballot_w64(takem) ? 1.0 : 0.0;
                    } else {
                        // the masks straight from the compares (scalar: a
                        // ballot of a combined bool costs two VALU per child)
                        uint64_t accm = __builtin_amdgcn_ballot_w64(D1 > ch.ca());
                        const uint64_t band = amask & ~accm & ~__builtin_amdgcn_ballot_w64(D1 < ch.cb());
                        if (band) {   // rare: inside the band the exact IEEE quotient decides
                            bool acc = false;
                            if (__builtin_amdgcn_inverse_ballot_w64(band))
                                acc = qrec_child_h(nodes, ref, ch.cref(), virt) /
                                          __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)) < theta;
                            accm |= band & __builtin_amdgcn_ballot_w64(acc);
                        }
                        takem = amask & accm;
                        // (BURST: ccnt came with the bundle; a select, no read under the mask)
                        wm = (double)(__builtin_amdgcn_inverse_ballot_w64(takem) ? ch.ccnt() : 0);
                        const uint64_t om = amask & ~accm;
                        if (om) {
                            if (PART && sp >= STACK) {
                                if (lane == 0) plim[2] = 1;
                            } else {
                                if (lane == 0) { L.sref[w][sp] = ch.cref(); L.smask[w][sp] = om; }
                                ++sp;
                            }
                        }
                    }
                    const double Q = recip_bh(D1);
                    const double mult = wm * Q;
                    const double sc = mult * Q;
                    fx = __fma_rn(sc, dx, fx);
                    fy = __fma_rn(sc, dy, fy);
                    zs += mult;
                    if (STATS) {   // children every active lane takes (summarised cell or leaf), full wave or not
                        if (takem == amask) {
                            if (amask == __ballot(valid)) ++wfull; else ++wpart;
                        }
                    }
                }
            }
            // duplicate kinds (rare), after the others: out of the main loop,
            // whose accumulators then stay in place
            if (__builtin_expect((nflags & (0xAA << QNCH_KIND)) != 0, 0)) {
                for (int c = 0; c < nch; ++c) {
                    const int kind = (nflags >> (QNCH_KIND + 2 * c)) & 3;
                    const RecChildAt<BURST> rc{brec + r, c};   // (read in place in either order: rare)
                    if (kind == QK_MULTI) {   // a leaf of ccnt copies: 0 if it is the query's point
                        if (act && !(rc.ccx() == qx && rc.ccy() == qy)) {
                            if (STATS) ++nvis;
                            const double dx = qx - rc.ccx(), dy = qy - rc.ccy();
                            cell_force(dx, dy, __fma_rn(dx, dx, dy * dy), rc.ccnt(), fx, fy, zs);
                        }
                    } else if (kind == QK_TIE) {
                        const BHNode &tn = nodes[__builtin_amdgcn_readfirstlane(rc.cref())];
                        if (STATS) wtie += (unsigned long long)(tn.last - tn.first + 1);
                        for (int p = tn.first; p <= tn.last; ++p) {
                            const double2 pp = pos[p];
                            if (act) { if (STATS) ++nvis; leaf_force(qx, qy, pp.x, pp.y, fx, fy, zs); }
                        }
                    }
                }
            }
        }
    }
    if (!PART && spe >= 0) sp_write(sv, L, w, spe, spt, sp, (int32_t)grp);
    if (!task) {
        if (valid) {
            F[s] = make_double2(fx, fy);
            Z[s] = zs;
        }
        if (lane == 0) {
            ttask_n[wid] = ntt;
            tcost[wid] = ntilepts + 16 * ntt;
            // (an add: the group's tasks add their pops too, possibly before this)
            if (spill_on) atomicAdd(&wcost[wid], npops + (ntilepts >> 6));
            else wcost[wid] = npops + (ntilepts >> 6);
        }
        if (TSNE_ST_TRAV && !PART && stv.ctl && ntt > 0 &&
            ntilepts + 16 * ntt <= (stv.maxcost > 0 ? stv.maxcost : stv.ctl[ST_W])) {
            // hand the list to the streaming consumers: every store of this
            // wave done, its claim word, an agent-scope release, then the item
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0) {
                __hip_atomic_store(st_claims(stv.ctl) + wid, stv.gen << 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const int32_t k = atomicAdd(&stv.ctl[ST_TAIL], 1);
                __hip_atomic_store(st_items(stv.ctl, stv.cap) + k,
                                   ((unsigned long long)(uint32_t)stv.gen << 32) | (unsigned long long)wid,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    } else {
        if (page >= 0 && lane == 0) { sv.pg_n[page] = ntt; sv.pg_grp[page] = (int32_t)grp; }
        if (valid && (fx != 0.0 || fy != 0.0 || zs != 0.0)) {
            unsigned long long *a = sv.acc + 6 * s;
            fxp_add(a, fx);
            fxp_add(a + 2, fy);
            fxp_add(a + 4, zs);
        }
        if (lane == 0) atomicAdd(&wcost[grp], npops + (ntilepts >> 6));
    }
    if (COST && bcost) {   // cost of this walk into its queries' 256-query buckets
        // the walk's own run time (shader clock / 64; the slices only move work
        // between ranks, every query's sums are unchanged)
        const unsigned long long c = ((unsigned long long)(clock64() - t_start) >> 6) + 1;
        if (cost_lab) {   // by label: an equal share into each query's label bucket
            if (valid) atomicAdd(&bcost[cost_lab[s] >> 8], (c + 63) >> 6);
        } else {
            const int64_t sf = wave_min(valid ? s : ((int64_t)1 << 62));
            if (lane == 0) atomicAdd(&bcost[sf >> 8], c);
        }
    }
    if (STATS && visits) {   // [0] reference-equivalent node evaluations, [3] wave-level pops,
                             // [4] wave-level tile points, [5] lane child evaluations, [6] wave
                             // child slots, [7..9] heaviest wave ([1], [2]: tile_apply), [32] tasks run
        const unsigned long long tv = wave_sum(nvis), te = wave_sum(nevals);
        if (lane == 0) {
            atomicAdd(visits, tv);
            atomicAdd(visits + 3, wpops);
            atomicAdd(visits + 4, wtile);
            atomicAdd(visits + 5, te);
            atomicAdd(visits + 6, wslots);
            atomicMax(visits + 7, wpops + wtile / 16);   // heaviest wave (pops + tile points/16)
            atomicMax(visits + 8, wpops);
            atomicMax(visits + 9, wtile);
            atomicAdd(visits + 13, wfull);
            atomicAdd(visits + 14, wpart);
            const unsigned long long w_end = wall_clock64();   // [15] longest wave, [16] ~first start,
            atomicMax(visits + 15, w_end - w_start);            // [17] last end, [18] sum of wave times
            atomicMax(visits + 16, ~0ull - w_start);
            atomicMax(visits + 17, w_end);
            atomicAdd(visits + 18, w_end - w_start);
            if (task) atomicAdd(visits + 32, 1ull);
            atomicAdd(visits + 37, (unsigned long long)(clock64() - t_start));   // shader cycles (wave_mhz)
            if (!TASK) wave_log_put(nv.wlog, w_start, w_end, 0);
            // the slowest wave's own counts (ticks << 24 | count: the max keeps that wave's)
            const unsigned long long tk = min(w_end - w_start, (1ull << 40) - 1) << 24, cm = (1ull << 24) - 1;
            atomicMax(visits + 33, tk | min(wpops, cm));
            atomicMax(visits + 34, tk | min(wtie, cm));
            atomicMax(visits + 35, tk | min(wtile, cm));
            atomicMax(visits + 36, tk | min(wslots, cm));
        }
    }
    // TASK: the next one of the level (never waiting for one to appear)
    if (!TASK || !sp_next(sv, L, w, grp, tsp)) break;
    }
}

// The heavy groups of the next traversal, from this one's costs (one
// workgroup): a group's cost is its wave's (pops + tile points / 64), or for a
// group that ran narrow 2 x its heaviest narrow wave's (hysteresis: the
// narrow waves each walk a part of the 64-query union).  Heavy: cost >= fac x
// the mean over all groups (and >= NARROW_MIN); at most hmax of them, listed
// in group order.  nflag[g] = heavy slot + 1 or 0.
// Fill mode (hfill > 0: too few 64-query waves to occupy the chip, e.g. one
// rank's share of the queries): also the hfill most costly groups, whatever
// the factor -- the threshold is lowered to the cost bucket (4 per doubling,
// plan_bucket) where the count from the top reaches hfill.
constexpr int32_t NARROW_MIN = 32;
__global__ __launch_bounds__(1024) void narrow_select(int32_t *__restrict__ wcost, int64_t waves,
                                                      int32_t *__restrict__ nflag, const int32_t *__restrict__ ncost,
                                                      int32_t *__restrict__ hlist, int32_t *__restrict__ hcount,
                                                      int64_t hmax, double fac, int64_t hfill,
                                                      int32_t *__restrict__ border, double ffac) {
    __shared__ unsigned long long red[16];
    __shared__ int32_t wtot[16];
    __shared__ int32_t hist[PLAN_BUCKETS];
    __shared__ int32_t sbucket;
    __shared__ double sthr;
    const int t = threadIdx.x, lane = lane_id(), w = t >> 6;
    if (t < PLAN_BUCKETS) hist[t] = 0;
    __syncthreads();
    unsigned long long acc = 0;
    for (int64_t g0 = (int64_t)w * 64; g0 < waves; g0 += 1024) {
        const int64_t g = g0 + lane;
        int32_t c = 0;
        if (g < waves) {
            c = wcost[g];
            const int32_t f = nflag[g];
            if (f > 0) {
                int32_t mx = 0;
                for (int p = 0; p < NPARTS; ++p) mx = max(mx, ncost[(int64_t)(f - 1) * NPARTS + p]);
                c = 2 * mx;
                wcost[g] = c;
            }
            acc += (unsigned long long)max(c, 0);
        }
        if (hfill > 0) (void)wave_bucket_add(hist, plan_bucket(c), g < waves);
    }
    acc = wave_sum(acc);
    if (lane == 0) red[w] = acc;
    __syncthreads();
    if (t == 0) {
        unsigned long long total = 0;
        for (int j = 0; j < 16; ++j) total += red[j];
        sthr = fmax((double)NARROW_MIN, fac * (double)total / (double)max<int64_t>(waves, 1));
        // fill mode: buckets >= sbucket hold at most hfill groups
        int64_t run = 0;
        int b = PLAN_BUCKETS;
        if (hfill > 0)
            while (b > 1 && run + hist[b - 1] <= hfill) run += hist[--b];
        sbucket = b;
    }
    __syncthreads();
    const double thr = sthr;
    const int bmin = sbucket;
    int32_t base = 0;
    for (int64_t g0 = 0; g0 < waves; g0 += 1024) {
        const int64_t g = g0 + t;
        bool hv = false;
        if (fac > 0.0 && g < waves) {
            const int32_t c = wcost[g];
            hv = c >= NARROW_MIN && ((double)c >= thr || plan_bucket(c) >= bmin);
        }
        const uint64_t b = __ballot(hv);
        if (lane == 0) wtot[w] = (int32_t)__popcll(b);
        __syncthreads();
        int32_t off = base, tot = 0;
        for (int j = 0; j < 16; ++j) {
            if (j < w) off += wtot[j];
            tot += wtot[j];
        }
        const int32_t slot = off + (int32_t)__popcll(b & lanemask_lt());
        if (g < waves) {
            const bool take = hv && slot < hmax;
            nflag[g] = take ? slot + 1 : 0;
            if (take) hlist[slot] = (int32_t)g;
        }
        base += tot;
        __syncthreads();
    }
    if (t == 0) *hcount = (int32_t)min<int64_t>(base, hmax);
    if (!border) return;
    // The next traversal's block order (option trav_front): the 64-query
    // workgroups whose heaviest wave (narrow groups excluded: they leave at
    // once) cost >= ffac x the mean first, then the rest, each in Morton order
    __syncthreads();
    const int64_t nb = (waves + TRAV_WPB - 1) / TRAV_WPB;
    const double fthr = ffac * (double)sthr / fmax(fac, 1e-300);   // sthr = fac x mean (or NARROW_MIN)
    int32_t pos = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int64_t b0 = 0; b0 < nb; b0 += 1024) {
            const int64_t b = b0 + t;
            bool in = false;
            if (b < nb) {
                int32_t c = 0;
                for (int k = 0; k < TRAV_WPB; ++k) {
                    const int64_t g = b * TRAV_WPB + k;
                    if (g < waves && nflag[g] == 0) c = max(c, wcost[g]);
                }
                const bool heavy = (double)c >= fthr;
                in = pass == 0 ? heavy : !heavy;
            }
            const uint64_t m = __ballot(in);
            if (lane == 0) wtot[w] = (int32_t)__popcll(m);
            __syncthreads();
            int32_t off = pos, tot = 0;
            for (int j = 0; j < 16; ++j) {
                if (j < w) off += wtot[j];
                tot += wtot[j];
            }
            if (in) border[off + (int32_t)__popcll(m & lanemask_lt())] = (int32_t)b;
            pos += tot;
            __syncthreads();
        }
    }
}

// The traversal waves' tiles, in recording order: one wave per traversal
// wave (same 64 queries).  For every (subtree, lanes) task each lane of the
// mask takes the subtree's exact leaf sum either from its moments -- when the
// series' truncation bound holds and moments were built this iteration, the
// lane appends the node to its own moment list, evaluated lane-parallel by
// moment_apply -- or densely: the points staged through LDS 64 at a time (one
// coalesced dwordx4 load per lane, the next chunk prefetched into registers)
// and read back as wave-uniform broadcasts.  Lanes whose bound holds are
// counted for the next iteration's moment gate.
// MODE 1 (PAGE): the spill tasks' tile pages instead (one wave per page, its
// group's 64 queries; moments evaluated in place; sums into the fixed-point
// accumulators, see "Spill").  MODE 2 (STREAM): the streaming consumer (see
// "Tile streaming"): persistent waves taking the handed-over lists, moments
// recorded per consumer lane and evaluated after its tiles, F += D + M.  MODE 0 skips the
// streamed waves' lists (st_streamed: their list length and tile cost).
//
// The packed rounds (Options::tile_pass).  PASS 0: each round of <= 64 staged
// points is swept by iterating the bits of the lane's 64-bit slot mask.
// PASS 1: the lane walks its TILES of the round (the round's tile masks
// transposed, as the lane-wise windows do) as runs of consecutive slots -- an
// increment and a compare inside a run, the mask pop only at its end -- and
// reads the next slot before it sums the current one.  PASS 2: a pass forms
// up to `tpass` consecutive rounds (the same tiles per round, the same
// <= 64-slot boundary), stages their points side by side and lets every lane
// walk its runs through all of them in one divergent loop; a lane folds its
// partial sums into (fx, fy, zs) and clears them each time it crosses from one
// round to the next, so the sums are grouped as by the one-round loops: the
// same bits for every value.  STATS: the counting instantiation (launched with
// `visits`); the other one carries none of the counters.
// Dynamic LDS per wave, for G = max(tpass, 1) rounds a pass (tile_lds_wave):
// G x 64 staged points, G x 64 transposed tile masks (the lane-wise windows'
// tile ranges share their space), G x 64 packed slot ranges, 64 slot marks.
__host__ __device__ constexpr int tile_lds_wave(int G) { return G * (1024 + 512 + 256) + 256; }
// PF (Options::tile_prefetch; MODE 0, PASS 0 only): the lane-wise windows'
// steps with the next step's gathers in flight (see "Lane-wise window").
template <int MODE, int PASS, bool STATS, bool PF = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void tile_apply(
    const double2 *__restrict__ pos, const BHNode *__restrict__ nodes, const TileTask *__restrict__ ttask,
    const int32_t *__restrict__ ttask_n, int64_t g0, int64_t g1, const int32_t *__restrict__ qlist,
    int32_t *__restrict__ mom_flag, double mom_tol, int32_t *__restrict__ mtask, int32_t *__restrict__ mtask_n,
    double2 *__restrict__ F, double *__restrict__ Z, unsigned long long *__restrict__ visits,
    const int32_t *__restrict__ torder, ChunkView cv, const double *__restrict__ mom, SpillView sv,
    StreamView stv, const int32_t *__restrict__ tcost, int tpass) {
    constexpr bool PAGE = MODE == 1, STREAM = MODE == 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char tile_lds[];
    constexpr float LW_COST = 1.0f;   // lane-wise cost per point relative to a sweep slot (gathers, refills;
                                      // 1.6 before the lane-wise loop lost its accumulator copies, round 5)
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int Gp = PASS == 2 ? tpass : 1;   // rounds a pass
    unsigned char *const wlds = tile_lds + w * tile_lds_wave(Gp);
    double2 *const buf = reinterpret_cast<double2 *>(wlds);                          // staged points
    uint64_t *const wmk = reinterpret_cast<uint64_t *>(wlds + Gp * 1024);            // lane -> its tiles of round g
    int2 *const srng = reinterpret_cast<int2 *>(wlds + Gp * 1024);                   // (lane-wise window: tile ranges)
    uint32_t *const rngw = reinterpret_cast<uint32_t *>(wlds + Gp * 1536);           // tile -> first | last << 16 slot
    int *const smark = reinterpret_cast<int *>(wlds + Gp * 1792);
    int64_t wid, qw;
    int tb, nt;
    bool chunked = false;   // (STATS) this wave is one of several chunks of its tile list
    const TileTask *mytt;
    // PAGE: pages blockIdx.x * 4 + w, + 4 gridDim.x, ... (the loop's end below)
    for (int64_t pit = (int64_t)blockIdx.x * 4 + w;; pit += (int64_t)gridDim.x * 4) {
    if (PAGE) {   // page wid of the spill tasks
        wid = pit;
        if (wid >= (int64_t)min(sv.ctl[SP_PAGES], sv.pg_cap)) return;
        qw = sv.pg_grp[wid];
        mytt = sv.pg_tiles + wid * SP_PAGE;
        tb = 0;
        nt = sv.pg_n[wid];
        if (nt == 0) return;
    } else if (STREAM) {   // the next handed-over list (see "Tile streaming")
        int32_t k = 0;
        if (lane == 0) k = atomicAdd(&stv.ctl[ST_HEAD], 1);
        k = __builtin_amdgcn_readfirstlane(k);
        int64_t got = -1;
        if (k < stv.total) {
            for (int poll = 0; poll < stv.wait; ++poll) {
                unsigned long long v = 0;
                if (lane == 0)
                    v = __hip_atomic_load(st_items(stv.ctl, stv.cap) + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t vhi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
                const uint32_t vlo = __builtin_amdgcn_readfirstlane((uint32_t)v);
                if (vhi == (uint32_t)stv.gen) { got = vlo; break; }
                __builtin_amdgcn_s_sleep(16);
            }
        }
        if (got < 0) return;   // nothing more for now: the slot path takes what comes later
        int32_t own = 0;
        if (lane == 0) own = st_claim(st_claims(stv.ctl), got, stv.gen, 2);
        if (__builtin_amdgcn_readfirstlane(own) != 2) continue;   // the slot path has it
        // the producer's release pairs with this acquire: its list, F and Z fresh
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wid = k;   // entries k x 64 + lane of the consumers' partial sums and moment lists
        qw = got;
        mytt = ttask + qw * TILE_CAP;
        tb = 0;
        nt = vec_load(ttask_n + qw);
        if (lane == 0) atomicAdd(&stv.ctl[ST_CUM], 1);
    } else {
        const int64_t blk = torder ? (int64_t)torder[blockIdx.x] : (int64_t)blockIdx.x;
        wid = blk * 4 + w;
        qw = wid;   // chunks: slot wid = chunk c of C of traversal wave qw's tile list
        int ch = 0, C = 1;
        if (cv.slot_w) {
            if (wid >= *cv.nslots) return;
            qw = cv.slot_w[wid];
            const int32_t v = cv.slot_c[wid];
            ch = v & 0xffff;
            C = v >> 16;
            chunked = C > 1;
        }
        if (g0 + qw * 64 >= g1) return;
        mytt = ttask + qw * TILE_CAP;
        // (a list a streaming consumer claimed first: nothing here, zero partials)
        int ntw = ttask_n[qw];
        if (stv.ctl) {
            int32_t own = 0;
            if (lane == 0) own = st_claim(st_claims(stv.ctl), qw, stv.gen, 1);
            if (__builtin_amdgcn_readfirstlane(own) == 2) ntw = 0;
        }
        tb = (int)((int64_t)ntw * ch / C);
        nt = (int)((int64_t)ntw * (ch + 1) / C);
    }
    const int64_t kq = g0 + qw * 64 + lane;
    const bool valid = kq < g1;
    const int64_t s = valid ? (qlist ? (int64_t)qlist[kq] : kq) : -1;
    const int64_t e = STREAM || cv.slot_w ? wid * 64 + lane : s;   // moment list / partial-sum entry
    if (MODE == 0 && nt == tb) {
        if (valid) {
            mtask_n[e] = 0;
            if (cv.slot_w) { cv.Fp[e] = make_double2(0.0, 0.0); cv.Zp[e] = 0.0; }
        }
        return;
    }
    double qx = 0.0, qy = 0.0;
    if (valid) { const double2 q = pos[s]; qx = q.x; qy = q.y; }
    const bool mom_on = mom_flag[0] != 0;
    const unsigned long long w_start = STATS ? wall_clock64() : 0;
    double fx = 0.0, fy = 0.0, zs = 0.0;
    int nwant = 0, ntask = 0;
    unsigned long long ndense = 0;
    unsigned long long wt_tasks = 0, wt_dense_pts = 0, wt_momchk = 0;   // wave-level diagnostics
    // per dense path (lane-wise, packed sweep, query-major, staged sweep): wave
    // steps (pair slots the wave issues) and this lane's useful pairs
    unsigned long long ps_steps[4] = {0, 0, 0, 0}, ps_pairs[4] = {0, 0, 0, 0};
    // (STATS, one round a pass) what passes over G = 2, 4, 8 consecutive packed
    // rounds [0..2] / lane-wise windows [3..5] would cost: the wave maximum of
    // each lane's steps summed over the G of them, a group ending where the
    // wave leaves that path; and the wave's packed rounds
    unsigned long long gsteps[6] = {0, 0, 0, 0, 0, 0};
    int gacc[6] = {0, 0, 0, 0, 0, 0}, gcnt[6] = {0, 0, 0, 0, 0, 0}, nrounds = 0;
    auto group_add = [&](int path, int mine) {   // one more round / window of `path` (1 packed, 0 lane-wise)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = (path ? 0 : 3) + k;
            gacc[i] += mine;
            if (++gcnt[i] == (2 << k)) { gsteps[i] += (unsigned long long)wave_max(gacc[i]); gacc[i] = 0; gcnt[i] = 0; }
        }
    };
    auto group_end = [&](int path) {   // the wave leaves `path`: its open groups end here
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = (path ? 0 : 3) + k;
            if (gcnt[i]) { gsteps[i] += (unsigned long long)wave_max(gacc[i]); gacc[i] = 0; gcnt[i] = 0; }
        }
    };
    int masked_until = tb;   // tiles before this one take the masked sweep
    for (int t = tb; t < nt;) {
        const TileTask tt = STREAM ? vec_load(mytt + t) : mytt[t];
        if (t >= masked_until && tt.last - tt.first + 1 < MOM_MIN_POINTS) {
            // Lane-wise window: the run of <= 64 consecutive small tiles
            // starting at t.  Each lane walks only the points of ITS tiles
            // (its bits of the 64 masks, transposed by 64 ballots), gathering
            // them itself, so a sweep costs the busiest lane's point count
            // instead of every tile point with most lanes masked off (the
            // masks of small tiles hold ~1/4 of the lanes in the mid phase).
            // Per lane the order is fixed (tile order, then point order).
            const int ti = t + lane;
            bool sm = false;
            int a_i = 0, b_i = -1;
            uint64_t m_i = 0;
            if (ti < nt) {
                const TileTask h = mytt[ti];
                if (h.last - h.first + 1 < MOM_MIN_POINTS) { sm = true; a_i = h.first; b_i = h.last; m_i = h.mask; }
            }
            const uint64_t nsm = ~__ballot(sm);
            const int wn = nsm ? __ffsll((long long)nsm) - 1 : 64;   // >= 1: tile t is small
            if (lane >= wn) m_i = 0;
            // 64 x 64 bit transpose (row i = tile t + i's lane mask): six
            // butterfly stages swapping the off-diagonal blocks of halving size
            uint64_t W = m_i;
#pragma unroll
            for (int st = 0; st < 6; ++st) {
                const int j = 32 >> st;
                const uint64_t lo = st == 0 ? 0x00000000FFFFFFFFull : st == 1 ? 0x0000FFFF0000FFFFull
                                  : st == 2 ? 0x00FF00FF00FF00FFull : st == 3 ? 0x0F0F0F0F0F0F0F0Full
                                  : st == 4 ? 0x3333333333333333ull : 0x5555555555555555ull;
                const uint32_t ylo = __shfl_xor((uint32_t)W, j, 64), yhi = __shfl_xor((uint32_t)(W >> 32), j, 64);
                const uint64_t y = ((uint64_t)yhi << 32) | ylo;
                W = (lane & j) ? ((W & ~lo) | ((y & ~lo) >> j)) : ((W & lo) | ((y & lo) << j));
            }
            // W bit i: tile t + i is one of mine.  Lane-wise costs the busiest
            // lane's points, the masked 64-slot sweep every point: take the
            // cheaper (LW_COST: lane-wise cost per point relative to a sweep
            // slot, gathers and refills included), the sweep for the whole window.
            const int cnt_i = b_i - a_i + 1;
            __builtin_amdgcn_wave_barrier();
            srng[lane] = PF ? make_int2(a_i << 4, b_i << 4) : make_int2(a_i, b_i);   // (PF: byte offsets from pos)
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            int cl = 0;
            for (uint64_t wb = W; wb; wb &= wb - 1) {
                const int2 r = srng[__ffsll((long long)wb) - 1];
                cl += r.y - r.x + (PF ? 16 : 1);
            }
            if (PF) cl >>= 4;
            const int cmax = wave_max(cl), ctot = wave_sum(lane < wn ? cnt_i : 0);
            if ((float)cmax * LW_COST >= (float)ctot) {
                masked_until = t + wn;
                goto masked;
            }
            double ux = 0.0, uy = 0.0, uz = 0.0;
            int nmine = 0, nit = 0;
            // a divergent do-while per lane (two points of one tile per step,
            // the second masked at a tile's odd end): the accumulators are
            // updated in place, not copied at the merges of a wave-uniform loop
            if constexpr (PF) {
                // Option tile_prefetch: the same steps, the gathers of a lane's
                // next step in flight while this step's pairs are summed.  p and
                // last are byte offsets from pos (32 bits: n <= 2^27, see
                // tile_apply_launch).  A step's offsets are min(p, last) and
                // min(p + 16, last): never past the tile's last point (so never
                // pos[n]), the last point twice at an odd end (masked by `two`)
                // and for a lane without a next step (never summed).  Every lane
                // issues both loads in every step (pos_issue2: asm, they stay
                // where they are issued) and the steps alternate between two
                // register pairs, so the wait in front of a step's pair terms is
                // vmcnt(2): on the loads the step before (or the prologue) issued.
                if (W) {
                    int i = __ffsll((long long)W) - 1;
                    W &= W - 1;
                    int2 r = srng[i];
                    uint32_t p = (uint32_t)r.x, last = (uint32_t)r.y;
                    auto gather = [&](f64x2_t &x0, f64x2_t &x1) {
                        pos_issue2(pos, min(p, last), min(p + 16u, last), x0, x1);
                    };
                    auto advance = [&]() -> bool {   // to the lane's next step (false: it has none)
                        // (the conditions as wave masks: one compare each, combined by scalar
                        // instructions, and evaluated here, not where the compiler would sink them)
                        p += 32u;
                        const uint64_t pm = __ballot(p > last), sm = pm & __ballot(W != 0);
                        if (__builtin_amdgcn_inverse_ballot_w64(sm)) {
                            i = __builtin_ctzll(W);   // (W != 0 here)
                            W &= W - 1;
                            r = srng[i];
                            p = (uint32_t)r.x; last = (uint32_t)r.y;
                        }
                        return __builtin_amdgcn_inverse_ballot_w64(~pm | sm);
                    };
                    f64x2_t a0, a1, b0 = {0.0, 0.0}, b1 = {0.0, 0.0};
                    gather(a0, a1);
                    for (;;) {
                        const uint64_t two_a = __ballot(p < last);   // (before p and last change, in place)
                        bool more = advance();
                        gather(b0, b1);
                        pos_wait2(a0, a1);
                        __builtin_amdgcn_sched_barrier(0);
                        pair_force(qx, qy, a0.x, a0.y, ux, uy, uz);
                        pair_force_r(__builtin_amdgcn_inverse_ballot_w64(two_a), qx, qy, a1.x, a1.y, ux, uy, uz);
                        if (STATS) { nmine += __builtin_amdgcn_inverse_ballot_w64(two_a) ? 2 : 1; ++nit; }
                        __builtin_amdgcn_sched_barrier(0);
                        if (!more) break;
                        const uint64_t two_b = __ballot(p < last);
                        more = advance();
                        gather(a0, a1);
                        pos_wait2(b0, b1);
                        __builtin_amdgcn_sched_barrier(0);
                        pair_force(qx, qy, b0.x, b0.y, ux, uy, uz);
                        pair_force_r(__builtin_amdgcn_inverse_ballot_w64(two_b), qx, qy, b1.x, b1.y, ux, uy, uz);
                        if (STATS) { nmine += __builtin_amdgcn_inverse_ballot_w64(two_b) ? 2 : 1; ++nit; }
                        __builtin_amdgcn_sched_barrier(0);
                        if (!more) break;
                    }
                    pos_drain(a0, a1, b0, b1);   // the pair nobody sums
                }
            } else
            if (W) {
                int i = __ffsll((long long)W) - 1;
                W &= W - 1;
                int2 r = srng[i];
                int p = r.x, last = r.y;
                bool more;
                do {
                    const bool two = p < last;
                    const double2 p0 = pos[p];
                    const double2 p1 = pos[two ? p + 1 : p];
                    pair_force(qx, qy, p0.x, p0.y, ux, uy, uz);
                    pair_force_m(two, qx, qy, p1.x, p1.y, ux, uy, uz);
                    if (STATS) { nmine += two ? 2 : 1; ++nit; }
                    p += 2;
                    if (p > last && W) {
                        i = __ffsll((long long)W) - 1;
                        W &= W - 1;
                        r = srng[i];
                        p = r.x; last = r.y;
                    }
                    more = p <= last;
                } while (more);
            }
            if (STATS) ps_steps[0] += 2ull * (unsigned long long)wave_max(nit);
            __builtin_amdgcn_wave_barrier();
            fx += ux; fy += uy; zs += uz;
            ndense += (unsigned long long)nmine;
            if (STATS) {
                group_end(1);
                group_add(0, nit);
                ps_pairs[0] += (unsigned long long)nmine;
                wt_tasks += (unsigned long long)wn;
                wt_dense_pts += (unsigned long long)wave_sum(lane < wn ? b_i - a_i + 1 : 0);
            }
            t += wn;
            continue;
        }
    masked:
        if (tt.last - tt.first + 1 < MOM_MIN_POINTS) {
            // Packed round: the run of consecutive small tiles (no moments below
            // MOM_MIN_POINTS) whose points fit 64 slots is staged as one batch of
            // (point, tile lane mask) and swept once, each lane taking the points
            // of its own tiles -- one staging round per <= 64 points instead of
            // one per tile (tiles average ~9 points in the mid phase).
            if (STATS) group_end(0);
            if constexpr (PASS == 0) {
            const int ti = t + lane;
            int c_i = 1 << 20, a_i = 0;
            uint64_t m_i = 0;
            if (ti < nt) {
                const TileTask h = mytt[ti];
                const int c = h.last - h.first + 1;
                if (c < MOM_MIN_POINTS) { c_i = c; a_i = h.first; m_i = h.mask; }
            }
            int S = c_i;   // inclusive prefix of the counts
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(S, o, 64);
                if (lane >= o) S += v;
            }
            const int mtake = __popcll(__ballot(S <= 64));   // >= 1: tile t itself fits
            const int total = __shfl(S, mtake - 1, 64);
            __builtin_amdgcn_wave_barrier();
            smark[lane] = -1;
            __builtin_amdgcn_wave_barrier();
            if (lane < mtake) smark[S - c_i] = lane;
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            int own = smark[lane];   // slot -> tile: running max of the start markers
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(own, o, 64);
                if (lane >= o) own = max(own, v);
            }
            const int st = __shfl(S - c_i, own, 64), fa = __shfl(a_i, own, 64);
            const uint64_t mk = __shfl(m_i, own, 64);
            __builtin_amdgcn_wave_barrier();
            buf[lane] = lane < total ? pos[fa + lane - st] : make_double2(0.0, 0.0);
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0);
            __builtin_amdgcn_wave_barrier();
            double ux = 0.0, uy = 0.0, uz = 0.0;
            int nmine = 0;
            // lane-wise over the staged slots: each lane walks only ITS slots
            // (the round's 64 slot masks transposed), two at a time, so the
            // round costs its busiest lane's slots instead of all of them;
            // a lane's order is still slot order (the same sums as the sweep)
            uint64_t M = lane < total ? mk : 0ull;
#pragma unroll
            for (int st2 = 0; st2 < 6; ++st2) {
                const int j = 32 >> st2;
                const uint64_t lo = st2 == 0 ? 0x00000000FFFFFFFFull : st2 == 1 ? 0x0000FFFF0000FFFFull
                                  : st2 == 2 ? 0x00FF00FF00FF00FFull : st2 == 3 ? 0x0F0F0F0F0F0F0F0Full
                                  : st2 == 4 ? 0x3333333333333333ull : 0x5555555555555555ull;
                const uint32_t ylo = __shfl_xor((uint32_t)M, j, 64), yhi = __shfl_xor((uint32_t)(M >> 32), j, 64);
                const uint64_t y = ((uint64_t)yhi << 32) | ylo;
                M = (lane & j) ? ((M & ~lo) | ((y & ~lo) >> j)) : ((M & lo) | ((y & lo) << j));
            }
            // a divergent do-while per lane, the next slot's point read before
            // the current one is summed: the accumulators are updated in place
            // (a wave-uniform loop with an `if (M)` body made the compiler copy
            // them at every merge -- ~20 moves per two pairs)
            if (M) {
                int j = __ffsll((long long)M) - 1;
                M &= M - 1;
                double2 pp = buf[j];
                bool more;
                do {
                    more = M != 0ull;
                    j = more ? __ffsll((long long)M) - 1 : j;
                    M &= M - 1;
                    const double2 pn = buf[j];
                    pair_force(qx, qy, pp.x, pp.y, ux, uy, uz);
                    if (STATS) ++nmine;
                    pp = pn;
                } while (more);
            }
            if (STATS) ps_steps[1] += (unsigned long long)wave_max(nmine);
            __builtin_amdgcn_wave_barrier();
            fx += ux; fy += uy; zs += uz;
            ndense += (unsigned long long)nmine;
            if (STATS) {
                wt_tasks += (unsigned long long)mtake; wt_dense_pts += (unsigned long long)total;
                ps_pairs[1] += (unsigned long long)nmine;
                group_add(1, nmine);
                ++nrounds;
            }
            t += mtake;
            } else {
            // A pass: up to Gp rounds, each formed as above (the tiles from t on
            // whose points fit 64 slots), while the next tile is small, inside
            // this chunk and before masked_until.  Round g's points go to slots
            // g x 64 .. of the stage; they are loaded one round ahead of their
            // LDS write (and the next round's tile headers before them), so a
            // round's loads fly while the next one is formed.
            int ng = 0, ntile_p = 0, npts_p = 0;
            double2 pend = make_double2(0.0, 0.0);
            // tile t + lane's range and mask, read unconditionally (past the
            // chunk's end: its last tile again, then ignored) so that nothing
            // but the loads themselves stands between their issue and their use
            int hf, hl;
            uint64_t hm;
            { const TileTask &h = mytt[min(t + lane, nt - 1)]; hf = h.first; hl = h.last; hm = h.mask; }
            for (;;) {
                int c_i = hl - hf + 1, a_i = hf;
                uint64_t m_i = hm;
                if (t + lane >= nt || c_i >= MOM_MIN_POINTS) { c_i = 1 << 20; a_i = 0; m_i = 0; }
                if (ng > 0 && __builtin_amdgcn_readfirstlane(c_i) == (1 << 20)) break;   // tile t is not small
                int S = c_i;   // inclusive prefix of the counts
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int v = __shfl_up(S, o, 64);
                    if (lane >= o) S += v;
                }
                const int mtake = __popcll(__ballot(S <= 64));   // >= 1: tile t itself fits
                const int total = __shfl(S, mtake - 1, 64);
                const int tn = t + mtake;
                const bool cont = ng + 1 < Gp && tn < nt && tn < masked_until;
                // the next round's tile headers (read even where the pass ends here)
                { const TileTask &h = mytt[min(tn + lane, nt - 1)]; hf = h.first; hl = h.last; hm = h.mask; }
                __builtin_amdgcn_wave_barrier();
                smark[lane] = -1;
                __builtin_amdgcn_wave_barrier();
                if (lane < mtake) smark[S - c_i] = lane;
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_s_waitcnt(0xc07f);
                __builtin_amdgcn_wave_barrier();
                int own = smark[lane];   // slot -> tile: running max of the start markers
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int v = __shfl_up(own, o, 64);
                    if (lane >= o) own = max(own, v);
                }
                const int st = __shfl(S - c_i, own, 64), fa = __shfl(a_i, own, 64);
                if (ng > 0) buf[(ng - 1) * 64 + lane] = pend;
                pend = pos[fa + (lane < total ? lane - st : 0)];   // (slots >= total: some point, never read)
                // row i = tile t + i's lane mask, transposed: bit i of lane l = tile t + i is one of l's
                uint64_t Wt = lane < mtake ? m_i : 0ull;
#pragma unroll
                for (int st2 = 0; st2 < 6; ++st2) {
                    const int j = 32 >> st2;
                    const uint64_t lo = st2 == 0 ? 0x00000000FFFFFFFFull : st2 == 1 ? 0x0000FFFF0000FFFFull
                                      : st2 == 2 ? 0x00FF00FF00FF00FFull : st2 == 3 ? 0x0F0F0F0F0F0F0F0Full
                                      : st2 == 4 ? 0x3333333333333333ull : 0x5555555555555555ull;
                    const uint32_t ylo = __shfl_xor((uint32_t)Wt, j, 64), yhi = __shfl_xor((uint32_t)(Wt >> 32), j, 64);
                    const uint64_t y = ((uint64_t)yhi << 32) | ylo;
                    Wt = (lane & j) ? ((Wt & ~lo) | ((y & ~lo) >> j)) : ((Wt & lo) | ((y & lo) << j));
                }
                wmk[ng * 64 + lane] = Wt;
                if (lane < mtake)
                    rngw[ng * 64 + lane] = (uint32_t)(ng * 64 + S - c_i) | ((uint32_t)(ng * 64 + S - 1) << 16);
                if (STATS) { ntile_p += mtake; npts_p += total; }
                t = tn;
                ++ng;
                if (!cont) break;
            }
            buf[(ng - 1) * 64 + lane] = pend;
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            double ux = 0.0, uy = 0.0, uz = 0.0;
            int nmine = 0;
            // a divergent do-while per lane over its runs (tile order, then slot
            // order: the one-round loops' order), the next slot read before the
            // current one is summed; the accumulators are updated in place
            int g = 0;
            uint64_t W = wmk[lane];
            if (PASS == 2)
                while (W == 0ull && g + 1 < ng) W = wmk[++g * 64 + lane];   // (rounds without a slot add +0.0: below)
            if (W) {
                uint32_t r = rngw[g * 64 + __ffsll((long long)W) - 1];
                W &= W - 1;
                int p = (int)(r & 0xffffu), last = (int)(r >> 16);
                double2 pp = buf[p];
                bool more;
                do {
                    bool cross = false;
                    more = true;
                    if (p < last) {
                        ++p;
                    } else {
                        if (PASS == 2)
                            while (W == 0ull && g + 1 < ng) { W = wmk[++g * 64 + lane]; cross = true; }
                        if (W) {
                            r = rngw[g * 64 + __ffsll((long long)W) - 1];
                            W &= W - 1;
                            p = (int)(r & 0xffffu); last = (int)(r >> 16);
                        } else {
                            more = false;   // (p stays: the read below is discarded)
                        }
                    }
                    const double2 pn = buf[p];
                    pair_force(qx, qy, pp.x, pp.y, ux, uy, uz);
                    if (STATS) ++nmine;
                    if (PASS == 2 && cross) {   // the old round's boundary: its partial sums folded, as its own loop did
                        fx += ux; fy += uy; zs += uz;
                        ux = 0.0; uy = 0.0; uz = 0.0;
                    }
                    pp = pn;
                } while (more);
            }
            __builtin_amdgcn_wave_barrier();
            // the last round's fold; a lane that left rounds behind without a
            // slot adds their +0.0 here (x + 0.0 = x for every sum these take:
            // none is ever -0.0, being sums that started from +0.0)
            fx += ux; fy += uy; zs += uz;
            if (STATS) {
                ps_steps[1] += (unsigned long long)wave_max(nmine);
                ndense += (unsigned long long)nmine;
                wt_tasks += (unsigned long long)ntile_p; wt_dense_pts += (unsigned long long)npts_p;
                ps_pairs[1] += (unsigned long long)nmine;
                nrounds += ng;
                if (PASS == 1) group_add(1, nmine);
            }
            }
            continue;
        }
        if (STATS) { group_end(0); group_end(1); }
        ++t;
        const int ref = __builtin_amdgcn_readfirstlane(tt.ref);
        const int a = __builtin_amdgcn_readfirstlane(tt.first), b = __builtin_amdgcn_readfirstlane(tt.last);
        const int cnt = __builtin_amdgcn_readfirstlane(tt.pad);
        const bool mine = (tt.mask >> lane) & 1ull;
        bool usem = false;
        if (mine && cnt >= MOM_MIN_POINTS && (PAGE || ntask < MOM_TASKS)) {
            const BHNode &nd = nodes[ref];
            if (moment_ok(nd.bx0, nd.bx1, nd.by0, nd.by1, qx, qy, mom_tol)) {
                ++nwant;
                if (mom_on) {
                    usem = true;
                    if (PAGE) {   // evaluated here (no per-query list for pages)
                        double cx, cy, R;
                        box_centre(nd, cx, cy, R);
                        moment_eval(mom + (int64_t)ref * MOM_K, qx - cx, qy - cy, fx, fy, zs);
                        ++ntask;
                    } else {
                        mtask[e * MOM_TASKS + ntask++] = ref;
                    }
                }
            }
        }
        const bool dense = mine && !usem;
        const uint64_t dm = __ballot(dense);
        const int kq = __popcll(dm), cnt_t = b - a + 1;
        if (STATS) {
            ++wt_tasks;
            if (dm) wt_dense_pts += (unsigned long long)cnt_t;
            if (cnt >= MOM_MIN_POINTS && (tt.mask != 0)) ++wt_momchk;
        }
        if (dm && kq * ((cnt_t + 63) / 64 + 6) < cnt_t) {
            // Few lanes, many points: query-major.  For each dense lane j in
            // turn, all 64 lanes split the tile's points and a butterfly sum
            // (fixed order: deterministic) hands lane j its total -- kq passes
            // of cnt/64 pairs instead of cnt pairs with most lanes masked off.
            uint64_t rem = dm;
            while (rem) {
                const int j = __ffsll((long long)rem) - 1;
                rem &= rem - 1;
                const double qjx = __shfl(qx, j, 64), qjy = __shfl(qy, j, 64);
                double ux = 0.0, uy = 0.0, uz = 0.0;
                int p = a + lane;
                for (; p + 64 <= b; p += 128) {
                    const double2 p0 = pos[p], p1 = pos[p + 64];
                    pair_force(qjx, qjy, p0.x, p0.y, ux, uy, uz);
                    pair_force(qjx, qjy, p1.x, p1.y, ux, uy, uz);
                }
                if (p <= b) {
                    const double2 p0 = pos[p];
                    pair_force(qjx, qjy, p0.x, p0.y, ux, uy, uz);
                }
                ux = wave_sum(ux); uy = wave_sum(uy); uz = wave_sum(uz);
                if (lane == j) { fx += ux; fy += uy; zs += uz; ndense += (unsigned long long)cnt_t; }
                if (STATS) {
                    ps_steps[2] += (unsigned long long)((cnt_t + 63) / 64 + 6);
                    if (lane == j) ps_pairs[2] += (unsigned long long)cnt_t;
                }
            }
        } else if (dm) {
            double2 nxt = make_double2(0.0, 0.0);
            if (a + lane <= b) nxt = pos[a + lane];
            double ux = 0.0, uy = 0.0, uz = 0.0;
            for (int c0 = a; c0 <= b; c0 += 64) {
                const int cn = min(64, b - c0 + 1);
                __builtin_amdgcn_wave_barrier();
                buf[lane] = nxt;
                if (c0 + 64 + lane <= b) nxt = pos[c0 + 64 + lane];
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's LDS writes landed
                __builtin_amdgcn_wave_barrier();
                int j = 0;
                for (; j + 4 <= cn; j += 4) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const double2 pp = buf[j + u];
                        pair_force(qx, qy, pp.x, pp.y, ux, uy, uz);
                    }
                }
                for (; j < cn; ++j) {
                    const double2 pp = buf[j];
                    pair_force(qx, qy, pp.x, pp.y, ux, uy, uz);
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (dense) { fx += ux; fy += uy; zs += uz; ndense += (unsigned long long)(b - a + 1); }
            if (STATS) {
                ps_steps[3] += (unsigned long long)(b - a + 1);
                if (dense) ps_pairs[3] += (unsigned long long)(b - a + 1);
            }
        }
    }
    if (PAGE) {
        if (valid && (fx != 0.0 || fy != 0.0 || zs != 0.0)) {
            unsigned long long *a = sv.acc + 6 * s;
            fxp_add(a, fx);
            fxp_add(a + 2, fy);
            fxp_add(a + 4, zs);
        }
    } else if (valid && (STREAM || cv.slot_w)) {   // STREAM: item entries (stream_finish adds them)
        mtask_n[e] = ntask;
        cv.Fp[e] = make_double2(fx, fy);
        cv.Zp[e] = zs;
    } else if (valid) {
        mtask_n[s] = ntask;
        if (fx != 0.0 || fy != 0.0 || zs != 0.0) {
            const double2 f = F[s];
            F[s] = make_double2(f.x + fx, f.y + fy);
            Z[s] = Z[s] + zs;
        }
    }
    const int wwant = wave_sum(nwant);
    // (only until the gate's threshold is reached: one memory-side atomic
    // per wave on one word would serialise ~n / 64 of them)
    if (lane == 0 && wwant && __hip_atomic_load(&mom_flag[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mom_flag[2])
        atomicAdd(&mom_flag[1], wwant);
    if (STATS) {   // [1] moment evaluations, [2] dense pair terms; [10..12] diagnostics:
                    // tile tasks, wave-level dense points, tasks with a moment check
        const unsigned long long tm = wave_sum((unsigned long long)ntask), td = wave_sum(ndense);
        unsigned long long pp[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) pp[k] = wave_sum(ps_pairs[k]);
        group_end(0); group_end(1);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {   // [24 + 2k] wave steps, [25 + 2k] lane pairs of dense path k
                atomicAdd(visits + 24 + 2 * k, ps_steps[k]);
                atomicAdd(visits + 25 + 2 * k, pp[k]);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {   // [38 + k] packed, [41 + k] lane-wise: passes over 2, 4, 8 (PASS < 2)
                atomicAdd(visits + 38 + k, gsteps[k]);
                atomicAdd(visits + 41 + k, 2ull * gsteps[3 + k]);
            }
            atomicMax(visits + 44, (unsigned long long)nrounds);   // most packed rounds in one wave
            if (chunked) atomicAdd(visits + 45, 1ull);             // waves that are a chunk of a split list
            atomicAdd(visits + 10, wt_tasks);
            atomicAdd(visits + 11, wt_dense_pts);
            atomicAdd(visits + 12, wt_momchk);
            atomicAdd(visits + 1, tm);
            atomicAdd(visits + 2, td);
            const unsigned long long w_end = wall_clock64();   // [19] longest wave, [20] ~first start,
            atomicMax(visits + 19, w_end - w_start);            // [21] last end, [22] sum of wave times
            atomicMax(visits + 20, ~0ull - w_start);
            atomicMax(visits + 21, w_end);
            atomicAdd(visits + 22, w_end - w_start);
            if (MODE == 0) wave_log_put(stv.wlog, w_start, w_end, 2);
        }
    }
    if (MODE == 0) break;
    }
}

// tile_apply<MODE> for Options::tile_pass (0: the slot-bit loops; 1: one round a
// pass; 2, 4, 8: that many -- the pages and the streaming consumers, whose
// lists are short, stay at one) and with or without the counters.
// `prefetch` (Options::tile_prefetch, and the sorted positions within the
// 32-bit byte offsets of that loop: the caller checks n): the lane-wise
// windows' prefetching steps, for the slot path's slot-bit kernels (MODE 0,
// tile_pass 0); the others keep the plain loop.
template <int MODE, class... Args>
static void tile_apply_launch(int tile_pass, bool prefetch, bool stats, dim3 grid, hipStream_t st, Args... args) {
    const int pass = tile_pass == 0 ? 0 : tile_pass == 1 || MODE != 0 ? 1 : 2;
    const int G = pass == 2 ? tile_pass : 1;
    const size_t lds = 4 * (size_t)tile_lds_wave(G);
#define TSNE_TILE_APPLY(P, S, ...) \
    hipLaunchKernelGGL((tile_apply<MODE, P, S, ##__VA_ARGS__>), grid, dim3(256), lds, st, args..., G)
    if constexpr (MODE == 0) {
        if (pass == 0 && prefetch) {
            if (stats) TSNE_TILE_APPLY(0, true, true); else TSNE_TILE_APPLY(0, false, true);
            return;
        }
    }
    if (pass == 0) { if (stats) TSNE_TILE_APPLY(0, true); else TSNE_TILE_APPLY(0, false); }
    else if (pass == 1) { if (stats) TSNE_TILE_APPLY(1, true); else TSNE_TILE_APPLY(1, false); }
    else if constexpr (MODE == 0) { if (stats) TSNE_TILE_APPLY(2, true); else TSNE_TILE_APPLY(2, false); }
#undef TSNE_TILE_APPLY
}

// Tile streaming's last step (see "Tile streaming"), on the consumers' stream
// after them: per handed-over list's query, moment_apply's terms M over its
// moment list, then F += D + M as moment_apply + chunk_combine would for a
// one-chunk wave (Fp = D; Fp += M if any; F += 0 + Fp if nonzero): the same bits.
__global__ __launch_bounds__(256) void stream_finish(const double2 *__restrict__ pos, const BHNode *__restrict__ nodes,
                                                     const double *__restrict__ mom, int32_t *__restrict__ ctl,
                                                     const int32_t *__restrict__ mtask,
                                                     const int32_t *__restrict__ mtask_n, const double2 *__restrict__ Dp,
                                                     const double *__restrict__ Dz, int64_t g0, int64_t g1,
                                                     double2 *__restrict__ F, double *__restrict__ Z, int32_t cap,
                                                     int32_t gen) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t k = i >> 6;
    if (k >= ctl[ST_TAIL]) return;
    const int64_t w = (int64_t)(uint32_t)st_items(ctl, cap)[k];
    if (st_claims(ctl)[w] != ((gen << 2) | 2)) return;   // summed by the slot path
    const int64_t s = g0 + w * 64 + (i & 63);
    if (s >= g1) return;
    double2 d = Dp[i];
    double dz = Dz[i];
    const int nt = mtask_n[i];
    if (nt > 0) {
        const double2 qp = pos[s];
        double fx = 0.0, fy = 0.0, zs = 0.0;
        for (int t = 0; t < nt; ++t) {
            const int node = mtask[i * MOM_TASKS + t];
            double cx, cy, R;
            box_centre(nodes[node], cx, cy, R);
            moment_eval(mom + (int64_t)node * MOM_K, qp.x - cx, qp.y - cy, fx, fy, zs);
        }
        d = make_double2(d.x + fx, d.y + fy);
        dz = dz + zs;
    }
    const double sx = 0.0 + d.x, sy = 0.0 + d.y, sz = 0.0 + dz;
    if (sx != 0.0 || sy != 0.0 || sz != 0.0) {
        const double2 f = F[s];
        F[s] = make_double2(f.x + sx, f.y + sy);
        Z[s] = Z[s] + sz;
    }
}

// F, Z of the queries of every group that spilled += their tasks' fixed-point
// sums (then zeroed); thread 0 also empties the queue for the next traversal.
__global__ void spill_combine(const int32_t *__restrict__ gflag, int32_t gen, unsigned long long *__restrict__ acc,
                              int64_t g0, int64_t g1, const int32_t *__restrict__ qlist, double2 *__restrict__ F,
                              double *__restrict__ Z, int32_t *__restrict__ ctl) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {   // the lists are empty for the next traversal
        ctl[SP_PAGES] = 0;
        for (int l = 1; l <= SP_LMAX; ++l) { ctl[sp_head(l)] = 0; ctl[sp_ttail(l)] = 0; ctl[sp_etail(l)] = 0; }
    }
    const int64_t k = g0 + i;
    if (k >= g1 || gflag[i >> 6] != gen) return;
    const int64_t s = qlist ? (int64_t)qlist[k] : k;
    ulonglong2 *a = reinterpret_cast<ulonglong2 *>(acc + 6 * s);
    const ulonglong2 vx = a[0], vy = a[1], vz = a[2];
    if ((vx.x | vx.y | vy.x | vy.y | vz.x | vz.y) == 0ull) return;
    const double2 f = F[s];
    F[s] = make_double2(f.x + fxp_value(vx.x, vx.y), f.y + fxp_value(vy.x, vy.y));
    Z[s] = Z[s] + fxp_value(vz.x, vz.y);
    const ulonglong2 zero = make_ulonglong2(0ull, 0ull);
    a[0] = zero; a[1] = zero; a[2] = zero;
}

// The next traversal's budgets from this one's costs (one workgroup): the
// mean walk cost per group (pops + tile points / 64, the group's tasks
// included; groups without a cost -- narrow ones before their selection --
// left out), B0 = max(bmin, fac mean), B1 = max(8, ftask B0).
__global__ __launch_bounds__(1024) void spill_budget(const int32_t *__restrict__ wcost, int64_t waves, double fac,
                                                     double ftask, int32_t bmin, int32_t *__restrict__ ctl) {
    __shared__ unsigned long long rs[16], rc[16];
    const int t = threadIdx.x, lane = lane_id(), w = t >> 6;
    unsigned long long sum = 0, cnt = 0;
    for (int64_t g = t; g < waves; g += 1024) {
        const int32_t c = wcost[g];
        if (c > 0) { sum += (unsigned long long)c; ++cnt; }
    }
    sum = wave_sum(sum);
    cnt = wave_sum(cnt);
    if (lane == 0) { rs[w] = sum; rc[w] = cnt; }
    __syncthreads();
    if (t == 0) {
        unsigned long long S = 0, C = 0;
        for (int k = 0; k < 16; ++k) { S += rs[k]; C += rc[k]; }
        const double mean = C ? (double)S / (double)C : 0.0;
        const int32_t b0 = (int32_t)fmin(2e9, fmax((double)bmin, fac * mean));
        ctl[SP_B0] = b0;
        ctl[SP_B1] = (int32_t)fmax(8.0, ftask * (double)b0);
    }
}

// Per query: what the traversal (root tile, z -= the query itself: no
// duplicates in this mode), tile_apply (moment task, or the dense leaf sum)
// and moment_apply write for it -- the moment sums from the root's
// polynomial coefficients (poly_moment_eval).
template <bool STATS>
__global__ __launch_bounds__(256) void root_tile_eval(const double2 *__restrict__ pos, const BHNode *__restrict__ nodes,
                                                      const double *__restrict__ coef, const int32_t *__restrict__ meta,
                                                      int64_t g0, int64_t g1, const int32_t *__restrict__ qlist,
                                                      double2 *__restrict__ F, double *__restrict__ Z,
                                                      unsigned long long *__restrict__ visits, double mom_tol) {
    const int64_t k = g0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = k < g1;
    const int64_t s = valid ? (qlist ? (int64_t)qlist[k] : k) : 0;
    const int m = meta[0];
    const BHNode &rt = nodes[0];
    bool usem = false;
    double fx = 0.0, fy = 0.0, zs = 0.0;
    if (valid) {
        const double2 q = pos[s];
        usem = moment_ok(rt.bx0, rt.bx1, rt.by0, rt.by1, q.x, q.y, mom_tol);
        if (usem) {
            double cx, cy, R;
            box_centre(rt, cx, cy, R);
            poly_moment_eval(coef, q.x - cx, q.y - cy, fx, fy, zs);
            F[s] = make_double2(0.0 + fx, 0.0 + fy);
        } else {   // the exact leaf sum (only if the series bound fails: not expected here)
            for (int p = 0; p < m; ++p) { const double2 pp = pos[p]; pair_force(q.x, q.y, pp.x, pp.y, fx, fy, zs); }
            F[s] = make_double2(fx, fy);
        }
        Z[s] = -1.0 + zs;
    }
    if (STATS && visits) {   // block totals, one set of atomics per block
        __shared__ unsigned long long sv[4][2];
        const unsigned long long nv = __popcll(__ballot(valid)), nu = __popcll(__ballot(usem));
        if (lane_id() == 0) { sv[threadIdx.x >> 6][0] = nv; sv[threadIdx.x >> 6][1] = nu; }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long bv = 0, bu = 0, bw = 0;
            for (int w = 0; w < 4; ++w) { bv += sv[w][0]; bu += sv[w][1]; bw += sv[w][0] ? 1 : 0; }
            if (bv) {
                atomicAdd(visits, bv * (unsigned long long)m);
                atomicAdd(visits + 1, bu);
                atomicAdd(visits + 2, (bv - bu) * (unsigned long long)m);
                atomicAdd(visits + 3, bw);
                atomicAdd(visits + 4, bw * (unsigned long long)m);
            }
        }
    }
}

// Sort keys of a longest-first block order: block b's cost = its heaviest wave.
__global__ void block_cost_keys(const int32_t *__restrict__ cost, int64_t nwaves, int64_t nblocks,
                                int32_t *__restrict__ key, int32_t *__restrict__ val) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblocks) return;
    int32_t c = 0;
    for (int w = 0; w < 4; ++w)
        if (4 * b + w < nwaves) c = max(c, cost[4 * b + w]);
    key[b] = c;
    val[b] = (int32_t)b;
}

// Heavy groups a traversal of `waves` 64-query waves turns narrow to fill the
// chip: narrowing h groups adds (NPARTS - 1) h waves; up to 8 waves per SIMD
// (32 per CU) in all.  0 once the 64-query waves alone fill it (one rank of
// 1M points: 15,625 waves).  Below half of that (one of 8 ranks at C3: 1,953
// waves) every group: there each 64-query wave is one latency-bound chain
// with ~2 waves per SIMD beside it, and the narrow layout cuts the chain
// (W = 8 projection, scripts/loop_projection.py: span 4.83 -> 3.99 s).
int64_t narrow_fill(const tsne_ctx *ctx, int64_t waves) {
    const int64_t cap = 32 * (int64_t)ctx->cu_count;
    if (waves >= cap) return 0;
    return waves < cap / 2 ? waves : (cap - waves) / (NPARTS - 1);
}

}  // namespace

// Longest-first order of nblocks blocks by the per-wave costs -> order.
static void block_order(tsne_ctx *ctx, BHTree &t, const int32_t *cost, int64_t nwaves, int64_t nblocks,
                        int32_t *order) {
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(block_cost_keys, dim3(ceil_div(nblocks, 256)), dim3(256), 0, st, cost, nwaves, nblocks, t.okey,
                       t.oval);
    size_t tb = t.osort_tmp_bytes;
    TSNE_HIP(hipcub::DeviceRadixSort::SortPairsDescending(t.osort_tmp, tb, t.okey, t.okey2, t.oval, order,
                                                          (int)nblocks, 0, 32, st));
}

// The evaluation's buffers, around the build's two pieces (bhtree_build.hip).
// The interleaving fixes the order of the first allocations (so the buffers'
// addresses) and of the work on the stream; nothing else depends on it.
void bh_alloc(tsne_ctx *ctx, BHTree &t, int64_t n, const std::string &pre) {
    Workspace &ws = ctx->ws;
    // (a selection still running on the second stream: done before its arrays
    // are resized or cleared -- bh_alloc_tree ends with a synchronisation)
    bh_select_join(ctx, t);
    bh_alloc_tree(ctx, t, n, pre);
    // tile_apply slots: traversal waves + at most half as many extra chunks (+ margin)
    const int64_t qwaves = ceil_div(n, 64) + 4;
    t.tile_waves = qwaves + qwaves / 2 + 64;
    t.mtask = ws.get<int32_t>(pre + "mtask", (size_t)std::max<int64_t>(n, t.tile_waves * 64) * MOM_TASKS);
    t.mtask_n = ws.get<int32_t>(pre + "mtask_n", std::max<int64_t>(n, t.tile_waves * 64));
    t.ttask = ws.get<TileTask>(pre + "ttask", (size_t)t.tile_waves * TILE_CAP);
    t.ttask_n = ws.get<int32_t>(pre + "ttask_n", t.tile_waves);
    bh_alloc_build_tmp(ctx, t, n, pre);
    const int64_t nb = ceil_div(t.tile_waves, 4);
    t.wcost = ws.get<int32_t>(pre + "wcost", t.tile_waves);
    t.tcost = ws.get<int32_t>(pre + "tcost", t.tile_waves);
    t.okey = ws.get<int32_t>(pre + "okey", nb);
    t.okey2 = ws.get<int32_t>(pre + "okey2", nb);
    t.oval = ws.get<int32_t>(pre + "oval", nb);
    t.border = ws.get<int32_t>(pre + "border", nb);
    t.torder = ws.get<int32_t>(pre + "torder", nb);
    size_t ob = 0;
    TSNE_HIP(hipcub::DeviceRadixSort::SortPairsDescending(nullptr, ob, t.okey, t.okey2, t.oval, t.border, (int)nb, 0,
                                                          32, ctx->stream));
    t.osort_tmp_bytes = ob;
    t.osort_tmp = ws.get<uint8_t>(pre + "osort_tmp", ob);
    t.sel_waves = 0;
    t.ran_narrow = false;
    t.ch_C = ws.get<int32_t>(pre + "ch_C", qwaves + 1);
    t.ch_slot0 = ws.get<int32_t>(pre + "ch_slot0", qwaves + 1);
    t.ch_slot_w = ws.get<int32_t>(pre + "ch_slot_w", t.tile_waves);
    t.ch_slot_c = ws.get<int32_t>(pre + "ch_slot_c", t.tile_waves);
    t.ch_scost = ws.get<int32_t>(pre + "ch_scost", t.tile_waves);
    t.ch_nslots = ws.get<int32_t>(pre + "ch_nslots", 1);
    t.ch_total = ws.get<unsigned long long>(pre + "ch_total", 1);
    t.ch_Fp = ws.get<double2>(pre + "ch_Fp", (size_t)t.tile_waves * 64);
    t.ch_Zp = ws.get<double>(pre + "ch_Zp", (size_t)t.tile_waves * 64);
    size_t cb = 0;
    TSNE_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, cb, t.ch_C, t.ch_slot0, (int)(qwaves + 1), ctx->stream));
    t.ch_scan_bytes = cb;
    t.ch_scan_tmp = ws.get<uint8_t>(pre + "ch_scan_tmp", cb);
    // narrow layout of heavy groups: at most 1/8 of the groups, their moment lists
    t.nar_hmax = std::max<int64_t>({(int64_t)1, ceil_div(qwaves, 8), std::min<int64_t>(qwaves, 16 * (int64_t)ctx->cu_count)});
    t.nflag = ws.get<int32_t>(pre + "nflag", t.tile_waves);
    TSNE_HIP(hipMemsetAsync(t.nflag, 0, sizeof(int32_t) * t.tile_waves, ctx->stream));
    t.hlist = ws.get<int32_t>(pre + "hlist", t.nar_hmax);
    t.hcount = ws.get<int32_t>(pre + "hcount", 1);
    t.hran = ws.get<int32_t>(pre + "hran", 1);
    TSNE_HIP(hipMemsetAsync(t.hcount, 0, sizeof(int32_t), ctx->stream));
    t.ncost = ws.get<int32_t>(pre + "ncost", (size_t)t.nar_hmax * NPARTS);
    t.nmtask = ws.get<int32_t>(pre + "nmtask", (size_t)t.nar_hmax * 64 * MOM_TASKS);
    t.nmtask_n = ws.get<int32_t>(pre + "nmtask_n", (size_t)t.nar_hmax * 64);
    t.pre = pre;
    t.sp_ctl = nullptr;   // spill buffers: on first use (bh_spill_alloc)
    t.pcost_valid = false;   // (trav_front_cur: no previous costs for this size)
    t.order_ready = false;
    t.sp_gen = 0;
    t.sp_waves = 0;
    t.ran_spill = false;
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
}

// The spill buffers (see "Spill"): per level, stack entries and tasks for
// max(16 per query group, 2^18) entries (far more than the budgets produce),
// 64-tile pages for n / 4 + 16384 pages of task tiles, 48 B of accumulators
// per point.
static void bh_spill_alloc(tsne_ctx *ctx, BHTree &t) {
    if (t.sp_ctl) return;
    Workspace &ws = ctx->ws;
    const std::string &pre = t.pre;
    const int64_t n = t.n, qwaves = ceil_div(n, 64) + 4;
    t.sp_cap = (int32_t)std::min<int64_t>(1 << 26, std::max<int64_t>(1 << 18, 16 * qwaves));
    t.sp_pg_cap = (int32_t)std::min<int64_t>(1 << 24, n / 4 + (1 << 14));
    t.sp_ctl = ws.get<int32_t>(pre + "sp_ctl", SP_NCTL);
    t.sp_task = ws.get<int4>(pre + "sp_task", (size_t)SP_LMAX * t.sp_cap);
    t.sp_ent = ws.get<uint4>(pre + "sp_ent", (size_t)SP_LMAX * t.sp_cap);
    t.sp_gflag = ws.get<int32_t>(pre + "sp_gflag", t.tile_waves);
    t.sp_acc = ws.get<unsigned long long>(pre + "sp_acc", 6 * (size_t)n);
    t.sp_pg_tiles = ws.get<TileTask>(pre + "sp_pg_tiles", (size_t)t.sp_pg_cap * SP_PAGE);
    t.sp_pg_grp = ws.get<int32_t>(pre + "sp_pg_grp", t.sp_pg_cap);
    t.sp_pg_n = ws.get<int32_t>(pre + "sp_pg_n", t.sp_pg_cap);
    hipStream_t st = ctx->stream;
    TSNE_HIP(hipMemsetAsync(t.sp_ctl, 0, sizeof(int32_t) * SP_NCTL, st));
    TSNE_HIP(hipMemsetAsync(t.sp_gflag, 0, sizeof(int32_t) * t.tile_waves, st));
    TSNE_HIP(hipMemsetAsync(t.sp_acc, 0, sizeof(unsigned long long) * 6 * n, st));
    t.sp_gen = 0;
}

// Tile streaming: control words, one item and one flag per traversal wave;
// the consumers' stream and events on the context.
static void bh_stream_alloc(tsne_ctx *ctx, BHTree &t) {
    if (!ctx->st_stream) {
        TSNE_HIP(hipStreamCreateWithFlags(&ctx->st_stream, hipStreamNonBlocking));
        for (auto &e : ctx->st_ev) TSNE_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    Workspace &ws = ctx->ws;
    // control words, the claims, the items; kept (with ST_W, the threshold
    // the last plan set) while the tree keeps its size
    const size_t words = ST_Q0 + 3 * (size_t)t.tile_waves + 2;
    int32_t *c = ws.get<int32_t>(t.pre + "st_ctl", words);
    const bool fresh = c != t.st_ctl || t.st_words != words;
    t.st_ctl = c;
    t.st_words = words;
    // per item (<= one per traversal wave slot) and lane: partial sums D and moment lists
    const size_t ent = (size_t)(ceil_div(t.n, 64) + TRAV_WPB) * 64;
    t.st_Dp = ws.get<double2>(t.pre + "st_Dp", ent);
    t.st_Dz = ws.get<double>(t.pre + "st_Dz", ent);
    t.st_mtask_n = ws.get<int32_t>(t.pre + "st_mtask_n", ent);
    t.st_mtask = ws.get<int32_t>(t.pre + "st_mtask", ent * MOM_TASKS);
    if (fresh) {
        TSNE_HIP(hipMemsetAsync(t.st_ctl, 0, sizeof(int32_t) * words, ctx->stream));
        t.st_gen = 0;
    }
}

int64_t bh_stream_counter(tsne_ctx *ctx, BHTree &t) {
    if (!t.st_ctl) return 0;
    int32_t c[ST_Q0];
    TSNE_HIP(hipMemcpyAsync(c, t.st_ctl, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
    return (int64_t)c[ST_CUM];
}

int64_t bh_spill_counter(tsne_ctx *ctx, BHTree &t, bool flags) {
    if (!t.sp_ctl) return 0;
    int32_t c[SP_NCTL];
    TSNE_HIP(hipMemcpyAsync(c, t.sp_ctl, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
    return flags ? (int64_t)c[SP_OVF] : (int64_t)c[SP_TASKS];
}

int64_t bh_narrow_groups(tsne_ctx *ctx, BHTree &t) {
    if (!t.ran_narrow || !t.hran) return 0;
    int32_t h = 0;
    TSNE_HIP(hipMemcpyAsync(&h, t.hran, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
    return h;
}

BHTree &bh_single_tree(tsne_ctx *ctx, int64_t n) {
    if (!ctx->single_tree) ctx->single_tree = new BHTree();
    BHTree &t = *ctx->single_tree;
    if (t.n != n) bh_alloc(ctx, t, n, "bh1.");
    // a single call is a function of its input alone unless the caller asked
    // for the previous call's costs (Options::reuse_costs): without costs the
    // traversal takes the 64-query layout everywhere
    if (!ctx->opts.reuse_costs) { t.sel_waves = 0; t.sp_waves = 0; t.front_waves = 0; }
    return t;
}

void bh_select_join(tsne_ctx *ctx, BHTree &t) {
    if (!t.sel_pending) return;
    t.sel_pending = false;
    TSNE_HIP(hipStreamWaitEvent(ctx->stream, t.sel_ev, 0));
}

// moment_count's workgroup size on the moments' own stream (Options::bh_chain):
// there it is dispatched beside the traversal pair and the attraction, where a
// 1,024-thread workgroup waits for 16 free wave slots on one CU until their
// grids thin out (24 us alone, 0.7 - 3.2 ms measured there)
// (-DMOM_COUNT_CHAIN=1024 for an A/B build)
#ifndef MOM_COUNT_CHAIN
#define MOM_COUNT_CHAIN 256
#endif

void bh_repulsion(tsne_ctx *ctx, BHTree &t, double theta, int64_t s0, int64_t s1,
                  double2 *dF, double *dz, unsigned long long *visits, const int32_t *qlist,
                  unsigned long long *bcost, bool cost_by_label, int32_t *plim) {
    if (s1 <= s0) return;
    hipStream_t st = ctx->stream;
    const double mom_tol = ctx->opts.mom_tol;
    if (t.root_tile) {
        if (visits)
            hipLaunchKernelGGL(root_tile_eval<true>, dim3(ceil_div(s1 - s0, 256)), dim3(256), 0, st, t.root_pos,
                               t.nodes, t.rcoef, t.meta, s0, s1, qlist, dF, dz, visits, mom_tol);
        else
            hipLaunchKernelGGL(root_tile_eval<false>, dim3(ceil_div(s1 - s0, 256)), dim3(256), 0, st, t.root_pos,
                               t.nodes, t.rcoef, t.meta, s0, s1, qlist, dF, dz, visits, mom_tol);
        TSNE_LAUNCH_CHECK();
        return;
    }
    // counters only when asked for: visits need every counter, the multi-GPU
    // cost buckets only the waves' run times
    const int mode = visits ? 2 : (bcost ? 1 : 0);
    // (option trav_burst: the plain and task walks; not the tree partition's)
    const bool burst = ctx->opts.trav_burst != 0;
    auto kern = plim ? (mode == 2 ? bh_traverse<2, true, false> : mode == 1 ? bh_traverse<1, true, false>
                                                                         : bh_traverse<0, true, false>)
                : burst ? (mode == 2 ? bh_traverse<2, false, false, true> : mode == 1 ? bh_traverse<1, false, false, true>
                                                                                   : bh_traverse<0, false, false, true>)
                        : (mode == 2 ? bh_traverse<2, false, false> : mode == 1 ? bh_traverse<1, false, false>
                                                                              : bh_traverse<0, false, false>);
    auto tkern = burst ? (mode == 2 ? bh_traverse<2, false, true, true> : mode == 1 ? bh_traverse<1, false, true, true>
                                                                                 : bh_traverse<0, false, true, true>)
                       : (mode == 2 ? bh_traverse<2, false, true> : mode == 1 ? bh_traverse<1, false, true>
                                                                           : bh_traverse<0, false, true>);
    const int64_t waves = ceil_div(s1 - s0, 64), nblocks = ceil_div(waves, TRAV_WPB);
    TSNE_REQUIRE(waves <= t.tile_waves, "tile task lists sized for fewer queries");
    // heavy groups: selected after the previous traversal of the same query
    // count from its costs (narrow_select at the end of this function, so
    // that nothing delays this traversal's dispatch behind the tree build);
    // none on a tree's first traversal or with Options::narrow = 0
    NarrowView nv;
    unsigned long long *wlog = visits && ctx->opts.wave_log ? ctx->ws.get<unsigned long long>("rep.wavelog", 1 + 2 * WAVE_LOG_CAP)
                                                             : nullptr;
    nv.wlog = wlog;
    const double nfac = ctx->opts.narrow;
    // (not with a tree partition: every rank walks all queries, the 64-query grid fills the chip)
    const bool narrow = nfac > 0.0 && t.sel_waves == waves && !plim;
    if (narrow) {
        nv.hlist = t.hlist; nv.hcount = t.hcount; nv.ncost = t.ncost; nv.mtask = t.nmtask; nv.mtask_n = t.nmtask_n;
        nv.nflag = t.nflag;
        nv.nbn = (int32_t)ceil_div(t.nar_hmax * NPARTS, 4);
    }
    t.ran_narrow = narrow;
    // work splitting of long walks (see "Spill"): budgets from the previous
    // traversal of the same query count (spill_budget), or forced (tests)
    const Options &o = ctx->opts;
    const bool spill = !plim && (o.spill_force > 0 || (o.spill > 0.0 && t.sp_waves == waves));
    SpillView sv;
    if (spill) {
        bh_spill_alloc(ctx, t);
        ++t.sp_gen;
        sv.ctl = t.sp_ctl; sv.task = t.sp_task; sv.ent = t.sp_ent; sv.gflag = t.sp_gflag; sv.acc = t.sp_acc;
        sv.pg_tiles = t.sp_pg_tiles; sv.pg_grp = t.sp_pg_grp; sv.pg_n = t.sp_pg_n;
        sv.cap = t.sp_cap; sv.pg_cap = t.sp_pg_cap; sv.gen = t.sp_gen;
        sv.lin = 0;
        sv.lout = 1;
        sv.force = o.spill_force;
    }
    t.ran_spill = spill;
    // tile streaming (see "Tile streaming"): one rank's own queries only (a
    // rank's list, a tree partition and spill keep the slot path)
    StreamView stv;
    const bool stream = o.tile_stream > 0 && !plim && !spill && !qlist;
    const int cblocks = std::max(1, ctx->cu_count * o.tile_stream);
    if (stream) {
        bh_stream_alloc(ctx, t);
        stv.ctl = t.st_ctl;
        stv.gen = ++t.st_gen;
        if (t.st_gen >= (1 << 29)) t.st_gen = 1;   // (claims hold gen << 2; 0: never claimed)
        stv.gen = t.st_gen;
        stv.maxcost = o.tile_stream_max;
        stv.wait = o.tile_stream_wait;
        stv.total = (int32_t)(nblocks * TRAV_WPB);
        stv.cap = (int32_t)t.tile_waves;
        // ungated, the consumers' stream starts behind everything before the
        // traversal (gated, the traversal's start implies that; and no marker
        // goes between the build and the traversal on this stream, which lets
        // the side stream's attraction reach the CUs first)
        if (!o.tile_stream_gate) {
            TSNE_HIP(hipEventRecord(ctx->st_ev[0], st));
            TSNE_HIP(hipStreamWaitEvent(ctx->st_stream, ctx->st_ev[0], 0));
        }
    }
    t.ran_stream = stream;
    // the moments the build deferred (Options::build_fuse): the streaming
    // consumers read them beside the traversal, so there they go first; else on
    // the second stream behind the narrow waves, enqueued after the traversal
    // (which stays the first launch behind the build), joined before tile_apply
    bool mom_late = false;
    if (t.mom_deferred) {
        t.mom_deferred = false;
        if (stream) bh_moments(t, st);
        else mom_late = true;
    }
    // Options::bh_chain ("Off the chain"): the deferred moments on
    // their own stream, so that they start with the traversal pair instead of
    // behind the narrow waves; the narrow waves' moment sums, the hran copy and
    // narrow_select on the second stream, so that tile_apply .. chunk_combine
    // and the update run behind nothing narrow.  The options whose kernels read
    // the selection or the costs on the main stream keep the order of bh_chain 0.
    const bool chain = o.bh_chain != 0 && o.tile_stream == 0 && o.spill <= 0.0 && o.spill_force == 0 &&
                       !(o.trav_front_cur > 0.0);
    const bool mom_own = mom_late && chain && ctx->mom_stream;
    const hipStream_t mst = mom_own ? ctx->mom_stream : ctx->aux_stream;
    if (mom_late && !narrow) {   // (narrow: its own event below orders the second stream behind the build)
        TSNE_HIP(hipEventRecord(ctx->aux_ev[0], st));
        if (!mom_own) TSNE_HIP(hipStreamWaitEvent(ctx->aux_stream, ctx->aux_ev[0], 0));
    }
    stv.prio = o.trav_prio;   // (also without streaming)
    if (o.trav_front > 0.0 && narrow && t.front_waves == waves) stv.border = t.trav_order;
    if (t.order_ready && narrow && !plim && !qlist && s0 == 0 && waves == ceil_div(t.n, 64)) {
        TSNE_HIP(hipStreamWaitEvent(st, t.ord_ev, 0));   // (done long before: made during the build)
        stv.border = t.trav_order;
    }
    stv.wlog = wlog;
    const int32_t *clab = cost_by_label ? t.idx_sorted : nullptr;
    if (narrow) {   // the narrow waves on the second stream, beside the 64-query grid
        TSNE_HIP(hipEventRecord(ctx->aux_ev[0], st));
        TSNE_HIP(hipStreamWaitEvent(ctx->aux_stream, ctx->aux_ev[0], 0));
        auto nk = mode == 2 ? bh_traverse_narrow<2> : mode == 1 ? bh_traverse_narrow<1> : bh_traverse_narrow<0>;
        hipLaunchKernelGGL(nk, dim3(nv.nbn), dim3(256), 0, ctx->aux_stream, t.pos, t.dupc, t.nodes, t.qrec, t.ttask_n,
                           t.meta, t.mom_flag, mom_tol, theta, s0, s1, qlist, (int32_t)t.n, dF, dz, visits, bcost,
                           t.tcost, clab, nv);
        if (!chain) TSNE_HIP(hipEventRecord(ctx->aux_ev[1], ctx->aux_stream));
    }
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64 * TRAV_WPB), 0, st, t.pos, t.dupc, t.nodes, t.qrec, t.ttask, t.ttask_n,
                       t.meta, t.mom_flag, mom_tol, theta, s0, s1, qlist, (int32_t)t.n, dF, dz, visits, bcost, t.wcost,
                       t.tcost, clab, nv, plim, sv, stv);
    if (mom_late) {
        // (their own stream: behind the build by the event recorded in front of the traversal pair)
        if (mom_own) TSNE_HIP(hipStreamWaitEvent(mst, ctx->aux_ev[0], 0));
        bh_moments(t, mst, mom_own ? MOM_COUNT_CHAIN : 1024);
        if (!t.mom_ev) TSNE_HIP(hipEventCreateWithFlags(&t.mom_ev, hipEventDisableTiming));
        TSNE_HIP(hipEventRecord(t.mom_ev, mst));
    }
    if (chain && narrow) {
        // the narrow waves' moment sums: behind the narrow kernel (this stream)
        // and the moments; they and the 64-query chain (tile_apply, moment_apply,
        // chunk_combine) write disjoint F, Z entries -- a narrow group has no
        // tiles (bh_traverse zeroes its ttask_n / tcost and leaves), so its
        // partial sums are zeros, which chunk_combine does not add
        if (mom_late) TSNE_HIP(hipStreamWaitEvent(ctx->aux_stream, t.mom_ev, 0));
        hipLaunchKernelGGL(narrow_moment_apply, dim3(ceil_div(t.nar_hmax * 64, 256)), dim3(256), 0, ctx->aux_stream, t.pos,
                           t.nodes, t.mom, t.hlist, t.hcount, t.nmtask, t.nmtask_n, s0, s1, qlist, dF, dz);
        TSNE_HIP(hipMemcpyAsync(t.hran, t.hcount, sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->aux_stream));
        TSNE_HIP(hipEventRecord(ctx->aux_ev[1], ctx->aux_stream));
    }
    // (narrow_select on the second stream, below: once bh_traverse has written wcost)
    const bool sel_off = chain && nfac > 0.0 && !plim;
    if (sel_off) TSNE_HIP(hipEventRecord(ctx->aux_ev[2], st));
    if (stream) {   // the consumers beside the traversal, then their moments and sums into F, Z
        // (tile_stream_gate: dispatched once every traversal block has started,
        // so that they take the slots its tail frees, not slots its blocks need)
        if (o.tile_stream_gate)
            TSNE_HIP(hipStreamWaitValue32(ctx->st_stream, t.st_ctl + ST_STARTED, (uint32_t)nblocks,
                                          hipStreamWaitValueGte, 0xffffffffu));
        ChunkView scv;
        scv.Fp = t.st_Dp;
        scv.Zp = t.st_Dz;
        tile_apply_launch<2>(o.tile_pass, false, visits != nullptr, dim3(cblocks), ctx->st_stream, t.pos, t.nodes, t.ttask,
                             t.ttask_n, s0, s1, qlist, t.mom_flag, mom_tol, t.st_mtask, t.st_mtask_n, dF, dz, visits,
                             (const int32_t *)nullptr, scv, t.mom, SpillView(), stv, t.tcost);
        // (F, Z of the traversal itself: read after its launch has ended)
        TSNE_HIP(hipEventRecord(ctx->st_ev[2], st));
        TSNE_HIP(hipStreamWaitEvent(ctx->st_stream, ctx->st_ev[2], 0));
        hipLaunchKernelGGL(stream_finish, dim3(ceil_div((int64_t)stv.total * 64, 256)), dim3(256), 0, ctx->st_stream,
                           t.pos, t.nodes, t.mom, t.st_ctl, t.st_mtask, t.st_mtask_n, t.st_Dp, t.st_Dz, s0, s1,
                           dF, dz, stv.cap, stv.gen);
        // the per-call words zeroed for the next call (after the traversal and the consumers)
        TSNE_HIP(hipMemsetAsync(t.st_ctl, 0, sizeof(int32_t) * ST_RESET, ctx->st_stream));
        TSNE_HIP(hipEventRecord(ctx->st_ev[1], ctx->st_stream));
    }
    // the levels' tasks: drain launch l takes level l (one wave per slot),
    // splitting into level l + 1; the last one without splits
    const int levels = std::min(o.spill_drains, SP_LMAX);
    for (int d = 1; spill && d <= levels; ++d) {
        SpillView dv = sv;
        dv.lin = d;
        dv.lout = d < levels ? d + 1 : 0;
        hipLaunchKernelGGL(tkern, dim3(std::max(1, ctx->cu_count * 32 / TRAV_WPB)), dim3(64 * TRAV_WPB), 0, st, t.pos,
                           t.dupc, t.nodes,
                           t.qrec, t.ttask, t.ttask_n, t.meta, t.mom_flag, mom_tol, theta, s0, s1, qlist, (int32_t)t.n,
                           dF, dz, visits, bcost, t.wcost, t.tcost, clab, nv, plim, dv, StreamView());
    }
    // tile chunks of heavy waves (ChunkView): the single-workgroup plan while
    // the per-wave costs fit its LDS, else the multi-launch plan and block sort
    ChunkView cv;
    const int64_t tslots = std::min<int64_t>(t.tile_waves, waves + waves / 2 + 64);
    const int32_t *torder = t.torder;
    if (waves <= PLAN_WAVES_MAX && ceil_div(tslots, 4) <= PLAN_BLOCKS_MAX) {
        hipLaunchKernelGGL(tile_plan, dim3(1), dim3(1024), 0, st, t.tcost, waves, tslots, t.ch_C, t.ch_slot0,
                           t.ch_slot_w, t.ch_slot_c, t.ch_nslots, t.torder, stream ? t.st_ctl + ST_Q0 : nullptr,
                           stv.gen, stream ? t.st_ctl + ST_W : nullptr, o.tile_stream_frac);
    } else {
        const int64_t wb = ceil_div(waves + 1, 256);
        TSNE_HIP(hipMemsetAsync(t.ch_total, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(chunk_total, dim3(wb), dim3(256), 0, st, t.tcost, waves, t.ch_total);
        hipLaunchKernelGGL(chunk_parts, dim3(wb), dim3(256), 0, st, t.tcost, t.ch_total, waves, t.ch_C,
                           stream ? t.st_ctl + ST_Q0 : nullptr, stv.gen, stream ? t.st_ctl + ST_W : nullptr,
                           o.tile_stream_frac);
        size_t tb = t.ch_scan_bytes;
        TSNE_HIP(hipcub::DeviceScan::ExclusiveSum(t.ch_scan_tmp, tb, t.ch_C, t.ch_slot0, (int)(waves + 1), st));
        hipLaunchKernelGGL(chunk_fill, dim3(wb), dim3(256), 0, st, t.ch_C, t.ch_slot0, t.tcost, waves, t.ch_slot_w,
                           t.ch_slot_c, t.ch_scost, tslots, t.ch_nslots);
        block_order(ctx, t, t.ch_scost, tslots, ceil_div(tslots, 4), t.torder);
    }
    cv.slot_w = t.ch_slot_w; cv.slot_c = t.ch_slot_c; cv.nslots = t.ch_nslots;
    cv.Fp = t.ch_Fp; cv.Zp = t.ch_Zp;
    if (mom_late) TSNE_HIP(hipStreamWaitEvent(st, t.mom_ev, 0));   // t.mom: read from here on
    // (tile_prefetch: its byte offsets from pos, and one step past them, fit 32 bits)
    const bool tile_pf = o.tile_prefetch != 0 && t.n <= ((int64_t)1 << 27);
    tile_apply_launch<0>(o.tile_pass, tile_pf, visits != nullptr, dim3(ceil_div(tslots, 4)), st, t.pos, t.nodes, t.ttask,
                         t.ttask_n, s0, s1, qlist, t.mom_flag, mom_tol, t.mtask, t.mtask_n, dF, dz, visits, torder, cv,
                         t.mom, SpillView(), stv, t.tcost);
    hipLaunchKernelGGL(moment_apply, dim3(ceil_div(tslots * 64, 256)), dim3(256), 0, st, t.pos, t.nodes, t.mom,
                       t.mtask, t.mtask_n, s0, s1, qlist, dF, dz, cv);
    const bool keep_pcost = o.trav_front_cur > 0.0 && !plim && !qlist && s0 == 0 && s1 == t.n;
    if (keep_pcost) {
        t.pcost = ctx->ws.get<int32_t>(t.pre + "pcost", (size_t)t.n);
        t.pred = ctx->ws.get<int32_t>(t.pre + "pred", (size_t)ceil_div(t.n, 64) + 1);
        t.trav_order = ctx->ws.get<int32_t>(t.pre + "trav_order", ceil_div(t.tile_waves, TRAV_WPB) + 1);
    }
    hipLaunchKernelGGL(chunk_combine, dim3(ceil_div(s1 - s0, 256)), dim3(256), 0, st, t.ch_Fp, t.ch_Zp, t.ch_C,
                       t.ch_slot0, s0, s1, qlist, dF, dz, keep_pcost ? t.pcost : nullptr, t.idx_sorted, t.wcost,
                       narrow ? t.nflag : nullptr);
    t.pcost_valid = keep_pcost;
    if (spill) {   // the tasks' tile pages, then their sums into F, Z
        tile_apply_launch<1>(o.tile_pass, false, visits != nullptr, dim3(std::max(1, ctx->cu_count * 4)), st, t.pos, t.nodes,
                             t.ttask, t.ttask_n, s0, s1, qlist, t.mom_flag, mom_tol, t.mtask, t.mtask_n, dF, dz, visits,
                             (const int32_t *)nullptr, ChunkView(), t.mom, sv, StreamView(), t.tcost);
        hipLaunchKernelGGL(spill_combine, dim3(ceil_div(s1 - s0, 256)), dim3(256), 0, st, t.sp_gflag, t.sp_gen,
                           t.sp_acc, s0, s1, qlist, dF, dz, t.sp_ctl);
    }
    // the narrow waves' own queries from here on (their F / Z entries are
    // disjoint from the 64-query waves' above, so the tiles did not wait for them)
    // (bh_chain: their moment sums and the hran copy ran there too, in front of the event)
    if (narrow) {
        TSNE_HIP(hipStreamWaitEvent(st, ctx->aux_ev[1], 0));
        if (!chain) {
            hipLaunchKernelGGL(narrow_moment_apply, dim3(ceil_div(t.nar_hmax * 64, 256)), dim3(256), 0, st, t.pos,
                               t.nodes, t.mom, t.hlist, t.hcount, t.nmtask, t.nmtask_n, s0, s1, qlist, dF, dz);
            TSNE_HIP(hipMemcpyAsync(t.hran, t.hcount, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        }
    }
    // the next traversal's heavy groups (of the same query count) from this one's costs
    // (bh_chain: on the second stream -- behind the narrow waves' ncost and the
    // readers of hlist / hcount above by its order, behind bh_traverse's wcost
    // and nflag reads by the event; nothing on the main stream reads what it
    // writes before the tree's next build, which joins it: bh_select_join)
    if (nfac > 0.0 && !plim) {
        const hipStream_t ss = sel_off ? ctx->aux_stream : st;
        if (sel_off) TSNE_HIP(hipStreamWaitEvent(ss, ctx->aux_ev[2], 0));
        if (!narrow) TSNE_HIP(hipMemsetAsync(t.nflag, 0, sizeof(int32_t) * waves, ss));   // no stale slots
        const bool front = o.trav_front > 0.0;
        if (front) t.trav_order = ctx->ws.get<int32_t>(t.pre + "trav_order", ceil_div(t.tile_waves, TRAV_WPB) + 1);
        hipLaunchKernelGGL(narrow_select, dim3(1), dim3(1024), 0, ss, t.wcost, waves, t.nflag, t.ncost, t.hlist,
                           t.hcount, t.nar_hmax, nfac, std::min<int64_t>(t.nar_hmax, narrow_fill(ctx, waves)),
                           front ? t.trav_order : nullptr, o.trav_front);
        if (sel_off) {
            if (!t.sel_ev) TSNE_HIP(hipEventCreateWithFlags(&t.sel_ev, hipEventDisableTiming));
            TSNE_HIP(hipEventRecord(t.sel_ev, ss));
            t.sel_pending = true;
        }
        t.sel_waves = waves;
        t.front_waves = front ? waves : 0;
    } else {
        t.sel_waves = 0;
        t.front_waves = 0;
    }
    // the next traversal's split budgets (of the same query count) from this one's costs
    if (o.spill > 0.0 && o.spill_force == 0 && !plim) {
        bh_spill_alloc(ctx, t);
        hipLaunchKernelGGL(spill_budget, dim3(1), dim3(1024), 0, st, t.wcost, waves, o.spill, o.spill_task,
                           (int32_t)o.spill_min, t.sp_ctl);
        t.sp_waves = waves;
    } else {
        t.sp_waves = 0;
    }
    // the streamed lists' sums are in F, Z (and the control words zeroed)
    // before anything after this call reads them
    if (stream) TSNE_HIP(hipStreamWaitEvent(st, ctx->st_ev[1], 0));
    TSNE_LAUNCH_CHECK();
}

bool repulsion_stat(tsne_ctx *ctx, const std::string &name, int64_t *value_out) {
    // indices of bh_traverse's counters (its STATS block): wave pops, tile
    // points, wave child slots, reference-equivalent evaluations
    const int at = name == "bh.pops" ? 3 : name == "bh.tile_points" ? 4 : name == "bh.child_slots" ? 6
                 : name == "bh.visits" ? 0 : name == "bh.wave_ticks_max" ? 15 : name == "bh.wave_ticks_sum" ? 18
                 : name == "bh.span_ticks" ? 17 : name == "bh.dense_pairs" ? 2 : name == "bh.moment_evals" ? 1
                 : name == "bh.tile_ticks_max" ? 19 : name == "bh.tile_ticks_sum" ? 22 : name == "bh.tile_span_ticks" ? 21
                 : name == "bh.slow_wave_ticks" ? 33 : name == "bh.slow_wave_pops" ? 33 : name == "bh.slow_wave_ties" ? 34
                 : name == "bh.slow_wave_tile_points" ? 35 : name == "bh.slow_wave_slots" ? 36
                 : name == "bh.wave_mhz" ? 37 : -1;
    // tile_apply's dense paths k = 0..3 (lane-wise, packed, query-major, staged
    // sweep): "bh.tile_steps<k>" wave steps issued, "bh.tile_pairs<k>" useful lane pairs
    int atk = at;
    if (at < 0 && name.size() == 14 && name.compare(0, 13, "bh.tile_steps") == 0) atk = 24 + 2 * (name[13] - '0');
    if (at < 0 && name.size() == 14 && name.compare(0, 13, "bh.tile_pairs") == 0) atk = 25 + 2 * (name[13] - '0');
    // "bh.tile_gsteps<p>_<G>": the wave steps passes over G = 2, 4, 8 consecutive lane-wise windows (p = 0) or
    // packed rounds (p = 1) would take (counted with tile_pass <= 1); "bh.tile_rounds_max": the most packed
    // rounds of one wave; "bh.tile_chunked_waves": tile_apply waves that are one chunk of a split list
    if (at < 0 && name.size() == 17 && name.compare(0, 14, "bh.tile_gsteps") == 0 && name[15] == '_' &&
        (name[14] == '0' || name[14] == '1') && (name[16] == '2' || name[16] == '4' || name[16] == '8'))
        atk = (name[14] == '1' ? 38 : 41) + (name[16] == '2' ? 0 : name[16] == '4' ? 1 : 2);
    if (name == "bh.tile_rounds_max") atk = 44;
    if (name == "bh.tile_chunked_waves") atk = 45;
    if (name == "bh.narrow_moment_tasks") atk = 46;   // moment tasks of the narrow groups' queries
    if (atk < 0 || atk >= VIS_N) return false;
    TSNE_REQUIRE(ctx->opts.rep_stats && ctx->ws.has("rep.visits"), "counter '" + name + "' needs option rep_stats");
    unsigned long long v[VIS_N];
    TSNE_HIP(hipMemcpyAsync(v, ctx->ws.get<unsigned long long>("rep.visits", VIS_N), sizeof(v), hipMemcpyDeviceToHost,
                            ctx->stream));
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
    // span: last wave end - first wave start ([16] holds ~first start), 100 MHz ticks
    *value_out = atk == 17 ? (int64_t)(v[17] - (~0ull - v[16])) : atk == 21 ? (int64_t)(v[21] - (~0ull - v[20]))
                                                                              : (int64_t)v[atk];
    if (atk == 37) *value_out = v[18] ? (int64_t)(100.0 * (double)v[37] / (double)v[18]) : 0;
    if (atk >= 33 && atk <= 36)   // (ticks << 24 | count) of the slowest wave
        *value_out = name == "bh.slow_wave_ticks" ? (int64_t)(v[atk] >> 24) : (int64_t)(v[atk] & ((1ull << 24) - 1));
    return true;
}

}  // namespace tsne
