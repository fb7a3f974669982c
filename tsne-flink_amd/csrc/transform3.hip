// transform3.hip -- embedding new points into a fitted 3-D map on gfx950: the
// octree counterpart of transform.hip.
//
// The reference map Yr (n x 3) is fixed: its octree (octree.hip, the octal
// records of build_orec) is built once, and new points are QUERIES that are
// not in the tree.  The records mean the right thing for such a query: a leaf
// contributes 0 when its point equals the query (by position), every cell is
// summarised when the restatement's h / D < theta says so (D the squared 3-D
// distance to the cell's centre of mass).  This file holds
//   * foreign_walk3: the traversal for foreign queries, 64 per wave;
//   * bhx3_queries:  computeRepulsiveForce for a batch of foreign points;
//   * xform3_step:   one transform iteration for every new point in one
//                    launch -- walk, attraction over the point's CSR row,
//                    gradient with the point's own normaliser z_i, update;
//   * xform3_update: the split form's second launch (option transform_split);
//   * xq3_keys, xform3_init and the host pieces transform.hip dispatches to.
//
// Canonical order (transform.hip's rules, unchanged).  A wave's 64 queries
// share one LDS stack of (record, lane mask) entries.  The stack is strictly
// LIFO, one record per pop, and an opened cell's children are taken in slot
// order 0..7, each cell child pushed with the mask of the lanes that open it.
// The pops a lane takes part in are therefore the depth-first order of the
// records that lane opens, whatever the other lanes do.  All control flow is
// wave-uniform; a lane adds its terms in that order and a masked-out lane adds
// nothing -- not a zero product, which would turn -0.0 into +0.0 and spread a
// NaN.  So a query's sums are a function of the tree and the query alone:
// bit-identical in any batch, in any lane, under any sort of the queries.
//
// No tile tests, no near-exact radius and no subtree moments: the records'
// rball2, thr and ONCH_TILE are ignored, every cell decision is the
// restatement's, from the record's sure-open / sure-accept bounds on 1 + D
// (QACC_BAND, bhtree.hpp) and the exact IEEE quotient in between.
//
// Key ties.  The octree's keys have 21 levels per axis: distinct map points
// that share a level-21 cell (closer than ~1e-6 of the extent on every axis)
// are one OK_TIE group and interact with a query directly, point by point,
// where the restatement would go on splitting.  Exact duplicates are such a
// group too; they count as the restatement counts them (dup_fix3 below).
#include <algorithm>

#include <hipcub/hipcub.hpp>

#include "transform.hpp"

namespace tsne {
namespace {

constexpr int X3WPB = 4;       // waves per workgroup
// Stack entries per wave: a pop takes one entry and pushes <= 8, and the
// entries of one level are consumed before their parent's siblings, so the
// depth is <= 7 per level over the 21 octal levels, plus the root: 149 (a
// virtual chain top of the duplicate fix-up is one more pop with one push: at
// most one more entry per level, 170).  A full stack sets flag[0] and drops
// the push (never expected; the host entry points report it).
constexpr int X3STACK = 256;
constexpr int OREC_V4 = sizeof(ORec) / 16;   // 31 pieces of 16 bytes
static_assert(8 * LEVELS3 + 2 <= X3STACK, "foreign walk stack bound");
static_assert(OREC_V4 <= 64, "one fetch round per record");

// 14 KB per workgroup: the record of the current pop and the stack, per wave
struct X3LDS {
    ORec rec[X3WPB];
    uint64_t smask[X3WPB][X3STACK];
    int32_t sref[X3WPB][X3STACK];
};

struct X3Tree {
    const double4 *pos;
    const OctNode *nodes;
    const ORec *orec;
    const ORec *vrec;      // virtual chain-top records (refs >= virt), null without exact duplicates
    const int32_t *meta;   // [0] in-root points, [1] root ref
    int32_t virt;          // record ref offset of the virtual records (= n)
};

// 1/x as the tree's own traversal forms it (octree.hip rcp2): v_rcp_f64 and
// one Newton step, within 11 ulp of the IEEE quotient.
__device__ __forceinline__ double x3_recip(double x) {
    const double r = __builtin_amdgcn_rcp(x);
    return __fma_rn(r, __fma_rn(-x, r, 1.0), r);
}

// cnt points at their centre of mass: D1 = 1 + D
__device__ __forceinline__ void x3_term(double dx, double dy, double dz, double D1, double cnt, double &fx,
                                        double &fy, double &fz, double &zs) {
    const double Q = x3_recip(D1);
    const double mult = cnt * Q;
    const double sc = mult * Q;
    fx = __fma_rn(sc, dx, fx);
    fy = __fma_rn(sc, dy, fy);
    fz = __fma_rn(sc, dz, fz);
    zs += mult;
}

// 1 + D from one rounding per axis (the records' bounds are on this form)
__device__ __forceinline__ double x3_d1(double dx, double dy, double dz) {
    return __fma_rn(dx, dx, __fma_rn(dy, dy, __fma_rn(dz, dz, 1.0)));
}

// D as summarise3 (octree.hip) forms it: fl(fl(dx^2 + dy^2) + dz^2)
__device__ __forceinline__ double x3_d(double dx, double dy, double dz) {
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// one point; nothing if it is the query's own position
__device__ __forceinline__ void x3_leaf(double qx, double qy, double qz, double4 p, double &fx, double &fy,
                                        double &fz, double &zs) {
    if (p.x == qx && p.y == qy && p.z == qz) return;
    const double dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
    x3_term(dx, dy, dz, x3_d1(dx, dy, dz), 1.0, fx, fy, fz, zs);
}

// The walk of one wave: lane's query (qx, qy, qz) if `valid`.  See "Canonical
// order" above.  All control flow is wave-uniform; `valid` / the entries'
// masks predicate the lanes' terms.  STATS: pops counts the wave's pops.
template <bool STATS>
__device__ __forceinline__ void foreign_walk3(X3LDS &L, int w, int lane, const X3Tree &T, double theta, bool valid,
                                              double qx, double qy, double qz, double &fx, double &fy, double &fz,
                                              double &zs, int32_t *__restrict__ flag, unsigned long long &pops) {
    int sp = 0;
    // the root: a single point, a key-tie group, or a cell tested like any other
    const int root = T.meta[1];
    if (root == ~0) {
        if (valid) x3_leaf(qx, qy, qz, T.pos[0], fx, fy, fz, zs);
        return;
    }
    if (root < 0) return;   // no point in the root cell
    {
        const OctNode &rt = T.nodes[root];
        if (rt.delta >= 63) {
            for (int p = rt.first; p <= rt.last; ++p) {
                const double4 pp = T.pos[p];
                if (valid) x3_leaf(qx, qy, qz, pp, fx, fy, fz, zs);
            }
            return;
        }
        bool open = false;
        if (valid) {
            const double dx = qx - rt.cx, dy = qy - rt.cy, dz = qz - rt.cz;
            const double D = x3_d(dx, dy, dz);
            if (rt.h / D < theta) x3_term(dx, dy, dz, 1.0 + D, (double)rt.cnt, fx, fy, fz, zs);
            else open = true;
        }
        const uint64_t om = __ballot(open);
        if (om) {
            if (lane == 0) { L.sref[w][0] = root; L.smask[w][0] = om; }
            sp = 1;
        }
    }
    while (sp > 0) {
        --sp;
        if (STATS) ++pops;
        __builtin_amdgcn_wave_barrier();
        const int ref = __builtin_amdgcn_readfirstlane(L.sref[w][sp]);
        const uint64_t mv = L.smask[w][sp];
        const uint64_t msk = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(mv >> 32)) << 32) |
                             (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)mv);
        // the record, once per pop: 31 lanes x 16 bytes into LDS, read back as broadcasts
        const ORec *rsrc = ref < T.virt ? T.orec + ref : T.vrec + (ref - T.virt);
        if (lane < OREC_V4)
            reinterpret_cast<uint4 *>(&L.rec[w])[lane] = reinterpret_cast<const uint4 *>(rsrc)[lane];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        const ORec &nd = L.rec[w];
        const bool act = (msk >> lane) & 1ull;
        const int nch = __builtin_amdgcn_readfirstlane(nd.nch) & 0xff;   // ONCH_TILE ignored
        const int kinds = __builtin_amdgcn_readfirstlane(nd.kinds);
        for (int c = 0; c < nch; ++c) {
            const int kind = (kinds >> (2 * c)) & 3;   // wave-uniform
            const double dx = qx - nd.ccx[c], dy = qy - nd.ccy[c], dz = qz - nd.ccz[c];
            if (kind == OK_LEAF) {
                if (act && !(dx == 0.0 && dy == 0.0 && dz == 0.0))
                    x3_term(dx, dy, dz, x3_d1(dx, dy, dz), 1.0, fx, fy, fz, zs);
            } else if (kind == OK_CELL) {
                const double D1 = x3_d1(dx, dy, dz);   // 1 + D
                bool acc = false;
                if (act) {
                    if (D1 > nd.ca[c]) acc = true;
                    else if (D1 < nd.cb[c]) acc = false;
                    else {   // the band: the restatement's own quotient decides (a virtual chain top: half its parent)
                        const int32_t cref = nd.cref[c];
                        const double ch = cref < T.virt ? T.nodes[cref].h : 0.5 * T.nodes[ref].h;
                        acc = ch / x3_d(dx, dy, dz) < theta;
                    }
                }
                if (act && acc) x3_term(dx, dy, dz, D1, (double)nd.ccnt[c], fx, fy, fz, zs);
                const uint64_t om = __ballot(act && !acc);
                if (om) {
                    if (sp < X3STACK) {
                        if (lane == 0) { L.sref[w][sp] = nd.cref[c]; L.smask[w][sp] = om; }
                        ++sp;
                    } else if (lane == 0) {
                        atomicOr(flag, 1);
                    }
                }
            } else {                                   // a key-tie group: every point directly
                const OctNode &tn = T.nodes[__builtin_amdgcn_readfirstlane(nd.cref[c])];
                const int p0 = __builtin_amdgcn_readfirstlane(tn.first), p1 = __builtin_amdgcn_readfirstlane(tn.last);
                for (int p = p0; p <= p1; ++p) {
                    const double4 pp = T.pos[p];   // w != 0: a copy the restatement's leaf does not count (x3_dup_fix)
                    if (act && pp.w == 0.0) x3_leaf(qx, qy, qz, pp, fx, fy, fz, zs);
                }
            }
        }
    }
}

// Morton key of every query in the octree's root cell (the build's own key
// function and W); queries outside the root sort last.
__global__ void xq3_keys(const double *__restrict__ Q, int64_t m, const double *__restrict__ Wp,
                         uint64_t *__restrict__ keys, int32_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    keys[i] = morton3_key(Q[3 * i], Q[3 * i + 1], Q[3 * i + 2], *Wp);
    idx[i] = (int32_t)i;
}

// computeRepulsiveForce for foreign points: slot -> query row perm[slot].
// STATS (option transform_stats): stats[0] += the wave's pops.
template <bool STATS>
__global__ __launch_bounds__(64 * X3WPB) void bhx3_queries(X3Tree T, double theta, const double *__restrict__ Q,
                                                           const int32_t *__restrict__ perm, int64_t m,
                                                           double *__restrict__ F, double *__restrict__ Z,
                                                           int32_t *__restrict__ flag,
                                                           unsigned long long *__restrict__ stats) {
    __shared__ X3LDS L;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int64_t slot = (int64_t)blockIdx.x * (64 * X3WPB) + threadIdx.x;
    if (slot - lane >= m) return;   // the whole wave
    const bool valid = slot < m;
    const int64_t i = valid ? (int64_t)perm[slot] : 0;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (valid) { qx = Q[3 * i]; qy = Q[3 * i + 1]; qz = Q[3 * i + 2]; }
    double fx = 0.0, fy = 0.0, fz = 0.0, zs = 0.0;
    unsigned long long pops = 0;
    foreign_walk3<STATS>(L, w, lane, T, theta, valid, qx, qy, qz, fx, fy, fz, zs, flag, pops);
    if (valid) {
        F[3 * i] = fx;
        F[3 * i + 1] = fy;
        F[3 * i + 2] = fz;
        Z[i] = zs;
    }
    if (STATS && lane == 0) atomicAdd(stats, pops);
}

__device__ __forceinline__ double jmax3(double a, double b) {  // java.lang.Math.max
    if (a != a) return a;
    if (b != b) return b;
    return a >= b ? a : b;
}

// updateEmbedding (TsneHelpers.scala:341-369) of one component
__device__ __forceinline__ void x3_update(double g, double &y, double &u, double &gn, double min_gain, double mom,
                                          double lr) {
    gn = ((g > 0.0) == (u > 0.0)) ? jmax3(gn * 0.8, min_gain) : jmax3(gn + 0.2, min_gain);
    u = __dsub_rn(__dmul_rn(mom, u), __dmul_rn(__dmul_rn(lr, gn), g));
    y = __dadd_rn(u, y);
}

// Attraction over new point i's CSR row (sequential, CSR order, multiply and
// add apart), the gradient attr - rep / z_i with the point's own normaliser,
// and updateEmbedding on the three components.
template <bool LOSS>
__device__ __forceinline__ void point_update3(int64_t i, double yx, double yy, double yz, double fx, double fy,
                                              double fz, double zs, const double *__restrict__ Yr,
                                              const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                              const double *__restrict__ P, double *__restrict__ Y,
                                              double *__restrict__ upd, double *__restrict__ gains, double ex,
                                              double mom, double lr, double min_gain, double *__restrict__ lossq) {
    double ax = 0.0, ay = 0.0, az = 0.0, ls = 0.0;
    const int64_t e1 = row_ptr[i + 1];
    for (int64_t e = row_ptr[i]; e < e1; ++e) {
        const double *yj = Yr + 3 * (int64_t)col[e];
        const double pe = ex * P[e];
        const double dx = yx - yj[0], dy = yy - yj[1], dz = yz - yj[2];
        const double q = 1.0 / (1.0 + x3_d(dx, dy, dz));
        const double s = pe * q;
        ax = __dadd_rn(ax, __dmul_rn(s, dx));
        ay = __dadd_rn(ay, __dmul_rn(s, dy));
        az = __dadd_rn(az, __dmul_rn(s, dz));
        if (LOSS) ls = __dadd_rn(ls, __dmul_rn(pe, log(pe / (q / zs))));
    }
    const double gx = __dsub_rn(ax, fx / zs), gy = __dsub_rn(ay, fy / zs), gz = __dsub_rn(az, fz / zs);
    double ux = upd[3 * i], uy = upd[3 * i + 1], uz = upd[3 * i + 2];
    double nx = gains[3 * i], ny = gains[3 * i + 1], nz = gains[3 * i + 2];
    x3_update(gx, yx, ux, nx, min_gain, mom, lr);
    x3_update(gy, yy, uy, ny, min_gain, mom, lr);
    x3_update(gz, yz, uz, nz, min_gain, mom, lr);
    Y[3 * i] = yx; Y[3 * i + 1] = yy; Y[3 * i + 2] = yz;
    upd[3 * i] = ux; upd[3 * i + 1] = uy; upd[3 * i + 2] = uz;
    gains[3 * i] = nx; gains[3 * i + 1] = ny; gains[3 * i + 2] = nz;
    if (LOSS) lossq[i] = ls;
}

// One transform iteration of every new point: nothing crosses points, so the
// walk, the attraction, the gradient and the update are one launch.  The
// working set is read and written in place in the caller's order (slot -> row
// perm[slot]).  LOSS: lossq[row] = sum_e pe ln(pe / (q_e / z_i)), pe = ex P_e.
template <bool LOSS>
__global__ __launch_bounds__(64 * X3WPB) void xform3_step(X3Tree T, double theta, const double *__restrict__ Yr,
                                                          const int64_t *__restrict__ row_ptr,
                                                          const int32_t *__restrict__ col,
                                                          const double *__restrict__ P,
                                                          const int32_t *__restrict__ perm, int64_t m,
                                                          double *__restrict__ Y, double *__restrict__ upd,
                                                          double *__restrict__ gains, double ex, double mom, double lr,
                                                          double min_gain, double *__restrict__ lossq,
                                                          int32_t *__restrict__ flag) {
    __shared__ X3LDS L;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int64_t slot = (int64_t)blockIdx.x * (64 * X3WPB) + threadIdx.x;
    if (slot - lane >= m) return;   // the whole wave
    const bool valid = slot < m;
    const int64_t i = valid ? (int64_t)perm[slot] : 0;
    double yx = 0.0, yy = 0.0, yz = 0.0;
    if (valid) { yx = Y[3 * i]; yy = Y[3 * i + 1]; yz = Y[3 * i + 2]; }
    double fx = 0.0, fy = 0.0, fz = 0.0, zs = 0.0;
    unsigned long long pops = 0;
    foreign_walk3<false>(L, w, lane, T, theta, valid, yx, yy, yz, fx, fy, fz, zs, flag, pops);
    if (!valid) return;
    point_update3<LOSS>(i, yx, yy, yz, fx, fy, fz, zs, Yr, row_ptr, col, P, Y, upd, gains, ex, mom, lr, min_gain,
                        lossq);
}

// The split form (option transform_split, an A/B of the fused launch): the
// same update from the sums a bhx3_queries launch left in F and Z, one thread
// per new point in the caller's order.  The same arithmetic per point, so the
// same bits.
template <bool LOSS>
__global__ __launch_bounds__(256) void xform3_update(const double *__restrict__ F, const double *__restrict__ Z,
                                                     const double *__restrict__ Yr,
                                                     const int64_t *__restrict__ row_ptr,
                                                     const int32_t *__restrict__ col, const double *__restrict__ P,
                                                     int64_t m, double *__restrict__ Y, double *__restrict__ upd,
                                                     double *__restrict__ gains, double ex, double mom, double lr,
                                                     double min_gain, double *__restrict__ lossq) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    point_update3<LOSS>(i, Y[3 * i], Y[3 * i + 1], Y[3 * i + 2], F[3 * i], F[3 * i + 1], F[3 * i + 2], Z[i], Yr,
                        row_ptr, col, P, Y, upd, gains, ex, mom, lr, min_gain, lossq);
}

// y_i = sum_e P_e Yr[col_e]: sequential in CSR order, multiply and add apart
__global__ void xform3_init(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                            const double *__restrict__ P, int64_t m, const double *__restrict__ Yr,
                            double *__restrict__ Y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double ax = 0.0, ay = 0.0, az = 0.0;
    const int64_t e1 = row_ptr[i + 1];
    for (int64_t e = row_ptr[i]; e < e1; ++e) {
        const double *yj = Yr + 3 * (int64_t)col[e];
        const double p = P[e];
        ax = __dadd_rn(ax, __dmul_rn(p, yj[0]));
        ay = __dadd_rn(ay, __dmul_rn(p, yj[1]));
        az = __dadd_rn(az, __dmul_rn(p, yj[2]));
    }
    Y[3 * i] = ax;
    Y[3 * i + 1] = ay;
    Y[3 * i + 2] = az;
}

// ---- Exact duplicates: the restatement's multiplicities (the 2-D rule of
// bhtree.hip "Exact duplicates", restated for the transform's octree; the
// fit's tree keeps full multiplicity).  The restatement keeps one
// leaf per distinct point and counts every copy on the way down, but when a
// leaf holding copies of v splits (a different point arrived) it re-inserts v
// ONCE: a cell created after the first copy of v was inserted counts 1 + the
// copies inserted after its creation.  A cell is created when its parent cell
// P splits, at the row t2(P) of the first point in P whose value differs from
// the value of P's first point.  So cell X with parent P leaves out every copy
// that is not its value's first row and has row < t2(P); the root leaves out
// none.  The tree's real cell X is the deepest of a chain X1 .. Xk of cells
// with the same points: X1's parent is the real cell A above (t2 of A's
// points), X2 .. Xk's parent holds X's own points.  Where the two counts
// differ, X1 becomes a virtual record (ref n + X) with X as its only child.
// A duplicate group's leaf (a tie group child of A's record) leaves out the
// copies with row < t2(A): they are marked in pos.w for the walk.
// Not covered: a root whose points all share one octant (its chain top), and
// tie groups that mix distinct points (already an approximation).

// notfirst[s] = 1 if an equal point with a smaller row exists; dflag = any
__global__ void x3_dup_mark(const double4 *__restrict__ pos, const uint64_t *__restrict__ keys,
                            const int32_t *__restrict__ idx_sorted, const int32_t *__restrict__ dupc, int64_t n,
                            int32_t *__restrict__ notfirst, int32_t *__restrict__ dflag) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    int nf = 0;
    if (dupc[s] > 1) {
        const double4 q = pos[s];
        const uint64_t k = keys[s];
        const int32_t r = idx_sorted[s];
        for (int64_t t = s - 1; t >= 0 && keys[t] == k; --t) {
            const double4 p = pos[t];
            nf |= (p.x == q.x && p.y == q.y && p.z == q.z && idx_sorted[t] < r);
        }
        for (int64_t t = s + 1; t < n && keys[t] == k; ++t) {
            const double4 p = pos[t];
            nf |= (p.x == q.x && p.y == q.y && p.z == q.z && idx_sorted[t] < r);
        }
        atomicOr(dflag, 1);
    }
    notfirst[s] = nf;
}

__device__ __forceinline__ bool x3_real(const OctNode &nd) { return nd.h >= 0.0 && nd.delta < 63; }

// One wave per binary node: t2 of every real cell (INT32_MAX: one value only)
__global__ __launch_bounds__(256) void x3_dup_t2(const double4 *__restrict__ pos, const int32_t *__restrict__ idx_sorted,
                                                 const OctNode *__restrict__ nodes, const int32_t *__restrict__ meta,
                                                 int32_t *__restrict__ t2) {
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= (int64_t)meta[0] - 1) return;   // the whole wave
    const OctNode &nd = nodes[i];
    if (!x3_real(nd)) return;
    const int a = nd.first, b = nd.last;
    unsigned long long best = ~0ull;   // (row, sorted position) of the cell's first point
    for (int p = a + lane; p <= b; p += 64) {
        const unsigned long long v = ((unsigned long long)(uint32_t)idx_sorted[p] << 32) | (uint32_t)p;
        best = v < best ? v : best;
    }
    best = wave_min(best);
    const double4 f = pos[(int)(uint32_t)best];
    int32_t t = INT32_MAX;
    for (int p = a + lane; p <= b; p += 64) {
        const double4 q = pos[p];
        if (q.x != f.x || q.y != f.y || q.z != f.z) t = min(t, idx_sorted[p]);
    }
    t = wave_min(t);
    if (lane == 0) t2[i] = t;
}

// One wave per real cell A: the child summaries of its record as the
// restatement counts them, the virtual chain tops, the leaf marks.
__global__ __launch_bounds__(256) void x3_dup_fix(double4 *__restrict__ pos, const int32_t *__restrict__ idx_sorted,
                                                  const int32_t *__restrict__ notfirst,
                                                  const OctNode *__restrict__ nodes, const int32_t *__restrict__ meta,
                                                  const int32_t *__restrict__ t2, double inv_theta, int32_t virt,
                                                  ORec *__restrict__ orec, ORec *__restrict__ vrec) {
    const int lane = lane_id();
    const int64_t A = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (A >= (int64_t)meta[0] - 1) return;   // the whole wave
    const OctNode &na = nodes[A];
    if (!x3_real(na)) return;
    ORec &r = orec[A];
    const int nch = r.nch & 0xff, kinds = r.kinds;
    const int32_t TA = t2[A];
    for (int c = 0; c < nch; ++c) {
        const int kind = (kinds >> (2 * c)) & 3;
        if (kind == OK_LEAF) continue;
        const int32_t x = r.cref[c];
        const OctNode &nx = nodes[x];
        const int a = nx.first, b = nx.last;
        if (kind == OK_TIE) {
            for (int p = a + lane; p <= b; p += 64)
                if (notfirst[p] && idx_sorted[p] < TA) pos[p].w = 1.0;
            continue;
        }
        const int k = ilogb(na.h) - ilogb(nx.h);   // chain length: octal levels from A down to x
        const int32_t Tk = k > 1 ? t2[x] : TA;
        int e1 = 0, ek = 0;
        double s1x = 0.0, s1y = 0.0, s1z = 0.0, skx = 0.0, sky = 0.0, skz = 0.0;
        for (int p = a + lane; p <= b; p += 64) {
            if (!notfirst[p]) continue;
            const int32_t row = idx_sorted[p];
            const double4 q = pos[p];
            if (row < TA) { ++e1; s1x += q.x; s1y += q.y; s1z += q.z; }
            if (row < Tk) { ++ek; skx += q.x; sky += q.y; skz += q.z; }
        }
        e1 = wave_sum(e1); ek = wave_sum(ek);
        if ((e1 | ek) == 0) continue;   // wave-uniform
        s1x = wave_sum(s1x); s1y = wave_sum(s1y); s1z = wave_sum(s1z);
        skx = wave_sum(skx); sky = wave_sum(sky); skz = wave_sum(skz);
        if (lane != 0) continue;
        const double cn = (double)nx.cnt;
        const double c1 = (double)(nx.cnt - e1), ck = (double)(nx.cnt - ek);
        const double x1 = (nx.cx * cn - s1x) / c1, y1 = (nx.cy * cn - s1y) / c1, z1 = (nx.cz * cn - s1z) / c1;
        const double xk = (nx.cx * cn - skx) / ck, yk = (nx.cy * cn - sky) / ck, zk = (nx.cz * cn - skz) / ck;
        if (e1 != ek) {   // the chain top counts differently: a virtual record with x as its only child
            ORec v = {};
            v.cx = x1; v.cy = y1; v.cz = z1;
            v.first = a; v.last = b; v.cnt = nx.cnt - e1; v.nch = 1; v.kinds = OK_CELL;
            v.ccx[0] = xk; v.ccy[0] = yk; v.ccz[0] = zk;
            v.cb[0] = r.cb[c]; v.ca[0] = r.ca[c];
            v.cref[0] = x; v.ccnt[0] = nx.cnt - ek;
            vrec[x] = v;
            const double h1 = 0.5 * na.h;
            r.cb[c] = qacc_open(h1, inv_theta);
            r.ca[c] = qacc_accept(h1, inv_theta);
            r.cref[c] = virt + x;
        }
        r.ccx[c] = x1; r.ccy[c] = y1; r.ccz[c] = z1;
        r.ccnt[c] = nx.cnt - e1;
    }
}

// The fix-up after a build; without an exact duplicate in the map only
// x3_dup_mark and the read-back of its flag run.
void dup_fix3(tsne_ctx *ctx, OctTree &t, double theta, const std::string &pre) {
    Workspace &ws = ctx->ws;
    hipStream_t st = ctx->stream;
    const int64_t n = t.n;
    t.vrec = nullptr;
    int32_t *dflag = ws.get<int32_t>(pre + "dflag", 1);
    int32_t *notfirst = ws.get<int32_t>(pre + "notfirst", n);
    TSNE_HIP(hipMemsetAsync(dflag, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(x3_dup_mark, dim3(ceil_div(n, 256)), dim3(256), 0, st, t.pos, t.keys_sorted, t.idx_sorted, t.dupc,
                       n, notfirst, dflag);
    int32_t h = 0;
    TSNE_HIP(hipMemcpyAsync(&h, dflag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TSNE_HIP(hipStreamSynchronize(st));
    if (!h) return;
    int32_t *t2 = ws.get<int32_t>(pre + "t2", n);
    t.vrec = ws.get<ORec>(pre + "vrec", n);
    const double inv_theta = theta > 0.0 ? 1.0 / theta : __builtin_inf();
    hipLaunchKernelGGL(x3_dup_t2, dim3(ceil_div(n, 4)), dim3(256), 0, st, t.pos, t.idx_sorted, t.nodes, t.meta, t2);
    hipLaunchKernelGGL(x3_dup_fix, dim3(ceil_div(n, 4)), dim3(256), 0, st, t.pos, t.idx_sorted, notfirst, t.nodes, t.meta,
                       t2, inv_theta, (int32_t)n, t.orec, t.vrec);
    TSNE_LAUNCH_CHECK();
}

X3Tree tree_view3(const OctTree &t) { return X3Tree{t.pos, t.nodes, t.orec, t.vrec, t.meta, (int32_t)t.n}; }

// Build the reference map's octree for foreign queries: the records whatever
// Options::oct_records says (they are what the walk reads), and no subtree
// moments (the walk uses none).
void build_tree3(tsne_ctx *ctx, OctTree &t, const double *dY, int64_t n, double theta, const char *pre) {
    if (t.n != n) oct_alloc(ctx, t, n, pre, true);
    oct_build(ctx, t, dY, theta, false, true);
    dup_fix3(ctx, t, theta, pre);
}

// perm = the queries' rows in the order of their Morton keys in t's root cell
int32_t *sort_queries3(tsne_ctx *ctx, const OctTree &t, const double *dQ, int64_t m, const std::string &pre) {
    Workspace &ws = ctx->ws;
    hipStream_t st = ctx->stream;
    uint64_t *keys = ws.get<uint64_t>(pre + "qkeys", m), *keys2 = ws.get<uint64_t>(pre + "qkeys2", m);
    int32_t *idx = ws.get<int32_t>(pre + "qidx", m), *perm = ws.get<int32_t>(pre + "qperm", m);
    hipLaunchKernelGGL(xq3_keys, dim3(ceil_div(m, 256)), dim3(256), 0, st, dQ, m, t.W, keys, idx);
    size_t tb = 0;
    TSNE_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys, keys2, idx, perm, (int)m, 0, 64, st));
    void *tmp = ws.get<uint8_t>(pre + "qsort_tmp", tb);
    TSNE_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb, keys, keys2, idx, perm, (int)m, 0, 64, st));
    return perm;
}

// the walk alone, slot -> row perm[slot]; stats: the waves' pops are counted
// into "octx1.stats" (option transform_stats, tsne_ctx_counter "xform3.pops")
void launch_queries3(tsne_ctx *ctx, const OctTree &t, double theta, const double *dQ, const int32_t *perm, int64_t m,
                     double *dF, double *dz, int32_t *flag, bool want_stats) {
    const dim3 grid(ceil_div(m, 64 * X3WPB)), block(64 * X3WPB);
    if (want_stats) {
        unsigned long long *stats = ctx->ws.get<unsigned long long>("octx1.stats", 1);
        TSNE_HIP(hipMemsetAsync(stats, 0, sizeof(unsigned long long), ctx->stream));
        hipLaunchKernelGGL(bhx3_queries<true>, grid, block, 0, ctx->stream, tree_view3(t), theta, dQ, perm, m, dF, dz,
                           flag, stats);
    } else {
        hipLaunchKernelGGL(bhx3_queries<false>, grid, block, 0, ctx->stream, tree_view3(t), theta, dQ, perm, m, dF, dz,
                           flag, (unsigned long long *)nullptr);
    }
}

}  // namespace

void repulsion_queries3_device(tsne_ctx *ctx, const double *dY, int64_t n, double theta, const double *dQ, int64_t m,
                               double *dF, double *dz) {
    TSNE_REQUIRE(n >= 1, "empty embedding");
    TSNE_REQUIRE(m >= 0, "negative query count");
    TSNE_REQUIRE(n < (int64_t)INT32_MAX && m < (int64_t)INT32_MAX, "n and m must fit int32 ids");
    if (m == 0) return;
    if (!ctx->query_tree3) ctx->query_tree3 = new OctTree();
    OctTree &t = *ctx->query_tree3;
    build_tree3(ctx, t, dY, n, theta, "octx1.");
    int32_t *flag = walk_flag(ctx, "octx1.");
    const int32_t *perm = sort_queries3(ctx, t, dQ, m, "octx1.");
    launch_queries3(ctx, t, theta, dQ, perm, m, dF, dz, flag, ctx->opts.transform_stats != 0);
    TSNE_LAUNCH_CHECK();
}

void transform_init3_device(tsne_ctx *ctx, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_P,
                            int64_t m, const double *d_Yref, int64_t n, double *d_Y) {
    TSNE_REQUIRE(m >= 0 && n >= 1, "bad sizes");
    if (m == 0) return;
    hipLaunchKernelGGL(xform3_init, dim3(ceil_div(m, 256)), dim3(256), 0, ctx->stream, d_row_ptr, d_col, d_P, m,
                       d_Yref, d_Y);
    TSNE_LAUNCH_CHECK();
}

void transform3_build(tsne_ctx *ctx, TransformState *s) {
    build_tree3(ctx, s->otree, s->Yref, s->n, s->prm.theta, "octx.");
    s->flag = walk_flag(ctx, "octx.");
    transform3_sort(ctx, s);
}

void transform3_sort(tsne_ctx *ctx, TransformState *s) {
    s->perm = sort_queries3(ctx, s->otree, s->Y, s->m, "octx.");
}

void transform3_launch(tsne_ctx *ctx, TransformState *s, double ex, double mom, bool loss) {
    const tsne_params &p = s->prm;
    hipStream_t st = ctx->stream;
    const dim3 grid(ceil_div(s->m, 64 * X3WPB)), block(64 * X3WPB);
    const X3Tree T = tree_view3(s->otree);
    if (ctx->opts.transform_split) {   // A/B: the walk and the update as two launches (the same bits)
        double *F = ctx->ws.get<double>("octx.splitF", 3 * (size_t)s->m);
        double *Z = ctx->ws.get<double>("octx.splitZ", s->m);
        launch_queries3(ctx, s->otree, p.theta, s->Y, s->perm, s->m, F, Z, s->flag, false);
        const dim3 ug(ceil_div(s->m, 256)), ub(256);
        if (loss)
            hipLaunchKernelGGL(xform3_update<true>, ug, ub, 0, st, F, Z, s->Yref, s->row_ptr, s->col, s->P, s->m, s->Y,
                               s->upd, s->gains, ex, mom, p.learning_rate, p.min_gain, s->lossq);
        else
            hipLaunchKernelGGL(xform3_update<false>, ug, ub, 0, st, F, Z, s->Yref, s->row_ptr, s->col, s->P, s->m, s->Y,
                               s->upd, s->gains, ex, mom, p.learning_rate, p.min_gain, s->lossq);
    } else if (loss) {
        hipLaunchKernelGGL(xform3_step<true>, grid, block, 0, st, T, p.theta, s->Yref, s->row_ptr, s->col, s->P,
                           s->perm, s->m, s->Y, s->upd, s->gains, ex, mom, p.learning_rate, p.min_gain, s->lossq,
                           s->flag);
    } else {
        hipLaunchKernelGGL(xform3_step<false>, grid, block, 0, st, T, p.theta, s->Yref, s->row_ptr, s->col, s->P,
                           s->perm, s->m, s->Y, s->upd, s->gains, ex, mom, p.learning_rate, p.min_gain, s->lossq,
                           s->flag);
    }
}

int64_t transform3_pops(tsne_ctx *ctx) {
    if (!ctx->ws.has("octx1.stats")) return 0;
    unsigned long long h = 0;
    TSNE_HIP(hipMemcpyAsync(&h, ctx->ws.get<unsigned long long>("octx1.stats", 1), sizeof(h), hipMemcpyDeviceToHost,
                            ctx->stream));
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
    return (int64_t)h;
}

}  // namespace tsne
