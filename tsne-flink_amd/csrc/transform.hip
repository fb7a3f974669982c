// transform.hip -- embedding new points into a fitted map on gfx950.
//
// The reference map Yr (n x C, C = 2 or 3) is fixed: its tree is built once --
// the quadtree with the records of bh_build (bhtree_build.hip) for C = 2, the octree
// with the octal records of build_orec (octree.hip) for C = 3 -- and new
// points are QUERIES that are not in the tree.  The records already mean the
// right thing for such a query: a leaf contributes 0 when its point equals
// the query (by position), every cell is summarised when the reference's
// h / D < theta says so (QuadTree.scala:134; D the squared distance to the
// cell's centre of mass, for C = 3 in the oracle's octree restatement).
// This file holds, once for both widths,
//   * the two traversals for foreign queries, 64 per wave: foreign_walk over
//     the quadtree's QRec records, foreign_walk3 over the octree's ORec
//     records, each behind a small trait (Quad / Oct) with its tree's view,
//     LDS layout, Morton key, build and workspace prefixes;
//   * bhx_queries:  computeRepulsiveForce for a batch of foreign points;
//   * xform_step:   one transform iteration for every new point in one
//                   launch -- walk, attraction over the point's CSR row,
//                   gradient with the point's own normaliser z_i, update;
//   * xform_update: the split form's second launch (option transform_split);
//   * the host side: the query sort, the trees kept in the context, the loss.
// Everything but the walks is written over the component count C; rows of C
// doubles are read and written through load_row / store_row.
//
// Canonical order.  A wave's 64 queries share one LDS stack of (record, lane
// mask) entries.  The stack is strictly LIFO, one record per pop, and an
// opened cell's children are taken in slot order (0..3, 0..7), each cell
// child pushed with the mask of the lanes that open it.  The sequence of pops
// is therefore the depth-first order of the TREE restricted to the records
// some lane opens; the pops a given lane takes part in are the depth-first
// order of the records that lane opens, whatever the other lanes do.  All
// control flow is wave-uniform; a lane adds its terms (the children of every
// record it is active for) in that order and a masked-out lane adds nothing
// -- not a zero product, which would turn -0.0 into +0.0 and spread a NaN.
// So a query's sums are a function of the tree and the query alone:
// bit-identical in any batch, in any lane, under any sort of the queries.
// The Morton sort of the queries only makes the lanes of a wave open the same
// records (fewer pops per wave).
//
// No subtree moments, no all-open tiles and no near-exact shortcut are used
// here (the octal records' rball2, thr and ONCH_TILE are ignored): every
// decision is the reference's, from the record's sure-accept / sure-open
// bounds on 1 + D (QACC_BAND, bhtree.hpp) and the exact IEEE quotient in
// between.
//
// Key ties (C = 3).  The octree's keys have 21 levels per axis: distinct map
// points that share a level-21 cell (closer than ~1e-6 of the extent on every
// axis) are one OK_TIE group and interact with a query directly, point by
// point, where the restatement would go on splitting.  Exact duplicates are
// such a group too; they count as the restatement counts them (dup_fix3
// below; the quadtree does that work inside bh_build).
#include <algorithm>

#include <hipcub/hipcub.hpp>

#include "transform.hpp"

namespace tsne {
namespace {

constexpr int XWPB = 4;       // waves per workgroup

// Per workgroup: the record of the current pop and the stack, per wave
template <class Rec, int N>
struct WalkLDS {
    static constexpr int STACK = N;
    Rec rec[XWPB];
    uint64_t smask[XWPB][N];
    int32_t sref[XWPB][N];
};
// Stack entries per wave.  A pop takes one entry and pushes <= 4 (8), and the
// entries of one level are consumed before their parent's siblings.  A full
// stack sets flag[0] and drops the push (never expected; the host entry
// points report it).
// Quadtree: <= 3 per level + 1 over the 31 quad levels, the root and the
// virtual chain tops of duplicate groups: < 128.  7 KB.
using XLDS = WalkLDS<QRec, 128>;
// Octree: <= 7 per level over the 21 octal levels, plus the root: 149 (a
// virtual chain top of the duplicate fix-up is one more pop with one push: at
// most one more entry per level, 170).  14 KB.
using X3LDS = WalkLDS<ORec, 256>;
static_assert(8 * LEVELS3 + 2 <= X3LDS::STACK, "foreign walk stack bound");
static_assert(sizeof(ORec) / 16 <= 64 && sizeof(QRec) / 16 <= 64, "one fetch round per record");

struct XTree {
    const double2 *pos;
    const BHNode *nodes;
    const QRec *qrec;
    const int32_t *meta;   // [0] in-root points, [1] root ref, [3] root replaced by its virtual chain top
    int32_t virt;          // record index offset of the virtual chain tops (= n)
};

struct X3Tree {
    const double4 *pos;
    const OctNode *nodes;
    const ORec *orec;
    const ORec *vrec;      // virtual chain-top records (refs >= virt), null without exact duplicates
    const int32_t *meta;   // [0] in-root points, [1] root ref
    int32_t virt;          // record ref offset of the virtual records (= n)
};

// Row i of an m x C array.  A 2-D row is one 16-byte access; a 24-byte 3-D
// row is not 16-byte aligned and takes three 8-byte ones.
template <int C>
__device__ __forceinline__ void load_row(const double *__restrict__ a, int64_t i, double (&v)[C]) {
    if constexpr (C == 2) {
        const double2 t = reinterpret_cast<const double2 *>(a)[i];
        v[0] = t.x; v[1] = t.y;
    } else {
#pragma unroll
        for (int k = 0; k < C; ++k) v[k] = a[C * i + k];
    }
}

template <int C>
__device__ __forceinline__ void store_row(double *__restrict__ a, int64_t i, const double (&v)[C]) {
    if constexpr (C == 2) {
        reinterpret_cast<double2 *>(a)[i] = make_double2(v[0], v[1]);
    } else {
#pragma unroll
        for (int k = 0; k < C; ++k) a[C * i + k] = v[k];
    }
}

// 1/x as the trees' own traversals form it (bhtree.hip recip_bh, octree.hip
// rcp2): v_rcp_f64 and one Newton step, within 11 ulp of the IEEE quotient.
__device__ __forceinline__ double x_recip(double x) {
    const double r = __builtin_amdgcn_rcp(x);
    return __fma_rn(r, __fma_rn(-x, r, 1.0), r);
}

// 1 + D from one rounding per axis, the 1 innermost at the last axis (the
// records' bounds are on this form)
template <int C>
__device__ __forceinline__ double x_d1(const double (&d)[C]) {
    double s = 1.0;
#pragma unroll
    for (int k = C - 1; k >= 0; --k) s = __fma_rn(d[k], d[k], s);
    return s;
}

// D as the reference forms it: separately rounded squares, added from axis 0
template <int C>
__device__ __forceinline__ double x_d(const double (&d)[C]) {
    double s = __dmul_rn(d[0], d[0]);
#pragma unroll
    for (int k = 1; k < C; ++k) s = __dadd_rn(s, __dmul_rn(d[k], d[k]));
    return s;
}

// cnt points at their centre of mass (QuadTree.scala:134-142): D1 = 1 + D
template <int C>
__device__ __forceinline__ void x_term(const double (&d)[C], double D1, double cnt, double (&f)[C], double &zs) {
    const double Q = x_recip(D1);
    const double mult = cnt * Q;
    const double sc = mult * Q;
#pragma unroll
    for (int k = 0; k < C; ++k) f[k] = __fma_rn(sc, d[k], f[k]);
    zs += mult;
}

// one point; nothing if it is the query's own position (QuadTree.scala:128)
template <int C>
__device__ __forceinline__ void x_leaf(const double (&q)[C], const double (&p)[C], double (&f)[C], double &zs) {
    bool same = true;
    double d[C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
        same = same && p[k] == q[k];
        d[k] = q[k] - p[k];
    }
    if (same) return;
    x_term(d, x_d1(d), 1.0, f, zs);
}

// ---- The pieces of a pop the two walks share (WalkLDS of either record).

// the entry at sp: its record ref and lane mask, wave-uniform
template <class LDS>
__device__ __forceinline__ int x_pop(const LDS &L, int w, int sp, uint64_t &msk) {
    __builtin_amdgcn_wave_barrier();
    const int ref = __builtin_amdgcn_readfirstlane(L.sref[w][sp]);
    const uint64_t mv = L.smask[w][sp];
    msk = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(mv >> 32)) << 32) |
          (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)mv);
    return ref;
}

// the record, once per pop: one lane per 16 bytes into LDS, read back as broadcasts
template <class Rec>
__device__ __forceinline__ void x_fetch(Rec &dst, int lane, const Rec *src) {
    if (lane < (int)(sizeof(Rec) / 16))
        reinterpret_cast<uint4 *>(&dst)[lane] = reinterpret_cast<const uint4 *>(src)[lane];
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
}

// push (ref, om) for the lanes om that open a cell child; a full stack raises the flag
template <class LDS>
__device__ __forceinline__ void x_push(LDS &L, int w, int lane, int &sp, int32_t ref, uint64_t om,
                                       int32_t *__restrict__ flag) {
    if (sp < LDS::STACK) {
        if (lane == 0) { L.sref[w][sp] = ref; L.smask[w][sp] = om; }
        ++sp;
    } else if (lane == 0) {
        atomicOr(flag, 1);
    }
}

// The quadtree walk of one wave: lane's query q if `valid`.  See "Canonical
// order" above.  All control flow is wave-uniform; `valid` / the entries'
// masks predicate the lanes' terms.
__device__ __forceinline__ void foreign_walk(XLDS &L, int w, int lane, const XTree &T, double theta, bool valid,
                                             const double (&q)[2], double (&f)[2], double &zs,
                                             int32_t *__restrict__ flag) {
    int sp = 0;
    // the root: a single point, a key-tie group, or a cell tested like any other
    const int root = T.meta[1];
    if (root == ~0) {
        const double2 pp = T.pos[0];
        if (valid) x_leaf<2>(q, {pp.x, pp.y}, f, zs);
        return;
    }
    if (root < 0) return;   // no point in the root cell
    {
        const BHNode &rt = T.nodes[root];
        if (rt.delta >= 62) {
            for (int p = rt.first; p <= rt.last; ++p) {
                const double2 pp = T.pos[p];
                if (valid) x_leaf<2>(q, {pp.x, pp.y}, f, zs);
            }
            return;
        }
        double rh = rt.h, rcx = rt.cx, rcy = rt.cy;
        int32_t rcnt = rt.cnt, rpush = root;
        if (T.meta[3]) {   // duplicates the reference root counts differently: its virtual record (h = W)
            const QRec &vq = T.qrec[T.virt + root];
            rh = ldexp(rt.h, rt.delta >> 1);
            rcx = vq.cx; rcy = vq.cy; rcnt = vq.cnt; rpush = T.virt + root;
        }
        bool open = false;
        if (valid) {
            const double d[2] = {q[0] - rcx, q[1] - rcy};
            const double D = x_d(d);
            if (rh / D < theta) x_term(d, 1.0 + D, (double)rcnt, f, zs);
            else open = true;
        }
        const uint64_t om = __ballot(open);
        if (om) {
            if (lane == 0) { L.sref[w][0] = rpush; L.smask[w][0] = om; }
            sp = 1;
        }
    }
    while (sp > 0) {
        --sp;
        uint64_t msk;
        const int ref = x_pop(L, w, sp, msk);
        x_fetch(L.rec[w], lane, T.qrec + ref);
        const QRec &nd = L.rec[w];
        const bool act = (msk >> lane) & 1ull;
        const int nflags = __builtin_amdgcn_readfirstlane(nd.nch);
        const int nch = nflags & 0xff;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c >= nch) break;
            const int kind = (nflags >> (QNCH_KIND + 2 * c)) & 3;   // wave-uniform
            const double d[2] = {q[0] - nd.ccx[c], q[1] - nd.ccy[c]};
            if (kind == QK_LEAF) {
                if (act && !(d[0] == 0.0 && d[1] == 0.0)) x_term(d, x_d1(d), 1.0, f, zs);
            } else if (kind == QK_CELL) {
                const double D1 = x_d1(d);   // 1 + D
                bool acc = false;
                if (act) {
                    if (D1 > nd.ca[c]) acc = true;
                    else if (D1 < nd.cb[c]) acc = false;
                    else {   // the band: the reference's own quotient decides
                        const int32_t cref = nd.cref[c];
                        const double ch = cref < T.virt ? T.nodes[cref].h : 0.5 * T.nodes[ref].h;
                        acc = ch / x_d(d) < theta;
                    }
                }
                if (act && acc) x_term(d, D1, (double)nd.ccnt[c], f, zs);
                const uint64_t om = __ballot(act && !acc);
                if (om) x_push(L, w, lane, sp, nd.cref[c], om, flag);
            } else if (kind == QK_MULTI) {   // a leaf of ccnt copies: 0 if it is the query's position
                if (act && !(nd.ccx[c] == q[0] && nd.ccy[c] == q[1])) x_term(d, x_d1(d), (double)nd.ccnt[c], f, zs);
            } else {                         // a key-tie group: every point directly
                const BHNode &tn = T.nodes[__builtin_amdgcn_readfirstlane(nd.cref[c])];
                const int p0 = __builtin_amdgcn_readfirstlane(tn.first), p1 = __builtin_amdgcn_readfirstlane(tn.last);
                for (int p = p0; p <= p1; ++p) {
                    const double2 pp = T.pos[p];
                    if (act) x_leaf<2>(q, {pp.x, pp.y}, f, zs);
                }
            }
        }
    }
}

// The octree walk of one wave, under the same rules.  STATS: pops counts the
// wave's pops.
template <bool STATS>
__device__ __forceinline__ void foreign_walk3(X3LDS &L, int w, int lane, const X3Tree &T, double theta, bool valid,
                                              const double (&q)[3], double (&f)[3], double &zs,
                                              int32_t *__restrict__ flag, unsigned long long &pops) {
    int sp = 0;
    // the root: a single point, a key-tie group, or a cell tested like any other
    const int root = T.meta[1];
    if (root == ~0) {
        const double4 pp = T.pos[0];
        if (valid) x_leaf<3>(q, {pp.x, pp.y, pp.z}, f, zs);
        return;
    }
    if (root < 0) return;   // no point in the root cell
    {
        const OctNode &rt = T.nodes[root];
        if (rt.delta >= 63) {
            for (int p = rt.first; p <= rt.last; ++p) {
                const double4 pp = T.pos[p];
                if (valid) x_leaf<3>(q, {pp.x, pp.y, pp.z}, f, zs);
            }
            return;
        }
        bool open = false;
        if (valid) {
            const double d[3] = {q[0] - rt.cx, q[1] - rt.cy, q[2] - rt.cz};
            const double D = x_d(d);
            if (rt.h / D < theta) x_term(d, 1.0 + D, (double)rt.cnt, f, zs);
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
        uint64_t msk;
        const int ref = x_pop(L, w, sp, msk);
        x_fetch(L.rec[w], lane, ref < T.virt ? T.orec + ref : T.vrec + (ref - T.virt));
        const ORec &nd = L.rec[w];
        const bool act = (msk >> lane) & 1ull;
        const int nch = __builtin_amdgcn_readfirstlane(nd.nch) & 0xff;   // ONCH_TILE ignored
        const int kinds = __builtin_amdgcn_readfirstlane(nd.kinds);
        for (int c = 0; c < nch; ++c) {
            const int kind = (kinds >> (2 * c)) & 3;   // wave-uniform
            const double d[3] = {q[0] - nd.ccx[c], q[1] - nd.ccy[c], q[2] - nd.ccz[c]};
            if (kind == OK_LEAF) {
                if (act && !(d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0)) x_term(d, x_d1(d), 1.0, f, zs);
            } else if (kind == OK_CELL) {
                const double D1 = x_d1(d);   // 1 + D
                bool acc = false;
                if (act) {
                    if (D1 > nd.ca[c]) acc = true;
                    else if (D1 < nd.cb[c]) acc = false;
                    else {   // the band: the restatement's own quotient decides (a virtual chain top: half its parent)
                        const int32_t cref = nd.cref[c];
                        const double ch = cref < T.virt ? T.nodes[cref].h : 0.5 * T.nodes[ref].h;
                        acc = ch / x_d(d) < theta;
                    }
                }
                if (act && acc) x_term(d, D1, (double)nd.ccnt[c], f, zs);
                const uint64_t om = __ballot(act && !acc);
                if (om) x_push(L, w, lane, sp, nd.cref[c], om, flag);
            } else {                                   // a key-tie group: every point directly
                const OctNode &tn = T.nodes[__builtin_amdgcn_readfirstlane(nd.cref[c])];
                const int p0 = __builtin_amdgcn_readfirstlane(tn.first), p1 = __builtin_amdgcn_readfirstlane(tn.last);
                for (int p = p0; p <= p1; ++p) {
                    const double4 pp = T.pos[p];   // w != 0: a copy the restatement's leaf does not count (x3_dup_fix)
                    if (act && pp.w == 0.0) x_leaf<3>(q, {pp.x, pp.y, pp.z}, f, zs);
                }
            }
        }
    }
}

// ---- Exact duplicates in the octree: the restatement's multiplicities (the
// 2-D rule of bhtree_build.hip "Exact duplicates", restated for the transform's
// octree; the fit's tree keeps full multiplicity).  The
// restatement keeps one leaf per distinct point and counts every copy on the
// way down, but when a leaf holding copies of v splits (a different point
// arrived) it re-inserts v ONCE: a cell created after the first copy of v was
// inserted counts 1 + the copies inserted after its creation.  A cell is
// created when its parent cell P splits, at the row t2(P) of the first point
// in P whose value differs from the value of P's first point.  So cell X with
// parent P leaves out every copy that is not its value's first row and has
// row < t2(P); the root leaves out none.  The tree's real cell X is the
// deepest of a chain X1 .. Xk of cells with the same points: X1's parent is
// the real cell A above (t2 of A's points), X2 .. Xk's parent holds X's own
// points.  Where the two counts differ, X1 becomes a virtual record (ref
// n + X) with X as its only child.  A duplicate group's leaf (a tie group
// child of A's record) leaves out the copies with row < t2(A): they are
// marked in pos.w for the walk.
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

// ---- The two trees behind one shape: what the kernels and the host side
// below need from a tree.  pre: the workspace prefix of the transform state's
// tree (tree()), pre1: that of the single-call operators' (tree1(), made on
// first use); two trees never share buffers.
struct Quad {
    static constexpr int C = 2;
    static constexpr bool counts_pops = false;
    static constexpr const char *pre = "bhx.", *pre1 = "bhx1.";
    using Tree = BHTree;
    using View = XTree;
    using LDS = XLDS;
    static __device__ __forceinline__ uint64_t key(const double (&q)[2], double W) {
        return morton2_key(q[0], q[1], W);
    }
    template <bool STATS>
    static __device__ __forceinline__ void walk(LDS &L, int w, int lane, const View &T, double theta, bool valid,
                                                const double (&q)[2], double (&f)[2], double &zs,
                                                int32_t *__restrict__ flag, unsigned long long &) {
        foreign_walk(L, w, lane, T, theta, valid, q, f, zs, flag);
    }
    static View view(const Tree &t) { return View{t.pos, t.nodes, t.qrec, t.meta, (int32_t)t.n}; }
    // The full build (no root-tile shortcut: its records are what the walk
    // reads).  The walk uses no subtree moments, so the ones the fused build
    // defers to the traversal call are not run at all.
    static void build(tsne_ctx *ctx, Tree &t, const double *dY, int64_t n, double theta, const char *p) {
        if (t.n != n) bh_alloc(ctx, t, n, p);
        bh_build(ctx, t, dY, theta, nullptr, false);
        t.mom_deferred = false;
    }
    static Tree &tree(TransformState *s) { return s->tree; }
    static Tree &tree1(tsne_ctx *ctx) {
        if (!ctx->query_tree) ctx->query_tree = new Tree();
        return *ctx->query_tree;
    }
};

struct Oct {
    static constexpr int C = 3;
    static constexpr bool counts_pops = true;   // option transform_stats
    static constexpr const char *pre = "octx.", *pre1 = "octx1.";
    using Tree = OctTree;
    using View = X3Tree;
    using LDS = X3LDS;
    static __device__ __forceinline__ uint64_t key(const double (&q)[3], double W) {
        return morton3_key(q[0], q[1], q[2], W);
    }
    template <bool STATS>
    static __device__ __forceinline__ void walk(LDS &L, int w, int lane, const View &T, double theta, bool valid,
                                                const double (&q)[3], double (&f)[3], double &zs,
                                                int32_t *__restrict__ flag, unsigned long long &pops) {
        foreign_walk3<STATS>(L, w, lane, T, theta, valid, q, f, zs, flag, pops);
    }
    static View view(const Tree &t) { return View{t.pos, t.nodes, t.orec, t.vrec, t.meta, (int32_t)t.n}; }
    // The records whatever Options::oct_records says (they are what the walk
    // reads), no subtree moments (the walk uses none), the duplicate fix-up.
    static void build(tsne_ctx *ctx, Tree &t, const double *dY, int64_t n, double theta, const char *p) {
        if (t.n != n) oct_alloc(ctx, t, n, p, true);
        oct_build(ctx, t, dY, theta, false, true);
        dup_fix3(ctx, t, theta, p);
    }
    static Tree &tree(TransformState *s) { return s->otree; }
    static Tree &tree1(tsne_ctx *ctx) {
        if (!ctx->query_tree3) ctx->query_tree3 = new Tree();
        return *ctx->query_tree3;
    }
};

// Morton key of every query in the tree's root cell (the build's own key
// function and W); queries outside the root sort last.
template <class T>
__global__ void xq_keys(const double *__restrict__ Q, int64_t m, const double *__restrict__ Wp,
                        uint64_t *__restrict__ keys, int32_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double q[T::C];
    load_row(Q, i, q);
    keys[i] = T::key(q, *Wp);
    idx[i] = (int32_t)i;
}

// computeRepulsiveForce for foreign points: slot -> query row perm[slot].
// STATS (option transform_stats, the octree only): stats[0] += the wave's pops.
template <class T, bool STATS>
__global__ __launch_bounds__(64 * XWPB) void bhx_queries(typename T::View V, double theta,
                                                         const double *__restrict__ Q,
                                                         const int32_t *__restrict__ perm, int64_t m,
                                                         double *__restrict__ F, double *__restrict__ Z,
                                                         int32_t *__restrict__ flag,
                                                         unsigned long long *__restrict__ stats) {
    __shared__ typename T::LDS L;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int64_t slot = (int64_t)blockIdx.x * (64 * XWPB) + threadIdx.x;
    if (slot - lane >= m) return;   // the whole wave
    const bool valid = slot < m;
    const int64_t i = valid ? (int64_t)perm[slot] : 0;
    double q[T::C] = {}, f[T::C] = {}, zs = 0.0;
    if (valid) load_row(Q, i, q);
    unsigned long long pops = 0;
    T::template walk<STATS>(L, w, lane, V, theta, valid, q, f, zs, flag, pops);
    if (valid) {
        store_row(F, i, f);
        Z[i] = zs;
    }
    if (STATS && lane == 0) atomicAdd(stats, pops);
}

__device__ __forceinline__ double jmax(double a, double b) {  // java.lang.Math.max
    if (a != a) return a;
    if (b != b) return b;
    return a >= b ? a : b;
}

// updateEmbedding (TsneHelpers.scala:341-369) of one component
__device__ __forceinline__ void x_update(double g, double &y, double &u, double &gn, double min_gain, double mom,
                                         double lr) {
    gn = ((g > 0.0) == (u > 0.0)) ? jmax(gn * 0.8, min_gain) : jmax(gn + 0.2, min_gain);
    u = __dsub_rn(__dmul_rn(mom, u), __dmul_rn(__dmul_rn(lr, gn), g));
    y = __dadd_rn(u, y);
}

// Attraction over new point i's CSR row (sequential, CSR order, multiply and
// add apart), the gradient attr - rep / z_i with the point's own normaliser,
// and updateEmbedding on every component.
template <int C, bool LOSS>
__device__ __forceinline__ void point_update(int64_t i, double (&y)[C], const double (&f)[C], double zs,
                                             const double *__restrict__ Yr, const int64_t *__restrict__ row_ptr,
                                             const int32_t *__restrict__ col, const double *__restrict__ P,
                                             double *__restrict__ Y, double *__restrict__ upd,
                                             double *__restrict__ gains, double ex, double mom, double lr,
                                             double min_gain, double *__restrict__ lossq) {
    double a[C] = {}, ls = 0.0;
    const int64_t e1 = row_ptr[i + 1];
    for (int64_t e = row_ptr[i]; e < e1; ++e) {
        double d[C];
        load_row(Yr, (int64_t)col[e], d);
        const double pe = ex * P[e];
#pragma unroll
        for (int k = 0; k < C; ++k) d[k] = y[k] - d[k];
        const double q = 1.0 / (1.0 + x_d(d));
        const double s = pe * q;
#pragma unroll
        for (int k = 0; k < C; ++k) a[k] = __dadd_rn(a[k], __dmul_rn(s, d[k]));
        if (LOSS) ls = __dadd_rn(ls, __dmul_rn(pe, log(pe / (q / zs))));
    }
    double u[C], gn[C];
    load_row(upd, i, u);
    load_row(gains, i, gn);
#pragma unroll
    for (int k = 0; k < C; ++k) x_update(__dsub_rn(a[k], f[k] / zs), y[k], u[k], gn[k], min_gain, mom, lr);
    store_row(Y, i, y);
    store_row(upd, i, u);
    store_row(gains, i, gn);
    if (LOSS) lossq[i] = ls;
}

// One transform iteration of every new point: nothing crosses points, so the
// walk, the attraction over the point's CSR row (sequential, CSR order), the
// gradient attr - rep / z_i and the update are one launch.  The working set
// is read and written in place in the caller's order (slot -> row perm[slot]).
// LOSS: lossq[row] = sum_e pe ln(pe / (q_e / z_i)), pe = ex P_e.
template <class T, bool LOSS>
__global__ __launch_bounds__(64 * XWPB) void xform_step(typename T::View V, double theta,
                                                        const double *__restrict__ Yr,
                                                        const int64_t *__restrict__ row_ptr,
                                                        const int32_t *__restrict__ col, const double *__restrict__ P,
                                                        const int32_t *__restrict__ perm, int64_t m,
                                                        double *__restrict__ Y, double *__restrict__ upd,
                                                        double *__restrict__ gains, double ex, double mom, double lr,
                                                        double min_gain, double *__restrict__ lossq,
                                                        int32_t *__restrict__ flag) {
    __shared__ typename T::LDS L;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int64_t slot = (int64_t)blockIdx.x * (64 * XWPB) + threadIdx.x;
    if (slot - lane >= m) return;   // the whole wave
    const bool valid = slot < m;
    const int64_t i = valid ? (int64_t)perm[slot] : 0;
    double y[T::C] = {}, f[T::C] = {}, zs = 0.0;
    if (valid) load_row(Y, i, y);
    unsigned long long pops = 0;
    T::template walk<false>(L, w, lane, V, theta, valid, y, f, zs, flag, pops);
    if (!valid) return;
    point_update<T::C, LOSS>(i, y, f, zs, Yr, row_ptr, col, P, Y, upd, gains, ex, mom, lr, min_gain, lossq);
}

// The split form (option transform_split, an A/B of the fused launch): the
// same update from the sums a bhx_queries launch left in F and Z, one thread
// per new point in the caller's order.  The same arithmetic per point, so the
// same bits.
template <int C, bool LOSS>
__global__ __launch_bounds__(256) void xform_update(const double *__restrict__ F, const double *__restrict__ Z,
                                                    const double *__restrict__ Yr,
                                                    const int64_t *__restrict__ row_ptr,
                                                    const int32_t *__restrict__ col, const double *__restrict__ P,
                                                    int64_t m, double *__restrict__ Y, double *__restrict__ upd,
                                                    double *__restrict__ gains, double ex, double mom, double lr,
                                                    double min_gain, double *__restrict__ lossq) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double y[C], f[C];
    load_row(Y, i, y);
    load_row(F, i, f);
    point_update<C, LOSS>(i, y, f, Z[i], Yr, row_ptr, col, P, Y, upd, gains, ex, mom, lr, min_gain, lossq);
}

// sum of v[0..m) in a fixed order: strided per-thread sums, then a tree in LDS
__global__ __launch_bounds__(1024) void xform_loss_reduce(const double *__restrict__ v, int64_t m,
                                                          double *__restrict__ out) {
    __shared__ double sm[1024];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += 1024) s += v[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sm[0];
}

// y_i = sum_e P_e Yr[col_e]: sequential in CSR order, multiply and add apart
template <int C>
__global__ void xform_init(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                           const double *__restrict__ P, int64_t m, const double *__restrict__ Yr,
                           double *__restrict__ Y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double a[C] = {};
    const int64_t e1 = row_ptr[i + 1];
    for (int64_t e = row_ptr[i]; e < e1; ++e) {
        double yj[C];
        load_row(Yr, (int64_t)col[e], yj);
        const double p = P[e];
#pragma unroll
        for (int k = 0; k < C; ++k) a[k] = __dadd_rn(a[k], __dmul_rn(p, yj[k]));
    }
    store_row(Y, i, a);
}

// perm = the queries' rows in the order of their Morton keys in t's root cell
template <class T>
int32_t *sort_queries(tsne_ctx *ctx, const typename T::Tree &t, const double *dQ, int64_t m, const std::string &pre) {
    Workspace &ws = ctx->ws;
    hipStream_t st = ctx->stream;
    uint64_t *keys = ws.get<uint64_t>(pre + "qkeys", m), *keys2 = ws.get<uint64_t>(pre + "qkeys2", m);
    int32_t *idx = ws.get<int32_t>(pre + "qidx", m), *perm = ws.get<int32_t>(pre + "qperm", m);
    hipLaunchKernelGGL(xq_keys<T>, dim3(ceil_div(m, 256)), dim3(256), 0, st, dQ, m, t.W, keys, idx);
    size_t tb = 0;
    TSNE_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys, keys2, idx, perm, (int)m, 0, 64, st));
    void *tmp = ws.get<uint8_t>(pre + "qsort_tmp", tb);
    TSNE_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb, keys, keys2, idx, perm, (int)m, 0, 64, st));
    return perm;
}

// The flag word of the walks on the tree with workspace prefix `pre`, cleared
int32_t *walk_flag(tsne_ctx *ctx, const std::string &pre) {
    int32_t *f = ctx->ws.get<int32_t>(pre + "qflag", 1);
    TSNE_HIP(hipMemsetAsync(f, 0, sizeof(int32_t), ctx->stream));
    return f;
}

// Fails if a walk on that tree met a full stack since its flag was cleared; synchronises
void flag_check(tsne_ctx *ctx, const char *pre) {
    const std::string name = std::string(pre) + "qflag";
    if (!ctx->ws.has(name)) return;
    int32_t h = 0;
    TSNE_HIP(hipMemcpyAsync(&h, ctx->ws.get<int32_t>(name, 1), sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
    if (h) fail(TSNE_ERR_HIP, "foreign-query traversal: wave stack full");
}

// the walk alone, slot -> row perm[slot]; want_stats (a tree that counts
// pops): the waves' pops are counted into "octx1.stats" (option
// transform_stats, tsne_ctx_counter "xform3.pops")
template <class T>
void launch_queries(tsne_ctx *ctx, const typename T::Tree &t, double theta, const double *dQ, const int32_t *perm,
                    int64_t m, double *dF, double *dz, int32_t *flag, bool want_stats) {
    unsigned long long *stats = nullptr;
    if (T::counts_pops && want_stats) {
        stats = ctx->ws.get<unsigned long long>("octx1.stats", 1);
        TSNE_HIP(hipMemsetAsync(stats, 0, sizeof(unsigned long long), ctx->stream));
    }
    const auto kernel = stats ? bhx_queries<T, T::counts_pops> : bhx_queries<T, false>;
    hipLaunchKernelGGL(kernel, dim3(ceil_div(m, 64 * XWPB)), dim3(64 * XWPB), 0, ctx->stream, T::view(t), theta, dQ,
                       perm, m, dF, dz, flag, stats);
}

template <class T>
void queries_once(tsne_ctx *ctx, const double *dY, int64_t n, double theta, const double *dQ, int64_t m, double *dF,
                  double *dz) {
    typename T::Tree &t = T::tree1(ctx);
    T::build(ctx, t, dY, n, theta, T::pre1);
    int32_t *flag = walk_flag(ctx, T::pre1);
    const int32_t *perm = sort_queries<T>(ctx, t, dQ, m, T::pre1);
    launch_queries<T>(ctx, t, theta, dQ, perm, m, dF, dz, flag, ctx->opts.transform_stats != 0);
}

// the tree of s->Yref with its flag and the first sort of s->Y
template <class T>
void setup_tree(tsne_ctx *ctx, TransformState *s) {
    T::build(ctx, T::tree(s), s->Yref, s->n, s->prm.theta, T::pre);
    s->flag = walk_flag(ctx, T::pre);
    s->perm = sort_queries<T>(ctx, T::tree(s), s->Y, s->m, T::pre);
}

// The launches of one iteration: the Morton re-sort when it is due, then the
// fused step, or the walk and the update apart under transform_split.
template <class T>
void launch_iteration(tsne_ctx *ctx, TransformState *s, double ex, double mom, bool loss) {
    constexpr int C = T::C;
    const tsne_params &p = s->prm;
    hipStream_t st = ctx->stream;
    const typename T::Tree &t = T::tree(s);
    if (ctx->opts.transform_resort > 0 && s->since_sort >= ctx->opts.transform_resort) {
        s->perm = sort_queries<T>(ctx, t, s->Y, s->m, T::pre);
        s->since_sort = 0;
    }
    ++s->since_sort;
    if (ctx->opts.transform_split) {   // A/B: the walk and the update as two launches (the same bits)
        double *F = ctx->ws.get<double>(std::string(T::pre) + "splitF", C * (size_t)s->m);
        double *Z = ctx->ws.get<double>(std::string(T::pre) + "splitZ", s->m);
        launch_queries<T>(ctx, t, p.theta, s->Y, s->perm, s->m, F, Z, s->flag, false);
        const auto update = loss ? xform_update<C, true> : xform_update<C, false>;
        hipLaunchKernelGGL(update, dim3(ceil_div(s->m, 256)), dim3(256), 0, st, F, Z, s->Yref, s->row_ptr, s->col, s->P,
                           s->m, s->Y, s->upd, s->gains, ex, mom, p.learning_rate, p.min_gain, s->lossq);
    } else {
        const auto step = loss ? xform_step<T, true> : xform_step<T, false>;
        hipLaunchKernelGGL(step, dim3(ceil_div(s->m, 64 * XWPB)), dim3(64 * XWPB), 0, st, T::view(t), p.theta, s->Yref,
                           s->row_ptr, s->col, s->P, s->perm, s->m, s->Y, s->upd, s->gains, ex, mom, p.learning_rate,
                           p.min_gain, s->lossq, s->flag);
    }
}

}  // namespace

void walk_flag_check(tsne_ctx *ctx, int32_t c) { flag_check(ctx, c == 3 ? Oct::pre1 : Quad::pre1); }

void repulsion_queries_device(tsne_ctx *ctx, const double *dY, int64_t n, int32_t c, double theta, const double *dQ,
                              int64_t m, double *dF, double *dz) {
    TSNE_REQUIRE(n >= 1, "empty embedding");
    TSNE_REQUIRE(m >= 0, "negative query count");
    TSNE_REQUIRE(n < (int64_t)INT32_MAX && m < (int64_t)INT32_MAX, "n and m must fit int32 ids");
    if (m == 0) return;
    if (c == 3) queries_once<Oct>(ctx, dY, n, theta, dQ, m, dF, dz);
    else queries_once<Quad>(ctx, dY, n, theta, dQ, m, dF, dz);
    TSNE_LAUNCH_CHECK();
}

void transform_init_device(tsne_ctx *ctx, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_P,
                           int64_t m, const double *d_Yref, int64_t n, int32_t c, double *d_Y) {
    TSNE_REQUIRE(m >= 0 && n >= 1, "bad sizes");
    if (m == 0) return;
    const auto init = c == 3 ? xform_init<3> : xform_init<2>;
    hipLaunchKernelGGL(init, dim3(ceil_div(m, 256)), dim3(256), 0, ctx->stream, d_row_ptr, d_col, d_P, m, d_Yref, d_Y);
    TSNE_LAUNCH_CHECK();
}

int32_t transform_dim(const tsne_params *p, bool allow3) {
    TSNE_REQUIRE(p != nullptr, "params is NULL");
    if (!allow3 && p->n_components != 2)
        fail(TSNE_ERR_UNSUPPORTED, "the transform is 2-D only (n_components must be 2)");
    if (p->n_components != 2 && p->n_components != 3)
        fail(TSNE_ERR_UNSUPPORTED, "the transform is 2-D or 3-D (n_components must be 2 or 3)");
    return p->n_components;
}

void transform_setup(tsne_ctx *ctx, const tsne_params *p, const double *d_Yref, int64_t n,
                     const int64_t *d_row_ptr, const int32_t *d_col, const double *d_P, int64_t m, double *d_Y,
                     double *d_upd, double *d_gains, bool allow3) {
    const int32_t c = transform_dim(p, allow3);
    TSNE_REQUIRE(m >= 0 && n >= 1, "bad sizes");
    TSNE_REQUIRE(n < (int64_t)INT32_MAX && m < (int64_t)INT32_MAX, "n and m must fit int32 ids");
    TSNE_REQUIRE(p->iterations >= 0, "negative iteration count");
    if (!ctx->xform) ctx->xform = new TransformState();
    TransformState *s = ctx->xform;
    s->prm = *p;
    s->dim = c;
    s->n = n;
    s->m = m;
    s->loss_keys.clear();
    if (m == 0) return;
    TSNE_REQUIRE(d_Yref && d_row_ptr && d_col && d_P && d_Y && d_upd && d_gains, "NULL buffer");
    s->Yref = d_Yref; s->row_ptr = d_row_ptr; s->col = d_col; s->P = d_P;
    s->Y = d_Y; s->upd = d_upd; s->gains = d_gains;
    if (c == 3) setup_tree<Oct>(ctx, s);
    else setup_tree<Quad>(ctx, s);
    s->since_sort = 0;
    const std::string pre = c == 3 ? Oct::pre : Quad::pre;
    s->lossq = ctx->ws.get<double>(pre + "lossq", m);
    s->loss_cap = p->iterations / 10 + 1;
    s->loss_d = ctx->ws.get<double>(pre + "loss", s->loss_cap);
}

void transform_step(tsne_ctx *ctx, int32_t t) {
    TransformState *s = ctx->xform;
    TSNE_REQUIRE(s != nullptr, "tsne_dev_transform_setup was not called");
    if (s->m == 0) return;
    const tsne_params &p = s->prm;
    // the reference phase schedule (TsneHelpers.scala:396-430)
    const int32_t n1 = std::min(p.iterations, 20), n2 = std::min(p.iterations - n1, 81);
    const double ex = t <= n1 + n2 ? p.early_exaggeration : 1.0;
    const double mom = t <= n1 ? p.initial_momentum : p.final_momentum;
    const bool loss = t % 10 == 0 && (int32_t)s->loss_keys.size() < s->loss_cap;
    if (s->dim == 3) launch_iteration<Oct>(ctx, s, ex, mom, loss);
    else launch_iteration<Quad>(ctx, s, ex, mom, loss);
    if (loss) {
        hipLaunchKernelGGL(xform_loss_reduce, dim3(1), dim3(1024), 0, ctx->stream, s->lossq, s->m,
                           s->loss_d + s->loss_keys.size());
        s->loss_keys.push_back(t);
    }
    TSNE_LAUNCH_CHECK();
}

void transform_sync(tsne_ctx *ctx) {
    TransformState *s = ctx->xform;
    TSNE_REQUIRE(s != nullptr, "tsne_dev_transform_setup was not called");
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
    if (s->m) flag_check(ctx, s->dim == 3 ? Oct::pre : Quad::pre);
}

int32_t transform_losses(tsne_ctx *ctx, int32_t *keys, double *vals, int32_t cap) {
    TransformState *s = ctx->xform;
    TSNE_REQUIRE(s != nullptr, "tsne_dev_transform_setup was not called");
    const int32_t k = (int32_t)s->loss_keys.size(), c = std::min(k, std::max(cap, 0));
    if (c > 0) {
        TSNE_REQUIRE(keys && vals, "NULL loss buffer");
        TSNE_HIP(hipMemcpyAsync(vals, s->loss_d, sizeof(double) * c, hipMemcpyDeviceToHost, ctx->stream));
        std::copy(s->loss_keys.begin(), s->loss_keys.begin() + c, keys);
    }
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
    return k;
}

int64_t transform_pops(tsne_ctx *ctx) {
    if (!ctx->ws.has("octx1.stats")) return 0;
    unsigned long long h = 0;
    TSNE_HIP(hipMemcpyAsync(&h, ctx->ws.get<unsigned long long>("octx1.stats", 1), sizeof(h), hipMemcpyDeviceToHost,
                            ctx->stream));
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
    return (int64_t)h;
}

void transform_destroy(tsne_ctx *ctx) {
    delete ctx->xform;
    ctx->xform = nullptr;
    delete ctx->query_tree;
    ctx->query_tree = nullptr;
    delete ctx->query_tree3;
    ctx->query_tree3 = nullptr;
}

}  // namespace tsne
