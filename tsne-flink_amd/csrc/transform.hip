// transform.hip -- embedding new points into a fitted map on gfx950.
//
// The reference map Yr is fixed: its quadtree (bhtree.hip, the records of
// bh_build) is built once, and new points are QUERIES that are not in the
// tree.  The records already mean the right thing for such a query: a leaf
// contributes 0 when its point equals the query (by position, QK_LEAF /
// QK_MULTI), every cell is summarised when the reference's h / D < theta says
// so (QuadTree.scala:134).  This file holds
//   * foreign_walk: the traversal for foreign queries, 64 per wave;
//   * bhx_queries:  computeRepulsiveForce for a batch of foreign points;
//   * xform_step:   one transform iteration for every new point in one
//                   launch -- walk, attraction over the point's CSR row,
//                   gradient with the point's own normaliser z_i, update;
//   * the host side: the query sort, the tree kept in the context, the loss.
// A 3-D map takes the same walk over the octree's records (transform3.hip);
// the host side here dispatches on the state's dimension.
//
// Canonical order.  A wave's 64 queries share one LDS stack of (record, lane
// mask) entries.  The stack is strictly LIFO, one record per pop, and an
// opened cell's children are pushed in slot order 0..3, each with the mask
// of the lanes that open it.  The sequence of pops is therefore the
// depth-first order of the TREE restricted to the records some lane opens;
// the pops a given lane takes part in are the depth-first order of the
// records that lane opens, whatever the other lanes do.  A lane adds its
// terms (children 0..3 of every record it is active for) in that order and a
// masked-out lane adds nothing -- not a zero product, which would turn -0.0
// into +0.0 and spread a NaN.  So a query's sums are a function of the tree
// and the query alone: bit-identical in any batch, in any lane, under any
// sort of the queries.  The Morton sort of the queries only makes the lanes
// of a wave open the same records (fewer pops per wave).
//
// No subtree moments, no all-open tiles and no near-exact shortcut are used
// here: every decision is the reference's, from the record's sure-accept /
// sure-open bounds on 1 + D (QACC_BAND, bhtree.hpp) and the exact IEEE
// quotient in between.
#include <algorithm>

#include <hipcub/hipcub.hpp>

#include "transform.hpp"

namespace tsne {
namespace {

constexpr int XWPB = 4;       // waves per workgroup
// Stack entries per wave: a pop takes one entry and pushes <= 4, and the
// entries of one level are consumed before their parent's siblings, so the
// depth is <= 3 per level + 1 over the 31 quad levels, the root and the
// virtual chain tops of duplicate groups: < 128.  A full stack sets flag[0]
// and drops the push (never expected; the host entry points report it).
constexpr int XSTACK = 128;
constexpr int QREC_V4 = sizeof(QRec) / 16;

// 7 KB per workgroup: the record of the current pop and the stack, per wave
struct XLDS {
    QRec rec[XWPB];
    uint64_t smask[XWPB][XSTACK];
    int32_t sref[XWPB][XSTACK];
};

struct XTree {
    const double2 *pos;
    const BHNode *nodes;
    const QRec *qrec;
    const int32_t *meta;   // [0] in-root points, [1] root ref, [3] root replaced by its virtual chain top
    int32_t virt;          // record index offset of the virtual chain tops (= n)
};

// 1/x as the tree's own traversal forms it (bhtree.hip recip_bh): v_rcp_f64 and
// one Newton step, within 11 ulp of the IEEE quotient.
__device__ __forceinline__ double x_recip(double x) {
    const double r = __builtin_amdgcn_rcp(x);
    return __fma_rn(r, __fma_rn(-x, r, 1.0), r);
}

// cnt points at their centre of mass (QuadTree.scala:134-142): D1 = 1 + D
__device__ __forceinline__ void x_term(double dx, double dy, double D1, double cnt, double &fx, double &fy,
                                       double &zs) {
    const double Q = x_recip(D1);
    const double mult = cnt * Q;
    const double sc = mult * Q;
    fx = __fma_rn(sc, dx, fx);
    fy = __fma_rn(sc, dy, fy);
    zs += mult;
}

// one point; nothing if it is the query's own position (QuadTree.scala:128)
__device__ __forceinline__ void x_leaf(double qx, double qy, double2 p, double &fx, double &fy, double &zs) {
    if (p.x == qx && p.y == qy) return;
    const double dx = qx - p.x, dy = qy - p.y;
    x_term(dx, dy, __fma_rn(dx, dx, __fma_rn(dy, dy, 1.0)), 1.0, fx, fy, zs);
}

// The walk of one wave: lane's query (qx, qy) if `valid`.  See "Canonical
// order" above.  All control flow is wave-uniform; `valid` / the entries'
// masks predicate the lanes' terms.
__device__ __forceinline__ void foreign_walk(XLDS &L, int w, int lane, const XTree &T, double theta, bool valid,
                                             double qx, double qy, double &fx, double &fy, double &zs,
                                             int32_t *__restrict__ flag) {
    int sp = 0;
    // the root: a single point, a key-tie group, or a cell tested like any other
    const int root = T.meta[1];
    if (root == ~0) {
        if (valid) x_leaf(qx, qy, T.pos[0], fx, fy, zs);
        return;
    }
    if (root < 0) return;   // no point in the root cell
    {
        const BHNode &rt = T.nodes[root];
        if (rt.delta >= 62) {
            for (int p = rt.first; p <= rt.last; ++p) {
                const double2 pp = T.pos[p];
                if (valid) x_leaf(qx, qy, pp, fx, fy, zs);
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
            const double dx = qx - rcx, dy = qy - rcy;
            const double D = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
            if (rh / D < theta) x_term(dx, dy, 1.0 + D, (double)rcnt, fx, fy, zs);
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
        __builtin_amdgcn_wave_barrier();
        const int ref = __builtin_amdgcn_readfirstlane(L.sref[w][sp]);
        const uint64_t mv = L.smask[w][sp];
        const uint64_t msk = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(mv >> 32)) << 32) |
                             (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)mv);
        // the record, once per pop: 16 lanes x 16 bytes into LDS, read back as broadcasts
        if (lane < QREC_V4)
            reinterpret_cast<uint4 *>(&L.rec[w])[lane] = reinterpret_cast<const uint4 *>(T.qrec + ref)[lane];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        const QRec &nd = L.rec[w];
        const bool act = (msk >> lane) & 1ull;
        const int nflags = __builtin_amdgcn_readfirstlane(nd.nch);
        const int nch = nflags & 0xff;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c >= nch) break;
            const int kind = (nflags >> (QNCH_KIND + 2 * c)) & 3;   // wave-uniform
            const double dx = qx - nd.ccx[c], dy = qy - nd.ccy[c];
            if (kind == QK_LEAF) {
                if (act && !(dx == 0.0 && dy == 0.0))
                    x_term(dx, dy, __fma_rn(dx, dx, __fma_rn(dy, dy, 1.0)), 1.0, fx, fy, zs);
            } else if (kind == QK_CELL) {
                const double D1 = __fma_rn(dx, dx, __fma_rn(dy, dy, 1.0));   // 1 + D
                bool acc = false;
                if (act) {
                    if (D1 > nd.ca[c]) acc = true;
                    else if (D1 < nd.cb[c]) acc = false;
                    else {   // the band: the reference's own quotient decides
                        const int32_t cref = nd.cref[c];
                        const double ch = cref < T.virt ? T.nodes[cref].h : 0.5 * T.nodes[ref].h;
                        acc = ch / __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)) < theta;
                    }
                }
                if (act && acc) x_term(dx, dy, D1, (double)nd.ccnt[c], fx, fy, zs);
                const uint64_t om = __ballot(act && !acc);
                if (om) {
                    if (sp < XSTACK) {
                        if (lane == 0) { L.sref[w][sp] = nd.cref[c]; L.smask[w][sp] = om; }
                        ++sp;
                    } else if (lane == 0) {
                        atomicOr(flag, 1);
                    }
                }
            } else if (kind == QK_MULTI) {   // a leaf of ccnt copies: 0 if it is the query's position
                if (act && !(nd.ccx[c] == qx && nd.ccy[c] == qy))
                    x_term(dx, dy, __fma_rn(dx, dx, __fma_rn(dy, dy, 1.0)), (double)nd.ccnt[c], fx, fy, zs);
            } else {                         // a key-tie group: every point directly
                const BHNode &tn = T.nodes[__builtin_amdgcn_readfirstlane(nd.cref[c])];
                const int p0 = __builtin_amdgcn_readfirstlane(tn.first), p1 = __builtin_amdgcn_readfirstlane(tn.last);
                for (int p = p0; p <= p1; ++p) {
                    const double2 pp = T.pos[p];
                    if (act) x_leaf(qx, qy, pp, fx, fy, zs);
                }
            }
        }
    }
}

// Morton key of every query in the tree's root cell (the build's own key
// function and W); queries outside the root sort last.
__global__ void xq_keys(const double2 *__restrict__ Q, int64_t m, const double *__restrict__ Wp,
                        uint64_t *__restrict__ keys, int32_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double2 q = Q[i];
    keys[i] = morton2_key(q.x, q.y, *Wp);
    idx[i] = (int32_t)i;
}

// computeRepulsiveForce for foreign points: slot -> query row perm[slot]
__global__ __launch_bounds__(64 * XWPB) void bhx_queries(XTree T, double theta, const double2 *__restrict__ Q,
                                                         const int32_t *__restrict__ perm, int64_t m,
                                                         double2 *__restrict__ F, double *__restrict__ Z,
                                                         int32_t *__restrict__ flag) {
    __shared__ XLDS L;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int64_t slot = (int64_t)blockIdx.x * (64 * XWPB) + threadIdx.x;
    if (slot - lane >= m) return;   // the whole wave
    const bool valid = slot < m;
    const int64_t i = valid ? (int64_t)perm[slot] : 0;
    double qx = 0.0, qy = 0.0;
    if (valid) { const double2 q = Q[i]; qx = q.x; qy = q.y; }
    double fx = 0.0, fy = 0.0, zs = 0.0;
    foreign_walk(L, w, lane, T, theta, valid, qx, qy, fx, fy, zs, flag);
    if (valid) {
        F[i] = make_double2(fx, fy);
        Z[i] = zs;
    }
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

// Attraction over new point i's CSR row (sequential, CSR order), the gradient
// attr - rep / z_i with the point's own normaliser, and updateEmbedding.
template <bool LOSS>
__device__ __forceinline__ void point_update(int64_t i, double2 y, double fx, double fy, double zs,
                                             const double2 *__restrict__ Yr, const int64_t *__restrict__ row_ptr,
                                             const int32_t *__restrict__ col, const double *__restrict__ P,
                                             double2 *__restrict__ Y, double2 *__restrict__ upd,
                                             double2 *__restrict__ gains, double ex, double mom, double lr,
                                             double min_gain, double *__restrict__ lossq) {
    double ax = 0.0, ay = 0.0, ls = 0.0;
    const int64_t e1 = row_ptr[i + 1];
    for (int64_t e = row_ptr[i]; e < e1; ++e) {
        const double2 yj = Yr[col[e]];
        const double pe = ex * P[e];
        const double dx = y.x - yj.x, dy = y.y - yj.y;
        const double q = 1.0 / (1.0 + __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
        const double s = pe * q;
        ax = __dadd_rn(ax, __dmul_rn(s, dx));
        ay = __dadd_rn(ay, __dmul_rn(s, dy));
        if (LOSS) ls = __dadd_rn(ls, __dmul_rn(pe, log(pe / (q / zs))));
    }
    const double gx = __dsub_rn(ax, fx / zs), gy = __dsub_rn(ay, fy / zs);
    double2 u = upd[i], gn = gains[i];
    x_update(gx, y.x, u.x, gn.x, min_gain, mom, lr);
    x_update(gy, y.y, u.y, gn.y, min_gain, mom, lr);
    Y[i] = y;
    upd[i] = u;
    gains[i] = gn;
    if (LOSS) lossq[i] = ls;
}

// One transform iteration of every new point: nothing crosses points, so the
// walk, the attraction over the point's CSR row (sequential, CSR order), the
// gradient attr - rep / z_i and the update are one launch.  The working set
// is read and written in place in the caller's order (slot -> row perm[slot]).
// LOSS: lossq[row] = sum_e pe ln(pe / (q_e / z_i)), pe = ex P_e.
template <bool LOSS>
__global__ __launch_bounds__(64 * XWPB) void xform_step(XTree T, double theta, const double2 *__restrict__ Yr,
                                                        const int64_t *__restrict__ row_ptr,
                                                        const int32_t *__restrict__ col, const double *__restrict__ P,
                                                        const int32_t *__restrict__ perm, int64_t m,
                                                        double2 *__restrict__ Y, double2 *__restrict__ upd,
                                                        double2 *__restrict__ gains, double ex, double mom, double lr,
                                                        double min_gain, double *__restrict__ lossq,
                                                        int32_t *__restrict__ flag) {
    __shared__ XLDS L;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int64_t slot = (int64_t)blockIdx.x * (64 * XWPB) + threadIdx.x;
    if (slot - lane >= m) return;   // the whole wave
    const bool valid = slot < m;
    const int64_t i = valid ? (int64_t)perm[slot] : 0;
    double2 y = make_double2(0.0, 0.0);
    if (valid) y = Y[i];
    double fx = 0.0, fy = 0.0, zs = 0.0;
    foreign_walk(L, w, lane, T, theta, valid, y.x, y.y, fx, fy, zs, flag);
    if (!valid) return;
    point_update<LOSS>(i, y, fx, fy, zs, Yr, row_ptr, col, P, Y, upd, gains, ex, mom, lr, min_gain, lossq);
}

// The split form (option transform_split, an A/B of the fused launch): the
// same update from the sums a bhx_queries launch left in F and Z, one thread
// per new point in the caller's order.  The same arithmetic per point, so the
// same bits.
template <bool LOSS>
__global__ __launch_bounds__(256) void xform_update(const double2 *__restrict__ F, const double *__restrict__ Z,
                                                    const double2 *__restrict__ Yr,
                                                    const int64_t *__restrict__ row_ptr,
                                                    const int32_t *__restrict__ col, const double *__restrict__ P,
                                                    int64_t m, double2 *__restrict__ Y, double2 *__restrict__ upd,
                                                    double2 *__restrict__ gains, double ex, double mom, double lr,
                                                    double min_gain, double *__restrict__ lossq) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double2 f = F[i];
    point_update<LOSS>(i, Y[i], f.x, f.y, Z[i], Yr, row_ptr, col, P, Y, upd, gains, ex, mom, lr, min_gain, lossq);
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
__global__ void xform_init(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                           const double *__restrict__ P, int64_t m, const double2 *__restrict__ Yr,
                           double2 *__restrict__ Y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double ax = 0.0, ay = 0.0;
    const int64_t e1 = row_ptr[i + 1];
    for (int64_t e = row_ptr[i]; e < e1; ++e) {
        const double2 yj = Yr[col[e]];
        const double p = P[e];
        ax = __dadd_rn(ax, __dmul_rn(p, yj.x));
        ay = __dadd_rn(ay, __dmul_rn(p, yj.y));
    }
    Y[i] = make_double2(ax, ay);
}

XTree tree_view(const BHTree &t) { return XTree{t.pos, t.nodes, t.qrec, t.meta, (int32_t)t.n}; }

// Build the reference map's tree for foreign queries: the full build (no
// root-tile shortcut: its records are what the walk reads).  The walk uses no
// subtree moments, so the ones the fused build defers to the traversal call
// are not run at all.
void build_tree(tsne_ctx *ctx, BHTree &t, const double *dY, int64_t n, double theta, const char *pre) {
    if (t.n != n) bh_alloc(ctx, t, n, pre);
    bh_build(ctx, t, dY, theta, nullptr, false);
    t.mom_deferred = false;
}

// perm = the queries' rows in the order of their Morton keys in t's root cell
int32_t *sort_queries(tsne_ctx *ctx, const BHTree &t, const double *dQ, int64_t m, const std::string &pre) {
    Workspace &ws = ctx->ws;
    hipStream_t st = ctx->stream;
    uint64_t *keys = ws.get<uint64_t>(pre + "qkeys", m), *keys2 = ws.get<uint64_t>(pre + "qkeys2", m);
    int32_t *idx = ws.get<int32_t>(pre + "qidx", m), *perm = ws.get<int32_t>(pre + "qperm", m);
    hipLaunchKernelGGL(xq_keys, dim3(ceil_div(m, 256)), dim3(256), 0, st, reinterpret_cast<const double2 *>(dQ), m,
                       t.W, keys, idx);
    size_t tb = 0;
    TSNE_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys, keys2, idx, perm, (int)m, 0, 64, st));
    void *tmp = ws.get<uint8_t>(pre + "qsort_tmp", tb);
    TSNE_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb, keys, keys2, idx, perm, (int)m, 0, 64, st));
    return perm;
}

}  // namespace

int32_t *walk_flag(tsne_ctx *ctx, const std::string &pre) {
    int32_t *f = ctx->ws.get<int32_t>(pre + "qflag", 1);
    TSNE_HIP(hipMemsetAsync(f, 0, sizeof(int32_t), ctx->stream));
    return f;
}

void walk_flag_check(tsne_ctx *ctx, const char *pre) {
    const std::string name = std::string(pre) + "qflag";
    if (!ctx->ws.has(name)) return;
    int32_t h = 0;
    TSNE_HIP(hipMemcpyAsync(&h, ctx->ws.get<int32_t>(name, 1), sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
    if (h) fail(TSNE_ERR_HIP, "foreign-query traversal: wave stack full");
}

void repulsion_queries_device(tsne_ctx *ctx, const double *dY, int64_t n, double theta, const double *dQ, int64_t m,
                              double *dF, double *dz) {
    TSNE_REQUIRE(n >= 1, "empty embedding");
    TSNE_REQUIRE(m >= 0, "negative query count");
    TSNE_REQUIRE(n < (int64_t)INT32_MAX && m < (int64_t)INT32_MAX, "n and m must fit int32 ids");
    if (m == 0) return;
    if (!ctx->query_tree) ctx->query_tree = new BHTree();
    BHTree &t = *ctx->query_tree;
    build_tree(ctx, t, dY, n, theta, "bhx1.");
    int32_t *flag = walk_flag(ctx, "bhx1.");
    const int32_t *perm = sort_queries(ctx, t, dQ, m, "bhx1.");
    hipLaunchKernelGGL(bhx_queries, dim3(ceil_div(m, 64 * XWPB)), dim3(64 * XWPB), 0, ctx->stream, tree_view(t), theta,
                       reinterpret_cast<const double2 *>(dQ), perm, m, reinterpret_cast<double2 *>(dF), dz, flag);
    TSNE_LAUNCH_CHECK();
}

void transform_init_device(tsne_ctx *ctx, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_P,
                           int64_t m, const double *d_Yref, int64_t n, double *d_Y) {
    TSNE_REQUIRE(m >= 0 && n >= 1, "bad sizes");
    if (m == 0) return;
    hipLaunchKernelGGL(xform_init, dim3(ceil_div(m, 256)), dim3(256), 0, ctx->stream, d_row_ptr, d_col, d_P, m,
                       reinterpret_cast<const double2 *>(d_Yref), reinterpret_cast<double2 *>(d_Y));
    TSNE_LAUNCH_CHECK();
}

void transform_setup(tsne_ctx *ctx, const tsne_params *p, const double *d_Yref, int64_t n,
                     const int64_t *d_row_ptr, const int32_t *d_col, const double *d_P, int64_t m, double *d_Y,
                     double *d_upd, double *d_gains, bool allow3) {
    TSNE_REQUIRE(p != nullptr, "params is NULL");
    if (!allow3 && p->n_components != 2)
        fail(TSNE_ERR_UNSUPPORTED, "the transform is 2-D only (n_components must be 2)");
    if (p->n_components != 2 && p->n_components != 3)
        fail(TSNE_ERR_UNSUPPORTED, "the transform is 2-D or 3-D (n_components must be 2 or 3)");
    TSNE_REQUIRE(m >= 0 && n >= 1, "bad sizes");
    TSNE_REQUIRE(n < (int64_t)INT32_MAX && m < (int64_t)INT32_MAX, "n and m must fit int32 ids");
    TSNE_REQUIRE(p->iterations >= 0, "negative iteration count");
    if (!ctx->xform) ctx->xform = new TransformState();
    TransformState *s = ctx->xform;
    s->prm = *p;
    s->dim = p->n_components;
    s->n = n;
    s->m = m;
    s->loss_keys.clear();
    if (m == 0) return;
    TSNE_REQUIRE(d_Yref && d_row_ptr && d_col && d_P && d_Y && d_upd && d_gains, "NULL buffer");
    s->Yref = d_Yref; s->row_ptr = d_row_ptr; s->col = d_col; s->P = d_P;
    s->Y = d_Y; s->upd = d_upd; s->gains = d_gains;
    if (s->dim == 3) {
        transform3_build(ctx, s);
    } else {
        build_tree(ctx, s->tree, d_Yref, n, p->theta, "bhx.");
        s->flag = walk_flag(ctx, "bhx.");
        s->perm = sort_queries(ctx, s->tree, d_Y, m, "bhx.");
    }
    s->since_sort = 0;
    const std::string pre = s->dim == 3 ? "octx." : "bhx.";
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
    if (ctx->opts.transform_resort > 0 && s->since_sort >= ctx->opts.transform_resort) {
        if (s->dim == 3) transform3_sort(ctx, s);
        else s->perm = sort_queries(ctx, s->tree, s->Y, s->m, "bhx.");
        s->since_sort = 0;
    }
    ++s->since_sort;
    hipStream_t st = ctx->stream;
    if (s->dim == 3) {   // the octree walk and the three-component update (transform3.hip)
        transform3_launch(ctx, s, ex, mom, loss);
        if (loss) {
            hipLaunchKernelGGL(xform_loss_reduce, dim3(1), dim3(1024), 0, st, s->lossq, s->m,
                               s->loss_d + s->loss_keys.size());
            s->loss_keys.push_back(t);
        }
        TSNE_LAUNCH_CHECK();
        return;
    }
    const dim3 grid(ceil_div(s->m, 64 * XWPB)), block(64 * XWPB);
    const XTree T = tree_view(s->tree);
    const auto Yr = reinterpret_cast<const double2 *>(s->Yref);
    const auto Y = reinterpret_cast<double2 *>(s->Y), U = reinterpret_cast<double2 *>(s->upd),
               G = reinterpret_cast<double2 *>(s->gains);
    if (ctx->opts.transform_split) {   // A/B: the walk and the update as two launches (the same bits)
        double2 *F = ctx->ws.get<double2>("bhx.splitF", s->m);
        double *Z = ctx->ws.get<double>("bhx.splitZ", s->m);
        hipLaunchKernelGGL(bhx_queries, grid, block, 0, st, T, p.theta, Y, s->perm, s->m, F, Z, s->flag);
        const dim3 ug(ceil_div(s->m, 256)), ub(256);
        if (loss)
            hipLaunchKernelGGL(xform_update<true>, ug, ub, 0, st, F, Z, Yr, s->row_ptr, s->col, s->P, s->m, Y, U, G, ex,
                               mom, p.learning_rate, p.min_gain, s->lossq);
        else
            hipLaunchKernelGGL(xform_update<false>, ug, ub, 0, st, F, Z, Yr, s->row_ptr, s->col, s->P, s->m, Y, U, G,
                               ex, mom, p.learning_rate, p.min_gain, s->lossq);
    } else if (loss) {
        hipLaunchKernelGGL(xform_step<true>, grid, block, 0, st, T, p.theta, Yr, s->row_ptr, s->col, s->P, s->perm, s->m,
                           Y, U, G, ex, mom, p.learning_rate, p.min_gain, s->lossq, s->flag);
    } else {
        hipLaunchKernelGGL(xform_step<false>, grid, block, 0, st, T, p.theta, Yr, s->row_ptr, s->col, s->P, s->perm,
                           s->m, Y, U, G, ex, mom, p.learning_rate, p.min_gain, s->lossq, s->flag);
    }
    if (loss) {
        hipLaunchKernelGGL(xform_loss_reduce, dim3(1), dim3(1024), 0, st, s->lossq, s->m,
                           s->loss_d + s->loss_keys.size());
        s->loss_keys.push_back(t);
    }
    TSNE_LAUNCH_CHECK();
}

void transform_sync(tsne_ctx *ctx) {
    TransformState *s = ctx->xform;
    TSNE_REQUIRE(s != nullptr, "tsne_dev_transform_setup was not called");
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
    if (s->m) walk_flag_check(ctx, s->dim == 3 ? "octx." : "bhx.");
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

void transform_destroy(tsne_ctx *ctx) {
    delete ctx->xform;
    ctx->xform = nullptr;
    delete ctx->query_tree;
    ctx->query_tree = nullptr;
    delete ctx->query_tree3;
    ctx->query_tree3 = nullptr;
}

}  // namespace tsne
