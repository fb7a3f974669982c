// bhtree_build.hip -- the Barnes-Hut quadtree up to a finished tree (TsneHelpers.scala:227-264,
// QuadTree.scala:38-152, Cell.scala:31-36) on gfx950; bhtree.hip evaluates it.
//
// Equivalence with the reference pointer quadtree (capacity 1, root
// Cell(0, 0, W) with W = max(dX, dY)):
//  * a point's Morton digits are computed by replaying the reference's own
//    fp64 cell arithmetic (child centres x -/+ 0.5*hW, closed containment
//    tests tried in the order NW, NE, SW, SE), so boundary ties and the
//    rounding of non-dyadic W land in the same cell as in the reference;
//  * the reference tree only splits cells holding >= 2 distinct points.
//    Cells with a single occupied child form chains with identical
//    (count, centre of mass); because the criterion max(hW,hH)/D < theta is
//    monotone along such a chain (h halves, D fixed), summarising the chain
//    at its deepest cell gives the same contribution as the reference's
//    walk down it.  The binary radix tree (Karras) over the sorted keys has
//    exactly one node per split; nodes that split inside a quad level are
//    transparent (always opened);
//  * leaves always interact directly; a leaf equal to the query contributes
//    nothing (QuadTree.scala:128); points outside the root cell are not in
//    the tree but still get a force (they are queries).
//  * exact duplicate embedding points get the reference's multiplicities
//    (dup_* kernels below: a leaf holding c copies re-inserts ONE of them
//    when it splits, QuadTree.scala:52-61), replayed from insertion rows.
// Known deviations (documented in DESIGN.md): cells deeper than 31 levels
// are not split further (keys tie: all points interact directly; duplicate
// groups sharing such a cell with other points keep full multiplicity);
// centres of mass are summed in tree order, not insertion order.
#include <hipcub/hipcub.hpp>

#include "bhtree_impl.hpp"

namespace tsne {
namespace {

constexpr uint64_t OUT_KEY = MORTON2_OUT_KEY;      // outside the root cell: sorts last (csort.hpp: 31 levels, 62 key bits)
constexpr int MOM_CHUNK = 2048;

__global__ void bbox_partial(const double *__restrict__ Y, int64_t n, double *__restrict__ part) {
    __shared__ double sm[4][4];
    double mnx = __builtin_inf(), mxx = -__builtin_inf(), mny = __builtin_inf(), mxy = -__builtin_inf();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        double x = Y[2 * i], y = Y[2 * i + 1];
        mnx = fmin(mnx, x); mxx = fmax(mxx, x);
        mny = fmin(mny, y); mxy = fmax(mxy, y);
    }
    mnx = wave_min(mnx); mxx = wave_max(mxx); mny = wave_min(mny); mxy = wave_max(mxy);
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) { sm[w][0] = mnx; sm[w][1] = mxx; sm[w][2] = mny; sm[w][3] = mxy; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            sm[0][0] = fmin(sm[0][0], sm[k][0]); sm[0][1] = fmax(sm[0][1], sm[k][1]);
            sm[0][2] = fmin(sm[0][2], sm[k][2]); sm[0][3] = fmax(sm[0][3], sm[k][3]);
        }
        for (int k = 0; k < 4; ++k) part[blockIdx.x * 4 + k] = sm[0][k];
    }
}

// One 256-thread block folds the per-block partials.
// Thread 0 also resets the build's counters and takes the moment gate
// (moment_count): mom_flag[0] = the previous traversal saw enough tiles that
// moments would serve (mom_flag[1] >= mom_flag[2]), then mom_flag[1] restarts.
__global__ void bbox_final(const double *__restrict__ part, int nb, double *__restrict__ W,
                           int32_t *__restrict__ meta, double *__restrict__ bb, int32_t *__restrict__ mom_flag,
                           int32_t *__restrict__ mom_items, int32_t *__restrict__ dflag) {
    __shared__ double sm[4][4];
    double mnx = __builtin_inf(), mxx = -__builtin_inf(), mny = __builtin_inf(), mxy = -__builtin_inf();
    for (int b = threadIdx.x; b < nb; b += blockDim.x) {
        mnx = fmin(mnx, part[4 * b]); mxx = fmax(mxx, part[4 * b + 1]);
        mny = fmin(mny, part[4 * b + 2]); mxy = fmax(mxy, part[4 * b + 3]);
    }
    mnx = wave_min(mnx); mxx = wave_max(mxx); mny = wave_min(mny); mxy = wave_max(mxy);
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) { sm[w][0] = mnx; sm[w][1] = mxx; sm[w][2] = mny; sm[w][3] = mxy; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            sm[0][0] = fmin(sm[0][0], sm[k][0]); sm[0][1] = fmax(sm[0][1], sm[k][1]);
            sm[0][2] = fmin(sm[0][2], sm[k][2]); sm[0][3] = fmax(sm[0][3], sm[k][3]);
        }
        const double a = sm[0][1] - sm[0][0], c = sm[0][3] - sm[0][2];
        *W = a > c ? a : c;  // scala.math.max(maxX - minX, maxY - minY)
        for (int k = 0; k < 4; ++k) bb[k] = sm[0][k];
        meta[0] = 0;
        meta[2] = 0;
        meta[3] = 0;         // root replaced by its virtual chain top (duplicates, dup_apply)
        if (mom_flag) {
            mom_flag[0] = mom_flag[1] >= mom_flag[2];
            mom_flag[1] = 0;
        }
        if (mom_items) *mom_items = 0;
        if (dflag) *dflag = 0;   // (Options::build_fuse: the build's duplicate flag cleared here, not by a fill)
    }
}

// (the Morton key itself: morton2_key, csort.hpp -- shared with the fused sort front end)
__global__ void morton_keys(const double *__restrict__ Y, int64_t n, const double *__restrict__ Wp,
                            uint64_t *__restrict__ keys, int32_t *__restrict__ idx,
                            int32_t *__restrict__ meta) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i0 < n;
    const int64_t i = live ? i0 : n - 1;
    const double W = *Wp;
    const uint64_t key = live ? morton2_key(Y[2 * i], Y[2 * i + 1], W) : MORTON2_OUT_KEY;
    if (live) {
        keys[i] = key;
        idx[i] = (int32_t)i;
    }
    (void)meta;   // the in-root count m is read off the sorted keys (count_in_root)
}

// m = number of in-root points = index of the first OUT_KEY in the sorted
// keys: a 64-ary search by one wave (4 rounds of one load per lane at 1M),
// instead of an atomic per wave on one counter (serialised in the L2).
__global__ void count_in_root(const uint64_t *__restrict__ ks, int64_t n, int32_t *__restrict__ meta) {
    const int lane = lane_id();
    int64_t lo = 0, hi = n;   // answer in [lo, hi]
    while (hi > lo) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t p = lo + (int64_t)lane * step;   // probe: is ks[p] an out-of-root key?
        const bool out = p < hi && ks[p] >= OUT_KEY;
        const uint64_t b = __ballot(out || p >= hi);
        const int f = b ? __ffsll((long long)b) - 1 : 64;   // first lane whose probe is out (or past hi)
        // first out-of-root index lies in (lo + (f-1) step, lo + f step]
        const int64_t nlo = f == 0 ? lo : lo + (int64_t)(f - 1) * step + 1;
        const int64_t nhi = min(hi, lo + (int64_t)f * step);
        if (f == 0) { hi = lo; break; }
        lo = nlo;
        hi = nhi;
    }
    if (lane == 0) {
        meta[0] = (int32_t)lo;
        meta[1] = lo >= 2 ? 0 : (lo == 1 ? ~0 : INT32_MIN);   // the root ref
    }
}

__global__ void gather_sorted(const double *__restrict__ Y, const int32_t *__restrict__ idx_sorted,
                              int64_t n, double2 *__restrict__ pos, int32_t *__restrict__ inv,
                              const int32_t *__restrict__ pcost, int32_t *__restrict__ pred) {
    int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // (option trav_front_cur: each new 64-query wave's predicted cost, the
    // largest previous cost of its points -- lanes = the wave's queries)
    if (pred) {
        const int32_t c = s < n ? pcost[idx_sorted[s]] : 0;
        const int32_t m = wave_max(c);
        if (lane_id() == 0 && s < n) pred[s >> 6] = m;
    }
    if (s >= n) return;
    int32_t i = idx_sorted[s];
    const double x = Y[2 * i], y = Y[2 * i + 1];
    pos[s] = make_double2(x, y);
    inv[i] = (int32_t)s;
}

// delta between sorted keys i and j (bits of common prefix of the 62-bit
// Morton field; ties extend with the index bits); -1 out of range.
__device__ __forceinline__ int kdelta(const uint64_t *__restrict__ k, int m, int i, int j) {
    if (j < 0 || j >= m) return -1;
    uint64_t a = k[i], b = k[j];
    if (a == b) return 62 + __clz((unsigned)(i ^ j));
    return __clzll((long long)(a ^ b)) - 2;
}

// Bottom-up workgroup ranges (bottom_up_intra): the leaves are cut into
// "frontier" subtrees, the maximal subtrees of <= BU_FRONT leaves; workgroup b
// takes the frontier subtrees that start in [b BU_NB, (b + 1) BU_NB), so every
// node of <= BU_FRONT leaves is combined inside one workgroup (LDS hand-off)
// and only the nodes above the frontier cross workgroups.
constexpr int BU_NB = 1024;
constexpr int BU_FRONT = 512;
constexpr int BU_CAP = BU_NB + BU_FRONT;

// Karras (2012) binary radix tree over the m in-root points.  fstart[p] =
// gen marks p as the first leaf of a frontier subtree (gen: this build's
// number, so no clearing pass is needed).
__global__ void karras_build(const uint64_t *__restrict__ k, int64_t n, const int32_t *__restrict__ meta,
                             BHNode *__restrict__ nodes, int32_t *__restrict__ parent_leaf,
                             int32_t *__restrict__ parent_node, int32_t *__restrict__ arrive,
                             int32_t *__restrict__ arrive2, int32_t *__restrict__ fstart, int32_t gen,
                             int32_t *__restrict__ top_cnt, int32_t *root_ref) {
    const int m = meta[0];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    // (the fused chain: m was summed by the sort's bucket workgroups, the root ref of count_in_root follows here)
    if (root_ref && i == 0) *root_ref = m >= 2 ? 0 : (m == 1 ? ~0 : INT32_MIN);
    if (i >= m - 1) return;
    if (i == 0 && top_cnt) *top_cnt = 0;
    arrive[i] = 0;
    arrive2[i] = 0;
    const int dr = kdelta(k, m, i, i + 1), dl = kdelta(k, m, i, i - 1);
    const int d = (dr > dl) ? 1 : -1;
    const int dmin = d > 0 ? dl : dr;
    int lmax = 2;
    while (kdelta(k, m, i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1)
        if (kdelta(k, m, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = kdelta(k, m, i, j);
    int s = 0;
    int t = l;
    do {
        t = (t + 1) >> 1;
        if (kdelta(k, m, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int gamma = i + s * d + (d < 0 ? -1 : 0);
    const int lo = min(i, j), hi = max(i, j);
    int left, right;
    if (lo == gamma) { left = ~gamma; parent_leaf[gamma] = i; }
    else { left = gamma; parent_node[gamma] = i; }
    if (hi == gamma + 1) { right = ~(gamma + 1); parent_leaf[gamma + 1] = i; }
    else { right = gamma + 1; parent_node[gamma + 1] = i; }
    nodes[i].left = left;
    nodes[i].right = right;
    nodes[i].delta = dnode;
    nodes[i].first = lo;
    nodes[i].last = hi;
    if (i == 0) parent_node[0] = -1;
    if (fstart) {
        if (hi - lo + 1 <= BU_FRONT) {
            if (i == 0) fstart[0] = gen;   // the root is the only frontier subtree
        } else {
            if (gamma - lo + 1 <= BU_FRONT) fstart[lo] = gen;
            if (hi - gamma <= BU_FRONT) fstart[gamma + 1] = gen;
        }
    }
}

// Bottom-up count / sums / bounding box / hmin.  The second thread to reach a
// node computes it from its two children (fixed order: deterministic sums).
// Cross-workgroup hand-off without fences (MI355X_MICROARCH.md, "Valid forms"):
// the per-node aggregates that a sibling thread reads are written and read
// with system-scope (sc0 sc1, write-through / cache-bypassing) 8-byte
// accesses; every thread drains its stores (s_waitcnt vmcnt(0)) before its
// relaxed arrival atomic.  Agent-scope __threadfence() (or an acq_rel
// arrival: buffer_wbl2 + buffer_inv at agent scope) here wrote back the whole
// XCD L2 per wave and cost ~8 ms per build at 1M points.  What orders the
// hand-off instead: the writer's stores complete (vmcnt(0), an asm with a
// memory clobber: also a compiler barrier) before its arrival is issued; the
// reader's loads are issued after its arrival returned (a branch on the
// result, plus a compiler-only signal fence so that the relaxed loads cannot
// be hoisted above the relaxed atomic), and they bypass the non-coherent
// caches (system scope).  This relies on gfx950's in-order issue and
// write-through / bypassing system-scope accesses, not on the HIP memory
// model's release / acquire; it is gfx950-only code like the rest.  Since
// round 5 the default arrival is an agent-scope acquire-release RMW instead
// (bottom_up_top<true>, Options::bu_acqrel): the memory model's own ordering,
// at no measurable cost in the two-phase scheme (the round-1 figure above was
// for every level crossing workgroups); the relaxed form stays as option 0.
__device__ __forceinline__ void st_sys(double *p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ double ld_sys(const double *p) {
    return __hip_atomic_load(const_cast<double *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

constexpr int AGG = 10;   // sx, sy, x0, x1, y0, y1, hmin, cnt, rball, (pad)

// rball: radius of a disc around the node's centre of mass inside which a
// query opens EVERY real cell of the subtree (so the subtree is all leaves
// for it).  A cell u is opened by q iff h_u / D(q, c_u) >= theta, i.e. q lies
// in the disc |q - c_u| <= sqrt(h_u / theta); ball(c_v, R_v) is inside
// ball(c_c, R_c) when R_v + |c_v - c_c| <= R_c, hence
// R_v = min(sqrt(h_v/theta) [real v], R_c - |c_v - c_c| over children c),
// shrunk by a relative 1e-9 per level for rounding.  Leaves impose nothing.
// Node p's aggregates from its two children's (child order fixed: the sums
// are deterministic whichever thread combines them); writes nodes[p] and
// returns the nine aggregates in o[] (sx, sy, x0, x1, y0, y1, hmin, cnt,
// rball) and p's parent.
__device__ __forceinline__ void bu_combine_d(int p, const double (&a)[2][7], const double (&c)[2], const double (&rb)[2],
                                             const int32_t (&ch)[2], int32_t dl, int par, int32_t pdelta, double W,
                                             double inv_theta, BHNode *nodes, double (&o)[9]) {
    const double cnt = c[0] + c[1];
    const double sx = a[0][0] + a[1][0], sy = a[0][1] + a[1][1];
    const double x0 = fmin(a[0][2], a[1][2]), x1 = fmax(a[0][3], a[1][3]);
    const double y0 = fmin(a[0][4], a[1][4]), y1 = fmax(a[0][5], a[1][5]);
    const int dlev = dl >> 1;
    bool real;
    if (dl >= 62) real = false;                      // keys tie below 31 levels
    else if (par < 0) real = true;                   // root cell chain
    else real = (pdelta >> 1) < dlev;                // first node of its quad level
    const double h = real ? ldexp(W, -dlev) : -1.0;  // -1 = transparent
    const double hmin = fmin(real ? h : __builtin_inf(), fmin(a[0][6], a[1][6]));
    const double cx = sx / cnt, cy = sy / cnt;       // centerOfMass = sum / cumSize
    double rball = real ? sqrt(h * inv_theta) : __builtin_inf();
    // the children's centres here only bound rball (shrunk by 1e-9 per level):
    // reciprocal + one Newton step instead of two IEEE divisions each
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (ch[k] >= 0) {
            const double r = __builtin_amdgcn_rcp(c[k]);
            const double ic = __fma_rn(r, __fma_rn(-c[k], r, 1.0), r);
            const double ccx = a[k][0] * ic, ccy = a[k][1] * ic;
            const double dd = sqrt((cx - ccx) * (cx - ccx) + (cy - ccy) * (cy - ccy));
            rball = fmin(rball, rb[k] - dd * (1.0 + 1e-12));
        }
    }
    rball = rball > 0.0 ? rball * (1.0 - 1e-9) : 0.0;
    BHNode &nd = nodes[p];                           // read by the traversal (later launches)
    nd.cx = cx;
    nd.cy = cy;
    nd.cnt = (int32_t)cnt;
    nd.h = h;
    nd.hmin = hmin;
    nd.rball = rball;
    nd.bx0 = x0; nd.bx1 = x1; nd.by0 = y0; nd.by1 = y1;
    o[0] = sx; o[1] = sy; o[2] = x0; o[3] = x1; o[4] = y0; o[5] = y1; o[6] = hmin; o[7] = cnt; o[8] = rball;
}
__device__ __forceinline__ int bu_combine(int p, const double (&a)[2][7], const double (&c)[2], const double (&rb)[2],
                                          const int32_t (&ch)[2], int32_t dl, double W, double inv_theta,
                                          BHNode *nodes, const int32_t *__restrict__ parent_node, double (&o)[9]) {
    const int par = parent_node[p];
    bu_combine_d(p, a, c, rb, ch, dl, par, par >= 0 ? nodes[par].delta : 0, W, inv_theta, nodes, o);
    return par;
}

__device__ __forceinline__ void bu_leaf(const double2 *__restrict__ pos, int s, double (&a)[7], double &c, double &rb) {
    const double2 q = pos[s];
    a[0] = q.x; a[1] = q.y; a[2] = q.x; a[3] = q.x; a[4] = q.y; a[5] = q.y;
    a[6] = __builtin_inf();
    c = 1.0;
    rb = __builtin_inf();
}

// Phase 1 of the bottom-up pass: every node inside the workgroup's leaf range
// [S0, S1) (whole frontier subtrees, see BU_FRONT) is combined through LDS
// arrival counters and aggregates.  A node whose parent lies outside the
// range publishes its aggregates to agg (plain stores: the next launch reads
// them) and appends the parent to the arrival list of phase 2, as does a leaf
// whose parent lies outside.  Nothing waits on another workgroup, so a
// workgroup's run is its own short climb.
// The climbs run in steps over an LDS queue of arrivals: each step every
// queued arrival is taken by one thread (the first arriver at a node stops,
// the second combines it and queues the parent for the next step), so the
// live climbers are packed into the first waves -- a climb per thread kept
// all 16 waves issuing every step for their one or two live lanes (round 5:
// 136 us at C3).  The sums are the same: each node is combined from its two
// children in a fixed order, whichever thread does it.
__global__ __launch_bounds__(BU_NB) void bottom_up_intra(const double2 *__restrict__ pos, const int32_t *__restrict__ meta,
                                                        const double *__restrict__ Wp, double inv_theta, BHNode *nodes,
                                                        double *__restrict__ agg, const int32_t *__restrict__ parent_leaf,
                                                        const int32_t *__restrict__ parent_node,
                                                        const int32_t *__restrict__ fstart, int32_t gen,
                                                        int32_t *__restrict__ top_list, int32_t *__restrict__ top_cnt) {
    // aggregates (sx, sy, x0, x1, y0, y1, hmin, rball) and the topology of the
    // range's nodes (ids [S0, S1), Karras: a node's id lies in its own leaf
    // range: count, children, delta, parent, whether the node lies inside the
    // range), staged once so that the climb never waits on global memory
    __shared__ double lagg[8][BU_CAP];
    __shared__ int32_t lleft[BU_CAP], lright[BU_CAP], ldelta[BU_CAP], lcnt[BU_CAP], lpar[BU_CAP];
    __shared__ int32_t larr[BU_CAP];
    __shared__ int32_t queue[2][BU_CAP];
    __shared__ uint8_t lself[BU_CAP];
    __shared__ int32_t sS[2], qn[2];
    const int m = meta[0];
    const int b = blockIdx.x;
    if (m < 2 || b * BU_NB >= m) return;
    const int t = threadIdx.x;
    if (t < 2) { sS[t] = INT32_MAX; qn[t] = 0; }
    __syncthreads();
    // a frontier subtree starts within any BU_FRONT + 1 consecutive leaves
    for (int j = t; j < 2 * (BU_FRONT + 1); j += BU_NB) {
        const int side = j / (BU_FRONT + 1);
        const int p = (b + side) * BU_NB + (j - side * (BU_FRONT + 1));
        if (p < m && fstart[p] == gen) atomicMin(&sS[side], p);
    }
    __syncthreads();
    const int S0 = b == 0 ? 0 : min(sS[0], m);
    const int S1 = (b + 1) * BU_NB >= m ? m : min(sS[1], m);
    for (int j = t; j < S1 - S0; j += BU_NB) {
        const int q = S0 + j;
        larr[j] = 0;
        if (q < m - 1) {
            const BHNode &nd = nodes[q];
            lleft[j] = nd.left; lright[j] = nd.right; ldelta[j] = nd.delta;
            lcnt[j] = nd.last - nd.first + 1; lpar[j] = parent_node[q];
            lself[j] = nd.first >= S0 && nd.last < S1;
        } else {
            lself[j] = 0;   // not a node: never in range
        }
    }
    __syncthreads();
    const double W = *Wp;
    auto in_blk = [&](int q) { return q >= S0 && q < S1 && lself[q - S0]; };
    // the leaves' arrivals: at a parent in the range (queue 0), or phase 2's
    for (int s = S0 + t; s < S1; s += BU_NB) {
        const int p = parent_leaf[s];
        if (p < 0) continue;
        if (!in_blk(p)) top_list[atomicAdd(top_cnt, 1)] = p;   // a leaf hanging off a node above the frontier
        else queue[0][atomicAdd(&qn[0], 1)] = p;
    }
    int cur = 0;
    while (true) {
        __syncthreads();   // the step's queue complete; the other queue empty
        const int na = qn[cur];
        if (na == 0) break;
        const int nxt = cur ^ 1;
        for (int e = t; e < na; e += BU_NB) {
            const int p = queue[cur][e];
            const int op = p - S0;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (__hip_atomic_fetch_add(&larr[op], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0)
                continue;                                // first arriver stops
            const int32_t ch[2] = {lleft[op], lright[op]};
            const int32_t dl = ldelta[op];
            double a[2][7], c[2], rb[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (ch[k] < 0) {
                    bu_leaf(pos, ~ch[k], a[k], c[k], rb[k]);
                } else {                                 // children of an in-range node are in range
                    const int o = ch[k] - S0;
#pragma unroll
                    for (int f = 0; f < 7; ++f) a[k][f] = lagg[f][o];
                    c[k] = (double)lcnt[o];
                    rb[k] = lagg[7][o];
                }
            }
            // bu_combine's global reads of the parent, from the staged topology
            const int par = lpar[op];
            const bool pin = par >= 0 && in_blk(par);
            const int32_t pdelta = pin ? ldelta[par - S0] : (par >= 0 ? nodes[par].delta : 0);
            double o9[9];
            bu_combine_d(p, a, c, rb, ch, dl, par, pdelta, W, inv_theta, nodes, o9);
            if (pin) {
#pragma unroll
                for (int f = 0; f < 7; ++f) lagg[f][op] = o9[f];
                lagg[7][op] = o9[8];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                queue[nxt][atomicAdd(&qn[nxt], 1)] = par;
            } else {
                double *g = agg + AGG * (int64_t)p;
#pragma unroll
                for (int f = 0; f < 9; ++f) g[f] = o9[f];
                if (par >= 0) top_list[atomicAdd(top_cnt, 1)] = par;
            }
        }
        __syncthreads();   // every push of the step done
        if (t == 0) qn[cur] = 0;   // consumed: the next step's push queue
        cur = nxt;
    }
}

// Phase 2: the nodes above the frontier.  Each arrival of phase 1 (a child
// published, the parent listed) starts a climb; the second arriver at a node
// combines it (agent-scope arrival counters, system-scope aggregates: the
// hand-off described above st_sys) and climbs on.  Only the top ~log2(m / BU_FRONT) levels remain
// for this cross-workgroup hand-off.
// ACQREL (Options::bu_acqrel = 1, the default): the arrival is an agent-scope
// acquire-release RMW -- the HIP memory model's own ordering of the
// aggregates' stores before it and the sibling's loads after it -- instead of
// relying on gfx950's in-order issue (0).  C3 whole schedule 5.46 / 5.45 s
// (ABAB, round 5): no measurable cost with the two-phase bottom-up, where
// only the top ~log2(m / 512) levels cross workgroups.
template <bool ACQREL>
__global__ __launch_bounds__(256) void bottom_up_top(const double2 *__restrict__ pos, const int32_t *__restrict__ meta,
                                                     const double *__restrict__ Wp, double inv_theta, BHNode *nodes,
                                                     double *agg, const int32_t *__restrict__ parent_node,
                                                     int32_t *arrive, const int32_t *__restrict__ top_list,
                                                     const int32_t *__restrict__ top_cnt) {
    if (meta[0] < 2) return;   // no karras launch reset the count
    const int ne = *top_cnt;
    const double W = *Wp;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += gridDim.x * blockDim.x) {
        int p = top_list[e];
        while (p >= 0) {
            if (ACQREL) {
                if (__hip_atomic_fetch_add(&arrive[p], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0) break;
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (__hip_atomic_fetch_add(&arrive[p], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) break;
            }
            __atomic_signal_fence(__ATOMIC_SEQ_CST);   // the sibling's aggregates are read after the arrival
            const int32_t ch[2] = {nodes[p].left, nodes[p].right};
            const int32_t dl = nodes[p].delta;
            double a[2][7], c[2], rb[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (ch[k] < 0) {
                    bu_leaf(pos, ~ch[k], a[k], c[k], rb[k]);
                } else {
                    const double *g = agg + AGG * (int64_t)ch[k];
#pragma unroll
                    for (int f = 0; f < 7; ++f) a[k][f] = ld_sys(g + f);
                    c[k] = ld_sys(g + 7);
                    rb[k] = ld_sys(g + 8);
                }
            }
            double o9[9];
            const int par = bu_combine(p, a, c, rb, ch, dl, W, inv_theta, nodes, parent_node, o9);
            double *g = agg + AGG * (int64_t)p;
#pragma unroll
            for (int f = 0; f < 9; ++f) st_sys(g + f, o9[f]);
            p = par;
        }
    }
}

// Number of points whose coordinates equal pos[s] exactly (itself included);
// they sit in the same equal-key run of the sorted order.
__global__ void dup_count(const double2 *__restrict__ pos, const uint64_t *__restrict__ keys, int64_t n,
                          int32_t *__restrict__ dupc, int32_t *__restrict__ vid, int32_t *__restrict__ dflag) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const double2 q = pos[s];
    const uint64_t k = keys[s];
    int32_t c = 1;
    int64_t first = s;   // value id: the first sorted position holding this exact point
    for (int64_t t = s - 1; t >= 0 && keys[t] == k; --t) {
        const double2 p = pos[t];
        if (p.x == q.x && p.y == q.y) { ++c; first = t; }
    }
    for (int64_t t = s + 1; t < n && keys[t] == k; ++t) {
        const double2 p = pos[t];
        c += (p.x == q.x && p.y == q.y);
    }
    dupc[s] = c;
    vid[s] = (int32_t)first;
    if (c > 1) dflag[0] = 1;
}

// ---- Exact duplicates (QuadTree.scala:52-61).  The reference keeps one
// leaf per distinct point and counts every copy on the way down, but when a
// leaf holding c copies of v splits (a different point arrived) it re-inserts
// v ONCE into the new child: cells created after the first copy of v was
// inserted count only 1 + the copies inserted after their creation.  A cell
// is created when its parent cell splits, i.e. at the row t2(parent) of the
// first point in the parent's cell whose value differs from the value of the
// parent cell's first point.  So for a duplicate group of m copies (rows
// r_1 < ... < r_m) and a cell X on its path with parent cell P:
// count_v(X) = m - max(0, #{r_i < t2(P)} - 1)  (the root: m), and the leaf
// of v (the quad child of the deepest cell R that also holds other points)
// has multiplicity m - max(0, #{r_i < t2(R)} - 1).  Only work when some
// point has a duplicate (dflag); no tile or moment ever covers such a group
// (the cells above it are traversed the reference's way).

// t2 per binary node from (first row, its value id, t2) of the two children:
// the union's first value is the earlier child's; its second distinct value
// arrives at the earlier of that child's t2 and the other child's first row
// (different value) or t2 (same value).
// (It also clears the correction arrays of dup_fixup, as dup_clear did.)
__global__ void dup_bottom_up(const int32_t *__restrict__ meta, const int32_t *__restrict__ dflag,
                              const int32_t *__restrict__ idx_sorted, const int32_t *__restrict__ rowmap,
                              const int32_t *__restrict__ vid, const BHNode *__restrict__ nodes,
                              const int32_t *__restrict__ parent_leaf, const int32_t *__restrict__ parent_node,
                              int32_t *arrive2, int32_t *rmin, int32_t *rvid, int32_t *rt2, int32_t *__restrict__ cntcorr,
                              double *__restrict__ sumcorr, int32_t *__restrict__ tiecnt, int32_t *__restrict__ notile,
                              int32_t *__restrict__ vflag, int32_t *__restrict__ vcnt, double *__restrict__ vsum) {
    const int m = meta[0];
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (!dflag[0] || s >= m) return;
    cntcorr[s] = 0;
    sumcorr[2 * s] = 0.0;
    sumcorr[2 * s + 1] = 0.0;
    tiecnt[s] = 0;
    notile[s] = 0;
    vflag[s] = 0;
    vcnt[s] = 0;
    vsum[2 * s] = 0.0;
    vsum[2 * s + 1] = 0.0;
    if (m < 2) return;
    auto leaf = [&](int q, int &r, int &v, int &t) {
        const int32_t l = idx_sorted[q];
        r = rowmap ? rowmap[l] : l;
        v = vid[q];
        t = INT32_MAX;
    };
    auto ld = [](const int32_t *p) { return __hip_atomic_load(const_cast<int32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
    auto st = [](int32_t *p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
    int p = parent_leaf[s];
    while (p >= 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (__hip_atomic_fetch_add(&arrive2[p], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
        int r[2], v[2], t[2];
        const int32_t ch[2] = {nodes[p].left, nodes[p].right};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (ch[k] < 0) leaf(~ch[k], r[k], v[k], t[k]);
            else { r[k] = ld(rmin + ch[k]); v[k] = ld(rvid + ch[k]); t[k] = ld(rt2 + ch[k]); }
        }
        const int a = r[0] < r[1] ? 0 : 1, b = 1 - a;   // a: the child holding the earlier first row
        const int other = v[b] != v[a] ? r[b] : t[b];
        st(rmin + p, r[a]);
        st(rvid + p, v[a]);
        st(rt2 + p, min(t[a], other));
        p = parent_node[p];
    }
}

__device__ __forceinline__ bool real_cell(const BHNode &nd) { return nd.h >= 0.0; }

// One thread per pure duplicate group (the first of m >= 2 exact copies that
// form a whole equal-key run): leaf multiplicity of its tie node, count / sum
// corrections and no-tile marks of the real cells above it.
__global__ void dup_fixup(const int32_t *__restrict__ meta, const int32_t *__restrict__ dflag,
                          const double2 *__restrict__ pos, const uint64_t *__restrict__ keys,
                          const int32_t *__restrict__ dupc, const int32_t *__restrict__ idx_sorted,
                          const int32_t *__restrict__ rowmap, const BHNode *__restrict__ nodes,
                          const int32_t *__restrict__ parent_leaf, const int32_t *__restrict__ parent_node,
                          const int32_t *__restrict__ rt2, int32_t *__restrict__ cntcorr, double *__restrict__ sumcorr,
                          int32_t *__restrict__ tiecnt, int32_t *__restrict__ notile, int32_t *__restrict__ vflag,
                          int32_t *__restrict__ vcnt, double *__restrict__ vsum) {
    const int mroot = meta[0];
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (!dflag[0] || s >= mroot || dupc[s] < 2) return;
    const double2 q = pos[s];
    if (s > 0 && pos[s - 1].x == q.x && pos[s - 1].y == q.y) return;   // not the group's first
    const int m = dupc[s], kb = s + m - 1;
    if (kb >= mroot) return;
    for (int u = s; u <= kb; ++u)
        if (pos[u].x != q.x || pos[u].y != q.y) return;                 // copies not contiguous: impure run
    if ((s > 0 && keys[s - 1] == keys[s]) || (kb + 1 < mroot && keys[kb + 1] == keys[s])) return;
    // the group's node: climb from its first leaf until the node spans [s, kb]
    int g = parent_leaf[s];
    while (g >= 0 && !(nodes[g].first == s && nodes[g].last == kb)) g = parent_node[g];
    if (g < 0 || g == 0) return;                                         // every point identical: root tie
    auto copies_before = [&](int t2) {
        int c = 0;
        for (int u = s; u <= kb; ++u) {
            const int32_t l = idx_sorted[u];
            c += (rowmap ? rowmap[l] : l) < t2;
        }
        return c;
    };
    auto real_above = [&](int x) {   // the nearest real cell strictly above binary node x, -1 if none
        int y = parent_node[x];
        while (y >= 0 && !real_cell(nodes[y])) y = parent_node[y];
        return y;
    };
    int R = real_above(g);
    if (R < 0) return;
    tiecnt[g] = m - max(0, copies_before(rt2[R]) - 1);   // the leaf: R's quad child, created at t2(R)
    // Real node X = the DEEPEST cell C_k of a chain C_1 > ... > C_k of
    // reference cells holding the same points (our binary node exists only
    // where they split).  C_1 (a quad child of the real cell P above) was
    // created at t2(P); C_2..C_k at t2(C_1) = t2(X), in one cascade.
    for (int X = R; X >= 0;) {
        notile[X] = 1;
        const int P = real_above(X);
        const int lx = nodes[X].delta >> 1;
        const int deep = max(0, copies_before(rt2[X]) - 1);
        int top, node_corr;
        bool chain;
        if (P < 0) {   // the root: C_1 is the reference root cell, which holds every copy
            top = 0;
            chain = lx > 0;
        } else {
            top = max(0, copies_before(rt2[P]) - 1);
            chain = lx > (nodes[P].delta >> 1) + 1;
        }
        node_corr = chain ? deep : top;
        if (node_corr > 0) {
            atomicAdd(&cntcorr[X], node_corr);
            atomicAdd(&sumcorr[2 * X], node_corr * q.x);
            atomicAdd(&sumcorr[2 * X + 1], node_corr * q.y);
        }
        if (chain) {   // the chain top's own count: a virtual record when it differs
            if (top > 0) {
                atomicAdd(&vcnt[X], top);
                atomicAdd(&vsum[2 * X], top * q.x);
                atomicAdd(&vsum[2 * X + 1], top * q.y);
            }
            if (top != deep) vflag[X] = 1;
        }
        X = P;
    }
}

// corrected counts / centres of mass of the cells above duplicate groups
__global__ void dup_apply(int32_t *__restrict__ meta, const int32_t *__restrict__ dflag,
                          const int32_t *__restrict__ cntcorr, const double *__restrict__ sumcorr,
                          const int32_t *__restrict__ vflag, const int32_t *__restrict__ vcnt,
                          const double *__restrict__ vsum, int32_t *__restrict__ vcntf, double *__restrict__ vcom,
                          BHNode *__restrict__ nodes) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (!dflag[0] || i >= meta[0] - 1 || (cntcorr[i] == 0 && !vflag[i])) return;
    BHNode &nd = nodes[i];
    const double c0 = nd.cnt, x0 = nd.cx * c0, y0 = nd.cy * c0;   // all copies
    if (vflag[i]) {   // the chain top C_1
        if (i == meta[1]) meta[3] = 1;   // the root's chain: the reference root cell holds every copy
        const int32_t ct = nd.cnt - vcnt[i];
        vcntf[i] = ct;
        vcom[2 * i] = (x0 - vsum[2 * i]) / ct;
        vcom[2 * i + 1] = (y0 - vsum[2 * i + 1]) / ct;
    }
    if (cntcorr[i] != 0) {
        const double c1 = nd.cnt - cntcorr[i];
        nd.cx = (x0 - sumcorr[2 * i]) / c1;
        nd.cy = (y0 - sumcorr[2 * i + 1]) / c1;
        nd.cnt -= cntcorr[i];
    }
}

// ---- subtree moments: chunk counts, item map, per-item partial sums, reduce
// Per binary node with >= MOM_MIN_POINTS points (when the gate is on, see
// bbox_final): its chunk count, its place in the list of moment nodes of
// several chunks (one atomic per block; moment_reduce's work list) and its item range (one atomic per block on the item
// counter off[n]; the placement of the ranges varies from run to run, a
// node's chunks are summed in chunk order, so the moments do not), with the
// item -> node map filled in.
__global__ __launch_bounds__(1024) void moment_count(const BHNode *__restrict__ nodes, int64_t n, const int32_t *__restrict__ meta,
                             const int32_t *__restrict__ mom_flag, int32_t *__restrict__ cnt,
                             int32_t *__restrict__ list, int32_t *__restrict__ meta_w, int32_t *__restrict__ off,
                             int32_t *__restrict__ item) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int m = meta[0];
    int32_t c = 0;
    if (i < m - 1 && mom_flag[0]) {
        const BHNode &nd = nodes[i];
        if (nd.cnt >= MOM_MIN_POINTS && nd.delta < 62) c = (nd.cnt + MOM_CHUNK - 1) / MOM_CHUNK;
    }
    if (i < n) cnt[i] = c;
    __shared__ int wcnt[16], wbase[16], wsum[16], wibase[16];
    const int w = threadIdx.x >> 6, lane = lane_id();
    const uint64_t bal = __ballot(c > 1);   // the list: nodes of several chunks (moment_reduce)
    int inc = c;   // inclusive scan of the chunk counts over the wave (item offsets)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[w] = inc;
    if (lane == 0) wcnt[w] = (int)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0, itot = 0;
        for (int k = 0; k < (int)(blockDim.x >> 6); ++k) {
            wbase[k] = tot; tot += wcnt[k];
            wibase[k] = itot; itot += wsum[k];
        }
        const int base = tot ? atomicAdd(&meta_w[2], tot) : 0;
        const int ibase = itot ? atomicAdd(&off[n], itot) : 0;
        for (int k = 0; k < (int)(blockDim.x >> 6); ++k) { wbase[k] += base; wibase[k] += ibase; }
    }
    __syncthreads();
    if (c > 1) list[wbase[w] + __popcll(bal & lanemask_lt())] = (int32_t)i;
    if (c > 0) {
        const int o = wibase[w] + inc - c;
        off[i] = o;
        for (int k = 0; k < c; ++k) item[o + k] = (int32_t)i;
    }
}

// Fixed-order wave reduction of MOM_K per-lane partial sums to dst[0..MOM_K)
// (LDSRED: 8 moments at a time transposed through a per-wave LDS tile -- 8
// row sums per column + 3 shuffle stages, ~20 instructions per 8 moments --
// instead of a 6-stage shuffle tree per moment).
template <bool LDSRED>
__device__ __forceinline__ void moments_wave_store(const double (&acc)[MOM_K], double *rw, int lane,
                                                   double *__restrict__ dst) {
    if (LDSRED) {
        const int col = lane & 7, r0 = (lane >> 3) * 8;
#pragma unroll
        for (int k0 = 0; k0 < MOM_K; k0 += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) rw[lane * 9 + j] = (k0 + j < MOM_K) ? acc[k0 + j] : 0.0;
            // the other lanes' stores must have landed before the cross-lane
            // loads (and those loads before the next round overwrites rw)
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
            __builtin_amdgcn_wave_barrier();
            double v = 0.0;
#pragma unroll
            for (int r = 0; r < 8; ++r) v += rw[(r0 + r) * 9 + col];
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            v += __shfl_xor(v, 8, 64);
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (lane < 8 && k0 + lane < MOM_K) dst[k0 + lane] = v;
        }
    } else {
#pragma unroll
        for (int k = 0; k < MOM_K; ++k) {
            const double v = wave_sum(acc[k]);
            if (lane == 0) dst[k] = v;
        }
    }
}

// One wave per item (<= MOM_CHUNK points of one node): lanes accumulate the
// scaled moments u_x^a u_y^b / (a! b!) in registers, then the fixed-order
// wave reduction.  A node of one chunk (chunk counts cnt, when given) gets its
// moments written directly to mom; moment_reduce sums the others' chunks.
template <bool LDSRED>
__global__ __launch_bounds__(256) void moment_items(const double2 *__restrict__ pos,
                                                    const BHNode *__restrict__ nodes,
                                                    const int32_t *__restrict__ off, int64_t n,
                                                    const int32_t *__restrict__ item,
                                                    double *__restrict__ part, const int32_t *__restrict__ cnt,
                                                    double *__restrict__ mom) {
    __shared__ double red[4][64 * 9];
    double *rw = red[threadIdx.x >> 6];
    const int total = off[n];
    const int lane = lane_id();
    const int nw = gridDim.x * (blockDim.x >> 6);
    for (int it = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); it < total; it += nw) {
        const int node = __builtin_amdgcn_readfirstlane(item[it]);
        const int c = it - off[node];
        const BHNode &nd = nodes[node];
        double cx, cy, R;
        box_centre(nd, cx, cy, R);
        const int p0 = nd.first + c * MOM_CHUNK;
        const int p1 = min(nd.last + 1, p0 + MOM_CHUNK);
        double acc[MOM_K];
#pragma unroll
        for (int k = 0; k < MOM_K; ++k) acc[k] = 0.0;
        for (int p = p0 + lane; p < p1; p += 64) {
            const double2 q = pos[p];
            const double ux = q.x - cx, uy = q.y - cy;
            double X[MOM_DEG + 1], Yv[MOM_DEG + 1];
            X[0] = 1.0; Yv[0] = 1.0;
#pragma unroll
            for (int e = 1; e <= MOM_DEG; ++e) {
                X[e] = X[e - 1] * ux * (1.0 / e);
                Yv[e] = Yv[e - 1] * uy * (1.0 / e);
            }
#pragma unroll
            for (int a = 0; a <= MOM_DEG; ++a)
#pragma unroll
                for (int b = 0; b <= MOM_DEG; ++b)
                    if (a + b <= MOM_DEG) acc[midx(a, b)] = __fma_rn(X[a], Yv[b], acc[midx(a, b)]);
        }
        const bool single = cnt && __builtin_amdgcn_readfirstlane(cnt[node]) == 1;
        moments_wave_store<LDSRED>(acc, rw, lane, single ? mom + (int64_t)node * MOM_K : part + (int64_t)it * MOM_K);
    }
}

// One wave per moment node of several chunks (the list; single-chunk nodes
// were written by moment_items): each lane sums its chunks' partials (chunk j
// to lane j mod 64, in order), then the fixed-order wave reduction -- the
// root's ~500 chunks are no longer one lane's serial chain.
__global__ __launch_bounds__(256) void moment_reduce(const int32_t *__restrict__ meta, const int32_t *__restrict__ list,
                                                     const int32_t *__restrict__ cnt, const int32_t *__restrict__ off,
                                                     const double *__restrict__ part, double *__restrict__ mom) {
    __shared__ double red[4][64 * 9];
    double *rw = red[threadIdx.x >> 6];
    const int nl = meta[2];
    const int lane = lane_id();
    const int nw = gridDim.x * (blockDim.x >> 6);
    for (int e = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); e < nl; e += nw) {
        const int node = __builtin_amdgcn_readfirstlane(list[e]);
        const int c = __builtin_amdgcn_readfirstlane(cnt[node]);
        const int o = __builtin_amdgcn_readfirstlane(off[node]);
        double acc[MOM_K];
#pragma unroll
        for (int k = 0; k < MOM_K; ++k) acc[k] = 0.0;
        for (int j = lane; j < c; j += 64) {
            const double *pp = part + (int64_t)(o + j) * MOM_K;
#pragma unroll
            for (int k = 0; k < MOM_K; ++k) acc[k] += pp[k];
        }
        moments_wave_store<true>(acc, rw, lane, mom + (int64_t)node * MOM_K);
    }
}

__device__ __forceinline__ double factd(int k) {
    double f = 1.0;
    for (int j = 2; j <= k; ++j) f *= j;
    return f;
}

// Coefficient c of the root polynomials from the node's moments mu (one
// thread per coefficient; (p, q) ordered like midx within each polynomial).
__global__ void poly_coef(const double *__restrict__ mu, double *__restrict__ coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= POLY_K) return;
    int kind = 0, i = 0, r = c;   // kind 0 z, 1 x, 2 y
    if (c >= POLY_Y) { kind = 2; r = c - POLY_Y; }
    else if (c >= POLY_X) { kind = 1; r = c - POLY_X; }
    for (;;) {
        const int len = poly_len(kind == 0 ? 2 * i : 2 * i + 1);
        if (r < len) break;
        r -= len;
        ++i;
    }
    const int d = kind == 0 ? 2 * i : 2 * i + 1;
    int p = 0;
    while (r >= d + 1 - p) { r -= d + 1 - p; ++p; }
    const int q = r;
    double s = 0.0;
    for (int a = p; a <= d; ++a) {
        const int b = d - a;
        const bool ok = kind == 0 ? !(a & 1) : kind == 1 ? (a & 1) : !(a & 1);
        if (!ok || b < q) continue;
        const int j = kind == 1 ? (a - 1) / 2 : a / 2;
        s += factd(i) / (factd(j) * factd(i - j)) * factd(a) * factd(b) * mu[midx(a - p, b - q)];
    }
    coef[c] = (((p + q) & 1) ? -s : s) / (factd(p) * factd(q));
}

// Quad records: one per real node, children found through transparent nodes
// (build_qrec below).  Slots of transparent nodes are never written: only
// real cells are ever pushed (and their records read) by the traversal.
struct DupView {   // duplicate-multiplicity data for build_qrec (nullptr members when there is none)
    const int32_t *tiecnt, *notile, *vflag, *vcntf;
    const double *vcom;
    int32_t virt;   // record index offset of the virtual chain tops (= n)
};
__device__ __forceinline__ void build_qrec_reg(const BHNode *__restrict__ nodes, const double2 *__restrict__ pos, int i,
                                               double inv_theta, double near_dmax, const DupView &dv, QRec &r);
// One thread per binary node: it builds its record in registers
// (build_qrec_reg) and writes it as 16 contiguous 16-byte stores (the partial
// lines of a wave's stores merge in the L2), so the occupancy is set by
// registers -- an LDS-staged version (coalesced copies of 64 records per
// workgroup, 16 KB of LDS each) took 103 us at C3, this one 87 us (round 5).
__global__ __launch_bounds__(256) void build_qrec(const BHNode *__restrict__ nodes,
                                                         const double2 *__restrict__ pos,
                                                         const int32_t *__restrict__ meta, double inv_theta,
                                                         double near_dmax, const int32_t *__restrict__ dflag,
                                                         DupView dv, QRec *__restrict__ qrec) {
    const int m = meta[0];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m - 1) return;
    const bool dups = dflag[0] != 0;
    if (!dups) dv = DupView{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    if (nodes[i].h >= 0.0) {   // transparent / key-tie nodes get no record
        QRec r;
        build_qrec_reg(nodes, pos, i, inv_theta, near_dmax, dv, r);
        const uint4 *src = reinterpret_cast<const uint4 *>(&r);
        uint4 *dst = reinterpret_cast<uint4 *>(qrec + i);
#pragma unroll
        for (int k = 0; k < (int)(sizeof(QRec) / 16); ++k) dst[k] = src[k];
    }
    if (dups && dv.vflag[i]) {   // node i's chain top C_1 (as build_qrec)
        const BHNode &nd = nodes[i];
        QRec v;
        v.cx = dv.vcom[2 * i]; v.cy = dv.vcom[2 * i + 1]; v.rball = 0.0;
        v.hmin = fmax(nd.hmin * inv_theta * (1.0 - 1e-12), near_dmax) * (1.0 - 1.1e-12);
        v.bx0 = nd.bx0; v.bx1 = nd.bx1; v.by0 = nd.by0; v.by1 = nd.by1;
        v.ex = 1e-15 * (fabs(nd.bx0) + fabs(nd.bx1) + fabs(nd.by0) + fabs(nd.by1));
        v.lmask = 0;
        v.first = nd.first; v.last = nd.last; v.cnt = dv.vcntf[i]; v.nch = 1;
        v.ccx[0] = nd.cx; v.ccy[0] = nd.cy; v.cref[0] = i; v.ccnt[0] = nd.cnt;
        v.ca[0] = qacc_accept(nd.h, inv_theta);
        v.cb[0] = qacc_open(nd.h, inv_theta);
        for (int k = 1; k < 4; ++k) {
            v.ccx[k] = 0.0; v.ccy[k] = 0.0; v.cb[k] = 0.0; v.ca[k] = 0.0; v.cref[k] = 0; v.ccnt[k] = 0;
        }
        qrec[dv.virt + i] = v;
    }
}

// One quad record, every array of it indexed by compile-time constants (the
// children's refs collected first, then one unrolled slot per child), so that
// the record stays in registers (build_qrec).
__device__ __forceinline__ void build_qrec_reg(const BHNode *__restrict__ nodes, const double2 *__restrict__ pos, int i,
                                               double inv_theta, double near_dmax, const DupView &dv, QRec &r) {
    const int32_t *tiecnt = dv.tiecnt, *notile = dv.notile;
    const BHNode &nd = nodes[i];
    r.cx = nd.cx; r.cy = nd.cy; r.rball = nd.rball * nd.rball * (1.0 - 1e-9);
    r.hmin = fmax(nd.hmin * inv_theta * (1.0 - 1e-12), near_dmax) * (1.0 - 1.1e-12);
    r.bx0 = nd.bx0; r.bx1 = nd.bx1; r.by0 = nd.by0; r.by1 = nd.by1;
    r.ex = 1e-15 * (fabs(nd.bx0) + fabs(nd.bx1) + fabs(nd.by0) + fabs(nd.by1));
    r.lmask = 0;
    r.first = nd.first; r.last = nd.last; r.cnt = nd.cnt;
    auto transparent = [&](int32_t c) { return c >= 0 && nodes[c].delta < 62 && nodes[c].h < 0.0; };
    // the quad children in key order (<= 4: a 2-deep descent through transparent nodes)
    int32_t l0 = 0, l1 = 0, l2 = 0, l3 = 0;
    int nc = 0;
    auto add = [&](int32_t c) {
        l3 = nc == 3 ? c : l3; l2 = nc == 2 ? c : l2; l1 = nc == 1 ? c : l1; l0 = nc == 0 ? c : l0;
        ++nc;
    };
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int32_t c = k == 0 ? nd.left : nd.right;
        if (transparent(c)) {
            const int32_t l = nodes[c].left, rr = nodes[c].right;
            if (transparent(l)) { add(nodes[l].left); add(nodes[l].right); } else add(l);
            if (transparent(rr)) { add(nodes[rr].left); add(nodes[rr].right); } else add(rr);
        } else {
            add(c);
        }
    }
    int kinds = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int32_t c = k == 0 ? l0 : k == 1 ? l1 : k == 2 ? l2 : l3;
        double x = 0.0, y = 0.0, cb = 0.0, ca = 0.0;
        int32_t cref = 0, ccnt = 0;
        if (k < nc) {
            double chv;
            if (c < 0) {
                const double2 p = pos[~c];
                x = p.x; y = p.y; chv = QCH_LEAF; cref = c; ccnt = 1;
            } else {
                const BHNode &cn = nodes[c];
                x = cn.cx; y = cn.cy; chv = cn.delta >= 62 ? QCH_TIE : cn.h;
                cref = c; ccnt = cn.cnt;
                if (cn.delta >= 62 && tiecnt && tiecnt[c] > 0) {   // pure duplicate group: one leaf, its multiplicity
                    const double2 p = pos[cn.first];
                    x = p.x; y = p.y; chv = QCH_MULTI; ccnt = tiecnt[c];
                } else if (cn.delta < 62 && dv.vflag && dv.vflag[c]) {   // the chain top C_1 of real node c
                    x = dv.vcom[2 * c]; y = dv.vcom[2 * c + 1]; chv = 0.5 * nd.h;
                    cref = dv.virt + c; ccnt = dv.vcntf[c];
                }
                if (chv >= 0.0) { ca = qacc_accept(chv, inv_theta); cb = qacc_open(chv, inv_theta); }
            }
            kinds |= (chv == QCH_LEAF ? QK_LEAF : chv == QCH_TIE ? QK_TIE : chv == QCH_MULTI ? QK_MULTI : QK_CELL)
                     << (QNCH_KIND + 2 * k);
        }
        r.ccx[k] = x; r.ccy[k] = y; r.cb[k] = cb; r.ca[k] = ca; r.cref[k] = cref; r.ccnt[k] = ccnt;
    }
    const double hx = 0.5 * (nd.bx1 - nd.bx0), hy = 0.5 * (nd.by1 - nd.by0);
    const bool tile_possible = (nd.rball > 0.0 || (hx * hx + hy * hy) * (1.0 - 1e-9) <= fmax(nd.hmin * inv_theta, near_dmax))
                               && !(notile && notile[i]);
    r.nch = nc | (tile_possible ? QNCH_TILE : 0) | kinds;
}

// Option trav_front_cur: the traversal's workgroup order from this build's
// predicted wave costs (gather_sorted): workgroups whose heaviest predicted
// 64-query wave (narrow groups excluded) is >= ffac x the mean first, the rest
// after, each in Morton order.  One workgroup, on the second stream during the build.
__global__ __launch_bounds__(1024) void trav_order_cur(const int32_t *__restrict__ pred,
                                                       const int32_t *__restrict__ nflag, int64_t waves, double ffac,
                                                       int32_t *__restrict__ border) {
    __shared__ unsigned long long red[16];
    __shared__ int32_t wtot[16];
    __shared__ double sthr;
    const int t = threadIdx.x, lane = lane_id(), w = t >> 6;
    unsigned long long acc = 0, cnt = 0;
    for (int64_t g = t; g < waves; g += 1024)
        if (!(nflag && nflag[g])) { acc += (unsigned long long)max(pred[g], 0); ++cnt; }
    acc = wave_sum(acc);
    cnt = wave_sum(cnt);
    if (lane == 0) { red[w] = acc; wtot[w] = (int32_t)cnt; }
    __syncthreads();
    if (t == 0) {
        unsigned long long a = 0, c = 0;
        for (int j = 0; j < 16; ++j) { a += red[j]; c += (unsigned long long)wtot[j]; }
        sthr = ffac * (double)a / (double)max(1ull, c);
    }
    __syncthreads();
    const double thr = sthr;
    const int64_t nb = (waves + TRAV_WPB - 1) / TRAV_WPB;
    int32_t pos = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int64_t b0 = 0; b0 < nb; b0 += 1024) {
            const int64_t b = b0 + t;
            bool in = false;
            if (b < nb) {
                int32_t c = 0;
                for (int k = 0; k < TRAV_WPB; ++k) {
                    const int64_t g = b * TRAV_WPB + k;
                    if (g < waves && !(nflag && nflag[g])) c = max(c, pred[g]);
                }
                const bool heavy = c > 0 && (double)c >= thr;
                in = pass == 0 ? heavy : !heavy;
            }
            const uint64_t m = __ballot(in);
            __syncthreads();
            if (lane == 0) wtot[w] = (int32_t)__popcll(m);
            __syncthreads();
            int32_t off = pos, tot = 0;
            for (int j = 0; j < 16; ++j) {
                if (j < w) off += wtot[j];
                tot += wtot[j];
            }
            if (in) border[off + (int32_t)__popcll(m & lanemask_lt())] = (int32_t)b;
            pos += tot;
        }
    }
}

// ---- Root-tile mode (the small-embedding phase).  When every point lies in
// the root cell, no point has an exact duplicate, the bounding box is so
// small that every query opens the root (4 theta max(dx, dy) < 1: a cell
// holding all points has half-width >= max(dx, dy) / 2 and D <= dx^2 + dy^2)
// and passes the near-exact test at it (every box corner within near_dmax),
// the normal path makes the root one tile for every lane, evaluated from the
// root's moments (tile_apply -> moment_apply).  This path computes that --
// the root's moments (moment_items / moment_reduce, chunks of the points in
// label order), the same per-query additions -- without the Morton sort, the
// radix tree, the bottom-up aggregates, the quad records or the moments of
// the other ~n/64 nodes.  Duplicates are found by a hash set instead of the
// sorted order (any duplicate: the full path).
//
// Exact-duplicate detection without sorting or atomics (device-scope atomics
// execute at the memory side, ~13 G/s for one CAS per point): rounds of a
// last-writer-wins table of 4n slots.  Round r: every open point stores its
// index at slot h_r(point) (plain stores; one of the points sharing a slot
// wins), then -- next kernel -- reads the slot back: the winner is done, a
// point that finds a point with its exact coordinates raises the flag, and a
// point that finds different coordinates stays open for the next round's
// hash.  Two copies of one position share every slot, so they stay open
// together until one of them wins one (found).  ~11 % of the points stay open
// after round 0, ~0.2 % after round 1; any still open after the last round
// raise the flag too (flag = "not shown duplicate-free": the full path, which
// handles every case).
constexpr int DUP_ROUNDS = 4;
__device__ __forceinline__ uint64_t hash_xy(double x, double y, uint64_t seed) {
    uint64_t h = ((uint64_t)__double_as_longlong(x) ^ seed) * 0x9E3779B97F4A7C15ull;
    h ^= (uint64_t)__double_as_longlong(y) + 0x632BE59BD9B4E019ull + (h << 6) + (h >> 2);
    h ^= h >> 31;
    h *= 0xD6E8FEB86659FD93ull;
    return h ^ (h >> 32);
}
__device__ __forceinline__ uint64_t dup_seed(int round) { return 0xA24BAED4963EE407ull * (uint64_t)(round + 1); }

__global__ __launch_bounds__(256) void dup_store(const double2 *__restrict__ Y, int64_t n, int32_t *__restrict__ tab,
                                                 uint64_t mask, const uint8_t *__restrict__ open, int round) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || (round > 0 && !open[i])) return;
    const double2 p = Y[i];
    tab[hash_xy(p.x, p.y, dup_seed(round)) & mask] = (int32_t)i;
}

__global__ __launch_bounds__(256) void dup_probe(const double2 *__restrict__ Y, int64_t n,
                                                 const int32_t *__restrict__ tab, uint64_t mask,
                                                 uint8_t *__restrict__ open, int round, int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || (round > 0 && !open[i])) return;
    const double2 p = Y[i];
    const int64_t w = tab[hash_xy(p.x, p.y, dup_seed(round)) & mask];
    bool still = false;
    if (w != i) {
        const double2 o = Y[w];
        if (o.x == p.x && o.y == p.y) flag[0] = 1;
        else still = true;
    }
    if (still && round == DUP_ROUNDS - 1) flag[0] = 1;
    if (round == 0 || !still) open[i] = still ? 1 : 0;
}

// The root's moments from its chunk partials (root-tile mode, ~n / MOM_CHUNK
// chunks): one block per moment, fixed strided + tree order.
__global__ __launch_bounds__(256) void root_moment_reduce(const int32_t *__restrict__ mom_off, int64_t n,
                                                          const double *__restrict__ part, double *__restrict__ mom) {
    __shared__ double red[256];
    const int k = blockIdx.x;
    const int K = mom_off[n];
    double s = 0.0;
    for (int it = threadIdx.x; it < K; it += 256) s += part[(int64_t)it * MOM_K + k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) mom[k] = red[0];
}

__global__ void root_tile_check(const int32_t *__restrict__ dflag, const double *__restrict__ bb,
                                const double *__restrict__ Wp, int64_t n, double theta, double near_dmax,
                                int32_t *__restrict__ status) {
    const double W = *Wp, dx = bb[1] - bb[0], dy = bb[3] - bb[2];
    const double amax = fmax(fmax(fabs(bb[0]), fabs(bb[1])), fmax(fabs(bb[2]), fabs(bb[3])));
    const double ex = 6e-15 * amax;   // the traversal's rounding margin, bounded for every query in the box
    const double dmax = ((dx + ex) * (dx + ex) + (dy + ex) * (dy + ex)) * (1.0 + 1e-11);
    // every point inside the root cell Cell(0, 0, W) (closed, Cell.scala:31-36)
    const bool in_root = -W <= bb[0] && bb[1] <= W && -W <= bb[2] && bb[3] <= W;
    const double box = 4.0 * theta * fmax(dx, dy) * (1.0 + 1e-12);
    const bool ok = in_root && n >= MOM_MIN_POINTS && !dflag[0] && W > 0.0 && theta > 0.0 && box < 1.0 &&
                    dmax <= near_dmax;
    status[0] = ok ? 1 : 0;
    // how far the box is from the test: floor(log2) of the larger ratio (the
    // host skips the test for a while once the embedding has outgrown it)
    const double r = fmax(box, near_dmax > 0.0 ? dmax / near_dmax : 0.0);
    status[1] = r > 1.0 ? (int32_t)fmin(60.0, floor(log2(r))) : 0;
}

// The root's moment items: node 0 = all m sorted points, its bounding box.
__global__ void root_tile_prep(const double *__restrict__ bb, int64_t n, BHNode *__restrict__ nodes,
                               int32_t *__restrict__ mom_cnt, int32_t *__restrict__ mom_off,
                               int32_t *__restrict__ mom_list, int32_t *__restrict__ mom_item, int32_t *__restrict__ meta_w,
                               int32_t *__restrict__ inv, int32_t *__restrict__ idx_sorted,
                               int32_t *__restrict__ mom_flag) {
    const int m = (int)n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        inv[i] = i;            // no sort: query / force slots are the labels
        idx_sorted[i] = i;
    }
    const int K = (m + MOM_CHUNK - 1) / MOM_CHUNK;
    for (int it = blockIdx.x * blockDim.x + threadIdx.x; it < K; it += gridDim.x * blockDim.x) mom_item[it] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        BHNode &r = nodes[0];
        r.first = 0; r.last = m - 1; r.cnt = m;
        r.bx0 = bb[0]; r.bx1 = bb[1]; r.by0 = bb[2]; r.by1 = bb[3];
        mom_cnt[0] = K;
        mom_off[0] = 0;
        mom_off[n] = K;
        mom_list[0] = 0;
        meta_w[0] = m;
        meta_w[2] = 1;
        // every query's tile is eligible: the next full build keeps moments on
        mom_flag[0] = 1;
        mom_flag[1] = mom_flag[2];
    }
}

}  // namespace

// The Morton sort (64-bit keys, int32 payload).  rocPRIM's radix sort picks
// its merge sort below 2^20 items (22 launches, ~200 us at 1M; Onesweep
// measured ~300 us at 1M).
static void morton_sort(void *tmp, size_t &bytes, const uint64_t *k_in, uint64_t *k_out, const int32_t *v_in,
                        int32_t *v_out, int64_t n, hipStream_t st) {
    TSNE_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, k_in, k_out, v_in, v_out, (int)n, 0, 64, st));
}

// The build's share of bh_alloc (bhtree.hip), in the two pieces bh_alloc
// calls: the tree itself, then (after the evaluation's task lists) the
// build's temporaries, root-tile tables and sort buffers.
void bh_alloc_tree(tsne_ctx *ctx, BHTree &t, int64_t n, const std::string &pre) {
    Workspace &ws = ctx->ws;
    t.n = n;
    t.keys = ws.get<uint64_t>(pre + "keys", n);
    t.keys_sorted = ws.get<uint64_t>(pre + "keys_sorted", n);
    t.idx = ws.get<int32_t>(pre + "idx", n);
    t.idx_sorted = ws.get<int32_t>(pre + "idx_sorted", n);
    t.inv = ws.get<int32_t>(pre + "inv", n);
    t.dupc = ws.get<int32_t>(pre + "dupc", n);
    t.vid = ws.get<int32_t>(pre + "vid", n);
    t.dflag = ws.get<int32_t>(pre + "dflag", 1);
    t.rmin = ws.get<int32_t>(pre + "rmin", n);
    t.rvid = ws.get<int32_t>(pre + "rvid", n);
    t.rt2 = ws.get<int32_t>(pre + "rt2", n);
    t.arrive2 = ws.get<int32_t>(pre + "arrive2", n);
    t.cntcorr = ws.get<int32_t>(pre + "cntcorr", n);
    t.tiecnt = ws.get<int32_t>(pre + "tiecnt", n);
    t.notile = ws.get<int32_t>(pre + "notile", n);
    t.sumcorr = ws.get<double>(pre + "sumcorr", 2 * (size_t)n);
    t.vflag = ws.get<int32_t>(pre + "vflag", n);
    t.vcnt = ws.get<int32_t>(pre + "vcnt", n);
    t.vcntf = ws.get<int32_t>(pre + "vcntf", n);
    t.vsum = ws.get<double>(pre + "vsum", 2 * (size_t)n);
    t.vcom = ws.get<double>(pre + "vcom", 2 * (size_t)n);
    t.pos = ws.get<double2>(pre + "pos", n);
    t.nodes = ws.get<BHNode>(pre + "nodes", n);
    t.qrec = ws.get<QRec>(pre + "qrec", 2 * (size_t)n);   // [n, 2n): virtual chain-top records (duplicates)
    t.agg = ws.get<double>(pre + "agg", AGG * (size_t)n);
    t.parent_leaf = ws.get<int32_t>(pre + "parent_leaf", n);
    t.parent_node = ws.get<int32_t>(pre + "parent_node", n);
    t.arrive = ws.get<int32_t>(pre + "arrive", n);
    t.fstart = ws.get<int32_t>(pre + "fstart", n);
    TSNE_HIP(hipMemsetAsync(t.fstart, 0, sizeof(int32_t) * n, ctx->stream));
    t.gen = 0;
    t.rt_skip = 0;
    t.top_list = ws.get<int32_t>(pre + "top_list", 2 * (size_t)n);
    t.top_cnt = ws.get<int32_t>(pre + "top_cnt", 1);
    t.meta = ws.get<int32_t>(pre + "meta", 4);
    t.mom = ws.get<double>(pre + "mom", (size_t)n * MOM_K);
    t.mom_cnt = ws.get<int32_t>(pre + "mom_cnt", n + 1);
    t.mom_off = ws.get<int32_t>(pre + "mom_off", n + 1);
    t.mom_list = ws.get<int32_t>(pre + "mom_list", n);
    // items <= sum over moment nodes of (cnt / MOM_CHUNK + 1); every point lies in
    // at most 94 nested nodes (62 key bits + 32 tie-break bits)
    t.mom_items_cap = n + ceil_div(n * 94, MOM_CHUNK);
    t.mom_item = ws.get<int32_t>(pre + "mom_item", t.mom_items_cap);
    t.mom_part = ws.get<double>(pre + "mom_part", (size_t)t.mom_items_cap * MOM_K);
    t.mom_flag = ws.get<int32_t>(pre + "mom_flag", 3);
    const int32_t flag_init[3] = {1, INT32_MAX, (int32_t)std::min<int64_t>(INT32_MAX, (n >> 6) + 1)};   // first build: moments on
    TSNE_HIP(hipMemcpyAsync(t.mom_flag, flag_init, sizeof(flag_init), hipMemcpyHostToDevice, ctx->stream));
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
}

void bh_alloc_build_tmp(tsne_ctx *ctx, BHTree &t, int64_t n, const std::string &pre) {
    Workspace &ws = ctx->ws;
    size_t sb = 0;
    TSNE_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, sb, t.mom_cnt, t.mom_off, (int)(n + 1), ctx->stream));
    t.scan_tmp_bytes = sb;
    t.scan_tmp = ws.get<uint8_t>(pre + "scan_tmp", sb);
    t.bbox_blocks = (int)std::min<int64_t>(1024, std::max<int64_t>(1, ceil_div(n, 256)));
    t.bbox_part = ws.get<double>(pre + "bbox_part", 4 * (size_t)t.bbox_blocks);
    t.W = ws.get<double>(pre + "W", 1);
    t.bb = ws.get<double>(pre + "bb", 4);
    t.status = ws.get<int32_t>(pre + "status", 4);
    t.status_h = ctx->pinned;
    t.rcoef = ws.get<double>(pre + "rcoef", POLY_K);
    t.dup_mask = ((uint64_t)1 << (64 - __builtin_clzll((uint64_t)std::max<int64_t>(2, 4 * n) - 1))) - 1;
    t.dup_tab = ws.get<int32_t>(pre + "dup_tab", t.dup_mask + 1);
    t.dup_open = ws.get<uint8_t>(pre + "dup_open", n);
    size_t tb = 0;
    morton_sort(nullptr, tb, t.keys, t.keys_sorted, t.idx, t.idx_sorted, n, ctx->stream);
    t.sort_tmp_bytes = tb;
    t.sort_tmp = ws.get<uint8_t>(pre + "sort_tmp", tb);
    csort_alloc(ctx, t.cs, n, pre);
    t.cs_primed = false;
}

// The near-exact tolerance of a build (Options::near_tol_early / near_tol_late;
// 0 disables the test)
double bh_near_tol(const tsne_ctx *ctx, bool late) { return late ? ctx->opts.near_tol_late : ctx->opts.near_tol_early; }

// Largest D for which 48 theta^2 D^2 (1 + 8 D) <= tol (see bh_traverse).
double bh_near_dmax(double theta, double tol) {
    if (!(theta > 0.0)) return __builtin_inf();   // theta = 0: the reference opens every cell
    if (!(tol > 0.0)) return -1.0;
    double d = std::sqrt(tol / (48.0 * theta * theta));
    while (48.0 * theta * theta * d * d * (1.0 + 8.0 * d) > tol) d *= 0.99;
    return d;
}

// moment_count reads the nodes' cnt (after dup_apply's corrections),
// moment_items their bottom-up boxes: after the whole build, on stream ms
void bh_moments(BHTree &t, hipStream_t ms, int count_threads) {
    const int64_t n = t.n;
    hipLaunchKernelGGL(moment_count, dim3(ceil_div(n + 1, count_threads)), dim3(count_threads), 0, ms, t.nodes, n, t.meta,
                       t.mom_flag, t.mom_cnt, t.mom_list, t.meta, t.mom_off, t.mom_item);
    const int mgrid = (int)std::min<int64_t>(2048, std::max<int64_t>(1, ceil_div(n, 256)));
    hipLaunchKernelGGL(moment_items<true>, dim3(mgrid), dim3(256), 0, ms, t.pos, t.nodes, t.mom_off, n, t.mom_item,
                       t.mom_part, t.mom_cnt, t.mom);
    hipLaunchKernelGGL(moment_reduce, dim3(mgrid), dim3(256), 0, ms, t.meta, t.mom_list, t.mom_cnt, t.mom_off,
                       t.mom_part, t.mom);
}

void bh_build(tsne_ctx *ctx, BHTree &t, const double *dY, double theta, const int32_t *rowmap, bool root_tile_ok,
              double near_tol) {
    if (near_tol < 0.0) near_tol = bh_near_tol(ctx, false);
    t.near_dmax = bh_near_dmax(theta, near_tol);
    hipStream_t st = ctx->stream;
    const int64_t n = t.n;
    // the previous traversal's selection (second stream with Options::bh_chain)
    // is read from here on: trav_order_cur below, the next traversal pair.  At
    // the build's head the join is off both the iteration's chain and the
    // build -> traversal gap
    bh_select_join(ctx, t);
    t.rowmap = rowmap;
    t.root_tile = false;
    t.mom_deferred = false;
    const bool fuse_opt = ctx->opts.build_fuse != 0;
    if (!fuse_opt) TSNE_HIP(hipMemsetAsync(t.dflag, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(bbox_partial, dim3(t.bbox_blocks), dim3(256), 0, st, dY, n, t.bbox_part);
    hipLaunchKernelGGL(bbox_final, dim3(1), dim3(256), 0, st, t.bbox_part, t.bbox_blocks, t.W, t.meta, t.bb,
                       t.mom_flag, t.mom_off + n, fuse_opt ? t.dflag : nullptr);
    // once the box failed the root-tile test by 2^k (k >= 3), the next 4 (k - 2)
    // builds (<= 64) skip the test and its host read-back: the embedding
    // shrinks by a few % per iteration at most (C3: extent 1e-3 -> 9e-5 over
    // t = 10..100), and a skipped test only means the full build, whose sums
    // the root-tile path reproduces (performance, not results)
    if (root_tile_ok && t.rt_skip > 0) {
        --t.rt_skip;
        root_tile_ok = false;
    }
    if (root_tile_ok) {   // small read-backs decide the path (the host must know which kernels to launch)
        // the box conditions first (dflag still 0): once the embedding has
        // outgrown the root tile, the duplicate rounds (~90 us at 1M) are skipped
        hipLaunchKernelGGL(root_tile_check, dim3(1), dim3(1), 0, st, t.dflag, t.bb, t.W, n, theta, t.near_dmax,
                           t.status);
        TSNE_HIP(hipMemcpyAsync(t.status_h, t.status, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        TSNE_HIP(hipStreamSynchronize(st));
        if (!t.status_h[0]) {
            root_tile_ok = false;
            if (t.status_h[1] >= 3) t.rt_skip = std::min(64, 4 * (t.status_h[1] - 2));
        }
    }
    if (root_tile_ok) {
        const auto Y2 = reinterpret_cast<const double2 *>(dY);
        for (int r = 0; r < DUP_ROUNDS; ++r) {
            hipLaunchKernelGGL(dup_store, dim3(ceil_div(n, 256)), dim3(256), 0, st, Y2, n, t.dup_tab, t.dup_mask,
                               t.dup_open, r);
            hipLaunchKernelGGL(dup_probe, dim3(ceil_div(n, 256)), dim3(256), 0, st, Y2, n, t.dup_tab, t.dup_mask,
                               t.dup_open, r, t.dflag);
        }
        hipLaunchKernelGGL(root_tile_check, dim3(1), dim3(1), 0, st, t.dflag, t.bb, t.W, n, theta, t.near_dmax,
                           t.status);
        TSNE_HIP(hipMemcpyAsync(t.status_h, t.status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        TSNE_HIP(hipStreamSynchronize(st));
        if (t.status_h[0]) {
            t.root_tile = true;
            hipLaunchKernelGGL(root_tile_prep, dim3(std::min<int64_t>(1024, ceil_div(n, 256))), dim3(256), 0, st, t.bb,
                               n, t.nodes, t.mom_cnt, t.mom_off, t.mom_list, t.mom_item, t.meta, t.inv, t.idx_sorted,
                               t.mom_flag);
            const int mgrid = (int)std::min<int64_t>(2048, std::max<int64_t>(1, ceil_div(n, 256)));
            hipLaunchKernelGGL(moment_items<true>, dim3(mgrid), dim3(256), 0, st, Y2, t.nodes, t.mom_off, n,
                               t.mom_item, t.mom_part, nullptr, nullptr);
            hipLaunchKernelGGL(root_moment_reduce, dim3(MOM_K), dim3(256), 0, st, t.mom_off, n, t.mom_part, t.mom);
            hipLaunchKernelGGL(poly_coef, dim3(ceil_div(POLY_K, 128)), dim3(128), 0, st, t.mom, t.rcoef);
            t.root_pos = Y2;
            TSNE_LAUNCH_CHECK();
            return;
        }
        TSNE_HIP(hipMemsetAsync(t.dflag, 0, sizeof(int32_t), st));   // dup_count recomputes it
    }
    // Options::build_fuse on the coherent-sort path: the sort's own kernels compute the
    // keys and write what count_in_root, gather_sorted and dup_count write (csort.hpp)
    const bool csort = t.cs.P > 0 && t.cs_primed && ctx->opts.coherent_sort;
    const bool fuse = csort && ctx->opts.build_fuse;
    if (!fuse) {
        hipLaunchKernelGGL(morton_keys, dim3(ceil_div(n, 256)), dim3(256), 0, st, dY, n, t.W, t.keys, t.idx, t.meta);
        TSNE_LAUNCH_CHECK();
    }
    // the previous full build's order buckets the keys (csort.hpp); the first
    // build, small trees and Options::coherent_sort = 0: rocPRIM's sort (the same
    // result: keys ascending, ties by point index)
    if (fuse) {
        csort_run_fused2(ctx, t.cs, dY, t.W, t.idx_sorted, t.keys_sorted, t.idx_sorted,
                         Csort2Out{t.pos, t.inv, t.meta, t.dupc, t.vid, t.dflag}, st);
    } else if (csort) {
        csort_run(ctx, t.cs, t.keys, t.idx_sorted, t.keys_sorted, t.idx_sorted, st);
    } else {
        size_t tb = t.sort_tmp_bytes;
        morton_sort(t.sort_tmp, tb, t.keys, t.keys_sorted, t.idx, t.idx_sorted, n, st);
    }
    t.cs_primed = true;
    if (!fuse) hipLaunchKernelGGL(count_in_root, dim3(1), dim3(64), 0, st, t.keys_sorted, n, t.meta);
    // (trav_front_cur: predictions from the previous traversal's per-point costs,
    // the order made on the second stream while the build goes on)
    const bool cur_order = ctx->opts.trav_front_cur > 0.0 && t.pcost_valid && t.sel_waves == ceil_div(n, 64);
    if (!fuse || cur_order)   // (fused: only for the predictions)
        hipLaunchKernelGGL(gather_sorted, dim3(ceil_div(n, 256)), dim3(256), 0, st, dY, t.idx_sorted, n, t.pos, t.inv,
                           cur_order ? t.pcost : nullptr, cur_order ? t.pred : nullptr);
    t.order_ready = false;
    if (cur_order) {
        TSNE_HIP(hipEventRecord(ctx->aux_ev[0], st));
        TSNE_HIP(hipStreamWaitEvent(ctx->aux_stream, ctx->aux_ev[0], 0));
        hipLaunchKernelGGL(trav_order_cur, dim3(1), dim3(1024), 0, ctx->aux_stream, t.pred, t.nflag, ceil_div(n, 64),
                           ctx->opts.trav_front_cur, t.trav_order);
        if (!t.ord_ev) TSNE_HIP(hipEventCreateWithFlags(&t.ord_ev, hipEventDisableTiming));
        TSNE_HIP(hipEventRecord(t.ord_ev, ctx->aux_stream));
        t.order_ready = true;
    }
    if (!fuse)
        hipLaunchKernelGGL(dup_count, dim3(ceil_div(n, 256)), dim3(256), 0, st, t.pos, t.keys_sorted, n, t.dupc, t.vid,
                           t.dflag);
    if (++t.gen <= 0) {   // wrapped: clear the marks once
        TSNE_HIP(hipMemsetAsync(t.fstart, 0, sizeof(int32_t) * n, st));
        t.gen = 1;
    }
    hipLaunchKernelGGL(karras_build, dim3(ceil_div(n, 256)), dim3(256), 0, st, t.keys_sorted, n, t.meta,
                       t.nodes, t.parent_leaf, t.parent_node, t.arrive, t.arrive2, t.fstart, t.gen, t.top_cnt,
                       fuse ? t.meta + 1 : nullptr);
    const double inv_theta = theta > 0.0 ? 1.0 / theta : __builtin_inf();
    hipLaunchKernelGGL(bottom_up_intra, dim3(ceil_div(n, BU_NB)), dim3(BU_NB), 0, st, t.pos, t.meta, t.W, inv_theta,
                       t.nodes, t.agg, t.parent_leaf, t.parent_node, t.fstart, t.gen, t.top_list, t.top_cnt);
    hipLaunchKernelGGL(ctx->opts.bu_acqrel ? bottom_up_top<true> : bottom_up_top<false>,
                       dim3(std::max(1, ctx->cu_count * 4)), dim3(256), 0, st, t.pos, t.meta, t.W,
                       inv_theta, t.nodes, t.agg, t.parent_node, t.arrive, t.top_list, t.top_cnt);
    // exact duplicates: the reference's multiplicities (each kernel returns
    // at once unless dup_count saw a duplicate)
    hipLaunchKernelGGL(dup_bottom_up, dim3(ceil_div(n, 256)), dim3(256), 0, st, t.meta, t.dflag, t.idx_sorted, rowmap,
                       t.vid, t.nodes, t.parent_leaf, t.parent_node, t.arrive2, t.rmin, t.rvid, t.rt2, t.cntcorr,
                       t.sumcorr, t.tiecnt, t.notile, t.vflag, t.vcnt, t.vsum);
    hipLaunchKernelGGL(dup_fixup, dim3(ceil_div(n, 256)), dim3(256), 0, st, t.meta, t.dflag, t.pos, t.keys_sorted,
                       t.dupc, t.idx_sorted, rowmap, t.nodes, t.parent_leaf, t.parent_node, t.rt2, t.cntcorr,
                       t.sumcorr, t.tiecnt, t.notile, t.vflag, t.vcnt, t.vsum);
    hipLaunchKernelGGL(dup_apply, dim3(ceil_div(n, 256)), dim3(256), 0, st, t.meta, t.dflag, t.cntcorr, t.sumcorr,
                       t.vflag, t.vcnt, t.vsum, t.vcntf, t.vcom, t.nodes);
    const DupView dv{t.tiecnt, t.notile, t.vflag, t.vcntf, t.vcom, (int32_t)n};
    hipLaunchKernelGGL(build_qrec, dim3(ceil_div(n, 256)), dim3(256), 0, st, t.nodes, t.pos, t.meta, inv_theta,
                       t.near_dmax, t.dflag, dv, t.qrec);
    // subtree moments for the all-open fast path.  The traversal only records
    // which moments a query wants; their values are read by the kernels after it
    // (tile_apply, moment_apply, narrow_moment_apply).  With Options::build_fuse
    // the three kernels therefore leave the chain in front of the traversal:
    // bh_repulsion launches them on the second stream once the traversal is
    // enqueued, and joins before the first reader.
    t.mom_deferred = ctx->opts.build_fuse && ctx->aux_stream;
    if (!t.mom_deferred) bh_moments(t, st);
    TSNE_LAUNCH_CHECK();
}

}  // namespace tsne
