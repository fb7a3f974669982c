// optimize.hip -- gradient combine, updateEmbedding, centerEmbedding and the
// device-resident optimize loop (TsneHelpers.scala:221-430) on gfx950.
//
// Per global iteration t (1-based, TsneHelpers.scala:403-427 phases):
//   ex  = earlyExaggeration if t <= min(T,20) + min(T-20, 81) else 1
//   mom = initialMomentum if t <= min(T,20) else finalMomentum
//   1. quadtree of the full Y (every rank builds the identical tree), or the
//      root-tile shortcut while the embedding is small (bhtree_build.hip)
//   2. BH repulsion for this rank's own points (its query list)
//   3. Z = sum z (TsneHelpers.scala:266): the per-iteration all-reduce
//   4. attraction per owned row of P over the CSR row (q = 1/(1+metric(y_i,
//      y_j)), TsneHelpers.scala:290-302; side stream outside loss
//      iterations), loss terms every 10th iteration, then combine_update:
//      grad = attr - F/Z (:311-317), gains/momentum/step (:341-369) -> Ynew
//   5. [multi-GPU] ragged all-gather of the owned Ynew slices
//   6. centre: Y = Ynew - mean(Ynew) (:320-329)
//
// Internal labels.  The optimizer keeps its own copy of P (full, every rank)
// and of the working set, indexed by internal point labels: P's graph order
// at setup (connected components, BFS levels), then every RELABEL_EVERY
// iterations the current Morton order of the embedding when that keeps more
// of P's edges local -- rows consecutive in memory gather Y_j from nearby
// labels, so the CSR attraction's gathers hit the L2.  Rank r owns a range of
// labels (cost-balanced cuts at relabels).  The caller's Y, upd and gains
// are written back in the original order by tsne_dev_opt_sync.
#include <hipcub/hipcub.hpp>

#include "attract.hpp"
#include "bhtree.hpp"
#include "octree.hpp"

namespace tsne {

struct OptState {
    tsne_params p{};
    int C = 2;
    int64_t n = 0, nnz = 0;
    // caller buffers (original order, n x C)
    double *Yu = nullptr, *updu = nullptr, *gainsu = nullptr;
    // the caller's P (original point order, every rank holds it), copied once
    int64_t *rp0 = nullptr;
    int32_t *col0 = nullptr;
    double *val0 = nullptr;
    // 2-D: this rank's rows (labels [L0, L1)) with columns in labels, rebuilt
    // from P0 at every relabel; row pointer local (rpw[r] for label L0 + r)
    int64_t *rpw = nullptr;
    int32_t *colw = nullptr;
    double *valw = nullptr;
    // labels: working set in label order (full n on every rank; upd / gains
    // are current on a rank only for its own labels between relabels)
    double *Y[2] = {nullptr, nullptr}, *upd[2] = {nullptr, nullptr}, *gains[2] = {nullptr, nullptr};
    int32_t *orig[2] = {nullptr, nullptr};   // label -> original index
    int32_t *lab = nullptr;                  // original index -> label
    int cur = 0;
    std::vector<int64_t> own;                // world + 1 label cuts (identical on every rank)
    int64_t L0 = 0, L1 = 0;
    int64_t *rowlen = nullptr;
    void *scan_tmp = nullptr;
    size_t scan_tmp_bytes = 0;
    int32_t *qlist = nullptr, *qcnt = nullptr, *qoff = nullptr;   // world > 1: this rank's BH queries
    void *qscan_tmp = nullptr;
    size_t qscan_tmp_bytes = 0;
    unsigned long long *lscore = nullptr;    // locality_score counters
    int relabels = 0, relabel_checks = 0;

    double *Ynew = nullptr;   // n x C (label order)
    double2 *F = nullptr;     // n, sorted order
    double2 *attr = nullptr;  // owned rows
    unsigned long long *bcost = nullptr;   // 256-position bucket costs of the last traversal
    int64_t *bounds = nullptr;             // world + 1 (device): cost-balanced cuts
    double *z = nullptr;      // n, sorted order
    double *scal = nullptr;   // [0] Z, [1] loss, [2..4] mean
    double *part = nullptr;   // reduction partials
    double *part2 = nullptr;  // second-level partials (NPART)
    double *loss = nullptr;   // per loss slot
    int32_t loss_slots = 0;
    std::vector<int32_t> loss_written;
    unsigned long long *visits = nullptr;
    BHTree tree;
    // 3-D embeddings (nComponents = 3, the SURVEY.md 8f octree extension):
    // labels stay the original indices (no relabel); owned rows are read
    // straight from P0; F3 (n x 3, sorted order) and attr3 (owned x 3).
    OctTree otree;
    double *F3 = nullptr, *attr3 = nullptr;
    bool profile = false;
    hipEvent_t ev[6] = {};
    // The attraction sums need only Y and P (not F or Z), so outside loss
    // iterations they run on a second stream concurrently with the BH
    // traversal (a latency-bound kernel that leaves CUs idle).
    hipStream_t side = nullptr;
    hipEvent_t ev_y = nullptr, ev_attr = nullptr;
    // per launch of the attraction kernel (ctx->timers "opt.attract"): its
    // iteration and whether it ran alone on the main stream (loss iterations)
    // or on the side stream concurrently with the BH traversal
    // (kept in step with the stage timer: its last StageTimers::CAP launches)
    std::deque<std::pair<int32_t, int32_t>> attract_iter;
    void log_attract(int32_t t, int32_t kind) {
        attract_iter.push_back({t, kind});
        while (attract_iter.size() > StageTimers::CAP) attract_iter.pop_front();
    }
    double *mpart = nullptr;  // centring mean: block partials of combine_update
    AttractLayout at;   // tiled attraction layout of the owned rows, rebuilt with them
    bool morton_labels = false;   // the labels follow the embedding's Morton order (a relabel happened)
    double last_ms[5] = {0, 0, 0, 0, 0};
    int64_t last_visits[10] = {};
    int64_t last_mhz = 0;   // the traced traversal's waves' shader clock (MHz)
    // tree partition (Options::bh_split, several ranks, 2-D): cuts of the sorted
    // points (world + 1), this rank's aligned [lo, hi) + overflow flag, the
    // ranks' traversal costs (all-reduced), F in label order (reduce-scatter)
    int64_t *pcuts = nullptr;
    int32_t *plim = nullptr;
    unsigned long long *pcost = nullptr;
    double2 *Fl = nullptr;
    bool split_last = false;   // the last iteration used the tree partition
};

// The sharded code path (query lists, collectives, centring from the gathered
// embedding) runs whenever the context has a communicator: world > 1, or a
// world-1 communicator made with Options::comm_world1 (transport tests).
static inline bool sharded(const tsne_ctx *ctx) { return ctx->comm != nullptr; }

namespace {

constexpr int NPART = 512;
constexpr int RELABEL_EVERY = 25;

__device__ __forceinline__ double jmax(double a, double b) {  // java.lang.Math.max
    if (a != a) return a;
    if (b != b) return b;
    return a >= b ? a : b;
}

// Deterministic sum of v[0..n) (stride elements, component c) into part[block].
__global__ void reduce_partial(const double *__restrict__ v, int64_t n, int stride, int c,
                               double *__restrict__ part) {
    __shared__ double sw[4];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        s += v[i * stride + c];
    s = wave_sum(s);
    if (lane_id() == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sw[0] + sw[1]) + (sw[2] + sw[3]);
}

// Sum of v[0 .. *np) into NPART block partials (reduce_partial with a device count).
__global__ void reduce_partial_devn(const double *__restrict__ v, const int64_t *__restrict__ np,
                                    double *__restrict__ part) {
    __shared__ double sw[4];
    const int64_t n = *np;
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        s += v[i];
    s = wave_sum(s);
    if (lane_id() == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sw[0] + sw[1]) + (sw[2] + sw[3]);
}

// Z-free KL terms: the kernels summed P ln(P (1 + metric)); the loss adds
// ln(Z) sum p (p = ex P over this rank's owned entries, sum P in scal[6])
// once Z is known.
__global__ void loss_add_lnz(double *scal, double ex) {
    if (threadIdx.x == 0) scal[1] += log(scal[0]) * (scal[6] * ex);
}
__global__ void set_unit(double *x) {
    if (threadIdx.x == 0) *x = 1.0;
}

__global__ void reduce_final(const double *__restrict__ part, int np, double *__restrict__ out,
                             double scale_div) {
    __shared__ double sw[4];
    double s = 0.0;
    for (int b = threadIdx.x; b < np; b += blockDim.x) s += part[b];
    s = wave_sum(s);
    if (lane_id() == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = (sw[0] + sw[1]) + (sw[2] + sw[3]);
        *out = scale_div > 0.0 ? t / scale_div : t;
    }
}

// grad = attr - F / Z (TsneHelpers.scala:311-317); MODE 0 writes it, MODE 1
// applies updateEmbedding (TsneHelpers.scala:341-369) -> Ynew.  One thread
// per row, all accesses coalesced except F[inv[i]] (near-identity gather).
// With `mpart` (MODE 1) each block also writes the sum of its rows' Ynew
// (x, y) to mpart[2 * block]: the centring mean's partials, fused into the
// update so that centerEmbedding costs one more pass (center2); the
// mean itself is mean2_final (finalising it in the last block instead saved a
// launch but cost 3,907 same-address arrival atomics: 0.062 -> 0.085 ms).
template <int MODE>
__global__ __launch_bounds__(256) void combine_update(
    int64_t r0, int64_t r1, const double2 *__restrict__ attr, const int32_t *__restrict__ inv,
    const double2 *__restrict__ F, const double *__restrict__ scal, const double *__restrict__ Y,
    double *__restrict__ grad, double *__restrict__ Ynew, double *__restrict__ upd, double *__restrict__ gains,
    double min_gain, double mom, double lr, double *__restrict__ mpart) {
    __shared__ double sm[2][4];
    const int64_t i = r0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < r1;
    double yn[2] = {0.0, 0.0};
    if (live) {
        const double Z = scal[0];
        const double2 at = attr[i - r0];
        const double2 f = F[inv ? inv[i] : i];   // sorted order, or already by label (inv = nullptr)
        const double gx = at.x - f.x / Z, gy = at.y - f.y / Z;  // attrForce - repForce / sumQ
        if (MODE == 0) {
            grad[2 * i] = gx;
            grad[2 * i + 1] = gy;
        } else {
            const double g[2] = {gx, gy};
            const double2 u2 = *reinterpret_cast<const double2 *>(upd + 2 * i);
            const double2 g2 = *reinterpret_cast<const double2 *>(gains + 2 * i);
            const double2 y2 = *reinterpret_cast<const double2 *>(Y + 2 * i);
            const double uu[2] = {u2.x, u2.y}, gg[2] = {g2.x, g2.y}, yy[2] = {y2.x, y2.y};
            double un[2], gn[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                gn[c] = ((g[c] > 0.0) == (uu[c] > 0.0)) ? jmax(gg[c] * 0.8, min_gain) : jmax(gg[c] + 0.2, min_gain);
                un[c] = __dsub_rn(__dmul_rn(mom, uu[c]), __dmul_rn(__dmul_rn(lr, gn[c]), g[c]));
                yn[c] = __dadd_rn(un[c], yy[c]);
            }
            *reinterpret_cast<double2 *>(gains + 2 * i) = make_double2(gn[0], gn[1]);
            *reinterpret_cast<double2 *>(upd + 2 * i) = make_double2(un[0], un[1]);
            *reinterpret_cast<double2 *>(Ynew + 2 * i) = make_double2(yn[0], yn[1]);
        }
    }
    if (MODE == 1 && mpart) {
        const double sx = wave_sum(yn[0]), sy = wave_sum(yn[1]);
        if (lane_id() == 0) { sm[0][threadIdx.x >> 6] = sx; sm[1][threadIdx.x >> 6] = sy; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const double px = (sm[0][0] + sm[0][1]) + (sm[0][2] + sm[0][3]);
            const double py = (sm[1][0] + sm[1][1]) + (sm[1][2] + sm[1][3]);
            mpart[2 * blockIdx.x] = px;
            mpart[2 * blockIdx.x + 1] = py;
        }
    }
}

// mean[c] = (sum of the nb block partials of component c, fixed order) / n
__global__ __launch_bounds__(256) void mean2_final(const double *__restrict__ mpart, int64_t nb, double n,
                                                   double *__restrict__ mean) {
    __shared__ double sm[2][4];
    double s[2] = {0.0, 0.0};
    for (int64_t b = threadIdx.x; b < nb; b += blockDim.x) { s[0] += mpart[2 * b]; s[1] += mpart[2 * b + 1]; }
    s[0] = wave_sum(s[0]);
    s[1] = wave_sum(s[1]);
    if (lane_id() == 0) { sm[0][threadIdx.x >> 6] = s[0]; sm[1][threadIdx.x >> 6] = s[1]; }
    __syncthreads();
    if (threadIdx.x < 2) mean[threadIdx.x] = ((sm[threadIdx.x][0] + sm[threadIdx.x][1]) + (sm[threadIdx.x][2] + sm[threadIdx.x][3])) / n;
}

// centerEmbedding (TsneHelpers.scala:320-329): Y = Ynew - mean, label order.
// The caller's copy (original point order) is written by tsne_dev_opt_sync
// (opt_sync), not here: its scattered 16-byte writes were a third of the
// update's HBM traffic per iteration (round 4: 69 of 250 MB).
__global__ __launch_bounds__(256) void center2(const double *__restrict__ Ynew, int64_t n,
                                               const double *__restrict__ mean, double *__restrict__ Y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double2 v = *reinterpret_cast<const double2 *>(Ynew + 2 * i);
    *reinterpret_cast<double2 *>(Y + 2 * i) = make_double2(v.x - mean[0], v.y - mean[1]);
}

__global__ void center_apply(const double *__restrict__ src, int64_t n, int32_t c,
                             const double *__restrict__ mean, double *__restrict__ dst) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * c) return;
    dst[e] = src[e] - mean[e % c];
}

__global__ void update_kernel(int64_t ne, const double *__restrict__ grad, double *__restrict__ Y,
                              double *__restrict__ upd, double *__restrict__ gains, double min_gain,
                              double mom, double lr) {
    int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= ne) return;
    const double g = grad[o], u = upd[o], gn0 = gains[o];
    const double gn = ((g > 0.0) == (u > 0.0)) ? jmax(gn0 * 0.8, min_gain) : jmax(gn0 + 0.2, min_gain);
    const double un = __dsub_rn(__dmul_rn(mom, u), __dmul_rn(__dmul_rn(lr, gn), g));
    gains[o] = gn;
    upd[o] = un;
    Y[o] = __dadd_rn(un, Y[o]);
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// N(0, 1e-4^2) by Box-Muller on a counter-based stream keyed by seed.
__global__ void init_ws_kernel(int64_t ne, uint64_t seed, double *__restrict__ Y,
                               double *__restrict__ upd, double *__restrict__ gains) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    const uint64_t a = splitmix64(seed ^ splitmix64(2 * (uint64_t)e));
    const uint64_t b = splitmix64(seed ^ splitmix64(2 * (uint64_t)e + 1));
    const double u1 = ((double)(a >> 11) + 1.0) * 0x1.0p-53;
    const double u2 = (double)(b >> 11) * 0x1.0p-53;
    Y[e] = 1e-4 * sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
    upd[e] = 0.0;
    gains[e] = 1.0;
}

// ---- internal labels
__global__ void iota_i32(int32_t *p, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = (int32_t)i;
}

// new label s <- old label order[s]: working set (C components) and the label
// maps orig1 (label -> original point) and lab (original point -> label)
__global__ void relabel_state(const int32_t *__restrict__ order, int64_t n, int C, const double *__restrict__ Y0,
                              const double *__restrict__ u0, const double *__restrict__ g0,
                              const int32_t *__restrict__ o0, double *__restrict__ Y1, double *__restrict__ u1,
                              double *__restrict__ g1, int32_t *__restrict__ o1, int32_t *__restrict__ lab) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int64_t i = order[s];
    for (int c = 0; c < C; ++c) {
        Y1[C * s + c] = Y0[C * i + c];
        u1[C * s + c] = u0[C * i + c];
        g1[C * s + c] = g0[C * i + c];
    }
    const int32_t o = o0[i];
    o1[s] = o;
    lab[o] = (int32_t)s;
}

// Row lengths of the owned labels [L0, L1) from the caller's P (original order)
__global__ void own_rowlen(const int32_t *__restrict__ orig, const int64_t *__restrict__ rp0, int64_t L0, int64_t L1,
                           int64_t *__restrict__ len) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > L1 - L0) return;
    if (r == L1 - L0) { len[r] = 0; return; }
    const int64_t o = orig[L0 + r];
    len[r] = rp0[o + 1] - rp0[o];
}

// One wave per owned row: the caller's row of its original point, columns
// renamed into labels (entry order kept: the attraction sums run in the
// reference's row order whatever the labelling).
__global__ void own_rows(const int32_t *__restrict__ orig, const int32_t *__restrict__ lab,
                         const int64_t *__restrict__ rp0, const int32_t *__restrict__ c0,
                         const double *__restrict__ v0, int64_t L0, int64_t L1, const int64_t *__restrict__ rpw,
                         int32_t *__restrict__ cw, double *__restrict__ vw) {
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (r >= L1 - L0) return;
    const int64_t o = orig[L0 + r];
    const int64_t a = rp0[o], len = rp0[o + 1] - a, b = rpw[r];
    for (int64_t e = lane_id(); e < len; e += 64) {
        cw[b + e] = lab[c0[a + e]];
        vw[b + e] = v0[a + e];
    }
}

// This rank's queries: the sorted positions whose label it owns, ascending
// (a stable compaction: flags, block counts, scan, scatter).
__global__ void qlist_count(const int32_t *__restrict__ idx_sorted, int64_t n, int64_t L0, int64_t L1,
                            int32_t *__restrict__ bcnt) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool f = s < n && idx_sorted[s] >= L0 && idx_sorted[s] < L1;
    __shared__ int wc[4];
    const int c = __popcll(__ballot(f));
    if (lane_id() == 0) wc[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) bcnt[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}
__global__ void qlist_fill(const int32_t *__restrict__ idx_sorted, int64_t n, int64_t L0, int64_t L1,
                           const int32_t *__restrict__ boff, int32_t *__restrict__ qlist) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool f = s < n && idx_sorted[s] >= L0 && idx_sorted[s] < L1;
    __shared__ int wc[4];
    const uint64_t bal = __ballot(f);
    if (lane_id() == 0) wc[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    const int w = threadIdx.x >> 6;
    int base = boff[blockIdx.x];
    for (int k = 0; k < w; ++k) base += wc[k];
    if (f) qlist[base + __popcll(bal & lanemask_lt())] = (int32_t)s;
}

// F in label order: Fl[l] = F[inv[l]] (the tree partition's reduce-scatter
// buffer: each rank's partial sums of every point, summed at the row owners)
__global__ void f_to_label(const int32_t *__restrict__ inv, int64_t n, const double2 *__restrict__ F,
                           double2 *__restrict__ Fl) {
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l < n) Fl[l] = F[inv[l]];
}

// Z partial of a rank: sum of z over its query list (fixed order per block)
__global__ void reduce_list_partial(const double *__restrict__ z, const int32_t *__restrict__ qlist, int64_t m,
                                    double *__restrict__ part) {
    __shared__ double sw[4];
    double acc = 0.0;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (int64_t)gridDim.x * blockDim.x)
        acc += z[qlist[k]];
    acc = wave_sum(acc);
    if (lane_id() == 0) sw[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sw[0] + sw[1]) + (sw[2] + sw[3]);
}

// ---- locality of the CSR attraction's gathers (relabel decisions)
// Connected components (minimum original index) and BFS level from that
// root over the symmetric P: fixpoint iterations, deterministic.
__global__ void cc_pull(const int64_t *__restrict__ rp, const int32_t *__restrict__ col, int64_t n,
                        int32_t *__restrict__ comp, int32_t *__restrict__ changed) {
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (i >= n) return;
    int32_t m = comp[i];
    for (int64_t e = rp[i] + lane_id(); e < rp[i + 1]; e += 64) m = min(m, comp[col[e]]);
    m = wave_min(m);
    if (lane_id() == 0 && m < comp[i]) {
        atomicMin(&comp[i], m);
        changed[0] = 1;
    }
}
__global__ void cc_jump(int32_t *__restrict__ comp, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    comp[i] = comp[comp[comp[i]]];
}
__global__ void level_init(const int32_t *__restrict__ comp, int64_t n, int32_t *__restrict__ lev) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) lev[i] = comp[i] == (int32_t)i ? 0 : INT32_MAX;
}
__global__ void level_pull(const int64_t *__restrict__ rp, const int32_t *__restrict__ col, int64_t n,
                           int32_t *__restrict__ lev, int32_t *__restrict__ changed) {
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (i >= n) return;
    int32_t m = INT32_MAX;
    for (int64_t e = rp[i] + lane_id(); e < rp[i + 1]; e += 64) m = min(m, lev[col[e]]);
    m = wave_min(m);
    if (lane_id() == 0 && m != INT32_MAX && m + 1 < lev[i]) {
        atomicMin(&lev[i], m + 1);
        changed[0] = 1;
    }
}
__global__ void graph_keys(const int32_t *__restrict__ comp, const int32_t *__restrict__ lev, int64_t n,
                           uint64_t *__restrict__ key, int32_t *__restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    key[i] = ((uint64_t)(uint32_t)comp[i] << 24) | (uint64_t)min(lev[i], (1 << 24) - 1);
    val[i] = (int32_t)i;
}

// Fraction of P's edges (a fixed sample of rows) whose endpoints lie within
// `win` labels of each other: under the current labels (cnt[0]) and under the
// Morton order of this iteration's tree (cnt[1]: label l -> inv[l]).
__global__ void locality_score(const int64_t *__restrict__ rp0, const int32_t *__restrict__ c0,
                               const int32_t *__restrict__ lab, const int32_t *__restrict__ inv, int64_t n,
                               int64_t stride, int64_t nsamp, int64_t win, unsigned long long *__restrict__ cnt) {
    const int64_t k = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (k >= nsamp) return;
    const int64_t o = k * stride;
    const int64_t li = lab[o], mi = inv[li];
    unsigned long long a = 0, b = 0;
    for (int64_t e = rp0[o] + lane_id(); e < rp0[o + 1]; e += 64) {
        const int64_t lj = lab[c0[e]];
        const int64_t da = li - lj, db = mi - (int64_t)inv[lj];
        a += (da <= win && -da <= win);
        b += (db <= win && -db <= win);
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane_id() == 0) { atomicAdd(cnt, a); atomicAdd(cnt + 1, b); }
}

// dst[orig[i]] = src[i], c components
__global__ void scatter_to_user_c(const double *__restrict__ src, const int32_t *__restrict__ orig, int64_t n,
                                  int32_t c, double *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t o = orig[i];
    for (int k = 0; k < c; ++k) dst[c * o + k] = src[c * i + k];
}

// ---- 3-D (nComponents = 3) optimizer kernels
// grad = attr - F / Z, then (MODE 1) updateEmbedding -> Ynew (3 components).
// With `mpart` (MODE 1, one rank) each block also writes the sums of its
// rows' Ynew to mpart[3 * block + c]: the centring mean's partials, as
// combine_update in 2-D (meanC_final, center3_scatter).
template <int MODE>
__global__ __launch_bounds__(256) void combine_update3(int64_t r0, int64_t r1, const double *__restrict__ attr,
                                                       const int32_t *__restrict__ inv, const double *__restrict__ F,
                                                       const double *__restrict__ scal, const double *__restrict__ Y,
                                                       double *__restrict__ grad, double *__restrict__ Ynew,
                                                       double *__restrict__ upd, double *__restrict__ gains,
                                                       double min_gain, double mom, double lr,
                                                       double *__restrict__ mpart) {
    __shared__ double sm[3][4];
    const int64_t i = r0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double yn[3] = {0.0, 0.0, 0.0};
    if (i < r1) {
        const double Z = scal[0];
        const int64_t si = inv[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double g = attr[3 * (i - r0) + c] - F[3 * si + c] / Z;
            const int64_t o = 3 * i + c;
            if (MODE == 0) { grad[o] = g; continue; }
            const double u = upd[o], gn0 = gains[o];
            const double gn = ((g > 0.0) == (u > 0.0)) ? jmax(gn0 * 0.8, min_gain) : jmax(gn0 + 0.2, min_gain);
            const double un = __dsub_rn(__dmul_rn(mom, u), __dmul_rn(__dmul_rn(lr, gn), g));
            gains[o] = gn;
            upd[o] = un;
            yn[c] = __dadd_rn(un, Y[o]);
            Ynew[o] = yn[c];
        }
    }
    if (MODE == 1 && mpart) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = wave_sum(yn[c]);
            if (lane_id() == 0) sm[c][threadIdx.x >> 6] = v;
        }
        __syncthreads();
        if (threadIdx.x < 3)
            mpart[3 * blockIdx.x + threadIdx.x] =
                (sm[threadIdx.x][0] + sm[threadIdx.x][1]) + (sm[threadIdx.x][2] + sm[threadIdx.x][3]);
    }
}

// mean[c] = (sum of the nb block partials mpart[3 b + c], fixed order) / n
__global__ __launch_bounds__(256) void mean3_final(const double *__restrict__ mpart, int64_t nb, double n,
                                                   double *__restrict__ mean) {
    __shared__ double sm[3][4];
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t b = threadIdx.x; b < nb; b += blockDim.x)
        for (int c = 0; c < 3; ++c) s[c] += mpart[3 * b + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v = wave_sum(s[c]);
        if (lane_id() == 0) sm[c][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3)
        mean[threadIdx.x] = ((sm[threadIdx.x][0] + sm[threadIdx.x][1]) + (sm[threadIdx.x][2] + sm[threadIdx.x][3])) / n;
}

// centerEmbedding (TsneHelpers.scala:320-329), 3-D: Y = Ynew - mean (the
// caller's copy at tsne_dev_opt_sync, as in 2-D)
__global__ __launch_bounds__(256) void center3(const double *__restrict__ Ynew, int64_t n,
                                               const double *__restrict__ mean, double *__restrict__ Y) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 3 * n) return;
    Y[e] = Ynew[e] - mean[e % 3];
}

template <int MODE>
static void combine_launch(hipStream_t st, int64_t r0, int64_t r1, const double2 *attr, const int32_t *inv,
                           const double2 *F, const double *scal, const double *Y, double *grad, double *Ynew,
                           double *upd, double *gains, double min_gain, double mom, double lr,
                           double *mpart = nullptr) {
    if (r1 <= r0) return;
    hipLaunchKernelGGL(combine_update<MODE>, dim3(ceil_div(r1 - r0, 256)), dim3(256), 0, st, r0, r1, attr, inv, F,
                       scal, Y, grad, Ynew, upd, gains, min_gain, mom, lr, mpart);
}

}  // namespace

// ------------------------------------------------------------ single ops

void update_device(tsne_ctx *ctx, int64_t n, int32_t c, const double *dgrad, double *dY,
                   double *dupd, double *dgains, double min_gain, double momentum, double lr) {
    const int64_t ne = n * c;
    if (ne <= 0) return;
    hipLaunchKernelGGL(update_kernel, dim3(ceil_div(ne, 256)), dim3(256), 0, ctx->stream, ne, dgrad,
                       dY, dupd, dgains, min_gain, momentum, lr);
    TSNE_LAUNCH_CHECK();
}

void center_device(tsne_ctx *ctx, int64_t n, int32_t c, double *dY) {
    if (n <= 0) return;
    TSNE_REQUIRE(c >= 1 && c <= 8, "n_components out of range");
    double *part = ctx->ws.get<double>("ctr.part", NPART);
    double *mean = ctx->ws.get<double>("ctr.mean", 8);
    double *tmp = ctx->ws.get<double>("ctr.tmp", (size_t)n * c);
    for (int k = 0; k < c; ++k) {
        hipLaunchKernelGGL(reduce_partial, dim3(NPART), dim3(256), 0, ctx->stream, dY, n, c, k, part);
        hipLaunchKernelGGL(reduce_final, dim3(1), dim3(256), 0, ctx->stream, part, NPART, mean + k, (double)n);
    }
    TSNE_HIP(hipMemcpyAsync(tmp, dY, sizeof(double) * n * c, hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(center_apply, dim3(ceil_div(n * c, 256)), dim3(256), 0, ctx->stream, tmp, n, c, mean, dY);
    TSNE_LAUNCH_CHECK();
}

void init_working_set_device(tsne_ctx *ctx, int64_t n, int32_t c, uint64_t seed, double *dY,
                             double *dupd, double *dgains) {
    const int64_t ne = n * c;
    if (ne <= 0) return;
    hipLaunchKernelGGL(init_ws_kernel, dim3(ceil_div(ne, 256)), dim3(256), 0, ctx->stream, ne, seed, dY,
                       dupd, dgains);
    TSNE_LAUNCH_CHECK();
}

// The root-tile shortcut of bh_build while the embedding is small
// (Options::root_tile = 0: always the full tree).
static bool root_tile_enabled(const tsne_ctx *ctx) { return ctx->opts.root_tile != 0; }

void gradient_device(tsne_ctx *ctx, const int64_t *d_row_ptr, const int32_t *d_col,
                     const double *d_P, int64_t n, const double *dY, int32_t metric, double theta,
                     double exaggeration, double *d_grad, double *h_sumq, double *h_loss) {
    TSNE_REQUIRE(n >= 1, "empty embedding");
    hipStream_t st = ctx->stream;
    BHTree &t = bh_single_tree(ctx, n);
    bh_build(ctx, t, dY, theta, nullptr, root_tile_enabled(ctx));
    double2 *F = ctx->ws.get<double2>("grad.F", n);
    double *z = ctx->ws.get<double>("grad.z", n);
    double *part = ctx->ws.get<double>("grad.part", NPART);
    double *scal = ctx->ws.get<double>("grad.scal", 4);
    bh_repulsion(ctx, t, theta, 0, n, F, z, nullptr);
    hipLaunchKernelGGL(reduce_partial, dim3(NPART), dim3(256), 0, st, z, n, 1, 0, part);
    hipLaunchKernelGGL(reduce_final, dim3(1), dim3(256), 0, st, part, NPART, scal, 0.0);
    double *lpart = ctx->ws.get<double>("grad.lpart", attract_max_blocks(n));
    const bool want_loss = h_loss != nullptr;
    double2 *attr = ctx->ws.get<double2>("grad.attr", n);
    AttractArgs aa{d_row_ptr, d_col, d_P, 0, n, dY, scal, metric, exaggeration, attr, lpart};
    const int64_t blocks = attract_launch_2d(st, AttractLayout{}, aa, want_loss);   // no layout: attract_rows
    combine_launch<0>(st, 0, n, attr, t.inv, F, scal, dY, d_grad, nullptr, nullptr, nullptr, 0.0, 0.0, 0.0);
    TSNE_LAUNCH_CHECK();
    if (want_loss) {   // two-level: block partials -> NPART -> 1
        hipLaunchKernelGGL(reduce_partial, dim3(NPART), dim3(256), 0, st, lpart, blocks, 1, 0, part);
        hipLaunchKernelGGL(reduce_final, dim3(1), dim3(256), 0, st, part, NPART, scal + 1, 0.0);
    }
    double hs[2] = {0, 0};
    TSNE_HIP(hipMemcpyAsync(hs, scal, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    TSNE_HIP(hipStreamSynchronize(st));
    if (h_sumq) *h_sumq = hs[0];
    if (h_loss) *h_loss = hs[1];
}

// per-point results from sorted order back to the original order
__global__ void unsort_fz(const int32_t *__restrict__ inv, int64_t n, int c, const double *__restrict__ Fs,
                          const double *__restrict__ zs, double *__restrict__ Fo, double *__restrict__ zo) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t si = inv[i];
    for (int k = 0; k < c; ++k) Fo[c * i + k] = Fs[c * si + k];
    zo[i] = zs[si];
}

// QuadTree.computeRepulsiveForce (QuadTree.scala:123-152) for every point of
// Y against the tree of all of them (c = 2), or the octree extension (c = 3):
// F (n x c) and z (sumQ contribution) per point, original order.
void repulsion_device(tsne_ctx *ctx, const double *dY, int64_t n, int32_t c, double theta, double *dF,
                      double *dz) {
    TSNE_REQUIRE(n >= 1, "empty embedding");
    hipStream_t st = ctx->stream;
    double *Fs = ctx->ws.get<double>("rep.F", (size_t)c * n);
    double *zs = ctx->ws.get<double>("rep.z", n);
    const int32_t *inv;
    if (c == 2) {
        BHTree &t = bh_single_tree(ctx, n);
        bh_build(ctx, t, dY, theta, nullptr, root_tile_enabled(ctx));
        unsigned long long *vis = nullptr;   // Options::rep_stats: the counting traversal
        if (ctx->opts.rep_stats) {
            vis = ctx->ws.get<unsigned long long>("rep.visits", VIS_N);
            TSNE_HIP(hipMemsetAsync(vis, 0, sizeof(unsigned long long) * VIS_N, st));
            if (ctx->opts.wave_log)   // (the log's count; bh_repulsion takes the buffer)
                TSNE_HIP(hipMemsetAsync(ctx->ws.get<unsigned long long>("rep.wavelog", 1), 0, 8, st));
        }
        bh_repulsion(ctx, t, theta, 0, n, reinterpret_cast<double2 *>(Fs), zs, vis);
        inv = t.inv;
    } else {
        OctTree t;
        oct_alloc(ctx, t, n, "oct1.");
        oct_build(ctx, t, dY, theta);
        oct_repulsion(ctx, t, theta, 0, n, Fs, zs);
        inv = t.inv;
    }
    hipLaunchKernelGGL(unsort_fz, dim3(ceil_div(n, 256)), dim3(256), 0, st, inv, n, c, Fs, zs, dF, dz);
    TSNE_LAUNCH_CHECK();
}

int64_t opt_wave_mhz(tsne_ctx *ctx) { return ctx->opt ? ctx->opt->last_mhz : 0; }

// 3-D gradient (octree): same contract as gradient_device, Y / grad n x 3.
void gradient3_device(tsne_ctx *ctx, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_P, int64_t n,
                      const double *dY, int32_t metric, double theta, double exaggeration, double *d_grad,
                      double *h_sumq, double *h_loss) {
    TSNE_REQUIRE(n >= 1, "empty embedding");
    hipStream_t st = ctx->stream;
    OctTree t;
    oct_alloc(ctx, t, n, "oct1.");
    oct_build(ctx, t, dY, theta);
    double *F = ctx->ws.get<double>("grad3.F", 3 * (size_t)n);
    double *z = ctx->ws.get<double>("grad.z", n);
    double *part = ctx->ws.get<double>("grad.part", NPART);
    double *scal = ctx->ws.get<double>("grad.scal", 4);
    oct_repulsion(ctx, t, theta, 0, n, F, z);
    hipLaunchKernelGGL(reduce_partial, dim3(NPART), dim3(256), 0, st, z, n, 1, 0, part);
    hipLaunchKernelGGL(reduce_final, dim3(1), dim3(256), 0, st, part, NPART, scal, 0.0);
    const bool want_loss = h_loss != nullptr;
    double *lpart = ctx->ws.get<double>("grad3.lpart", attract3_blocks(n));
    double *attr = ctx->ws.get<double>("grad3.attr", 3 * (size_t)n);
    AttractArgs aa{d_row_ptr, d_col, d_P, 0, n, dY, scal, metric, exaggeration, nullptr, lpart};
    const int64_t blocks = attract_launch_3d(st, AttractLayout{}, aa, attr, want_loss);   // no layout: attract3
    hipLaunchKernelGGL(combine_update3<0>, dim3(ceil_div(n, 256)), dim3(256), 0, st, 0, n, attr, t.inv, F, scal, dY,
                       d_grad, nullptr, nullptr, nullptr, 0.0, 0.0, 0.0, nullptr);
    TSNE_LAUNCH_CHECK();
    if (want_loss) {
        hipLaunchKernelGGL(reduce_partial, dim3(NPART), dim3(256), 0, st, lpart, blocks, 1, 0, part);
        hipLaunchKernelGGL(reduce_final, dim3(1), dim3(256), 0, st, part, NPART, scal + 1, 0.0);
    }
    double hs[2] = {0, 0};
    TSNE_HIP(hipMemcpyAsync(hs, scal, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    TSNE_HIP(hipStreamSynchronize(st));
    if (h_sumq) *h_sumq = hs[0];
    if (h_loss) *h_loss = hs[1];
}

// ------------------------------------------------------------ optimizer

void opt_destroy(tsne_ctx *ctx) {
    if (!ctx->opt) return;
    OptState *s = ctx->opt;
    for (auto &e : s->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {s->ev_y, s->ev_attr})
        if (e) (void)hipEventDestroy(e);
    if (s->side) {
        (void)hipStreamSynchronize(s->side);
        (void)hipStreamDestroy(s->side);
    }
    // (the tree's last narrow_select may still run there, Options::bh_chain: done
    // before a next optimizer clears the same workspace arrays)
    if (ctx->aux_stream) (void)hipStreamSynchronize(ctx->aux_stream);
    delete ctx->opt;
    ctx->opt = nullptr;
}

// cuts of [0, n) into world equal label ranges
static std::vector<int64_t> equal_cuts(int64_t n, int world) {
    std::vector<int64_t> c(world + 1);
    const int64_t chunk = ceil_div(n, world);
    for (int r = 0; r <= world; ++r) c[r] = std::min<int64_t>(n, chunk * r);
    return c;
}

// make every rank's upd / gains current for all labels (each rank updates
// only its own labels between relabels): ragged all-gather of the slices
static void gather_working_set(tsne_ctx *ctx, OptState *s) {
    if (!sharded(ctx)) return;
    const int c = s->cur;
    std::vector<int64_t> off(ctx->world + 1);
    for (int r = 0; r <= ctx->world; ++r) off[r] = s->own[r] * s->C * (int64_t)sizeof(double);
    comm_allgatherv(ctx, s->upd[c], off.data());
    comm_allgatherv(ctx, s->gains[c], off.data());
}

// this rank's rows of P in the current labels (2-D)
static void build_own_rows(tsne_ctx *ctx, OptState *s) {
    hipStream_t st = ctx->stream;
    const int64_t m = s->L1 - s->L0;
    const int32_t *orig = s->orig[s->cur];
    hipLaunchKernelGGL(own_rowlen, dim3(ceil_div(m + 1, 256)), dim3(256), 0, st, orig, s->rp0, s->L0, s->L1, s->rowlen);
    size_t tb = s->scan_tmp_bytes;
    TSNE_HIP(hipcub::DeviceScan::ExclusiveSum(s->scan_tmp, tb, s->rowlen, s->rpw, (int)(m + 1), st));
    if (m > 0)
        hipLaunchKernelGGL(own_rows, dim3(ceil_div(m, 4)), dim3(256), 0, st, orig, s->lab, s->rp0, s->col0, s->val0,
                           s->L0, s->L1, s->rpw, s->colw, s->valw);
    TSNE_LAUNCH_CHECK();
    // sum of the owned P entries (scal[6]) and Z = 1 (scal[7]) for the Z-free
    // loss terms of an attraction launched before this iteration's Z
    hipLaunchKernelGGL(reduce_partial_devn, dim3(NPART), dim3(256), 0, st, s->valw, s->rpw + m, s->part2);
    hipLaunchKernelGGL(reduce_final, dim3(1), dim3(256), 0, st, s->part2, NPART, s->scal + 6, 0.0);
    hipLaunchKernelGGL(set_unit, dim3(1), dim3(64), 0, st, s->scal + 7);
    attract_layout_build(ctx, s->at, s->rpw, s->colw, s->valw, m, s->n, s->nnz, s->C, s->morton_labels);
}

// world > 1: the sorted positions of this rank's labels, ascending
static void build_qlist(tsne_ctx *ctx, OptState *s, const int32_t *idx_sorted) {
    hipStream_t st = ctx->stream;
    const int64_t n = s->n, nb = ceil_div(n, 256);
    hipLaunchKernelGGL(qlist_count, dim3(nb), dim3(256), 0, st, idx_sorted, n, s->L0, s->L1, s->qcnt);
    size_t tb = s->qscan_tmp_bytes;
    TSNE_HIP(hipcub::DeviceScan::ExclusiveSum(s->qscan_tmp, tb, s->qcnt, s->qoff, (int)nb, st));
    hipLaunchKernelGGL(qlist_fill, dim3(nb), dim3(256), 0, st, idx_sorted, n, s->L0, s->L1, s->qoff, s->qlist);
    TSNE_LAUNCH_CHECK();
}

// Renumber labels: new label j holds old label order[j] (device); new cuts.
static void relabel(tsne_ctx *ctx, OptState *s, const int32_t *order, const std::vector<int64_t> &cuts) {
    hipStream_t st = ctx->stream;
    const int a = s->cur, b = 1 - a;
    gather_working_set(ctx, s);   // full upd / gains under the old cuts
    hipLaunchKernelGGL(relabel_state, dim3(ceil_div(s->n, 256)), dim3(256), 0, st, order, s->n, s->C, s->Y[a],
                       s->upd[a], s->gains[a], s->orig[a], s->Y[b], s->upd[b], s->gains[b], s->orig[b], s->lab);
    TSNE_LAUNCH_CHECK();
    s->cur = b;
    s->own = cuts;
    s->L0 = cuts[ctx->rank];
    s->L1 = cuts[ctx->rank + 1];
    build_own_rows(ctx, s);
    ++s->relabels;
}

// Initial labels: P's connected components (smallest original index), then
// the BFS level from that root, then the original index -- points that
// share neighbourhoods in P get nearby labels, so each XCD's rows gather
// their Y_j from a few components instead of the whole embedding while the
// embedding itself is still unrelated to P (the first ~150 iterations, before
// the Morton relabelling below takes over).  Deterministic fixpoints.
static void graph_order(tsne_ctx *ctx, OptState *s, int32_t *order) {
    hipStream_t st = ctx->stream;
    Workspace &ws = ctx->ws;
    const int64_t n = s->n;
    int32_t *comp = ws.get<int32_t>("opt.g.comp", n);
    int32_t *lev = ws.get<int32_t>("opt.g.lev", n);
    int32_t *flag = ws.get<int32_t>("opt.g.flag", 1);
    uint64_t *key = ws.get<uint64_t>("opt.g.key", n), *key2 = ws.get<uint64_t>("opt.g.key2", n);
    int32_t *val = ws.get<int32_t>("opt.g.val", n);
    hipLaunchKernelGGL(iota_i32, dim3(ceil_div(n, 256)), dim3(256), 0, st, comp, n);
    auto fixpoint = [&](auto &&pass) {
        for (int it = 0; it < 10000; ++it) {
            int32_t h = 0;
            TSNE_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), st));
            pass();
            TSNE_HIP(hipMemcpyAsync(&h, flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            TSNE_HIP(hipStreamSynchronize(st));
            if (!h) return;
        }
        fail(TSNE_ERR_HIP, "graph ordering did not converge");
    };
    fixpoint([&] {
        hipLaunchKernelGGL(cc_pull, dim3(ceil_div(n, 4)), dim3(256), 0, st, s->rp0, s->col0, n, comp, flag);
        hipLaunchKernelGGL(cc_jump, dim3(ceil_div(n, 256)), dim3(256), 0, st, comp, n);
    });
    hipLaunchKernelGGL(level_init, dim3(ceil_div(n, 256)), dim3(256), 0, st, comp, n, lev);
    fixpoint([&] { hipLaunchKernelGGL(level_pull, dim3(ceil_div(n, 4)), dim3(256), 0, st, s->rp0, s->col0, n, lev, flag); });
    hipLaunchKernelGGL(graph_keys, dim3(ceil_div(n, 256)), dim3(256), 0, st, comp, lev, n, key, val);
    size_t tb = 0;
    TSNE_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, key, key2, val, order, (int)n, 0, 64, st));
    void *tmp = ws.get<uint8_t>("opt.g.tmp", tb);
    TSNE_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb, key, key2, val, order, (int)n, 0, 64, st));
    TSNE_LAUNCH_CHECK();
}

void opt_setup(tsne_ctx *ctx, const tsne_params *p, const int64_t *d_row_ptr, const int32_t *d_col,
               const double *d_P, int64_t n, double *dY, double *dupd, double *dgains) {
    TSNE_REQUIRE(p != nullptr, "params is NULL");
    if (p->n_components != 2 && p->n_components != 3)
        fail(TSNE_ERR_UNSUPPORTED, "n_components must be 2 (quadtree) or 3 (octree extension)");
    TSNE_REQUIRE(n >= 1, "empty embedding");
    TSNE_REQUIRE(p->metric >= 0 && p->metric <= 2, "unknown metric");
    TSNE_REQUIRE(n < (int64_t)INT32_MAX, "n must fit int32 point ids");
    hipStream_t st = ctx->stream;
    opt_destroy(ctx);
    OptState *s = new OptState();
    ctx->opt = s;
    s->p = *p;
    s->C = p->n_components;
    const int C = s->C;
    const int world = ctx->world;
    s->n = n;
    s->Yu = dY;
    s->updu = dupd;
    s->gainsu = dgains;
    int64_t nnz = 0;
    TSNE_HIP(hipMemcpyAsync(&nnz, d_row_ptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    TSNE_HIP(hipStreamSynchronize(st));
    s->nnz = nnz;
    Workspace &ws = ctx->ws;
    s->rp0 = ws.get<int64_t>("opt.rp0", n + 1);
    s->col0 = ws.get<int32_t>("opt.col0", nnz + 1);
    s->val0 = ws.get<double>("opt.val0", nnz + 1);
    TSNE_HIP(hipMemcpyAsync(s->rp0, d_row_ptr, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToDevice, st));
    TSNE_HIP(hipMemcpyAsync(s->col0, d_col, sizeof(int32_t) * nnz, hipMemcpyDeviceToDevice, st));
    TSNE_HIP(hipMemcpyAsync(s->val0, d_P, sizeof(double) * nnz, hipMemcpyDeviceToDevice, st));
    for (int b = 0; b < 2; ++b) {
        const std::string k = std::to_string(b);
        s->Y[b] = ws.get<double>("opt.Y" + k, C * n);
        s->upd[b] = ws.get<double>("opt.upd" + k, C * n);
        s->gains[b] = ws.get<double>("opt.gains" + k, C * n);
        s->orig[b] = ws.get<int32_t>("opt.orig" + k, n);
    }
    s->lab = ws.get<int32_t>("opt.lab", n);
    s->cur = 0;
    TSNE_HIP(hipMemcpyAsync(s->Y[0], dY, sizeof(double) * C * n, hipMemcpyDeviceToDevice, st));
    TSNE_HIP(hipMemcpyAsync(s->upd[0], dupd, sizeof(double) * C * n, hipMemcpyDeviceToDevice, st));
    TSNE_HIP(hipMemcpyAsync(s->gains[0], dgains, sizeof(double) * C * n, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(iota_i32, dim3(ceil_div(n, 256)), dim3(256), 0, st, s->orig[0], n);
    hipLaunchKernelGGL(iota_i32, dim3(ceil_div(n, 256)), dim3(256), 0, st, s->lab, n);
    s->own = equal_cuts(n, world);
    s->L0 = s->own[ctx->rank];
    s->L1 = s->own[ctx->rank + 1];
    const int64_t rows_cap = n;   // owned rows (cost-balanced cuts may give one rank most of them)
    s->rowlen = ws.get<int64_t>("opt.rowlen", rows_cap + 1);
    size_t tb = 0;
    TSNE_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, s->rowlen, s->rowlen, (int)(rows_cap + 1), st));
    s->scan_tmp_bytes = tb;
    s->scan_tmp = ws.get<uint8_t>("opt.scan_tmp", tb);
    s->Ynew = ws.get<double>("opt.Ynew", C * n);
    s->attr = ws.get<double2>("opt.attr", rows_cap);
    s->F = ws.get<double2>("opt.F", n);
    s->z = ws.get<double>("opt.z", n);
    s->scal = ws.get<double>("opt.scal", 8);
    s->part = ws.get<double>("opt.part", std::max<int64_t>(NPART, attract_max_blocks(rows_cap)));
    s->part2 = ws.get<double>("opt.part2", NPART);
    s->mpart = ws.get<double>("opt.mpart", 3 * ceil_div(rows_cap, 256) + 3);   // C <= 3 components
    s->bcost = ws.get<unsigned long long>("opt.bcost", ceil_div(n, 256) + 1);
    s->bounds = ws.get<int64_t>("opt.bounds", world + 1);
    s->lscore = ws.get<unsigned long long>("opt.lscore", 2);
    s->loss_slots = std::max(1, p->iterations / 10 + 1);
    s->loss = ws.get<double>("opt.loss", s->loss_slots);
    s->loss_written.assign(s->loss_slots, 0);
    s->visits = ws.get<unsigned long long>("opt.visits", VIS_N);
    if (sharded(ctx)) {
        const int64_t nb = ceil_div(n, 256);
        if (C == 2) {
            s->pcuts = ws.get<int64_t>("opt.pcuts", world + 1);
            s->plim = ws.get<int32_t>("opt.plim", 4);
            s->pcost = ws.get<unsigned long long>("opt.pcost", world);
            s->Fl = ws.get<double2>("opt.Fl", n);
            std::vector<int64_t> c0(world + 1);
            for (int r = 0; r <= world; ++r) c0[r] = n * r / world;
            TSNE_HIP(hipMemcpyAsync(s->pcuts, c0.data(), sizeof(int64_t) * (world + 1), hipMemcpyHostToDevice, st));
            TSNE_HIP(hipMemsetAsync(s->plim, 0, 4 * sizeof(int32_t), st));
            TSNE_HIP(hipStreamSynchronize(st));
        }
        s->qlist = ws.get<int32_t>("opt.qlist", n);
        s->qcnt = ws.get<int32_t>("opt.qcnt", nb);
        s->qoff = ws.get<int32_t>("opt.qoff", nb);
        size_t qb = 0;
        TSNE_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, qb, s->qcnt, s->qoff, (int)nb, st));
        s->qscan_tmp_bytes = qb;
        s->qscan_tmp = ws.get<uint8_t>("opt.qscan_tmp", qb);
    }
    TSNE_HIP(hipMemsetAsync(s->Ynew, 0, sizeof(double) * C * n, st));
    TSNE_HIP(hipMemsetAsync(s->F, 0, sizeof(double2) * n, st));
    TSNE_HIP(hipMemsetAsync(s->z, 0, sizeof(double) * n, st));
    if (C == 3) {
        oct_alloc(ctx, s->otree, n);
        s->F3 = ws.get<double>("opt.F3", 3 * (size_t)n);
        s->attr3 = ws.get<double>("opt.attr3", 3 * (size_t)rows_cap);
        s->part = ws.get<double>("opt.part", std::max<int64_t>(NPART, attract3_blocks(rows_cap)));
        TSNE_HIP(hipMemsetAsync(s->F3, 0, sizeof(double) * 3 * n, st));
    } else {
        bh_alloc(ctx, s->tree, n);
    }
    s->rpw = ws.get<int64_t>("opt.rpw", rows_cap + 1);
    s->colw = ws.get<int32_t>("opt.colw", nnz + 1);
    s->valw = ws.get<double>("opt.valw", nnz + 1);
    {   // initial labels in P's graph order (Options::graph_order = 0: the original order);
        // in 3-D too since round 6 (attract3's Y_j gathers then hit the L2 as in 2-D)
        const bool gorder = ctx->opts.graph_order != 0;
        const bool dense_small = s->nnz / n > 1024 && n * 16 <= (2 << 20);   // see maybe_relabel
        if (gorder && n >= 2 && !(dense_small && !sharded(ctx))) {
            int32_t *order = ws.get<int32_t>("opt.g.order", n);
            graph_order(ctx, s, order);
            relabel(ctx, s, order, s->own);
        } else {
            build_own_rows(ctx, s);
        }
    }
    for (auto &e : s->ev) TSNE_HIP(hipEventCreate(&e));
    TSNE_HIP(hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking));   // the attraction's (stream priorities: no gain, round 1)
    TSNE_HIP(hipEventCreateWithFlags(&s->ev_y, hipEventDisableTiming));
    TSNE_HIP(hipEventCreateWithFlags(&s->ev_attr, hipEventDisableTiming));
    ctx->timers.reset("opt.attract");
    ctx->timers.reset("opt.update");
    TSNE_LAUNCH_CHECK();
}

// Z = sum of z over all queries: locally (one rank) or this rank's partial
// over its query list + an all-reduce of one double
static void reduce_Z(tsne_ctx *ctx, OptState *s, const double *z, bool all_points = false) {
    hipStream_t st = ctx->stream;
    if (!sharded(ctx) || all_points) {   // every point (a tree partition: this rank's partial sums)
        hipLaunchKernelGGL(reduce_partial, dim3(NPART), dim3(256), 0, st, z, s->n, 1, 0, s->part2);
    } else {
        hipLaunchKernelGGL(reduce_list_partial, dim3(NPART), dim3(256), 0, st, z, s->qlist, s->L1 - s->L0, s->part2);
    }
    hipLaunchKernelGGL(reduce_final, dim3(1), dim3(256), 0, st, s->part2, NPART, s->scal, 0.0);
    if (sharded(ctx)) comm_allreduce_sum_f64(ctx, s->scal, 1);
}

// loss of this iteration (all ranks' partial sums) into its slot
static void record_loss(tsne_ctx *ctx, OptState *s, int32_t t, int64_t blocks, bool zfree = false,
                        double ex = 1.0) {
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(reduce_partial, dim3(NPART), dim3(256), 0, st, s->part, blocks, 1, 0, s->part2);
    hipLaunchKernelGGL(reduce_final, dim3(1), dim3(256), 0, st, s->part2, NPART, s->scal + 1, 0.0);
    if (zfree) hipLaunchKernelGGL(loss_add_lnz, dim3(1), dim3(64), 0, st, s->scal, ex);
    if (sharded(ctx)) comm_allreduce_sum_f64(ctx, s->scal + 1, 1);
    const int slot = t / 10 - 1;
    if (slot >= 0 && slot < s->loss_slots) {
        TSNE_HIP(hipMemcpyAsync(s->loss + slot, s->scal + 1, sizeof(double), hipMemcpyDeviceToDevice, st));
        s->loss_written[slot] = t;
    }
}

// the updated embedding of every rank's labels on every rank
static void gather_Ynew(tsne_ctx *ctx, OptState *s) {
    std::vector<int64_t> off(ctx->world + 1);
    for (int r = 0; r <= ctx->world; ++r) off[r] = s->own[r] * s->C * (int64_t)sizeof(double);
    comm_allgatherv(ctx, s->Ynew, off.data());
}

static void finish_profile(tsne_ctx *ctx, OptState *s, int32_t t) {
    TSNE_HIP(hipEventRecord(s->ev[5], ctx->stream));
    TSNE_HIP(hipEventSynchronize(s->ev[5]));
    for (int k = 0; k < 5; ++k) {   // [3]: the attraction kernel alone, on its own stream
        float ms = 0.f;
        if (k != 3) TSNE_HIP(hipEventElapsedTime(&ms, s->ev[k], s->ev[k + 1]));
        s->last_ms[k] = ms;
    }
    s->last_ms[3] = ctx->timers.last_ms("opt.attract");
    if (s->C == 3) {
        for (int k = 0; k < 10; ++k) s->last_visits[k] = 0;
        return;
    }
    unsigned long long v[VIS_N] = {};
    TSNE_HIP(hipMemcpy(v, s->visits, sizeof(v), hipMemcpyDeviceToHost));
    for (int k = 0; k < 10; ++k) s->last_visits[k] = (int64_t)v[k];
    // the traversal waves' shader clock: their cycles over their 100 MHz wall ticks
    s->last_mhz = v[18] ? (int64_t)(100.0 * (double)v[37] / (double)v[18]) : 0;
    const bool dbg = debug_tiles();   // tile_apply diagnostics
    if (dbg)
        fprintf(stderr, "[tiles] t=%d tasks=%llu dense_pts=%llu momchk=%llu moment_evals=%llu dense_pairs=%llu "
                "pops=%llu child_slots=%llu all_take_full=%llu all_take_partial=%llu\n", t,
                v[10], v[11], v[12], v[1], v[2], v[3], v[6], v[13], v[14]);
    if (dbg && v[17] > 0)   // traversal wave times (100 MHz wall clock): span of the grid vs its waves
        fprintf(stderr, "[waves] t=%d span_us=%.1f max_wave_us=%.1f mean_wave_us=%.2f\n", t,
                (double)(v[17] - (~0ull - v[16])) * 0.01, (double)v[15] * 0.01,
                (double)v[18] * 0.01 / (double)std::max<int64_t>(1, ceil_div(s->L1 - s->L0, 64)));
    if (dbg)   // tile_apply dense paths: wave steps / useful lane pairs
        fprintf(stderr, "[tpaths] t=%d lanewise %llu/%llu packed %llu/%llu qmajor %llu/%llu staged %llu/%llu\n", t,
                v[24], v[25], v[26], v[27], v[28], v[29], v[30], v[31]);
    if (dbg && v[21] > 0)   // tile_apply waves (only waves with tiles report)
        fprintf(stderr, "[twaves] t=%d span_us=%.1f max_wave_us=%.1f\n", t,
                (double)(v[21] - (~0ull - v[20])) * 0.01, (double)v[19] * 0.01);
}

// One iteration of the 3-D (octree) optimizer: labels are P's graph order
// (set once at setup, as in 2-D; no Morton relabels), rank r owns labels
// [L0, L1) -- its rows of P in labels (rpw / colw / valw) -- and computes BH
// for exactly those points (its query list in octree order); only Z, the loss
// and the updated embedding cross ranks.
static void opt_step3(tsne_ctx *ctx, OptState *s, int32_t t) {
    hipStream_t st = ctx->stream;
    const tsne_params &p = s->p;
    const int32_t T = p.iterations;
    const int32_t n1 = std::min(T, 20);
    const int32_t n2 = std::min(T - n1, 81);
    const double ex = (t <= n1 + n2) ? p.early_exaggeration : 1.0;
    const double mom = (t <= n1) ? p.initial_momentum : p.final_momentum;
    const bool want_loss = (t % 10 == 0);
    const int64_t n = s->n;
    const int c = s->cur;
    double *Y = s->Y[c];
    // this rank's rows by label (row pointer local to L0); the sums go to attr3
    AttractArgs aa{s->rpw - s->L0, s->colw, s->valw, s->L0, s->L1, Y, s->scal, p.metric, ex, nullptr, s->part};
    aa.n = n;
    if (s->profile) TSNE_HIP(hipEventRecord(s->ev[0], st));
    oct_build(ctx, s->otree, Y, p.theta, ex == 1.0);
    if (s->profile) TSNE_HIP(hipEventRecord(s->ev[1], st));
    // the attraction of a non-loss iteration needs no Z: on the side stream,
    // beside the traversal (after the build, whose latency-bound kernels it
    // would stretch; the 2-D rule); a loss iteration's after Z, as before
    const bool side = !want_loss;
    int64_t blocks = 0;
    if (side) {
        TSNE_HIP(hipEventRecord(s->ev_y, st));
        TSNE_HIP(hipStreamWaitEvent(s->side, s->ev_y, 0));
        ctx->timers.begin("opt.attract", s->side);
        blocks = attract_launch_3d(s->side, s->at, aa, s->attr3, false);
        ctx->timers.end("opt.attract", s->side);
        TSNE_HIP(hipEventRecord(s->ev_attr, s->side));
    }
    if (sharded(ctx)) {
        build_qlist(ctx, s, s->otree.idx_sorted);
        oct_repulsion(ctx, s->otree, p.theta, 0, s->L1 - s->L0, s->F3, s->z, s->qlist);
    } else {
        oct_repulsion(ctx, s->otree, p.theta, 0, n, s->F3, s->z, nullptr);
    }
    if (s->profile) TSNE_HIP(hipEventRecord(s->ev[2], st));
    reduce_Z(ctx, s, s->z);
    if (s->profile) TSNE_HIP(hipEventRecord(s->ev[3], st));
    if (side) {
        TSNE_HIP(hipStreamWaitEvent(st, s->ev_attr, 0));
    } else {
        ctx->timers.begin("opt.attract", st);
        blocks = attract_launch_3d(st, s->at, aa, s->attr3, want_loss);
        ctx->timers.end("opt.attract", st);
    }
    s->log_attract(t, side ? 0 : 1);   // 0: beside the traversal (side stream); 1: loss launch alone after Z
    if (s->profile) TSNE_HIP(hipEventRecord(s->ev[4], st));
    ctx->timers.begin("opt.update", st);
    // one rank: the mean's block partials from combine_update3, one
    // workgroup for the mean, one pass for the centring
    const bool fused_mean = !sharded(ctx);
    if (s->L1 > s->L0)
        hipLaunchKernelGGL(combine_update3<1>, dim3(ceil_div(s->L1 - s->L0, 256)), dim3(256), 0, st, s->L0, s->L1,
                           s->attr3, s->otree.inv, s->F3, s->scal, Y, nullptr, s->Ynew, s->upd[c], s->gains[c],
                           p.min_gain, mom, p.learning_rate, fused_mean ? s->mpart : nullptr);
    TSNE_LAUNCH_CHECK();
    if (want_loss) record_loss(ctx, s, t, blocks);
    if (fused_mean) {
        hipLaunchKernelGGL(mean3_final, dim3(1), dim3(256), 0, st, s->mpart, ceil_div(s->L1 - s->L0, 256), (double)n,
                           s->scal + 2);
        hipLaunchKernelGGL(center3, dim3(ceil_div(n * 3, 256)), dim3(256), 0, st, s->Ynew, n, s->scal + 2, Y);
    } else {
        gather_Ynew(ctx, s);
        for (int k = 0; k < 3; ++k) {
            hipLaunchKernelGGL(reduce_partial, dim3(NPART), dim3(256), 0, st, s->Ynew, n, 3, k, s->part2);
            hipLaunchKernelGGL(reduce_final, dim3(1), dim3(256), 0, st, s->part2, NPART, s->scal + 2 + k, (double)n);
        }
        hipLaunchKernelGGL(center_apply, dim3(ceil_div(n * 3, 256)), dim3(256), 0, st, s->Ynew, n, 3, s->scal + 2, Y);
    }
    ctx->timers.end("opt.update", st);
    TSNE_LAUNCH_CHECK();
    if (s->profile) finish_profile(ctx, s, t);
}

// Several ranks with the tiled layout keep P's graph order (TSNE_RELABEL
// unset): the ownership is re-cut in that order instead of a Morton relabel,
// which would hand the attraction back to attract_rows (C3 standalone: 2.35 vs
// 0.77 ms).  Each query's traversal cost goes to its label's 256-label bucket
// (an equal share of its wave's time); the all-reduced buckets give cuts of
// equal cost, applied (owned rows and their tiles rebuilt) when a cut moves
// by more than 1/16 of a rank's share.
// The tree partition (Options::bh_split): several ranks, 2-D.
static bool split_mode(const tsne_ctx *ctx, const OptState *s) {
    return sharded(ctx) && ctx->opts.bh_split && s->C == 2 && s->pcuts != nullptr;
}

static bool recut_mode(tsne_ctx *ctx, OptState *s) {
    if (split_mode(ctx, s)) return false;   // BH cost does not follow the row ownership there
    return ctx->opts.recut && ctx->opts.relabel == -1 && sharded(ctx) && s->at.at_on && !s->morton_labels;
}
static void recut(tsne_ctx *ctx, OptState *s, const std::vector<int64_t> &cuts) {
    gather_working_set(ctx, s);   // full upd / gains under the old cuts
    s->own = cuts;
    s->L0 = cuts[ctx->rank];
    s->L1 = cuts[ctx->rank + 1];
    build_own_rows(ctx, s);
    ++s->relabels;
}
static void maybe_recut(tsne_ctx *ctx, OptState *s) {
    hipStream_t st = ctx->stream;
    const int64_t n = s->n;
    ++s->relabel_checks;
    std::vector<int64_t> cuts(ctx->world + 1);
    comm_allreduce_sum_u64(ctx, s->bcost, (size_t)ceil_div(n, 256));
    bh_balance(ctx, s->bcost, n, ctx->world, s->bounds);
    TSNE_HIP(hipMemcpyAsync(cuts.data(), s->bounds, sizeof(int64_t) * (ctx->world + 1), hipMemcpyDeviceToHost, st));
    TSNE_HIP(hipStreamSynchronize(st));
    int64_t moved = 0;
    for (int r = 1; r < ctx->world; ++r) moved = std::max<int64_t>(moved, std::llabs(cuts[r] - s->own[r]));
    if (moved * 16 * ctx->world > n) recut(ctx, s, cuts);   // identical decision on every rank
}

// Relabel check (every RELABEL_EVERY iterations, 2-D): renumber the labels
// into this iteration's Morton order when that order keeps more of P's edges
// within a window of labels than the current one (identical decision on
// every rank: the score reads only replicated data).  With several ranks the
// new cuts balance the BH cost measured in this iteration (all-reduced
// 256-position bucket costs); the qlist waves of the NEXT iterations follow.
static void maybe_relabel(tsne_ctx *ctx, OptState *s) {
    hipStream_t st = ctx->stream;
    const int64_t n = s->n;
    if (recut_mode(ctx, s)) {   // several ranks on the tiled layout: re-cut the graph order by cost
        maybe_recut(ctx, s);
        return;
    }
    // dense rows over a small embedding (the distance-matrix mode, C5): every
    // row gathers all of Y, which sits in one XCD's L2 (n * 16 B <= 2 MiB)
    // whatever the labels, so a relabel (a copy of the whole P) buys nothing
    if (!sharded(ctx) && s->nnz / std::max<int64_t>(1, n) > 1024 && n * 16 <= (2 << 20)) return;
    // Options::relabel: 0 never, 1 by the locality score, 2 always; -1: by the
    // score, except on one rank with the tiled layout, which keeps P's graph
    // order (attract_tiles reads Y in label windows; a Morton relabel hands
    // the attraction back to attract_rows: whole C3 schedule 7.23 -> 7.01 s
    // without relabels, A/B on one box)
    const int mode = ctx->opts.relabel;
    if (mode == 0 || (mode == -1 && !sharded(ctx) && s->at.at_on)) return;
    // a fixed sample of rows, ~1 << 22 entries at most (dense rows: fewer rows)
    const int64_t avg = std::max<int64_t>(1, s->nnz / std::max<int64_t>(1, n));
    const int64_t nsamp = std::max<int64_t>(1, std::min<int64_t>({n, 1 << 16, (1 << 22) / avg}));
    const int64_t stride = std::max<int64_t>(1, n / nsamp);
    const int64_t win = std::max<int64_t>(64, n / 64);
    TSNE_HIP(hipMemsetAsync(s->lscore, 0, 2 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(locality_score, dim3(ceil_div(nsamp, 4)), dim3(256), 0, st, s->rp0, s->col0, s->lab,
                       s->tree.inv, n, stride, nsamp, win, s->lscore);
    unsigned long long sc[2] = {0, 0};
    TSNE_HIP(hipMemcpyAsync(sc, s->lscore, sizeof(sc), hipMemcpyDeviceToHost, st));
    TSNE_HIP(hipStreamSynchronize(st));
    ++s->relabel_checks;
    const bool go = mode == 2 || sc[1] > sc[0];
    if (!go) return;
    std::vector<int64_t> cuts = s->own;
    if (sharded(ctx) && !split_mode(ctx, s)) {   // (tree partition: the rows keep equal label cuts)
        comm_allreduce_sum_u64(ctx, s->bcost, (size_t)ceil_div(n, 256));
        bh_balance(ctx, s->bcost, n, ctx->world, s->bounds);
        TSNE_HIP(hipMemcpyAsync(cuts.data(), s->bounds, sizeof(int64_t) * (ctx->world + 1), hipMemcpyDeviceToHost, st));
        TSNE_HIP(hipStreamSynchronize(st));
    }
    s->morton_labels = true;
    relabel(ctx, s, s->tree.idx_sorted, cuts);
}

void opt_step(tsne_ctx *ctx, int32_t t) {
    OptState *s = ctx->opt;
    TSNE_REQUIRE(s != nullptr, "tsne_dev_opt_setup has not been called");
    TSNE_REQUIRE(t >= 1, "iteration numbers start at 1");
    if (s->C == 3) {
        opt_step3(ctx, s, t);
        return;
    }
    hipStream_t st = ctx->stream;
    const tsne_params &p = s->p;
    const int32_t T = p.iterations;
    const int32_t n1 = std::min(T, 20);
    const int32_t n2 = std::min(T - n1, 81);
    const double ex = (t <= n1 + n2) ? p.early_exaggeration : 1.0;
    const double mom = (t <= n1) ? p.initial_momentum : p.final_momentum;
    const int want_loss = (t % 10 == 0);
    const bool check_relabel = t % RELABEL_EVERY == 0;
    const int64_t n = s->n;
    double *Y = s->Y[s->cur];
    if (s->profile) {
        TSNE_HIP(hipMemsetAsync(s->visits, 0, VIS_N * sizeof(unsigned long long), st));
        TSNE_HIP(hipEventRecord(s->ev[0], st));
    }
    // attraction over this rank's rows (row pointer local to L0)
    AttractArgs aa{s->rpw - s->L0, s->colw, s->valw, s->L0, s->L1, Y, s->scal, p.metric, ex, s->attr, s->part};
    aa.n = n;
    // 0. attraction sums on the side stream, concurrent with the BH
    // traversal (in loss iterations with Z-free KL terms, P ln(P (1 + metric)):
    // ln(Z) sum P is added once Z is known; the loss launch alone after Z:
    // whole schedule +1 %) -- or, while the last build took the root-tile
    // path, already with the tree build, on 3 blocks per CU (as fast as 8:
    // miss-bound) so that the build's short kernels keep the other slots.  A
    // full build is not overlapped: its latency-bound kernels stretch under
    // the attraction (morton_keys 15 -> 800 us; whole schedule 8.53 -> 8.97 s).
    const bool rt_phase = s->tree.root_tile;
    if (want_loss) aa.scal = s->scal + 7;   // Z = 1 in the kernel
    int64_t blocks = 0;
    if (rt_phase) aa.bpc = 3;
    auto side_attract = [&] {
        TSNE_HIP(hipEventRecord(s->ev_y, st));
        TSNE_HIP(hipStreamWaitEvent(s->side, s->ev_y, 0));
        ctx->timers.begin("opt.attract", s->side);
        blocks = attract_launch_2d(s->side, s->at, aa, want_loss != 0);
        TSNE_LAUNCH_CHECK();
        ctx->timers.end("opt.attract", s->side);
        s->log_attract(t, want_loss ? 2 : 0);
        TSNE_HIP(hipEventRecord(s->ev_attr, s->side));
    };
    // (attract_serial_t0 <= t <= attract_serial_t1: the attraction alone on
    // this stream after the BH kernels instead -- an A/B of the overlap's cost)
    const bool serial_at = t >= ctx->opts.attract_serial_t0 && t <= ctx->opts.attract_serial_t1 && !rt_phase;
    if (rt_phase) side_attract();
    // 1. tree (identical on every rank)
    // insertion rows = original indices; the root-tile shortcut while the
    // embedding is small
    // the strict near-exact tolerance while P is exaggerated (the dynamics
    // amplify any difference fastest there), the late one after
    bh_build(ctx, s->tree, Y, p.theta, s->orig[s->cur], root_tile_enabled(ctx), bh_near_tol(ctx, ex == 1.0));
    if (sharded(ctx)) comm_mark(ctx, s->tree.root_tile ? "tree_rt" : "tree");
    if (!rt_phase && !serial_at) side_attract();
    if (s->profile) TSNE_HIP(hipEventRecord(s->ev[1], st));
    // 2. repulsion for this rank's points: all of them, or its query list
    // (its labels' sorted positions, ascending: the waves stay Morton-local);
    // bucket costs only where a relabel may re-cut the ownership
    // tree partition: every query over this rank's cells (sorted-position
    // range, re-cut by the ranks' traversal costs every iteration)
    const bool split = split_mode(ctx, s) && !s->tree.root_tile;
    s->split_last = split;
    unsigned long long *bcost = (sharded(ctx) && check_relabel && !split_mode(ctx, s)) ? s->bcost : nullptr;
    if (bcost) TSNE_HIP(hipMemsetAsync(bcost, 0, sizeof(unsigned long long) * ceil_div(n, 256), st));
    if (split) {
        part_align(ctx, s->tree, s->pcuts, ctx->world, ctx->rank, s->plim);
        bh_repulsion(ctx, s->tree, p.theta, 0, n, s->F, s->z, s->profile ? s->visits : nullptr, nullptr, nullptr, false,
                     s->plim);
        comm_mark(ctx, "bh");
    } else if (sharded(ctx)) {
        build_qlist(ctx, s, s->tree.idx_sorted);
        bh_repulsion(ctx, s->tree, p.theta, 0, s->L1 - s->L0, s->F, s->z, s->profile ? s->visits : nullptr, s->qlist,
                     bcost, recut_mode(ctx, s));
        comm_mark(ctx, s->tree.root_tile ? "bh_rt" : "bh");
    } else {
        bh_repulsion(ctx, s->tree, p.theta, 0, n, s->F, s->z, s->profile ? s->visits : nullptr);
    }
    if (serial_at) side_attract();   // (the side stream waits for everything above)
    if (s->profile) TSNE_HIP(hipEventRecord(s->ev[2], st));
    // 3. Z (TsneHelpers.scala:266): the only per-iteration all-reduce
    reduce_Z(ctx, s, s->z, split);
    const double2 *Fc = s->F;           // combine_update's forces: sorted order (inv) ...
    const int32_t *Finv = s->tree.inv;
    if (split) {
        // the next iteration's cuts from this traversal's costs (identical on every rank)
        TSNE_HIP(hipMemsetAsync(s->pcost, 0, sizeof(unsigned long long) * ctx->world, st));
        part_cost(ctx, s->tree, ceil_div(n, 64), s->pcost + ctx->rank);
        comm_allreduce_sum_u64(ctx, s->pcost, (size_t)ctx->world);
        part_recut(ctx, s->pcost, ctx->world, n, s->pcuts);
        // ... or, with the tree partition, by label after the reduce-scatter of
        // every rank's partial sums to the row owners
        hipLaunchKernelGGL(f_to_label, dim3(ceil_div(n, 256)), dim3(256), 0, st, s->tree.inv, n, s->F, s->Fl);
        std::vector<int64_t> off(ctx->world + 1);
        for (int r = 0; r <= ctx->world; ++r) off[r] = 2 * s->own[r];
        comm_reduce_scatterv_f64(ctx, reinterpret_cast<double *>(s->Fl), off.data());
        Fc = s->Fl;
        Finv = nullptr;
    }
    if (s->profile) TSNE_HIP(hipEventRecord(s->ev[3], st));
    // 4. the attraction's sums + update for owned rows
    TSNE_HIP(hipStreamWaitEvent(st, s->ev_attr, 0));
    if (s->profile) TSNE_HIP(hipEventRecord(s->ev[4], st));
    // update + centre: combine_update (with the mean's block partials when one
    // rank holds every row), mean, centre + write-back of the caller's Y
    ctx->timers.begin("opt.update", st);
    const bool fused_mean = !sharded(ctx);
    const int c = s->cur;
    combine_launch<1>(st, s->L0, s->L1, s->attr, Finv, Fc, s->scal, Y, nullptr, s->Ynew, s->upd[c],
                      s->gains[c], p.min_gain, mom, p.learning_rate, fused_mean ? s->mpart : nullptr);
    if (want_loss) record_loss(ctx, s, t, blocks, true, ex);
    // 5. exchange (all-gather of the owned slices) + 6. centre
    if (fused_mean) {
        hipLaunchKernelGGL(mean2_final, dim3(1), dim3(256), 0, st, s->mpart, ceil_div(s->L1 - s->L0, 256),
                           (double)n, s->scal + 2);
    } else {
        gather_Ynew(ctx, s);
        for (int k = 0; k < 2; ++k) {
            hipLaunchKernelGGL(reduce_partial, dim3(NPART), dim3(256), 0, st, s->Ynew, n, 2, k, s->part2);
            hipLaunchKernelGGL(reduce_final, dim3(1), dim3(256), 0, st, s->part2, NPART, s->scal + 2 + k, (double)n);
        }
    }
    hipLaunchKernelGGL(center2, dim3(ceil_div(n, 256)), dim3(256), 0, st, s->Ynew, n, s->scal + 2, Y);
    ctx->timers.end("opt.update", st);
    TSNE_LAUNCH_CHECK();
    if (check_relabel) maybe_relabel(ctx, s);
    if (s->profile) finish_profile(ctx, s, t);
}

// The tree partition's traversal stack guard (bh_traverse<., true>): never
// expected to trip (the cut alignment bounds the shared depth); loud if it did.
static void check_split_overflow(tsne_ctx *ctx, const OptState *s) {
    if (!s->plim) return;
    int32_t f = 0;
    TSNE_HIP(hipMemcpyAsync(&f, s->plim + 2, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
    if (f) fail(TSNE_ERR_HIP, "tree-partition traversal stack overflow (results invalid)");
}

// Write upd / gains (and Y) back to the caller's buffers in the original order.
void opt_sync(tsne_ctx *ctx) {
    OptState *s = ctx->opt;
    TSNE_REQUIRE(s != nullptr, "tsne_dev_opt_setup has not been called");
    check_split_overflow(ctx, s);
    hipStream_t st = ctx->stream;
    gather_working_set(ctx, s);
    const int c = s->cur;
    const int64_t n = s->n;
    const int C = s->C;
    hipLaunchKernelGGL(scatter_to_user_c, dim3(ceil_div(n, 256)), dim3(256), 0, st, s->Y[c], s->orig[c], n, C, s->Yu);
    hipLaunchKernelGGL(scatter_to_user_c, dim3(ceil_div(n, 256)), dim3(256), 0, st, s->upd[c], s->orig[c], n, C,
                       s->updu);
    hipLaunchKernelGGL(scatter_to_user_c, dim3(ceil_div(n, 256)), dim3(256), 0, st, s->gains[c], s->orig[c], n, C,
                       s->gainsu);
    TSNE_LAUNCH_CHECK();
}

int32_t opt_losses(tsne_ctx *ctx, int32_t *keys, double *vals, int32_t cap) {
    OptState *s = ctx->opt;
    TSNE_REQUIRE(s != nullptr, "tsne_dev_opt_setup has not been called");
    check_split_overflow(ctx, s);
    std::vector<double> h(s->loss_slots);
    TSNE_HIP(hipMemcpyAsync(h.data(), s->loss, sizeof(double) * s->loss_slots, hipMemcpyDeviceToHost, ctx->stream));
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
    int32_t k = 0;
    for (int32_t i = 0; i < s->loss_slots; ++i) {
        if (!s->loss_written[i]) continue;
        if (k < cap) {
            if (keys) keys[k] = s->loss_written[i];
            if (vals) vals[k] = h[i];
        }
        ++k;
    }
    return k;
}

int32_t opt_attract_log(tsne_ctx *ctx, int32_t *iters, int32_t *standalone, double *ms, int32_t cap) {
    OptState *s = ctx->opt;
    TSNE_REQUIRE(s != nullptr, "tsne_dev_opt_setup has not been called");
    const std::vector<double> v = ctx->timers.ms("opt.attract");
    TSNE_REQUIRE(v.size() == s->attract_iter.size(), "attraction timer log out of step");
    const int32_t k = (int32_t)v.size();
    for (int32_t e = 0; e < k && e < cap; ++e) {
        if (iters) iters[e] = s->attract_iter[e].first;
        if (standalone) standalone[e] = s->attract_iter[e].second;
        if (ms) ms[e] = v[e];
    }
    return k;
}

int64_t opt_attract_kernel(tsne_ctx *ctx) {
    OptState *s = ctx->opt;
    if (!s) return -1;
    return s->C == 3 ? (s->at.at_on ? 3 : 2) : (s->at.at_on ? 1 : 0);
}

int64_t opt_attract_cfg(tsne_ctx *ctx) {
    OptState *s = ctx->opt;
    return (s && s->at.at_on) ? s->at.at_cfg : -1;
}

int64_t opt_attract_pad(tsne_ctx *ctx) {
    OptState *s = ctx->opt;
    return (s && s->at.at_on && s->at.at_stream) ? s->at.at_pad_ppm : 0;
}

BHTree *opt_tree(tsne_ctx *ctx) {
    OptState *s = ctx->opt;
    return (s && s->C == 2) ? &s->tree : nullptr;
}

double opt_last_z(tsne_ctx *ctx) {
    OptState *s = ctx->opt;
    TSNE_REQUIRE(s != nullptr, "tsne_dev_opt_setup has not been called");
    double z = 0.0;
    TSNE_HIP(hipMemcpyAsync(&z, s->scal, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TSNE_HIP(hipStreamSynchronize(ctx->stream));
    return z;
}

void opt_profile(tsne_ctx *ctx, int enable, double *ms5, int64_t *visits) {
    OptState *s = ctx->opt;
    TSNE_REQUIRE(s != nullptr, "tsne_dev_opt_setup has not been called");
    if (enable >= 0) s->profile = enable != 0;
    if (ms5)
        for (int k = 0; k < 5; ++k) ms5[k] = s->last_ms[k];
    if (visits)
        for (int k = 0; k < 10; ++k) visits[k] = s->last_visits[k];
}

}  // namespace tsne
