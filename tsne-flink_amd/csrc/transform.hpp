// transform.hpp -- embedding new points into a fitted map: Barnes-Hut
// repulsion for query points that are not in the tree, and the optimizer that
// moves only the new points, for 2-D maps (the quadtree) and 3-D maps (the
// octree): transform.hip.
#pragma once
#include "bhtree.hpp"
#include "octree.hpp"

namespace tsne {

// The device-resident transform (tsne_dev_transform_*): the reference map's
// tree, built once at setup, and the new points' working set, which stays in
// the caller's buffers and order (a step reads and writes it in place through
// the Morton permutation of the queries).
struct TransformState {
    int32_t dim = 2;                   // the map's dimension: which tree is built
    BHTree tree;                       // the reference map's quadtree ("bhx.", dim 2)
    OctTree otree;                     // the reference map's octree ("octx.", dim 3)
    tsne_params prm{};
    int64_t n = 0, m = 0;
    const double *Yref = nullptr;      // caller's device buffers
    const int64_t *row_ptr = nullptr;
    const int32_t *col = nullptr;
    const double *P = nullptr;
    double *Y = nullptr, *upd = nullptr, *gains = nullptr;
    int32_t *perm = nullptr;           // Morton slot -> query row
    int32_t *flag = nullptr;           // [0] != 0: a walk's stack was full (never expected)
    double *lossq = nullptr;           // per query: its KL term sum of the last loss iteration
    double *loss_d = nullptr;          // device: loss values in the order of loss_keys
    int32_t loss_cap = 0;
    std::vector<int32_t> loss_keys;
    int32_t since_sort = 0;            // steps since the queries were last sorted
};

// computeRepulsiveForce (QuadTree.scala:123-152) of the tree of the n points
// of dY (n x c, c = 2: the quadtree, 3: the octree) for the m foreign points
// dQ: dF (m x c) and dz (m), caller's order.
void repulsion_queries_device(tsne_ctx *ctx, const double *dY, int64_t n, int32_t c, double theta, const double *dQ,
                              int64_t m, double *dF, double *dz);
// y_i = sum_e P_e Yref[col_e] (rows of c), sequential in CSR order (separate multiply and add)
void transform_init_device(tsne_ctx *ctx, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_P,
                           int64_t m, const double *d_Yref, int64_t n, int32_t c, double *d_Y);
// The map's dimension of a transform, params->n_components.  allow3 (the _c
// entry points): 3 is the 3-D transform; otherwise it is
// TSNE_ERR_UNSUPPORTED, as any value but 2 and 3 always is.
int32_t transform_dim(const tsne_params *p, bool allow3);
void transform_setup(tsne_ctx *ctx, const tsne_params *p, const double *d_Yref, int64_t n,
                     const int64_t *d_row_ptr, const int32_t *d_col, const double *d_P, int64_t m, double *d_Y,
                     double *d_upd, double *d_gains, bool allow3 = false);
void transform_step(tsne_ctx *ctx, int32_t t);
void transform_sync(tsne_ctx *ctx);
int32_t transform_losses(tsne_ctx *ctx, int32_t *keys, double *vals, int32_t cap);
void transform_destroy(tsne_ctx *ctx);   // the transform state and tsne_repulsion_queries[_c]'s trees
// Fails (TSNE_ERR_HIP) if a walk of repulsion_queries_device on the tree of a
// c-dimensional map met a full stack since its flag was cleared; synchronises.
void walk_flag_check(tsne_ctx *ctx, int32_t c);
// wave pops of the last repulsion_queries_device walk of a 3-D map run under
// option transform_stats (tsne_ctx_counter "xform3.pops"; 0 if none); synchronises
int64_t transform_pops(tsne_ctx *ctx);

}  // namespace tsne
