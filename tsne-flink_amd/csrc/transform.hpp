// transform.hpp -- embedding new points into a fitted map: Barnes-Hut
// repulsion for query points that are not in the tree, and the optimizer that
// moves only the new points (transform.hip for 2-D maps, transform3.hip for
// 3-D ones).
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
// of dY for the m foreign points dQ: dF (m x 2) and dz (m), caller's order.
void repulsion_queries_device(tsne_ctx *ctx, const double *dY, int64_t n, double theta, const double *dQ, int64_t m,
                              double *dF, double *dz);
// y_i = sum_e P_e Yref[col_e], sequential in CSR order (separate multiply and add)
void transform_init_device(tsne_ctx *ctx, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_P,
                           int64_t m, const double *d_Yref, int64_t n, double *d_Y);
// allow3: params->n_components == 3 sets up the 3-D transform (the _c entry
// points); otherwise it is TSNE_ERR_UNSUPPORTED, as any other value always is
void transform_setup(tsne_ctx *ctx, const tsne_params *p, const double *d_Yref, int64_t n,
                     const int64_t *d_row_ptr, const int32_t *d_col, const double *d_P, int64_t m, double *d_Y,
                     double *d_upd, double *d_gains, bool allow3 = false);
void transform_step(tsne_ctx *ctx, int32_t t);
void transform_sync(tsne_ctx *ctx);
int32_t transform_losses(tsne_ctx *ctx, int32_t *keys, double *vals, int32_t cap);
void transform_destroy(tsne_ctx *ctx);   // the transform state and tsne_repulsion_queries[_c]'s trees
// The flag word of the walks on the tree with workspace prefix `pre`, cleared
int32_t *walk_flag(tsne_ctx *ctx, const std::string &pre);
// Fails (TSNE_ERR_HIP) if a walk on the tree with workspace prefix `pre`
// ("bhx." / "bhx1." / "octx." / "octx1.") met a full stack since its flag was
// cleared; synchronises.
void walk_flag_check(tsne_ctx *ctx, const char *pre);

// ---- 3-D maps (transform3.hip): the same operators over the octree of dY /
// d_Yref (n x 3); F, Y, upd, gains are m x 3.
void repulsion_queries3_device(tsne_ctx *ctx, const double *dY, int64_t n, double theta, const double *dQ, int64_t m,
                               double *dF, double *dz);
void transform_init3_device(tsne_ctx *ctx, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_P,
                            int64_t m, const double *d_Yref, int64_t n, double *d_Y);
// the pieces transform_setup / transform_step dispatch to when s->dim == 3:
// the tree of s->Yref with the flag and the first sort; the Morton sort of
// s->Y; the launches of one iteration (fused, or split under transform_split)
void transform3_build(tsne_ctx *ctx, TransformState *s);
void transform3_sort(tsne_ctx *ctx, TransformState *s);
void transform3_launch(tsne_ctx *ctx, TransformState *s, double ex, double mom, bool loss);
// wave pops of the last repulsion_queries3_device walk run under option
// transform_stats (tsne_ctx_counter "xform3.pops"; 0 if none); synchronises
int64_t transform3_pops(tsne_ctx *ctx);

}  // namespace tsne
