// transform.hpp -- embedding new points into a fitted map: Barnes-Hut
// repulsion for query points that are not in the tree, and the optimizer that
// moves only the new points (transform.hip).
#pragma once
#include "bhtree.hpp"

namespace tsne {

// The device-resident transform (tsne_dev_transform_*): the reference map's
// tree, built once at setup, and the new points' working set, which stays in
// the caller's buffers and order (a step reads and writes it in place through
// the Morton permutation of the queries).
struct TransformState {
    BHTree tree;                       // the reference map's tree ("bhx.")
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
void transform_setup(tsne_ctx *ctx, const tsne_params *p, const double *d_Yref, int64_t n,
                     const int64_t *d_row_ptr, const int32_t *d_col, const double *d_P, int64_t m, double *d_Y,
                     double *d_upd, double *d_gains);
void transform_step(tsne_ctx *ctx, int32_t t);
void transform_sync(tsne_ctx *ctx);
int32_t transform_losses(tsne_ctx *ctx, int32_t *keys, double *vals, int32_t cap);
void transform_destroy(tsne_ctx *ctx);   // the transform state and tsne_repulsion_queries' tree
// Fails (TSNE_ERR_HIP) if a walk on the tree with workspace prefix `pre`
// ("bhx." / "bhx1.") met a full stack since its flag was cleared; synchronises.
void walk_flag_check(tsne_ctx *ctx, const char *pre);

}  // namespace tsne
