// ranks.hpp -- exact neighbour ranks and the rank-based scores of a map
// (ranks.hip; include/tsne_hip.h "scoring a map").
#pragma once

#include "common.hpp"

namespace tsne {

constexpr int32_t RANKS_MAX_M = 1024;   // candidates per row: the threshold sort's LDS capacity

// rank[a * m + e] = rank_A(rows[a], cand[a * m + e]): 0 for the row itself, else
// 1 + the number of points l != i with (dkey(D(i, l)), l) < (dkey(D(i, j)), j),
// D the exact fp64 metric of metric.hpp.  d_rows NULL: row a is point a (s <= n).
// Ids are trusted (the host entry points validate them).  Enqueues on
// ctx->stream; workspace under "ranks.*".  The scan's time is the stage timer
// "ranks.scan" (one interval per call; reset_timer drops the earlier ones).
void ranks_device(tsne_ctx *ctx, const double *dA, int64_t n, int32_t d, int32_t metric, const int64_t *d_rows,
                  int64_t s, const int32_t *d_cand, int32_t m, int32_t *d_rank, bool reset_timer = true);

// The three integer sums S_T, S_C, S_R over the scored rows (sums_out, host)
// and per row (d_row_sums, s x 3 on the device; may be NULL).  Synchronises.
// Workspace under "quality.*" (and the kNN's and the rank scan's own).
void quality_device(tsne_ctx *ctx, const double *dX, int64_t n, int32_t d, int32_t metric, const double *dY, int32_t c,
                    int32_t k, const int64_t *d_rows, int64_t s, int64_t *d_row_sums, int64_t sums_out[3]);

// trustworthiness / continuity from S_T / S_C, recall from S_R
inline double quality_trust(int64_t sum, int64_t n, int64_t k, int64_t s) {
    return 1.0 - 2.0 * (double)sum / ((double)s * (double)k * (double)(2 * n - 3 * k - 1));
}
inline double quality_recall(int64_t sum, int64_t k, int64_t s) { return (double)sum / ((double)s * (double)k); }

}  // namespace tsne
