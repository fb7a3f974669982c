// metric.hpp -- the exact breeze metric in fp64, shared by the kNN's re-rank
// (knn.hip) and the rank scan (ranks.hip): one definition, so a distance the
// kNN returns and a distance the rank kernel counts by have the same bits.
#pragma once

#include "common.hpp"

namespace tsne {

// breeze norm(): the sequential sum of squares, no FMA contraction (the cosine
// metric's |a|; prep_rows keeps it per row as norm64)
__device__ __forceinline__ double exact_norm(const double *__restrict__ x, int32_t d) {
    double s = 0.0;
    for (int32_t c = 0; c < d; ++c) s = __dadd_rn(s, __dmul_rn(x[c], x[c]));
    return sqrt(s);
}

// The metric's value from the finished sequential sum s (of (a_t - b_t)^2, or
// of a_t b_t for cosine).
__device__ __forceinline__ double metric_finish(double s, int32_t metric, double na, double nb) {
    if (metric == TSNE_METRIC_COSINE) return 1.0 - s / (na * nb);
    return metric == TSNE_METRIC_EUCLIDEAN ? sqrt(s) : s;
}

// Exact breeze metric in fp64, sequential over the coordinates (no FMA).
__device__ __forceinline__ double exact_metric(const double *__restrict__ a,
                                               const double *__restrict__ b, int32_t d,
                                               int32_t metric, double na, double nb) {
    if (metric == TSNE_METRIC_COSINE) {
        double s = 0.0;
        for (int32_t t = 0; t < d; ++t) s = __dadd_rn(s, __dmul_rn(a[t], b[t]));
        return 1.0 - s / (na * nb);
    }
    double s = 0.0;
    for (int32_t t = 0; t < d; ++t) {
        double df = __dsub_rn(a[t], b[t]);
        s = __dadd_rn(s, __dmul_rn(df, df));
    }
    return metric == TSNE_METRIC_EUCLIDEAN ? sqrt(s) : s;
}

}  // namespace tsne
