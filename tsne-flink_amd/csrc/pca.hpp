// pca.hpp -- principal components of the input rows on the device (pca.hip).
//
// Definitions (the contract of tsne_[dev_]pca*, include/tsne_hip.h).  For X
// (n x d, fp64, row-major):
//   mu_j   = (1/n) sum_i X_ij
//   C      = (1/n) sum_i (x_i - mu)(x_i - mu)^T      two-pass: the rows are
//            centred before the products, never X^T X / n - mu mu^T
//   lambda_1 >= lambda_2 >= ... the eigenvalues of C, v_1, v_2, ... the unit
//            eigenvectors, each signed so that its coordinate of largest
//            absolute value is positive (ties: the lowest index decides)
//   scores = (X - mu) V^T, n x c_out; score (i, a) is the sequential sum over
//            j = 0..d-1 of (X_ij - mu_j) * V_aj, each product and each sum
//            rounded (no contraction)
//   PCA initialisation with c columns: Y = scores[:, :c] * (1e-4 / sqrt(lambda_1)),
//            upd = 0, gains = 1; the first column of Y then has standard
//            deviation 1e-4, the scale of initWorkingSet's N(0, 1e-4^2).
//            lambda_1 <= 0 (constant data) is TSNE_ERR_ARG.
// Every sum runs in a fixed order that depends on n and d only -- never on the
// device's CU count -- and no floating-point atomic is used: the same call on
// the same data gives the same bits, and the host-buffer and device-buffer
// forms give the same bits.
//
// Kernels.  pca_colmean_partial sums every column over chunks of 1024 rows
// (four interleaved row lanes per chunk, combined in lane order) and
// pca_colmean_final adds the chunks over 16 interleaved chunk lanes, combined
// in lane order.  pca_gram accumulates the
// centred Gram matrix on v_mfma_f64_16x16x4_f64: d is padded to d_pad (a
// multiple of 16) with zero columns, a workgroup of 8 waves takes one chunk of
// rows and one pair (pi <= pj) of column panels of at most 128 columns, stages
// 32 rows at a time in LDS with mu subtracted (zero rows past the chunk's end),
// and each wave owns up to 8 of the pair's 16 x 16 tiles (I <= J only),
// 8 VGPRs of accumulator each.  Every row of X is read once per panel pair: once
// in total for d <= 128.  Each (chunk, tile) partial goes to a workspace;
// pca_gram_reduce adds the chunks in index order, divides by n and writes
// both triangles from the upper one, so C is exactly symmetric.
//
// Chunks: 2048 rows, doubled until the workspace chunks * d_pad^2 * 8 bytes
// is at most 256 MiB (PCA_GRAM_WS_BYTES).  d <= 2048 (PCA_MAX_D; C then
// crosses to the host eigen-solver, pca_eig.hpp, as at most 32 MB),
// c_out <= 64 (PCA_MAX_OUT).
#pragma once

#include "common.hpp"
#include "pca_eig.hpp"

namespace tsne {

constexpr int PCA_MAX_D = 2048;
constexpr int PCA_MAX_OUT = 64;
constexpr int64_t PCA_GRAM_ROWS = 2048;
constexpr int64_t PCA_GRAM_WS_BYTES = (int64_t)256 << 20;

// rows per pca_gram chunk for an n x d input (a function of n and d only)
int64_t pca_gram_chunk_rows(int64_t n, int32_t d);

// All pointers on the context's device; work is enqueued on its stream.
// d_mean: d, d_cov: d x d.
void pca_covariance_device(tsne_ctx *ctx, const double *dX, int64_t n, int32_t d, double *d_mean, double *d_cov);
// d_mean: d, d_comp: c_out x d, d_eig: c_out, d_scores: n x c_out; any may be
// NULL.  Synchronises the stream (C goes through the host eigen-solver).
void pca_device(tsne_ctx *ctx, const double *dX, int64_t n, int32_t d, int32_t c_out, double *d_mean, double *d_comp,
                double *d_eig, double *d_scores);
// dY, dupd, dgains: n x c, c = 2 or 3.
void pca_init_device(tsne_ctx *ctx, const double *dX, int64_t n, int32_t d, int32_t c, double *dY, double *dupd,
                     double *dgains);

}  // namespace tsne
