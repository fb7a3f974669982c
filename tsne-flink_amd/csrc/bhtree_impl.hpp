// bhtree_impl.hpp -- internal to the quadtree: what bhtree_build.hip (the build),
// bhtree.hip (the evaluation) and bhpart.hip (the several-rank helpers) share.
// Included by those three files only; the rest of the library sees bhtree.hpp.
// A constant or helper that one of the three uses alone lives in that file.
#pragma once

#include "bhtree.hpp"

namespace tsne {
namespace {

// ---- Subtree moments (the all-open fast path, see bh_traverse)
// For a subtree every cell of which a query would open, the reference sums
// 1/(1+D) and (q-y)/(1+D)^2 over all of the subtree's points (A15 at every
// leaf).  With u = y - c about the subtree's bounding-box centre c, v = q - c,
// A = |v|^2, E = D - A = |u|^2 - 2 v.u and B = 1/(1+A):
//   1/(1+D)   = B   sum_k (-B E)^k,        1/(1+D)^2 = B^2 sum_k (k+1) (-B E)^k,
// a series in rho = B max|E| <= B (R^2 + 2 |v| R) (R = the box half-diagonal).
// Truncated at k = MOM_ORDER, every term is a polynomial of degree <= 2k+1 in
// u, so the subtree sums follow from its moments sum u_x^a u_y^b
// (a + b <= MOM_DEG), shifted to the query.  The path is taken only when the
// truncation bound (MOM_ORDER+2) rho^(MOM_ORDER+1) / (1-rho)^2 <= Options::mom_tol (1e-12),
// i.e. the result equals the reference's exact leaf sum to ~1e-14 relative
// (fp64 rounding level); otherwise the dense leaf tile runs.  This turns the
// near-exact O(N^2) phase of a small embedding into
// O(N) moment evaluations.
constexpr int MOM_ORDER = 4;
constexpr int MOM_DEG = 2 * MOM_ORDER + 1;
constexpr int MOM_K = (MOM_DEG + 1) * (MOM_DEG + 2) / 2;
constexpr int MOM_MIN_POINTS = 64;
// moment (a, b), a + b <= MOM_DEG: rows of decreasing length
__host__ __device__ constexpr int midx(int a, int b) { return a * (MOM_DEG + 1) - a * (a - 1) / 2 + b; }

// ---- The same sums as polynomials in v (root-tile mode: ONE subtree for
// every query).  moment_eval computes z = sum_i om_i(A) Qz_i(v) with
//   Qz_i(v) = sum_{a+b=2i, a,b even} C(i, a/2) a! b! nu(a, b),
//   nu(a, b) = sum_{p<=a, q<=b} mu(a-p, b-q) (-v_x)^p (-v_y)^q / (p! q!),
// a polynomial of degree 2i in (v_x, v_y); gx / gy likewise with ph_i and
// Qx_i (a odd) / Qy_i (b odd) of degree 2i+1.  Their POLY_K coefficients
// depend on the subtree's moments only: poly_coef computes them once, and a
// query evaluates 3 (MOM_ORDER+1) small polynomials by Horner with uniform
// (scalar-loaded) coefficients instead of shifting the moments itself --
// ~40 VGPRs instead of 256 + spills.
__host__ __device__ constexpr int poly_len(int d) { return (d + 1) * (d + 2) / 2; }
__host__ __device__ constexpr int poly_off_z(int i) { return i == 0 ? 0 : poly_off_z(i - 1) + poly_len(2 * i - 2); }
constexpr int POLY_X = poly_off_z(MOM_ORDER + 1);
__host__ __device__ constexpr int poly_off_x(int i) { return i == 0 ? POLY_X : poly_off_x(i - 1) + poly_len(2 * i - 1); }
constexpr int POLY_Y = poly_off_x(MOM_ORDER + 1);
__host__ __device__ constexpr int poly_off_y(int i) { return POLY_Y + poly_off_x(i) - POLY_X; }
constexpr int POLY_K = POLY_Y + (POLY_Y - POLY_X);
static_assert(POLY_K == 345, "MOM_ORDER 4: 95 + 125 + 125 coefficients");

// Waves per block of the 64-query traversal (a block holds its LDS and wave
// slots until its last wave ends; 2 instead of 4: C3 loop 5.03 / 5.02 vs
// 5.03 / 5.04 s, t = 450 snapshot span 13.6 vs 13.5 ms -- not the limiter,
// round 6)
#ifndef TRAV_WPB
#define TRAV_WPB 4
#endif

// Tree partition (several ranks; see "Tree partition" in bhtree.hip): the flag
// of a ref pushed in exact-sum mode, and the cell level the ranks' cuts sit on.
constexpr int32_t REF_FORCED = 1 << 30;
constexpr int PART_LEVEL = 10;

__device__ __forceinline__ void box_centre(double bx0, double bx1, double by0, double by1, double &cx, double &cy,
                                           double &R) {
    cx = 0.5 * (bx0 + bx1);
    cy = 0.5 * (by0 + by1);
    const double ex = 0.5 * (bx1 - bx0), ey = 0.5 * (by1 - by0);
    R = sqrt(ex * ex + ey * ey) * (1.0 + 1e-12);
}
__device__ __forceinline__ void box_centre(const BHNode &nd, double &cx, double &cy, double &R) {
    box_centre(nd.bx0, nd.bx1, nd.by0, nd.by1, cx, cy, R);
}

}  // namespace

// The subtree moments of a finished build on stream ms: bh_repulsion launches
// the ones bh_build deferred (Options::build_fuse).  count_threads:
// moment_count's workgroup size (a multiple of 64, <= 1024; the moments do
// not depend on it, only the placement of the nodes' item ranges).
void bh_moments(BHTree &t, hipStream_t ms, int count_threads = 1024);

// The build's share of bh_alloc, in its place in the allocation order: the
// tree's own buffers (ends with a stream synchronisation: mom_flag's initial
// copy), then the build's temporaries, root-tile tables and sort buffers.
void bh_alloc_tree(tsne_ctx *ctx, BHTree &t, int64_t n, const std::string &pre);
void bh_alloc_build_tmp(tsne_ctx *ctx, BHTree &t, int64_t n, const std::string &pre);

}  // namespace tsne
