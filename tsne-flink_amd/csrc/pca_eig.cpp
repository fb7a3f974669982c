// pca_eig.cpp -- symmetric eigen-solver on the host (see pca_eig.hpp).
//
// The two classical steps (EISPACK tred2 / tql2, as in Numerical Recipes and
// JAMA): Householder reflections reduce A to tridiagonal form while their
// product is accumulated, then QL iterations with implicit Wilkinson shifts
// diagonalise it, rotating the accumulated basis.  The basis is kept with one
// eigenvector per ROW during the QL phase, so each Givens rotation works on
// two contiguous rows.
#include "pca_eig.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <numeric>
#include <vector>

namespace tsne {
namespace {

// V (n x n, row-major) holds A on entry and the accumulated reflections
// (eigenvector basis of the tridiagonal form, as columns) on exit; d the
// diagonal, e the sub-diagonal in e[1..n).
void tridiagonalise(int n, double *V, double *d, double *e) {
    const size_t N = (size_t)n;
    for (int j = 0; j < n; ++j) d[j] = V[(N - 1) * N + j];
    for (int i = n - 1; i > 0; --i) {
        double scale = 0.0, h = 0.0;
        for (int k = 0; k < i; ++k) scale += std::fabs(d[k]);
        if (scale == 0.0) {
            e[i] = d[i - 1];
            for (int j = 0; j < i; ++j) {
                d[j] = V[(size_t)(i - 1) * N + j];
                V[(size_t)i * N + j] = 0.0;
                V[(size_t)j * N + i] = 0.0;
            }
        } else {
            for (int k = 0; k < i; ++k) {
                d[k] /= scale;
                h += d[k] * d[k];
            }
            double f = d[i - 1];
            double g = std::sqrt(h);
            if (f > 0) g = -g;
            e[i] = scale * g;
            h -= f * g;
            d[i - 1] = f - g;
            for (int j = 0; j < i; ++j) e[j] = 0.0;
            for (int j = 0; j < i; ++j) {
                f = d[j];
                V[(size_t)j * N + i] = f;
                g = e[j] + V[(size_t)j * N + j] * f;
                for (int k = j + 1; k <= i - 1; ++k) {
                    g += V[(size_t)k * N + j] * d[k];
                    e[k] += V[(size_t)k * N + j] * f;
                }
                e[j] = g;
            }
            f = 0.0;
            for (int j = 0; j < i; ++j) {
                e[j] /= h;
                f += e[j] * d[j];
            }
            const double hh = f / (h + h);
            for (int j = 0; j < i; ++j) e[j] -= hh * d[j];
            for (int j = 0; j < i; ++j) {
                f = d[j];
                g = e[j];
                for (int k = j; k <= i - 1; ++k) V[(size_t)k * N + j] -= (f * e[k] + g * d[k]);
                d[j] = V[(size_t)(i - 1) * N + j];
                V[(size_t)i * N + j] = 0.0;
            }
        }
        d[i] = h;
    }
    for (int i = 0; i < n - 1; ++i) {
        V[(N - 1) * N + i] = V[(size_t)i * N + i];
        V[(size_t)i * N + i] = 1.0;
        const double h = d[i + 1];
        if (h != 0.0) {
            for (int k = 0; k <= i; ++k) d[k] = V[(size_t)k * N + i + 1] / h;
            for (int j = 0; j <= i; ++j) {
                double g = 0.0;
                for (int k = 0; k <= i; ++k) g += V[(size_t)k * N + i + 1] * V[(size_t)k * N + j];
                for (int k = 0; k <= i; ++k) V[(size_t)k * N + j] -= g * d[k];
            }
        }
        for (int k = 0; k <= i; ++k) V[(size_t)k * N + i + 1] = 0.0;
    }
    for (int j = 0; j < n; ++j) {
        d[j] = V[(N - 1) * N + j];
        V[(N - 1) * N + j] = 0.0;
    }
    V[(N - 1) * N + (N - 1)] = 1.0;
    e[0] = 0.0;
}

// Z (n x n): row j = basis vector j on entry, eigenvector of d[j] on exit.
bool ql_implicit(int n, double *Z, double *d, double *e) {
    const size_t N = (size_t)n;
    for (int i = 1; i < n; ++i) e[i - 1] = e[i];
    e[n - 1] = 0.0;
    double f = 0.0, tst1 = 0.0;
    const double eps = std::ldexp(1.0, -52);
    for (int l = 0; l < n; ++l) {
        tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
        int m = l;
        while (m < n - 1 && std::fabs(e[m]) > eps * tst1) ++m;   // e[n-1] == 0 ends the search
        if (m > l) {
            int iter = 0;
            do {
                if (++iter > 60) return false;
                double g = d[l];
                double p = (d[l + 1] - g) / (2.0 * e[l]);
                double r = std::hypot(p, 1.0);
                if (p < 0) r = -r;
                d[l] = e[l] / (p + r);
                d[l + 1] = e[l] * (p + r);
                const double dl1 = d[l + 1];
                double h = g - d[l];
                for (int i = l + 2; i < n; ++i) d[i] -= h;
                f += h;
                p = d[m];
                double c = 1.0, c2 = c, c3 = c;
                const double el1 = e[l + 1];
                double s = 0.0, s2 = 0.0;
                for (int i = m - 1; i >= l; --i) {
                    c3 = c2;
                    c2 = c;
                    s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = std::hypot(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    double *z0 = Z + (size_t)i * N, *z1 = z0 + N;
                    for (int k = 0; k < n; ++k) {
                        h = z1[k];
                        z1[k] = s * z0[k] + c * h;
                        z0[k] = c * z0[k] - s * h;
                    }
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
            } while (std::fabs(e[l]) > eps * tst1);
        }
        d[l] = d[l] + f;
        e[l] = 0.0;
    }
    return true;
}

}  // namespace

int sym_eig(const double *A, int d, double *evals, double *evecs) {
    if (d < 1) return 1;
    const size_t N = (size_t)d;
    for (size_t i = 0; i < N * N; ++i)
        if (!std::isfinite(A[i])) return 1;
    std::vector<double> V(N * N), Z(N * N), w(N), e(N);
    for (size_t i = 0; i < N; ++i)   // the lower triangle, mirrored
        for (size_t j = 0; j <= i; ++j) V[i * N + j] = V[j * N + i] = A[i * N + j];
    tridiagonalise(d, V.data(), w.data(), e.data());
    for (size_t i = 0; i < N; ++i)
        for (size_t j = 0; j < N; ++j) Z[j * N + i] = V[i * N + j];
    if (!ql_implicit(d, Z.data(), w.data(), e.data())) return 2;
    std::vector<int> order(N);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return w[(size_t)a] > w[(size_t)b]; });
    for (size_t a = 0; a < N; ++a) {
        const double *z = Z.data() + (size_t)order[a] * N;
        size_t big = 0;
        for (size_t j = 1; j < N; ++j)
            if (std::fabs(z[j]) > std::fabs(z[big])) big = j;
        const double sgn = z[big] < 0 ? -1.0 : 1.0;
        evals[a] = w[(size_t)order[a]];
        for (size_t j = 0; j < N; ++j) evecs[a * N + j] = sgn * z[j];
    }
    return 0;
}

}  // namespace tsne
