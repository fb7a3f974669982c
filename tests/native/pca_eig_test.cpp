// Stand-alone check of tsne::sym_eig (tsne-flink_amd/csrc/pca_eig.cpp), built
// by tests/test_pca_host.py with -fsanitize=address,undefined: random symmetric
// matrices, the identity and a rank-1 matrix at d = 1, 2, 17, 130; every
// result must satisfy the solver's invariants.  Prints "ok", exits 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pca_eig.hpp"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
double uniform() {   // splitmix64 -> (-1, 1)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1.0p-52 - 1.0;
}

bool check(const std::vector<double> &A, int d, const char *what) {
    const size_t N = (size_t)d;
    std::vector<double> w(N), V(N * N);
    if (tsne::sym_eig(A.data(), d, w.data(), V.data()) != 0) {
        std::printf("%s d=%d: solver failed\n", what, d);
        return false;
    }
    double lmax = 0;
    for (size_t a = 0; a < N; ++a) lmax = std::fmax(lmax, std::fabs(w[a]));
    const double tol = 64.0 * d * 0x1.0p-53;
    for (size_t a = 0; a + 1 < N; ++a)
        if (!(w[a] >= w[a + 1])) {
            std::printf("%s d=%d: eigenvalues not descending at %zu\n", what, d, a);
            return false;
        }
    for (size_t a = 0; a < N; ++a) {
        const double *v = &V[a * N];
        size_t big = 0;
        for (size_t j = 1; j < N; ++j)
            if (std::fabs(v[j]) > std::fabs(v[big])) big = j;
        if (!(v[big] > 0)) {
            std::printf("%s d=%d: sign rule broken for vector %zu\n", what, d, a);
            return false;
        }
        for (size_t i = 0; i < N; ++i) {   // residual of A v = lambda v
            double s = 0;
            for (size_t j = 0; j < N; ++j) s += A[i * N + j] * v[j];
            if (!(std::fabs(s - w[a] * v[i]) <= tol * std::fmax(lmax, 1e-300))) {
                std::printf("%s d=%d: residual %g of pair %zu\n", what, d, std::fabs(s - w[a] * v[i]), a);
                return false;
            }
        }
        for (size_t b = 0; b < N; ++b) {   // orthonormal rows
            double s = 0;
            for (size_t j = 0; j < N; ++j) s += v[j] * V[b * N + j];
            if (!(std::fabs(s - (a == b ? 1.0 : 0.0)) <= tol)) {
                std::printf("%s d=%d: V V^T - I = %g at (%zu, %zu)\n", what, d, s - (a == b), a, b);
                return false;
            }
        }
    }
    return true;
}

}  // namespace

int main() {
    const int dims[] = {1, 2, 17, 130};
    bool ok = true;
    for (int d : dims) {
        const size_t N = (size_t)d;
        std::vector<double> A(N * N);
        for (size_t i = 0; i < N; ++i)
            for (size_t j = 0; j <= i; ++j) A[i * N + j] = A[j * N + i] = uniform();
        ok = check(A, d, "random") && ok;
        std::vector<double> I(N * N, 0.0);
        for (size_t i = 0; i < N; ++i) I[i * N + i] = 1.0;
        ok = check(I, d, "identity") && ok;
        std::vector<double> u(N), R(N * N);
        for (size_t i = 0; i < N; ++i) u[i] = uniform();
        for (size_t i = 0; i < N; ++i)
            for (size_t j = 0; j < N; ++j) R[i * N + j] = u[i] * u[j];
        ok = check(R, d, "rank-1") && ok;
    }
    double bad[4] = {1.0, NAN, NAN, 1.0}, w[2], V[4];
    ok = (tsne::sym_eig(bad, 2, w, V) == 1) && ok;
    if (ok) std::printf("ok\n");
    return ok ? 0 : 1;
}
