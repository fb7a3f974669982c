// pca_eig.hpp -- host eigen-solver of the PCA operators (pca_eig.cpp).  Plain
// C++: no HIP include, so a stand-alone program can build it with g++.
#pragma once

namespace tsne {

// All d eigenpairs of the symmetric d x d matrix A (row-major fp64; the lower
// triangle is read): Householder tridiagonalisation, then implicit-shift QL.
// evals[d] descending (equal values keep the solver's order); evecs is d x d,
// row a = the unit eigenvector of evals[a], signed so that its coordinate of
// largest absolute value is positive (ties: the lowest index decides).
// Single-threaded and deterministic.  Returns 0, 1 for a non-finite entry of
// A or d < 1, 2 if an eigenvalue did not converge.
int sym_eig(const double *A, int d, double *evals, double *evecs);

}  // namespace tsne
