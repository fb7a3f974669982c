"""Host side of the PCA operators: tsne_sym_eig (tsne-flink_amd/csrc/pca_eig.cpp,
Householder tridiagonalisation + implicit-shift QL) against numpy.linalg.eigh,
its invariants on matrices with repeated eigenvalues, and the stand-alone
sanitizer build of the solver.  No GPU is touched: tsne_sym_eig takes no context.

Every tolerance is the backward-error scale of a symmetric eigen-solver,
64 * d * 2^-53 (relative to the largest |eigenvalue| where the quantity scales
with the matrix)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import tsne_amd as T

ROOT = Path(__file__).resolve().parent.parent
U = 2.0 ** -53


def check_invariants(A, w, V):
    d = A.shape[0]
    lmax = np.abs(w).max()
    tol = 64 * d * U
    assert np.all(w[:-1] >= w[1:]), "eigenvalues not descending"
    assert np.abs(A @ V.T - V.T * w).max() <= tol * lmax
    assert np.abs(V @ V.T - np.eye(d)).max() <= tol
    big = np.abs(V).argmax(axis=1)          # first index of the largest |coordinate|
    assert np.all(V[np.arange(d), big] > 0), "sign rule"


def signed(Vref):
    big = np.abs(Vref).argmax(axis=1)
    return Vref * np.sign(Vref[np.arange(len(Vref)), big])[:, None]


@pytest.mark.parametrize("d", [1, 2, 3, 17, 64, 130])
def test_sym_eig_matches_eigh(d):
    rng = np.random.default_rng(100 + d)
    A = rng.normal(size=(d, d))
    A = (A + A.T) / 2
    w, V = T.sym_eig(A)
    check_invariants(A, w, V)
    wr, Vr = np.linalg.eigh(A)
    wr, Vr = wr[::-1], signed(Vr.T[::-1])
    assert np.abs(w - wr).max() <= 64 * d * U * np.abs(wr).max()
    # random symmetric matrices have simple eigenvalues: the vectors agree too
    # (to the gap-dependent accuracy of either solver; a loose sanity bound)
    assert np.abs(np.sum(V * Vr, axis=1)).min() >= 1 - 1e-6


@pytest.mark.parametrize("d", [1, 2, 3, 17, 64, 130])
def test_sym_eig_repeated_eigenvalues(d):
    """The identity and a rank-1 matrix: the eigenvectors of a repeated
    eigenvalue are not unique, so only the invariants are checked."""
    w, V = T.sym_eig(np.eye(d))
    check_invariants(np.eye(d), w, V)
    assert np.abs(w - 1).max() <= 64 * d * U
    u = np.random.default_rng(d).normal(size=d)
    A = np.outer(u, u)
    w, V = T.sym_eig(A)
    check_invariants(A, w, V)
    assert abs(w[0] - u @ u) <= 64 * d * U * (u @ u)
    assert np.abs(w[1:]).max(initial=0.0) <= 64 * d * U * (u @ u)


def test_sym_eig_is_deterministic_and_reads_the_lower_triangle():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(40, 40))
    A = (A + A.T) / 2
    w0, V0 = T.sym_eig(A)
    w1, V1 = T.sym_eig(np.tril(A))
    assert np.array_equal(w0, w1) and np.array_equal(V0, V1)
    w2, V2 = T.sym_eig(A)
    assert np.array_equal(w0, w2) and np.array_equal(V0, V2)


def test_sym_eig_argument_errors():
    with pytest.raises(T.TsneError) as e:
        T.sym_eig(np.array([[1.0, np.nan], [np.nan, 1.0]]))
    assert e.value.status == -1
    with pytest.raises(T.TsneError) as e:
        T.sym_eig(np.zeros((0, 0)))
    assert e.value.status == -1


def test_pca_eig_standalone_under_sanitizers(tmp_path):
    """tests/native/pca_eig_test.cpp + pca_eig.cpp as one program with its own
    main, built with AddressSanitizer and UBSan; d = 1, 2, 17, 130."""
    exe = tmp_path / "pca_eig_test"
    csrc = ROOT / "tsne-flink_amd" / "csrc"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", str(csrc),
                           str(ROOT / "tests" / "native" / "pca_eig_test.cpp"), str(csrc / "pca_eig.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
