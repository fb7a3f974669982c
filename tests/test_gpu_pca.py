"""PCA on the device (tsne-flink_amd/csrc/pca.hip): column means, the centred
Gram matrix on the fp64 MFMA, the host eigen-solve, the projection and the PCA
initialisation of the working set, against numpy in extended precision.

Planted data, so that the leading eigenvectors are well defined:
X = (G diag(1.6^-j)) Q^T 3 + offset, G standard normal, Q orthogonal, offset a
row of magnitude ~50 (which a one-pass covariance would not survive).

The shapes cover d below 16, d no multiple of 16, d across the 128-column
panel edge (130, 257: 2 and 3 panels), n no multiple of 4, n below one
2048-row chunk, and several chunks with a ragged last one (4099, 20001).

Every tolerance is a rounding bound of the sums involved (u = 2^-53):
  mean         n u max|X|                      n sequential additions
  C_jk         4 n u sqrt(C_jj C_kk)           centring + n products and additions
  V V^T - I    64 d u                          symmetric eigen-solver backward error
  C v - l v    64 d u lambda_1
  scores       4 d u max_i |x_i - mean|_2      d products and additions, |v| = 1
"""
import numpy as np
import pytest

import tsne_amd as T
from tsne_amd.api import default_params

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SHAPES = [(2, 3), (5, 17), (67, 33), (4099, 130), (1500, 257), (20001, 40)]


def planted(n, d, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * n + d)
    G = rng.normal(size=(n, d)) * 1.6 ** -np.arange(d)
    Q, _ = np.linalg.qr(rng.normal(size=(d, d)))
    offset = rng.normal(size=d) * 50
    return np.ascontiguousarray(G @ Q.T * 3 + offset)


_cache = {}


def case(n, d):
    """(X, longdouble mean, longdouble two-pass covariance), computed once per shape."""
    if (n, d) not in _cache:
        X = planted(n, d)
        Xl = X.astype(np.longdouble)
        mean = Xl.sum(axis=0) / n
        Xc = Xl - mean
        cov = np.empty((d, d), dtype=np.longdouble)
        for j in range(d):          # column by column: longdouble has no BLAS, keep the temporaries small
            cov[j] = (Xc * Xc[:, j:j + 1]).sum(axis=0) / n
        X.setflags(write=False)
        _cache[(n, d)] = (X, mean, cov)
    return _cache[(n, d)]


@pytest.fixture(scope="module")
def ctx():
    with T.Context(0) as c:
        yield c


def signed(V):
    big = np.abs(V).argmax(axis=1)
    return V * np.sign(V[np.arange(len(V)), big])[:, None]


@pytest.mark.parametrize("n,d", SHAPES)
def test_mean_and_covariance(ctx, n, d):
    X, mean_ref, cov_ref = case(n, d)
    mean, C = ctx.pcaCovariance(X)
    err_m = np.abs(mean - mean_ref).max()
    bound_m = n * U * np.abs(X).max()
    sd = np.sqrt(np.diag(cov_ref).astype(np.float64))
    ratio = (np.abs(C - cov_ref).astype(np.float64) / (4 * n * U * np.outer(sd, sd))).max()
    print(f"n={n} d={d}: mean error {float(err_m):.3g} (bound {bound_m:.3g}), covariance error / bound {ratio:.3g}")
    assert err_m <= bound_m
    assert ratio <= 1.0
    assert np.array_equal(C, C.T)


def check_pca(ctx, n, d, c_out):
    X, _, cov_ref = case(n, d)
    scores, comp, eig, mean = ctx.pca(X, c_out)
    mean2, C = ctx.pcaCovariance(X)
    assert np.array_equal(mean, mean2)
    assert scores.shape == (n, c_out) and comp.shape == (c_out, d) and eig.shape == (c_out,)
    assert np.all(eig[:-1] >= eig[1:])
    big = np.abs(comp).argmax(axis=1)
    assert np.all(comp[np.arange(c_out), big] > 0)
    assert np.abs(comp @ comp.T - np.eye(c_out)).max() <= 64 * d * U
    assert np.abs(C @ comp.T - comp.T * eig).max() <= 64 * d * U * eig[0]
    # numpy's vectors of the extended-precision covariance, on the well-separated
    # components only.  A vector moves by about |dC| / gap: |dC| <= 4 n u d lambda_1
    # (the bound above over a row) is < 4e-10 lambda_1 for every shape here, the
    # planted gaps are ~0.6 lambda_a, and 1 - 1e-9 allows an angle of 4e-5: so
    # lambda_a >= 1e-4 lambda_1 is safe (all of the leading four; the trailing
    # ones of the c_out = d case, down to 1e-13 lambda_1, are not determined by C).
    wr, Vr = np.linalg.eigh(cov_ref.astype(np.float64))
    sep = eig >= 1e-4 * eig[0]
    assert sep[:min(4, c_out)].all()
    Vr = signed(Vr.T[::-1])[:c_out]
    dots = np.sum(comp * Vr, axis=1)[sep]
    assert dots.min() >= 1 - 1e-9, dots
    Xc = X - mean
    ref = Xc.astype(np.longdouble) @ comp.T.astype(np.longdouble)
    bound = 4 * d * U * np.sqrt((Xc * Xc).sum(axis=1)).max()
    err = np.abs(scores - ref).max()
    print(f"n={n} d={d} c_out={c_out}: score error {float(err):.3g} (bound {bound:.3g})")
    assert err <= bound
    return scores, comp, eig, mean


@pytest.mark.parametrize("n,d", SHAPES)
def test_pca_leading_components(ctx, n, d):
    check_pca(ctx, n, d, min(4, n - 1, d))


@pytest.mark.parametrize("c_out", [1, 33])
def test_pca_one_and_all_components(ctx, c_out):
    check_pca(ctx, 67, 33, c_out)


def test_component_does_not_depend_on_c_out(ctx):
    X, _, _ = case(67, 33)
    s4, v4, e4, _ = ctx.pca(X, 4)
    s33, v33, e33, _ = ctx.pca(X, 33)
    assert np.array_equal(s4, s33[:, :4]) and np.array_equal(v4, v33[:4]) and np.array_equal(e4, e33[:4])


@pytest.mark.parametrize("n,d", [(67, 33), (4099, 130), (20001, 40)])
def test_repeatable_and_host_equals_device_form(ctx, n, d):
    import torch
    X, _, _ = case(n, d)
    c_out = 4
    first = ctx.pca(X, c_out) + ctx.pcaCovariance(X) + ctx.initWorkingSetPCA(X, 3)
    again = ctx.pca(X, c_out) + ctx.pcaCovariance(X) + ctx.initWorkingSetPCA(X, 3)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    dev = torch.device("cuda", 0)
    dX = torch.from_numpy(np.array(X)).to(dev)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)   # noqa: E731
    ds, dv, de, dm = z(n, c_out), z(c_out, d), z(c_out), z(d)
    ctx.dev_pca(dX, c_out, dm, dv, de, ds)
    dm2, dC = z(d), z(d, d)
    ctx.dev_pca_covariance(dX, dm2, dC)
    dY, du, dg = z(n, 3), z(n, 3), z(n, 3)
    ctx.dev_init_working_set_pca(dX, dY, du, dg)
    ctx.synchronize()
    got = [t.cpu().numpy() for t in (ds, dv, de, dm, dm2, dC, dY, du, dg)]
    for a, b in zip(first, got):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("c", [2, 3])
def test_pca_initialisation(ctx, c):
    n, d = 67, 33
    X, _, _ = case(n, d)
    scores, _, eig, _ = ctx.pca(X, c)
    Y, upd, gains = ctx.initWorkingSetPCA(X, c)
    ref = scores * (1e-4 / np.sqrt(eig[0]))
    assert np.all(np.abs(Y - ref) <= 2 * np.spacing(np.abs(ref)))
    assert abs(np.std(Y[:, 0]) - 1e-4) <= 1e-12 * 1e-4
    assert np.all(upd == 0) and np.all(gains == 1)
    k = 15
    idx, dist = ctx.kNearestNeighbors(X, k)
    rp = np.arange(0, n * k + 1, k, dtype=np.int64)
    p = ctx.pairwiseAffinities(rp, dist.ravel(), 5.0)
    jr, jc, jv = ctx.jointDistribution(rp, idx.ravel(), p, n)
    loss = ctx.optimize(jr, jc, jv, Y, upd, gains, default_params(iterations=20, theta=0.5, n_components=c))
    assert np.isfinite(Y).all() and all(np.isfinite(v) for v in loss.values())


def test_argument_errors(ctx):
    rng = np.random.default_rng(0)
    X = rng.normal(size=(67, 70))

    def status(fn, *a):
        with pytest.raises(T.TsneError) as e:
            fn(*a)
        return e.value.status

    assert status(ctx.initWorkingSetPCA, np.full((67, 33), 2.5), 2) == -1      # constant data: lambda_1 = 0
    assert status(ctx.pca, X, 65) == -1                                        # c_out > 64
    assert status(ctx.pca, X[:, :3], 4) == -1                                  # c_out > d
    assert status(ctx.pca, X[:1], 1) == -1                                     # n = 1
    assert status(ctx.pcaCovariance, X[:1]) == -1
    assert status(ctx.initWorkingSetPCA, X[:, :2], 3) == -1                    # c > d
    assert status(ctx.pca, rng.normal(size=(2, 2049)), 1) == -4                # d > 2048
    assert status(ctx.pcaCovariance, rng.normal(size=(2, 2049))) == -4
    assert status(ctx.initWorkingSetPCA, X, 4) == -4                           # c not 2 or 3
    scores, comp, eig, mean = ctx.pca(X, 64)                                   # the limits themselves are fine
    assert scores.shape == (67, 64)
