"""Exact neighbour ranks (Context.neighborRanks) and the rank-based scores of a
map (Context.embeddingQuality): trustworthiness, continuity, kNN recall.

References: numpy (per-coordinate sums accumulated in index order, which have
the kernel's bits) and the CPU oracle's kNN with k = n - 1 (the position in its
row is the rank).  Every comparison of ranks and sums is array_equal."""
import ctypes as C

import numpy as np
import pytest

import oracle_ctypes as O
import tsne_amd as T
from tsne_amd.api import default_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with T.Context(0) as c:
        yield c


def seq_dist(X, rows, metric="sqeuclidean"):
    """D(i, l) for i in rows, every l: the coordinates accumulated one by one."""
    Q = X[rows]
    s = np.zeros((len(rows), len(X)))
    if metric == "cosine":
        nx = np.zeros(len(X))
        for t in range(X.shape[1]):
            s = s + Q[:, t, None] * X[None, :, t]
            nx = nx + X[:, t] * X[:, t]
        nx = np.sqrt(nx)
        return 1.0 - s / (nx[rows][:, None] * nx[None, :])
    for t in range(X.shape[1]):
        df = Q[:, t, None] - X[None, :, t]
        s = s + df * df
    return np.sqrt(s) if metric == "euclidean" else s


def ranks_from_dist(D, rows):
    """rank of every point per row: position by (D, index), the row's point removed by index."""
    n = D.shape[1]
    ids = np.arange(n)
    R = np.zeros(D.shape, dtype=np.int64)
    for a, i in enumerate(rows):
        order = np.lexsort((ids, D[a]))
        order = order[order != i]
        R[a, order] = np.arange(1, n)
        R[a, i] = 0
    return R


def ranks_from_oracle(X, metric):
    """n x n ranks: the position in the oracle's kNN row with k = n - 1."""
    n = len(X)
    oi, _ = O.knn(X, n - 1, metric)
    R = np.zeros((n, n), dtype=np.int64)
    R[np.arange(n)[:, None], oi] = np.arange(1, n)[None, :]
    return R


def take(R, cand):
    return np.take_along_axis(R, cand.astype(np.int64), axis=1)


# ------------------------------------------------------------------ 1. full order
@pytest.mark.parametrize("metric", ["sqeuclidean", "euclidean", "cosine"])
def test_ranks_against_full_order(ctx, metric):
    rng = np.random.default_rng(1)
    n, d, m = 777, 33, 37
    X = rng.normal(size=(n, d))
    R = ranks_from_oracle(X, metric)
    cand = rng.integers(0, n, (n, m)).astype(np.int32)
    cand[:, 5] = np.arange(n)                  # the row itself
    cand[:, 11] = np.argmax(R, axis=1)         # its farthest point
    got = ctx.neighborRanks(X, cand, metric=metric)
    assert got.dtype == np.int32 and got.shape == (n, m)
    assert np.array_equal(got[:, 5], np.zeros(n)) and np.array_equal(got[:, 11], np.full(n, n - 1))
    assert np.array_equal(got, take(R, cand))


# ------------------------------------------------------------------ 2. tiling edges
@pytest.mark.parametrize("d", [1, 2, 3])
def test_shapes_where_tiling_breaks(ctx, d):
    rng = np.random.default_rng(2 + d)
    n, s, m = 70_001, 130, 90
    X = rng.normal(size=(n, d))
    rows = rng.integers(0, n, s)
    rows[:4] = [n - 1, 0, 12345, 12345]        # both ends, a repeated id, unsorted
    cand = rng.integers(0, n, (s, m)).astype(np.int32)
    cand[:, 7] = cand[:, 3]                    # repeated candidates within a row
    cand[0, :3] = [0, n - 1, n - 1]
    R = ranks_from_dist(seq_dist(X, rows), rows)
    assert np.array_equal(ctx.neighborRanks(X, cand, rows=rows), take(R, cand))


# ------------------------------------------------------------------ 3. ties
def test_ties_on_a_lattice(ctx):
    rng = np.random.default_rng(3)
    n, m = 1000, 50
    X = rng.integers(0, 6, (n, 2)).astype(np.float64)     # ~27 exact duplicates of every point
    R = ranks_from_dist(seq_dist(X, np.arange(n)), np.arange(n))
    cand = rng.integers(0, n, (n, m)).astype(np.int32)
    cand[:, 0] = np.arange(n)
    assert np.array_equal(ctx.neighborRanks(X, cand), take(R, cand))
    Xc = rng.integers(1, 5, (n, 3)).astype(np.float64)    # no zero row
    Rc = ranks_from_oracle(Xc, "cosine")
    assert np.array_equal(ctx.neighborRanks(Xc, cand, metric="cosine"), take(Rc, cand))


# ------------------------------------------------------------------ 4. the kNN's own order
def test_agreement_with_the_knn(ctx):
    rng = np.random.default_rng(4)
    n, d, k = 3000, 16, 90
    X = rng.normal(size=(6, d))[rng.integers(0, 6, n)] * 4 + rng.normal(size=(n, d))
    idx, _ = ctx.kNearestNeighbors(X, k)
    got = ctx.neighborRanks(X, idx)
    assert np.array_equal(got, np.broadcast_to(np.arange(1, k + 1), (n, k)))


# ------------------------------------------------------------------ 5. threshold limits
@pytest.mark.parametrize("m", [1, 896])
def test_threshold_limits(ctx, m):
    rng = np.random.default_rng(5)
    n, d, s = 2000, 8, 70
    X = rng.normal(size=(n, d))
    rows = rng.permutation(n)[:s]
    cand = rng.integers(0, n, (s, m)).astype(np.int32)
    R = ranks_from_dist(seq_dist(X, rows), rows)
    assert np.array_equal(ctx.neighborRanks(X, cand, rows=rows), take(R, cand))


# ------------------------------------------------------------------ 6. independence
def test_subset_and_device_form(ctx):
    import torch
    rng = np.random.default_rng(6)
    n, d, m = 1500, 5, 40
    X = rng.normal(size=(n, d))
    cand = rng.integers(0, n, (n, m)).astype(np.int32)
    full = ctx.neighborRanks(X, cand)
    rows = rng.permutation(n)[:97]
    assert np.array_equal(ctx.neighborRanks(X, cand[rows], rows=rows), full[rows])
    strided = T.quality_rows(n, 100)
    assert np.array_equal(strided, (np.arange(100) * n) // 100)
    assert np.array_equal(ctx.neighborRanks(X, cand[strided], rows=100), full[strided])
    dX, dc = torch.from_numpy(X).cuda(), torch.from_numpy(cand).cuda()
    dr = torch.zeros((n, m), dtype=torch.int32, device="cuda")
    ctx.dev_neighbor_ranks(dX, dc, dr)
    ctx.synchronize()
    assert np.array_equal(dr.cpu().numpy(), full)
    drows = torch.from_numpy(rows).cuda()
    dcs = torch.from_numpy(np.ascontiguousarray(cand[rows])).cuda()
    drs = torch.zeros((len(rows), m), dtype=torch.int32, device="cuda")
    ctx.dev_neighbor_ranks(dX, dcs, drs, d_rows=drows)
    ctx.synchronize()
    assert np.array_equal(drs.cpu().numpy(), full[rows])


# ------------------------------------------------------------------ 7. scores
def scores_ref(RX, RY, k, rows=None):
    """sums, row_sums and the three doubles from full n x n rank matrices."""
    n = len(RX)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    NX = np.argsort(RX, axis=1, kind="stable")[:, 1:k + 1]     # rank 0 is the point itself
    NY = np.argsort(RY, axis=1, kind="stable")[:, 1:k + 1]
    rs = np.zeros((len(rows), 3), dtype=np.int64)
    for a, i in enumerate(rows):
        rs[a] = (np.maximum(0, RX[i, NY[i]] - k).sum(), np.maximum(0, RY[i, NX[i]] - k).sum(),
                 len(np.intersect1d(NX[i], NY[i])))
    sums = rs.sum(axis=0)
    s = len(rows)
    den = s * k * (2 * n - 3 * k - 1)
    return sums, rs, (1 - 2 * int(sums[0]) / den, 1 - 2 * int(sums[1]) / den, int(sums[2]) / (s * k))


def check_quality(q, ref):
    sums, rs, (t, c, r) = ref
    assert q.sums.dtype == np.int64 and q.row_sums.dtype == np.int64
    assert np.array_equal(q.sums, sums) and np.array_equal(q.row_sums, rs)
    assert abs(q.trustworthiness - t) <= 1e-15 and abs(q.continuity - c) <= 1e-15 and abs(q.knn_recall - r) <= 1e-15


@pytest.fixture(scope="module")
def mixture():
    rng = np.random.default_rng(7)
    n = 1500
    X = rng.normal(size=(5, 10))[rng.integers(0, 5, n)] * 3 + rng.normal(size=(n, 10))
    Y3 = np.ascontiguousarray(X[:, :3] + 0.3 * rng.normal(size=(n, 3)))
    return X, Y3, ranks_from_oracle(X, "sqeuclidean")


@pytest.mark.parametrize("c", [2, 3])
def test_scores_against_full_rank_matrices(ctx, mixture, c):
    import torch
    X, Y3, RX = mixture
    n, k = len(X), 12
    Y = np.ascontiguousarray(Y3[:, :c])
    RY = ranks_from_oracle(Y, "sqeuclidean")
    q = ctx.embeddingQuality(X, Y, k)
    check_quality(q, scores_ref(RX, RY, k))
    assert 0.0 < q.trustworthiness < 1.0 and 0.0 < q.continuity < 1.0 and 0.0 < q.knn_recall < 1.0
    strided = T.quality_rows(n, 100)
    check_quality(ctx.embeddingQuality(X, Y, k, rows=100), scores_ref(RX, RY, k, strided))
    shuffled = np.random.default_rng(8).permutation(n)[:211]
    check_quality(ctx.embeddingQuality(X, Y, k, rows=shuffled), scores_ref(RX, RY, k, shuffled))
    # the device form, all rows and a row list
    dX, dY = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    drs = torch.zeros((n, 3), dtype=torch.int64, device="cuda")
    qd = ctx.dev_embedding_quality(dX, dY, k, d_row_sums=drs)
    assert (qd.trustworthiness, qd.continuity, qd.knn_recall) == (q.trustworthiness, q.continuity, q.knn_recall)
    assert np.array_equal(qd.sums, q.sums) and np.array_equal(drs.cpu().numpy(), q.row_sums)
    qs = ctx.dev_embedding_quality(dX, dY, k, d_rows=torch.from_numpy(shuffled).cuda())
    assert np.array_equal(qs.sums, scores_ref(RX, RY, k, shuffled)[0])
    sk = pytest.importorskip("sklearn.manifold")
    assert abs(q.trustworthiness - sk.trustworthiness(X, Y, n_neighbors=k)) <= 1e-12
    assert abs(q.continuity - sk.trustworthiness(Y, X, n_neighbors=k)) <= 1e-12


def test_scores_identity_map_and_cosine(ctx, mixture):
    X, Y3, _ = mixture
    X2 = np.ascontiguousarray(X[:, :2])
    q = ctx.embeddingQuality(X2, X2.copy(), 12)
    assert np.array_equal(q.sums, [0, 0, len(X2) * 12]) and not q.row_sums[:, :2].any()
    assert (q.trustworthiness, q.continuity, q.knn_recall) == (1.0, 1.0, 1.0)
    n, k = 800, 9
    Xc, Yc = np.ascontiguousarray(X[:n]), np.ascontiguousarray(Y3[:n, :2])
    ref = scores_ref(ranks_from_oracle(Xc, "cosine"), ranks_from_oracle(Yc, "sqeuclidean"), k)
    check_quality(ctx.embeddingQuality(Xc, Yc, k, metric="cosine"), ref)


# ------------------------------------------------------------------ 8. after a real fit
def test_after_a_real_fit(ctx):
    rng = np.random.default_rng(0)
    n, d, k = 512, 32, 30
    X = rng.normal(size=(5, d))[rng.integers(0, 5, n)] * 5 + rng.normal(size=(n, d))
    gi, gd = ctx.kNearestNeighbors(X, k)
    rp = np.arange(0, n * k + 1, k, dtype=np.int64)
    p = ctx.pairwiseAffinities(rp, gd.ravel(), 10.0)
    jr, jc, jv = ctx.jointDistribution(rp, gi.ravel(), p, n)
    Y = rng.normal(size=(n, 2)) * 1e-4
    ctx.optimize(jr, jc, jv, Y, np.zeros_like(Y), np.ones_like(Y), default_params(iterations=20, theta=0.5))
    q = ctx.embeddingQuality(X, Y, k)
    for v in (q.trustworthiness, q.continuity, q.knn_recall):
        assert np.isfinite(v) and 0.0 <= v <= 1.0
    check_quality(q, scores_ref(ranks_from_oracle(X, "sqeuclidean"), ranks_from_oracle(Y, "sqeuclidean"), k))


# ------------------------------------------------------------------ 9. errors
def test_argument_errors(ctx):
    rng = np.random.default_rng(9)
    n = 60
    X, Y = rng.normal(size=(n, 4)), rng.normal(size=(n, 2))
    cand = rng.integers(0, n, (n, 3)).astype(np.int32)

    def refused(fn, *words):
        with pytest.raises(T.TsneError) as e:
            fn()
        assert e.value.status == -1, e.value
        assert all(w in str(e.value) for w in words), e.value

    refused(lambda: ctx.embeddingQuality(X, Y, 40), "2 n - 3 k - 1")          # 120 - 120 - 1 <= 0
    refused(lambda: ctx.embeddingQuality(X, Y, 0), "k")
    refused(lambda: ctx.embeddingQuality(X, Y, 5, rows=[3, n, 7]), "rows[1]", str(n))
    refused(lambda: ctx.embeddingQuality(X, Y, 5, rows=[]), "rows")
    refused(lambda: ctx.neighborRanks(X, cand[:3], rows=[3, -2, 7]), "rows[1]", "-2")
    bad = cand.copy()
    bad[2, 1] = n
    refused(lambda: ctx.neighborRanks(X, bad), "cand[7]", str(n))
    refused(lambda: ctx.neighborRanks(X, cand, metric="manhattan"), "not defined")
    refused(lambda: ctx.neighborRanks(X, cand, metric=7), "metric")
    refused(lambda: ctx.embeddingQuality(X, Y, 5, metric=-1), "metric")
    # rows NULL with s != n, through the raw C calls
    L, p = T.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
    out, sc = np.zeros((n, 3), dtype=np.int32), np.zeros(3)
    assert L.tsne_neighbor_ranks(ctx.handle, p(X), n, 4, 0, None, n - 1, p(cand), 3, p(out)) == -1
    assert b"s must equal n" in L.tsne_last_error()
    assert L.tsne_embedding_quality(ctx.handle, p(X), n, 4, 0, p(Y), 2, 5, None, n - 1, p(sc), None, None) == -1
    assert b"s must equal n" in L.tsne_last_error()
    # s == 0 is a no-op for the ranks
    assert L.tsne_neighbor_ranks(ctx.handle, p(X), n, 4, 0, None, 0, p(cand), 3, p(out)) == 0
    # the context still works
    R = ranks_from_dist(seq_dist(X, np.arange(n)), np.arange(n))
    assert np.array_equal(ctx.neighborRanks(X, cand), take(R, cand))
    q = ctx.embeddingQuality(X, Y, 5, rows=np.arange(n))
    assert np.array_equal(q.sums, ctx.embeddingQuality(X, Y, 5).sums)
