"""The tiled attraction's stream layout ("attract_stream" 1, the default:
attract_tiles_stream on the non-loss launches) against attract_tiles over the
jagged layout ("attract_stream" 0) and against the oracle.

Every case runs 10 iterations at theta 0 through Context.optimize on separate
contexts: Y, update, gains and the loss dict of the two settings are equal
bit for bit, and the stream run matches the oracle at the tolerances of
test_tiled_attraction_matches_oracle (1e-9 relative on Y and on the loss).
The shapes are the smallest that reach each edge of the layout: wide slices
and several windows (hub rows), a one-label window, fewer slices than waves
and a partial slice, row lengths around the four-step group, owned rows that
start past label 0 (two loopback ranks), and a padding share of exactly 1."""
import numpy as np
import pytest

import oracle_ctypes as O
import tsne_amd as T
from tsne_amd.api import default_params

pytestmark = pytest.mark.gpu


def gmm(n, d, k=5, seed=0, scale=10.0):
    rng = np.random.default_rng(seed)
    centers = rng.normal(size=(k, d)) * scale
    return centers[rng.integers(0, k, n)] + rng.normal(size=(n, d))


def knn_problem(n, k, seed):
    X = gmm(n, 10, seed=seed)
    oi, od = O.knn(X, k)
    rp = np.arange(0, n * k + 1, k, dtype=np.int64)
    p, _ = O.affinities(rp, od.ravel(), k / 3)
    return O.joint(rp, oi.ravel(), p, n)


def hub_problem(n=12000, seed=71):
    """The problem of test_gpu_parity.hub_problem: a kNN joint P plus three
    dense hub rows / columns (> 4000 entries: wide slices in every window)."""
    import scipy.sparse as sp
    rp, col, val = knn_problem(n, 30, seed)
    A = sp.csr_matrix((val, col, rp), shape=(n, n))
    rng = np.random.default_rng(seed + 1)
    hubs = np.array([3, n // 2 - 500, n - 1])
    B = sp.lil_matrix((n, n))
    for h in hubs:
        B[h, :] = rng.random(n) * 1e-7
    B = B.tocsr()
    B.setdiag(0.0)
    P = (A + B + B.T).tocsr()
    P.eliminate_zeros()
    P.sort_indices()
    P = P / P.sum()
    assert np.diff(P.indptr)[hubs].min() > 4000
    return P.indptr.astype(np.int64), P.indices.astype(np.int32), P.data.astype(np.float64)


def rows_problem(lengths, seed, band=None):
    """A P whose row i has lengths[i] entries: distinct columns != i (within
    `band` labels of i when given), random positive values, sum 1."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    n = len(lengths)
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(lengths)
    row = np.repeat(np.arange(n), lengths)
    j = np.arange(rp[-1]) - rp[row]
    # row i draws from M candidates (the labels but i, or the 2 band + 1 around i but i):
    # an arithmetic sequence modulo M with a stride coprime to M, so distinct
    M = n - 1 if band is None else 2 * band
    assert lengths.max() <= M
    strides = np.array([q for q in range(1, 200) if np.gcd(q, M) == 1])
    c = (rng.integers(0, M, n)[row] + strides[rng.integers(0, len(strides), n)][row] * j) % M
    if band is not None:
        c += np.clip(np.arange(n) - band, 0, n - 2 * band - 1)[row]
    c[c >= row] += 1
    order = np.lexsort((c, row))
    val = rng.random(rp[-1]) + 0.1
    return rp, c[order].astype(np.int32), val / val.sum()


def run(P, Y0, opts, metric="sqeuclidean", theta=0.0, devices=None):
    """-> (Y, upd, gains, losses, padding counter) of 10 iterations on a fresh context."""
    c = T.Context.multi(devices) if devices else T.Context(0)
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        Y, u, g = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
        prm = default_params(iterations=10, theta=theta, metric=metric, learning_rate=200.0)
        loss = c.optimize(*P, Y, u, g, prm)
        assert c.counter("opt.attract_kernel") == 1   # the tiled attraction ran
        pad = c.counter("opt.attract_pad_ppm")
    finally:
        c.close()
    return Y, u, g, loss, pad


def check(P, Y0, opts=None, metric="sqeuclidean", devices=None, ref=None):
    """Stream on / off bit-equal, the stream run against the oracle (ref: its
    (Y, losses) where a caller shares one run); -> padding (ppm)."""
    opts = dict(opts or {})
    Y1, u1, g1, l1, pad = run(P, Y0, {**opts, "attract_stream": 1}, metric, devices=devices)
    Y0_, u0, g0, l0, pad0 = run(P, Y0, {**opts, "attract_stream": 0}, metric, devices=devices)
    assert pad0 == 0 and pad >= 1000000, (pad0, pad)
    assert np.array_equal(Y1, Y0_) and np.array_equal(u1, u0) and np.array_equal(g1, g0)
    assert l1 == l0 and sorted(l1) == [10]
    if ref is None:
        Yo, uo, go = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
        lo = O.optimize(*P, Yo, uo, go, metric=metric, learning_rate=200.0, iterations=10, theta=0.0, threads=8)
        ref = (Yo, lo)
    Yo, lo = ref
    print("max |Y - Yo| / max |Yo| = %.3e, loss rel = %.3e, padding = %.4f"
          % (np.abs(Y1 - Yo).max() / np.abs(Yo).max(), abs(l1[10] - lo[10]) / abs(lo[10]), pad / 1e6))
    assert np.abs(Y1 - Yo).max() <= 1e-9 * np.abs(Yo).max()
    assert abs(l1[10] - lo[10]) <= 1e-9 * abs(lo[10])
    return pad


@pytest.fixture(scope="module")
def hub():
    P = hub_problem()
    Y0 = np.random.default_rng(74).normal(size=(12000, 2)) * 5.0
    Yo, uo, go = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    lo = O.optimize(*P, Yo, uo, go, learning_rate=200.0, iterations=10, theta=0.0, threads=8)
    return P, Y0, Yo, lo


@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
def test_stream_hub_rows_every_config(hub, cfg):
    """Hub rows (wide slices in each of three windows) at every row-block
    configuration; one oracle run shared by the four."""
    P, Y0, Yo, lo = hub
    check(P, Y0, {"attract_cfg": cfg}, ref=(Yo, lo))


@pytest.mark.parametrize("metric", ["sqeuclidean", "euclidean", "cosine"])
def test_stream_one_label_window(metric):
    """n = 5889: a full window and a window of one label (tiles of one column)."""
    n = 5889
    P = knn_problem(n, 12, seed=81)
    Y0 = np.random.default_rng(82).normal(size=(n, 2)) * 5.0
    check(P, Y0, metric=metric)


@pytest.mark.parametrize("n", [70, 63])
def test_stream_fewer_slices_than_waves(n):
    """k = 5 over 70 / 63 points: one slice and a partial one / one partial
    slice, every other wave without a slice."""
    P = knn_problem(n, 5, seed=83 + n)
    Y0 = np.random.default_rng(84).normal(size=(n, 2)) * 5.0
    check(P, Y0)


def test_stream_widths_around_the_group():
    """Rows of 1, 2, 3, 4, 5, 7, 8 and 9 entries mixed in each of four 64-row
    slices (widths that are no multiple of the four-step group; lanes past
    their rows in every step but the first) and a slice whose 64 rows have one
    entry each, in the original label order."""
    lengths = [[1, 2, 3, 4, 5, 7, 8, 9][i % 8] for i in range(256)] + [1] * 64
    P = rows_problem(lengths, seed=85)
    Y0 = np.random.default_rng(86).normal(size=(len(lengths), 2)) * 5.0
    pad = check(P, Y0, {"graph_order": 0})
    # four slices of width 9 holding 8 rows of each length, one of width 1
    assert pad == (4 * 9 + 1) * 64 * 1000000 // sum(lengths)


def test_stream_padding_exactly_one():
    """Equal row lengths in every slice (64 consecutive rows of each of 9, 8,
    7, 5, 4, 3, 2, 1 entries, original label order): no padded slot."""
    lengths = [L for L in (9, 8, 7, 5, 4, 3, 2, 1) for _ in range(64)]
    P = rows_problem(lengths, seed=87)
    Y0 = np.random.default_rng(88).normal(size=(len(lengths), 2)) * 5.0
    assert check(P, Y0, {"graph_order": 0}) == 1000000


def test_stream_two_loopback_ranks():
    """Two ranks on one device: the second owns labels [3001, 6001), 3000 rows
    (no multiple of 64), over two windows."""
    n = 6001
    P = knn_problem(n, 12, seed=89)
    Y0 = np.random.default_rng(90).normal(size=(n, 2)) * 5.0
    check(P, Y0, devices=[0, 0])


def test_stream_many_slices_per_tile():
    """More slices in a tile than waves (1216-row blocks at 300000 banded rows
    of 1 .. 40 entries, hub rows among them): the deal by width gives a wave
    several slices of one tile.  Stream on / off bit-equal at theta 0.5 (no
    oracle at this size)."""
    n = 300000
    rng = np.random.default_rng(91)
    lengths = rng.integers(1, 41, size=n)
    lengths[rng.integers(0, n, 200)] = 700
    P = rows_problem(lengths, seed=92, band=400)
    Y0 = np.random.default_rng(93).normal(size=(n, 2)) * 5.0
    a = run(P, Y0, {"attract_cfg": 3, "attract_stream": 1}, theta=0.5)
    b = run(P, Y0, {"attract_cfg": 3, "attract_stream": 0}, theta=0.5)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    assert a[4] > 1000000 and b[4] == 0
    c = run(P, Y0, {"attract_cfg": 3}, theta=0.5)   # a second run of the new path: the same bits
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], c[:3])) and a[3] == c[3]
