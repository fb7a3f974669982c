"""The front half of the pipeline (kNN filter, affinities, joint) on inputs
chosen against the kernels: libtsne_hip through the C ABI against the CPU
oracle.  kNN indices and distances are compared bit for bit, affinities at
abs 1e-12, the joint's pattern exactly and its values at abs 1e-15.

Every kNN case runs on two contexts, the bf16x3 threshold filter (option
"knn_bf16" 1, the default) and the f32-input one (0): both are exact only as
long as their error bound (knn_run's delta_coef) holds, and the inputs below
bring the k-th neighbour gaps down to the size of that bound.  The counter
"knn.fallback_queries" tells the filter + re-rank path from the exact scan."""
import numpy as np
import pytest

import oracle_ctypes as O
import tsne_amd as T
from tsne_amd._lib import TsneError, lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_f32():
    c = T.Context(0)
    c.set_option("knn_bf16", 0)
    yield c
    c.close()


def gmm(n, d, k=5, seed=0, scale=10.0):
    """The suite's blobs (test_gpu_parity.gmm)."""
    rng = np.random.default_rng(seed)
    centers = rng.normal(size=(k, d)) * scale
    return centers[rng.integers(0, k, n)] + rng.normal(size=(n, d))


def same(a, b):
    """Bit-for-bit equality of (idx, dist) pairs, NaN distances at the same places."""
    return (np.array_equal(a[0], b[0]) and np.array_equal(np.isnan(a[1]), np.isnan(b[1]))
            and np.array_equal(a[1][~np.isnan(a[1])], b[1][~np.isnan(b[1])]))


def knn_both(ctx, ctx_f32, X, k, metric="sqeuclidean", want=None, **kw):
    """kNN on both filters against the oracle (or `want`) and each other ->
    the two contexts' "knn.fallback_queries"."""
    if want is None:
        want = O.knn(X, k, metric, threads=8, **kw)
    a = ctx.kNearestNeighbors(X, k, metric, **kw)
    fa = ctx.counter("knn.fallback_queries")
    b = ctx_f32.kNearestNeighbors(X, k, metric, **kw)
    fb = ctx_f32.counter("knn.fallback_queries")
    print("knn.fallback_queries n=%d d=%d k=%d %s: bf16x3 %d, f32 %d" % (X.shape[0], X.shape[1], k, metric, fa, fb))
    assert same(a, want), "bf16x3 filter differs from the oracle"
    assert same(b, want), "f32 filter differs from the oracle"
    assert same(a, b)
    return fa, fb


# ------------------------------------------------------------------ 1. kNN
def two_clusters(n, d, R, seed):
    """Exactly n / 2 rows at each of +-R on the first axis, unit normal noise:
    the centred norms grow as R^2 (and with them the filter's error bound)
    while the neighbour gaps stay those of the unit noise."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    X[:, 0] += np.where(rng.permutation(n) < n // 2, R, -R)
    return X


@pytest.mark.parametrize("metric", ["sqeuclidean", "euclidean"])
@pytest.mark.parametrize("R", [30, 100, 300, 3000])
@pytest.mark.parametrize("d,k", [(3, 10), (16, 30), (33, 30)])
def test_knn_conditioning_sweep(ctx, ctx_f32, d, k, R, metric):
    """a. The filter's error bound against neighbour gaps of its own size.  At
    R = 30 no candidate band comes near the buffers' capacity, so every query
    must be answered by the filter + re-rank; beyond, either path may answer."""
    X = two_clusters(1500, d, float(R), seed=1000 * d + R)
    fa, fb = knn_both(ctx, ctx_f32, X, k, metric)
    if R == 30:
        assert fa == 0 and fb == 0


@pytest.mark.parametrize("sigma", [0.3, 0.03, 0.003])
@pytest.mark.parametrize("d,k", [(3, 10), (16, 30), (33, 30)])
def test_knn_conditioning_cosine(ctx, ctx_f32, d, k, sigma):
    """a (cosine). Rows L_i (u + sigma noise), lengths log-uniform over six
    decades: all the angles lie within ~sigma of one direction."""
    rng = np.random.default_rng(int(1e4 * sigma) + d)
    u = rng.normal(size=d)
    u /= np.linalg.norm(u)
    L = 10.0 ** rng.uniform(-3, 3, size=(1500, 1))
    X = L * (u + sigma * rng.normal(size=(1500, d)))
    knn_both(ctx, ctx_f32, X, k, "cosine")


def test_knn_below_fp32_resolution(ctx, ctx_f32):
    """b. 60 groups of 20 rows that differ by 1e-9 within a group: with k = 30
    the k-th boundary lies inside the second-nearest group, whose members are
    one value in fp32.  The order exists only in fp64."""
    rng = np.random.default_rng(21)
    X = np.repeat(gmm(60, 12, seed=21), 20, axis=0) + 1e-9 * rng.normal(size=(1200, 12))
    knn_both(ctx, ctx_f32, X, 30)


def crowd():
    """n = 1400, d = 6: 700 exact copies of one row, spread over the index range."""
    X = gmm(1400, 6, seed=33)
    where = np.random.default_rng(34).permutation(1400)[:700]
    X[where] = X[where[0]]
    return X, where


def test_knn_fallback_crowd(ctx, ctx_f32):
    """c. 700 exact copies of one row: each copy has 699 candidates at its k-th
    distance (0), more than half the candidate buffer, whatever the bound --
    those queries must take the exact scan (self excluded by key, ties by j)."""
    X, _ = crowd()
    fa, fb = knn_both(ctx, ctx_f32, X, 25)
    assert fa >= 700 and fb >= 700


def test_knn_crowd_large_buffers(ctx, ctx_f32):
    """c. The same crowd at k = 250: knn_run<4096>, whose buffers hold it."""
    X, _ = crowd()
    knn_both(ctx, ctx_f32, X, 250)


def test_knn_fallback_crowd_cosine_zero_rows(ctx, ctx_f32):
    """c. The crowd plus two zero rows under cosine: NaN distances order last,
    on the scan path as on the re-rank path."""
    X, where = crowd()
    rest = np.setdiff1d(np.arange(1400), where)
    X[rest[5]] = 0.0
    X[rest[400]] = 0.0
    fa, fb = knn_both(ctx, ctx_f32, X, 25, "cosine")
    assert fa >= 700 and fb >= 700


@pytest.mark.parametrize("k", [192, 193, 500, 896])
def test_knn_capacity_classes(ctx, ctx_f32, k):
    """d. kk <= 192 runs knn_run<1024>, 193..896 knn_run<4096> (64 register
    rounds in its compaction)."""
    knn_both(ctx, ctx_f32, gmm(1500, 10, seed=44), k)


def test_knn_k_beyond_capacity_is_unsupported(ctx):
    with pytest.raises(TsneError) as e:
        ctx.kNearestNeighbors(gmm(1500, 10, seed=44), 897)
    assert e.value.status == -4


@pytest.mark.parametrize("k", [300, 897])
def test_knn_cross_capacity_classes(ctx, ctx_f32, k):
    """d. The cross form: k = 300 through knn_run<4096>, k = 897 by the exact
    scan of every query."""
    n, m = 1500, 130
    X, Xq = gmm(n, 10, seed=44), gmm(m, 10, seed=45)
    a = ctx.kNearestNeighborsCross(X, Xq, k)
    fa = ctx.counter("knn.fallback_queries")
    b = ctx_f32.kNearestNeighborsCross(X, Xq, k)
    assert a[0].shape == (m, k)
    for q in range(m):
        oi, od = O.knn(np.vstack([X, Xq[q:q + 1]]), k, q0=n, q1=n + 1)
        assert np.array_equal(a[0][q], oi[0]) and np.array_equal(a[1][q], od[0]), q
    assert same(a, b)
    if k == 897:
        assert fa == m


class Lattice:
    """e. The 32 x 32 x 33 integer lattice, its rows stored in a seeded random
    permutation, and every row's 10 nearest rows worked out from the lattice:
    the offsets within +-3 that stay inside, by (squared distance, row id).
    (A corner has 10 rows within squared distance 4; outside +-3 it is >= 16.)"""

    def __init__(self):
        nx, ny, nz, k = 32, 32, 33, 10
        n = nx * ny * nz
        g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(n, 3)
        perm = np.random.default_rng(55).permutation(n)
        C = g[perm]                                   # row r is the lattice point C[r]
        row_of = np.empty(n, dtype=np.int64)
        row_of[perm] = np.arange(n)                   # lattice index -> row
        r = np.arange(-3, 4)
        off = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
        off = off[(off != 0).any(axis=1)]
        d2 = (off * off).sum(axis=1)
        idx = np.empty((n, k), dtype=np.int32)
        dist = np.empty((n, k))
        big = np.int64(1) << 40
        for a in range(0, n, 4096):                   # chunks: n x 342 keys at once is needless memory
            P = C[a:a + 4096, None, :] + off[None, :, :]
            ok = ((P >= 0) & (P < [nx, ny, nz])).all(axis=2)
            lin = (np.clip(P[..., 0], 0, nx - 1) * ny + np.clip(P[..., 1], 0, ny - 1)) * nz + np.clip(P[..., 2], 0, nz - 1)
            key = np.where(ok, d2[None, :] * n + row_of[lin], big)
            key = np.sort(key, axis=1)[:, :k]
            assert (key < big).all()
            idx[a:a + 4096] = key % n
            dist[a:a + 4096] = key // n
        self.X = C.astype(np.float64)
        self.n, self.k, self.want = n, k, (idx, dist)


@pytest.fixture(scope="module")
def lattice():
    return Lattice()


def test_knn_lattice_expectation_is_the_oracle(lattice):
    """e. The analytic neighbours are the oracle's, on the first, middle and last rows."""
    n, k = lattice.n, lattice.k
    for q0, q1 in ((0, 300), (16200, 16600), (n - 300, n)):
        got = O.knn(lattice.X, k, q0=q0, q1=q1, threads=8)
        assert same(got, (lattice.want[0][q0:q1], lattice.want[1][q0:q1]))


def test_knn_lattice_whole_raster(ctx, ctx_f32, lattice):
    """e. n = 33,792: 17 candidate groups of 2048, 132 query tiles (three
    super-tile columns, the last one padded): with the rows permuted, a skipped
    or doubled (query tile, candidate group) block changes some row.  The
    candidate bands are a few dozen entries: no query may take the scan."""
    fa, fb = knn_both(ctx, ctx_f32, lattice.X, lattice.k, want=lattice.want)
    assert fa == 0 and fb == 0


def test_knn_lattice_query_range(ctx, ctx_f32, lattice):
    q0, q1 = 16300, 33001
    want = (lattice.want[0][q0:q1], lattice.want[1][q0:q1])
    fa, fb = knn_both(ctx, ctx_f32, lattice.X, lattice.k, want=want, q0=q0, q1=q1)
    assert fa == 0 and fb == 0


@pytest.fixture(scope="module")
def scale_base():
    X = gmm(300, 8, seed=66)
    return X, O.knn(X, 15)


@pytest.mark.parametrize("s", [-100, -40, 40, 100])
def test_knn_power_of_two_scale(ctx, ctx_f32, scale_base, s):
    """f. Scaling by 2^s is exact in fp64: the same neighbours, the distances
    times 2^(2s).  At |s| = 100 the fp32 squares of the filter underflow to 0 /
    overflow to inf; the answer must still be exact (by whichever path)."""
    X, (i0, d0) = scale_base
    Xs = X * 2.0 ** s
    want = O.knn(Xs, 15)
    assert np.array_equal(want[0], i0) and np.array_equal(want[1], d0 * 2.0 ** (2 * s))
    knn_both(ctx, ctx_f32, Xs, 15, want=(i0, d0 * 2.0 ** (2 * s)))


@pytest.mark.parametrize("metric", ["sqeuclidean", "euclidean"])
@pytest.mark.parametrize("d", [1, 32, 96])
def test_knn_dimension_edges(ctx, ctx_f32, d, metric):
    """g. One column, exactly one 32-column stage, exactly three."""
    knn_both(ctx, ctx_f32, two_clusters(700, d, 30.0, seed=77 + d), 20, metric)


def test_knn_fallback_counter_device_and_reset(ctx):
    """0. The counter is that of the handle's last kNN call, device form included."""
    import torch
    X, _ = crowd()
    dev = torch.device("cuda", 0)
    dX = torch.from_numpy(X).to(dev)
    di = torch.zeros((1400, 25), dtype=torch.int32, device=dev)
    dd = torch.zeros((1400, 25), dtype=torch.float64, device=dev)
    ctx.dev_knn(dX, 25, "sqeuclidean", 0, 1400, di, dd)
    ctx.synchronize()
    assert ctx.counter("knn.fallback_queries") >= 700
    assert same((di.cpu().numpy(), dd.cpu().numpy()), O.knn(X, 25))
    ctx.kNearestNeighbors(gmm(300, 4, seed=1), 5)
    assert ctx.counter("knn.fallback_queries") == 0


def test_knn_fallback_counter_sums_over_ranks(ctx):
    """0. A group handle splits the queries over its ranks: the counter is their
    sum (a query's path does not depend on which other queries run with it)."""
    X, _ = crowd()
    want = O.knn(X, 25)
    assert same(ctx.kNearestNeighbors(X, 25), want)
    single = ctx.counter("knn.fallback_queries")
    g = T.Context.multi([0, 0])
    try:
        assert same(g.kNearestNeighbors(X, 25), want)
        assert g.counter("knn.fallback_queries") == single >= 700
        g.kNearestNeighbors(X, 25, q0=10, q1=11)      # one query: the second rank gets none
        assert g.counter("knn.fallback_queries") <= 1
    finally:
        g.close()


# ----------------------------------------------------------- 2. affinities
# One call per kernel variant: the longest row picks beta_search<2> (<= 128),
# beta_search_block<4, 1024, 0> (<= 4096), <16, 1024, 0> (<= 16384) or
# <58, 512, 20000>, whose registers hold 29,696 entries and registers + LDS
# 49,696 (the rest is re-read).
AFF_LENS = {
    "wave": [0, 1, 2, 63, 64, 65, 127, 128],
    "block4": [1, 129, 1023, 1024, 1025, 4095, 4096],
    "block16": [0, 200, 4097, 16383, 16384],
    "block58": [16385, 29695, 29696, 29697, 49695, 49696, 49697, 60000, 1, 0, 130],
}
# "zeros": every distance 0; "half": every other entry of a row 0.  (Nonzero
# constant rows longer than the perplexity are left out on purpose: their
# search ends by budget where exp underflows, the oracle's own p sums to 0
# there, and libm's last bits decide the answer.)
AFF_VARIANTS = {"1": 1.0, "1e-12": 1e-12, "1e6": 1e6, "1e12": 1e12, "zeros": None, "half": None}


def aff_input(call, variant):
    lens = np.array(AFF_LENS[call], dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    d = np.random.default_rng(len(call) + int(rp[-1])).uniform(0, 50, size=int(rp[-1]))
    if variant == "zeros":
        d[:] = 0.0
    elif variant == "half":
        for a, b in zip(rp[:-1], rp[1:]):
            d[a:b:2] = 0.0
    else:
        d *= AFF_VARIANTS[variant]
    return rp, d


AFF_CASES = [(c, "1") for c in AFF_LENS] + [(c, v) for c in ("wave", "block58") for v in AFF_VARIANTS if v != "1"]


@pytest.mark.parametrize("perplexity", [2.0, 30.0, 1000.0])
@pytest.mark.parametrize("call,variant", AFF_CASES)
def test_affinities_row_length_boundaries(ctx, call, variant, perplexity):
    """Row lengths on both sides of every kernel and storage boundary, rows of
    length 0 and 1, perplexities beyond the row length (the 50-step budget runs
    out), zero distances, and scales from 1e-12 to 1e12."""
    rp, d = aff_input(call, variant)
    po, _ = O.affinities(rp, d, perplexity)
    # the input is well-posed: one ulp on every distance moves the oracle's own p by <= 1e-13
    pn, _ = O.affinities(rp, np.nextafter(d, np.inf), perplexity)
    assert not np.isnan(po).any() and np.abs(pn - po).max() <= 1e-13
    p = ctx.pairwiseAffinities(rp, d, perplexity)
    assert not np.isnan(p).any()
    err = np.abs(p - po).max()
    print("affinities %s/%s perplexity %g: max abs error %.3g" % (call, variant, perplexity, err))
    assert err <= 1e-12


def test_affinities_device_form_equals_host_form(ctx):
    import torch
    rp, d = aff_input("block58", "1")
    p = ctx.pairwiseAffinities(rp, d, 30.0)
    dev = torch.device("cuda", 0)
    drp, dd = torch.from_numpy(rp).to(dev), torch.from_numpy(d).to(dev)
    dp = torch.zeros_like(dd)
    ctx.dev_affinities(drp, dd, len(rp) - 1, 30.0, dp)
    ctx.synchronize()
    assert np.array_equal(dp.cpu().numpy(), p)


# ---------------------------------------------------------------- 3. joint
def rows_to_csr(rows, rng):
    """rows: one list of columns per row -> (row_ptr, col, p), p uniform in (0, 1]."""
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.array([c for r in rows for c in r], dtype=np.int32)
    return rp, col, 1.0 - rng.uniform(size=len(col))


def check_joint(ctx, rp, col, p, n):
    a = ctx.jointDistribution(rp, col, p, n)
    b = O.joint(rp, col, p, n)
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1])
    assert np.abs(a[2] - b[2]).max() <= 1e-15
    assert abs(a[2].sum() - 1.0) <= 1e-12
    return a


def ragged_case():
    """n = 257, unsorted rows of 0..40 distinct columns.  Rows 0 and 77 are
    empty and named by nobody (empty output rows), rows 5, 200 and 256 are
    empty but named (rows of reverse entries only); some rows name themselves."""
    n = 257
    rng = np.random.default_rng(88)
    pool = np.setdiff1d(np.arange(n), [0, 77])
    rows = []
    for i in range(n):
        ln = 0 if i in (0, 77, 5, 200, 256) else int(rng.integers(0, 41))
        rows.append([int(c) for c in rng.choice(pool, size=ln, replace=False)])
    for i, c in ((10, 5), (11, 5), (12, 200), (255, 256), (1, 256)):
        if c not in rows[i]:
            rows[i].append(c)
    for i in (3, 64, 128, 254):
        if i not in rows[i]:
            rows[i].insert(len(rows[i]) // 2, i)
    assert sum(len(r) == 0 for r in rows) >= 5
    return (n,) + rows_to_csr(rows, rng)


def test_joint_ragged(ctx):
    n, rp, col, p = ragged_case()
    orp, _, _ = check_joint(ctx, rp, col, p, n)
    ln = np.diff(orp)
    assert ln[0] == 0 and ln[77] == 0 and ln[5] >= 2 and ln[200] >= 1 and ln[256] >= 2


def symmetric_rows(n, seed):
    rng = np.random.default_rng(seed)
    A = rng.uniform(size=(n, n)) < 0.08
    A = A | A.T
    A[np.arange(0, n, 7), np.arange(0, n, 7)] = True   # some self entries
    A[50] = False                                        # one empty row / column
    A[:, 50] = False
    return [list(np.flatnonzero(A[i])) for i in range(n)], rng


def test_joint_sorted_fully_mutual(ctx):
    """Sorted input, every entry mutual: no sort and the direct write into the output."""
    rows, rng = symmetric_rows(100, 90)
    check_joint(ctx, *rows_to_csr(rows, rng), 100)


def test_joint_sorted_not_mutual(ctx):
    """The same pattern with one direction of one pair removed: sorted input, one reverse entry."""
    rows, rng = symmetric_rows(100, 90)
    i = next(i for i in range(100) if any(c != i for c in rows[i]))
    j = next(c for c in rows[i] if c != i)
    rows[i].remove(j)
    rp, col, p = rows_to_csr(rows, rng)
    a = check_joint(ctx, rp, col, p, 100)
    assert len(a[1]) == len(col) + 1


def test_joint_hub_row_and_hub_column(ctx):
    """One row that holds every other column, one column named by every row."""
    n = 5000
    rng = np.random.default_rng(91)
    rows = [[7] + [int(c) for c in rng.choice(np.setdiff1d(np.arange(n), [7, i]), size=3, replace=False)]
            for i in range(n)]
    rows[0] = [int(c) for c in rng.permutation(np.arange(1, n))]
    check_joint(ctx, *rows_to_csr(rows, rng), n)


@pytest.mark.parametrize("sorted_input", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
def test_joint_repeated_columns(ctx, reverse, sorted_input):
    """A row that repeats a column: the reference sums the copies
    (groupBy(0, 1).reduce, TsneHelpers.scala:188), one output entry per (i, j)."""
    n = 50
    rng = np.random.default_rng(92)
    pool = np.setdiff1d(np.arange(n), [3, 4, 9, 11, 20])
    rows = [[int(c) for c in rng.choice(pool, size=int(rng.integers(0, 9)), replace=False)] for _ in range(n)]
    rows[3] += [9, 9]                 # twice
    rows[4] += [11, 11, 11]           # three times
    rows[20] = [20, 5, 20, 4, 4]      # a repeated self entry; 4 twice, and 4 does not name 20
    if reverse:
        rows[9].append(3)
        rows[11] += [4, 4]            # both directions repeat
    if sorted_input:
        rows = [sorted(r) for r in rows]
    rp, col, p = rows_to_csr(rows, rng)
    a = check_joint(ctx, rp, col, p, n)
    for i in range(n):                # no output row names a column twice
        assert len(set(a[1][a[0][i]:a[0][i + 1]])) == a[0][i + 1] - a[0][i]


def test_joint_device_form_equals_host_form(ctx):
    import torch
    n, rp, col, p = ragged_case()
    a = ctx.jointDistribution(rp, col, p, n)
    dev = torch.device("cuda", 0)
    cap = 2 * len(col) + 1
    orp = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    oc = torch.zeros(cap, dtype=torch.int32, device=dev)
    ov = torch.zeros(cap, dtype=torch.float64, device=dev)
    nnz = ctx.dev_joint(torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev), torch.from_numpy(p).to(dev),
                        n, cap, orp, oc, ov)
    ctx.synchronize()
    assert nnz == len(a[1])
    assert np.array_equal(orp.cpu().numpy(), a[0])
    assert np.array_equal(oc.cpu().numpy()[:nnz], a[1]) and np.array_equal(ov.cpu().numpy()[:nnz], a[2])


def test_joint_capacity(ctx):
    """cap one short: TSNE_ERR_CAPACITY with the required size reported; cap = nnz succeeds."""
    import ctypes as C
    n, rp, col, p = ragged_case()
    want = O.joint(rp, col, p, n)
    nnz = len(want[1])

    def call(cap):
        orp = np.zeros(n + 1, dtype=np.int64)
        oc = np.zeros(max(cap, 1), dtype=np.int32)
        ov = np.zeros(max(cap, 1))
        out = C.c_int64(-7)
        rc = lib().tsne_joint_distribution(ctx.handle, rp.ctypes.data, col.ctypes.data, p.ctypes.data, n, cap,
                                           orp.ctypes.data, oc.ctypes.data, ov.ctypes.data, C.byref(out))
        return rc, out.value, orp, oc, ov

    rc, need, _, _, _ = call(nnz - 1)
    assert rc == -5 and need == nnz
    rc, need, orp, oc, ov = call(nnz)
    assert rc == 0 and need == nnz
    assert np.array_equal(orp, want[0]) and np.array_equal(oc, want[1]) and np.abs(ov - want[2]).max() <= 1e-15
