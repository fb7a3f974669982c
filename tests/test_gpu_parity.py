"""GPU parity: libtsne_hip (through the C ABI) against the CPU oracle and the
reference goldens.  Tolerances: kNN indices bit-exact (ties ordered by
(d, j)), kNN distances bit-exact fp64; goldens at the reference suite's own
tolerances; BH gradients at 1e-4 relative to max|grad| (north_star)."""
import numpy as np
import pytest

import oracle_ctypes as O
import tsne_amd as T
from golden_data import csr_to_dict, dense_input, goldens, triples_to_csr
from tsne_amd.api import default_params

pytestmark = pytest.mark.gpu
G = goldens()


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(0)
    yield c
    c.close()


def knn_csr(idx, dist):
    n, k = idx.shape
    return np.arange(0, n * k + 1, k, dtype=np.int64), idx.ravel(), dist.ravel()


# ------------------------------------------------------------------ kNN
def test_knn_golden(ctx):
    X = np.array([v for _, v in G["knnInput"]])
    idx, dist = ctx.kNearestNeighbors(X, 2)
    got = {(i, int(idx[i, t]), float(dist[i, t])) for i in range(9) for t in range(2)}
    assert got == {tuple(t) for t in G["knnResults"]}


def gmm(n, d, k=5, seed=0, scale=10.0):
    rng = np.random.default_rng(seed)
    centers = rng.normal(size=(k, d)) * scale
    return centers[rng.integers(0, k, n)] + rng.normal(size=(n, d))


@pytest.mark.parametrize("n,d,k,metric", [
    (300, 4, 5, "sqeuclidean"), (1000, 50, 90, "sqeuclidean"), (777, 33, 30, "euclidean"),
    (640, 784, 90, "sqeuclidean"), (500, 20, 10, "cosine"), (2000, 50, 90, "sqeuclidean"),
    (100, 3, 99, "sqeuclidean"), (129, 7, 200, "sqeuclidean")])
def test_knn_matches_oracle(ctx, n, d, k, metric):
    X = gmm(n, d, seed=n + d)
    gi, gd = ctx.kNearestNeighbors(X, k, metric)
    oi, od = O.knn(X, k, metric)
    assert np.array_equal(gi, oi)
    assert np.array_equal(gd, od)


def test_knn_ties_and_duplicates(ctx):
    # integer grid with many exact distance ties, plus 40 copies of one point
    rng = np.random.default_rng(3)
    X = rng.integers(0, 4, size=(600, 6)).astype(np.float64)
    X[100:140] = X[5]
    gi, gd = ctx.kNearestNeighbors(X, 25)
    oi, od = O.knn(X, 25)
    assert np.array_equal(gi, oi) and np.array_equal(gd, od)


def test_knn_query_range(ctx):
    X = gmm(900, 16, seed=9)
    gi, gd = ctx.kNearestNeighbors(X, 12, q0=333, q1=701)
    oi, od = O.knn(X, 12, q0=333, q1=701)
    assert np.array_equal(gi, oi) and np.array_equal(gd, od)


def test_knn_large_norm_offset(ctx):
    # far from the origin: exercises the centring + error bound of the fp32 filter
    X = gmm(1500, 64, seed=5) + 1e4
    gi, gd = ctx.kNearestNeighbors(X, 40)
    oi, od = O.knn(X, 40)
    assert np.array_equal(gi, oi) and np.array_equal(gd, od)


def test_knn_cosine_zero_rows(ctx):
    X = gmm(400, 12, seed=2)
    X[7] = 0.0
    X[200] = 0.0
    gi, gd = ctx.kNearestNeighbors(X, 15, "cosine")
    oi, od = O.knn(X, 15, "cosine")
    assert np.array_equal(gi, oi)
    assert np.array_equal(np.isnan(gd), np.isnan(od))
    assert np.array_equal(gd[~np.isnan(gd)], od[~np.isnan(od)])


# ----------------------------------------------------------- affinities
def test_pairwise_affinities_golden(ctx):
    ids, X = dense_input()
    idx, dist = ctx.kNearestNeighbors(X, 10)
    rp, col, d = knn_csr(idx, dist)
    p = ctx.pairwiseAffinities(rp, d, 2.0)
    want = {(a, b): c for a, b, c in G["densePairwiseAffinitiesResults"]}
    got = {(i, int(col[e])): p[e] for i in range(10) for e in range(rp[i], rp[i + 1])}
    assert set(got) == set(want)
    assert max(abs(got[k] - v) for k, v in want.items()) <= 1e-12


def test_affinities_match_oracle(ctx):
    X = gmm(3000, 30, seed=1)
    oi, od = O.knn(X, 90)
    rp, col, d = knn_csr(oi, od)
    p = ctx.pairwiseAffinities(rp, d, 30.0)
    po, _ = O.affinities(rp, d, 30.0)
    assert np.abs(p - po).max() <= 1e-12


def test_affinities_long_rows(ctx):
    # distance-matrix mode: one row holds every other point (> 128 entries)
    rng = np.random.default_rng(4)
    lens = rng.integers(1, 700, size=40)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    d = rng.uniform(0, 50, size=rp[-1])
    p = ctx.pairwiseAffinities(rp, d, 20.0)
    po, _ = O.affinities(rp, d, 20.0)
    assert np.abs(p - po).max() <= 1e-12


# ---------------------------------------------------------------- joint
@pytest.mark.parametrize("name,n,tol", [("dense", 10, 1e-12), ("sparse", 12, 1e-6)])
def test_joint_goldens(ctx, name, n, tol):
    src = G["densePairwiseAffinitiesResults" if name == "dense" else "sparsePairwiseAffinitiesResults"]
    want = G["denseJointProbabilitiesResults" if name == "dense" else "sparseJointProbabilitiesResults"]
    rp, col, val = triples_to_csr(src, n)
    orp, oc, ov = ctx.jointDistribution(rp, col, val, n)
    got = csr_to_dict(orp, oc, ov)
    w = {(a, b): c for a, b, c in want}
    assert set(got) == set(w)
    assert max(abs(got[k] - v) for k, v in w.items()) <= tol
    assert abs(ov.sum() - 1.0) <= 1e-12


def test_joint_matches_oracle(ctx):
    X = gmm(2500, 20, seed=8)
    oi, od = O.knn(X, 30)
    rp, col, d = knn_csr(oi, od)
    p, _ = O.affinities(rp, d, 10.0)
    a = ctx.jointDistribution(rp, col, p, 2500)
    b = O.joint(rp, col, p, 2500)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.abs(a[2] - b[2]).max() <= 1e-15


# ------------------------------------------------------------- gradient
def _emb():
    return np.array([v for _, v in sorted(G["initialEmbedding"])])


def test_gradient_golden(ctx):
    rp, col, val = triples_to_csr(G["denseJointProbabilitiesResults"], 10)
    grad, Z, _ = ctx.gradient(rp, col, val, _emb(), theta=0.0)
    want = np.array([v for _, v in sorted(G["denseGradientResults"])])
    assert np.abs(grad - want).max() <= 1e-12
    assert abs(Z - G["denseSumQ"]) <= 1e-9


def near_tol(c, late=False):
    """The library's own near-exact bound (per summarised cell, relative), read
    from the context: single gradients and the optimizer's early-exaggeration
    phase run at "near_tol_early" (1e-6), the optimizer after it at
    "near_tol_late" (5e-6)."""
    return c.get_option("near_tol_late" if late else "near_tol_early")


def random_problem(n, k, seed):
    X = gmm(n, 10, seed=seed)
    oi, od = O.knn(X, k)
    rp, col, d = knn_csr(oi, od)
    p, _ = O.affinities(rp, d, k / 3)
    return O.joint(rp, col, p, n)


@pytest.mark.parametrize("scale,theta,metric", [
    (1e-4, 0.5, "sqeuclidean"), (1.0, 0.25, "sqeuclidean"), (30.0, 0.5, "sqeuclidean"),
    (5.0, 0.5, "euclidean"), (5.0, 0.25, "cosine"), (20.0, 0.0, "sqeuclidean")])
def test_gradient_matches_oracle(ctx, scale, theta, metric):
    n = 1500
    rp, col, val = random_problem(n, 30, seed=int(scale * 10) + 1)
    Y = np.random.default_rng(1).normal(size=(n, 2)) * scale
    g, Z, loss = ctx.gradient(rp, col, val, Y, theta, metric, exaggeration=4.0, want_loss=True)
    r = O.gradient(rp, col, val, Y, theta, metric, exaggeration=4.0, want_loss=True)
    scale_g = np.abs(r["grad"]).max()
    assert np.abs(g - r["grad"]).max() <= 1e-4 * scale_g
    assert abs(Z - r["Z"]) <= near_tol(ctx) * r["Z"]
    assert abs(loss - r["loss"]) <= 1e-6 * abs(r["loss"])


@pytest.mark.parametrize("n,scale", [(20000, 1e-4), (20000, 1e-3), (20000, 0.03), (12000, 0.3)])
def test_gradient_large_near_exact(ctx, n, scale):
    """Near-exact regime of a small embedding at a size where the all-open
    subtrees carry moments (moment path) and, at the larger scales, partly
    fail the truncation bound (dense leaf tiles)."""
    rp, col, val = random_problem(n, 10, seed=int(scale * 1000) + 3)
    Y = np.random.default_rng(3).normal(size=(n, 2)) * scale
    g, Z, loss = ctx.gradient(rp, col, val, Y, 0.5, exaggeration=12.0, want_loss=True)
    r = O.gradient(rp, col, val, Y, 0.5, exaggeration=12.0, want_loss=True)
    assert np.abs(g - r["grad"]).max() <= 1e-4 * np.abs(r["grad"]).max()
    # near-exact subtrees: each summarised cell within near_tol of its exact leaf sum
    assert np.abs(g - r["grad"]).max() <= 10 * near_tol(ctx) * np.abs(r["grad"]).max()
    assert abs(Z - r["Z"]) <= near_tol(ctx) * r["Z"]
    if np.isnan(r["loss"]):   # some P_ij underflowed to 0: 0 * ln 0 (TsneHelpers.scala:300)
        assert np.isnan(loss)
    else:
        assert abs(loss - r["loss"]) <= 1e-6 * abs(r["loss"])


@pytest.mark.parametrize("n,scale,dups", [(20000, 1e-4, False), (5000, 1e-3, False), (5000, 1e-4, True)])
def test_root_tile_mode_per_point(ctx, n, scale, dups):
    """Root-tile mode (bhtree_build.hip: a small embedding's whole tree is one
    near-exact subtree for every query -> the root's moments as polynomials,
    no sort / tree): per-point F and z against the oracle's quadtree.  With
    exact duplicates the hash-round check sends the build to the full path
    (the reference's multiplicities)."""
    rng = np.random.default_rng(n + int(1e5 * scale))
    Y = rng.normal(size=(n, 2)) * scale
    if dups:
        Y[[7, 4000, 123]] = Y[7]
        Y[[99, 98]] = Y[99]
    F, z = ctx.repulsion(Y, 0.5)
    rep, zi = O.repulsion(Y, 0.5, threads=8)
    assert np.abs(z - zi).max() <= near_tol(ctx) * zi.max()
    assert np.abs(F - rep).max() <= near_tol(ctx) * np.abs(rep).max()


@pytest.mark.parametrize("theta,scale", [(0.0, 1.0), (0.5, 1.0), (0.25, 30.0), (0.5, 1e-3)])
def test_gradient_duplicate_multiplicity(ctx, theta, scale):
    """Exact duplicate embedding points (QuadTree.scala:52-61): a leaf holding
    c copies re-inserts ONE when it splits, so cells created after a group's
    first copy count fewer copies, depending on the insertion (row) order.
    Groups of 2..7 copies at early, late and interleaved rows."""
    n = 600
    rp, col, val = random_problem(n, 12, seed=71)
    rng = np.random.default_rng(int(theta * 100) + int(scale))
    Y = rng.normal(size=(n, 2)) * scale
    groups = [[3, 4], [10, 300, 590], [50, 51, 52, 53, 598, 599], [7, 100, 200, 300 + 1, 400, 500, 595],
              [595 - 300, 2]]
    for g in groups:
        Y[g] = Y[g[0]]
    g_, Z, loss = ctx.gradient(rp, col, val, Y, theta, exaggeration=4.0, want_loss=True)
    r = O.gradient(rp, col, val, Y, theta, exaggeration=4.0, want_loss=True)
    tol = 1e-12 if theta == 0.0 else near_tol(ctx)
    assert np.abs(g_ - r["grad"]).max() <= tol * np.abs(r["grad"]).max()
    assert abs(Z - r["Z"]) <= tol * r["Z"]
    F, z = ctx.repulsion(Y, theta)
    assert np.abs(z - r["zi"]).max() <= tol * r["zi"].max()
    assert np.abs(F - r["rep"]).max() <= tol * np.abs(r["rep"]).max()


def test_optimize_duplicates_device_path_matches_oracle(ctx):
    """Duplicates inside the device optimizer (relabelled labels: insertion
    rows are the original indices): one step against the oracle."""
    import torch
    n = 500
    rp, col, val = random_problem(n, 12, seed=72)
    Y0 = np.random.default_rng(11).normal(size=(n, 2)) * 1e-2
    for g in ([5, 6, 400], [100, 20, 499, 250]):
        Y0[g] = Y0[g[0]]
    p = default_params(iterations=30, theta=0.5)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    dY, du, dg = t(Y0, torch.float64), torch.zeros((n, 2), dtype=torch.float64, device=dev), \
        torch.ones((n, 2), dtype=torch.float64, device=dev)
    ctx.dev_opt_setup(p, t(rp, torch.int64), t(col, torch.int32), t(val, torch.float64), n, dY, du, dg)
    ctx.dev_opt_step(1)
    ctx.dev_opt_sync()
    ctx.synchronize()
    gr = O.gradient(rp, col, val, Y0, 0.5, exaggeration=p.early_exaggeration)["grad"]
    Yo, uo, go = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    O.update(gr, Yo, uo, go, p.min_gain, p.initial_momentum, p.learning_rate)
    O.center(Yo)
    assert np.abs(dY.cpu().numpy() - Yo).max() <= 1e-6 * np.abs(Yo).max()


def test_gradient_points_outside_root_and_duplicates(ctx):
    # n = 2 on one side: W = range < |x| drops points from the reference tree
    n = 400
    rp, col, val = random_problem(n, 10, seed=11)
    Y = np.random.default_rng(2).normal(size=(n, 2)) + np.array([5.0, 3.0])
    g, Z, _ = ctx.gradient(rp, col, val, Y, 0.5)
    r = O.gradient(rp, col, val, Y, 0.5)
    assert np.abs(g - r["grad"]).max() <= 1e-4 * np.abs(r["grad"]).max()
    assert abs(Z - r["Z"]) <= near_tol(ctx) * r["Z"]


# ---------------------------------------------------------- update / centre
def test_update_and_center_goldens(ctx):
    Y = _emb().copy()
    g = np.array([v for _, v in sorted(G["denseGradientResults"])])
    upd, gains = np.zeros_like(Y), np.ones_like(Y)
    ctx.updateEmbedding(g, Y, upd, gains, 0.01, 0.5, 300.0)
    assert np.abs(Y - np.array([v for _, v in sorted(G["updatedEmbeddingResults"])])).max() <= 1e-9
    assert np.abs(gains - np.array([v for _, v in sorted(G["updatedGainsResults"])])).max() <= 1e-12
    ctx.centerEmbedding(Y)
    assert np.abs(Y - np.array([v for _, v in sorted(G["updatedAndCentredEmbeddingResults"])])).max() <= 1e-9
    C = np.array([v for _, v in sorted(G["centeringInput"])])
    ctx.centerEmbedding(C)
    assert np.array_equal(C, np.array([v for _, v in sorted(G["centeringResults"])]))


def test_iteration_golden_via_optimize(ctx):
    # iterationComputation, 1 iteration, theta 0, lr 300, momentum 0.5
    rp, col, val = triples_to_csr(G["denseJointProbabilitiesResults"], 10)
    Y = _emb().copy()
    upd, gains = np.zeros_like(Y), np.ones_like(Y)
    p = default_params(iterations=1, learning_rate=300.0, theta=0.0, early_exaggeration=1.0)
    ctx.optimize(rp, col, val, Y, upd, gains, p)
    want = np.array([v for _, v in sorted(G["updatedAndCentredEmbeddingResults"])])
    assert np.abs(Y - want).max() <= 1e-9


def test_init_working_set(ctx):
    Y, upd, gains = ctx.initWorkingSet(5000, 2, seed=7)
    assert np.all(upd == 0) and np.all(gains == 1)
    assert abs(Y.std() - 1e-4) < 5e-6 and abs(Y.mean()) < 5e-6
    Y2, _, _ = ctx.initWorkingSet(5000, 2, seed=7)
    assert np.array_equal(Y, Y2)


def test_optimize_per_iteration_gradients(ctx):
    """Per-iteration parity: drive the GPU loop one step at a time and check
    each step's embedding against the oracle's step from the same state."""
    n = 800
    rp, col, val = random_problem(n, 30, seed=21)
    Y = np.random.default_rng(5).normal(size=(n, 2)) * 1e-2
    upd, gains = np.zeros_like(Y), np.ones_like(Y)
    T_ = 130
    for t in range(1, T_ + 1):
        p = default_params(iterations=T_, theta=0.5, learning_rate=200.0)
        ex = 4.0 if t <= 101 else 1.0
        mom = 0.5 if t <= 20 else 0.8
        g, Z, _ = ctx.gradient(rp, col, val, Y, 0.5, exaggeration=ex)
        r = O.gradient(rp, col, val, Y, 0.5, exaggeration=ex)
        assert np.abs(g - r["grad"]).max() <= 1e-4 * np.abs(r["grad"]).max(), t
        ctx.updateEmbedding(r["grad"], Y, upd, gains, 0.01, mom, 200.0)
        ctx.centerEmbedding(Y)
        del p


def test_optimize_loss_matches_oracle(ctx):
    """lossFile parity.  The reference dynamics are chaotic: perturbing Y0 by
    1e-15 (relative) moves the oracle's own KL at t = 200 over a spread of
    ~0.2 (std, theta = 0.5; 40 samples span [-3.65, -2.66]).  So: the first
    iterations (before divergence) must agree within 1%, and the final KL must
    lie within 4 standard deviations (+1%) of the oracle's own perturbation
    ensemble (hard part iv)."""
    n = 600
    rp, col, val = random_problem(n, 30, seed=31)
    Y0 = np.random.default_rng(6).normal(size=(n, 2)) * 1e-4
    p = default_params(iterations=200, theta=0.5)
    Yg, ug, gg = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    lg = ctx.optimize(rp, col, val, Yg, ug, gg, p)
    runs = []
    for s in range(16):
        eps = 0.0 if s == 0 else 1e-15
        Yo = Y0 * (1 + eps * np.random.default_rng(s).normal(size=Y0.shape))
        uo, go = np.zeros_like(Y0), np.ones_like(Y0)
        runs.append(O.optimize(rp, col, val, Yo, uo, go, iterations=200, theta=0.5))
    lo = runs[0]
    assert sorted(lg) == sorted(lo) == list(range(10, 201, 10))
    # the exaggerated phase runs at the strict near-exact bound (near_tol_early)
    assert near_tol(ctx) <= 1e-6
    for t in (10, 20, 30, 40, 50):
        assert abs(lg[t] - lo[t]) <= 0.01 * abs(lo[t]), t
    final = np.array([r[200] for r in runs])
    mu, sd = final.mean(), final.std()
    assert abs(lg[200] - mu) <= 4.0 * sd + 0.01 * abs(mu), (lg[200], final)


def test_host_api_converts_csr_types(ctx):
    """int32 row_ptr, int64 col and float32 P are converted by the binding (and
    the converted copies stay alive across the library call)."""
    n = 500
    rp, col, val = random_problem(n, 10, seed=61)
    val32 = val.astype(np.float32)
    Y0 = np.random.default_rng(4).normal(size=(n, 2)) * 1e-2
    g_ref, z_ref, _ = ctx.gradient(rp, col, val32.astype(np.float64), Y0, 0.5)
    g, z, _ = ctx.gradient(rp.astype(np.int32), col.astype(np.int64), val32, Y0, 0.5)
    assert np.array_equal(g, g_ref) and z == z_ref
    p = default_params(iterations=15, theta=0.5)
    Ya, ua, ga = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    la = ctx.optimize(rp, col, val32.astype(np.float64), Ya, ua, ga, p)
    Yb, ub, gb = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    lb = ctx.optimize(list(rp), col.astype(np.int16), val32, Yb, ub, gb, p)
    assert np.array_equal(Ya, Yb) and la == lb
    with pytest.raises(ValueError):
        ctx.optimize(rp, col, val, Y0.astype(np.float32), ua, ga, p)


def test_context_options():
    """tsne_ctx_set_option / get_option: per-handle, range-checked, unknown
    keys refused (TSNE_ERR_ARG); another handle keeps the defaults."""
    with T.Context(0) as a, T.Context(0) as b:
        assert a.get_option("near_tol_early") == 1e-6 and a.get_option("near_tol_late") == 5e-6
        assert a.get_option("mom_tol") == 1e-12 and a.get_option("narrow") == 3.0
        a.set_option("near_tol_late", 2e-6)
        a.set_option("relabel", 2)
        assert a.get_option("near_tol_late") == 2e-6 and a.get_option("relabel") == 2.0
        assert b.get_option("near_tol_late") == 5e-6 and b.get_option("relabel") == -1.0
        for key, v in (("relabel", 3), ("relabel", 0.5), ("near_tol_late", -1.0), ("no_such_key", 1.0)):
            with pytest.raises(T.TsneError) as e:
                a.set_option(key, v)
            assert e.value.status == -1
        with pytest.raises(T.TsneError):
            a.counter("no_such_counter")


def test_unsupported_components(ctx):
    rp, col, val = triples_to_csr(G["denseJointProbabilitiesResults"], 10)
    Y = np.zeros((10, 4))
    p = default_params(n_components=4)
    with pytest.raises(T.TsneError) as e:
        ctx.optimize(rp, col, val, Y, np.zeros_like(Y), np.ones_like(Y), p)
    assert e.value.status == -4


def test_device_optimizer_matches_host_path(ctx):
    """tsne_dev_opt_* on torch device tensors (graph-order labels; the Morton
    relabel modes: test_relabel_modes_agree) == tsne_optimize on host buffers."""
    import torch
    n = 700
    rp, col, val = random_problem(n, 20, seed=41)
    Y0 = np.random.default_rng(8).normal(size=(n, 2)) * 1e-3
    p = default_params(iterations=80, theta=0.5)
    Yh, uh, gh = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    lh = ctx.optimize(rp, col, val, Yh, uh, gh, p)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    dY, du, dg = t(Y0, torch.float64), torch.zeros((n, 2), dtype=torch.float64, device=dev), \
        torch.ones((n, 2), dtype=torch.float64, device=dev)
    ctx.dev_opt_setup(p, t(rp, torch.int64), t(col, torch.int32), t(val, torch.float64), n, dY, du, dg)
    for it in range(1, 81):
        ctx.dev_opt_step(it)
    ctx.dev_opt_sync()
    ctx.synchronize()
    assert np.array_equal(dY.cpu().numpy(), Yh)
    assert np.array_equal(du.cpu().numpy(), uh) and np.array_equal(dg.cpu().numpy(), gh)
    assert ctx.dev_opt_losses() == lh


def hub_problem(n=6000, seed=71):
    """A kNN joint P plus three dense hub rows/columns (rows spanning several
    waves, windows and wide slices of the tiled attraction)."""
    import scipy.sparse as sp
    rp, col, val = random_problem(n, 30, seed=seed)
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


@pytest.mark.parametrize("metric", ["sqeuclidean", "euclidean", "cosine"])
def test_tiled_attraction_matches_oracle(ctx, metric):
    """The optimizer's tiled attraction (attract_tiles: row blocks x 5888-label
    column windows, rows as lanes of jagged-diagonal slices, hub rows split
    over a wave) on a P with dense hub rows and columns, over 10 iterations at
    theta 0 (exact repulsion on both sides): the embedding and the loss at
    t = 10 against the oracle."""
    n = 6000
    rp2, col2, val2 = hub_problem(n)
    Y0 = np.random.default_rng(73).normal(size=(n, 2)) * 5.0
    prm = default_params(iterations=10, theta=0.0, metric=metric, learning_rate=200.0)
    Yg, ug, gg = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    lg = ctx.optimize(rp2, col2, val2, Yg, ug, gg, prm)
    Yo, uo, go = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    lo = O.optimize(rp2, col2, val2, Yo, uo, go, metric=metric, learning_rate=200.0, iterations=10, theta=0.0,
                    threads=8)
    assert np.abs(Yg - Yo).max() <= 1e-9 * np.abs(Yo).max()
    assert abs(lg[10] - lo[10]) <= 1e-9 * abs(lo[10])


def test_tiled_attraction_every_config():
    """Each row-block configuration of attract_tiles (512 ... 4096 rows; a run
    picks one by its owned rows, the "attract_cfg" option forces it) and
    attract_rows ("attract_tiles" 0), each on its own context, against the
    oracle."""
    n = 12000
    rp, col, val = hub_problem(n)
    Y0 = np.random.default_rng(74).normal(size=(n, 2)) * 5.0
    Yo, uo, go = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    lo = O.optimize(rp, col, val, Yo, uo, go, learning_rate=200.0, iterations=10, theta=0.0, threads=8)
    for opt in ({"attract_cfg": 0}, {"attract_cfg": 1}, {"attract_cfg": 2}, {"attract_cfg": 3},
                {"attract_cfg": 0, "attract_dyn": 0}, {"attract_cfg": 2, "attract_dyn": 0}, {"attract_tiles": 0}):
        with T.Context(0) as c:
            for k, v in opt.items():
                c.set_option(k, v)
            Yg, ug, gg = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
            lg = c.optimize(rp, col, val, Yg, ug, gg, default_params(iterations=10, theta=0.0, learning_rate=200.0))
        assert np.abs(Yg - Yo).max() <= 1e-9 * np.abs(Yo).max(), opt
        assert abs(lg[10] - lo[10]) <= 1e-9 * abs(lo[10]), opt


def test_tiled_attraction_pipe_identical():
    """The pipelined tiled attraction ("attract_pipe" 1..5: the next 1..3
    slices' entries in flight while a wave sums the current one; non-loss
    launches) and attract_tiles with claimed slices ("attract_dyn" 1, non-loss
    launches) return the same bits as attract_tiles over 10 iterations of a P
    with hub rows (wide slices, rows past the pipelined steps), at the
    4096-row configuration the pipeline is built for; and the oracle's
    embedding within 1e-9."""
    n = 12000
    rp, col, val = hub_problem(n)
    Y0 = np.random.default_rng(75).normal(size=(n, 2)) * 5.0
    Yo, uo, go = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    lo = O.optimize(rp, col, val, Yo, uo, go, learning_rate=200.0, iterations=10, theta=0.0, threads=8)
    ref = None
    for pipe, dyn in [(0, 0), (0, 1)] + [(k, 0) for k in range(1, 6)]:
        with T.Context(0) as c:
            c.set_option("attract_cfg", 3)
            c.set_option("attract_pipe", pipe)
            c.set_option("attract_dyn", dyn)
            Yg, ug, gg = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
            lg = c.optimize(rp, col, val, Yg, ug, gg, default_params(iterations=10, theta=0.0, learning_rate=200.0))
        if ref is None:
            ref = (Yg, ug, gg, lg)
        else:
            assert np.array_equal(Yg, ref[0]) and np.array_equal(ug, ref[1]) and np.array_equal(gg, ref[2]), pipe
            assert lg == ref[3], pipe
        assert np.abs(Yg - Yo).max() <= 1e-9 * np.abs(Yo).max(), pipe
        assert abs(lg[10] - lo[10]) <= 1e-9 * abs(lo[10]), pipe


def _relabel_run(relabel):
    """60 iterations host API and device API with the given "relabel" option:
    both bit-equal; returns (Y, loss at t = 60)."""
    import torch
    n = 700
    rp, col, val = random_problem(n, 20, seed=41)
    Y0 = np.random.default_rng(8).normal(size=(n, 2)) * 1e-3
    p = default_params(iterations=60, theta=0.5)
    with T.Context(0) as c:
        c.set_option("relabel", relabel)
        Yh, uh, gh = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
        lh = c.optimize(rp, col, val, Yh, uh, gh, p)
        dev = torch.device("cuda", 0)
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)  # noqa: E731
        dY = t(Y0, torch.float64)
        du = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        dg = torch.ones((n, 2), dtype=torch.float64, device=dev)
        c.dev_opt_setup(p, t(rp, torch.int64), t(col, torch.int32), t(val, torch.float64), n, dY, du, dg)
        for it in range(1, 61):
            c.dev_opt_step(it)
        c.dev_opt_sync()
        c.synchronize()
        assert np.array_equal(dY.cpu().numpy(), Yh) and c.dev_opt_losses() == lh
    return Yh, lh[60]


def test_relabel_modes_agree():
    """One rank with the tiled layout keeps P's graph order by default (no
    Morton relabel); "relabel" 2 relabels at every check (t % 25 == 0) and
    hands the attraction to attract_rows.  Both: device path == host path bit
    for bit, and the two trajectories agree within 1e-6 relative after 60
    iterations (two relabels).  They differ only in summation orders
    (~1e-16), which the BH decisions amplify: on this problem the oracle's own
    runs from Y0 perturbed by 1e-15 (relative) differ by 2e-8..2e-6 at t = 30
    and 3e-2..0.9 at t = 60; the two modes measured 5e-9 at t = 60
    (deterministic runs: a stable check)."""
    ya, la = _relabel_run(-1)
    yb, lb = _relabel_run(2)
    assert np.abs(ya - yb).max() <= 1e-6 * np.abs(yb).max()
    assert abs(la - lb) <= 1e-6 * abs(lb)


def test_moment_path_engaged(ctx):
    """Tiny embedding (the first iterations): every query's whole tree is one
    near-exact subtree, evaluated from the root's moments (one moment task per
    point, no dense pair terms), and the step still matches the host path."""
    import torch
    n = 20000
    rp, col, val = random_problem(n, 10, seed=51)
    Y0 = np.random.default_rng(9).normal(size=(n, 2)) * 1e-4
    p = default_params(iterations=3, theta=0.5)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    dY, du, dg = t(Y0, torch.float64), torch.zeros((n, 2), dtype=torch.float64, device=dev), \
        torch.ones((n, 2), dtype=torch.float64, device=dev)
    ctx.dev_opt_setup(p, t(rp, torch.int64), t(col, torch.int32), t(val, torch.float64), n, dY, du, dg)
    ctx.dev_opt_profile(1)
    ctx.dev_opt_step(1)
    _, cnt = ctx.dev_opt_profile(0)
    assert cnt[1] == n and cnt[2] == 0, cnt
    ctx.dev_opt_sync()
    ctx.synchronize()
    g = O.gradient(rp, col, val, Y0, 0.5, exaggeration=p.early_exaggeration)["grad"]
    Yo, uo, go = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    O.update(g, Yo, uo, go, p.min_gain, p.initial_momentum, p.learning_rate)
    O.center(Yo)
    assert np.abs(dY.cpu().numpy() - Yo).max() <= 1e-9 * np.abs(Yo).max()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_device_balance_cuts_match_host_rule(ctx, world):
    """The multi-GPU optimizer's per-iteration cost-balanced BH slices (device
    kernel balance_slices) equal the host rule tsne_balance_cuts."""
    import torch
    rng = np.random.default_rng(world)
    for n, zero_frac in ((1_000_000, 0.0), (300_000, 0.9), (5_000, 1.0)):
        nb = -(-n // 256)
        c = rng.integers(1, 5000, nb).astype(np.uint64)
        c[rng.random(nb) < zero_frac] = 0
        want = T.balance_cuts(c, n, world)
        dc = torch.from_numpy(c.astype(np.int64)).cuda()
        db = torch.zeros(world + 1, dtype=torch.int64, device="cuda")
        ctx.dev_balance_cuts(dc, n, world, db)
        ctx.synchronize()
        assert db.cpu().numpy().tolist() == want.tolist(), (n, zero_frac)


# ------------------------------------------- 3-D embeddings (octree extension)
@pytest.mark.parametrize("n,scale,theta", [
    (600, 1.0, 0.0), (3000, 1e-4, 0.5), (3000, 0.05, 0.5), (3000, 1.0, 0.5), (3000, 20.0, 0.25),
    (20000, 3.0, 0.5), (20000, 1e-3, 0.5), (20000, 0.02, 0.5), (20000, 0.1, 0.25)])
def test_gradient3_matches_oracle(ctx, n, scale, theta):
    """nComponents = 3: the GPU octree vs the octree
    restatement (oracle/tsne_oracle.c oracle_gradient3; parity unpinned by
    the reference, which requires 2-D).  The small scales make whole
    subtrees exact tiles evaluated from their moments (oct_mom_apply)."""
    rp, col, val = random_problem(n, 10, seed=n + int(scale * 100))
    Y = np.random.default_rng(n).normal(size=(n, 3)) * scale
    g, Z, loss = ctx.gradient(rp, col, val, Y, theta, exaggeration=4.0, want_loss=True)
    r = O.gradient3(rp, col, val, Y, theta, exaggeration=4.0, want_loss=True)
    tol = 1e-12 if theta == 0.0 else 1e-6
    assert np.abs(g - r["grad"]).max() <= tol * np.abs(r["grad"]).max()
    assert abs(Z - r["Z"]) <= 1e-7 * r["Z"]
    assert abs(loss - r["loss"]) <= 1e-6 * abs(r["loss"])


def test_gradient3_outside_root_and_metrics(ctx):
    n = 800
    rp, col, val = random_problem(n, 10, seed=12)
    Y = np.random.default_rng(3).normal(size=(n, 3)) + np.array([4.0, -2.0, 1.0])   # points outside the root
    # (exact duplicates are a documented deviation: the reference restarts their
    # multiplicity at every split of their leaf, QuadTree.scala:57-60; the fit's
    # own rule -- full multiplicity, nothing from a copy at the query's position --
    # is held against the exact sums and the oracle in test_gpu_octree_edges.py,
    # with boundary points, key ties, degenerate clouds and small trees)
    for metric in ("sqeuclidean", "euclidean", "cosine"):
        g, Z, _ = ctx.gradient(rp, col, val, Y, 0.5, metric=metric)
        r = O.gradient3(rp, col, val, Y, 0.5, metric=metric)
        assert np.abs(g - r["grad"]).max() <= 1e-4 * np.abs(r["grad"]).max(), metric


def test_optimize3_matches_oracle_and_device_path(ctx):
    import torch
    n = 500
    rp, col, val = random_problem(n, 30, seed=33)
    Y0 = np.random.default_rng(7).normal(size=(n, 3)) * 1e-4
    p = default_params(n_components=3, iterations=60, theta=0.5)
    Yh, uh, gh = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    lh = ctx.optimize(rp, col, val, Yh, uh, gh, p)
    Yo, uo, go = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    lo = O.optimize3(rp, col, val, Yo, uo, go, iterations=60, theta=0.5)
    assert sorted(lh) == sorted(lo) == list(range(10, 61, 10))
    for t in (10, 20, 30):
        assert abs(lh[t] - lo[t]) <= 0.01 * abs(lo[t]), t
    assert np.isfinite(Yh).all() and np.abs(Yh.mean(0)).max() <= 1e-9 * (1 + np.abs(Yh).max())
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    dY = t(Y0, torch.float64)
    du = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    dg = torch.ones((n, 3), dtype=torch.float64, device=dev)
    ctx.dev_opt_setup(p, t(rp, torch.int64), t(col, torch.int32), t(val, torch.float64), n, dY, du, dg)
    for it in range(1, 61):
        ctx.dev_opt_step(it)
    ctx.dev_opt_sync()
    ctx.synchronize()
    assert np.array_equal(dY.cpu().numpy(), Yh)
    assert np.array_equal(dg.cpu().numpy(), gh)
    assert ctx.dev_opt_losses() == lh


# ------------------------------------------------ projectKnn (--knnMethod project)
@pytest.mark.parametrize("n,d,k,it,metric", [
    (3000, 16, 10, 3, "sqeuclidean"), (2000, 40, 30, 4, "euclidean"), (1500, 20, 12, 2, "cosine"),
    (500, 1, 8, 1, "sqeuclidean"), (60, 5, 90, 3, "sqeuclidean")])
def test_project_knn_matches_oracle(ctx, n, d, k, it, metric):
    """GPU Z-order merge sorts + candidate ranking vs the restatement, on
    nonnegative data (where the reference comparator is a total order)."""
    rng = np.random.default_rng(n + d)
    X = np.abs(rng.normal(size=(6, d)))[rng.integers(0, 6, n)] * 2 + rng.random((n, d))
    sh = rng.random((it - 1, d))
    gi, gd = ctx.projectKnn(X, k, metric, iterations=it, shifts=sh)
    oi, od = O.project_knn(X, k, metric, iterations=it, shifts=sh)
    assert np.array_equal(gi, oi)
    assert np.array_equal(gd, od)
