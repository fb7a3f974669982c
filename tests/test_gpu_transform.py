"""Embedding new points into a fitted map (csrc/transform.hip): the cross
kNN, Barnes-Hut repulsion for query points that are not in the tree, and the
optimizer that moves only the new points.

Bounds.  Foreign-query repulsion against the oracle, per query:
|z - z_o| <= 1e-11 z_o and max|F - F_o| <= 1e-11 z_o.  At most n = 5000 terms
of a few roundings each give n * 4 * 2^-53 ~ 2e-12 of the sum of absolute
terms; every force term has |q^2 d| <= q / 2, so that sum is at most z / 2.  A
wrong cell decision shows at 1e-6 or more.  The inputs avoid Morton key ties
(no two distinct reference points closer than 1e-9 of the extent): a tie
group follows the library's documented approximation, not the oracle.

A transform step: the gradient error is <= 3e-11 (the bound above through
rep / z with |rep / z| <= 1/2 gives 2e-11, plus the k-term attraction), so
|dY|, |dupd| <= 3e-11 lr (gains_o + 1) + 4 * 2^-52 |Y_o|; the (gains_o + 1)
factor also covers a flipped sign test of the gains rule, which needs
|g| <= 3e-11.  Gains are bit-equal wherever |g_o| > 3e-11."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_ctypes as O
import tsne_amd as T
from tsne_amd.api import default_params

pytestmark = pytest.mark.gpu

N_REF = 5000
DUP_GROUPS = ([5, 6, 400], [99, 98])


# ------------------------------------------------------------------ A: inputs
def ref_map(case):
    rng = np.random.default_rng(11)
    Y = rng.normal(size=(N_REF, 2))
    Y -= Y.mean(axis=0)
    if case == "s1e-2":
        Y *= 1e-2
    elif case == "s30":
        Y *= 30.0
    elif case == "offcentre":     # some points fall outside the reference root Cell(0, 0, W)
        Y += np.array([5.0, 3.0])
    elif case == "dups":
        for g in DUP_GROUPS:
            Y[g[1:]] = Y[g[0]]
    else:
        assert case == "s1"
    return np.ascontiguousarray(Y)


def queries(Y, m=1003):
    rng = np.random.default_rng(23)
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    mid, ext = 0.5 * (lo + hi), float((hi - lo).max())
    sd = Y.std(axis=0)
    parts = [Y.mean(axis=0) + rng.normal(size=(m - 400, 2)) * sd]          # the map's distribution
    rows = rng.integers(0, N_REF, 100)
    rows[0] = DUP_GROUPS[0][0]                                              # a member of a duplicate group
    parts.append(Y[rows].copy())                                            # bitwise copies of reference rows
    a, b = rng.integers(0, N_REF, 100), rng.integers(0, N_REF, 100)
    parts.append(0.5 * (Y[a] + Y[b]))                                       # midpoints of reference pairs
    ang = rng.uniform(0, 2 * np.pi, 100)
    fac = np.exp(rng.uniform(np.log(1.5), np.log(1000.0), 100))
    fac[0] = 1.5                                                            # the root summarised in one visit
    parts.append(mid + (ext * fac)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1))
    side = rng.integers(0, 4, 100)                                          # just outside the bounding box
    u = rng.uniform(0, 1, 100)
    eps = ext * np.exp(rng.uniform(np.log(1e-9), np.log(1e-2), 100))
    px = np.where(side == 0, lo[0] - eps, np.where(side == 1, hi[0] + eps, lo[0] + u * (hi[0] - lo[0])))
    py = np.where(side == 2, lo[1] - eps, np.where(side == 3, hi[1] + eps, lo[1] + u * (hi[1] - lo[1])))
    parts.append(np.stack([px, py], axis=1))
    Q = np.ascontiguousarray(np.concatenate(parts))
    assert Q.shape == (m, 2)
    return Q


_cases = {}


def case_data(case):
    """Per reference map: Y, the queries, the oracle tree (built once, shared)."""
    if case not in _cases:
        Y = ref_map(case)
        # no Morton key ties: distinct points are farther apart than 1e-9 of the extent
        ext = float((Y.max(axis=0) - Y.min(axis=0)).max())
        order = np.argsort(Y[:, 0])
        Ys = Y[order]
        for s in range(1, 40):
            d = np.abs(Ys[s:] - Ys[:-s]).max(axis=1)
            assert not np.any((d > 0) & (d < 1e-9 * ext))
        _cases[case] = (Y, queries(Y), O.Tree(Y))
    return _cases[case]


def check_against_oracle(F, z, Fo, zo):
    print("max |z - zo| / zo = %.3e, max |F - Fo| / zo = %.3e"
          % (np.max(np.abs(z - zo) / zo), np.max(np.abs(F - Fo).max(axis=1) / zo)))
    assert np.all(zo > 0)
    assert np.all(np.abs(z - zo) <= 1e-11 * zo)
    assert np.all(np.abs(F - Fo).max(axis=1) <= 1e-11 * zo)


@pytest.fixture(scope="module")
def ctx():
    with T.Context(0) as c:
        yield c


@pytest.mark.parametrize("theta", [0.0, 0.25, 0.5])
@pytest.mark.parametrize("case", ["s1e-2", "s1", "s30", "offcentre", "dups"])
def test_foreign_queries_match_oracle(ctx, case, theta):
    Y, Q, tree = case_data(case)
    Fo, zo, _ = tree.query(theta, Q)
    F, z = ctx.repulsionQueries(Y, theta, Q)
    check_against_oracle(F, z, Fo, zo)
    for m in (1, 65):   # one lane; one full wave and a single lane of the next
        Fm, zm = ctx.repulsionQueries(Y, theta, Q[700:700 + m])
        check_against_oracle(Fm, zm, Fo[700:700 + m], zo[700:700 + m])


def test_foreign_queries_oracle_forms_agree():
    """O.repulsion_queries (tree built inside) is the same reference as O.Tree(Y).query."""
    Y, Q, tree = case_data("s1")
    Fo, zo, _ = tree.query(0.5, Q[:50])
    F2, z2 = O.repulsion_queries(Y, 0.5, Q[:50])
    assert np.array_equal(Fo, F2) and np.array_equal(zo, z2)


# ------------------------------------------------------ B: batch independence
@pytest.mark.parametrize("case,theta", [("s1", 0.5), ("dups", 0.25)])
def test_repulsion_queries_batch_independent(ctx, case, theta):
    Y, Q, _ = case_data(case)
    F, z = ctx.repulsionQueries(Y, theta, Q)
    rng = np.random.default_rng(3)
    sub = rng.permutation(len(Q))[:130]
    Fs, zs = ctx.repulsionQueries(Y, theta, Q[sub])
    assert np.array_equal(Fs, F[sub]) and np.array_equal(zs, z[sub])
    for i in (0, 603, 650, 750, 800, 950, 1002):   # each group of the queries, alone
        F1, z1 = ctx.repulsionQueries(Y, theta, Q[i:i + 1])
        assert np.array_equal(F1[0], F[i]) and z1[0] == z[i]


# ---------------------------------------------------- C: members as queries
@pytest.mark.parametrize("theta", [0.25, 0.5])
def test_members_as_queries_match_member_path(theta):
    Y, _, _ = case_data("s1")
    with T.Context(0) as c:
        c.set_option("near_tol_early", 0)   # the member path's near-exact test off
        Fm, zm = c.repulsion(Y, theta)
        F, z = c.repulsionQueries(Y, theta, Y)
    check_against_oracle(F, z, Fm, zm)


# ------------------------------------------------------------- D: cross kNN
@pytest.mark.parametrize("k", [10, 5000])
@pytest.mark.parametrize("metric", ["sqeuclidean", "euclidean", "cosine"])
@pytest.mark.parametrize("d", [7, 64])
def test_knn_cross_matches_oracle(ctx, d, metric, k):
    n, m = 3000, 257
    rng = np.random.default_rng(100 + d)
    X = rng.normal(size=(5, d))[rng.integers(0, 5, n)] * 3 + rng.normal(size=(n, d))
    X[11] = X[10]                                  # two identical reference rows: the tie is ordered by j
    Xq = rng.normal(size=(5, d))[rng.integers(0, 5, m)] * 3 + rng.normal(size=(m, d))
    Xq[0] = X[1234]                                # a query equal to a reference row: distance 0, kept
    Xq[1] = X[10]
    gi, gd = ctx.kNearestNeighborsCross(X, Xq, k, metric)
    kk = min(k, n)
    assert gi.shape == (m, kk) and gd.shape == (m, kk)
    for q in range(m):
        oi, od = O.knn(np.vstack([X, Xq[q:q + 1]]), k, metric, q0=n, q1=n + 1)
        assert np.array_equal(gi[q], oi[0]), q
        assert np.array_equal(gd[q], od[0]), q
    assert gi[0, 0] == 1234 and (metric == "cosine" or gd[0, 0] == 0.0)
    assert list(gi[1, :2]) == [10, 11]


# --------------------------------------------- E, F, G: the transform input
class XInput:
    """n = 2000 map points in five blobs (one triple of coincident points),
    m = 300 new points with their 30 nearest map points and P at perplexity 10."""

    def __init__(self, ctx):
        rng = np.random.default_rng(7)
        n, m, k = 2000, 300, 30
        centres = rng.normal(size=(5, 2)) * 12.0
        Yr = centres[rng.integers(0, 5, n)] + rng.normal(size=(n, 2)) * 2.0
        Yr -= Yr.mean(axis=0)
        Yr[[700, 701]] = Yr[17]
        hidden = Yr[rng.integers(0, n, m)] + rng.normal(size=(m, 2)) * 0.7
        d2 = ((hidden[:, None, :] - Yr[None, :, :]) ** 2).sum(axis=2)
        col = np.argsort(d2, axis=1, kind="stable")[:, :k].astype(np.int32)
        dist = np.take_along_axis(d2, col.astype(np.int64), axis=1)
        self.n, self.m, self.k = n, m, k
        self.Yr = np.ascontiguousarray(Yr)
        self.rp = np.arange(0, m * k + 1, k, dtype=np.int64)
        self.col = np.ascontiguousarray(col.ravel())
        self.P = ctx.pairwiseAffinities(self.rp, dist.ravel(), 10.0)
        self.prm = default_params(iterations=110, theta=0.5, learning_rate=1.0)
        self.tree = O.Tree(self.Yr)


@pytest.fixture(scope="module")
def xin(ctx):
    return XInput(ctx)


def init_loop(xin):
    Y0 = np.zeros((xin.m, 2))
    for i in range(xin.m):
        ax = ay = 0.0
        for e in range(xin.rp[i], xin.rp[i + 1]):
            p, j = float(xin.P[e]), xin.col[e]
            ax = ax + p * float(xin.Yr[j, 0])
            ay = ay + p * float(xin.Yr[j, 1])
        Y0[i] = (ax, ay)
    return Y0


def test_transform_init_is_sequential_weighted_mean(ctx, xin):
    assert np.array_equal(ctx.transformInit(xin.rp, xin.col, xin.P, xin.Yr), init_loop(xin))


def schedule(prm, t):
    n1 = min(prm.iterations, 20)
    n2 = min(prm.iterations - n1, 81)
    return (prm.early_exaggeration if t <= n1 + n2 else 1.0,
            prm.initial_momentum if t <= n1 else prm.final_momentum)


def oracle_terms(xin, Y, ex):
    """rep, z from the oracle tree; attraction and loss terms by numpy in CSR order."""
    rep, z, _ = xin.tree.query(xin.prm.theta, Y)
    col = xin.col.reshape(xin.m, xin.k)
    pe = ex * xin.P.reshape(xin.m, xin.k)
    dx = Y[:, None, 0] - xin.Yr[col, 0]
    dy = Y[:, None, 1] - xin.Yr[col, 1]
    q = 1.0 / (1.0 + (dx * dx + dy * dy))
    s = pe * q
    attr = np.zeros((xin.m, 2))
    for e in range(xin.k):   # sequential over a row's entries
        attr[:, 0] = attr[:, 0] + s[:, e] * dx[:, e]
        attr[:, 1] = attr[:, 1] + s[:, e] * dy[:, e]
    grad = attr - rep / z[:, None]
    terms = pe * np.log(pe / (q / z[:, None]))
    return grad, terms


@pytest.fixture(scope="module")
def stepped(ctx, xin):
    """The device transform stepped through t = 1..110; the state before and
    after the checked steps and before every loss step."""
    dev = "cuda:0"
    dYr = torch.tensor(xin.Yr, device=dev)
    drp, dcol, dP = torch.tensor(xin.rp, device=dev), torch.tensor(xin.col, device=dev), torch.tensor(xin.P, device=dev)
    dY = torch.tensor(ctx.transformInit(xin.rp, xin.col, xin.P, xin.Yr), device=dev)
    du, dg = torch.zeros_like(dY), torch.ones_like(dY)
    torch.cuda.synchronize()
    ctx.dev_transform_setup(xin.prm, dYr, drp, dcol, dP, dY, du, dg)

    def state():
        ctx.dev_transform_sync()
        return dY.cpu().numpy().copy(), du.cpu().numpy().copy(), dg.cpu().numpy().copy()

    pre, post = {}, {}
    for t in range(1, xin.prm.iterations + 1):
        if t in (1, 2, 20, 21, 101, 102, 110) or t % 10 == 0:
            pre[t] = state()
        ctx.dev_transform_step(t)
        if t in (1, 2, 20, 21, 101, 102, 110):
            post[t] = state()
    final = state()
    return pre, post, final, ctx.dev_transform_losses()


@pytest.mark.parametrize("t", [1, 2, 20, 21, 101, 102, 110])
def test_transform_step_matches_oracle_step(xin, stepped, t):
    pre, post, _, _ = stepped
    Y, upd, gains = (a.copy() for a in pre[t])
    ex, mom = schedule(xin.prm, t)
    grad, _ = oracle_terms(xin, Y, ex)
    lr = xin.prm.learning_rate
    O.update(np.ascontiguousarray(grad), Y, upd, gains, xin.prm.min_gain, mom, lr)
    Yg, ug, gg = post[t]
    bound = 3e-11 * lr * (gains + 1.0) + 4 * 2.0 ** -52 * np.abs(Y)
    print("t = %d: max |dY| / bound = %.3e, max |dupd| / bound = %.3e"
          % (t, np.max(np.abs(Yg - Y) / bound), np.max(np.abs(ug - upd) / bound)))
    assert np.all(np.abs(Yg - Y) <= bound)
    assert np.all(np.abs(ug - upd) <= bound)
    sure = np.abs(grad) > 3e-11
    assert np.count_nonzero(~sure) <= 1e-3 * grad.size
    assert np.array_equal(gg[sure], gains[sure])


def test_transform_losses_match_formula(xin, stepped):
    pre, _, _, losses = stepped
    assert sorted(losses) == list(range(10, 111, 10))
    for t, got in losses.items():
        ex, _ = schedule(xin.prm, t)
        _, terms = oracle_terms(xin, pre[t][0], ex)
        print("t = %d: loss %.12g, numpy %.12g" % (t, got, terms.sum()))
        assert abs(got - terms.sum()) <= 1e-9 * np.abs(terms).sum()


# ---------------------------------------------------------- G: consistency
def host_transform(ctx, xin, rows, iterations):
    """tsne_transform on the new points `rows` (all iterations in one call)."""
    k = xin.k
    rp = np.arange(0, len(rows) * k + 1, k, dtype=np.int64)
    col = np.ascontiguousarray(xin.col.reshape(-1, k)[rows].ravel())
    P = np.ascontiguousarray(xin.P.reshape(-1, k)[rows].ravel())
    Y = ctx.transformInit(rp, col, P, xin.Yr)
    upd, gains = np.zeros_like(Y), np.ones_like(Y)
    prm = default_params(iterations=iterations, theta=0.5, learning_rate=1.0)
    losses = ctx.transform(xin.Yr, rp, col, P, Y, upd, gains, prm)
    return Y, upd, gains, losses


def test_transform_one_call_equals_stepping(ctx, xin, stepped):
    _, _, (Ys, us, gs), losses = stepped
    Y, upd, gains, hl = host_transform(ctx, xin, np.arange(xin.m), 110)
    assert np.array_equal(Y, Ys) and np.array_equal(upd, us) and np.array_equal(gains, gs)
    assert hl == losses


def test_transform_batch_independent(ctx, xin):
    Y, upd, gains, _ = host_transform(ctx, xin, np.arange(xin.m), 40)
    sub = np.random.default_rng(9).permutation(xin.m)[:70]
    Ys, us, gs, _ = host_transform(ctx, xin, sub, 40)
    assert np.array_equal(Ys, Y[sub]) and np.array_equal(us, upd[sub]) and np.array_equal(gs, gains[sub])


@pytest.mark.parametrize("option,value", [("transform_resort", 0), ("transform_resort", 1), ("transform_split", 1)])
def test_transform_layout_options_change_no_bit(ctx, xin, option, value):
    """How often the new points are re-sorted, and the walk and the update as
    two launches instead of one, change which lanes and launches do the work,
    not a bit of the result (the canonical order)."""
    base = host_transform(ctx, xin, np.arange(xin.m), 40)
    with T.Context(0) as c:
        c.set_option(option, value)
        other = host_transform(c, xin, np.arange(xin.m), 40)
    for a, b in zip(base[:3], other[:3]):
        assert np.array_equal(a, b)
    assert base[3] == other[3]


def test_transform_end_to_end_places_rows_near_their_neighbours(ctx):
    """tsne_amd.transform on 2000 x 16 GMM rows.  The map is a linear one (the
    two leading principal axes of the reference rows, scaled to t-SNE's usual
    extent): cheap, deterministic, and neighbours in X are neighbours on it."""
    rng = np.random.default_rng(41)
    n, m, d = 1700, 300, 16
    centres = rng.normal(size=(6, d)) * 4.0
    X = centres[rng.integers(0, 6, n + m)] + rng.normal(size=(n + m, d))
    X_ref, X_new = X[:n], X[n:]
    Xc = X_ref - X_ref.mean(axis=0)
    _, _, vt = np.linalg.svd(Xc, full_matrices=False)
    Y_ref = Xc @ vt[:2].T
    Y_ref *= 30.0 / np.abs(Y_ref).max()
    Y_new, losses = T.transform(ctx, X_ref, Y_ref, X_new, k=30, perplexity=10.0)
    assert Y_new.shape == (m, 2) and np.all(np.isfinite(Y_new))
    assert sorted(losses) == list(range(10, 301, 10))
    d2 = ((X_new[:, None, :] - X_ref[None, :, :]) ** 2).sum(axis=2)
    target = Y_ref[np.argsort(d2, axis=1)[:, :5]].mean(axis=1)
    placed = np.linalg.norm(Y_new - target, axis=1).mean()
    shuffled = np.linalg.norm(Y_new[rng.permutation(m)] - target, axis=1).mean()
    print("mean distance to the 5 nearest reference rows' map position: %.3f (permuted: %.3f)" % (placed, shuffled))
    assert placed < shuffled


# -------------------------------------------------------- H: argument errors
def test_transform_argument_errors(ctx, xin):
    Y = ctx.transformInit(xin.rp, xin.col, xin.P, xin.Yr)
    upd, gains = np.zeros_like(Y), np.ones_like(Y)
    with pytest.raises(T.TsneError) as e:
        ctx.transform(xin.Yr, xin.rp, xin.col, xin.P, Y, upd, gains, default_params(n_components=3, iterations=5))
    assert e.value.status == -4
    rp = xin.rp.copy()
    rp[4:] -= xin.k                                 # row 3 has no entries
    with pytest.raises(T.TsneError) as e:
        ctx.transformInit(rp, xin.col[:rp[-1]], xin.P[:rp[-1]], xin.Yr)
    assert e.value.status == -1
    for bad in (-1, xin.n):
        col = xin.col.copy()
        col[77] = bad
        with pytest.raises(T.TsneError) as e:
            ctx.transform(xin.Yr, xin.rp, col, xin.P, Y, upd, gains, default_params(iterations=5))
        assert e.value.status == -1
    # m = 0 is a no-op
    rc = T.lib().tsne_transform(ctx.handle, C.byref(default_params(iterations=5)), xin.Yr.ctypes.data_as(C.c_void_p),
                                xin.n, None, None, None, 0, None, None, None, None, None, 0, None)
    assert rc == 0
