"""Embedding new points into a fitted 3-D map (csrc/transform.hip): the
octree walk for query points that are not in the tree, and the optimizer that
moves only the new points.  Section by section the 3-D form of
test_gpu_transform.py, against the oracle's octree restatement
(oracle_repulsion3_queries).

Bounds.  Foreign-query repulsion against the oracle, per query:
|z - z_o| <= 1e-11 z_o and max|F - F_o| <= 1e-11 z_o.  The 2-D file's
derivation holds in any dimension: every force term has |q^2 d| <= q / 2, and
n = 5000 terms of five roundings each give n * 5 * 2^-53 ~ 2.8e-12 of z / 2.
A wrong cell decision shows at 1e-6 or more.  The inputs avoid Morton key
ties: the octree has 21 levels per axis, a level-21 cell is about 1e-6 of the
extent, and no two distinct reference points are closer than 1e-5 of it (in
the Chebyshev distance); a tie group follows the library's documented
approximation, not the oracle.  Exact duplicates are counted as the oracle
counts them (the re-insert-once rule, transform.hip dup_fix3).

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
from test_gpu_transform import XInput as XInput2
from test_gpu_transform import queries as queries2
from test_gpu_transform import ref_map as ref_map2
from tsne_amd.api import default_params

pytestmark = pytest.mark.gpu

N_REF = 5000
DUP_GROUPS = ([5, 6, 400], [99, 98])


# ------------------------------------------------------------------ A: inputs
def ref_map3(case):
    rng = np.random.default_rng(11)
    Y = rng.normal(size=(N_REF, 3))
    Y -= Y.mean(axis=0)
    if case == "s1e-2":
        Y *= 1e-2
    elif case == "s30":
        Y *= 30.0
    elif case == "offcentre":     # some points fall outside the root Cell(0, 0, 0, W)
        Y += np.array([5.0, 3.0, -4.0])
    elif case == "dups":
        for g in DUP_GROUPS:
            Y[g[1:]] = Y[g[0]]
    else:
        assert case == "s1"
    return np.ascontiguousarray(Y)


def queries3(Y, m=1003):
    rng = np.random.default_rng(23)
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    mid, ext = 0.5 * (lo + hi), float((hi - lo).max())
    sd = Y.std(axis=0)
    parts = [Y.mean(axis=0) + rng.normal(size=(m - 400, 3)) * sd]          # the map's distribution
    rows = rng.integers(0, N_REF, 100)
    rows[0] = DUP_GROUPS[0][0]                                              # a member of a duplicate group
    parts.append(Y[rows].copy())                                            # bitwise copies of reference rows
    a, b = rng.integers(0, N_REF, 100), rng.integers(0, N_REF, 100)
    parts.append(0.5 * (Y[a] + Y[b]))                                       # midpoints of reference pairs
    u = rng.normal(size=(100, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    fac = np.exp(rng.uniform(np.log(1.5), np.log(1000.0), 100))
    fac[0] = 1.5                                                            # the root summarised in one visit
    parts.append(mid + (ext * fac)[:, None] * u)
    axis, sign = rng.integers(0, 3, 100), rng.integers(0, 2, 100)           # just outside one face of the box
    p = lo + rng.uniform(0, 1, (100, 3)) * (hi - lo)
    eps = ext * np.exp(rng.uniform(np.log(1e-9), np.log(1e-2), 100))
    r = np.arange(100)
    p[r, axis] = np.where(sign == 0, lo[axis] - eps, hi[axis] + eps)
    parts.append(p)
    Q = np.ascontiguousarray(np.concatenate(parts))
    assert Q.shape == (m, 3)
    return Q


def min_chebyshev(Y):
    """Smallest Chebyshev distance between two distinct points of Y."""
    best = np.inf
    for s in range(0, len(Y), 500):
        d = np.abs(Y[s:s + 500, None, :] - Y[None, :, :]).max(axis=2)
        best = min(best, d[d > 0].min())
    return float(best)


_cases, _oracle = {}, {}


def case_data(case):
    """Per reference map: Y and the queries (made once, shared)."""
    if case not in _cases:
        Y = ref_map3(case)
        ext = float((Y.max(axis=0) - Y.min(axis=0)).max())
        assert min_chebyshev(Y) > 1e-5 * ext   # no key ties at 21 levels per axis
        _cases[case] = (Y, queries3(Y))
    return _cases[case]


def oracle_queries(case, theta):
    """The oracle's answer for all queries of the case (computed once, shared, left unchanged)."""
    if (case, theta) not in _oracle:
        Y, Q = case_data(case)
        Fo, zo = O.repulsion3_queries(Y, theta, Q)
        Fo.setflags(write=False)
        zo.setflags(write=False)
        _oracle[(case, theta)] = (Fo, zo)
    return _oracle[(case, theta)]


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
def test_foreign_queries3_match_oracle(ctx, case, theta):
    Y, Q = case_data(case)
    Fo, zo = oracle_queries(case, theta)
    F, z = ctx.repulsionQueries(Y, theta, Q)
    assert F.shape == (len(Q), 3) and z.shape == (len(Q),)
    check_against_oracle(F, z, Fo, zo)
    for m in (1, 65):   # one lane; one full wave and a single lane of the next
        Fm, zm = ctx.repulsionQueries(Y, theta, Q[700:700 + m])
        check_against_oracle(Fm, zm, Fo[700:700 + m], zo[700:700 + m])


@pytest.mark.parametrize("theta", [0.0, 0.25, 0.5])
def test_foreign_queries3_duplicates_above_a_chain(ctx, theta):
    """Copies of one point inserted before and after its cell chain came to be:
    the reference re-inserts a splitting leaf's point once, so the top cell of
    the chain around the tight cluster counts one copy more than the cells
    below it (rows 0 and 1 precede the first other point, row 50 precedes the
    cluster's other members, rows 390..394).  Same bound as above."""
    rng = np.random.default_rng(31)
    Y = rng.normal(size=(400, 3))
    Y -= Y.mean(axis=0)
    Y[[1, 50]] = Y[0]
    Y[390:395] = Y[0] + rng.normal(size=(5, 3)) * 1e-3
    ext = float((Y.max(axis=0) - Y.min(axis=0)).max())
    assert min_chebyshev(Y) > 1e-5 * ext
    Q = np.concatenate([rng.normal(size=(300, 3)), Y[0] + rng.normal(size=(150, 3)) * 0.5,
                        Y[0] + rng.normal(size=(50, 3)) * 1e-2, Y[[0, 392]]])
    Fo, zo = O.repulsion3_queries(Y, theta, Q)
    F, z = ctx.repulsionQueries(Y, theta, Q)
    check_against_oracle(F, z, Fo, zo)


def test_offcentre_map_has_points_outside_the_root():
    """The case is there for map points that are queries only: outside Cell(0, 0, 0, W)."""
    Y, _ = case_data("offcentre")
    W = float((Y.max(axis=0) - Y.min(axis=0)).max())
    assert np.count_nonzero(np.abs(Y).max(axis=1) > W) > 0


# ------------------------------------------------------ B: batch independence
@pytest.mark.parametrize("case,theta", [("s1", 0.5), ("dups", 0.25)])
def test_repulsion_queries3_batch_independent(ctx, case, theta):
    Y, Q = case_data(case)
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
def test_members_as_queries3_match_member_path(theta):
    Y, _ = case_data("s1")
    with T.Context(0) as c:
        c.set_option("near_tol3_early", 0)   # the member path's near-exact test and moments off
        c.set_option("oct_moments", 0)
        Fm, zm = c.repulsion(Y, theta)
        F, z = c.repulsionQueries(Y, theta, Y)
    check_against_oracle(F, z, Fm, zm)


# --------------------------------------------- D, E, F, G: the transform input
class XInput3:
    """n = 2000 map points in five blobs (one triple of coincident points),
    m = 300 new points with their 30 nearest map points and P at perplexity 10."""

    def __init__(self, ctx):
        rng = np.random.default_rng(7)
        n, m, k = 2000, 300, 30
        centres = rng.normal(size=(5, 3)) * 12.0
        Yr = centres[rng.integers(0, 5, n)] + rng.normal(size=(n, 3)) * 2.0
        Yr -= Yr.mean(axis=0)
        Yr[[700, 701]] = Yr[17]
        hidden = Yr[rng.integers(0, n, m)] + rng.normal(size=(m, 3)) * 0.7
        d2 = ((hidden[:, None, :] - Yr[None, :, :]) ** 2).sum(axis=2)
        col = np.argsort(d2, axis=1, kind="stable")[:, :k].astype(np.int32)
        dist = np.take_along_axis(d2, col.astype(np.int64), axis=1)
        self.n, self.m, self.k = n, m, k
        self.Yr = np.ascontiguousarray(Yr)
        self.rp = np.arange(0, m * k + 1, k, dtype=np.int64)
        self.col = np.ascontiguousarray(col.ravel())
        self.P = ctx.pairwiseAffinities(self.rp, dist.ravel(), 10.0)
        self.prm = default_params(n_components=3, iterations=110, theta=0.5, learning_rate=1.0)


@pytest.fixture(scope="module")
def xin(ctx):
    return XInput3(ctx)


def init_loop(xin):
    Y0 = np.zeros((xin.m, 3))
    for i in range(xin.m):
        acc = [0.0, 0.0, 0.0]
        for e in range(xin.rp[i], xin.rp[i + 1]):
            p, j = float(xin.P[e]), xin.col[e]
            for c in range(3):
                acc[c] = acc[c] + p * float(xin.Yr[j, c])
        Y0[i] = acc
    return Y0


def test_transform_init3_is_sequential_weighted_mean(ctx, xin):
    Y0 = ctx.transformInit(xin.rp, xin.col, xin.P, xin.Yr)
    assert Y0.shape == (xin.m, 3)
    assert np.array_equal(Y0, init_loop(xin))


def schedule(prm, t):
    n1 = min(prm.iterations, 20)
    n2 = min(prm.iterations - n1, 81)
    return (prm.early_exaggeration if t <= n1 + n2 else 1.0,
            prm.initial_momentum if t <= n1 else prm.final_momentum)


def oracle_terms(xin, Y, ex):
    """rep, z from the oracle octree; attraction and loss terms by numpy in CSR order."""
    rep, z = O.repulsion3_queries(xin.Yr, xin.prm.theta, Y)
    col = xin.col.reshape(xin.m, xin.k)
    pe = ex * xin.P.reshape(xin.m, xin.k)
    d = Y[:, None, :] - xin.Yr[col]
    q = 1.0 / (1.0 + ((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]))
    s = pe * q
    attr = np.zeros((xin.m, 3))
    for e in range(xin.k):   # sequential over a row's entries
        for c in range(3):
            attr[:, c] = attr[:, c] + s[:, e] * d[:, e, c]
    grad = attr - rep / z[:, None]
    terms = pe * np.log(pe / (q / z[:, None]))
    return grad, terms


CHECKED = (1, 2, 20, 21, 101, 102, 110)


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
        if t in CHECKED or t % 10 == 0:
            pre[t] = state()
        ctx.dev_transform_step(t)
        if t in CHECKED:
            post[t] = state()
    final = state()
    return pre, post, final, ctx.dev_transform_losses()


@pytest.mark.parametrize("t", CHECKED)
def test_transform3_step_matches_oracle_step(xin, stepped, t):
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


def test_transform3_losses_match_formula(xin, stepped):
    pre, _, _, losses = stepped
    assert sorted(losses) == list(range(10, 111, 10))
    for t, got in losses.items():
        ex, _ = schedule(xin.prm, t)
        _, terms = oracle_terms(xin, pre[t][0], ex)
        print("t = %d: loss %.12g, numpy %.12g" % (t, got, terms.sum()))
        assert abs(got - terms.sum()) <= 1e-9 * np.abs(terms).sum()


# ---------------------------------------------------------- G: consistency
def host_transform(ctx, xin, rows, iterations):
    """tsne_transform_c on the new points `rows` (all iterations in one call)."""
    k = xin.k
    rp = np.arange(0, len(rows) * k + 1, k, dtype=np.int64)
    col = np.ascontiguousarray(xin.col.reshape(-1, k)[rows].ravel())
    P = np.ascontiguousarray(xin.P.reshape(-1, k)[rows].ravel())
    Y = ctx.transformInit(rp, col, P, xin.Yr)
    upd, gains = np.zeros_like(Y), np.ones_like(Y)
    prm = default_params(n_components=3, iterations=iterations, theta=0.5, learning_rate=1.0)
    losses = ctx.transform(xin.Yr, rp, col, P, Y, upd, gains, prm)
    return Y, upd, gains, losses


@pytest.fixture(scope="module")
def base40(ctx, xin):
    """40 iterations on the full batch with the default options (made once, left unchanged)."""
    return host_transform(ctx, xin, np.arange(xin.m), 40)


def test_transform3_one_call_equals_stepping(ctx, xin, stepped):
    _, _, (Ys, us, gs), losses = stepped
    Y, upd, gains, hl = host_transform(ctx, xin, np.arange(xin.m), 110)
    assert Y.shape == (xin.m, 3)
    assert np.array_equal(Y, Ys) and np.array_equal(upd, us) and np.array_equal(gains, gs)
    assert hl == losses


def test_transform3_batch_independent(ctx, xin, base40):
    Y, upd, gains, _ = base40
    sub = np.random.default_rng(9).permutation(xin.m)[:70]
    Ys, us, gs, _ = host_transform(ctx, xin, sub, 40)
    assert np.array_equal(Ys, Y[sub]) and np.array_equal(us, upd[sub]) and np.array_equal(gs, gains[sub])


@pytest.mark.parametrize("option,value", [("transform_resort", 0), ("transform_resort", 1), ("transform_split", 1)])
def test_transform3_layout_options_change_no_bit(xin, base40, option, value):
    """How often the new points are re-sorted, and the walk and the update as
    two launches instead of one, change which lanes and launches do the work,
    not a bit of the result (the canonical order)."""
    with T.Context(0) as c:
        c.set_option(option, value)
        other = host_transform(c, xin, np.arange(xin.m), 40)
    for a, b in zip(base40[:3], other[:3]):
        assert np.array_equal(a, b)
    assert base40[3] == other[3]


# ---------------------------------------------------------- H: end to end
def test_transform3_end_to_end_places_rows_near_their_neighbours(ctx):
    """tsne_amd.transform on 2000 x 16 GMM rows.  The map is a linear one (the
    three leading principal axes of the reference rows, scaled to t-SNE's usual
    extent): cheap, deterministic, and neighbours in X are neighbours on it."""
    rng = np.random.default_rng(41)
    n, m, d = 1700, 300, 16
    centres = rng.normal(size=(6, d)) * 4.0
    X = centres[rng.integers(0, 6, n + m)] + rng.normal(size=(n + m, d))
    X_ref, X_new = X[:n], X[n:]
    Xc = X_ref - X_ref.mean(axis=0)
    _, _, vt = np.linalg.svd(Xc, full_matrices=False)
    Y_ref = Xc @ vt[:3].T
    Y_ref *= 30.0 / np.abs(Y_ref).max()
    Y_new, losses = T.transform(ctx, X_ref, Y_ref, X_new, k=30, perplexity=10.0)
    assert Y_new.shape == (m, 3) and np.all(np.isfinite(Y_new))
    assert sorted(losses) == list(range(10, 301, 10))
    d2 = ((X_new[:, None, :] - X_ref[None, :, :]) ** 2).sum(axis=2)
    target = Y_ref[np.argsort(d2, axis=1)[:, :5]].mean(axis=1)
    placed = np.linalg.norm(Y_new - target, axis=1).mean()
    shuffled = np.linalg.norm(Y_new[rng.permutation(m)] - target, axis=1).mean()
    print("mean distance to the 5 nearest reference rows' map position: %.3f (permuted: %.3f)" % (placed, shuffled))
    assert placed < shuffled


# -------------------------------------------------------- I: arguments
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_transform3_column_counts_must_match_the_map(ctx, xin):
    Y3, Q3 = case_data("s1")
    with pytest.raises(ValueError):
        ctx.repulsionQueries(Y3, 0.5, Q3[:10, :2])
    with pytest.raises(ValueError):
        ctx.repulsionQueries(Y3[:, :2], 0.5, Q3[:10])
    Y = ctx.transformInit(xin.rp, xin.col, xin.P, xin.Yr)
    prm = default_params(n_components=3, iterations=5)
    for bad in ("Y", "upd", "gains"):
        arrs = dict(Y=Y.copy(), upd=np.zeros_like(Y), gains=np.ones_like(Y))
        arrs[bad] = np.ascontiguousarray(arrs[bad][:, :2])
        with pytest.raises(ValueError):
            ctx.transform(xin.Yr, xin.rp, xin.col, xin.P, arrs["Y"], arrs["upd"], arrs["gains"], prm)


def test_transform3_argument_errors(ctx, xin):
    L = T.lib()
    Y = ctx.transformInit(xin.rp, xin.col, xin.P, xin.Yr)
    upd, gains = np.zeros_like(Y), np.ones_like(Y)
    # c = 4: unsupported
    Y4 = np.zeros((50, 4))
    F4, z4 = np.zeros((5, 4)), np.zeros(5)
    assert L.tsne_repulsion_queries_c(ctx.handle, _p(Y4), 50, 4, 0.5, _p(Y4), 5, _p(F4), _p(z4)) == -4
    prm4 = default_params(n_components=4, iterations=5)
    rc = L.tsne_transform_c(ctx.handle, C.byref(prm4), _p(xin.Yr), xin.n, _p(xin.rp), _p(xin.col), _p(xin.P), xin.m,
                            _p(Y), _p(upd), _p(gains), None, None, 0, None)
    assert rc == -4
    # a row without entries
    rp = xin.rp.copy()
    rp[4:] -= xin.k                                 # row 3 has no entries
    with pytest.raises(T.TsneError) as e:
        ctx.transformInit(rp, xin.col[:rp[-1]], xin.P[:rp[-1]], xin.Yr)
    assert e.value.status == -1
    out = np.zeros((xin.m, 3))
    assert L.tsne_transform_init_c(ctx.handle, _p(rp), _p(xin.col), _p(xin.P), xin.m, _p(xin.Yr), xin.n, 3,
                                   _p(out)) == -1
    # a column index out of range
    prm = default_params(n_components=3, iterations=5)
    for bad in (-1, xin.n):
        col = xin.col.copy()
        col[77] = bad
        with pytest.raises(T.TsneError) as e:
            ctx.transform(xin.Yr, xin.rp, col, xin.P, Y, upd, gains, prm)
        assert e.value.status == -1
        with pytest.raises(T.TsneError) as e:
            ctx.transformInit(xin.rp, col, xin.P, xin.Yr)
        assert e.value.status == -1
    # m = 0 is a no-op
    assert L.tsne_transform_c(ctx.handle, C.byref(prm), _p(xin.Yr), xin.n, None, None, None, 0, None, None, None,
                              None, None, 0, None) == 0
    assert L.tsne_repulsion_queries_c(ctx.handle, _p(xin.Yr), xin.n, 3, 0.5, None, 0, None, None) == 0
    assert L.tsne_transform_init_c(ctx.handle, None, None, None, 0, _p(xin.Yr), xin.n, 3, None) == 0


def test_c_entry_points_with_c2_equal_the_old_ones(ctx):
    """tsne_repulsion_queries_c and tsne_transform_c with c = 2 are the 2-D path, bit for bit."""
    L = T.lib()
    Y2 = ref_map2("s1")
    Q2 = queries2(Y2)
    F, z = ctx.repulsionQueries(Y2, 0.5, Q2)
    Fc, zc = np.zeros_like(F), np.zeros_like(z)
    assert L.tsne_repulsion_queries_c(ctx.handle, _p(Y2), len(Y2), 2, 0.5, _p(Q2), len(Q2), _p(Fc), _p(zc)) == 0
    assert np.array_equal(F, Fc) and np.array_equal(z, zc)

    x2 = XInput2(ctx)
    prm = default_params(iterations=40, theta=0.5, learning_rate=1.0)
    Y0 = ctx.transformInit(x2.rp, x2.col, x2.P, x2.Yr)
    Y0c = np.zeros_like(Y0)
    assert L.tsne_transform_init_c(ctx.handle, _p(x2.rp), _p(x2.col), _p(x2.P), x2.m, _p(x2.Yr), x2.n, 2,
                                   _p(Y0c)) == 0
    assert np.array_equal(Y0, Y0c)
    Y, upd, gains = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    losses = ctx.transform(x2.Yr, x2.rp, x2.col, x2.P, Y, upd, gains, prm)
    Yc, uc, gc = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    keys, vals, nl = np.zeros(5, dtype=np.int32), np.zeros(5), C.c_int32()
    rc = L.tsne_transform_c(ctx.handle, C.byref(prm), _p(x2.Yr), x2.n, _p(x2.rp), _p(x2.col), _p(x2.P), x2.m, _p(Yc),
                            _p(uc), _p(gc), _p(keys), _p(vals), 5, C.byref(nl))
    assert rc == 0
    assert np.array_equal(Y, Yc) and np.array_equal(upd, uc) and np.array_equal(gains, gc)
    assert dict(zip(keys[:nl.value].tolist(), vals[:nl.value].tolist())) == losses
