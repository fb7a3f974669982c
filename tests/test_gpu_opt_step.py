"""One iteration of the optimizer as tsne_dev_opt_step runs it, from a given
state, against the oracle on the same inputs; and the first committed tests
of attract_tiles3 (option "attract_tiles3" 1).

A step is: the (exaggeration, momentum) of iteration t picked from the
three-phase schedule, an attraction kernel (attract_tiles / attract_rows in
2-D; attract3 / attract_tiles3 in 3-D), combine_update / combine_update3, the
mean, the centring and the loss record.  tsne_dev_opt_setup takes any Y, upd
and gains and tsne_dev_opt_step takes t, so setup -> one step -> sync gives a
state that is compared with O.gradient / O.gradient3, O.update and O.center of
the same inputs; rounding is the only difference (a whole trajectory instead
amplifies it: the spreads in profiles/r11_opt_step_bounds.txt).

The reference runs at theta 0 (exact repulsion on both sides), embeddings at
scale 5.0 (the regime of every theta-0 oracle comparison of the suite; the
near-exact moment paths are not engaged there).

Bounds (none tuned on the code under test):
  tol_g   the gradient's: 3-D 1e-12 max|g_o| (test_gradient3_matches_oracle at
          theta 0); 2-D max(1e-12, 10 d) max|g_o|, d = D2 below the largest
          relative deviation of tsne_gradient at theta 0 from the oracle on
          this file's 2-D states, measured once on an MI355X: d = 1.2e-15
          (`PYTHONPATH=tsne-flink_amd python tests/test_gpu_opt_step.py`;
          profiles/r11_opt_step_bounds.txt), so the bound is the floor 1e-12;
  upd     |u1 - u_ref| <= lr gain_ref tol_g + 4 ulp(|u_ref|) elementwise (the
          gradient is the only inexact input);
  Y       the same + n 2^-53 max|Ynew| (two summation orders of the mean);
  gains   bit-equal, given min|g_o| > 1e-9 max|g_o| (asserted on the oracle
          alone first: no component's sign is inside the gradient's bound);
  Z, loss 1e-9 relative (check_opt_step, test_tiled_attraction_matches_oracle).
"""
import functools

import numpy as np
import pytest
import torch

import oracle_ctypes as O
import tsne_amd as T
from test_gpu_attract_stream import hub_problem, knn_problem, rows_problem
from test_gpu_configs import check_opt_step
from tsne_amd.api import default_params

pytestmark = pytest.mark.gpu
THREADS = 16
MIN_GAIN = 0.01
# the largest |g_gpu - g_o| / max|g_o| of tsne_gradient (2-D, theta 0) over
# states_2d() on an MI355X: 1.2e-15 (profiles/r11_opt_step_bounds.txt), so the
# 2-D gradient bound is the floor 1e-12, the 3-D one
D2 = 1.2e-15
TOL_G = {2: max(1e-12, 10.0 * D2), 3: 1e-12}   # x max|g_o|


def schedule(t, T_):
    """(exaggeration, momentum) of iteration t of T_: TsneHelpers.scala:396-430,
    restated."""
    n1 = min(T_, 20)
    n2 = min(T_ - n1, 81)
    return (4.0 if t <= n1 + n2 else 1.0), (0.5 if t <= n1 else 0.8)


def _step(c, P, state, t, params):
    """dev_opt_setup on torch copies of `state`, ONE dev_opt_step(t), dev_opt_sync."""
    dev = torch.device("cuda", 0)
    n = state[0].shape[0]
    Pd = (torch.from_numpy(np.ascontiguousarray(P[0], dtype=np.int64)).to(dev),
          torch.from_numpy(np.ascontiguousarray(P[1], dtype=np.int32)).to(dev),
          torch.from_numpy(np.ascontiguousarray(P[2], dtype=np.float64)).to(dev))
    Y, u, g = (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).copy()).to(dev) for x in state)
    c.dev_opt_setup(params, *Pd, n, Y, u, g)
    c.dev_opt_step(t)
    c.dev_opt_sync()
    c.synchronize()
    losses = c.dev_opt_losses()
    return dict(Y=Y.cpu().numpy(), u=u.cpu().numpy(), g=g.cpu().numpy(), Z=c.dev_opt_last_z(), losses=losses,
                loss=losses.get(t), kernel=c.counter("opt.attract_kernel"), cfg=c.counter("opt.attract_cfg"))


def one_step(opts, P, state, t, params, full=False):
    """A fresh context with `opts`, setup from state = (Y0, u0, g0), one step t
    -> (Y1, u1, g1, Z, loss of t or None, the attraction kernel's id); full:
    _step's dict instead (the whole loss dict and the tile configuration too)."""
    with T.Context(0) as c:
        for k, v in opts.items():
            c.set_option(k, v)
        r = _step(c, P, state, t, params)
    return r if full else (r["Y"], r["u"], r["g"], r["Z"], r["loss"], r["kernel"])


def oracle_gradient(P, Y0, metric, ex):
    fn = O.gradient if Y0.shape[1] == 2 else O.gradient3
    return fn(*P, Y0, 0.0, metric, exaggeration=ex, want_loss=True, threads=THREADS)


def reference(P, state, t, T_, metric, lr, r=None):
    """The oracle's iteration t from `state` at theta 0 -> dict; `r` a shared
    O.gradient result of the same (P, Y0, metric, exaggeration)."""
    ex, mom = schedule(t, T_)
    Y0, u0, g0 = state
    r = r or oracle_gradient(P, Y0, metric, ex)
    g_o = r["grad"]
    gmax = np.abs(g_o).max()
    # the condition for bit-equal gains: no component's sign within the gradient's bound
    assert np.abs(g_o).min() > 1e-9 * gmax, ("gradient band", np.abs(g_o).min() / gmax)
    Y, u, g = Y0.copy(), u0.copy(), g0.copy()
    O.update(np.ascontiguousarray(g_o), Y, u, g, MIN_GAIN, mom, lr)
    Ynew = Y.copy()
    O.center(Y)
    return dict(Y=Y, Ynew=Ynew, u=u, g=g, grad=g_o, gmax=gmax, Z=r["Z"], loss=r["loss"], ex=ex, mom=mom)


def check_state(got, ref, lr, t, what=""):
    """got: _step's dict; ref: reference()'s.  Figures first, then the bounds of
    the module docstring."""
    n, c = ref["Y"].shape
    tol_g = TOL_G[c] * ref["gmax"]
    bu = lr * ref["g"] * tol_g + 4.0 * np.spacing(np.abs(ref["u"]))
    by = bu + n * 2.0 ** -53 * np.abs(ref["Ynew"]).max()
    du, dy = np.abs(got["u"] - ref["u"]), np.abs(got["Y"] - ref["Y"])
    zrel = abs(got["Z"] - ref["Z"]) / ref["Z"]
    print("%s t=%d c=%d: gains differ %d, max du/bound %.3e, max dY/bound %.3e, Z rel %.3e"
          % (what, t, c, int((got["g"] != ref["g"]).sum()), (du / bu).max(), (dy / by).max(), zrel), end="")
    if t % 10 == 0:
        print(", loss rel %.3e" % (abs(got["loss"] - ref["loss"]) / abs(ref["loss"])))
    else:
        print()
    assert np.array_equal(got["g"], ref["g"]), (what, t, "gains", int((got["g"] != ref["g"]).sum()))
    assert (du <= bu).all(), (what, t, "upd", float((du / bu).max()))
    assert (dy <= by).all(), (what, t, "Y", float((dy / by).max()))
    assert zrel <= 1e-9, (what, t, "Z", got["Z"], ref["Z"])
    if t % 10 == 0:
        assert sorted(got["losses"]) == [t], (what, t, got["losses"])
        assert abs(got["loss"] - ref["loss"]) <= 1e-9 * abs(ref["loss"]), (what, t, got["loss"], ref["loss"])
    else:
        assert got["losses"] == {}, (what, t, got["losses"])


def random_state(n, c, seed):
    """Y at scale 5.0; upd of both signs; gains in [-0.5, 4) (the few below
    the minimum reach the clamp from both branches of the rule)."""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, c)) * 5.0, rng.normal(size=(n, c)) * 0.5, rng.uniform(-0.5, 4.0, size=(n, c))


# ------------------------------------------------------------ shared problems
@functools.lru_cache(maxsize=None)
def problem(name):
    if name == "knn1000":
        return knn_problem(1000, 12, seed=111)
    if name == "knn600":
        return knn_problem(600, 12, seed=112)
    if name == "hub6000":
        return hub_problem(6000)
    if name.startswith("knn"):                       # "knn<n>k<k>"
        n, k = (int(v) for v in name[3:].split("k"))
        return knn_problem(n, k, seed=83 + n)          # (seeds without an underflowed P entry: the loss is finite)
    if name == "rows":   # 1 .. 9 entries mixed in each of four 64-row slices, and a slice of one-entry rows
        lengths = [[1, 2, 3, 4, 5, 7, 8, 9][i % 8] for i in range(256)] + [1] * 64
        return rows_problem(lengths, seed=114)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def shared_gradient(name, c, metric, ex, seed):
    """One oracle gradient per (problem, state, metric, exaggeration), left unchanged."""
    P = problem(name)
    Y0 = random_state(len(P[0]) - 1, c, seed)[0]
    return oracle_gradient(P, Y0, metric, ex)


# ------------------------------------------------- 1. schedule edges, 2-D / 3-D
EDGES = [(1000, t) for t in (1, 20, 21, 100, 101, 102, 110)] + [(15, 10), (15, 15), (21, 20), (21, 21),
                                                                  (50, 21), (50, 50)]


@pytest.mark.parametrize("c", [2, 3])
@pytest.mark.parametrize("lr", [1000.0, 200.0])
@pytest.mark.parametrize("T_,t", EDGES)
def test_step_at_schedule_edges(c, lr, T_, t):
    """Iteration t of a T_-iteration run next to each edge of the schedule
    (n1 = min(T, 20) of momentum 0.5, n1 + min(T - n1, 81) of exaggeration 4),
    stepped directly after setup from a random state: a wrong momentum or
    exaggeration moves upd far outside the bound (upd and gains of both signs
    and of order 1).  The loss dict holds exactly {t} at t % 10 == 0."""
    P = problem("knn1000")
    state = random_state(1000, c, 120 + c)
    prm = default_params(iterations=T_, theta=0.0, learning_rate=lr, n_components=c)
    ref = reference(P, state, t, T_, "sqeuclidean", lr,
                    r=shared_gradient("knn1000", c, "sqeuclidean", schedule(t, T_)[0], 120 + c))
    got = one_step({}, P, state, t, prm, full=True)
    assert got["kernel"] == (1 if c == 2 else 2)
    check_state(got, ref, lr, t, "T=%d lr=%g" % (T_, lr))


# ------------------------------------------- 2. the gains rule on crafted state
U_VALS = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-6, -1e-6, 1e-2, -1e-2])
G_VALS = np.array([0.01, 0.0125, 0.012, 1.0, 7.3])


@pytest.mark.parametrize("c", [2, 3])
@pytest.mark.parametrize("n,t", [(255, 1), (256, 21), (257, 102)])
def test_gains_rule_on_crafted_state(n, t, c):
    """updateEmbedding's rule gain' = max(same sign ? 0.8 gain : gain + 0.2,
    0.01), "same sign" being (g > 0) == (upd > 0), on upd in {+0, -0, +-5e-324,
    +-1e-6, +-1e-2} x gains in {0.01, 0.0125, 0.012 (0.8 x below, at and below
    the minimum), 1, 7.3} x both signs of the gradient, every combination
    present; n around the 256-row blocks of combine_update and of the mean's
    partials.  Through the optimizer's step (combine_update / combine_update3,
    mean, centring) and, with the oracle's gradient, through
    tsne_update_embedding + tsne_center_embedding (update_kernel, center_apply):
    those two bit-equal to O.update for upd and gains, Y within the mean's bound."""
    name = "knn%dk12" % n
    P = problem(name)
    lr, T_ = 200.0, 1000
    ex, mom = schedule(t, T_)
    r = shared_gradient(name, c, "sqeuclidean", ex, 130 + c)
    Y0 = random_state(n, c, 130 + c)[0]
    # deal the 40 (upd, gains) pairs over the components of each gradient sign
    pos = (r["grad"] > 0.0).ravel()
    combo = np.zeros(n * c, dtype=np.int64)
    for s in (False, True):
        combo[pos == s] = np.arange((pos == s).sum()) % 40
    u0 = U_VALS[combo % 8].reshape(n, c).copy()
    g0 = G_VALS[combo // 8].reshape(n, c).copy()
    seen = {(float(abs(a)), bool(np.signbit(a)), float(b), bool(s)) for a, b, s in zip(u0.ravel(), g0.ravel(), pos)}
    want = {(float(abs(a)), bool(np.signbit(a)), float(b), s) for a in U_VALS for b in G_VALS for s in (False, True)}
    assert seen == want and len(want) == 80
    state = (Y0, u0, g0)
    ref = reference(P, state, t, T_, "sqeuclidean", lr, r=r)
    prm = default_params(iterations=T_, theta=0.0, learning_rate=lr, n_components=c)
    got = one_step({}, P, state, t, prm, full=True)
    check_state(got, ref, lr, t, "crafted n=%d" % n)
    # the host operators on the oracle's own gradient: nothing inexact but the mean
    Y, u, g = Y0.copy(), u0.copy(), g0.copy()
    with T.Context(0) as ctx:
        ctx.updateEmbedding(r["grad"], Y, u, g, MIN_GAIN, mom, lr)
        assert np.array_equal(u, ref["u"]) and np.array_equal(g, ref["g"]), "update_kernel"
        assert np.array_equal(Y, ref["Ynew"]), "update_kernel Y"
        ctx.centerEmbedding(Y)
    dy = np.abs(Y - ref["Y"]).max()
    print("centerEmbedding: max dY %.3e, bound %.3e" % (dy, n * 2.0 ** -53 * np.abs(ref["Ynew"]).max()))
    assert dy <= n * 2.0 ** -53 * np.abs(ref["Ynew"]).max()


# --------------------------------------- 3. attract_tiles3, small configuration
SHAPES3 = {   # name -> (problem, context options)
    "hub6000": ("hub6000", {}),            # wide slices; rows of > 4000 entries over two 4096-label windows
    "n4097": ("knn4097k12", {}),           # the last window holds one label: the window copy's odd tail
    "n4098": ("knn4098k12", {}),           # ... two labels
    "n63": ("knn63k5", {}),                # one partial slice, every other wave without one
    "n70": ("knn70k5", {}),                # one slice and a partial one
    "rows": ("rows", {"graph_order": 0}),  # widths 1 .. 9 mixed in a slice, in the original label order
}


@pytest.mark.parametrize("metric", ["sqeuclidean", "euclidean", "cosine"])
@pytest.mark.parametrize("shape", list(SHAPES3))
def test_attract_tiles3_small_configuration(shape, metric):
    """attract_tiles3 (512-row blocks: configuration 5) and attract3 on the same
    inputs, each against the theta-0 reference (not bit-equal to each other:
    the summation orders differ), at t = 109 (a non-loss launch on the side
    stream) and t = 110 (a LOSS launch after Z)."""
    name, opts = SHAPES3[shape]
    P = problem(name)
    n = len(P[0]) - 1
    lr, T_ = 200.0, 1000
    state = random_state(n, 3, 140)
    prm = default_params(iterations=T_, theta=0.0, learning_rate=lr, n_components=3, metric=metric)
    r = shared_gradient(name, 3, metric, 1.0, 140)
    for t in (109, 110):
        ref = reference(P, state, t, T_, metric, lr, r=r)
        tiled = one_step({**opts, "attract_tiles3": 1}, P, state, t, prm, full=True)
        assert tiled["kernel"] == 3 and tiled["cfg"] == 5, (tiled["kernel"], tiled["cfg"])
        check_state(tiled, ref, lr, t, "%s %s attract_tiles3" % (shape, metric))
        rows = one_step(opts, P, state, t, prm, full=True)
        assert rows["kernel"] == 2 and rows["cfg"] == -1, (rows["kernel"], rows["cfg"])
        check_state(rows, ref, lr, t, "%s %s attract3" % (shape, metric))


# ------------------------ 4. attract_tiles3 with more than one slice per tile
def _ceil_div(a, b):
    return -(-a // b)


def layout3(n, cus):
    """at_cfg / attract_layout_build for n rows of a 3-D run on `cus` CUs ->
    (configuration, rows per block)."""
    cfg = 4 if _ceil_div(n, 2048) >= cus - cus // 16 else 5
    rbs = min(2048 if cfg == 4 else 512, _ceil_div(_ceil_div(n, cus), 64) * 64)
    return cfg, rbs


def big_rows_problem(n, seed, band):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 17, size=n)
    lengths[rng.integers(0, n, 5)] = 3000 if band is None else 2000   # (a banded row has 2 band candidates)
    return rows_problem(lengths, seed=seed + 1, band=band)


def run_big(n, cfg_want, metric, P, opts, seed):
    """One step at t = 109 and t = 110 of T = 1000 at theta 0.5, each checked by
    check_opt_step: every row's attraction against O.attraction3_rows at 1e-6 of
    the row's scale, 64 gradient rows, the gains, the centring, the loss at 1e-9."""
    lr, T_, theta = 200.0, 1000, 0.5
    state = random_state(n, 3, seed)
    prm = default_params(iterations=T_, theta=theta, learning_rate=lr, n_components=3, metric=metric)
    with T.Context(0) as c:
        for k, v in {**opts, "attract_tiles3": 1}.items():
            c.set_option(k, v)
        for t in (109, 110):
            got = _step(c, P, state, t, prm)
            assert got["kernel"] == 3 and got["cfg"] == cfg_want, (got["kernel"], got["cfg"])
            assert sorted(got["losses"]) == ([t] if t % 10 == 0 else [])
            check_opt_step(c, P, state, (got["Y"], got["u"], got["g"]), got["Z"], t, T_, theta, metric, n // 2, 64,
                           c=3, loss_gpu=got["loss"], lr=lr, all_rows=True, key="attract_tiles3 cfg %d" % cfg_want)


@pytest.mark.parametrize("metric", ["sqeuclidean", "euclidean", "cosine"])
def test_attract_tiles3_blocks_of_192_rows(metric):
    """(a) configuration 5 with row blocks of >= 192 rows (three slices a
    block): n = 156 CUs + 64 (40,000 on 256 CUs), rows of 1 .. 16 entries and a
    few of 3000, columns over every window."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 156 * cus + 64
    cfg, rbs = layout3(n, cus)
    assert cfg == 5 and rbs >= 192, (n, cus, cfg, rbs)
    run_big(n, 5, metric, big_rows_problem(n, 150, None), {}, 151)


@pytest.mark.parametrize("band", [None, 1024])
def test_attract_tiles3_2048_row_configuration(band):
    """(b) configuration 4 (ATCfg3D, up to 2048-row blocks): the smallest n with
    ceil(n / 2048) >= CUs - CUs / 16 (489,473 on 256 CUs).  band None: the
    columns of a row anywhere, so its tiles spread over every window (few rows
    of a block meet in one tile).  band 1024 in the original label order
    ("graph_order" 0): a block's rows meet in one or two windows, so a tile
    holds more 64-row slices than the workgroup has waves and a wave takes a
    second slice of it (the prefetch of slice s + WAVES) -- asserted on P."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2048 * (cus - cus // 16 - 1) + 1
    cfg, rbs = layout3(n, cus)
    assert cfg == 4 and layout3(n - 1, cus)[0] == 5, (n, cus)
    P = big_rows_problem(n, 160, band)
    opts = {}
    if band is not None:
        opts = {"graph_order": 0}
        row = np.repeat(np.arange(n), np.diff(P[0]))
        tile_row = np.unique((row // rbs * _ceil_div(n, 4096) + P[1] // 4096) * rbs + row % rbs)
        rows_in_tile = np.unique(tile_row // rbs, return_counts=True)[1]
        assert rows_in_tile.max() > 16 * 64, rows_in_tile.max()   # more slices than the 16 waves
    run_big(n, 4, "sqeuclidean", P, opts, 161)


# --------------------------------------------- 5. short schedules end to end
def oracle_run(P, Y0, T_, c):
    Y, u, g = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    fn = O.optimize if c == 2 else O.optimize3
    lo = fn(*P, Y, u, g, learning_rate=1000.0, iterations=T_, theta=0.0, threads=THREADS)
    return Y, lo


def oracle_spread(P, Y0, T_, c):
    """s: the largest relative difference of the oracle's own Y after T_
    iterations from Y0 (1 + 1e-15 xi), xi standard normal, over 8 seeds."""
    Yb, lo = oracle_run(P, Y0, T_, c)
    s = 0.0
    for seed in range(1, 9):
        Yp, _ = oracle_run(P, Y0 * (1.0 + 1e-15 * np.random.default_rng(seed).normal(size=Y0.shape)), T_, c)
        s = max(s, np.abs(Yp - Yb).max() / np.abs(Yb).max())
    return Yb, lo, s


@pytest.mark.parametrize("c", [2, 3])
@pytest.mark.parametrize("T_", [1, 9, 10, 19, 20, 21])
def test_short_schedules_end_to_end(T_, c):
    """Context.optimize with T below, at and just past n1 = min(T, 20) (so
    n2 = min(T - n1, 81) is 0 or 1): the loss keys are the multiples of 10 up to
    T, the host path is bit-equal to the device path stepped 1 .. T, and Y
    matches the oracle within max(1e-9, 10 s), s the oracle's own spread under a
    1e-15 perturbation of Y0 at that T (computed here on the CPU; ten times it
    because GPU and oracle differ by a handful of roundings per term where the
    probe differs by one).  Measured s: profiles/r11_opt_step_bounds.txt."""
    n = 600
    P = problem("knn600")
    Y0 = np.random.default_rng(170 + c).normal(size=(n, c)) * 5.0
    prm = default_params(iterations=T_, theta=0.0, learning_rate=1000.0, n_components=c)
    Yo, lo, s = oracle_spread(P, Y0, T_, c)
    with T.Context(0) as ctx:
        Yh, uh, gh = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
        lh = ctx.optimize(*P, Yh, uh, gh, prm)
        dev = torch.device("cuda", 0)
        Pd = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in P)
        dY = torch.from_numpy(Y0.copy()).to(dev)
        du, dg = torch.zeros_like(dY), torch.ones_like(dY)
        ctx.dev_opt_setup(prm, *Pd, n, dY, du, dg)
        for t in range(1, T_ + 1):
            ctx.dev_opt_step(t)
        ctx.dev_opt_sync()
        ctx.synchronize()
        ld = ctx.dev_opt_losses()
    rel = np.abs(Yh - Yo).max() / np.abs(Yo).max()
    print("T=%d c=%d: oracle spread s = %.3e, max |Y - Yo| / max |Yo| = %.3e" % (T_, c, s, rel))
    assert sorted(lh) == sorted(lo) == list(range(10, T_ + 1, 10))
    assert np.array_equal(dY.cpu().numpy(), Yh) and np.array_equal(du.cpu().numpy(), uh)
    assert np.array_equal(dg.cpu().numpy(), gh) and ld == lh
    assert rel <= max(1e-9, 10.0 * s), (rel, s)
    for t in lo:
        assert abs(lh[t] - lo[t]) <= max(1e-9, 10.0 * s) * abs(lo[t]), (t, lh[t], lo[t])


# ------------------------------------------------------- the 2-D figure D2
def states_2d():
    """(name, P, Y0, exaggerations) of every 2-D state of this file."""
    yield "knn1000", problem("knn1000"), random_state(1000, 2, 122)[0], (4.0, 1.0)
    for n in (255, 256, 257):
        yield "knn%dk12" % n, problem("knn%dk12" % n), random_state(n, 2, 132)[0], (4.0, 1.0)
    yield "knn600", problem("knn600"), np.random.default_rng(172).normal(size=(600, 2)) * 5.0, (4.0,)


def measure_d2():
    """Prints, per 2-D state, max |g_gpu - g_o| / max |g_o| of tsne_gradient at
    theta 0 against the oracle; D2 above is the largest."""
    worst = 0.0
    with T.Context(0) as ctx:
        for name, P, Y0, exs in states_2d():
            for ex in exs:
                g, _, _ = ctx.gradient(*P, Y0, 0.0, exaggeration=ex)
                g_o = oracle_gradient(P, Y0, "sqeuclidean", ex)["grad"]
                d = np.abs(g - g_o).max() / np.abs(g_o).max()
                worst = max(worst, d)
                print("2-D gradient, theta 0, %s ex=%g: d = %.3e" % (name, ex, d))
    print("largest d = %.3e" % worst)


if __name__ == "__main__":
    measure_d2()
