"""Option bh_chain (bhtree.hip bh_repulsion, DESIGN.md 3 "Off the chain"): the
subtree moments a fused build defers run on a stream of their own beside the
traversal pair, and the narrow groups' moment sums, the hran copy and
narrow_select on the second stream instead of the main one.  Which stream a
kernel runs on changes no operand and no order of additions, so every F, z,
Y, update, gain and loss must keep its bits: arm 1 (the default) is compared
with arm 0 (the earlier order) by np.array_equal, and with itself over two
runs (an ordering hole would show as a difference between runs or arms).

Sizes.  A single call turns every group narrow while its 64-query waves fill
less than half of the chip's wave slots (narrow_fill: fewer than 16 x CUs
waves, 4,096 on 256 CUs), and at most min(waves, 16 x CUs) groups fit the
heavy list (bh_alloc's nar_hmax).  So that narrow and 64-query groups exist
side by side the two single-call inputs have 300,000 points (4,688 waves:
at most 4,096 narrow), not test_gpu_narrow's 40,000 / 20,000; the calls are
compared with each other only, so the size costs no oracle time."""
import functools

import numpy as np
import pytest
import torch

import tsne_amd as T
from tsne_amd.api import default_params
from test_gpu_narrow import clustered

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def single_input(name):
    n = 300_000
    if name == "clustered":   # test_gpu_narrow's blobs, at the scale where the blobs' subtrees are near-exact tiles
        Y, factor = clustered(n, 5) * 1e-3, 0.25
    else:                     # its extent-0.03 embedding with a dense core
        rng = np.random.default_rng(12)
        Y = rng.normal(size=(n, 2)) * 0.03
        Y[: n // 4] *= 0.01
        factor = 0.5
    Y = np.ascontiguousarray(Y)
    Y.setflags(write=False)
    return Y, factor


def single_calls(Y, factor, chain):
    """Four calls on one context (reuse_costs 1): the first selects, the
    second to fourth run narrow groups; (F, z) of the third and fourth and the
    fourth's counters."""
    with T.Context(0) as c:
        c.set_option("bh_chain", chain)
        c.set_option("reuse_costs", 1)
        c.set_option("narrow", factor)
        c.set_option("rep_stats", 1)
        out = [c.repulsion(Y, 0.5) for _ in range(4)]
        stats = {k: c.counter(k) for k in ("bh.narrow_groups", "bh.moment_evals", "bh.narrow_moment_tasks")}
    return out[2], out[3], stats


@pytest.mark.parametrize("name", ["clustered", "small_embedding"])
def test_single_call_repulsion_keeps_its_bits(name):
    Y, factor = single_input(name)
    a3, a4, sa = single_calls(Y, factor, 1)
    b3, b4, sb = single_calls(Y, factor, 1)
    o3, o4, so = single_calls(Y, factor, 0)
    print(name, sa, so)
    waves = (len(Y) + 63) // 64
    assert 0 < sa["bh.narrow_groups"] < waves            # narrow and 64-query groups side by side
    assert sa["bh.moment_evals"] > 0                      # moment_apply had tasks
    assert sa["bh.narrow_moment_tasks"] > 0               # narrow_moment_apply had tasks
    assert sa == sb == so
    for x, y, z in ((a3, b3, o3), (a4, b4, o4)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
        assert np.array_equal(x[0], z[0]) and np.array_equal(x[1], z[1])


def handover(chain):
    """Sizes 20,000 -> 5,000 -> 20,000 (the tree's arrays re-made while a
    selection may still run), then narrow off -> on -> off at one size (the
    nflag fill instead of a selection's): (narrow groups, F, z) per call."""
    big, small = clustered(20_000, 5), clustered(5_000, 6)
    out = []
    with T.Context(0) as c:
        c.set_option("bh_chain", chain)
        c.set_option("reuse_costs", 1)
        c.set_option("narrow", 0.25)
        for Y in (big, big, small, small, big, big):
            F, z = c.repulsion(Y, 0.5)
            out.append((c.counter("bh.narrow_groups"), F, z))
        for factor in (0, 0.25, 0.25, 0, 0, 0.25, 0.25):
            c.set_option("narrow", factor)
            F, z = c.repulsion(big, 0.5)
            out.append((c.counter("bh.narrow_groups"), F, z))
    return out


def test_handover_across_calls():
    a, b, o = handover(1), handover(1), handover(0)
    groups = [r[0] for r in a]
    print(groups)
    # the second call of a size runs narrow groups, the first (fresh arrays) and the calls after "off" none
    assert groups[0] == 0 and groups[1] > 0 and groups[2] == 0 and groups[3] > 0 and groups[4] == 0 and groups[5] > 0
    assert groups[6] == 0 and groups[7] == 0 and groups[8] > 0 and groups[9] == 0 and groups[10] == 0
    assert groups[11] == 0 and groups[12] > 0
    for x, y, z in zip(a, b, o):
        assert x[0] == y[0] == z[0]
        assert np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])
        assert np.array_equal(x[1], z[1]) and np.array_equal(x[2], z[2])


@functools.lru_cache(maxsize=None)
def opt_problem(n):
    from test_gpu_parity import random_problem
    rp, col, val = random_problem(n, 30, seed=23)
    Y0 = np.random.default_rng(4).normal(size=(n, 2)) * 1e-4
    return rp, col, val, Y0


def optimize(n, iterations, chain):
    rp, col, val, Y0 = opt_problem(n)
    p = default_params(iterations=iterations, theta=0.5)
    dev = torch.device("cuda", 0)
    Pd = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rp, col, val))
    with T.Context(0) as c:
        c.set_option("bh_chain", chain)
        c.set_option("narrow", 0.25)
        Y = torch.from_numpy(Y0.copy()).to(dev)
        u, g = torch.zeros_like(Y), torch.ones_like(Y)
        c.dev_opt_setup(p, *Pd, n, Y, u, g)
        used = 0
        for t in range(1, iterations + 1):
            c.dev_opt_step(t)
            if t % 10 == 0:
                used += c.counter("opt.narrow_groups")
        c.dev_opt_sync()
        c.synchronize()
        return Y.cpu().numpy(), u.cpu().numpy(), g.cpu().numpy(), c.dev_opt_losses(), used


def test_optimizer_keeps_its_bits():
    a, b, o = optimize(6000, 150, 1), optimize(6000, 150, 1), optimize(6000, 150, 0)
    assert a[4] > 0 and a[4] == b[4] == o[4]
    for other in (b, o):
        for x, y in zip(a[:3], other[:3]):
            assert np.array_equal(x, y)
        assert a[3] == other[3]
    assert len(a[3]) == 15


def transform(chain):
    """A 5,000-point map fitted on the context (60 iterations, narrow groups
    forced), then 300 new points embedded into it: the map's tree ("bhx.")
    beside the optimizer's and the single-call trees."""
    n, m, k = 5000, 300, 30
    rp, col, val, Y0 = opt_problem(n)
    rng = np.random.default_rng(11)
    with T.Context(0) as c:
        c.set_option("bh_chain", chain)
        c.set_option("narrow", 0.25)
        Yr, u, g = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
        c.optimize(rp, col, val, Yr, u, g, default_params(iterations=60, theta=0.5))
        nb = np.argsort(rng.random((m, n)), axis=1)[:, :k].astype(np.int32)   # k distinct map points per new one
        xrp = np.arange(0, m * k + 1, k, dtype=np.int64)
        P = c.pairwiseAffinities(xrp, rng.uniform(0.5, 2.0, size=m * k), 10.0)
        Y = c.transformInit(xrp, nb.ravel(), P, Yr)
        upd, gains = np.zeros_like(Y), np.ones_like(Y)
        losses = c.transform(Yr, xrp, nb.ravel(), P, Y, upd, gains,
                             default_params(iterations=40, theta=0.5, learning_rate=1.0))
        F, z = c.repulsionQueries(Yr, 0.5, Y)   # the single-call query tree ("bhx1.")
    return Yr, Y, upd, gains, losses, F, z


def test_transform_on_a_fitted_map_keeps_its_bits():
    a, b, o = transform(1), transform(1), transform(0)
    for other in (b, o):
        for i in (0, 1, 2, 3, 5, 6):
            assert np.array_equal(a[i], other[i]), i
        assert a[4] == other[4]


def test_teardown_releases_streams_and_events():
    """Context open, three optimizer steps, close, ten times over: the tree's
    events and the moments' stream go with the context while a selection may
    still be queued on the second stream."""
    n = 6000
    rp, col, val, Y0 = opt_problem(n)
    p = default_params(iterations=150, theta=0.5)
    dev = torch.device("cuda", 0)
    Pd = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rp, col, val))
    ends = []
    for _ in range(10):
        c = T.Context(0)
        c.set_option("narrow", 0.25)
        Y = torch.from_numpy(Y0.copy() * 1e4).to(dev)   # (past the root-tile phase: full builds and traversals)
        u, g = torch.zeros_like(Y), torch.ones_like(Y)
        c.dev_opt_setup(p, *Pd, n, Y, u, g)
        for t in range(1, 4):
            c.dev_opt_step(t)
        c.close()
        torch.cuda.synchronize()
        ends.append(Y.cpu().numpy())
    assert all(np.array_equal(ends[0], e) for e in ends[1:])
    assert np.isfinite(ends[0]).all()


def test_option_default_and_range():
    with T.Context(0) as c:
        assert c.get_option("bh_chain") == 1
        c.set_option("bh_chain", 0)
        assert c.get_option("bh_chain") == 0
        with pytest.raises(Exception):
            c.set_option("bh_chain", 2)
