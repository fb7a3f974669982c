"""tile_apply's lane-wise windows with the next step's two points gathered
ahead (option "tile_prefetch" 1) against the loop that waits for its own
gathers (0): per lane the same points in the same order through the same
operations, so the repulsion (F, z) and a device-optimizer trajectory with its
losses are equal with np.array_equal, with and without the counters (the
counting instantiation is a kernel of its own).  Shapes as in
test_gpu_tile_pass.py (one wave, a partial last wave, below and above
CSORT_MIN_N, theta 0.5 and 0.25, with and without clumps, duplicates, points
outside the root cell, the unprimed and a primed build of one context; each
also through the counting kernels), and a
41-point shape whose lane-wise tile of odd length ends at the last sorted
point: the step that must not read past the positions."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import oracle_ctypes as O
import tsne_amd as T
from test_gpu_csort import ring_problem, run
from test_gpu_tile_pass import embedding

ROOT = Path(__file__).resolve().parent.parent


def test_tile_prefetch_option_declared():
    """No device: the key is in the option table (range 0..1) and in the
    header's list with its default, and Options has it."""
    capi = (ROOT / "tsne-flink_amd" / "csrc" / "capi.cpp").read_text()
    assert re.search(r'\{"tile_prefetch",\s*nullptr,\s*&Options::tile_prefetch,\s*0,\s*1\}', capi)
    common = (ROOT / "tsne-flink_amd" / "csrc" / "common.hpp").read_text()
    m = re.search(r"\bint tile_prefetch = (\d);", common)
    assert m and int(m.group(1)) in (0, 1)
    assert re.search(r'"tile_prefetch" %s\b' % m.group(1), (ROOT / "include" / "tsne_hip.h").read_text())


@pytest.mark.gpu
def test_tile_prefetch_option_round_trip():
    with T.Context(0) as a, T.Context(0) as b:
        default = a.get_option("tile_prefetch")
        assert default in (0.0, 1.0)
        for v in (0, 1, 0, 1):
            a.set_option("tile_prefetch", v)
            assert a.get_option("tile_prefetch") == float(v) and b.get_option("tile_prefetch") == default
        for bad in (2, -1, 0.5):
            with pytest.raises(T.TsneError):
                a.set_option("tile_prefetch", bad)
        assert a.get_option("tile_prefetch") == 1.0


def repulsions(Ys, theta, prefetch, stats=False, counters=()):
    """(F, z) of each call in one context (the first build is unprimed, the
    later ones take the previous order), tile_pass 0; `stats`: through the
    counting kernels, then also the "bh." counters named, of the last call."""
    with T.Context(0) as c:
        c.set_option("tile_pass", 0)
        c.set_option("tile_prefetch", prefetch)
        if stats:
            c.set_option("rep_stats", 1)
        out = [c.repulsion(Y, theta) for Y in Ys]
        return out, {k: c.counter("bh." + k) for k in counters}


def assert_same(Ys, theta, stats=False):
    ref, _ = repulsions(Ys, theta, 0)
    for pf in ((0, 1) if stats else (1,)):
        got, _ = repulsions(Ys, theta, pf, stats)
        assert len(got) == len(ref)
        for (Fa, za), (Fb, zb) in zip(ref, got):
            assert np.array_equal(Fa, Fb) and np.array_equal(za, zb), pf


@pytest.mark.gpu
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("clumps", [False, True])
@pytest.mark.parametrize("theta", [0.5, 0.25])
@pytest.mark.parametrize("n", [64, 4097, 20_000, 50_000])
def test_repulsion_same_bits(n, theta, clumps, stats):
    Y = embedding(n, 31 + n, clumps)
    assert_same([Y, Y * 1.02 + 0.01], theta, stats)


@pytest.mark.gpu
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("n,theta", [(4097, 0.5), (50_000, 0.25)])
def test_repulsion_duplicates(n, theta, stats):
    assert_same([embedding(n, 5, True, dups=True), embedding(n, 6, False, dups=True)], theta, stats)


@pytest.mark.gpu
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("n,theta", [(4097, 0.25), (50_000, 0.5)])
def test_repulsion_outside_root_cell(n, theta, stats):
    assert_same([embedding(n, 8, True, outside=True), embedding(n, 9, False, outside=True)], theta, stats)


@pytest.mark.gpu
@pytest.mark.parametrize("theta", [0.5, 0.25])
def test_largest_shape_runs_the_lane_wise_windows(theta):
    """Not vacuous: at n = 50,000 with clumps the lane-wise windows sum pairs
    under tile_prefetch 1, as many (and in as many steps) as under 0."""
    Y = embedding(50_000, 31 + 50_000, True)
    keys = ("tile_pairs0", "tile_steps0")
    _, c0 = repulsions([Y, Y * 1.02 + 0.01], theta, 0, True, keys)
    _, c1 = repulsions([Y, Y * 1.02 + 0.01], theta, 1, True, keys)
    print(c0, c1)
    assert c1["tile_pairs0"] > 0
    assert c1 == c0


@functools.lru_cache(maxsize=None)
def end_of_pos(odd_high):
    """(Y, oracle F, oracle z), read only: two clumps of 20 and 21 points (width
    1e-3) at (-0.5, -0.5) and (0.5, 0.5), n = 41.  At theta 0.5 a lane takes
    its own clump as one small tile and the other as a cell, so the busiest
    lane's 20-21 points are fewer than the window's 41 and the window goes
    lane-wise; the clump sorted last is a tile that ends at the last sorted
    point.  `odd_high`: the 21-point clump is the one at (0.5, 0.5) -- one of
    the two placements puts the tile of odd length last, whichever way the
    Morton order runs."""
    rng = np.random.default_rng(41)
    lo, hi = (20, 21) if odd_high else (21, 20)
    Y = np.concatenate([np.array([-0.5, -0.5]) + rng.normal(size=(lo, 2)) * 1e-3,
                        np.array([0.5, 0.5]) + rng.normal(size=(hi, 2)) * 1e-3])
    Y = np.ascontiguousarray(Y[rng.permutation(41)])
    rep, zi = O.repulsion(Y, 0.5, threads=8)
    for a in (Y, rep, zi):
        a.setflags(write=False)
    return Y, rep, zi


@pytest.mark.gpu
@pytest.mark.parametrize("odd_high", [False, True])
def test_odd_tile_at_the_end_of_pos(odd_high):
    Y, rep, zi = end_of_pos(odd_high)
    ref, c0 = repulsions([Y, Y], 0.5, 0, True, ("tile_pairs0",))
    got, c1 = repulsions([Y, Y], 0.5, 1, True, ("tile_pairs0",))
    plain, _ = repulsions([Y, Y], 0.5, 1)
    print(c0, c1)
    assert c1["tile_pairs0"] > 0 and c1 == c0
    with T.Context(0) as c:
        tol = c.get_option("near_tol_early")
    for (Fa, za), (Fb, zb), (Fc, zc) in zip(ref, got, plain):
        assert np.array_equal(Fa, Fb) and np.array_equal(za, zb)
        assert np.array_equal(Fa, Fc) and np.array_equal(za, zc)
        assert np.abs(zc - zi).max() <= tol * zi.max()
        assert np.abs(Fc - rep).max() <= tol * np.abs(rep).max()


_RING = {}


@pytest.mark.gpu
def test_trajectory():
    """40 device-optimizer iterations (a build and a repulsion in each) from a
    mid-phase-sized start with duplicates: Y and the losses, 1 against 0."""
    n = 20_000
    if n not in _RING:
        _RING[n] = ring_problem(n)
    opts = (("graph_order", 0), ("tile_pass", 0))
    Y0, l0, over = run(n, 2, 1, 31, dups=True, scale=0.4, problem=_RING[n], options=opts + (("tile_prefetch", 0),))
    assert over == 0 and len(l0) > 0
    Y1, l1, _ = run(n, 2, 1, 31, dups=True, scale=0.4, problem=_RING[n], options=opts + (("tile_prefetch", 1),))
    assert l1 == l0
    assert np.array_equal(Y1, Y0)
