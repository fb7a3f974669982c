"""tile_apply's packed rounds walked by runs and over passes of several rounds
(option "tile_pass": 1, 2, 4, 8) against the slot-bit loops, a round at a
time (tile_pass 0): the partial sums are grouped alike, so the repulsion
(F, z) and a device-optimizer trajectory with its losses are equal with
np.array_equal for every value, with and without the counters (the counting
instantiation is a kernel of its own).  Shapes: one wave (n = 64), a partial
last wave (4,097), below and above CSORT_MIN_N (20,000 and 50,000), theta 0.5
and 0.25, points N(0, sigma^2) of extent ~2-3 (the mid phase: small all-open
tiles) and the same with tight clumps in it (tiles that whole waves take: the
packed path, long tile lists that are cut into chunks), exact duplicates and
a 40-point run of one point, points outside the root cell, the first
(unprimed) and a later (primed) build of one context.  The per-path counters
show that the largest shape runs what it is meant to."""
import re
from pathlib import Path

import numpy as np
import pytest

import tsne_amd as T
from test_gpu_csort import ring_problem, run

ROOT = Path(__file__).resolve().parent.parent
PASSES = (1, 2, 4, 8)   # against 0


def test_tile_pass_option_declared():
    """No device: the key is in the option table (range 0..8; 3, 5, 6, 7 are
    refused by set_option) and in the header's list, and Options has it."""
    capi = (ROOT / "tsne-flink_amd" / "csrc" / "capi.cpp").read_text()
    assert re.search(r'\{"tile_pass",\s*nullptr,\s*&Options::tile_pass,\s*0,\s*8\}', capi)
    assert "option 'tile_pass' takes 0, 1, 2, 4 or 8" in capi
    common = (ROOT / "tsne-flink_amd" / "csrc" / "common.hpp").read_text()
    m = re.search(r"\bint tile_pass = (\d);", common)
    assert m and int(m.group(1)) in (0,) + PASSES
    assert re.search(r'"tile_pass" %s\b' % m.group(1), (ROOT / "include" / "tsne_hip.h").read_text())


@pytest.mark.gpu
def test_tile_pass_option_round_trip():
    with T.Context(0) as a, T.Context(0) as b:
        default = a.get_option("tile_pass")
        assert default in (0.0, 1.0, 2.0, 4.0, 8.0)
        for v in (0,) + PASSES:
            a.set_option("tile_pass", v)
            assert a.get_option("tile_pass") == float(v) and b.get_option("tile_pass") == default
        for bad in (3, 5, 6, 7, 9, -1, 0.5):
            with pytest.raises(T.TsneError):
                a.set_option("tile_pass", bad)
        assert a.get_option("tile_pass") == 8.0


def embedding(n, seed, clumps=False, outside=False, dups=False, nclumps=20, width=5e-4):
    """n x 2 points N(0, 0.4^2): an extent of ~3.  `clumps`: 70% of them in 20
    clumps of width 5e-4 instead, centres N(0, 0.3^2) (chosen with the counters
    of test_largest_shape_runs_every_path: 50 clumps leave the busiest wave at
    8 packed rounds at theta 0.5, 20 give 10 and 13); `outside`: squeezed and
    shifted, so the root cell (centred at 0) leaves some out; `dups`: exact
    duplicates and a 40-point run of one point."""
    rng = np.random.default_rng(seed)
    Y = rng.normal(size=(n, 2)) * 0.4
    if clumps:
        cen = rng.normal(size=(nclumps, 2)) * 0.3
        k = int(0.3 * n)
        Y[k:] = cen[rng.integers(0, nclumps, n - k)] + rng.normal(size=(n - k, 2)) * width
        Y = Y[rng.permutation(n)]
    if outside:
        Y = Y * np.array([1.0, 0.4]) + np.array([0.35, -0.15])
    if dups and n > 1040:
        Y[[3, 500, n - 7]] = Y[3]
        Y[1000:1040] = Y[1000]
    return Y


def repulsions(Ys, theta, tile_pass, stats=False):
    """(F, z) of each call in one context (the first build is unprimed, the
    later ones take the previous order); `stats`: through the counting kernels."""
    with T.Context(0) as c:
        c.set_option("tile_pass", tile_pass)
        if stats:
            c.set_option("rep_stats", 1)
        return [c.repulsion(Y, theta) for Y in Ys]


def assert_all_passes_same(Ys, theta, stats=False):
    ref = repulsions(Ys, theta, 0)
    for tp in ((0,) if stats else ()) + PASSES:
        got = repulsions(Ys, theta, tp, stats)
        assert len(got) == len(ref)
        for (Fa, za), (Fb, zb) in zip(ref, got):
            assert np.array_equal(Fa, Fb) and np.array_equal(za, zb), tp


@pytest.mark.gpu
@pytest.mark.parametrize("clumps", [False, True])
@pytest.mark.parametrize("theta", [0.5, 0.25])
@pytest.mark.parametrize("n", [64, 4097, 20_000, 50_000])
def test_repulsion_same_bits(n, theta, clumps):
    Y = embedding(n, 31 + n, clumps)
    assert_all_passes_same([Y, Y * 1.02 + 0.01], theta)


@pytest.mark.gpu
@pytest.mark.parametrize("n,theta", [(4097, 0.5), (50_000, 0.25)])
def test_repulsion_duplicates(n, theta):
    assert_all_passes_same([embedding(n, 5, True, dups=True), embedding(n, 6, False, dups=True)], theta)


@pytest.mark.gpu
@pytest.mark.parametrize("n,theta", [(4097, 0.25), (50_000, 0.5)])
def test_repulsion_outside_root_cell(n, theta):
    assert_all_passes_same([embedding(n, 8, True, outside=True), embedding(n, 9, False, outside=True)], theta)


@pytest.mark.gpu
def test_counting_kernels_same_bits():
    """The counting instantiations (rep_stats) of every value sum the same bits."""
    Y = embedding(50_000, 13, True, dups=True)
    assert_all_passes_same([Y, Y * 0.98], 0.25, stats=True)


@pytest.mark.gpu
@pytest.mark.parametrize("theta", [0.5, 0.25])
def test_largest_shape_runs_every_path(theta):
    """Not vacuous: at n = 50,000 with clumps (tile_pass 0) the lane-wise
    windows and the packed rounds both sum pairs, some wave has more packed
    rounds than the largest pass holds, and some tile lists are cut into chunks."""
    Y = embedding(50_000, 31 + 50_000, True)
    with T.Context(0) as c:
        c.set_option("tile_pass", 0)
        c.set_option("rep_stats", 1)
        c.repulsion(Y, theta)
        c.repulsion(Y * 1.02 + 0.01, theta)
        got = {k: c.counter("bh." + k) for k in ("tile_pairs0", "tile_pairs1", "tile_rounds_max",
                                                 "tile_chunked_waves")}
    print(got)
    assert got["tile_pairs0"] > 0 and got["tile_pairs1"] > 0
    assert got["tile_rounds_max"] > max(PASSES)
    assert got["tile_chunked_waves"] >= 1


_RING = {}


@pytest.mark.gpu
def test_trajectory():
    """40 device-optimizer iterations (a build and a repulsion in each) from a
    mid-phase-sized start with duplicates: Y and the losses, for every value."""
    n = 20_000
    if n not in _RING:
        _RING[n] = ring_problem(n)
    opts = (("graph_order", 0),)
    Y0, l0, over = run(n, 2, 1, 31, dups=True, scale=0.4, problem=_RING[n], options=opts + (("tile_pass", 0),))
    assert over == 0 and len(l0) > 0
    for tp in PASSES:
        Y1, l1, _ = run(n, 2, 1, 31, dups=True, scale=0.4, problem=_RING[n], options=opts + (("tile_pass", tp),))
        assert l1 == l0, tp
        assert np.array_equal(Y1, Y0), tp
