"""The 2-D tree build's short chain (option "build_fuse", csort_run_fused2 and
the subtree moments on the second stream beside the traversal) against the
one-launch-per-pass chain (build_fuse 0): every array the build produces keeps its bits, so the
repulsion (F, z) and a device-optimizer trajectory with its losses are equal
with np.array_equal.  Shapes: the smallest at which each seam of the build
can fail -- the bottom-up boundaries (BU_FRONT 512, BU_NB 1024) on rocPRIM's
path, CSORT_MIN_N (16384) with a partial last workgroup above it, the first
(unprimed) and later (primed) builds of one context, points outside the root
cell, exact duplicates and a key-tie run, an oversized bucket (the sort's
global-memory path), theta 0 and 0.5, and trav_front_cur (the separate
gather_sorted stays)."""
import re
from pathlib import Path

import numpy as np
import pytest

import tsne_amd as T
from test_gpu_csort import ring_problem, run

ROOT = Path(__file__).resolve().parent.parent


def test_build_fuse_option_declared():
    """No device: the key is in the option table (default 1, range 0..1) and in
    the header's list (a context, hence tsne_ctx_get_option, needs a device:
    the round trip itself is test_build_fuse_option_round_trip)."""
    capi = (ROOT / "tsne-flink_amd" / "csrc" / "capi.cpp").read_text()
    assert re.search(r'\{"build_fuse",\s*nullptr,\s*&Options::build_fuse,\s*0,\s*1\}', capi)
    common = (ROOT / "tsne-flink_amd" / "csrc" / "common.hpp").read_text()
    assert re.search(r"\bint build_fuse = 1;", common)
    assert '"build_fuse" 1' in (ROOT / "include" / "tsne_hip.h").read_text()


@pytest.mark.gpu
def test_build_fuse_option_round_trip():
    with T.Context(0) as a, T.Context(0) as b:
        assert a.get_option("build_fuse") == 1.0
        a.set_option("build_fuse", 0)
        assert a.get_option("build_fuse") == 0.0 and b.get_option("build_fuse") == 1.0
        a.set_option("build_fuse", 1)
        assert a.get_option("build_fuse") == 1.0
        for bad in (2, -1, 0.5):
            with pytest.raises(T.TsneError):
                a.set_option("build_fuse", bad)


def embedding(n, seed, outside=True, dups=False):
    """n x 2 points; `outside`: shifted, so the root cell (centred at 0, half
    width = the larger extent) leaves some of them out; `dups`: exact
    duplicates and a 40-point run of one point (test_gpu_csort.run)."""
    Y = np.random.default_rng(seed).normal(size=(n, 2)) * 3.0
    if outside:
        Y = Y * np.array([1.0, 0.4]) + np.array([2.5, -1.0])
    if dups and n > 1040:
        Y[[3, 500, n - 7]] = Y[3]
        Y[1000:1040] = Y[1000]
    return Y


def repulsions(Ys, theta, fuse, options=()):
    """(F, z) of each of the calls in one context: the first build of a context
    is unprimed (rocPRIM's sort), the later ones take the previous order."""
    with T.Context(0) as c:
        c.set_option("build_fuse", fuse)
        for k, v in options:
            c.set_option(k, v)
        return [c.repulsion(Y, theta) for Y in Ys]


def assert_same(a, b):
    assert len(a) == len(b)
    for (Fa, za), (Fb, zb) in zip(a, b):
        assert np.array_equal(Fa, Fb) and np.array_equal(za, zb)


@pytest.mark.gpu
@pytest.mark.parametrize("theta", [0.0, 0.5])
@pytest.mark.parametrize("n", [2, 3, 513, 1025, 1537])
def test_repulsion_small_trees(n, theta):
    """Below CSORT_MIN_N: rocPRIM's sort and the old front end either way, the
    moments deferred to the traversal call; around BU_FRONT and BU_NB; two builds."""
    Ys = [embedding(n, 11 + n), embedding(n, 12 + n, dups=True)]
    assert_same(repulsions(Ys, theta, 1), repulsions(Ys, theta, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("n,theta,dups", [(16384, 0.0, False), (16384, 0.5, True), (20000, 0.5, False),
                                          (20000, 0.5, True), (50000, 0.5, False), (50000, 0.5, True)])
def test_repulsion_across_csort_min_n(n, theta, dups):
    """The fused front end from the second build on: points outside the root
    cell, a moved embedding (other buckets), then duplicates."""
    Y = embedding(n, 21 + n)
    Ys = [Y, Y * 1.02 + 0.01, embedding(n, 22 + n, dups=dups), embedding(n, 23 + n, outside=False, dups=dups)]
    assert_same(repulsions(Ys, theta, 1), repulsions(Ys, theta, 0))


@pytest.mark.gpu
def test_repulsion_oversized_bucket():
    """12k copies of one point at n = 60000: one bucket beyond the LDS sort, its
    epilogue (positions, duplicate counts) from the global-memory path."""
    n = 60_000
    Y = np.random.default_rng(4).normal(size=(n, 2))
    Y3 = Y * 1.01
    Y3[5000:17000] = Y3[5000]
    out = {}
    for fuse in (1, 0):
        with T.Context(0) as c:
            c.set_option("build_fuse", fuse)
            out[fuse] = [c.repulsion(Y, 0.5), c.repulsion(Y3, 0.5)]
            assert c.counter("bh.csort_oversized") >= 1
    assert_same(out[1], out[0])


@pytest.mark.gpu
def test_repulsion_trav_front_cur():
    opts = (("reuse_costs", 1), ("trav_front_cur", 0.8))
    Y = embedding(40_000, 9)
    Ys = [Y, Y * 1.01, Y * 1.02]
    assert_same(repulsions(Ys, 0.5, 1, opts), repulsions(Ys, 0.5, 0, opts))


_RINGS = {}


def ring(n):
    if n not in _RINGS:
        _RINGS[n] = ring_problem(n)
    return _RINGS[n]


@pytest.mark.gpu
@pytest.mark.parametrize("n,dups,scale", [(513, False, 3.0), (1537, True, 3.0), (16384, False, 3.0),
                                          (16384, False, 1e-4), (20000, True, 3.0), (50000, True, 3.0)])
def test_trajectory(n, dups, scale):
    """40 device-optimizer iterations (a full build in each; scale 1e-4 with the
    root tile off: the subtree-moment phase), Y and the losses."""
    opts = (("graph_order", 0), ("root_tile", 0))
    Ya, la, over = run(n, 2, 1, 31, dups=dups, scale=scale, problem=ring(n), options=opts + (("build_fuse", 1),))
    Yb, lb, _ = run(n, 2, 1, 31, dups=dups, scale=scale, problem=ring(n), options=opts + (("build_fuse", 0),))
    assert over == 0
    assert la == lb and len(la) > 0
    assert np.array_equal(Ya, Yb)
