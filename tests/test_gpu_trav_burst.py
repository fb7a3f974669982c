"""Option trav_burst (bhtree.hip RecHead / RecChild): the 64-query BH
traversal reads a popped record's fields from its LDS copy in bursts -- the
head's with child 0's at the top of the pop, child c + 1's while child c is
evaluated -- instead of one by one at first use (0, the order before).  Only
the order of the LDS reads and the copy's layout differ: the same operations
on the same operands per lane, the same pushes, tile lists and costs.  So F
and z must be bit-equal between 0 and 1 on every path of the pop loop, also
with heavy groups in the narrow layout (whose selection reads the costs the
64-query walk recorded, and whose own kernel the option does not touch), and
1 must match the oracle within the library's near-exact bound.

Inputs, the smallest at which each path runs: the mid-phase shape at two
theta (every child kind mix, pushes, tiles recorded from the head burst); a
tiny embedding with a dense core (near-exact tiles at almost every pop:
first / last / cnt from the burst); duplicates and key ties (QK_MULTI, QK_TIE
and virtual chain tops: the rare kinds, read in place after the child loop);
a geometric cascade of clusters (deep walks over records of 1-2 children,
the likeliest to reach the one-record batches taken once the stack is over
half full -- the library has no counter for that branch, so whether it ran is
not asserted); 70 and 4,097 uniform points (a partial last wave, batches of
fewer than 4 records, records whose last child is child 0)."""
import functools

import numpy as np
import pytest

import oracle_ctypes as O
import tsne_amd as T
from test_gpu_narrow import clustered

pytestmark = pytest.mark.gpu


def _clustered(theta):
    return clustered(20_000, 5), theta


def _small_embedding():
    n = 20_000
    rng = np.random.default_rng(12)
    Y = rng.normal(size=(n, 2)) * 0.03
    Y[: n // 4] *= 0.01
    return Y, 0.5


def _duplicates_and_ties():
    Y = clustered(20_000, 9)
    Y[[5, 900, 17_000]] = Y[5]
    Y[100:140] = Y[100]
    return Y, 0.25


def _cascade():
    """Cluster k: ~300 points at scale 4^-k around the origin, k = 0..25."""
    rng = np.random.default_rng(31)
    return np.concatenate([rng.normal(size=(300 + k, 2)) * 4.0 ** -k for k in range(26)]), 0.5


def _uniform(n):
    return np.random.default_rng(n).uniform(-1.0, 1.0, size=(n, 2)), 0.5


INPUTS = {
    "clustered_theta0.5": functools.partial(_clustered, 0.5),
    "clustered_theta0.25": functools.partial(_clustered, 0.25),
    "small_embedding": _small_embedding,
    "duplicates_ties": _duplicates_and_ties,
    "cascade": _cascade,
    "uniform70": functools.partial(_uniform, 70),
    "uniform4097": functools.partial(_uniform, 4097),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """(Y, theta, oracle F, oracle z): made once per input, shared by its cases, read only."""
    Y, theta = INPUTS[name]()
    Y = np.ascontiguousarray(Y)
    rep, zi = O.repulsion(Y, theta, threads=8)
    for a in (Y, rep, zi):
        a.setflags(write=False)
    return Y, theta, rep, zi


def traverse(Y, theta, burst, narrow):
    """(F, z, narrow groups) with trav_burst = burst.  narrow > 0: the first
    call only selects (from its own costs, reuse_costs 1); the second one runs
    the heavy groups in the narrow layout."""
    with T.Context(0) as c:
        c.set_option("trav_burst", burst)
        c.set_option("reuse_costs", 1)
        c.set_option("narrow", narrow)
        F, z = c.repulsion(Y, theta)
        assert c.counter("bh.narrow_groups") == 0
        ng = 0
        if narrow > 0:
            F, z = c.repulsion(Y, theta)
            ng = c.counter("bh.narrow_groups")
        tol = c.get_option("near_tol_early")
    return F, z, ng, tol


@pytest.mark.parametrize("narrow", [0, 0.25])
@pytest.mark.parametrize("name", list(INPUTS))
def test_burst_equals_in_place_reads_and_oracle(name, narrow):
    Y, theta, rep, zi = problem(name)
    F0, z0, ng0, _ = traverse(Y, theta, 0, narrow)
    F1, z1, ng1, tol = traverse(Y, theta, 1, narrow)
    assert ng0 == ng1   # the same costs, so the same selection
    if narrow > 0 and len(Y) >= 20_000:
        assert ng1 > 0
    assert np.array_equal(F0, F1) and np.array_equal(z0, z1)
    assert np.abs(z1 - zi).max() <= tol * zi.max()
    assert np.abs(F1 - rep).max() <= tol * np.abs(rep).max()


def test_option_default_and_range():
    with T.Context(0) as c:
        assert c.get_option("trav_burst") == 1
        with pytest.raises(Exception):
            c.set_option("trav_burst", 2)
