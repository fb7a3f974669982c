"""The fit's octree (csrc/octree.hip, octree.hpp) on degenerate geometry and
small trees: points exactly on cell boundaries and on the root's face, exact
duplicates, key-tie groups, coplanar / collinear / anisotropic clouds, and
tree sizes at the build's own edges (one wave, OREC_BLK, MOM3_MIN, the
bottom-up block, MOM3_CHUNK, DENSE3_MAX).  Every other 3-D fit test feeds the
tree an isotropic Gaussian cloud without duplicates.

All tests but section F call Context.repulsion(Y, theta) (per-point F and z):
no P matrix, so a tree error cannot hide behind the attraction.

References.
  exact3(Y)   numpy longdouble, O(n^2): z_i = sum_j 1 / (1 + D_ij),
              F_i = sum_j (y_i - y_j) / (1 + D_ij)^2 over the sources j: the
              rows inside the root cell, |y_jk| <= W for k = 0, 1, 2 with
              W = the largest column extent (fp64, as build_otree has it);
              rows outside are queries only.  A source at D_ij = 0 gives 0.
  the oracle  O.repulsion3_queries(Y, theta, Y), the octree restatement.

The fit's duplicate rule: exact duplicates count at full multiplicity for
every other query and give nothing to a query at their own position.  The
oracle counts that way only when every copy beyond a group's first sits in
the last rows (then no leaf holding copies splits afterwards), which is how
the duplicate cases here are built; the GPU sorts, so its result does not
depend on the row order.  The CPU tests below hold the two references against
each other on every case, so the construction itself is checked.

Sections (the unmarked tests run without a GPU):
  CPU  oracle(theta 0) == exact3 to 1e-13 on every case; the edge guard: for
       every (case, theta > 0) pair used below the oracle's z moves by
       <= 1e-12 max z between theta (1 - 1e-13) and theta (1 + 1e-13), i.e.
       no cell sits on the opening criterion, where a last-bit difference of
       a centre of mass would legitimately flip the decision.
  A    theta 0 against exact3, each traversal ("oct_records" 0, 1, 2):
       1e-12 of max z_e, max |F_e| (test_gradient3_matches_oracle's bound).
  B    theta > 0 strict ("near_tol3_early" 0, "oct_moments" 0), each traversal,
       against the oracle per point: |z - zo| <= 1e-11 zo and
       max_k |F - Fo| <= 1e-11 zo (test_gpu_transform3.check_against_oracle,
       whose derivation covers n <= 5000 terms).
  C    theta > 0 with the default options (and each traversal alone) against
       the oracle: z 1e-7 max zo, F 1e-6 max |Fo|
       (test_octal_records_match_binary_walk_and_oracle's bounds).
  D    the two record layouts agree to 1e-12 on every case of C.
  E    a call's result does not depend on the calls before it.
  F    the same inputs through tsne_gradient and one device optimizer step.

Each GPU test prints its error as a fraction of its bound and the section's
running worst per layout (pytest -s); DESIGN.md section 4 records them.
"""
import numpy as np
import pytest

import oracle_ctypes as O
import tsne_amd as T
from tsne_amd.api import default_params

SIZES = (2, 3, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025, 2047, 2049)


# ---------------------------------------------------------------- the cases
def lat(g):
    """The lattice g x g x g."""
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))


def _gauss():
    return np.random.default_rng(0).normal(size=(1500, 3))


def _dups_last():
    Y = _gauss()
    Y[-40:] = Y[7]
    Y[-45:-40] = Y[300]
    Y[-47:-45] = Y[900]
    return Y


def _build(name):
    G = _gauss()
    if name == "gauss":                 # the control
        return G
    if name == "offset":                # 2 points outside the root cell
        return G + np.array([4.0, -2.0, 1.0])
    if name == "coplanar0":             # every point on the root's z split plane, and on a face ever after
        G[:, 2] = 0.0
        return G
    if name == "coplanar":
        G[:, 2] = 0.75
        return G
    if name == "coplanar_x0":           # on the root's x split plane: the axis whose closed rule (west iff
        G[:, 0] = 0.0                   # x <= cx) differs from the floor of the fixed-point digits
        return G
    if name == "line_diag":
        return np.outer(np.random.default_rng(1).normal(size=700), np.ones(3))
    if name == "line_axis":             # only column 0 non-zero
        Y = np.zeros((700, 3))
        Y[:, 0] = np.random.default_rng(2).normal(size=700)
        return Y
    if name == "aniso":
        return G * np.array([1.0, 1e-3, 1e-6])
    if name == "lat_centred":           # the outermost planes on the level-1 split planes
        return lat((np.arange(12) - 5.5) / 8)
    if name == "lat_octant":            # minimum exactly 0: one face of points on the root's face (|y_k| == W)
        return lat(np.arange(12) / 8)
    if name == "lat_planes":            # points on the split planes of every level down to 1/8
        return lat((np.arange(13) - 6) / 8)
    if name == "lat_octant8":
        return lat(np.arange(8) / 8)
    if name == "tight":                 # key ties: 1e-9 << W 2^-21
        G[1000:1040] = G[1000] + np.random.default_rng(3).normal(size=(40, 3)) * 1e-9
        return G
    if name == "dups_last":             # groups of 41, 6 and 3 copies, every copy beyond the first in the last rows
        return _dups_last()
    if name == "dups_small":            # the whole tree near-exact: tiles that hold the query's own duplicates
        return _dups_last() * 1e-3
    if name == "all_same":              # W = 0: the root cell is the origin alone, every point outside it
        return np.tile(np.random.default_rng(4).normal(size=3), (70, 1))
    if name == "all_same0":             # W = 0 at the origin: the root is one 70-point key-tie group
        return np.zeros((70, 3))
    if name == "one_apart":             # W = the small gap: every point outside the root cell
        p = np.array([5.0, -6.0, 7.0])
        Y = np.tile(p, (70, 1))
        Y[1] = p + np.array([0.25, -0.5, 0.125])
        return Y
    if name == "dup_heavy":             # one point and 69 copies of another, all inside the root cell
        Y = np.tile(np.array([0.3, -0.2, 0.1]), (70, 1))
        Y[1] = np.array([-0.5, 0.6, -0.4])
        return Y
    n, s = name[1:].split("_s")
    return np.random.default_rng(int(n)).normal(size=(int(n), 3)) * float(s)


SHAPED = ["gauss", "offset", "coplanar0", "coplanar", "coplanar_x0", "line_diag", "line_axis", "aniso", "lat_centred", "lat_octant",
          "lat_planes", "lat_octant8", "tight", "dups_last", "dups_small", "all_same", "all_same0", "one_apart",
          "dup_heavy"]
SIZES_1 = ["n%d_s1.0" % n for n in SIZES]
SIZES_SMALL = ["n%d_s1e-3" % n for n in SIZES]
ALL_CASES = SHAPED + SIZES_1 + SIZES_SMALL
ZERO_CASES = ("all_same", "all_same0", "one_apart")   # exact zeros expected

# B: theta > 0, strict.  The lattices sit on the opening criterion at 0.5 and
# 0.25 (the edge guard moves z by up to 1.5e-3 there) and run at the theta the
# guard passes; lat_planes fails it at all three and runs at theta 0 only.
B_GENERIC = ["gauss", "offset", "coplanar0", "coplanar", "coplanar_x0", "line_diag", "line_axis", "aniso",
             "dups_last"] + SIZES_1
LATTICE_PAIRS = [("lat_centred", 0.3), ("lat_octant", 0.3), ("lat_octant8", 0.5)]
B_PAIRS = [(c, th) for c in B_GENERIC for th in (0.5, 0.25)] + LATTICE_PAIRS
# C: theta > 0, default options.  tight's tie group, dups_small and the
# s = 1e-3 sizes (dense tiles, moment tasks, their ndup corrections) join.
C_PAIRS = [(c, 0.5) for c in B_GENERIC + ["tight", "dups_small", "dup_heavy"] + SIZES_SMALL] + LATTICE_PAIRS
GUARD_PAIRS = sorted(set(B_PAIRS + C_PAIRS))

_cases, _exact, _oracle = {}, {}, {}


def case(name):
    """The case's points (made once, shared, read-only)."""
    if name not in _cases:
        Y = np.ascontiguousarray(_build(name), dtype=np.float64)
        assert Y.ndim == 2 and Y.shape[1] == 3 and len(Y) <= 2200
        Y.setflags(write=False)
        _cases[name] = Y
    return _cases[name]


def root_half_width(Y):
    """W of the root Cell(0, 0, 0, W): the largest column extent, in fp64."""
    return float(np.max(Y.max(axis=0) - Y.min(axis=0)))


def exact3(Y):
    """The O(n^2) sums over the rows inside the root cell, in longdouble, rounded to fp64."""
    src = np.all(np.abs(Y) <= root_half_width(Y), axis=1)
    S = Y[src].astype(np.longdouble)
    F, z = np.zeros((len(Y), 3)), np.zeros(len(Y))
    for a in range(0, len(Y), 256):
        d = Y[a:a + 256, None, :].astype(np.longdouble) - S[None, :, :]
        D = (d * d).sum(axis=2)
        q = np.where(D == 0, np.longdouble(0), 1 / (1 + D))
        z[a:a + 256] = q.sum(axis=1)
        F[a:a + 256] = ((q * q)[:, :, None] * d).sum(axis=1)
    return F, z


def exact(name):
    if name not in _exact:
        F, z = exact3(case(name))
        F.setflags(write=False)
        z.setflags(write=False)
        _exact[name] = (F, z)
    return _exact[name]


def oracle(name, theta):
    """The oracle's (F, z) for every point of the case as a query (computed once, shared, read-only)."""
    if (name, theta) not in _oracle:
        Y = case(name)
        F, z = O.repulsion3_queries(Y, theta, Y)
        F.setflags(write=False)
        z.setflags(write=False)
        _oracle[(name, theta)] = (F, z)
    return _oracle[(name, theta)]


def worst(err, bound):
    """max err / bound; a zero bound asks for err == 0."""
    err, bound = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    r = np.where(err == 0, 0.0, np.inf)
    np.divide(err, bound, out=r, where=bound > 0)
    return float(r.max())


_figures = {}


def report(section, layout, name, theta, rz, rf):
    """Print the test's error / bound ratios and the section's running worst per layout."""
    w = _figures.setdefault((section, layout), [0.0, 0.0])
    w[0], w[1] = max(w[0], rz), max(w[1], rf)
    print("%s layout %s %s theta %g: z %.3e F %.3e of the bound (worst so far: z %.3e F %.3e)"
          % (section, layout, name, theta, rz, rf, w[0], w[1]))


# ------------------------------------------------------------ CPU: references
def test_cases_are_what_they_claim():
    """The properties the cases are there for."""
    Y = case("offset")
    assert np.count_nonzero(np.abs(Y).max(axis=1) > root_half_width(Y)) == 2
    for name in ("all_same", "one_apart"):      # every point outside the root cell
        Y = case(name)
        assert np.all(np.abs(Y).max(axis=1) > root_half_width(Y)), name
    for name in ("all_same", "all_same0"):
        assert root_half_width(case(name)) == 0.0
    for name in ("dup_heavy", "all_same0", "dups_last", "dups_small", "tight", "lat_octant", "lat_planes"):
        Y = case(name)
        assert np.all(np.abs(Y) <= root_half_width(Y)), name
    Y = case("lat_octant")                      # a face of points on the root's face, another on its split planes
    W = root_half_width(Y)
    assert Y.min() == 0.0 and np.count_nonzero(Y == W) == 3 * 144 and np.count_nonzero(Y == 0.0) == 3 * 144
    Y = case("lat_planes")                      # W = 1.5: on the split planes 0, +-0.75 and +-0.375
    W = root_half_width(Y)
    assert W == 1.5 and all(np.count_nonzero(Y == v) == 3 * 169 for v in (0.0, 0.75, -0.75, 0.375, -0.375))
    Y = case("tight")                           # 40 distinct points within 1e-2 of a level-21 cell's width
    ext = root_half_width(Y)
    assert len(np.unique(Y[1000:1040], axis=0)) == 40
    assert np.abs(Y[1000:1040] - Y[1000]).max() < 1e-2 * ext * 2.0 ** -20
    Y = case("dups_last")                       # copies beyond a group's first: the last rows only
    first = {}
    late = [i for i, r in enumerate(map(tuple, Y)) if first.setdefault(r, i) != i]
    assert late == list(range(1500 - 47, 1500))


@pytest.mark.parametrize("name", ALL_CASES)
def test_oracle_theta0_equals_exact3(name):
    """Both references, the source rule and the duplicates-last construction:
    the octree restatement at theta 0 is the exact sum (measured <= 8e-16)."""
    Fe, ze = exact(name)
    Fo, zo = oracle(name, 0.0)
    rz, rf = worst(np.abs(zo - ze).max(), 1e-13 * ze.max()), worst(np.abs(Fo - Fe).max(), 1e-13 * np.abs(Fe).max())
    print("%s: z %.3e F %.3e of 1e-13" % (name, rz, rf))
    assert rz <= 1.0 and rf <= 1.0
    if name in ZERO_CASES:
        assert not ze.any() and not Fe.any() and not zo.any() and not Fo.any()


@pytest.mark.parametrize("name,theta", GUARD_PAIRS)
def test_edge_guard(name, theta):
    """No cell of the case sits on the opening criterion at this theta: a
    later change of a case cannot silently make a comparison ill-posed."""
    Y = case(name)
    _, z = oracle(name, theta)
    for th in (theta * (1.0 - 1e-13), theta * (1.0 + 1e-13)):
        _, z1 = O.repulsion3_queries(Y, th, Y)
        assert np.abs(z1 - z).max() <= 1e-12 * z.max(), th


# ------------------------------------------------------------------ contexts
@pytest.fixture(scope="module")
def contexts():
    """One context per option set, made on first use, closed with the module."""
    made = {}

    def get(**opts):
        key = tuple(sorted(opts.items()))
        if key not in made:
            c = T.Context(0)
            for k, v in opts.items():
                c.set_option(k, v)
            made[key] = c
        return made[key]

    yield get
    for c in made.values():
        c.close()


def strict(rec):
    return dict(oct_records=rec, oct_layout_switch=0, near_tol3_early=0, oct_moments=0)


def layout_opts(layout):
    """"default": the library's options (the per-call layout switch included); 0 / 1 / 2: that traversal alone."""
    return {} if layout == "default" else dict(oct_records=layout, oct_layout_switch=0)


# ------------------------------------------------------- A: theta 0, exact
@pytest.mark.gpu
@pytest.mark.parametrize("rec", [0, 1, 2])
@pytest.mark.parametrize("name", ALL_CASES)
def test_theta0_matches_exact(contexts, name, rec):
    Fe, ze = exact(name)
    F, z = contexts(oct_records=rec, oct_layout_switch=0).repulsion(case(name), 0.0)
    rz, rf = worst(np.abs(z - ze).max(), 1e-12 * ze.max()), worst(np.abs(F - Fe).max(), 1e-12 * np.abs(Fe).max())
    report("A", rec, name, 0.0, rz, rf)
    assert rz <= 1.0 and rf <= 1.0
    if name in ZERO_CASES:
        assert not z.any() and not F.any()


# ------------------------------------------------------ B: theta > 0, strict
def check_strict(section, rec, name, theta, F, z):
    Fo, zo = oracle(name, theta)
    rz, rf = worst(np.abs(z - zo), 1e-11 * zo), worst(np.abs(F - Fo).max(axis=1), 1e-11 * zo)
    report(section, rec, name, theta, rz, rf)
    assert rz <= 1.0 and rf <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("rec", [0, 1, 2])
@pytest.mark.parametrize("name,theta", B_PAIRS)
def test_strict_matches_oracle_per_point(contexts, name, theta, rec):
    """No near-exact tiles, no moments: the same cells opened and summarised
    as the oracle's, so each point agrees to rounding.  The bound is the
    foreign walk's 1e-11 zo for all three traversals: measured on an MI355X on
    the gauss control, max |z - zo| / zo = 1.4e-15 / 6.7e-16 / 1.6e-15 and
    max |F - Fo| / zo = 3.5e-16 / 2.6e-16 / 3.5e-16 for "oct_records" 0 / 1 / 2
    (theta 0.5 and 0.25), so no layout needs a bound of its own; the worst
    case of the section is `offset` at 2.7e-15."""
    F, z = contexts(**strict(rec)).repulsion(case(name), theta)
    check_strict("B", rec, name, theta, F, z)


# --------------------------------------- C, D: theta > 0, the default options
_gpu_c = {}


def default_run(contexts, layout, name, theta):
    if (layout, name, theta) not in _gpu_c:
        _gpu_c[(layout, name, theta)] = contexts(**layout_opts(layout)).repulsion(case(name), theta)
    return _gpu_c[(layout, name, theta)]


def check_default(section, layout, name, theta, F, z):
    Fo, zo = oracle(name, theta)
    rz, rf = worst(np.abs(z - zo).max(), 1e-7 * zo.max()), worst(np.abs(F - Fo).max(), 1e-6 * np.abs(Fo).max())
    report(section, layout, name, theta, rz, rf)
    assert rz <= 1.0 and rf <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["default", 0, 1, 2])
@pytest.mark.parametrize("name,theta", C_PAIRS)
def test_default_options_match_oracle(contexts, name, theta, layout):
    F, z = default_run(contexts, layout, name, theta)
    check_default("C", layout, name, theta, F, z)


@pytest.mark.gpu
@pytest.mark.parametrize("name,theta", C_PAIRS)
def test_record_layouts_agree(contexts, name, theta):
    """The 8-query and the 64-query record traversals take the same decisions:
    equal to re-association level."""
    F1, z1 = default_run(contexts, 1, name, theta)
    F2, z2 = default_run(contexts, 2, name, theta)
    rz, rf = worst(np.abs(z1 - z2).max(), 1e-12 * z1.max()), worst(np.abs(F1 - F2).max(), 1e-12 * np.abs(F1).max())
    report("D", "1 vs 2", name, theta, rz, rf)
    assert rz <= 1.0 and rf <= 1.0


# --------------------------------------------------- E: history independence
# (lat_centred at theta 0.5 fails the edge guard: it is here as a call in
# between, of another size and shape, and is not compared with the oracle)
HISTORY = ("gauss", "dups_small", "lat_centred", "gauss")


@pytest.mark.gpu
def test_single_calls3_are_history_free():
    with T.Context(0) as c:
        c.set_option("oct_moments", 0)
        out = [c.repulsion(case(name), 0.5) for name in HISTORY]
    assert np.array_equal(out[0][0], out[-1][0]) and np.array_equal(out[0][1], out[-1][1])


@pytest.mark.gpu
def test_single_calls3_default_options_stay_in_bound():
    """The moment gate follows the previous traversal's demand: whatever ran
    before, a call stays within the default options' bound."""
    with T.Context(0) as c:
        out = [c.repulsion(case(name), 0.5) for name in HISTORY]
    print("first and last call bit-equal: %s" % (np.array_equal(out[0][0], out[-1][0]) and
                                                 np.array_equal(out[0][1], out[-1][1])))
    for k in (0, 1, 3):
        check_default("E", "default", HISTORY[k], 0.5, *out[k])


# ------------------------------------------------------------ F: one level up
@pytest.mark.gpu
@pytest.mark.parametrize("name,seed", [("coplanar0", 81), ("dups_last", 82)])
def test_gradient3_on_degenerate_input(contexts, name, seed):
    """tsne_gradient on the same points (test_gradient3_matches_oracle's tolerances)."""
    from test_gpu_parity import random_problem
    Y = case(name)
    rp, col, val = random_problem(len(Y), 10, seed=seed)
    g, Z, loss = contexts().gradient(rp, col, val, Y, 0.5, exaggeration=4.0, want_loss=True)
    r = O.gradient3(rp, col, val, Y, 0.5, exaggeration=4.0, want_loss=True)
    print("%s: grad %.3e of 1e-6 max|grad|, Z %.3e of 1e-7, loss %.3e of 1e-6"
          % (name, np.abs(g - r["grad"]).max() / (1e-6 * np.abs(r["grad"]).max()),
             abs(Z - r["Z"]) / (1e-7 * r["Z"]), abs(loss - r["loss"]) / (1e-6 * abs(r["loss"]))))
    assert np.abs(g - r["grad"]).max() <= 1e-6 * np.abs(r["grad"]).max()
    assert abs(Z - r["Z"]) <= 1e-7 * r["Z"]
    assert abs(loss - r["loss"]) <= 1e-6 * abs(r["loss"])


@pytest.mark.gpu
def test_optimize3_duplicates_device_path_matches_oracle(contexts):
    """Duplicates inside the 3-D device optimizer: one step against the oracle
    (the 2-D test_optimize_duplicates_device_path_matches_oracle's form; the
    copies sit in the last rows)."""
    import torch
    from test_gpu_parity import random_problem
    n = 500
    rp, col, val = random_problem(n, 12, seed=72)
    Y0 = np.random.default_rng(11).normal(size=(n, 3)) * 1e-2
    Y0[-3:] = Y0[5]
    Y0[-6:-3] = Y0[100]
    p = default_params(n_components=3, iterations=30, theta=0.5)
    ctx = contexts()
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    dY = t(Y0, torch.float64)
    du = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    dg = torch.ones((n, 3), dtype=torch.float64, device=dev)
    ctx.dev_opt_setup(p, t(rp, torch.int64), t(col, torch.int32), t(val, torch.float64), n, dY, du, dg)
    ctx.dev_opt_step(1)
    ctx.dev_opt_sync()
    ctx.synchronize()
    gr = O.gradient3(rp, col, val, Y0, 0.5, exaggeration=p.early_exaggeration)["grad"]
    Yo, uo, go = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
    O.update(gr, Yo, uo, go, p.min_gain, p.initial_momentum, p.learning_rate)
    O.center(Yo)
    err = np.abs(dY.cpu().numpy() - Yo).max()
    print("one step with duplicates: max |dY| = %.3e of 1e-6 max|Y|" % (err / (1e-6 * np.abs(Yo).max())))
    assert err <= 1e-6 * np.abs(Yo).max()
