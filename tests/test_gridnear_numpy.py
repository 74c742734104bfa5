"""CPU: the claims of include/loik_amd_gridnear.h on the numpy reference (tests/gridnear_numpy.py), from first principles: the passes over
the 64-bit keys give the transform of the brute force, ties to the lowest index; the chosen cube bounds the exact distance from above
where the grid header's pair bounds it from below; the gradient of a grid constraint is the derivative of the exact distance to the
chosen cube; the shares of configurations that the GPU tests leave out stay under their cap; the wall of voxels holds the reference
back as the analytic wall does."""
import numpy as np
import pytest

import avoid_numpy as AN
import clearance_numpy as CN
import grid_numpy as GN
import gridnear_cases as GC
import gridnear_numpy as NN
import pose_numpy as P

EPS = 1e-12     # as test_grid_numpy.py: a few ulps of the largest coordinate per operation
H = 1e-6        # the step of the central difference, test_avoid_numpy.py's
FD_REL = 1e-6   # |g - fd| <= FD_REL max |fd|: relative, as the issue sets it
FD_FLOOR = 1e-3 # a row whose max |fd| is below this is left out: the central difference itself is rounded to ~ 1e-16 / H = 1e-10, which is
                # 1e-6 of a derivative of 1e-4; the floor leaves ten times that.  (A sphere whose motion is orthogonal to the normal.)


@pytest.mark.parametrize("seed", range(8))
def test_passes_equal_brute_force(seed):
    rng = np.random.default_rng(seed)
    for frac in (0.0, 0.05, 0.2, 0.6, 1.0):
        dims = tuple(int(d) for d in rng.integers(1, 8, size=3))
        occ = GN.random_occupancy(dims, frac, seed) if 0.0 < frac < 1.0 else np.full(dims[::-1], int(frac), dtype=np.uint8)
        G, F = NN.feature_passes(occ)
        assert np.array_equal(F, NN.feature_brute(occ)) and np.array_equal(G, GN.field_brute(occ)), (dims, frac)
    assert np.all(NN.feature_brute(np.zeros((2, 3, 4))) == NN.NO_VOXEL)
    assert np.array_equal(NN.feature_brute(np.ones((2, 3, 4))).ravel(), np.arange(24))


@pytest.mark.parametrize("name", GC.BUILD)
def test_build_cases_equal_brute_force(name):
    occ = GC.build_occupancy(name)
    G, F = GC.build_want(name)
    assert np.array_equal(F, NN.feature_brute(occ)) and np.array_equal(G, GN.field_brute(occ))


def test_the_feature_attains_the_field():
    """F[v] is occupied and at G[v] from v: the high words of the keys are the field"""
    for name in GC.BUILD:
        occ = GC.build_occupancy(name)
        G, F = GC.build_want(name)
        if not occ.any():
            assert np.all(F == NN.NO_VOXEL) and np.all(G == GN.EMPTY)
            continue
        nz, ny, nx = occ.shape
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        u = F.astype(np.int64)
        ux, uy, uz = u % nx, (u // nx) % ny, u // (nx * ny)
        assert np.all(occ[uz, uy, ux] != 0)
        assert np.array_equal(GN.g(x - ux) + GN.g(y - uy) + GN.g(z - uz), G.astype(np.int64))


def test_ties_go_to_the_lowest_index():
    """two occupied voxels at equal distance along each axis and diagonally: F of the voxel between them, and the chosen cube of a
    centre there, is the lower index; a centre inside a cube takes the face of the largest d, the lowest axis on a tie"""
    for grid, sph, winner, inside_n in GC.tie_case():
        a = np.argwhere(grid.occ)
        mid = (a[0] + a[1]) // 2
        assert grid.F[mid[0], mid[1], mid[2]] == winner[0] and np.array_equal(NN.feature_passes(grid.occ)[1], grid.F)
        got = NN.query(sph, grid)
        assert np.array_equal(got["vox"][:, 1], winner)
        both = NN.cube_distance(sph[:3, None, :3], np.array([(p[0] * 5 + p[1]) * 5 + p[2] for p in a])[None, :], grid)
        assert np.all(both[:, 0] == both[:, 1]) and np.all(both[:, 0] > 0)
        assert np.array_equal(got["normal"][3:], inside_n) and np.all(got["val"][3:, 1] == -sph[3:, 3])


def _points(grid, rng, n):
    ext = grid.hi - grid.origin
    return np.concatenate([grid.origin + rng.uniform(size=(n, 3)) * ext, grid.origin + rng.uniform(-1.0, 2.0, size=(n, 3)) * ext])


def test_lower_bound_exact_upper_bound():
    """v <= exact <= d_u - r for a centre outside O; the upper bound is the distance to an occupied cube; the normal is a unit vector and
    the derivative of that distance"""
    rng = np.random.default_rng(21)
    seen = 0
    for k in range(10):
        dims = tuple(int(d) for d in rng.integers(1, 9, size=3))
        occ = GN.random_occupancy(dims, (0.05, 0.2, 0.5)[k % 3], 200 + k)
        grid = NN.Grid(occ, rng.uniform(-1.0, 1.0, size=3), rng.uniform(0.05, 0.4))
        pts = _points(grid, rng, 80)
        r = rng.uniform(0.0, 0.1, size=pts.shape[0])
        pr = NN.pair(pts, r, grid)
        if not occ.any():
            assert np.all(pr["u"] == -1) and np.all(np.isposinf(pr["upper"])) and not pr["normal"].any()
            continue
        exact = GN.exact_distance(pts, grid) - r
        out = exact + r > 0
        assert np.all(pr["v"][out] <= exact[out] + EPS) and np.all(exact[out] <= pr["upper"][out] + EPS)
        assert np.all(pr["v"][~out] <= -r[~out] + EPS)
        u = pr["u"]
        assert np.all(grid.occ.ravel()[u])
        free = out & (pr["du"] > 1e-3)
        assert np.allclose(np.linalg.norm(pr["normal"][free], axis=1), 1.0, rtol=0, atol=EPS)
        for j in range(3):
            e = np.zeros(3)
            e[j] = H
            fd = (NN.cube_distance(pts[free] + e, u[free], grid) - NN.cube_distance(pts[free] - e, u[free], grid)) / (2 * H)
            kink = np.min(np.abs(np.abs(pts[free] - NN.cube_centre(u[free], grid)) - 0.5 * grid.h), axis=1) < 1e-4
            assert np.all(np.abs(fd - pr["normal"][free][:, j])[~kink] <= 1e-8)
        seen += int(free.sum())
    assert seen > 500


def test_query_reference_on_the_seeded_spheres():
    grid, sph = GC.query_grid(), GC.query_spheres()
    want = NN.query(sph, grid)
    assert want["near"].mean() <= 0.01 and grid.occ.any()
    exact = GN.exact_distance(sph[:, :3], grid) - sph[:, 3]
    out = exact + sph[:, 3] > 0
    assert np.all(want["val"][out, 0] <= exact[out] + EPS) and np.all(exact[out] <= want["val"][out, 1] + EPS)
    assert len(set(want["vox"][:, 1].tolist())) > 5 and np.all(want["val"][:, 0] <= want["val"][:, 1] + EPS)
    nan = NN.query(np.array([[0.0, np.nan, 0.0, 0.1], [0.0, 0.0, 0.0, np.inf]]), grid)
    assert np.all(np.isnan(nan["val"])) and np.all(nan["vox"] == -1) and np.all(np.isnan(nan["normal"]))


def fd_rows(c, want):
    """the rows of gridnear_cases.fd_case on which the finite-difference check is defined: the witness is a grid pair with a cube, not
    near, and under q (+) +-H e_j for every j the chosen cube, the face region and the witness sphere stay the same.  -> [(i, a, u, fd [nv])],
    fd the central difference of the exact distance to the cube u, less the radius"""
    model, links, spheres, grid = c["model"], c["links"], c["spheres"], c["grid"]
    rows = []
    for i in range(c["q"].shape[0]):
        kind, a, _ = (int(x) for x in want["witness"][i])
        u = int(want["cube"][i])
        if kind != GN.WORLD_GRID or u < 0 or want["near"][i] or not AN.pair_dofs(model, links[a]).any():   # (a sphere on link 0 moves with no DoF)
            continue
        qs = []
        for j in range(model.nv):
            v = np.zeros(model.nv)
            v[j] = H
            qs += [P.integrate(model, c["q"][i], v), P.integrate(model, c["q"][i], -v)]
        cen = CN.centres(model, np.stack(qs), [links[a]], spheres[[a]])[:, 0]
        pr = NN.pair(cen, spheres[a, 3], grid)
        region = lambda x: np.abs(x - NN.cube_centre(u, grid)) - 0.5 * grid.h > 0.0
        if np.any(pr["u"] != u) or np.any(region(cen) != region(want["centres"][i, a])) or np.all(~region(want["centres"][i, a])):
            continue
        d = NN.cube_distance(cen, np.full(cen.shape[0], u), grid)
        if np.max(np.abs(d[0::2] - d[1::2])) / (2.0 * H) < FD_FLOOR:
            continue
        rows.append((i, a, u, (d[0::2] - d[1::2]) / (2.0 * H)))
    return rows


def test_gradient_of_a_grid_witness_is_the_derivative_of_the_distance_to_the_cube():
    c = GC.fd_case()
    want = c["grad"]
    assert np.all(want["witness"][:, 0] == GN.WORLD_GRID)
    rows = fd_rows(c, want)
    assert len(rows) >= 20, len(rows)
    worst = 0.0
    for i, a, u, fd in rows:
        err = float(np.max(np.abs(want["grad"][i] - fd))) / float(np.max(np.abs(fd)))
        worst = max(worst, err)
        assert err <= FD_REL, (i, a, u, err)
        assert not np.any(want["grad"][i][~AN.pair_dofs(c["model"], c["links"][a])])
    print("gridnear_numpy: %d rows, max |g - fd| / max |fd| %.3e" % (len(rows), worst))


@pytest.mark.parametrize("name", GC.ROBOTS)
def test_share_of_configurations_left_out(name):
    """the GPU test leaves out the configurations in which a sphere lies within FACE of a face or a mid-plane, or a decision of the rule
    is near: at most NEAR_SHARE; and the case means something: grid partners among the active constraints"""
    c = GC.avoid_case(name)
    assert c["box"]["near"].mean() <= GC.NEAR_SHARE and c["grad"]["near"].mean() <= GC.NEAR_SHARE, (c["box"]["near"].mean(), c["grad"]["near"].mean())
    nwo = c["ws"].shape[0] + c["wb"].shape[0]
    kinds = [k["partner"] == nwo and k["kind"] == 0 for row in c["box"]["cons"] for k in row]
    assert sum(kinds) >= 3 and not all(kinds), (sum(kinds), len(kinds))
    assert (c["box"]["partner"][:, :, 0] == nwo).any() and (c["box"]["partner"][:, :, 0] < nwo).any()
    # the minima and the witness are grid_numpy.clearance's
    plain = GN.clearance(c["model"], c["q"], c["links"], c["spheres"], c["ws"], c["wb"], c["grid"], c["pairs"])
    assert np.array_equal(plain["min"], c["grad"]["min"]) and np.array_equal(plain["witness"], c["grad"]["witness"])
    # without a grid the reference is avoid_numpy's, bit for bit
    args = (c["model"], c["q"][:5], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"])
    a, b = NN.avoidance_box(*args, 0.25, -1.0, 1.0, 0.02, 0.15, 0.5), AN.avoidance_box(*args, 0.25, -1.0, 1.0, 0.02, 0.15, 0.5)
    assert all(np.array_equal(a[k], b[k]) for k in ("lo", "hi", "pairs", "partner", "near"))


def size_conditions(inp):
    """what an input of test_gridnear.test_sizes_with_a_grid misses (empty: nothing): no row is near (at 17 and 9 rows a share means
    nothing), and a grid witness"""
    ref = GC.size_ref(inp)
    miss = []
    for k in ("box", "grad"):
        if ref[k]["near"].any():
            miss.append((k, "near", int(ref[k]["near"].sum())))
    if not (ref["grad"]["witness"][~ref["grad"]["near"], 0] == GN.WORLD_GRID).any():
        miss.append("no grid witness")
    nwo = inp["ws"].shape[0] + inp["wb"].shape[0]
    if not (ref["box"]["partner"][~ref["box"]["near"]][:, :, 0] == nwo).any():
        miss.append("no grid partner")
    return miss


@pytest.mark.parametrize("ns", GC.SIZE_NS)
def test_size_inputs_with_a_grid(ns):
    inputs = GC.size_inputs(ns)
    assert len(inputs) == (len(GC.SIZE_WORLDS) if ns > 2 else 3)
    for inp in inputs:
        assert size_conditions(inp) == [], inp["what"]
    # with no other world object every sphere's world partner is the grid, at ordinal 0
    alone = GC.size_ref(inputs[0])["box"]
    assert inputs[0]["split"] == (0, 0) and np.all(alone["partner"][:, :, 0] == 0)


def test_half_grid_and_empty_grid_inputs():
    """the robot leaves the half grid's box: centres outside it among the grid partners and the active grid constraints; the share left out"""
    c = GC.half_grid_case()
    assert c["box"]["near"].mean() <= GC.NEAR_SHARE and c["grad"]["near"].mean() <= GC.NEAR_SHARE
    nwo = c["ws"].shape[0] + c["wb"].shape[0]
    keep = ~c["box"]["near"]
    assert c["outside"].mean() >= 0.1 and (c["outside"] & (c["box"]["partner"][:, :, 0] == nwo) & keep[:, None]).any()
    active = [(i, k["a"]) for i, row in enumerate(c["box"]["cons"]) if keep[i] for k in row if k["kind"] == 0 and k["partner"] == nwo]
    assert any(c["outside"][i, a] for i, a in active) and any(not c["outside"][i, a] for i, a in active)
    assert ((c["grad"]["witness"][:, 0] == GN.WORLD_GRID) & ~c["grad"]["near"]).any()
    # an empty grid: every pair of it is +inf, so the reference's box is the box without a grid
    e = GC.empty_grid_case()
    args = (e["model"], e["q"][:5], e["links"], e["spheres"], e["ws"], e["wb"], e["pairs"])
    a, b = NN.avoidance_box(*args, 0.25, -1.0, 1.0, 0.02, 0.15, 0.5, grid=e["grid"]), AN.avoidance_box(*args, 0.25, -1.0, 1.0, 0.02, 0.15, 0.5)
    assert all(np.array_equal(a[k], b[k]) for k in ("lo", "hi", "pairs", "partner"))


# ---- the pose loops ------------------------------------------------------------------------------------------------------------------
# The wall of voxels.  The rule promises, to first order in dt |z|, d(next) - d_safe >= (1 - kappa) (d - d_safe) for the clearance d it
# reads, which here is the lower bound v <= the exact clearance: no recorded configuration may come nearer to the cubes than d_safe less
# the first-order slack, for which test_avoid_pose.py allows half of d_safe on the analytic wall; the same floor here.  WALL_PROGRESS as
# there: with the latch every instance still closes part of its pose error before the wall holds it; measured on the reference
# (0.70 in the median, 0.75 at most: the voxel wall holds the arm up to sqrt(3) h earlier than the analytic one) and asserted below
WALL_FLOOR = 0.025
WALL_PROGRESS = 0.8


def exact_path_clearance(w, paths):
    """the least exact clearance to the cubes over each instance's configurations"""
    c = w["col"]
    boxes = GN.cubes(c["grid"])
    return np.array([GN.exact_clearance(w["model"], p, c["links"], c["spheres"], c["grid"], boxes).min() for p in paths])


def test_wall_of_voxels_holds_the_reference():
    import test_avoid_pose as TP
    assert WALL_FLOOR == TP.WALL["d_safe"] / 2 and GC.WALL_H <= TP.WALL["d_safe"]
    w = GC.wall_workload()
    assert w["col"]["grid"].occ.sum() > 100
    held = GC.pose_oracle(w, TP.WALL_DT, TP.WALL_GAIN, TP.WALL_STEPS, TP.WALL, TP.TOL)
    free = GC.pose_oracle(w, TP.WALL_DT, TP.WALL_GAIN, TP.WALL_STEPS, dict(d_safe=-1e9, d_influence=-1e8, kappa=0.5), TP.TOL)
    cheld, cfree = exact_path_clearance(w, held["q_path"]), exact_path_clearance(w, free["q_path"])
    e0, e1 = TP.wall_errors(w, w["q0"]), np.abs(held["err"]).max(axis=(1, 2))
    print("gridnear_numpy wall: least exact clearance held %.4f, free %.4f; progress median %.3f max %.3f; near %.3f" %
          (cheld.min(), cfree.min(), np.median(e1 / e0), (e1 / e0).max(), held["near"].mean()))
    assert (cfree < WALL_FLOOR).mean() >= 0.5 and np.all(cheld >= WALL_FLOOR)
    assert np.all(e1 <= WALL_PROGRESS * e0) and (held["avoid_active_steps"] > 0).mean() >= 0.5
    assert np.all(np.abs(held["q"] - w["q0"]).max(axis=1) > 0.2)


@pytest.mark.parametrize("name", ["panda7", "talos32"])
def test_pose_workloads_mean_something(name):
    import test_avoid_pose as TP
    w = GC.pose_workload(name)
    nwo = w["col"]["ws"].shape[0] + w["col"]["wb"].shape[0]
    for k in (1, 4):
        o = GC.pose_oracle(w, 0.25, 0.5, k, TP.AVOID, TP.TOL)
        assert o["near"].mean() <= GC.NEAR_SHARE, (name, k, o["near"].mean())
        assert (o["avoid_active_steps"] > 0).mean() >= 0.25
    t = NN.nearest(w["model"], w["q0"], w["col"]["links"], w["col"]["spheres"], w["col"]["ws"], w["col"]["wb"], w["col"]["pairs"], w["col"]["grid"])
    assert ((t["partner"][:, :, 0] == nwo) & (t["pairs"][:, :, 0] < TP.AVOID["d_influence"])).any()
