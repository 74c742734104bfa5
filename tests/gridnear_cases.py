"""The inputs that the CPU and the GPU tests of include/loik_amd_gridnear.h share, each computed once: the grids of the build test, the
spheres of the query test, the three robots of the gradient / box test with their numpy answers, and the pose workloads with their
lock-step oracles (gridnear_numpy.narrower behind pose_step_numpy.lockstep_pose_loop_step, which with max_backtracks = 0 and
patience = 0 is SolvePose: test_avoid_routes_numpy.py proves that identity)."""
import numpy as np

import clearance_numpy as CN
import grid_numpy as GN
import gridnear_numpy as NN

_CACHE = {}

# ---- 1. the build -----------------------------------------------------------------------------------------------------------------------
BUILD = ["1x1x1", "2x1x1-full", "5x4x3", "65x33x3", "3x3x257", "33x257x2", "empty", "full"]


def build_occupancy(name):
    """[nz][ny][nx] uint8.  65 voxels along x: a partial tile past one tile width; 257 along z and along y: the narrow tile of either pass"""
    if name == "1x1x1":
        return np.ones((1, 1, 1), dtype=np.uint8)
    if name == "2x1x1-full":
        return np.ones((1, 1, 2), dtype=np.uint8)
    if name == "empty":
        return np.zeros((4, 5, 6), dtype=np.uint8)
    if name == "full":
        return np.ones((4, 5, 6), dtype=np.uint8)
    dims = tuple(int(d) for d in name.split("x"))
    return GN.random_occupancy(dims, {"5x4x3": 0.2}.get(name, 0.003), 3000 + BUILD.index(name))


def build_want(name):
    """(G, F) by the passes of the reference, which test_gridnear_numpy.py proves equal to the brute force on these very grids"""
    if ("build", name) not in _CACHE:
        _CACHE[("build", name)] = NN.feature_passes(build_occupancy(name))
    return _CACHE[("build", name)]


# ---- 2. the query ------------------------------------------------------------------------------------------------------------------------
def query_grid():
    if "qgrid" not in _CACHE:
        import test_grid_clearance as TG
        _CACHE["qgrid"] = NN.of(TG._grid(3100))
    return _CACHE["qgrid"]


def query_spheres(n=4096, seed=3101):
    """n spheres around the query grid, inside it and outside by up to half an extent, none within FACE voxels of a voxel face or of a
    mid-plane through voxel centres (redrawn until so)"""
    grid = query_grid()
    rng = np.random.default_rng(seed)
    ext = grid.hi - grid.origin
    c = grid.origin + rng.uniform(-0.5, 1.5, size=(n, 3)) * ext
    for _ in range(64):
        bad = NN.near_plane(c, grid)
        if not bad.any():
            break
        c[bad] = grid.origin + rng.uniform(-0.5, 1.5, size=(int(bad.sum()), 3)) * ext
    assert not NN.near_plane(c, grid).any()
    return np.concatenate([c, rng.uniform(0.0, 0.1, size=(n, 1))], axis=1)


def plane_spheres():
    """a small set exactly on voxel faces, on mid-planes, on the grid's boundary and outside the box: there the device may read an
    adjacent cell"""
    grid = query_grid()
    rng = np.random.default_rng(3102)
    n = 48
    c = grid.origin + rng.uniform(0.0, 1.0, size=(n, 3)) * (grid.hi - grid.origin)
    k = rng.integers(0, 3, size=n)
    idx = rng.integers(0, grid.n[k] + 1)
    c[np.arange(n), k] = grid.origin[k] + np.where(np.arange(n) % 2 == 0, idx, np.minimum(idx, grid.n[k] - 1) + 0.5) * grid.h
    corner = grid.origin + rng.integers(0, 2, size=(8, 3)) * (grid.hi - grid.origin)
    outside = grid.origin + rng.uniform(-1.0, 2.0, size=(16, 3)) * (grid.hi - grid.origin)
    c = np.concatenate([c, corner, outside])
    return np.concatenate([c, np.full((c.shape[0], 1), 0.02)], axis=1)


def tie_case():
    """a grid with two occupied voxels and spheres whose centres are at equal distance from both cubes: along each axis and diagonally;
    and centres inside a cube.  Binary coordinates: every quantity is exact, so the tie is a tie on the device too.
    -> a list of (grid, spheres [n][4], the cube that must win [n], the normal of an inside centre or None)"""
    h, origin = 0.25, np.array([-1.0, -0.5, 0.0])
    out = []
    for step in ((2, 0, 0), (0, 2, 0), (0, 0, 2), (2, 2, 0), (0, 2, 2), (2, 2, 2)):   # the second cube two voxels on: one voxel between them
        occ = np.zeros((5, 5, 5), dtype=np.uint8)
        a = np.array([1, 1, 1])
        b = a + np.array(step)
        occ[a[2], a[1], a[0]] = occ[b[2], b[1], b[0]] = 1
        mid = origin + (0.5 * (a + b) + 0.5) * h                                       # the centre of the voxel between the two
        off = np.where(np.array(step) == 0, 1.0, 0.0) * np.array([[0.0, 0.0, 0.0], [h / 8, h / 16, h / 4], [-h / 4, -h / 8, -h / 16]])
        c = mid + off                                                                   # (moved only along the axes the cubes share)
        inside = origin + (a + 0.5) * h + np.array([[h / 8, h / 16, 0.0], [h / 8, h / 8, 0.0], [-h / 16, h / 8, -h / 8]])
        sph = np.concatenate([np.concatenate([c, inside]), np.full((6, 1), 0.03125)], axis=1)
        out.append((NN.Grid(occ, origin, h), sph, np.full(6, (a[2] * 5 + a[1]) * 5 + a[0]),
                    np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])))
    return out


# ---- 3. gradient and box on three robots ----------------------------------------------------------------------------------------------
ROBOTS = ("panda7", "talos32", "tree330")
NEAR_SHARE = 0.10   # configurations with a sphere within FACE of a face or a mid-plane, or near in avoid_numpy's sense, are left out


def avoid_case(name):
    """test_grid_clearance.case(name): spheres, boxes, a grid and self pairs at once; 24 (panda7), 66 (talos32) and 100 (tree330, the first
    100 of its 329: the reference is O(n ns^2), and the kernel takes its HBM path for the joints, not for the spheres) spheres; with the
    numpy box and gradient"""
    if ("avoid", name) not in _CACHE:
        import test_avoid_box as TB
        import test_grid_clearance as TG
        c = dict(TG.case(name))
        if len(c["links"]) > 100:
            c["links"], c["spheres"] = c["links"][:100], c["spheres"][:100]
            c["pairs"] = CN.self_pairs(c["model"].parents, c["links"])
        c["grid"] = NN.of(c["grid"])
        args = (c["model"], c["q"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"])
        c["box"] = NN.avoidance_box(*args, TB.DT, -np.inf, np.inf, grid=c["grid"], **TB.PRM)
        c["grad"] = NN.clearance_gradient(*args, grid=c["grid"])
        _CACHE[("avoid", name)] = c
    return _CACHE[("avoid", name)]


def fd_case():
    """panda7 against the grid alone: every witness is a grid pair"""
    if "fd" not in _CACHE:
        c = dict(avoid_case("panda7"))
        c["ws"], c["wb"], c["pairs"] = np.zeros((0, 4)), np.zeros((0, 15)), []
        c["grad"] = NN.clearance_gradient(c["model"], c["q"], c["links"], c["spheres"], grid=c["grid"])
        _CACHE["fd"] = c
    return _CACHE["fd"]


# ---- 3b. the sizes and the worlds of the grid branch ---------------------------------------------------------------------------------------
# lp = 0, 1, 2 and 6 sphere slots a wavefront, partial last trips on either side of 64, and the largest model
SIZE_NS = [1, 2, 3, 33, 63, 64, 65, 256]
# ((world spheres, boxes) beside the grid, self pairs on): the grid alone (nws == 0 and nwb == 0: the ordinal arithmetic of the grid pair
# with nothing before it), one kind of object missing, and a full world
SIZE_WORLDS = (((0, 0), False), ((0, 0), True), ((1, 0), False), ((0, 1), True), ((33, 32), False), ((33, 32), True))
SIZE_WORLD_SCALE = 0.25   # the radii and half extents of the full world, against test_clearance._world's
SIZE_ROWS = 17   # configurations (9 at 256 spheres): a last workgroup with idle wavefronts; the reference is O(n ns^2)
# the seed of each size's worlds: the first from 0 on for which test_gridnear_numpy.test_size_inputs_with_a_grid holds
SIZE_SEEDS = {1: 1}   # (the one sphere of ns = 1 sits on the universe: the first draw puts the world's sphere nearer to it than any cube)


def size_grid():
    """the grid of every size: test_grid_clearance._grid around panda7's base at a density of 2 %"""
    if "sgrid" not in _CACHE:
        import test_grid_clearance as TG
        _CACHE["sgrid"] = NN.of(TG._grid(3300, frac=0.02))
    return _CACHE["sgrid"]


def size_inputs(ns):
    """test_avoid_box.size_inputs(ns) -- panda7, the spheres dealt round-robin to the links 0..7 -- with the worlds of SIZE_WORLDS beside
    size_grid(); a world with self pairs on is left out where the spheres have none (ns <= 2)"""
    if ("sizes", ns) not in _CACHE:
        import test_avoid_box as TB
        import test_clearance as TC
        base = TB.size_inputs(ns)[0]
        model, links, spheres = base["model"], base["links"], base["spheres"]
        q = base["q"][:SIZE_ROWS]
        pairs_on = CN.self_pairs(model.parents, links)
        rng = np.random.default_rng(3310 + 100 * SIZE_SEEDS.get(ns, 0) + ns)
        out = []
        for split, self_on in SIZE_WORLDS:
            if self_on and not pairs_on:
                continue
            ws, wb = TC._world(rng, *split)
            if split[0] > 1:   # (65 objects of the stock size hold the overall minimum in every row: no grid witness would occur)
                ws[:, 3] *= SIZE_WORLD_SCALE
                wb[:, 12:15] *= SIZE_WORLD_SCALE
            pairs = pairs_on if self_on else []
            out.append(dict(what="panda7 ns=%d world=%d+%d+grid self=%d" % (ns, split[0], split[1], len(pairs)), model=model, q=q, links=links,
                            spheres=spheres, ws=ws, wb=wb, pairs=pairs, split=split, self_on=self_on, grid=size_grid()))
        _CACHE[("sizes", ns)] = out
    return _CACHE[("sizes", ns)]


def size_ref(inp):
    """the numpy box and gradient of one of those inputs, computed once"""
    key = ("sizeref", inp["what"])
    if key not in _CACHE:
        import test_avoid_box as TB
        args = (inp["model"], inp["q"], inp["links"], inp["spheres"], inp["ws"], inp["wb"], inp["pairs"])
        _CACHE[key] = dict(box=NN.avoidance_box(*args, TB.DT, -np.inf, np.inf, grid=inp["grid"], **TB.PRM),
                           grad=NN.clearance_gradient(*args, grid=inp["grid"]))
    return _CACHE[key]


def half_grid_case():
    """avoid_case("panda7") against the middle half of size_grid()'s extent along every axis (the query grid's box and voxel, at a density
    that leaves an eighth of the volume some cubes): the arm leaves the grid's box, so many centres are clamped into it (dout > 0, and
    clamped indices among the candidates)"""
    if "half" not in _CACHE:
        import test_avoid_box as TB
        c = dict(avoid_case("panda7"))
        g = size_grid()
        nz, ny, nx = g.occ.shape
        z0, y0, x0 = nz // 4, ny // 4, nx // 4
        occ = np.ascontiguousarray(g.occ[z0:z0 + (nz + 1) // 2, y0:y0 + (ny + 1) // 2, x0:x0 + (nx + 1) // 2])
        c["grid"] = NN.Grid(occ, g.origin + g.h * np.array([x0, y0, z0], dtype=float), g.h)
        args = (c["model"], c["q"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"])
        c["box"] = NN.avoidance_box(*args, TB.DT, -np.inf, np.inf, grid=c["grid"], **TB.PRM)
        c["grad"] = NN.clearance_gradient(*args, grid=c["grid"])
        cen = c["box"]["centres"]
        c["outside"] = ((cen < c["grid"].origin) | (cen > c["grid"].hi)).any(axis=-1)   # [n][ns]
        _CACHE["half"] = c
    return _CACHE["half"]


def empty_grid_case():
    """avoid_case("panda7") with no voxel occupied"""
    c = dict(avoid_case("panda7"))
    g = c["grid"]
    c["grid"] = NN.Grid(np.zeros_like(g.occ), g.origin, g.h)
    return c


# ---- 4. the pose loops -------------------------------------------------------------------------------------------------------------------
def pose_workload(name):
    """test_avoid_pose._workload(name, 0) with a grid beside its spheres and boxes.  The robot starts clear of the voxels: a cube within
    d_safe + 2 h of a sphere of some seed is taken out, so that the bound v (at most sqrt(3) h under the distance) is above d_safe at
    every seed.  (At or below d_safe the sign of a gradient entry alone decides a bound, and the face of a cube has the normal of a world
    axis, about which talos32 has a joint: a run that starts there is near in gridnear_numpy's sense, and says nothing.)"""
    if ("pose", name) not in _CACHE:
        import test_avoid_pose as TP
        import test_grid_clearance as TG
        w = dict(TP._workload(name, 0))
        g = TG._grid(3200 + len(name), frac=0.01)
        cen = CN.centres(w["model"], w["q0"], w["col"]["links"], w["col"]["spheres"])
        occ = np.array(g.occ, dtype=np.uint8)
        for (uz, uy, ux), cube in zip(np.argwhere(g.occ), GN.cubes(g)):
            if np.min(CN.sphere_box(cen, w["col"]["spheres"][None, :, 3], cube)) < TP.AVOID["d_safe"] + 2.0 * g.h:
                occ[uz, uy, ux] = 0
        w["col"] = dict(w["col"], grid=NN.Grid(occ, g.origin, g.h))
        _CACHE[("pose", name)] = w
    return _CACHE[("pose", name)]


def pose_oracle(w, dt, gain, k, avoid, tol):
    """SolvePose of k steps by the lock-step reference, with avoid_min_seen / avoid_active_steps / avoid_flags / near and q_path (the
    step-start configurations of every instance)"""
    key = ("oracle", id(w), dt, gain, k, tuple(sorted(avoid.items())))
    if key not in _CACHE:
        import pose_step_numpy as PS
        from test_pose_ik import PRM
        hook = NN.narrower(w["model"], w["col"], avoid, dt, w["B"])
        paths = [[] for _ in range(w["B"])]

        def recording(b, q_b, lo, hi):
            paths[b].append(np.array(q_b))
            return hook(b, q_b, lo, hi)

        lb, ub = w["box"]
        o = PS.lockstep_pose_loop_step(w["model"], PRM, w["q0"], np.eye(6), np.zeros(6), w["links"], w["A"], lb, ub, w["tg"], dt, gain, tol, k,
                                       max_backtracks=0, patience=0, narrow=recording)
        o.update(hook.results)
        o["q_path"] = [np.array(p + [o["q"][b]]) for b, p in enumerate(paths)]
        _CACHE[key] = o
    return _CACHE[key]


WALL_H = 0.04   # <= d_safe of test_avoid_pose.WALL


def wall_workload():
    """test_avoid_pose._wall_case with its slab voxelised: the voxels of edge WALL_H whose centre lies in the slab, and no box"""
    if "wall" not in _CACHE:
        import test_avoid_pose as TP
        w = dict(TP._wall_case())
        box = w["col"]["wb"][0]
        reach = np.abs(box[:9].reshape(3, 3)) @ box[12:15]
        origin = box[9:12] - reach - WALL_H
        dims = tuple(int(d) for d in np.ceil((2.0 * reach + 2.0 * WALL_H) / WALL_H))
        occ = NN.voxelise_box(box, origin, WALL_H, dims)
        w["col"] = dict(w["col"], wb=np.zeros((0, 15)), grid=NN.Grid(occ, origin, WALL_H, G=GN.field_passes(occ), F=NN.feature_passes(occ)[1]))
        _CACHE["wall"] = w
    return _CACHE["wall"]
