"""CPU: the claims of include/loik_amd_grid.h on the numpy reference (tests/grid_numpy.py), from first principles: the three min-plus
passes give the field of the brute force; (h / 2) sqrt(G) is the distance from a voxel's centre to the occupied cubes; the pair is a
lower bound of the exact distance to the union of the cubes (clearance_numpy.sphere_box per occupied voxel), never positive inside an
occupied cube, and within sqrt(3) h of the distance for a centre inside the grid's box -- on faces, on edges and outside the box too."""
import numpy as np
import pytest

import clearance_numpy as CN
import grid_numpy as GN

# the rounding of the pair and of the exact distance: a few ulps of the largest coordinate (about 10) per operation
EPS = 1e-12


def _grids():
    rng = np.random.default_rng(11)
    out = []
    for k in range(12):
        dims = tuple(int(d) for d in rng.integers(1, 8, size=3))
        occ = GN.random_occupancy(dims, (0.05, 0.2, 0.6)[k % 3], 100 + k)
        out.append(GN.Grid(occ, rng.uniform(-1.0, 1.0, size=3), rng.uniform(0.05, 0.4)))
    return out


GRIDS = _grids()


@pytest.mark.parametrize("seed", range(8))
def test_passes_equal_brute_force(seed):
    rng = np.random.default_rng(seed)
    for frac in (0.0, 0.05, 0.2, 0.6, 1.0):
        dims = tuple(int(d) for d in rng.integers(1, 8, size=3))
        occ = GN.random_occupancy(dims, frac, seed) if 0.0 < frac < 1.0 else np.full(dims[::-1], int(frac), dtype=np.uint8)
        assert np.array_equal(GN.field_passes(occ), GN.field_brute(occ)), (dims, frac)
    assert np.all(GN.field_brute(np.zeros((2, 3, 4))) == GN.EMPTY) and np.all(GN.field_brute(np.ones((2, 3, 4))) == 0)


def test_field_is_the_distance_of_the_voxel_centres():
    for grid in GRIDS:
        if not grid.occ.any():
            continue
        nz, ny, nx = grid.occ.shape
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        ctr = grid.origin + (np.stack([x, y, z], axis=-1) + 0.5) * grid.h
        d = np.maximum(GN.exact_distance(ctr, grid), 0.0)
        assert np.allclose(0.5 * grid.h * np.sqrt(grid.G.astype(float)), d, rtol=0, atol=EPS)


def _points(grid, rng, n):
    """inside the box, on voxel faces, on voxel edges, on the box's boundary, and outside by up to one extent"""
    ext = grid.hi - grid.origin
    inside = grid.origin + rng.uniform(size=(n, 3)) * ext
    face = inside.copy()
    k = rng.integers(0, 3, size=n)
    idx = rng.integers(0, grid.n[k] + 1)
    face[np.arange(n), k] = grid.origin[k] + idx * grid.h                    # one coordinate on a voxel face (the box's faces included)
    edge = face.copy()
    k2 = (k + 1) % 3
    edge[np.arange(n), k2] = grid.origin[k2] + rng.integers(0, grid.n[k2] + 1) * grid.h
    corner = grid.origin + rng.integers(0, 2, size=(n, 3)) * ext
    outside = grid.origin + rng.uniform(-1.0, 2.0, size=(n, 3)) * ext
    return dict(inside=inside, face=face, edge=edge, corner=corner, outside=outside)


def test_pair_is_a_lower_bound_and_within_sqrt3_h_inside():
    rng = np.random.default_rng(5)
    worst = 0.0
    for grid in GRIDS:
        boxes = GN.cubes(grid)
        for kind, pts in _points(grid, rng, 60).items():
            r = rng.uniform(0.0, 0.1, size=pts.shape[0])
            v, vox = GN.sphere_grid(pts, r, grid)
            assert np.all((vox >= 0) & (vox < grid.occ.size))
            d = GN.exact_distance(pts, grid, boxes)
            if not grid.occ.any():
                assert np.all(np.isposinf(v)) and np.all(np.isposinf(d))
                continue
            bound = v + r
            pos = d > 0
            assert np.all(bound[pos] <= d[pos] + EPS), (kind, (bound - d)[pos].max())
            assert np.all(bound[~pos] <= EPS), kind                            # in O: never a positive clearance
            if kind != "outside":
                gap = (np.maximum(d, 0.0) - bound)[pos]
                if gap.size:
                    assert gap.max() <= np.sqrt(3.0) * grid.h + EPS, (kind, gap.max() / grid.h)
                    worst = max(worst, gap.max() / grid.h)
    assert 0.5 < worst <= np.sqrt(3.0)      # (the cases do exercise the slack)


def test_any_voxel_gives_a_lower_bound():
    """the first property for every voxel of the grid, not only the one the index rule picks: a rounded index is never unsound"""
    rng = np.random.default_rng(9)
    grid = next(g for g in GRIDS if g.occ.any() and g.occ.size >= 27)
    pts = grid.origin + rng.uniform(size=(40, 3)) * (grid.hi - grid.origin)
    d = GN.exact_distance(pts, grid)
    nz, ny, nx = grid.occ.shape
    for iz in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                x = grid.origin + (np.array([ix, iy, iz]) + 0.5) * grid.h
                m = 0.5 * grid.h * np.sqrt(float(grid.G[iz, iy, ix])) - np.sqrt(((pts - x) ** 2).sum(axis=1))
                assert np.all(m[d > 0] <= d[d > 0] + EPS)


def test_the_tables_put_the_grid_between_boxes_and_self_pairs():
    names = GN.pair_names(3, 2, 1, GRIDS[0], [(0, 2)])
    assert names[:, 0].tolist() == [CN.WORLD_SPHERE] * 6 + [CN.WORLD_BOX] * 3 + [GN.WORLD_GRID] * 3 + [CN.SELF]
    assert names[9:12, 1].tolist() == [0, 1, 2]
    assert GN.pair_names(3, 2, 1, None, [(0, 2)]).shape[0] == 10


# ---- the references of the motion layer with a grid (shortcut_numpy, plan_numpy, blend_numpy: grid=) -------------------------------------
def test_the_face_predicate_flags_inner_faces_only():
    grid = GN.Grid(np.zeros((4, 4, 4)), (-0.25, 0.5, -1.0), 0.25)
    o, h = grid.origin, grid.h
    at = lambda *p: (o + h * np.array(p))[None]
    assert GN.near_face(at(1.0, 1.5, 2.5), grid) and GN.near_face(at(0.5, 3.0, 0.5), grid) and GN.near_face(at(1.5, 2.5, 1.0 + 0.5e-9), grid)
    assert not GN.near_face(at(1.5, 2.5, 1.0 + 1e-8), grid) and not GN.near_face(at(0.5, 0.5, 0.5), grid)
    # the faces of the box and every centre clamped onto them: the index is 0 or n - 1 whatever the rounding
    assert not GN.near_face(at(0.0, 0.5, 0.5), grid) and not GN.near_face(at(4.0, 0.5, 4.0), grid) and not GN.near_face(at(-3.0, 9.0, 0.5), grid)
    assert GN.near_face(at(-3.0, 9.0, 2.0), grid)
    # [..., ns, 3]: one flag per configuration
    both = np.stack([np.concatenate([at(0.5, 0.5, 0.5), at(1.0, 0.5, 0.5)]), np.concatenate([at(0.5, 0.5, 0.5), at(0.5, 0.5, 0.5)])])
    assert GN.near_face(both, grid).tolist() == [True, False]


def test_grid_none_is_the_reference_without_a_grid(monkeypatch):
    """on the inputs of test_shortcut_numpy, test_plan_numpy and test_blend_numpy: grid=None returns what the call without the keyword
    returns, key by key and bit by bit, and reaches none of grid_numpy's tables"""
    import blend_numpy as BN
    import plan_numpy as PN
    import shortcut_numpy as SN
    import test_blend_numpy as TB
    import test_plan_numpy as TP
    import test_shortcut as TS

    def same(a, b, what):
        assert a.keys() == b.keys(), what
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), (what, k)
            else:
                assert repr(a[k]) == repr(b[k]), (what, k)

    def never(*a, **kw):
        raise AssertionError("grid_numpy's tables reached without a grid")
    for fn in ("advance", "pair_values", "pair_names", "near_face", "sphere_grid"):
        monkeypatch.setattr(GN, fn, never)
    for name in ("panda7", "multidof13"):
        c = TS.shortcut_case(name)
        same(SN.shortcut(c["model"], c["paths"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], grid=None, **c["kw"]), c["want"], "shortcut " + name)
    for name in ("panda7", "talos32"):
        c = TP.plan_case(name)
        same(PN.plan(c["model"], c["start"], c["goal"], c["links"], c["spheres"], c["lo"], c["hi"], TP.T_PLAN, c["ws"], c["wb"], c["pairs"], grid=None, **c["kw"]),
             c["want"], "plan " + name)
    for name in ("panda7", "multidof13"):
        c = TB.blend_case(name)
        args = (c["model"], c["paths"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], c["v_max"], c["a_max"])
        same(BN.blend(*args, S=TB.S_ROWS, grid=None, **c["kw"]), c["want"], "blend " + name)
    # advance_curves on its own, positionally as blend calls it
    c = TB.blend_case("panda7")
    model, paths = c["model"], c["paths"]
    dv = BN.differences(model, paths[0])
    a = (model, paths[0, 1:3], -0.2 * dv[0:2], 0.2 * dv[1:3], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], c["margin"], TB.TOL, TB.MAX_EVALS)
    same(BN.advance_curves(*a, grid=None), BN.advance_curves(*a), "advance_curves")


@pytest.mark.parametrize("name", ["panda7-clear", "panda7"])
def test_what_the_references_certify_is_clear_of_the_geometry(name):
    """panda7 among three spheres, two boxes, its self pairs and a grid: every segment that grid_numpy.advance, shortcut_numpy and
    plan_numpy call FREE and every blend that blend_numpy calls TAKEN, at 257 points, keeps the margin against the spheres, the boxes
    and the union of the occupied cubes themselves (grid_numpy.exact_clearance, motion_numpy.clearance_min): the references are tied
    to the geometry, not to one another.

    panda7-clear: spheres that do not overlap, a margin above zero; the exact clearance is the signed one.  panda7: the sphere model of
    the GPU tests, whose overlapping self pairs put the margin at -0.10, below -r of every sphere.  There a FREE segment may pass through
    an occupied cube, and does: the pair is <= -r inside one and says nothing about the depth (loik_amd_grid.h), so what FREE bounds
    against the cubes is the distance to them, zero inside, less r -- not the depth.  (Segment 64 of grid_cases.motion_case("panda7") has a
    sphere of radius 0.0796 whose centre lies 0.0272 deep in a cube: signed clearance -0.1069 under the margin -0.1041, distance-based
    clearance -0.0796 above it.)"""
    import blend_numpy as BN
    import grid_cases as GC
    import motion_numpy as MN
    import plan_numpy as PN
    ss = np.linspace(0.0, 1.0, 257)
    depth = name == GC.CLEAR

    def clear(c, q, what):
        assert (c["margin"] >= 0.0) == depth
        worst = float(GC.exact_clearance_at(c, q, depth=depth).min())
        assert worst >= c["margin"], (what, worst, c["margin"])
        return worst - c["margin"]
    seen = {}
    c = GC.motion_case(name)
    model = c["model"]
    free = np.flatnonzero(c["want"]["status"] == MN.FREE)
    slack = [clear(c, MN.interpolate_many(model, c["qa"][i], c["dv"][i], ss), ("segment", i)) for i in free]
    seen["segments"] = (free.size, min(slack))
    c = GC.shortcut_case(name)
    ok = [(b, i, j) for (b, i, j), st in zip(c["tried"], c["tried_want"]["status"]) if st == MN.FREE]
    slack = [clear(c, MN.interpolate_many(model, c["paths"][b, i], MN.difference(model, c["paths"][b, i], c["paths"][b, j])[0], ss), ("shortcut", b, i, j))
             for b, i, j in ok]
    seen["shortcuts"] = (len(ok), min(slack))
    c = GC.plan_case(name)
    ok = [(x, y) for b in range(c["B"]) for x, y, st in c["want"]["edges"][b] if st == MN.FREE]
    slack = [clear(c, MN.interpolate_many(model, x, PN.diff(model, x, y), ss), ("edge", k)) for k, (x, y) in enumerate(ok)]
    seen["edges"] = (len(ok), min(slack))
    c = GC.blend_case(name)
    want = c["want"]
    taken = np.argwhere(want["corner_info"][:, :, 0] == BN.TAKEN)
    slack = []
    for b, k in taken:
        P0, P2 = want["controls"][(int(b), int(k) + 1)]
        slack.append(clear(c, np.stack([BN.curve_point(model, c["paths"][b, k + 1], P0, P2, u) for u in ss]), ("blend", b, k)))
    seen["blends"] = (len(taken), min(slack))
    print("grid_numpy certificates %s (count, least exact clearance - margin): %s" % (name, seen))
    assert all(n > 0 for n, _ in seen.values()), seen
