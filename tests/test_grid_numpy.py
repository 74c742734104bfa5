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
