"""GPU: the clearance query with a voxel world (include/loik_amd_grid.h) against the numpy reference of tests/grid_numpy.py (proven on the CPU
by test_grid_numpy.py): three robots (tree330 takes the placements from HBM) in a world that has spheres, boxes and a grid at once, the
sphere counts at which the kernel changes its path, centres exactly on a voxel face, on the grid's boundary and outside it, a NaN row,
the bound against the exact distance to the union of the cubes, neutrality of a grid that was set and cleared, and the validation."""
import ctypes as C

import numpy as np
import pytest

from loik_amd import capi

from test_clearance import BOUND, _case, _open, _raises, _world
import clearance_numpy as CN
import grid_numpy as GN
import qp_cases as QC

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -20, -24
ROBOTS = ("panda7", "talos32", "tree330")
_CASES = {}


def _grid(seed, dims=(25, 21, 17), h=0.06, frac=0.002):
    """a sparse grid centred near the robot's base: most centres of the arms inside, some outside; a few dozen occupied voxels, so that
    some configurations are clear of the cubes and some are not"""
    occ = GN.random_occupancy(dims, frac, seed)
    return GN.Grid(occ, -0.5 * h * np.array(dims, dtype=float) + np.array([0.013, -0.021, 0.2]), h)


def _set(s, grid):
    s.set_collision_grid(grid.occ, grid.origin, grid.h)


def case(name):
    """the model, q, spheres and pairs of test_clearance._case, a world of three spheres and two boxes, a grid, and the numpy answer"""
    if name not in _CASES:
        c = dict(_case(name))
        c["ws"], c["wb"] = _world(np.random.default_rng(900), 3, 2)
        c["grid"] = _grid(901 + ROBOTS.index(name))
        c["want"] = GN.clearance(c["model"], c["q"], c["links"], c["spheres"], c["ws"], c["wb"], c["grid"], c["pairs"])
        _CASES[name] = c
    return _CASES[name]


def _voxel_value(c, r, grid, vox):
    """the pair's value with the voxel `vox` read"""
    n = grid.n
    i = np.array([vox % n[0], (vox // n[0]) % n[1], vox // (n[0] * n[1])])
    p = np.minimum(np.maximum(c, grid.origin), grid.hi)
    x = grid.origin + (i + 0.5) * grid.h
    Gv = grid.G[i[2], i[1], i[0]]
    m = np.inf if Gv == GN.EMPTY else 0.5 * grid.h * np.sqrt(float(Gv)) - np.sqrt(((p - x) ** 2).sum())
    dout = np.sqrt(((c - p) ** 2).sum())
    return (np.sqrt(dout * dout + max(m, 0.0) ** 2) if dout > 0 else m) - r


def _compare(got, want, spheres, grid, what):
    """the three minima within BOUND * scale; the witness names a pair (of kind 4: a voxel of the grid) whose value is the minimum;
    min == min(min_world, min_self) exactly.  Returns the number of witnesses of kind 4"""
    scale = 1.0 + float(np.max(np.abs(want["centres"]))) + float(np.max(spheres[:, 3]))
    for key in ("min", "min_world", "min_self"):
        g, w = got[key], want[key]
        inf = np.isposinf(w)
        assert np.array_equal(np.isposinf(g), inf), (what, key)
        err = float(np.max(np.abs(g[~inf] - w[~inf]), initial=0.0))
        print("grid_measured %s %s: max |got - numpy| %.3e, scale %.3f, relative %.3e" % (what, key, err, scale, err / scale))
        assert err <= BOUND * scale, (what, key, err, scale)
    assert np.array_equal(got["min"], np.minimum(got["min_world"], got["min_self"]))
    names, seen = want["names"], 0
    for i in range(want["min"].size):
        kind, a, b = (int(v) for v in got["witness"][i])
        if kind == GN.WORLD_GRID:
            seen += 1
            assert 0 <= a < spheres.shape[0] and 0 <= b < grid.occ.size
            v = _voxel_value(want["centres"][i, a], spheres[a, 3], grid, b)
        else:
            k = np.flatnonzero((names[:, 0] == kind) & (names[:, 1] == a) & (names[:, 2] == b))
            assert k.size == 1, (what, i, kind, a, b)
            v = want["values"][i, k[0]]
        assert abs(v - want["min"][i]) <= BOUND * scale, (what, i, kind, a, b)
    return seen


# ---- 1. against numpy, spheres, boxes and a grid at once ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROBOTS)
def test_clearance_with_a_grid_matches_numpy(name):
    c = case(name)
    s = _open(c["model"], c["q"])
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    _set(s, c["grid"])
    got, again = s.clearance(), s.clearance()
    seen = _compare(got, c["want"], c["spheres"], c["grid"], name)
    print("grid_measured %s: %d of %d witnesses are grid pairs" % (name, seen, c["n"]))
    assert all(np.array_equal(got[k], again[k]) for k in got)      # two launches, the same bits
    # the grid alone: every witness is a grid pair and names its voxel; the device's value is a lower bound of the exact distance to the
    # union of the cubes
    s.set_collision_world(None, None)
    s.set_self_collision(False)
    alone = s.clearance()
    want_alone = GN.clearance(c["model"], c["q"], c["links"], c["spheres"], grid=c["grid"])
    assert _compare(alone, want_alone, c["spheres"], c["grid"], name + " grid alone") == c["n"]
    assert np.all(np.isposinf(alone["min_self"])) and np.array_equal(alone["min"], alone["min_world"])
    exact = GN.exact_clearance(c["model"], c["q"], c["links"], c["spheres"], c["grid"])
    scale = 1.0 + float(np.max(np.abs(c["want"]["centres"]))) + float(np.max(c["spheres"][:, 3]))
    out = exact > 0
    print("grid_measured %s: exact - device over the %d configurations clear of the cubes: %.4f .. %.4f (h %.2f)" % (
        name, int(out.sum()), float((exact - alone["min"])[out].min(initial=np.inf)), float((exact - alone["min"])[out].max(initial=-np.inf)), c["grid"].h))
    assert np.all(alone["min"][out] <= exact[out] + BOUND * scale)
    assert np.all(alone["min"][~out] <= BOUND * scale)
    s.close()


# ---- 2. the sizes at which the kernel changes its path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 63, 64, 65, 130])
def test_sizes(ns):
    """panda7, the spheres dealt round-robin to the links 0..7 (the universe included), one world sphere, one box, the grid, self pairs on;
    65 resident configurations (a last workgroup with idle wavefronts) and 3 explicit ones"""
    model = QC.model_of("panda7")
    rng = np.random.default_rng(920 + ns)
    q = model.random_configurations(rng, 65)
    links = np.arange(ns, dtype=np.int32) % model.njoints
    _, spheres = CN.make_spheres(model, 1, 930 + ns, links=links)
    pairs = CN.self_pairs(model.parents, links)
    ws, wb = _world(rng, 1, 1)
    grid = _grid(940 + ns)
    s = _open(model, q)
    s.set_collision_spheres(links, spheres)
    s.set_collision_world(ws, wb)
    s.set_self_collision(True)
    _set(s, grid)
    for rows in (q, q[:3]):
        want = GN.clearance(model, rows, links, spheres, ws, wb, grid, pairs)
        _compare(s.clearance(None if rows is q else rows), want, spheres, grid, "ns=%d n=%d" % (ns, rows.shape[0]))
    # the grid alone: every witness is a grid pair
    s.set_collision_world(None, None)
    s.set_self_collision(False)
    assert _compare(s.clearance(), GN.clearance(model, q, links, spheres, grid=grid), spheres, grid, "ns=%d grid alone" % ns) == 65
    s.close()


# ---- 3. centres on a voxel face, on the boundary, outside -----------------------------------------------------------------------------------
def test_exact_centres_on_faces_boundary_and_outside():
    """a sphere on the universe has its offset as its world centre, exactly: the device and numpy read the same voxel and agree to
    rounding where the bound jumps from one voxel to the next"""
    model = QC.model_of("panda7")
    q = model.random_configurations(np.random.default_rng(950), 1)
    occ = np.zeros((4, 4, 4), dtype=np.uint8)
    occ[1, 2, 3] = occ[0, 0, 0] = occ[3, 3, 0] = 1
    grid = GN.Grid(occ, (-0.25, 0.5, -1.0), 0.25)          # (every face is a binary fraction: the products are exact)
    o, h = grid.origin, grid.h
    pts = [o + h * np.array(p) for p in ((1.0, 1.5, 2.5), (2.0, 3.0, 0.5), (3.0, 2.0, 1.0), (0.0, 0.3, 0.3), (4.0, 4.0, 4.0), (4.0, 2.5, 1.5),
                                         (0.0, 0.0, 0.0), (-0.5, 1.0, 1.0), (5.0, 6.0, -1.0), (2.5, 2.5, 9.0), (3.5, 2.5, 1.5), (3.75, 2.5, 1.0))]
    s = _open(model, q)
    _set(s, grid)
    for c in pts:
        sph = np.array([[c[0], c[1], c[2], 0.05]])
        s.set_collision_spheres([0], sph)
        got = s.clearance()
        v, vox = GN.sphere_grid(c, 0.05, grid)
        assert tuple(got["witness"][0]) == (capi.CLR_WORLD_GRID, 0, int(vox)), (c, got["witness"][0], vox)
        assert abs(got["min"][0] - v) <= BOUND * (1.0 + np.abs(c).max()) and got["min"][0] == got["min_world"][0], (c, got["min"][0], v)
        d = GN.exact_distance(c, grid)
        assert got["min"][0] + 0.05 <= max(d, 0.0) + BOUND * 10
    # an empty grid: +inf, and the pair is still the witness (the lowest ordinal among equals)
    s.set_collision_grid(np.zeros((2, 2, 2)), (0, 0, 0), 1.0)
    got = s.clearance()
    assert np.isposinf(got["min"][0]) and np.isposinf(got["min_world"][0]) and got["witness"][0, 0] == capi.CLR_WORLD_GRID
    s.close()


# ---- 4. a NaN row ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["panda7", "tree330"])
def test_a_nan_row_is_nan_and_alone(name):
    c = case(name)
    q = c["q"].copy()
    q[1, q.shape[1] // 2] = np.nan
    s = _open(c["model"], q)
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    _set(s, c["grid"])
    got = s.clearance()
    assert all(np.isnan(got[k][1]) for k in ("min", "min_world", "min_self")) and tuple(got["witness"][1]) == (CN.NONE, -1, -1)
    want = c["want"]
    rest = np.arange(q.shape[0]) != 1
    scale = 1.0 + float(np.max(np.abs(want["centres"]))) + float(np.max(c["spheres"][:, 3]))
    assert np.all(np.abs(got["min"][rest] - want["min"][rest]) <= BOUND * scale)
    s.close()


# ---- 5. neutrality ---------------------------------------------------------------------------------------------------------------------------
def test_a_grid_set_and_cleared_leaves_a_fresh_handle():
    import test_plan as TPL
    c = TPL.case("panda7")
    fresh, used = TPL.TM._open(c), TPL.TM._open(c)
    _set(used, _grid(960, frac=0.5))      # (dense: it decides minima even in the crowded world of that case)
    assert used.collision_grid(field=False)["dims"] == (25, 21, 17)
    with_grid = used.clearance(c["q"])
    used.set_collision_grid(None)
    dv = 0.3 * np.random.default_rng(961).uniform(-1.0, 1.0, size=(c["q"].shape[0], c["model"].nv))
    a, b = fresh.clearance(c["q"]), used.clearance(c["q"])
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["min"], with_grid["min"])       # (the grid did matter while it was set)
    a, b = (h.motion_clearance(c["q"], dv=dv, margin=c["margin"], tol=1e-3, max_evals=12) for h in (fresh, used))
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    a, b = (TPL._plan(h, c) for h in (fresh, used))
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    fresh.close(); used.close()


# ---- 6. the validation -----------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_model_as_it_was():
    c = case("panda7")
    model, q, grid = c["model"], c["q"], c["grid"]
    s = _open(model, q)
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    _set(s, grid)
    before, field = s.clearance(), s.collision_grid()
    L, h = s.L, s.h
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    occ = np.ones(8, dtype=np.uint8)
    org = np.zeros(3)

    def call(occ_p, dims, origin, edge, flags=0, handle=h):
        d = None if dims is None else np.array(dims, dtype=np.int32)
        o = None if origin is None else np.array(origin, dtype=float)
        return L.loikb_collision_set_world_grid(handle, occ_p, None if d is None else d.ctypes.data_as(ip), None if o is None else o.ctypes.data_as(dp),
                                                edge, flags)
    op = occ.ctypes.data_as(vp)
    assert call(op, (2, 2, 2), org, 0.1, handle=None) == ERR_ARG
    assert call(op, None, org, 0.1) == ERR_ARG and call(op, (2, 2, 2), None, 0.1) == ERR_ARG
    for dims in ((0, 2, 2), (2, -1, 2), (2, 2, 513), (513, 1, 1)):
        assert call(op, dims, org, 0.1) == ERR_ARG and b"dimension" in L.loikb_last_error(), dims
    assert call(op, (512, 512, 512), org, 0.1) == ERR_ARG and b"voxels" in L.loikb_last_error()      # 2^27 voxels: refused before occ is read
    for bad in (np.nan, np.inf, -np.inf):
        assert call(op, (2, 2, 2), (0.0, bad, 0.0), 0.1) == ERR_ARG and b"origin" in L.loikb_last_error()
        assert call(op, (2, 2, 2), org, bad) == ERR_ARG and b"edge" in L.loikb_last_error()
    assert call(op, (2, 2, 2), org, 0.0) == ERR_ARG and call(op, (2, 2, 2), org, -0.1) == ERR_ARG
    assert call(op, (2, 2, 2), org, 0.1, flags=2) == ERR_ARG and call(op, (2, 2, 2), org, 0.1, flags=3) == ERR_ARG
    out = np.empty(3, dtype=np.int32)
    assert L.loikb_collision_get_world_grid(h, out.ctypes.data_as(ip), None, None, None, 2) == ERR_ARG
    # ... and after all of it the grid and the answers are what they were
    after, field2 = s.clearance(), s.collision_grid()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    assert field2["dims"] == field["dims"] and field2["voxel"] == field["voxel"] and np.array_equal(field2["G"], field["G"])
    # avoidance does not read a grid, and says so
    lb, ub = -np.ones(model.nv), np.ones(model.nv)
    few = np.arange(8, dtype=np.int32) % model.njoints
    s.set_self_collision(False)
    s.set_collision_spheres(few, CN.make_spheres(model, 1, 970, links=few)[1])
    _raises(ERR_STATE, "grid", s.set_collision_avoidance, 0.01, 0.1)
    _raises(ERR_STATE, "grid", s.clearance_gradient, q)
    _raises(ERR_STATE, "grid", s.avoidance_box, q, 0.01, lb, ub, 0.01, 0.1)
    assert s.collision_avoidance() is None
    s.clear_collision_avoidance()        # (NULL parameters clear the latch whatever is set)
    # they work again once the grid is cleared; and the latch refuses a grid
    s.set_collision_grid(None)
    assert s.clearance_gradient(q)["grad"].shape == (q.shape[0], model.nv)
    assert s.avoidance_box(q, 0.01, lb, ub, 0.01, 0.1)["lo"].shape == (q.shape[0], model.nv)
    s.set_collision_avoidance(0.01, 0.1)
    _raises(ERR_STATE, "avoidance", _set, s, grid)
    assert s.collision_grid() is None
    s.clear_collision_avoidance()
    _set(s, grid)
    assert s.collision_grid(field=False)["dims"] == field["dims"]
    s.close()
