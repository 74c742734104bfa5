"""GPU: include/loik_amd_gridnear.h against the numpy reference of tests/gridnear_numpy.py (proven on the CPU by test_gridnear_numpy.py):
the transform that loikb_collision_grid_set_nearest builds, exactly; the query; loikb_clearance_gradient and loikb_avoid_box with the grid
as one more world object on three robots (tree330 takes its placements from HBM); neutrality of the latch, the routes, a caller's stream
and the validation.  The pose loops are in test_gridnear_pose.py."""
import ctypes as C

import numpy as np
import pytest

from loik_amd import capi

from test_avoid_box import BOX_BOUND, DT, GRAD_BOUND, PRM, _back, _err, _ints, _rel, _scale
from test_clearance import BOUND, _open
from test_grid_build import _DeviceBytes
import clearance_numpy as CN
import grid_numpy as GN
import gridnear_cases as GC
import gridnear_numpy as NN
import qp_cases as QC
import stream_harness as H
from test_gridnear_numpy import FD_REL, fd_rows

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -20, -24
ORIGIN, VOXEL = (0.1, -0.2, 0.3), 0.05
_S = {}


def _solver():
    """one handle for the build tests: the grid and the latch are set afresh by every test"""
    if "s" not in _S:
        model = QC.model_of("panda7")
        _S["s"] = _open(model, model.random_configurations(np.random.default_rng(1), 2))
    s = _S["s"]
    s.set_collision_grid(None)
    s.set_collision_grid_nearest(False)
    return s


# ---- 1. the build -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GC.BUILD)
def test_transform_equals_brute_force(name):
    occ = GC.build_occupancy(name)
    G, F = GC.build_want(name)
    s = _solver()
    s.set_collision_grid(occ, ORIGIN, VOXEL)
    assert s.collision_grid_nearest() is None
    plain = s.collision_grid()["G"]
    assert np.array_equal(plain, G)
    s.set_collision_grid_nearest(True)                 # grid first, then the latch
    got = s.collision_grid_nearest()
    assert got.dtype == np.uint32 and got.shape == occ.shape
    assert np.array_equal(got, F), "%d voxels differ" % int((got != F).sum())
    assert np.array_equal(s.collision_grid()["G"], plain)   # the latch leaves G alone
    s.set_collision_grid(None)
    assert s.collision_grid_nearest() is None
    s.set_collision_grid(occ, ORIGIN, VOXEL)           # latch first, then the grid
    assert np.array_equal(s.collision_grid_nearest(), F) and np.array_equal(s.collision_grid()["G"], plain)
    s.set_collision_grid(_DeviceBytes(occ), ORIGIN, VOXEL)   # a device occupancy
    assert np.array_equal(s.collision_grid_nearest(), F) and np.array_equal(s.collision_grid()["G"], plain)


def test_failed_set_off_and_on_again():
    s = _solver()
    occ, other = GC.build_occupancy("5x4x3"), GC.build_occupancy("65x33x3")
    F, F2 = GC.build_want("5x4x3")[1], GC.build_want("65x33x3")[1]
    s.set_collision_grid_nearest(True)
    s.set_collision_grid(occ, ORIGIN, VOXEL)
    G = s.collision_grid()["G"]
    dims = np.array([0, 4, 3], dtype=np.int32)
    org = np.array(ORIGIN)
    rc = s.L.loikb_collision_set_world_grid(s.h, occ.ctypes.data_as(C.c_void_p), dims.ctypes.data_as(C.POINTER(C.c_int)), org.ctypes.data_as(C.POINTER(C.c_double)), VOXEL, 0)
    assert rc == ERR_ARG
    _err(lambda: s.set_collision_grid(occ, ORIGIN, -1.0), ERR_ARG)
    assert np.array_equal(s.collision_grid_nearest(), F) and np.array_equal(s.collision_grid()["G"], G)
    s.set_collision_grid(other, ORIGIN, VOXEL)         # a larger grid, then the first again: the two buffers change places
    assert np.array_equal(s.collision_grid_nearest(), F2)
    s.set_collision_grid(occ, ORIGIN, VOXEL)
    assert np.array_equal(s.collision_grid_nearest(), F)
    s.set_collision_grid_nearest(False)
    assert s.collision_grid_nearest() is None and np.array_equal(s.collision_grid()["G"], G)
    s.set_collision_grid_nearest(True)                 # off, then on: rebuilt
    assert np.array_equal(s.collision_grid_nearest(), F)
    # into a device buffer
    dev = capi.DeviceArray(np.zeros((occ.size + 1) // 2))
    assert s.L.loikb_collision_grid_get_nearest(s.h, C.c_void_p(dev.data_ptr()), capi.OUT_DEVICE) == 1
    assert np.array_equal(_back(dev, occ.shape, np.uint32), F)
    dev.free()
    for bad in (2, -1):
        _err(lambda: s.set_collision_grid_nearest(bad), ERR_ARG)
    assert s.L.loikb_collision_grid_get_nearest(s.h, None, 2) == ERR_ARG and s.L.loikb_collision_grid_set_nearest(None, 1) == ERR_ARG
    assert s.L.loikb_collision_grid_get_nearest(None, None, 0) == 0
    assert np.array_equal(s.collision_grid_nearest(), F)


# ---- 2. the query -----------------------------------------------------------------------------------------------------------------------
def _grid_handle(grid):
    s = _solver()
    s.set_collision_grid_nearest(True)
    s.set_collision_grid(grid.occ, grid.origin, grid.h)
    return s


def test_query_matches_numpy():
    grid, sph = GC.query_grid(), GC.query_spheres()
    want = NN.query(sph, grid)
    s = _grid_handle(grid)
    got = s.grid_nearest(sph)
    keep = ~want["near"]
    assert np.array_equal(got["vox"][keep], want["vox"][keep])
    scale = 1.0 + float(np.max(np.abs(sph[:, :3]))) + float(np.max(sph[:, 3]))
    ev, en = float(np.max(np.abs(got["val"][keep] - want["val"][keep]))), float(np.max(np.abs(got["normal"][keep] - want["normal"][keep])))
    print("gridnear_measured query: max |val - numpy| %.3e, |normal - numpy| %.3e, scale %.3f, %d of %d near left out" % (ev, en, scale, int((~keep).sum()), sph.shape[0]))
    assert ev <= BOUND * scale and en <= BOUND * scale
    # the device route, and a NaN row among good ones
    dsph = capi.DeviceArray(sph)
    outs = (capi.DeviceArray(np.zeros((sph.shape[0], 2))), _ints(2 * sph.shape[0]), capi.DeviceArray(np.zeros((sph.shape[0], 3))))
    s.grid_nearest(dsph, out=outs)
    assert np.array_equal(_back(outs[0], got["val"].shape), got["val"]) and np.array_equal(_back(outs[1], got["vox"].shape, np.int32), got["vox"])
    assert np.array_equal(_back(outs[2], got["normal"].shape), got["normal"])
    for a in outs + (dsph,):
        a.free()
    bad = np.array(sph[:5])
    bad[1, 2], bad[3, 3] = np.nan, np.inf
    gb = s.grid_nearest(bad)
    for k in ("val", "vox", "normal"):
        assert np.array_equal(gb[k][[0, 2, 4]], got[k][[0, 2, 4]])
    assert np.all(np.isnan(gb["val"][[1, 3]])) and np.all(gb["vox"][[1, 3]] == -1) and np.all(np.isnan(gb["normal"][[1, 3]]))


def test_query_on_planes_boundary_and_outside():
    """exactly on a voxel face, on a mid-plane, on the grid's boundary and outside: the device's answer is the reference's for the centre
    itself or for one moved by a hair across the planes it lies on"""
    grid, sph = GC.query_grid(), GC.plane_spheres()
    s = _grid_handle(grid)
    got = s.grid_nearest(sph)
    scale = 1.0 + float(np.max(np.abs(sph[:, :3]))) + float(np.max(sph[:, 3]))
    tiny = 1e-7 * grid.h
    for i in range(sph.shape[0]):
        ok = False
        for shift in np.array(np.meshgrid([0.0, -tiny, tiny], [0.0, -tiny, tiny], [0.0, -tiny, tiny])).reshape(3, -1).T:
            w = NN.query(np.concatenate([sph[i, :3] + shift, sph[i, 3:]])[None], grid)
            if np.array_equal(w["vox"][0], got["vox"][i]) and np.all(np.abs(w["val"][0] - got["val"][i]) <= 1e-6 * grid.h + BOUND * scale) \
                    and np.all(np.abs(w["normal"][0] - got["normal"][i]) <= 1e-5):
                ok = True
                break
        assert ok, (i, sph[i], got["vox"][i], got["val"][i])
        v, u = got["vox"][i]
        assert 0 <= v < grid.occ.size and grid.occ.ravel()[u]


def test_ties_and_inside_a_cube():
    for grid, sph, winner, inside_n in GC.tie_case():
        s = _grid_handle(grid)
        got, want = s.grid_nearest(sph), NN.query(sph, grid)
        assert np.array_equal(got["vox"], want["vox"]) and np.array_equal(got["vox"][:, 1], winner)
        assert np.array_equal(got["val"], want["val"]) and np.array_equal(got["normal"], want["normal"])   # binary coordinates: exact
        assert np.array_equal(got["normal"][3:], inside_n)
    empty = NN.Grid(np.zeros((3, 4, 5), dtype=np.uint8), (0.0, 0.0, 0.0), 0.25)
    s = _grid_handle(empty)
    got = s.grid_nearest(np.array([[0.3, 0.2, 0.1, 0.05], [5.0, 5.0, 5.0, 0.0]]))
    assert np.all(np.isposinf(got["val"])) and np.all(got["vox"][:, 1] == -1) and np.all(got["vox"][:, 0] >= 0) and not got["normal"].any()
    assert np.all(s.collision_grid_nearest() == capi.GRID_NO_VOXEL)


# ---- 3. gradient and box ----------------------------------------------------------------------------------------------------------------
def _open_case(c, latch=True):
    s = _open(c["model"], c["q"])
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(len(c["pairs"]) > 0)
    if latch:
        s.set_collision_grid_nearest(True)
    g = c["grid"]
    s.set_collision_grid(g.occ, g.origin, g.h)
    return s


@pytest.mark.parametrize("name", GC.ROBOTS)
def test_gradient_and_box_match_numpy(name):
    c = GC.avoid_case(name)
    s = _open_case(c)
    want, wg = c["box"], c["grad"]
    scale = _scale(want["centres"], c["spheres"])
    # the gradient: the minima and the witness of clearance() on the same handle, bit for bit
    gg, plain = s.clearance_gradient(), s.clearance()
    for k in ("min", "min_world", "min_self", "witness"):
        assert np.array_equal(gg[k], plain[k]), (name, k)
    kg = ~wg["near"]
    assert (~kg).mean() <= GC.NEAR_SHARE
    assert np.array_equal(gg["witness"][kg], wg["witness"][kg])
    eg = float(np.max(np.abs(gg["grad"][kg] - wg["grad"][kg]))) / scale
    print("gridnear_measured %s gradient: max |grad - numpy| / scale %.3e, scale %.3f, %d grid witnesses" % (name, eg, scale, int((gg["witness"][:, 0] == GN.WORLD_GRID).sum())))
    assert eg <= GRAD_BOUND, (name, eg)
    # the box over an unbounded base
    got = s.avoidance_box(None, DT, -np.inf, np.inf, **PRM)
    keep = ~want["near"]
    assert (~keep).mean() <= GC.NEAR_SHARE
    inf = np.isposinf(want["pairs"][keep])   # (a row left out may have a sphere on a voxel face, where the bound jumps)
    assert np.array_equal(np.isposinf(got["pairs"][keep]), inf)
    e = float(np.max(np.abs(got["pairs"][keep][~inf] - want["pairs"][keep][~inf]), initial=0.0))
    assert e <= BOUND * scale, (name, e, scale)
    assert np.array_equal(got["partner"][keep], want["partner"][keep])
    nwo = c["ws"].shape[0] + c["wb"].shape[0]
    assert (got["partner"][:, :, 0] == nwo).any()
    assert np.all(got["lo"] <= 0.0) and np.all(got["hi"] >= 0.0)
    mask = keep[:, None] & ~want["tiny"]     # (gridnear_numpy.constraints: a derivative that is 0 by structure)
    worst = max(_rel(got["lo"][mask], want["lo"][mask], name), _rel(got["hi"][mask], want["hi"][mask], name))
    print("gridnear_measured %s box: max relative error %.3e over %d rows (%d left out, %d entries 0 by structure), clearances %.3e / scale %.3f" %
          (name, worst, int(keep.sum()), int((~keep).sum()), int(want["tiny"].sum()), e, scale))
    assert worst <= BOX_BOUND, (name, worst)
    sub = s.avoidance_box(c["q"][:3], DT, -np.inf, np.inf, **PRM)
    assert all(np.array_equal(sub[k], got[k][:3]) for k in got)
    s.close()
    # the handle that never latched the transform still refuses all three
    u = _open_case(c, latch=False)
    for fn in (lambda: u.set_collision_avoidance(**PRM), lambda: u.clearance_gradient(), lambda: u.avoidance_box(None, DT, -1.0, 1.0, **PRM)):
        msg = _err(fn, ERR_STATE)
        assert "grid" in msg and "avoidance" in msg and "loikb_collision_grid_set_nearest" in msg
    u.close()


def _check_with_grid(s, inp, ref):
    """test_avoid_box._check_against_numpy with the grid: the box and the gradient of the handle's resident q against ref = dict(box,
    grad) of gridnear_numpy, under the bounds and with the rows and entries left out as in test_gradient_and_box_match_numpy; the minima
    and the witness of clearance() bit for bit; 3 and 1 of the rows bit for bit.  Returns (box, gradient) of the device"""
    what, q, spheres = inp["what"], inp["q"], inp["spheres"]
    want, wg = ref["box"], ref["grad"]
    scale = _scale(want["centres"], spheres)
    gg, plain = s.clearance_gradient(), s.clearance()
    for k in ("min", "min_world", "min_self", "witness"):
        assert np.array_equal(gg[k], plain[k]), (what, k)
    kg, keep = ~wg["near"], ~want["near"]
    assert np.array_equal(gg["witness"][kg], wg["witness"][kg]), what
    assert np.all(np.abs(gg["min"][kg] - wg["min"][kg]) <= BOUND * scale), what
    eg = float(np.max(np.abs(gg["grad"][kg] - wg["grad"][kg]), initial=0.0)) / scale
    assert eg <= GRAD_BOUND, (what, eg)
    got = s.avoidance_box(None, DT, -np.inf, np.inf, **PRM)
    inf = np.isposinf(want["pairs"][keep])
    assert np.array_equal(np.isposinf(got["pairs"][keep]), inf), what
    e = float(np.max(np.abs(got["pairs"][keep][~inf] - want["pairs"][keep][~inf]), initial=0.0))
    assert e <= BOUND * scale, (what, e, scale)
    assert np.array_equal(got["partner"][keep], want["partner"][keep]), what
    assert np.all(got["lo"] <= 0.0) and np.all(got["hi"] >= 0.0), what
    mask = keep[:, None] & ~want["tiny"]
    worst = max(_rel(got["lo"][mask], want["lo"][mask], what), _rel(got["hi"][mask], want["hi"][mask], what))
    print("gridnear_measured %s: box max relative error %.3e, gradient %.3e / scale, clearances %.3e / scale %.3f, left out %d + %d rows, %d grid witnesses"
          % (what, worst, eg, e, scale, int((~keep).sum()), int((~kg).sum()), int((gg["witness"][:, 0] == GN.WORLD_GRID).sum())))
    assert worst <= BOX_BOUND, (what, worst)
    for n in (3, 1):   # an explicit q, n != B: a last workgroup with idle wavefronts
        sub, subg = s.avoidance_box(q[:n], DT, -np.inf, np.inf, **PRM), s.clearance_gradient(q[:n])
        assert all(np.array_equal(sub[k], got[k][:n]) for k in got), (what, n)
        assert all(np.array_equal(subg[k], gg[k][:n]) for k in gg), (what, n)
    return got, gg


@pytest.mark.parametrize("ns", GC.SIZE_NS)
def test_sizes_with_a_grid(ns):
    """test_avoid_box.test_sizes with a grid latched: 2^lp = 1, 2, 4 and 64 sphere slots a wavefront, partial last trips, and the worlds in
    which the grid's ordinal arithmetic degenerates -- the grid alone (nws == nwb == 0), one kind of object missing -- self pairs off
    and on; a grid witness in every world (test_gridnear_numpy.test_size_inputs_with_a_grid says so of the reference)"""
    inputs = GC.size_inputs(ns)
    model, q, links, spheres, g = (inputs[0][k] for k in ("model", "q", "links", "spheres", "grid"))
    s = _open(model, q)
    s.set_collision_spheres(links, spheres)
    s.set_collision_grid_nearest(True)
    s.set_collision_grid(g.occ, g.origin, g.h)
    for inp in inputs:
        s.set_collision_world(inp["ws"], inp["wb"])
        s.set_self_collision(inp["self_on"])
        got, gg = _check_with_grid(s, inp, GC.size_ref(inp))
        assert (gg["witness"][:, 0] == GN.WORLD_GRID).any(), inp["what"]
        nwo = inp["ws"].shape[0] + inp["wb"].shape[0]
        assert (got["partner"][:, :, 0] == nwo).any(), inp["what"]
        if not inp["self_on"]:
            assert np.all(np.isposinf(got["pairs"][:, :, 1])) and np.all(got["partner"][:, :, 1] == -1)
        if inp["split"] == (0, 0):   # the grid is every sphere's only world object
            assert np.all(got["partner"][:, :, 0] == 0) and np.isfinite(got["pairs"][:, :, 0]).all()
    s.close()


def test_the_robot_leaves_the_grids_box():
    """half the extent: most centres lie outside the grid's box and are clamped into it (the dout > 0 branch of clr_sphere_grid, clamped
    indices among the candidates of gridnear_cube)"""
    c = GC.half_grid_case()
    s = _open_case(c)
    got, gg = _check_with_grid(s, dict(c, what="panda7 half grid"), c)
    nwo = c["ws"].shape[0] + c["wb"].shape[0]
    assert (c["outside"] & (got["partner"][:, :, 0] == nwo)).any() and (gg["witness"][:, 0] == GN.WORLD_GRID).any()
    s.close()


def test_an_empty_grid_under_the_latch():
    """no voxel occupied: every grid pair is +inf (loik_amd_gridnear.h).  Beside other world objects it is never a partner nor the
    witness, and box, table and gradient are those of a handle without a grid, bit for bit.  With nothing else in the world it is each
    sphere's partner at +inf, narrows nothing, and is the witness only of a configuration with no other pair at all"""
    c = GC.empty_grid_case()
    s, t = _open_case(c), _open_case(c, latch=False)
    t.set_collision_grid(None)
    for world in (True, False):
        if not world:
            for h in (s, t):
                h.set_collision_world(np.zeros((0, 4)), np.zeros((0, 15)))
        a, b = s.avoidance_box(None, DT, -np.inf, np.inf, **PRM), t.avoidance_box(None, DT, -np.inf, np.inf, **PRM)
        ga, gb, pa = s.clearance_gradient(), t.clearance_gradient(), s.clearance()
        assert all(np.array_equal(ga[k], pa[k]) for k in ("min", "min_world", "min_self", "witness"))
        for k in ("lo", "hi", "pairs"):
            assert np.array_equal(a[k], b[k]), (world, k)
        assert all(np.array_equal(ga[k], gb[k]) for k in ga), world   # (self pairs: never the grid)
        assert np.array_equal(a["partner"][:, :, 1], b["partner"][:, :, 1])
        if world:
            assert np.array_equal(a["partner"], b["partner"]) and np.isfinite(a["lo"]).any()
        else:
            assert np.all(np.isposinf(a["pairs"][:, :, 0])) and np.all(a["partner"][:, :, 0] == 0) and np.all(b["partner"][:, :, 0] == -1)
    for h in (s, t):
        h.set_self_collision(False)
    ga, gb, pa = s.clearance_gradient(), t.clearance_gradient(), s.clearance()
    assert all(np.array_equal(ga[k], pa[k]) for k in ("min", "min_world", "min_self", "witness"))
    assert np.all(np.isposinf(ga["min"])) and np.all(np.isposinf(gb["min"])) and not ga["grad"].any() and not gb["grad"].any()
    g = c["grid"]
    vox = GN.sphere_grid(CN.centres(c["model"], c["q"], c["links"][:1], c["spheres"][:1])[:, 0], c["spheres"][0, 3], g)[1]
    assert np.all(gb["witness"] == (CN.NONE, -1, -1)) and np.all(ga["witness"][:, 0] == GN.WORLD_GRID) and np.all(ga["witness"][:, 1] == 0)
    keep = ~GN.near_face(CN.centres(c["model"], c["q"], c["links"][:1], c["spheres"][:1]), g)
    assert keep.mean() >= 0.9 and np.array_equal(ga["witness"][keep, 2], vox[keep])
    a = s.avoidance_box(None, DT, -1.0, 1.0, **PRM)
    assert np.all(a["lo"] == -1.0) and np.all(a["hi"] == 1.0)
    s.close(); t.close()


def test_gradient_is_the_derivative_of_the_distance_to_the_chosen_cube():
    c = GC.fd_case()
    s = _open_case(c)
    got = s.clearance_gradient()
    want = c["grad"]
    rows = fd_rows(c, want)
    assert len(rows) >= 20
    worst = 0.0
    for i, a, u, fd in rows:
        assert tuple(got["witness"][i][:2]) == (GN.WORLD_GRID, a)
        err = float(np.max(np.abs(got["grad"][i] - fd))) / float(np.max(np.abs(fd)))
        worst = max(worst, err)
        assert err <= FD_REL, (i, a, u, err)
    print("gridnear_measured finite differences: %d rows, max |g - fd| / max |fd| %.3e" % (len(rows), worst))
    s.close()


# ---- 5. neutrality, routes, a caller's stream, validation --------------------------------------------------------------------------------
def test_latch_on_and_off_leaves_a_fresh_handle():
    c = dict(GC.avoid_case("panda7"))
    fresh = _open(c["model"], c["q"])
    fresh.set_collision_spheres(c["links"], c["spheres"])
    fresh.set_collision_world(c["ws"], c["wb"])
    fresh.set_self_collision(True)
    want = (fresh.avoidance_box(None, DT, -1.0, 1.0, **PRM), fresh.clearance_gradient())
    fresh.close()
    s = _open_case(c)
    with_grid = s.avoidance_box(None, DT, -1.0, 1.0, **PRM)
    assert not np.array_equal(with_grid["pairs"], want[0]["pairs"])
    s.set_collision_grid(None)                          # latch on, the grid cleared
    for got, w in zip((s.avoidance_box(None, DT, -1.0, 1.0, **PRM), s.clearance_gradient()), want):
        assert all(np.array_equal(got[k], w[k]) for k in w)
    g = c["grid"]
    s.set_collision_grid(g.occ, g.origin, g.h)
    s.set_collision_grid_nearest(False)                 # latch off, then the grid cleared
    s.set_collision_grid(None)
    for got, w in zip((s.avoidance_box(None, DT, -1.0, 1.0, **PRM), s.clearance_gradient()), want):
        assert all(np.array_equal(got[k], w[k]) for k in w)
    s.close()


def test_a_grid_set_under_the_avoidance_latch_and_the_state_errors():
    c = GC.avoid_case("panda7")
    s = _open_case(c)
    g = c["grid"]
    s.set_collision_avoidance(**PRM)
    before = s.avoidance_box(None, DT, -1.0, 1.0, **PRM)
    msg = _err(lambda: s.set_collision_grid_nearest(False), ERR_STATE)      # a grid is set and avoidance is latched
    assert "avoidance" in msg
    assert s.collision_grid_nearest() is not None and s.collision_avoidance() == PRM
    after = s.avoidance_box(None, DT, -1.0, 1.0, **PRM)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    occ2 = np.roll(g.occ, 3, axis=2)
    s.set_collision_grid(occ2, g.origin, g.h)           # accepted while avoidance is latched, and read by the next call
    moved = s.avoidance_box(None, DT, -1.0, 1.0, **PRM)
    want = NN.avoidance_box(c["model"], c["q"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], DT, -1.0, 1.0, grid=NN.Grid(occ2, g.origin, g.h), **PRM)
    inf = np.isposinf(want["pairs"])
    assert np.array_equal(np.isposinf(moved["pairs"]), inf) and not np.array_equal(moved["pairs"], before["pairs"])
    assert np.max(np.abs(moved["pairs"][~inf] - want["pairs"][~inf])) <= BOUND * _scale(want["centres"], c["spheres"])
    s.set_collision_grid(None)                          # without a grid the latch may go while avoidance stays
    s.set_collision_grid_nearest(False)
    msg = _err(lambda: s.set_collision_grid(g.occ, g.origin, g.h), ERR_STATE)
    assert "grid" in msg and "avoidance" in msg and "loikb_collision_grid_set_nearest" in msg
    # the query's validation
    sph = np.zeros((2, 4))
    _err(lambda: s.grid_nearest(sph), ERR_STATE)        # no grid
    s.clear_collision_avoidance()
    s.set_collision_grid(g.occ, g.origin, g.h)
    msg = _err(lambda: s.grid_nearest(sph), ERR_STATE)  # a grid, no latch
    assert "loikb_collision_grid_set_nearest" in msg
    s.set_collision_grid_nearest(True)
    L = s.L
    v, x, n = np.zeros((2, 2)), np.zeros((2, 2), dtype=np.int32), np.zeros((2, 3))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.loikb_grid_nearest_query(s.h, p(sph), -1, 0, p(v), p(x), p(n), 0) == ERR_ARG
    assert L.loikb_grid_nearest_query(s.h, None, 2, 0, p(v), p(x), p(n), 0) == ERR_ARG
    assert L.loikb_grid_nearest_query(s.h, p(sph), 2, 0, p(v), None, p(n), 0) == ERR_ARG
    assert L.loikb_grid_nearest_query(s.h, p(sph), 2, 4, p(v), p(x), p(n), 0) == ERR_ARG
    assert L.loikb_grid_nearest_query(None, p(sph), 2, 0, p(v), p(x), p(n), 0) == ERR_ARG
    assert L.loikb_grid_nearest_query(s.h, None, 0, 0, None, None, None, 0) == 0
    assert s.grid_nearest(sph)["vox"].shape == (2, 2)
    s.close()


def test_on_a_callers_stream():
    """the latch, the grid under it, the transform getter, the query, the gradient and the box on a caller's stream behind pending work,
    byte for byte what the null stream gives (stream_harness)"""
    c = GC.avoid_case("panda7")
    g = c["grid"]
    sph = GC.query_spheres(256, 3103)
    n, nv, ns = c["q"].shape[0], c["model"].nv, len(c["links"])

    def make():
        s = _open(c["model"], c["q"])
        s.set_collision_spheres(c["links"], c["spheres"])
        s.set_collision_world(c["ws"], c["wb"])
        s.set_self_collision(True)
        return s

    def raw(s, fn, *head):
        def call(outs):
            ptrs = [o.ctypes.data_as(C.c_void_p) if isinstance(o, np.ndarray) else C.c_void_p(o.data_ptr()) for o in outs]
            flag = 0 if isinstance(outs[0], np.ndarray) else capi.OUT_DEVICE
            rc = fn(s.h, *head, *ptrs, flag)
            assert rc >= 0, s.L.loikb_last_error()
        return call

    def sequence(run, s):
        run.do(s.set_collision_grid, g.occ, g.origin, g.h)
        run.do(s.set_collision_grid_nearest, True)                                    # builds F for the grid that is set
        run.get_n(["F after the latch"], raw(s, s.L.loikb_collision_grid_get_nearest), [(g.occ.shape, np.uint32)])
        run.do(s.set_collision_grid, np.roll(g.occ, 2, axis=1), g.origin, g.h)        # builds G and F
        run.get_n(["F after a set"], raw(s, s.L.loikb_collision_grid_get_nearest), [(g.occ.shape, np.uint32)])
        d = run.inp(sph)
        dp, dflag = (d.ctypes.data_as(C.c_void_p), 0) if isinstance(d, np.ndarray) else (C.c_void_p(d.data_ptr()), capi.IN_DEVICE)
        run.get_n(["val", "vox", "normal"], raw(s, s.L.loikb_grid_nearest_query, dp, sph.shape[0], dflag),
                  [((sph.shape[0], 2), np.float64), ((sph.shape[0], 2), np.int32), ((sph.shape[0], 3), np.float64)])
        run.get_n(["min", "witness", "grad"], raw(s, s.L.loikb_clearance_gradient, None, n, 0), [((n, 3), np.float64), ((n, 3), np.int32), ((n, nv), np.float64)])
        box = run.do(s.avoidance_box, None, DT, -1.0, 1.0, **PRM)
        for k, v in box.items():
            run.put("box " + k, v)

    rec, gates = H.run_both(make, sequence, what="gridnear")
    assert gates >= 6 and (rec["witness"][:, 0] == GN.WORLD_GRID).any()
