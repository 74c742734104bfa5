"""GPU: nothing downstream can tell a voxel world that was integrated from a depth image (include/loik_amd_depth.h) from one that was set
as an occupancy -- clearance, the certified motion check, a planning query, the nearest-voxel transform and the clearance gradient are
bit for bit those of a second handle given collision_occupancy() through set_collision_grid --, the self-filter makes a robot that
sees itself free, the carve frees the place an obstacle has left, a call on a caller's stream behind pending work gives the same bits,
and a second call of the same size allocates nothing."""
import ctypes as C

import numpy as np
import pytest

from loik_amd import capi

from stream_harness import run_both
from test_clearance import _open
import depth_cases as DC
import depth_numpy as DN
import grid_numpy as GN
import motion_numpy as MN

pytestmark = pytest.mark.gpu

H = 0.04
DIMS, ORIGIN = (72, 64, 56), np.array([-1.2, -1.28, -0.7]) + 1.0 / 8192.0
WALL = [[1.0, 0.0, 0.0, 2.4]]   # behind the grid: every pixel has a return, none of the wall's points falls into the grid
_W = {}


def world():
    """panda7 with two spheres a link, eight configurations, a camera that looks at the robot from 1.6 m"""
    if not _W:
        r = DC.robot()
        q = r["model"].random_configurations(np.random.default_rng(2400), 8)
        _W.update(model=r["model"], links=r["links"], spheres=r["spheres"], q=q, centres=MN.centres(r["model"], q, r["links"], r["spheres"]),
                  cam=DN.Camera(96, 72, 80.0, 80.0, 47.5, 35.5, DC.LOOK_X, [-1.6, 0.0, 0.4], 0.2, 6.0))
    return _W


def _handle(w):
    s = _open(w["model"], w["q"])
    s.set_collision_spheres(w["links"], w["spheres"])
    return s


def _box(c, half=0.06):
    return np.concatenate([np.eye(3).reshape(9), c, [half, half, half]])


def _scene_image(w):
    """two boxes near the arm's reach and the wall"""
    return DN.render(w["cam"], boxes=[_box([0.45, 0.3, 0.55], 0.1), _box([0.3, -0.45, 0.2], 0.12)], planes=WALL)


def _same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


@pytest.mark.parametrize("nearest", [False, True])
def test_an_integrated_world_reads_like_one_that_was_set(nearest):
    w = world()
    s, t = _handle(w), _handle(w)
    try:
        if nearest:
            s.set_collision_grid_nearest(True)
            t.set_collision_grid_nearest(True)
        st = s.integrate_depth(_scene_image(w), w["cam"].as_dict(), DIMS, ORIGIN, H)
        assert st["occupied_after"] > 20
        occ = s.collision_occupancy()
        t.set_collision_grid(occ, ORIGIN, H)
        assert np.array_equal(t.collision_occupancy(), occ)   # the getter reads a grid that was set as well
        gs, gt = s.collision_grid(), t.collision_grid()
        assert gs["dims"] == gt["dims"] and np.array_equal(gs["origin"], gt["origin"]) and gs["voxel"] == gt["voxel"] and np.array_equal(gs["G"], gt["G"])
        q = w["q"]
        _same(s.clearance(), t.clearance(), "clearance")
        assert np.isfinite(s.clearance()["min"]).all()
        kw = dict(margin=0.0, tol=1e-3, max_evals=24)
        _same(s.motion_clearance(q, qb=np.roll(q, 1, axis=0), **kw), t.motion_clearance(q, qb=np.roll(q, 1, axis=0), **kw), "motion_clearance")
        pk = dict(step=0.5, max_iters=8, max_nodes=32, seed=7, margin=-0.05, tol=1e-3, max_evals=24)
        _same(s.plan_paths(q[:4], q[4:], -2.5, 2.5, 8, **pk), t.plan_paths(q[:4], q[4:], -2.5, 2.5, 8, **pk), "plan_paths")
        if nearest:
            assert np.array_equal(s.collision_grid_nearest(), t.collision_grid_nearest())
            _same(s.clearance_gradient(), t.clearance_gradient(), "clearance_gradient")
        else:
            assert s.collision_grid_nearest() is None
    finally:
        s.close()
        t.close()


def test_a_robot_that_sees_itself_is_in_collision_without_the_filter_and_free_with_it():
    w = world()
    s = _handle(w)
    try:
        cen = w["centres"][0]
        img = DN.render(w["cam"], spheres=np.concatenate([cen, w["spheres"][:, 3:]], axis=1), planes=[[1.0, 0.0, 0.0, 1.4]])
        cam = w["cam"].as_dict()
        s.integrate_depth(img, cam, DIMS, ORIGIN, H)
        raw = s.clearance()["min"][0]
        st = s.integrate_depth(img, cam, DIMS, ORIGIN, H, filter_q=1)   # the resident q, the recommended pad
        seen = s.clearance()["min"][0]
        print("depth_measured self-filter: clearance %.4f without, %.4f with; %d voxels stay" % (raw, seen, st["occupied_after"]))
        assert raw <= 0.0 < seen and st["occupied_after"] > 100
        # the same from host q, and the filter clears the prior in FUSE as well
        s.integrate_depth(img, cam, DIMS, ORIGIN, H)
        s.integrate_depth(img, cam, DIMS, ORIGIN, H, mode="fuse", filter_q=w["q"][:1])
        assert s.clearance()["min"][0] == seen
    finally:
        s.close()


@pytest.mark.parametrize("carve", [True, False])
def test_an_obstacle_that_moves_frees_its_place_only_with_the_carve(carve):
    w = world()
    model, q = w["model"], w["q"]
    qa, qb = q[0:1], q[1:2]
    dv = MN.difference(model, qa, qb)
    # the obstacle sits where the last sphere is halfway along the segment, then far from the arm
    A = MN.centres(model, MN.interpolate(model, qa[0], dv[0], 0.5)[None], w["links"], w["spheres"])[0, -1]
    Bp = np.array([1.2, -1.0, -0.4])
    f1, f2 = DN.render(w["cam"], boxes=[_box(A)], planes=WALL), DN.render(w["cam"], boxes=[_box(Bp)], planes=WALL)
    s = _handle(w)
    try:
        cam, kw = w["cam"].as_dict(), dict(margin=0.0, tol=1e-3, max_evals=64)
        s.integrate_depth(f1, cam, DIMS, ORIGIN, H)
        assert s.motion_clearance(qa, qb=qb, **kw)["status"][0] == capi.MOTION_BLOCKED
        for frame in (f2, f2):
            st = s.integrate_depth(frame, cam, DIMS, ORIGIN, H, mode="fuse", carve=carve)   # the recommended band
        got = s.motion_clearance(qa, qb=qb, **kw)
        # the reference, frame by frame
        ref = DN.integrate(cam=w["cam"], depth=f1, dims=DIMS, origin=ORIGIN, h=H, field=False)
        for frame in (f2, f2):
            ref = DN.integrate(cam=w["cam"], depth=frame, mode=DN.FUSE, carve_on=carve, band=DN.COVER * H, prior=ref["occ"], dims=DIMS, origin=ORIGIN, h=H)
        assert not ref["touched"].any() and np.array_equal(s.collision_occupancy(), ref["occ"]) and st["occupied_after"] == ref["stats"][3]
        assert got["status"][0] == (capi.MOTION_FREE if carve else capi.MOTION_BLOCKED)
        want = GN.advance(model, qa, dv, w["links"], w["spheres"], grid=GN.Grid(ref["occ"], ORIGIN, H, G=ref["G"]), **kw)
        assert want["status"][0] == got["status"][0]
    finally:
        s.close()


def test_on_a_callers_stream_behind_pending_work():
    w = world()
    img, prev = _scene_image(w), DN.render(w["cam"], boxes=[_box([0.2, 0.5, 0.4], 0.1)], planes=WALL)
    pts = DN.back_project(img, w["cam"])[0]
    cam = w["cam"]
    cs = capi.DepthCamera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, (C.c_double * 12)(*np.concatenate([cam.R.reshape(9), cam.p])), 1.0, cam.z_min, cam.z_max)
    dm = np.array(DIMS, dtype=np.int32)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)

    def ptr(a):
        return (a.ctypes.data_as(C.c_void_p), 0) if isinstance(a, np.ndarray) else (C.c_void_p(a.data_ptr()), 1)

    def sequence(run, s):
        L = s.L
        vox = DIMS[0] * DIMS[1] * DIMS[2]

        def depth(image, qf, prm, key):
            d, q = run.inp(image, dtype=np.float32), run.inp(qf)
            st = np.zeros(4, dtype=np.int64)
            (dptr, dflag), (qptr, qflag) = ptr(d), ptr(q)
            rc = run.do(L.loikb_collision_grid_integrate_depth, s.h, dptr, capi.DEPTH_F32, C.byref(cs), dm.ctypes.data_as(ip), ORIGIN.ctypes.data_as(dp), H,
                        C.byref(prm), qptr, qf.shape[0], dflag | (capi.DEPTH_Q_DEVICE if qflag else 0), st.ctypes.data_as(C.c_void_p))
            assert rc == 0, capi.lib().loikb_last_error()
            run.put("stats " + key, st)
            run.get_n(["occ " + key], lambda o: L.loikb_collision_grid_get_occupancy(s.h, *(lambda p: (p[0], p[1]))(ptr(o[0]))), [((vox,), np.uint8)])
            run.get_n(["G " + key], lambda o: L.loikb_collision_get_world_grid(s.h, None, None, None, *(lambda p: (p[0], p[1]))(ptr(o[0]))), [((vox,), np.uint32)])

        depth(prev, w["q"][:2], capi.DepthParams(capi.DEPTH_REPLACE, 0, 0.0, 0.05, 0), "replace")
        depth(img, w["q"][:3], capi.DepthParams(capi.DEPTH_FUSE, 1, DN.COVER * H, 0.05, 0), "fuse")
        p = run.inp(pts)
        st = np.zeros(4, dtype=np.int64)
        prm = capi.DepthParams(capi.DEPTH_FUSE, 0, 0.0, 0.05, 0)
        pp, pflag = ptr(p)
        rc = run.do(L.loikb_collision_grid_integrate_points, s.h, pp, pts.shape[0], dm.ctypes.data_as(ip), ORIGIN.ctypes.data_as(dp), H, C.byref(prm), None, 2, pflag,
                    st.ctypes.data_as(C.c_void_p))
        assert rc == 0, capi.lib().loikb_last_error()
        run.put("stats points", st)
        run.get_n(["occ points"], lambda o: L.loikb_collision_grid_get_occupancy(s.h, *(lambda p: (p[0], p[1]))(ptr(o[0]))), [((vox,), np.uint8)])
        run.get_n(["min", "witness"], lambda o: L.loikb_clearance(s.h, None, w["q"].shape[0], 0, *(lambda a, b: (a[0], b[0], a[1]))(ptr(o[0]), ptr(o[1]))),
                  [((w["q"].shape[0], 3), np.float64), ((w["q"].shape[0], 3), np.int32)])

    rec, gates = run_both(lambda: _handle(w), sequence, what="depth")
    assert gates >= 8 and rec["stats fuse"][2] > 0 and rec["stats points"][1] > 0 and rec["occ fuse"].sum() == rec["stats fuse"][3]


def test_a_second_call_of_the_same_size_allocates_nothing():
    w = world()

    def counters():
        out = (C.c_ulonglong * 4)()
        assert capi.lib().loikb_debug_device_memory(out) == 0
        return tuple(int(x) for x in out)

    s = _handle(w)
    try:
        s.set_collision_grid_nearest(True)
        img, cam = _scene_image(w), w["cam"].as_dict()
        pts = DN.back_project(img, w["cam"])[0]
        first = counters()
        s.integrate_depth(img, cam, DIMS, ORIGIN, H, filter_q=w["q"][:3])
        s.integrate_depth(img, cam, DIMS, ORIGIN, H, mode="fuse", carve=True, filter_q=w["q"][:3])   # (the second set of a grid fills the spare buffers)
        s.integrate_points(pts, DIMS, ORIGIN, H, filter_q=3)
        s.collision_occupancy()
        grown = counters()
        assert grown[1] > first[1]
        for _ in range(2):
            s.integrate_depth(img, cam, DIMS, ORIGIN, H, mode="fuse", carve=True, filter_q=w["q"][:3])
            s.integrate_depth(img[:48], dict(cam), DIMS, ORIGIN, H, filter_q=1)          # a smaller image fits what is there
            s.integrate_points(pts[:1000], DIMS, ORIGIN, H, mode="fuse", filter_q=2)
            s.collision_occupancy()
            assert counters() == grown
    finally:
        s.close()
