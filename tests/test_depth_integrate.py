"""GPU: depth images and point clouds into the voxel world (include/loik_amd_depth.h) against the numpy reference of tests/depth_numpy.py
(proven on the CPU by test_depth_numpy.py): occupancy, stats and field.

Exact cases (tests/depth_cases.py) are compared bit for bit.  In a general case the occupancy must agree on every voxel that no ambiguous
decision of the reference touches, the field must be grid_numpy.field_brute of the occupancy the device produced, and the counters must
be the reference's up to its ambiguous points.  Then the shapes and values at which a kernel can go wrong: every kind of pixel that is no
return, points on and outside every face, a voxel behind the camera, a filter sphere clipped by every face and one outside the grid,
every route of the image, the points and the filter configurations, and every error of the header with the handle unchanged after it."""
import numpy as np
import pytest

from loik_amd import capi

from stream_harness import DevBuf
from test_clearance import _open, _raises
import depth_cases as DC
import depth_numpy as DN
import grid_numpy as GN

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -20, -24
_HANDLE = {}


def handle():
    """one handle for the file: panda7 with its spheres, three resident configurations"""
    if "s" not in _HANDLE:
        r = DC.robot()
        s = _open(r["model"], r["q"])
        s.set_collision_spheres(r["links"], r["spheres"])
        _HANDLE["s"] = s
    return _HANDLE["s"]


def _filter_arg(c, route, keep):
    if c["nf"] == 0:
        return None
    q = DC.robot()["q"][:c["nf"]]
    if route == "resident":
        return c["nf"]
    if route == "device":
        keep.append(DevBuf(q))
        return keep[-1]
    return q


def _image_arg(img, device, keep):
    if not device:
        return img
    keep.append(DevBuf(img))
    return keep[-1]


def _check(name, what, got_stats, s, want, exact):
    occ, G = s.collision_occupancy(), s.collision_grid()["G"]
    stats = np.array([got_stats[k] for k in ("returns", "inside", "occupied_before", "occupied_after")])
    diff = occ != want["occ"]
    print("depth_measured %s %s: stats %s (numpy %s), %d voxels differ, %d touched by an ambiguous decision" % (
        name, what, stats.tolist(), want["stats"].tolist(), int(diff.sum()), int(want["touched"].sum())))
    assert occ.dtype == np.uint8 and set(np.unique(occ)) <= {0, 1}
    assert stats[3] == int(occ.sum())
    if exact:
        assert np.array_equal(occ, want["occ"]) and np.array_equal(stats, want["stats"]) and np.array_equal(G, want["G"]), (name, what)
        return
    assert not (diff & ~want["touched"]).any(), (name, what, int((diff & ~want["touched"]).sum()))
    assert stats[0] == want["stats"][0] and stats[2] == want["stats"][2]
    assert abs(stats[1] - want["stats"][1]) <= want["ambiguous"]["points"][0]
    assert np.array_equal(G, want["G"] if not diff.any() else GN.field_brute(occ)), (name, what)


ROUTES = ("host", "device", "resident")


@pytest.mark.parametrize("name", list(DC.CASES))
def test_a_frame_matches_numpy(name):
    """REPLACE with the self-filter; then FUSE with the carve onto the frame before"""
    c = DC.case(name)
    s = handle()
    k = list(DC.CASES).index(name)
    keep = []
    try:
        kw = dict(dims=c["dims"], origin=c["origin"], voxel=c["h"])
        fkw = dict(filter_q=_filter_arg(c, ROUTES[k % 3], keep), filter_pad=c["pad"])
        cam = c["cam"].as_dict()
        st = s.integrate_depth(_image_arg(c["img"], k % 2 == 1, keep), cam, **kw, **fkw)
        _check(name, "replace", st, s, c["replace"], c["kind"] == "exact")
        # FUSE ignores a prior when mode is REPLACE: the frame before, alone, then this frame onto it
        st = s.integrate_depth(c["prev"], cam, **kw)
        assert np.array_equal(s.collision_occupancy(), c["prior"]) or c["kind"] != "exact"
        prior_ok = np.array_equal(s.collision_occupancy(), c["prior"])
        st = s.integrate_depth(_image_arg(c["img"], k % 2 == 0, keep), cam, mode="fuse", carve=True, band=c["band"], **kw, **fkw)
        if prior_ok:
            _check(name, "fuse", st, s, c["fuse"], c["kind"] == "exact")
        else:   # (an ambiguous point of the frame before: the reference starts from the device's prior)
            want = DN.integrate(cam=c["cam"], depth=c["img"], mode=DN.FUSE, carve_on=True, band=c["band"], prior=s.collision_occupancy(), dims=c["dims"],
                                origin=c["origin"], h=c["h"], filter_centres=c["centres"], filter_radii=c["radii"], filter_pad=c["pad"])
            _check(name, "fuse", st, s, want, False)
    finally:
        for b in keep:
            b.free()


def test_carve_with_no_band_and_fuse_without_carve():
    c = DC.case("exact-65x3-odd-u16")
    s = handle()
    cam, kw = c["cam"].as_dict(), dict(dims=c["dims"], origin=c["origin"], voxel=c["h"])
    nkw = dict(cam=c["cam"], depth=c["img"], mode=DN.FUSE, prior=c["prior"], dims=c["dims"], origin=c["origin"], h=c["h"])
    for carve, band in ((True, 0.0), (False, 0.0)):
        s.integrate_depth(c["prev"], cam, **kw)
        st = s.integrate_depth(c["img"], cam, mode="fuse", carve=carve, band=band, **kw)
        _check("exact-65x3-odd-u16", "fuse carve=%d band=%g" % (carve, band), st, s, DN.integrate(carve_on=carve, band=band, **nkw), True)
    assert st["occupied_after"] >= st["occupied_before"]   # without the carve nothing goes
    # FUSE with no grid set: the empty prior
    s.set_collision_grid(None)
    st = s.integrate_depth(c["img"], cam, mode="fuse", carve=True, band=0.0, **kw)
    _check("exact-65x3-odd-u16", "fuse onto nothing", st, s, DN.integrate(cam=c["cam"], depth=c["img"], dims=c["dims"], origin=c["origin"], h=c["h"]), True)


def test_points_on_and_outside_every_face_and_the_depth_route_by_points():
    s = handle()
    dims, origin, h = (5, 4, 3), np.array([0.25, -0.5, 1.0]), 0.125
    hi = origin + np.array(dims) * h
    mid = origin + 0.5 * np.array(dims) * h + 0.01
    pts = [mid.copy()]
    for k in range(3):
        for v in (origin[k] - 0.01, hi[k] + 0.01, origin[k], hi[k]):   # outside low, outside high, exactly on the low face (in), on the high (out)
            p = mid.copy()
            p[k] = v
            pts.append(p)
    pts += [[np.nan, mid[1], mid[2]], [mid[0], np.inf, mid[2]]]
    pts = np.array(pts)
    want = DN.integrate(points=pts, dims=dims, origin=origin, h=h)
    assert want["stats"].tolist() == [13, 4, 0, 4]
    keep = DevBuf(pts)
    try:
        for arg in (pts, keep):
            s.set_collision_grid(None)
            st = s.integrate_points(arg, dims, origin, h)
            _check("faces", "points", st, s, want, True)
        occ = s.collision_occupancy()
        assert occ[:, :, 0].sum() == 1 and occ[:, 0, :].sum() == 1 and occ[0, :, :].sum() == 1 and occ[:, :, -1].sum() == 0
        # FUSE of points keeps the prior
        st = s.integrate_points(mid[None] + [[h, 0.0, 0.0]], dims, origin, h, mode="fuse")
        assert (st["occupied_before"], st["occupied_after"]) == (4, 5)
    finally:
        keep.free()
    # the depth route and the points route on the same back-projected points: the same occupancy, stats and field
    c = DC.case("general-vga-odd")
    xw, ret = DN.back_project(c["img"], c["cam"])
    kw = dict(dims=c["dims"], origin=c["origin"], voxel=c["h"])
    a = s.integrate_depth(c["img"], c["cam"].as_dict(), **kw)
    occ_a, G_a = s.collision_occupancy(), s.collision_grid()["G"]
    b = s.integrate_points(np.where(ret[:, None], xw, np.nan), **kw)
    assert a == b and np.array_equal(occ_a, s.collision_occupancy()) and np.array_equal(G_a, s.collision_grid()["G"])


def test_a_voxel_behind_the_camera_is_not_carved():
    s = handle()
    cam = DN.Camera(9, 7, 64.0, 64.0, 4.0, 3.0, DC.LOOK_X, [0.5, 0.0, 0.0], 0.25, 8.0)
    dims, origin, h = (16, 3, 3), np.array([0.0, -0.09375, -0.09375]) + 1.0 / 8192.0, 0.0625   # x 0 .. 1: half of it behind the camera
    img = np.full((7, 9), 4.0, dtype=np.float32)
    prior = np.ones(dims[::-1], dtype=np.uint8)
    s.set_collision_grid(prior, origin, h)
    st = s.integrate_depth(img, cam.as_dict(), dims, origin, h, mode="fuse", carve=True, band=0.0)
    want = DN.integrate(cam=cam, depth=img, mode=DN.FUSE, carve_on=True, band=0.0, prior=prior, dims=dims, origin=origin, h=h)
    _check("behind", "fuse", st, s, want, True)
    occ = s.collision_occupancy()
    assert occ[:, :, :8].all() and not occ[1, 1, 9:].any()


def test_filter_spheres_clipped_by_every_face_and_outside_the_grid():
    """spheres on the universe link, so that their world centres are the numbers given"""
    r = DC.robot()
    s = _open(r["model"], r["q"])
    try:
        dims, origin, h = DC.GRIDS["thin"], np.array([0.5, -0.09375, 0.0]) + 1.0 / 8192.0, 0.0625
        full = np.ones(dims[::-1], dtype=np.uint8)
        mid = origin + 0.5 * np.array(dims) * h
        for what, spheres in (("clipped by every face", [[*mid, 1.9]]), ("outside", [[mid[0], mid[1] + 3.0, mid[2], 0.5]]),
                              ("both and a small one", [[*mid, 1.9], [mid[0], mid[1] + 3.0, mid[2], 0.5], [origin[0], origin[1], origin[2], 0.2]])):
            spheres = np.array(spheres)
            s.set_collision_spheres(np.zeros(len(spheres), dtype=np.int32), spheres)
            s.set_collision_grid(full, origin, h)
            st = s.integrate_points(np.zeros((0, 3)), dims, origin, h, mode="fuse", filter_q=1, filter_pad=0.03125)
            want = DN.integrate(points=np.zeros((0, 3)), mode=DN.FUSE, prior=full, dims=dims, origin=origin, h=h, filter_centres=spheres[:, :3],
                                filter_radii=spheres[:, 3], filter_pad=0.03125)
            assert want["ambiguous"]["filter"][0] == 0
            _check("filter", what, st, s, want, True)
        assert 0 < st["occupied_after"] < st["occupied_before"]
    finally:
        s.close()


def test_every_error_leaves_the_handle_as_it_was():
    c = DC.case("exact-65x3-thin")
    s = handle()
    cam, dims, origin, h = c["cam"].as_dict(), c["dims"], c["origin"], c["h"]
    s.integrate_depth(c["img"], cam, dims, origin, h)
    before = (s.collision_grid(), s.collision_occupancy())

    def bad(code, text, fn, *a, **kw):
        _raises(code, text, fn, *a, **kw)
        g = s.collision_grid()
        assert g["dims"] == before[0]["dims"] and np.array_equal(g["origin"], before[0]["origin"]) and g["voxel"] == before[0]["voxel"]
        assert np.array_equal(g["G"], before[0]["G"]) and np.array_equal(s.collision_occupancy(), before[1])

    img = c["img"]
    D = lambda **over: s.integrate_depth(img, dict(cam, **over), dims, origin, h)
    for over, text in ((dict(fx=0.0), "intrinsics"), (dict(fy=-1.0), "intrinsics"), (dict(cx=np.nan), "intrinsics"), (dict(cy=np.inf), "intrinsics"),
                       (dict(T_world_cam=np.concatenate([2.0 * DC.LOOK_X.reshape(9), np.zeros(3)])), "orthonormal"),
                       (dict(T_world_cam=np.concatenate([np.diag([1.0, 1.0, -1.0]).reshape(9), np.zeros(3)])), "orthonormal"),
                       (dict(T_world_cam=np.concatenate([DC.LOOK_X.reshape(9), [0.0, np.nan, 0.0]])), "orthonormal"),
                       (dict(depth_scale=0.0), "depth_scale"), (dict(z_min=0.0), "z_min"), (dict(z_min=2.0, z_max=1.0), "z_min"), (dict(z_max=np.inf), "z_min")):
        bad(ERR_ARG, text, D, **over)
    bad(ERR_ARG, "band", s.integrate_depth, img, cam, dims, origin, h, mode="fuse", carve=True, band=-0.1)
    bad(ERR_ARG, "filter_pad", s.integrate_depth, img, cam, dims, origin, h, filter_pad=-0.1)
    bad(ERR_ARG, "carve needs", s.integrate_depth, img, cam, dims, origin, h, carve=True)
    bad(ERR_ARG, "LOIKB_GRID_MAX_DIM", s.integrate_depth, img, cam, (0, 3, 9), origin, h)
    bad(ERR_ARG, "LOIKB_GRID_MAX_DIM", s.integrate_depth, img, cam, (513, 3, 9), origin, h)
    bad(ERR_ARG, "2^26", s.integrate_depth, img, cam, (512, 512, 512), origin, h)
    bad(ERR_ARG, "voxel edge", s.integrate_depth, img, cam, dims, origin, 0.0)
    bad(ERR_ARG, "not finite", s.integrate_depth, img, cam, dims, [np.nan, 0.0, 0.0], h)
    bad(ERR_ARG, "n_filter", s.integrate_depth, img, cam, dims, origin, h, filter_q=np.zeros((65, 7)))
    bad(ERR_STATE, "batch", s.integrate_depth, img, cam, dims, origin, h, filter_q=4)
    bad(ERR_STATE, "other dims", s.integrate_depth, img, cam, (65, 3, 8), origin, h, mode="fuse")
    bad(ERR_STATE, "other dims", s.integrate_depth, img, cam, dims, origin + 1e-6, h, mode="fuse")
    bad(ERR_STATE, "other dims", s.integrate_points, np.zeros((1, 3)), dims, origin, 2.0 * h, mode="fuse")
    # the raw call: NULL arguments, unknown type, mode, flags
    import ctypes as C
    L = s.L
    image = np.ascontiguousarray(img)
    cs = capi.DepthCamera(c["cam"].width, c["cam"].height, 64.0, 64.0, c["cam"].cx, c["cam"].cy, (C.c_double * 12)(*cam["T_world_cam"]), 1.0, 0.25, 8.0)
    dm, org = np.array(dims, dtype=np.int32), np.array(origin, dtype=float)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)

    def raw(depth=image.ctypes.data_as(C.c_void_p), dtype=capi.DEPTH_F32, camera=C.byref(cs), d=dm.ctypes.data_as(ip), o=org.ctypes.data_as(dp), prm=None, q=None,
            nf=0, flags=0, **p):
        prm = capi.DepthParams(**dict(dict(mode=0, carve=0, band=0.0, filter_pad=0.0, flags=0), **p)) if prm is None else prm
        rc = L.loikb_collision_grid_integrate_depth(s.h, depth, dtype, camera, d, o, h, C.byref(prm) if prm != "null" else None, q, nf, flags, None)
        if rc:
            capi._check(rc)

    assert L.loikb_collision_grid_integrate_depth(None, None, 0, None, None, None, 0.0, None, None, 0, 0, None) == ERR_ARG
    for kw, text in ((dict(depth=None), "image"), (dict(camera=None), "camera"), (dict(d=None), "dims"), (dict(o=None), "dims"), (dict(prm="null"), "params"),
                     (dict(dtype=2), "depth_type"), (dict(mode=2), "mode"), (dict(mode=1, carve=2), "carve"), (dict(flags=4), "in_flags"), (dict(**{"flags": 0, "nf": -1}), "n_filter"),
                     (dict(band=np.nan, mode=1, carve=1), "band")):
        bad(ERR_ARG, text, raw, **kw)
    pr = capi.DepthParams(0, 0, 0.0, 0.0, 1)
    bad(ERR_ARG, "params flags", raw, prm=pr)
    wide = capi.DepthCamera(4097, 1, 64.0, 64.0, 0.0, 0.0, (C.c_double * 12)(*cam["T_world_cam"]), 1.0, 0.25, 8.0)
    bad(ERR_ARG, "width or height", raw, camera=C.byref(wide))
    pc = capi.DepthParams(1, 1, 0.0, 0.0, 0)
    pts = np.zeros((1, 3))
    rc = L.loikb_collision_grid_integrate_points(s.h, pts.ctypes.data_as(C.c_void_p), 1, dm.ctypes.data_as(ip), org.ctypes.data_as(dp), h, C.byref(pc), None, 0, 0, None)
    assert rc == ERR_ARG and b"no camera" in L.loikb_last_error()
    assert L.loikb_collision_grid_integrate_points(s.h, None, 1, dm.ctypes.data_as(ip), org.ctypes.data_as(dp), h, C.byref(pc), None, 0, 0, None) == ERR_ARG
    assert L.loikb_collision_grid_get_occupancy(s.h, None, 2) == ERR_ARG and L.loikb_collision_grid_get_occupancy(None, None, 0) == 0
    bad(ERR_ARG, "n_filter", raw, nf=65)
    # no spheres: a filter is refused
    r = DC.robot()
    t = _open(r["model"], r["q"])
    try:
        _raises(ERR_STATE, "spheres", t.integrate_depth, img, cam, dims, origin, h, filter_q=1)
        assert t.collision_grid() is None and t.collision_occupancy() is None
        # avoidance latched without the nearest transform: the refusal of set_collision_grid
        t.set_collision_spheres(r["links"], r["spheres"])
        t.set_collision_avoidance(0.01, 0.1)
        _raises(ERR_STATE, "avoidance", t.integrate_depth, img, cam, dims, origin, h)
        assert t.collision_grid() is None
        t.set_collision_grid_nearest(True)
        t.integrate_depth(img, cam, dims, origin, h)
        assert np.array_equal(t.collision_occupancy(), before[1])
    finally:
        t.close()


def test_close_the_handle():
    s = _HANDLE.pop("s", None)
    if s is not None:
        s.close()
