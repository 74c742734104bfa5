"""GPU: the output routes of the query entry points that nothing else reaches, through the C ABI itself.  The device route
(LOIKB_OUT_DEVICE) of loikb_forward_kinematics, loikb_frame_placements and loikb_frame_dexterity -- their Python wrappers have no
out= -- against the host route of the same call, and the host route of loikb_clearance without a witness and of
loikb_shortcut_paths without keep rows and lengths against the full call (the device route of the latter: test_shortcut.py).
Byte for byte: a route decides where a kernel's output lands, never what it is."""
import ctypes as C

import numpy as np
import pytest

from loik_amd import capi

from test_pose_ik import _handle

pytestmark = pytest.mark.gpu

B, T = 5, 4
LINKS = np.array([7, 3, 7], dtype=np.int32)   # one link twice
ROWS = np.array([0x07, 0x38, 0x1f], dtype=np.int32)
_ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)


def _frame(angle, p):
    """iMf [12]: a rotation about z, then the translation"""
    c, s = np.cos(angle), np.sin(angle)
    return np.r_[c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0, p]


# non-identity frames on the first two entries, the joint frame on the repeated link
FRAMES = np.ascontiguousarray(np.stack([_frame(0.7, [0.1, -0.2, 0.3]), _frame(-1.1, [0.0, 0.05, -0.15]), _frame(0.0, [0.0, 0.0, 0.0])]))


@pytest.fixture(scope="module")
def solver(panda7):
    q = panda7.random_configurations(np.random.default_rng(41), B)
    s, _ = _handle(panda7, B, [7], q)   # (SolveInit: q is resident, one active constraint)
    yield s
    s.close()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _both_routes(call, shape):
    """call(out pointer, out_flags) once into a host array and once into a device array: the host array, after the two agreed"""
    host = np.full(shape, np.nan)
    assert call(_ptr(host), 0) == 0, capi.lib().loikb_last_error()
    assert np.isfinite(host).all()
    dev = capi.DeviceArray(np.full(shape, np.nan))
    assert call(C.c_void_p(dev.data_ptr()), capi.OUT_DEVICE) == 0, capi.lib().loikb_last_error()
    back = np.empty(shape)
    assert capi.DeviceArray.hip().hipMemcpy(_ptr(back), C.c_void_p(dev.data_ptr()), back.nbytes, 2) == 0   # hipMemcpyDeviceToHost
    dev.free()
    assert back.tobytes() == host.tobytes()
    return host


def test_forward_kinematics_device_route(solver):
    L = capi.lib()
    got = _both_routes(lambda p, f: L.loikb_forward_kinematics(solver.h, LINKS.ctypes.data_as(_ip), 3, p, f), (B, 3, 12))
    assert got[:, 0].tobytes() == got[:, 2].tobytes() and got[:, 0].tobytes() != got[:, 1].tobytes()
    assert np.array_equal(solver._to44(got), solver.forward_kinematics(LINKS))


def test_frame_placements_device_route(solver):
    L = capi.lib()
    got = _both_routes(lambda p, f: L.loikb_frame_placements(solver.h, LINKS.ctypes.data_as(_ip), FRAMES.ctypes.data_as(_dp), 3, p, f), (B, 3, 12))
    assert np.array_equal(solver._to44(got), solver.frame_placements(LINKS, FRAMES))
    # the repeated link with the joint frame is the link's own placement; the tool frame on the same link is not
    fk = solver.forward_kinematics(LINKS)
    assert np.array_equal(solver._to44(got)[:, 2], fk[:, 2]) and not np.array_equal(solver._to44(got)[:, 0], fk[:, 0])


def test_frame_dexterity_device_route_of_given_links(solver):
    L = capi.lib()
    prm = capi.DexterityParams(0.25, 0)
    got = _both_routes(lambda p, f: L.loikb_frame_dexterity(solver.h, LINKS.ctypes.data_as(_ip), FRAMES.ctypes.data_as(_dp), ROWS.ctypes.data_as(_ip), 3,
                                                            C.byref(prm), p, f), (B, 3, capi.DEX_N))
    want = solver.frame_dexterity(LINKS, FRAMES, ROWS, length=0.25)
    assert np.array_equal(got[..., :6], want["sigma"]) and np.array_equal(got[..., capi.DEX_MANIPULABILITY], want["manipulability"])
    assert not got[:, 0, 3:6].any() and got[:, 2, 4].all() and not got[:, 2, 5].any()   # (zero past the rows a mask selects)


def test_frame_dexterity_device_route_of_the_handles_tasks(solver):
    L = capi.lib()
    prm = capi.DexterityParams(0.25, 0)
    solver.set_pose_tasks(["position"], FRAMES[:1])
    try:
        got = _both_routes(lambda p, f: L.loikb_frame_dexterity(solver.h, None, None, None, 1, C.byref(prm), p, f), (B, 1, capi.DEX_N))
        # the handle's task is the first entry above: link 7, the same frame, the position rows
        want = solver.frame_dexterity(LINKS[:1], FRAMES[:1], ROWS[:1], length=0.25)
        assert np.array_equal(got[..., :6], want["sigma"]) and np.array_equal(got[..., capi.DEX_INV_CONDITION], want["inv_condition"])
    finally:
        solver.clear_pose_tasks()


@pytest.fixture(scope="module")
def spheres(solver):
    """a 3-sphere model and one world sphere"""
    solver.set_collision_spheres([3, 5, 7], [[0.0, 0.0, 0.0, 0.06], [0.0, 0.02, 0.0, 0.05], [0.0, 0.0, 0.05, 0.04]])
    solver.set_collision_world([[0.45, 0.1, 0.55, 0.12]])
    yield solver
    solver.set_collision_world(None, None)
    solver.set_collision_spheres([], np.zeros((0, 4)))


def test_clearance_host_route_without_witness(spheres):
    L = capi.lib()
    s = spheres
    mins, wit, alone = np.full((B, 3), np.nan), np.full((B, 3), -9, dtype=np.int32), np.full((B, 3), np.nan)
    assert L.loikb_clearance(s.h, None, B, 0, _ptr(mins), _ptr(wit), 0) == 0, L.loikb_last_error()
    assert L.loikb_clearance(s.h, None, B, 0, _ptr(alone), None, 0) == 0, L.loikb_last_error()
    assert np.isfinite(mins[:, :2]).all() and (wit != -9).all()
    assert alone.tobytes() == mins.tobytes()


def test_shortcut_paths_host_route_without_keep_and_lengths(spheres, panda7):
    L = capi.lib()
    s, nq = spheres, panda7.nq
    paths = np.ascontiguousarray(panda7.random_configurations(np.random.default_rng(43), B * T).reshape(B, T, nq))
    prm = capi.ShortcutParams(0.0, 1e-3, 64, 8, 5, 0)
    path, keep, info, val = np.full((B, T, nq), np.nan), np.full((B, T), -9, dtype=np.int32), np.full((B, 6), -9, dtype=np.int32), np.full((B, 2), np.nan)
    assert L.loikb_shortcut_paths(s.h, _ptr(paths), None, B, T, 0, C.byref(prm), _ptr(path), _ptr(keep), _ptr(info), _ptr(val), 0) == 0, L.loikb_last_error()
    assert np.isfinite(path).all() and np.isfinite(val).all() and (keep != -9).all() and (info != -9).all()
    assert info[:, 1].sum() > 0   # (shortcuts were tried)
    path2, info2 = np.full((B, T, nq), np.nan), np.full((B, 6), -9, dtype=np.int32)
    assert L.loikb_shortcut_paths(s.h, _ptr(paths), None, B, T, 0, C.byref(prm), _ptr(path2), None, _ptr(info2), None, 0) == 0, L.loikb_last_error()
    assert path2.tobytes() == path.tobytes() and info2.tobytes() == info.tobytes()
