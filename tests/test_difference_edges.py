"""GPU: loikb_difference at the edges of its branches, against the group exponentials in 50-digit arithmetic: the inputs and the
bounds of tests/test_difference_mpmath.py (which proves the numpy reference inside them on the CPU) with the device's difference in
place of numpy's.  Here the rotation that pose_log3 / pose_log6 see comes out of quat_to_rot of a relative quaternion or of
R0^T R1 and the linear part through R0^T (t1 - t0), not out of forward kinematics as in test_pose_ik.py: another way into the same
series below theta = 1e-4 and 1e-3, the symmetric-part branch below cos theta = -0.8 and pi itself; the planar joint's series
below |w| = 1e-4 and the atan2 of the (cos, sin) joints at +-pi are difference_joint's own.  Then what the numbers cannot show:
q1 = q0, the sign of a quaternion, the device routes and the sizes around k_difference's workgroup of 64 threads."""
import ctypes as C

import numpy as np
import pytest

from loik_amd import capi

from test_pose_ik import EDGE_ABS
import integrate_mp as MP
import test_clearance as TC
import test_difference_mpmath as DM

pytestmark = pytest.mark.gpu


def _open(model, q):
    return TC._open(model, q[:DM.ROWS])


# ---- 1. the sweep ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", DM.TREES)
def test_difference_inverts_the_group_exponential(k):
    c = DM.edge_case(k)
    model, q0, q1 = c["model"], c["q0"], c["q1"]
    s = _open(model, q0)
    got = s.difference(q0, q1)     # every (angle, linear) cell in one call
    s.close()
    DM.check_edges(model.name, model, q0, q1, c["v"], got)


@pytest.mark.parametrize("angle", [np.pi, 4.0], ids=["pi", "4"])
@pytest.mark.parametrize("k", DM.TREES[:2])
def test_difference_at_pi_and_beyond(k, angle):
    model, q0, q1 = DM.beyond_case(k, angle)
    s = _open(model, q0)
    got = s.difference(q0, q1)
    s.close()
    DM.check_round_trip("%s at %.3f" % (model.name, angle), model, q0, q1, got)


def test_planar_joint_small_angles_under_a_large_offset():
    model, q0, v, q1, unique = DM.planar_case()
    s = _open(model, q0)
    got = s.difference(q0, q1)
    s.close()
    DM.check_edges("planar root", model, q0[unique], q1[unique], v[unique], got[unique])
    DM.check_round_trip("planar root at +-pi", model, q0[~unique], q1[~unique], got[~unique])


def test_unbounded_revolute_at_its_edges():
    model, q0, v, q1, unique = DM.revolute_case()
    s = _open(model, q0)
    got = s.difference(q0, q1)
    s.close()
    DM.check_edges("(cos, sin) joints", model, q0[unique], q1[unique], v[unique], got[unique])
    DM.check_round_trip("(cos, sin) joints at +-pi", model, q0[~unique], q1[~unique], got[~unique])


# ---- 2. what holds exactly -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", DM.TREES)
def test_identity_signs_routes_and_sizes(k):
    c = DM.edge_case(k)
    model, q0, q1 = c["model"], c["q0"], c["q1"]
    n = q0.shape[0]
    s = _open(model, q0)
    full = s.difference(q0, q1)
    # q1 = q0: nothing moves
    still = s.difference(q0, q0)
    assert np.all(np.isfinite(still)) and np.max(np.abs(still)) <= EDGE_ABS, np.max(np.abs(still))
    # q and -q are one rotation: quat_to_rot is quadratic, and the spherical branch forms conj(q0) q1 first
    quats = [o for o, m in MP.unit_blocks(model) if m == 4]
    for side in (0, 1):
        a, b = q0.copy(), q1.copy()
        for o in quats:
            (a, b)[side][:, o:o + 4] *= -1.0
        assert np.array_equal(s.difference(a, b), full), side
    # the device routes
    d0, d1, dv = capi.DeviceArray(q0), capi.DeviceArray(q1), capi.DeviceArray(np.full((n, model.nv), -1.0))
    assert np.array_equal(s.difference(d0, d1), full)
    hip = capi.DeviceArray.hip()
    for a, b in ((q0, q1), (d0, d1)):
        s.difference(a, b, out=dv)
        back = np.empty((n, model.nv))
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(dv.data_ptr()), back.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        assert np.array_equal(back, full)
    for a in (d0, d1, dv):
        a.free()
    # the sizes around one workgroup of 64 threads, taken across the cells
    for m in (1, 63, 64, 65):
        rows = np.arange(m) * (n // 65)
        assert np.array_equal(s.difference(q0[rows], q1[rows]), full[rows]), m
    s.close()
