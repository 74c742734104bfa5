"""GPU: integrate(dt) -- q <- q (+) dt z of the resident configurations -- at the edges of its branches, against the group exponentials
in 50-digit arithmetic (tests/integrate_mp.py, pinned to pose_numpy.integrate on the CPU by tests/test_integrate_mpmath.py).
se3_integrate and so3_exp_quat of loik_device.hpp switch to Maclaurin series below |w|^2 = 1.220703125e-4; the planar joint
switches below |w| = 1e-4.  After one solve that leaves a non-trivial z, dt is chosen from the handle's own z so that the
batch median of a joint's angular step sits at 0 (dt = 0), 1e-200, 1e-9, the switch itself (both branches in one call), 1 and 3;
q is read before and after each call.  dt scales the linear and the angular step together, so these calls meet a small angle only
under a small linear step; the planar joint's small angles under an O(1) linear step -- where (1 - cos w) / w, written as that
quotient, is off by (w / 2) |v| -- have a test of their own at the end.

The bound is 1e-12 max(1, |q|_inf), what test_multidof.test_gpu_integrate_on_the_configuration_manifold holds the kernel to: just
under the switch the series' truncation is at most about 2e-11 |w x v| = 2.3e-13 |v_lin| on the translation and about 2e-13 on
the quaternion's vector part after the first-order re-normalisation, both below the bound for linear steps up to O(1)."""
import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from helpers import FIXTURE, random_tree_multidof
from test_multidof import _batch
from test_pose_ik import _fk_models
import integrate_mp as MP
import pose_numpy as P

pytestmark = pytest.mark.gpu

B = 128
SWITCH2 = 1.220703125e-4                 # the device's |w|^2 switch
SWITCH = 0.011048                        # its square root, to five digits
MEDIANS = [1e-200, 1e-9, SWITCH, 1.0, 3.0]
TOL, UNIT_TOL, ZERO_TOL = 1e-12, 1e-12, 1e-15
KIND_NAMES = {P.J_FREEFLYER: "free-flyer", P.J_SPHERICAL: "spherical", P.J_PLANAR: "planar"}


def _primaries(model):
    """the first joint of each kind that integrates on a group: (name, first velocity index, count) of its angular part; a tree
    without one steers dt by the largest coordinate step of the instance instead"""
    out, seen = [], set()
    for jt, iv, n in MP.angular_dofs(model):
        name = KIND_NAMES.get(jt, "(cos, sin)")
        if name not in seen:
            seen.add(name)
            out.append((name, iv, n))
    return out or [("largest step", 0, model.nv)]


@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("k", range(2, 6))
def test_integrate_matches_the_group_exponential_at_its_branch_edges(k, precision):
    model = _fk_models()[k]
    wl = _batch(model, B, 800 + k)
    s = loik_amd.BatchedLoik(model, B, precision=precision, **dict(FIXTURE, max_iter=300, tol_abs=1e-6, tol_rel=0.0))
    s.Solve(wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])
    z = s.get("z")      # (an fp32 handle: the float tiles widened, which is what the kernel multiplies by dt)
    assert z.shape == (B, model.nv) and np.all(np.isfinite(z)) and np.abs(z).max() > 1e-3
    blocks = MP.unit_blocks(model)
    groups = MP.angular_dofs(model)
    calls = [("dt = 0", 0.0, None)]
    for name, iv, n in _primaries(model):
        size = np.linalg.norm(z[:, iv:iv + n], axis=1) if name != "largest step" else np.abs(z).max(axis=1)
        med = float(np.median(size))
        assert med > 1e-6, (model.name, name, med)
        calls += [("%s at %g" % (name, m), m / med, (name, iv, n) if m == SWITCH else None) for m in MEDIANS]
    for what, dt, at_switch in calls:
        q0 = s.get("q")
        s.integrate(dt)
        q1 = s.get("q")
        assert q1.shape == (B, model.nq) and np.all(np.isfinite(q1)), (model.name, what)
        if at_switch is not None and at_switch[0] in ("free-flyer", "spherical"):   # both branches of the device in this one call
            _, iv, n = at_switch
            above = ((dt * z[:, iv:iv + n]) ** 2).sum(axis=1) > SWITCH2
            assert 0.1 <= above.mean() <= 0.9, (model.name, what, above.mean())
        want = np.stack([MP.integrate(model, q0[b], dt * z[b]) for b in range(B)])
        rel = np.abs(q1 - want).max(axis=1) / np.maximum(1.0, np.abs(want).max(axis=1))
        unit = max([float(np.max(np.abs(np.linalg.norm(q1[:, o:o + n], axis=1) - 1.0))) for o, n in blocks] or [0.0])
        steps = [float(np.median(np.linalg.norm(dt * z[:, iv:iv + n], axis=1))) for _, iv, n in groups]
        print("integrate_measured %s %s | %s | dt %.3e | max |dq| / max(1, |q|_inf) %.3e | unit %.3e | median angular steps %s"
              % (model.name, "f32" if precision == capi.F32 else "f64", what, dt, rel.max(), unit, ["%.2e" % x for x in steps]))
        assert rel.max() <= TOL, (model.name, what, rel.max(), int(rel.argmax()))
        assert unit <= UNIT_TOL, (model.name, what, unit)
        if dt == 0.0:
            assert np.max(np.abs(q1 - q0)) <= ZERO_TOL, (model.name, np.max(np.abs(q1 - q0)))
    s.close()


def test_planar_joint_small_angles_under_a_large_linear_step():
    """a planar root joint whose link is asked to move by (vx, vy, w) with |(vx, vy)| = 0.4 and |w| log-uniform in 1e-9 .. 1e-4: the
    root link's velocity is its joint's, so the solve returns z = (vx, vy, w) and integrate(1) takes those steps.  With
    tx = (sin(w) vx - (1 - cos(w)) vy) / w the rounding of cos(w) costs up to 1e-16 / |w| of |v|: 4e-11 at |w| = 1e-6, 4e-9 at
    1e-8, against the bound of 1e-12"""
    model = random_tree_multidof(seed=31, nb=7, root_freeflyer=False, n_spherical=0, n_translation=0, n_zyx=1, n_planar=1, n_rub=2,
                                 root_planar=True)
    assert int(model.jtype[1]) == P.J_PLANAR and int(model.parents[1]) == 0
    iv = int(model.idx_v[1])
    rng = np.random.default_rng(5)
    q = model.random_configurations(rng, B)
    w = rng.choice([-1.0, 1.0], size=B) * 10.0 ** rng.uniform(-9, -4, size=B)
    ang = rng.uniform(0, 2 * np.pi, size=B)
    bis = np.zeros((B, 1, 6))
    bis[:, 0, 0], bis[:, 0, 1], bis[:, 0, 5] = 0.4 * np.cos(ang), 0.4 * np.sin(ang), w
    s = loik_amd.BatchedLoik(model, B, **dict(FIXTURE, max_iter=1000, tol_abs=1e-12, tol_rel=0.0))
    s.Solve(q, np.eye(6), np.zeros(6), np.array([1], dtype=np.int32), np.eye(6)[None], bis, -0.5 * np.ones(model.nv), 0.5 * np.ones(model.nv))
    z = s.get("z")
    small = (np.abs(z[:, iv + 2]) > 1e-10) & (np.abs(z[:, iv + 2]) < 1e-6)
    assert small.mean() >= 0.25 and np.all(np.linalg.norm(z[:, iv:iv + 2], axis=1) > 0.39), (small.mean(), np.abs(z[:, iv + 2]).min())
    s.integrate(1.0)
    q1 = s.get("q")
    s.close()
    want = np.stack([MP.integrate(model, q[b], z[b]) for b in range(B)])
    rel = np.abs(q1 - want).max(axis=1) / np.maximum(1.0, np.abs(want).max(axis=1))
    print("integrate_measured %s planar |w| in [%.1e, %.1e] under |v| = 0.4 | max |dq| / max(1, |q|_inf) %.3e (over |w| < 1e-6: %.3e)"
          % (model.name, np.abs(z[:, iv + 2]).min(), np.abs(z[:, iv + 2]).max(), rel.max(), rel[small].max()))
    assert rel.max() <= TOL, (rel.max(), int(rel.argmax()), z[int(rel.argmax()), iv + 2])
