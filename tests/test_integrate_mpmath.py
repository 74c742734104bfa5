"""CPU: pose_numpy.integrate -- the numpy integrator under every lock-step pose oracle -- against the group exponentials in 50-digit
arithmetic (tests/integrate_mp.py): SE(3), SO(3), SE(2), SO(2) on (cos, sin) and the plain sums, on the four multi-DoF trees of
test_pose_ik._fk_models()[2:6] (every joint kind they hold, composite included), at angular steps of exactly zero, 1e-200, 1e-9,
either side of |w| = 0.011048 (where the device switches to its series), 1, 3 and one beyond pi, with unit and 1e-3 linear steps."""
import numpy as np
import pytest

from loik_amd import workloads as W

from test_pose_ik import _fk_models
import integrate_mp as MP
import pose_numpy as P

DEVICE_SWITCH = 0.011048                      # sqrt(1.220703125e-4): se3_integrate / so3_exp_quat of loik_device.hpp
ANGLES = [0.0, 1e-200, 1e-9, 0.9 * DEVICE_SWITCH, 1.1 * DEVICE_SWITCH, 1.0, 3.0, 4.0]   # (4.0: beyond pi, the hemisphere rule)
LINEAR = [1.0, 1e-3]
TOL = 1e-13                                   # times max(1, |q|_inf): a few hundred ulps of O(1) numbers in double
N_CONFIGS = 6


def _unit(rng, n):
    a = rng.normal(size=n)
    return a / np.linalg.norm(a)


def _velocity(model, rng, angle, linear):
    """a velocity whose every group joint takes an angular step of exactly the size `angle` (a random direction) and whose every
    other block is a random direction of the size `linear`"""
    v = np.empty(model.nv)
    for k in range(model.nv):
        v[k] = linear * rng.choice([-1.0, 1.0]) * rng.uniform(0.3, 1.0)
    chain = W._Chain(model) if getattr(model, "composite", None) else model
    for i in range(1, chain.njoints):
        jt, iv = int(chain.jtype[i]), int(chain.idx_v[i])
        if jt == P.J_FREEFLYER:
            v[iv:iv + 3] = linear * _unit(rng, 3)
        elif jt == P.J_PLANAR:
            v[iv:iv + 2] = linear * _unit(rng, 2)
    for jt, iv, n in MP.angular_dofs(model):
        v[iv:iv + n] = angle * _unit(rng, n)
    return v


def test_the_four_trees_hold_every_joint_kind():
    kinds = set()
    for model in _fk_models()[2:6]:
        chain = W._Chain(model) if getattr(model, "composite", None) else model
        kinds |= {int(t) for t in chain.jtype[1:]}
        if getattr(model, "composite", None):
            kinds.add(P.J_COMPOSITE)
    want = {P.J_FREEFLYER, P.J_SPHERICAL, P.J_TRANSLATION, P.J_SPHERICAL_ZYX, P.J_PLANAR, P.J_COMPOSITE}
    assert want <= kinds, sorted(want - kinds)
    assert kinds & {P.J_RUBX, P.J_RUBY, P.J_RUBZ} and kinds & {P.J_HX, P.J_HY, P.J_HZ, P.J_HU}
    assert kinds & {P.J_RX, P.J_RY, P.J_RZ, P.J_RU} and kinds & {P.J_PX, P.J_PY, P.J_PZ, P.J_PU}


@pytest.mark.parametrize("k", range(2, 6))
def test_numpy_integrate_is_the_group_exponential(k):
    model = _fk_models()[k]
    rng = np.random.default_rng(900 + k)
    qs = model.random_configurations(rng, N_CONFIGS)
    worst = {}
    for angle in ANGLES:
        for linear in LINEAR:
            m = 0.0
            for q in qs:
                v = _velocity(model, rng, angle, linear)
                got, want = P.integrate(model, q, v), MP.integrate(model, q, v)
                assert np.all(np.isfinite(got)), (model.name, angle, linear)
                m = max(m, float(np.max(np.abs(got - want)) / max(1.0, np.max(np.abs(want)))))
            worst[(angle, linear)] = m
    print("integrate_measured numpy vs mpmath %s: max |dq| / max(1, |q|_inf) = %.3e; by (angle, linear): %s"
          % (model.name, max(worst.values()), {key: "%.1e" % val for key, val in worst.items()}))
    for key, val in worst.items():
        assert val <= TOL, (model.name, key, val)


def test_zero_velocity_leaves_the_configuration_as_it_is():
    """the case that used to return NaN: a free-flyer whose angular step is exactly zero"""
    for model in _fk_models()[2:6]:
        q = model.random_configurations(np.random.default_rng(17), 3)
        for b in range(3):
            got = P.integrate(model, q[b], np.zeros(model.nv))
            assert np.max(np.abs(got - q[b])) <= 1e-15, model.name
            assert np.max(np.abs(MP.integrate(model, q[b], np.zeros(model.nv)) - q[b])) <= 1e-15, model.name
