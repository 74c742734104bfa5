"""CPU: motion_numpy.difference -- the numpy reference of loikb_difference -- at the edges of its branches, against the group
exponentials in 50-digit arithmetic (tests/integrate_mp.py), the way test_integrate_mpmath.py pins pose_numpy.integrate.  With
q1 = MP.integrate(q0, v) the configuration q1 is q0 (+) v to one rounding and its quaternion and (cos, sin) blocks are unit to an
ulp, so difference(q0, q1) must give v back: on the four multi-DoF trees of test_pose_ik._fk_models()[2:6], at angular steps of
zero, 1e-200, 1e-9, either side of the theta = 1e-4 series of log3 (and of the planar joint), of the theta = 1e-3 series of log6's
beta and of the cos theta = -0.8 switch to the symmetric part, 0.011, 1, 3 and pi approached down to 1e-12, under unit and 1e-3
linear steps.  At pi itself and beyond it v is not unique (or is the short way round): there integrate(q0, v_got) must be q1 again.
The planar joint's small angles under an O(1) offset, the unbounded revolute at +-pi and the cost of a quaternion that is not
unit have cases of their own.  tests/test_difference_edges.py holds the device to the same inputs and bounds."""
import numpy as np
import pytest

from loik_amd import workloads as W

from helpers import random_tree_multidof
from test_integrate_mpmath import _velocity
from test_pose_ik import EDGE_ABS, EDGE_REL, _fk_models
import integrate_mp as MP
import motion_numpy as MN
import pose_numpy as P

SWITCH_08 = float(np.arccos(-0.8))
ANGLES = [0.0, 1e-200, 1e-9, 1e-4 * (1 - 1e-3), 1e-4 * (1 + 1e-3), 1e-3 * (1 - 1e-3), 1e-3 * (1 + 1e-3), 0.011, 1.0, SWITCH_08 - 1e-6,
          SWITCH_08 + 1e-6, 3.0, np.pi - 1e-3, np.pi - 1e-6, np.pi - 1e-9, np.pi - 1e-12]
LINEAR = [1.0, 1e-3]
ROWS = 16                    # per (angle, linear) cell
TREES = list(range(2, 6))
TOL = 1e-12                  # times max(1, |q|_inf): the bound of test_integrate_edges.py, for the round trips at and beyond pi
PLANAR_OFFSET = 0.4

_CASES = {}


def _chain(model):
    return W._Chain(model) if getattr(model, "composite", None) else model


def blocks(model):
    """(angular [(iv, n)], linear [(iv, n)]): the angular part of every joint that integrates on a group; the free-flyer's and the
    planar joint's linear part as a block each and every other degree of freedom as a block of its own"""
    ang = [(iv, n) for _, iv, n in MP.angular_dofs(model)]
    ch = _chain(model)
    lin, taken = [], set()
    for iv, n in ang:
        taken |= set(range(iv, iv + n))
    for i in range(1, ch.njoints):
        jt, iv = int(ch.jtype[i]), int(ch.idx_v[i])
        if jt in (P.J_FREEFLYER, P.J_PLANAR):
            n = 3 if jt == P.J_FREEFLYER else 2
            lin.append((iv, n))
            taken |= set(range(iv, iv + n))
    lin += [(k, 1) for k in range(int(model.nv)) if k not in taken]
    return ang, lin


def _integrate_rows(model, q0, v):
    return np.stack([MP.integrate(model, q0[r], v[r]) for r in range(q0.shape[0])])


def edge_case(k):
    """tree k of _fk_models(): ROWS rows per (angle, linear) cell, all cells in one array.  dict(model, q0, q1, v, theta [n], cell [n])"""
    if k not in _CASES:
        model = _fk_models()[k]
        rng = np.random.default_rng(1000 + k)
        q0, v, theta = [], [], []
        for angle in ANGLES:
            for linear in LINEAR:
                q0.append(model.random_configurations(rng, ROWS))
                v += [_velocity(model, rng, angle, linear) for _ in range(ROWS)]
                theta += [angle] * ROWS
        q0, v = np.concatenate(q0), np.array(v)
        _CASES[k] = dict(model=model, q0=q0, v=v, q1=_integrate_rows(model, q0, v), theta=np.array(theta))
    return _CASES[k]


def check_edges(what, model, q0, q1, v, got):
    """|v_ang - v0| <= EDGE_REL theta + EDGE_ABS per group block, |v_lin - v0| <= EDGE_REL |v0| + EDGE_ABS max(1, |q0|_inf, |q1|_inf) per
    linear block, in the Euclidean norm of the block.  Prints the largest errors before it asserts"""
    assert got.shape == v.shape and np.all(np.isfinite(got)), what
    ang, lin = blocks(model)
    size = np.maximum(1.0, np.maximum(np.abs(q0).max(axis=1), np.abs(q1).max(axis=1)))
    largest, beyond, failures = {"angular": 0.0, "linear": 0.0}, 0.0, []
    for kind, blks, floor in (("angular", ang, EDGE_ABS), ("linear", lin, EDGE_ABS * size)):
        for iv, m in blks:
            e = np.linalg.norm(got[:, iv:iv + m] - v[:, iv:iv + m], axis=1)
            rel = EDGE_REL * np.linalg.norm(v[:, iv:iv + m], axis=1)
            largest[kind] = max(largest[kind], float(e.max()))
            beyond = max(beyond, float(np.max((e - rel) / (floor / EDGE_ABS))))
            failures += [(kind, iv, int(r), float(e[r]), float(rel[r])) for r in np.flatnonzero(e > rel + floor)[:1]]
    print("motion_measured difference edges %s: %d rows, max |dv_ang| %.3e, max |dv_lin| %.3e, largest error beyond the relative part %.3e (floor %.1e)"
          % (what, q0.shape[0], largest["angular"], largest["linear"], beyond, EDGE_ABS))
    assert not failures, (what, failures)


def same_configuration(model, qa, qb):
    """max |qa - qb| / max(1, |qb|_inf) per row, a quaternion block compared up to its sign"""
    qa = qa.copy()
    for o, n in MP.unit_blocks(model):
        if n == 4:
            flip = (qa[:, o:o + 4] * qb[:, o:o + 4]).sum(axis=1) < 0
            qa[flip, o:o + 4] *= -1.0
    return np.abs(qa - qb).max(axis=1) / np.maximum(1.0, np.abs(qb).max(axis=1))


def check_round_trip(what, model, q0, q1, got):
    """where v is not unique: integrate(q0, v_got) is q1 as a configuration within TOL, and no angular block is longer than pi"""
    assert np.all(np.isfinite(got)), what
    back = same_configuration(model, _integrate_rows(model, q0, got), q1)
    longest = max([float(np.linalg.norm(got[:, iv:iv + n], axis=1).max()) for _, iv, n in MP.angular_dofs(model)] or [0.0])
    print("motion_measured difference round trip %s: max |q0 (+) v - q1| / max(1, |q|_inf) %.3e, longest angular block pi + %.3e"
          % (what, back.max(), longest - np.pi))
    assert back.max() <= TOL, (what, int(back.argmax()), back.max())
    assert longest <= np.pi * (1 + 1e-15), (what, longest)


def beyond_case(k, angle, rows=4):
    """tree k with every group joint stepping by `angle` (pi, or more): (model, q0, q1)"""
    model = _fk_models()[k]
    rng = np.random.default_rng(1100 + k)
    q0 = model.random_configurations(rng, len(LINEAR) * rows)
    v = np.array([_velocity(model, rng, angle, LINEAR[r % len(LINEAR)]) for r in range(q0.shape[0])])
    return model, q0, _integrate_rows(model, q0, v)


def planar_tree():
    """the planar-root tree of test_integrate_edges.py"""
    model = random_tree_multidof(seed=31, nb=7, root_freeflyer=False, n_spherical=0, n_translation=0, n_zyx=1, n_planar=1, n_rub=2,
                                 root_planar=True)
    assert int(model.jtype[1]) == P.J_PLANAR and int(model.parents[1]) == 0
    return model


PLANAR_EDGES = [1e-4 * (1 - 1e-3), 1e-4 * (1 + 1e-3), -1e-4 * (1 - 1e-3), -1e-4 * (1 + 1e-3), np.pi - 1e-12, -(np.pi - 1e-12)]
REVOLUTE_EDGES = [1e-200, -1e-200, 1e-9, -1e-9, np.pi - 1e-12, -(np.pi - 1e-12)]


def planar_case():
    """the planar root joint: relative angles log-uniform in 1e-9 .. 1e-4 (64 rows, either sign) and PLANAR_EDGES (4 rows each) under a
    planar offset of norm PLANAR_OFFSET, every other step of size 1e-3; then +pi and -pi: (model, q0, v, q1, rows whose v is unique)"""
    model = planar_tree()
    iv = int(model.idx_v[1])
    rng = np.random.default_rng(1200)
    w = np.concatenate([rng.choice([-1.0, 1.0], size=64) * 10.0 ** rng.uniform(-9, -4, size=64), np.repeat(PLANAR_EDGES, 4), [np.pi] * 4, [-np.pi] * 4])
    q0 = model.random_configurations(rng, w.size)
    v = 1e-3 * rng.uniform(-1.0, 1.0, size=(w.size, model.nv))
    ang = rng.uniform(0, 2 * np.pi, size=w.size)
    v[:, iv], v[:, iv + 1], v[:, iv + 2] = PLANAR_OFFSET * np.cos(ang), PLANAR_OFFSET * np.sin(ang), w
    return model, q0, v, _integrate_rows(model, q0, v), np.abs(w) < np.pi


def revolute_case():
    """the unbounded revolute joints of multidof13 at REVOLUTE_EDGES (4 rows each), every other group joint at an angle of 0.3; then
    +pi and -pi: (model, q0, v, q1, rows whose v is unique)"""
    model = _fk_models()[3]
    rub = [iv for jt, iv, n in MP.angular_dofs(model) if jt in (P.J_RUBX, P.J_RUBY, P.J_RUBZ, P.J_RUBU)]
    assert len(rub) == 3
    rng = np.random.default_rng(1300)
    w = np.concatenate([np.repeat(REVOLUTE_EDGES, 4), [np.pi] * 4, [-np.pi] * 4])
    q0 = model.random_configurations(rng, w.size)
    v = np.array([_velocity(model, rng, 0.3, 1.0) for _ in range(w.size)])
    for iv in rub:
        v[:, iv] = w
    return model, q0, v, _integrate_rows(model, q0, v), np.abs(w) < np.pi


# ---- 1. the sweep ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", TREES)
def test_numpy_difference_inverts_the_group_exponential(k):
    c = edge_case(k)
    model = c["model"]
    assert c["q0"].shape == (len(ANGLES) * len(LINEAR) * ROWS, model.nq)
    for o, n in MP.unit_blocks(model):   # (what the bound relies on: unit to an ulp)
        assert np.max(np.abs(np.linalg.norm(c["q1"][:, o:o + n], axis=1) - 1.0)) <= 4e-16
    check_edges("numpy %s" % model.name, model, c["q0"], c["q1"], c["v"], MN.difference(model, c["q0"], c["q1"]))


def test_the_sweep_reaches_every_branch():
    """free-flyer, spherical, planar and (cos, sin) joints all occur, and the angles sit on both sides of every switch"""
    kinds = set()
    for k in TREES:
        kinds |= {jt for jt, _, _ in MP.angular_dofs(_fk_models()[k])}
    assert {P.J_FREEFLYER, P.J_SPHERICAL, P.J_PLANAR} <= kinds and kinds & {P.J_RUBX, P.J_RUBY, P.J_RUBZ, P.J_RUBU}
    a = np.array(ANGLES)
    for switch in (1e-4, 1e-3, SWITCH_08):
        assert (a < switch).any() and (a > switch).any() and np.min(np.abs(a - switch)) <= 1e-3 * switch
    assert a.max() == np.pi - 1e-12 and a.min() == 0.0


# ---- 2. at pi and beyond -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angle", [np.pi, 4.0], ids=["pi", "4"])
@pytest.mark.parametrize("k", TREES)
def test_numpy_difference_at_pi_and_beyond(k, angle):
    model, q0, q1 = beyond_case(k, angle)
    check_round_trip("numpy %s at %.3f" % (model.name, angle), model, q0, q1, MN.difference(model, q0, q1))


# ---- 3. the planar joint and the unbounded revolute ----------------------------------------------------------------------------------
def test_numpy_planar_joint_small_angles_under_a_large_offset():
    """(vx, vy) = V(w)^-1 R0^T (t1 - t0): with (1 - cos w) / w written as that quotient the rounding of cos w costs 1e-16 / |w| of |v|,
    4e-9 at |w| = 1e-8, which is what integrate once lost"""
    model, q0, v, q1, unique = planar_case()
    got = MN.difference(model, q0, q1)
    check_edges("numpy planar root", model, q0[unique], q1[unique], v[unique], got[unique])
    check_round_trip("numpy planar root at +-pi", model, q0[~unique], q1[~unique], got[~unique])


def test_numpy_unbounded_revolute_at_its_edges():
    model, q0, v, q1, unique = revolute_case()
    got = MN.difference(model, q0, q1)
    check_edges("numpy (cos, sin) joints", model, q0[unique], q1[unique], v[unique], got[unique])
    check_round_trip("numpy (cos, sin) joints at +-pi", model, q0[~unique], q1[~unique], got[~unique])


# ---- 4. a quaternion that is not unit -------------------------------------------------------------------------------------------------
def test_a_quaternion_off_the_unit_sphere_costs_four_times_its_defect():
    """include/loik_amd_motion.h: the rotation of a quaternion block is taken without normalising it (Eigen's toRotationMatrix, as the
    reference library does): a block of norm 1 + e gives R + 2 e (R - I).  In a free-flyer block of q0 that moves the angular part of v
    by 2 e |sin theta_0| at most (theta_0 the angle of q0's own rotation, not of the step) and the linear part R0^T (t1 - t0) by
    2 e |(R0 - I)^T (t1 - t0)| <= 4 e |t1 - t0|, whatever the angular step: recorded here with e = 1e-12 against an angular step of 1e-9
    under a linear step of 1, where it is some thousandths of the step"""
    e = 1e-12
    worst, bound = 0.0, 0.0
    for k in (2, 3):
        c = edge_case(k)
        model = c["model"]
        rows = np.flatnonzero(c["theta"] == 1e-9)[:ROWS]   # (the cell with the unit linear step)
        q0, q1 = c["q0"][rows].copy(), c["q1"][rows]
        clean = MN.difference(model, q0, q1)
        assert int(model.jtype[1]) == P.J_FREEFLYER and int(model.idx_q[1]) == 0   # (the root: t in q[0:3], its quaternion in q[3:7])
        q0[:, 3:7] *= 1.0 + e
        bound = max(bound, float(np.linalg.norm(q1[:, :3] - q0[:, :3], axis=1).max()))
        worst = max(worst, float(np.max(np.abs(MN.difference(model, q0, q1) - clean))))
    print("motion_measured difference: a quaternion norm of 1 + %.0e moves v by %.3e = %.2f e (largest |t1 - t0| %.3f)" % (e, worst, worst / e, bound))
    assert 0.9 < bound < 1.1
    assert 1.0 * e <= worst <= 4.0 * e * bound * (1 + 1e-3), worst
