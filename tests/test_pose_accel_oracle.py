"""CPU: the rule of include/loik_amd_accel.h and the lock-step oracle built on it (tests/pose_accel_numpy.py) are proven before
they referee the device.
 (a) an adversarial simulation of the rule alone: whatever is picked inside [lo, hi] -- the upper edge, the lower edge, a random
     point -- the box is never empty, the velocity changes by a dt at most, and a coordinate that starts in range at rest stays
     in range before any clamp;
 (b) with a = inf dyn_box IS pose_limits_numpy.step_box;
 (c) with a = inf the two lock-step loops ARE lockstep_pose_loop_limits and lockstep_track_loop(q_lo=...): np.array_equal."""
import numpy as np
import pytest

import loik_amd

from test_pose_ik import PRM, _links
from test_pose_parity import _box, _nonsym_A, _seeds
import pose_limits_numpy as PL
import pose_track_numpy as TR
import pose_accel_numpy as PA

N_TRAJ = 64     # DoFs simulated side by side per (dt, pick)
N_STEPS = 200


@pytest.mark.parametrize("pick", ["hi", "lo", "random", "bang"])
@pytest.mark.parametrize("dt", [0.01, 0.25, 2.0])
def test_rule_keeps_its_invariant_under_any_choice_inside_the_box(dt, pick):
    """each DoF of one dyn_box call is an independent 1-DoF trajectory: random ranges, boxes and a in 10^[-2, 2], a start in range at
    rest; "bang" switches between the edges at random.  The excursion bound 1e-13 is rounding: the issue's run over 20 000
    trajectories saw 4e-15."""
    rng = np.random.default_rng(int(1000 * dt) + len(pick))
    n = N_TRAJ
    a = 10.0 ** rng.uniform(-2, 2, size=n)
    q_lo = rng.uniform(-2, 0, size=n)
    q_hi = q_lo + 10.0 ** rng.uniform(-3, 0.5, size=n)
    lb, ub = -10.0 ** rng.uniform(-2, 1, size=n), 10.0 ** rng.uniform(-2, 1, size=n)
    one = rng.random(n) < 0.2          # a fifth of the DoFs with one limit only
    q_lo[one & (np.arange(n) % 2 == 0)] = -np.inf
    q_hi[one & (np.arange(n) % 2 == 1)] = np.inf
    lo_f, hi_f = np.where(np.isfinite(q_lo), q_lo, -3.0), np.where(np.isfinite(q_hi), q_hi, 3.0)
    q = rng.uniform(lo_f, hi_f)
    zp = np.zeros(n)
    s = a * dt
    qidx = np.arange(n)
    worst_exc, worst_acc = 0.0, 0.0
    for step in range(N_STEPS):
        lo, hi, flags, inside = PA.dyn_box(q, zp, a, q_lo, q_hi, lb, ub, dt, qidx)
        assert np.all(lo <= hi), (dt, pick, step)
        assert np.all(lb <= lo) and np.all(hi <= ub)
        if pick == "hi":
            z = hi
        elif pick == "lo":
            z = lo
        elif pick == "random":
            z = lo + rng.random(n) * (hi - lo)
            z = np.minimum(np.maximum(z, lo), hi)
        else:
            z = np.where(rng.random(n) < 0.5, lo, hi)
        acc = np.abs(z - zp) / s
        worst_acc = max(worst_acc, float(acc.max()))
        assert np.all(np.abs(z - zp) <= s * (1.0 + 1e-12)), (dt, pick, step, float(acc.max()))
        q = q + dt * z
        exc = np.maximum(q_lo - q, q - q_hi).max()
        worst_exc = max(worst_exc, float(exc))
        assert exc < 1e-13, (dt, pick, step, float(exc))
        zp = z
    print("accel rule dt %g pick %s: worst |dz| / s = %.15f, worst excursion %.3e" % (dt, pick, worst_acc, worst_exc))
    if pick in ("hi", "lo"):   # the case means something: joints ran up to a limit and came to rest on it
        side = q_hi if pick == "hi" else q_lo
        fin = np.isfinite(side)
        assert np.mean(np.abs(q - side)[fin] < 1e-9) > 0.5


def test_vmax_is_the_inverse_of_the_braking_distance():
    rng = np.random.default_rng(7)
    dt, s = 0.25, 10.0 ** rng.uniform(-3, 1, size=2000)
    d = 10.0 ** rng.uniform(-6, 1, size=2000)
    v = PA.vmax(d, s, dt)
    dist = np.zeros_like(v)
    z = v.copy()
    while np.any(z > 0):
        dist += dt * np.maximum(z, 0)
        z = z - s
    assert np.all(np.abs(dist - d) <= 1e-12 * np.maximum(d, 1.0))
    # the guards: beyond the limit, no acceleration limit, no position limit
    assert PA.vmax(np.array([-0.5]), np.array([1.0]), dt)[0] == -0.5 / dt
    assert PA.vmax(np.array([0.5]), np.array([np.inf]), dt)[0] == 0.5 / dt
    assert PA.vmax(np.array([np.inf]), np.array([1.0]), dt)[0] == np.inf
    assert PA.vmax(np.array([0.0]), np.array([1.0]), dt)[0] == 0.0


def test_infinite_a_is_step_box():
    rng = np.random.default_rng(11)
    model = loik_amd.builtin_model("talos32")
    qidx = PL.limit_q_index(model)
    nv = model.nv
    for trial in range(200):
        dt = [0.01, 0.25, 2.0][trial % 3]
        q = model.random_configurations(rng, 1)[0]
        q_lo, q_hi = -np.inf * np.ones(nv), np.inf * np.ones(nv)
        pick = rng.random(nv) < 0.6
        c = q[qidx]
        q_lo[pick] = c[pick] + rng.uniform(-1, 0.2, size=pick.sum())     # (some coordinates start outside their range)
        q_hi[pick] = np.maximum(q_lo[pick], c[pick] + rng.uniform(-0.2, 1, size=pick.sum()))
        q_lo[pick & (rng.random(nv) < 0.2)] = -np.inf
        q_hi[pick & (rng.random(nv) < 0.2)] = np.inf
        lb, ub = -10.0 ** rng.uniform(-2, 1, size=nv), 10.0 ** rng.uniform(-2, 1, size=nv)
        assert np.all(lb < ub)
        zp = rng.normal(size=nv)
        want = PL.step_box(q, q_lo, q_hi, lb, ub, dt, qidx)
        got = PA.dyn_box(q, zp, np.inf * np.ones(nv), q_lo, q_hi, lb, ub, dt, qidx)
        for g, w, key in zip(got, want, ("lo", "hi", "flags", "inside")):
            assert np.array_equal(g, w), (trial, key)
        assert want[2].any()


B = 12
TOL = 1e-4


@pytest.mark.parametrize("name,nc,per_inst", [("talos32", 2, True), ("panda7", 1, False)])
def test_infinite_a_reproduces_the_limits_oracles(name, nc, per_inst):
    model = loik_amd.builtin_model(name)
    links = _links(model, nc)
    rng = np.random.default_rng(950 + nc)
    A = _nonsym_A(rng, nc, B if per_inst else None)
    lb, ub = _box(model)
    inf = np.inf * np.ones(model.nv)
    # SolvePose
    q0, tg = _seeds(model, B, links, seed=951, spread=(1e-7, 0.15))
    q_t = model.random_configurations(np.random.default_rng(951), B)
    q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, seed=952, pct=(5.0, 95.0))
    for dt, gain in ((0.25, 0.5), (2.0, 1.7)):
        want = PL.lockstep_pose_loop_limits(model, PRM, q0, np.eye(6), np.zeros(6), links, A, lb, ub, tg, dt, gain, TOL, 4, q_lo, q_hi)
        got = PA.lockstep_pose_loop_accel(model, PRM, q0, np.eye(6), np.zeros(6), links, A, lb, ub, tg, dt, gain, TOL, 4, q_lo, q_hi, inf)
        for key in ("q", "steps", "status", "z", "iter", "err", "limit_flags"):
            assert np.array_equal(got[key], want[key]), (name, dt, key)
        assert want["limit_flags"].any() and len(set(want["steps"].tolist())) > 1
        assert not got["edge"].any()
    # TrackPose
    T = 4
    q_a, smp, q_path = TR.joint_path_workload(model, links, B, T, seed=953)
    q_lo, q_hi, q_a = PL.binding_limits(model, q_path[:, T], q_a, 954)
    for ff in (TR.FF_NONE, TR.FF_DIFFERENCE):
        want = TR.lockstep_track_loop(model, PRM, q_a, np.eye(6), np.zeros(6), links, A, lb, ub, smp, 0.5, 0.8, TOL, ff=ff, q_lo=q_lo, q_hi=q_hi)
        got = PA.lockstep_track_loop_accel(model, PRM, q_a, np.eye(6), np.zeros(6), links, A, lb, ub, smp, 0.5, 0.8, TOL, q_lo, q_hi, inf, ff=ff)
        for key in want:
            assert np.array_equal(got[key], want[key], equal_nan=True), (name, ff, key)
        assert (want["inner"] & TR.IN_LIMIT).any()
        assert np.array_equal(got["velocity"], want["z_traj"][:, T - 1])


def test_finite_a_bounds_the_oracle_loops():
    """the oracle's own trajectories obey the bound with finite limits, and the limits bind (the loops differ from the a = inf ones)"""
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 1)
    A = _nonsym_A(np.random.default_rng(960), 1)
    lb, ub = _box(model)
    T, dt = 6, 0.5
    q_a, smp, q_path = TR.joint_path_workload(model, links, B, T, seed=961)
    q_lo, q_hi, q_a = PL.binding_limits(model, q_path[:, T], q_a, 962)
    a = PA.accel_limits(model, 963, dt, ub[0], 1e-3, 1e-2)
    o = PA.lockstep_track_loop_accel(model, PRM, q_a, np.eye(6), np.zeros(6), links, A, lb, ub, smp, dt, 0.8, TOL, q_lo, q_hi, a)
    z = np.concatenate([np.zeros((B, 1, model.nv)), o["z_traj"]], axis=1)
    fin = np.isfinite(a)
    assert np.all(np.abs(np.diff(z, axis=1))[:, :, fin] <= (a[fin] * dt) * (1 + 1e-12))
    assert o["edge"].any() and (o["inner"] & PA.IN_ACCEL).any()
    lim = np.isfinite(q_lo)
    ci = PL.limit_q_index(model)[lim]
    assert np.all(q_lo[lim] <= o["q_traj"][:, :, ci]) and np.all(o["q_traj"][:, :, ci] <= q_hi[lim])
