"""GPU: joint acceleration limits with braking-aware position limits in the pose loops (include/loik_amd_accel.h) against the
lock-step CPU oracle built on the same rule (tests/pose_accel_numpy.py, proven on the CPU by tests/test_pose_accel_oracle.py).
The parity gate is tests/test_pose_parity.py's: on the oracle's strided subset, the same reached / steps on >= 99 % of the
instances, |dq| < 1e-7 on those, and flags differing on <= 1 % of those.  Every parity workload is built so that the
acceleration window binds, which is asserted on the ORACLE's output (_assert_binds): on 25 % to 75 % of the instances some
DoF's z sits on an edge of its window in some step, >= 10 % reached, >= 10 % not."""
import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from test_engines import ENGINES
from test_pose_ik import BOUND, PRM, _links
from test_pose_parity import ENGINE_ENV, _box, _gate, _handle, _nonsym_A, _subset
from test_pose_limits import LAWS, TOL, _assert_contained, _limited, _workload
from test_pose_track import _smp_of, _track_workload
import pose_numpy as P
import pose_limits_numpy as PL
import pose_track_numpy as TR
import pose_accel_numpy as PA

pytestmark = pytest.mark.gpu

ADT = (1e-4, 1e-3)   # a dt, as a fraction of BOUND, uniform in this range on the DoFs that carry an acceleration limit


def _accel_workload(case, dt, adt=ADT):
    """test_pose_limits._workload (position limits by binding_limits) plus a_max on a seeded half of the DoFs"""
    w = _workload(*case)
    w["a_max"] = PA.accel_limits(w["model"], case[-1] + 3, dt, BOUND, *adt)
    return w


def _oracle(w, idx, dt, gain, k, prm=PRM):
    A, (lb, ub) = w["A"], w["box"]
    return PA.lockstep_pose_loop_accel(w["model"], prm, w["q0"][idx], np.eye(6), np.zeros(6), w["links"], A[idx] if A.ndim == 4 else A,
                                       lb[idx] if lb.ndim == 2 else lb, ub[idx] if ub.ndim == 2 else ub, w["tg"][idx], dt, gain, TOL, k,
                                       w["q_lo"], w["q_hi"], w["a_max"])


def _assert_binds(o, what):
    """the conditions on the oracle's result that make a parity case mean something"""
    edge, reached = o["edge"].mean(), o["reached"].mean()
    print("%s: oracle edge-active %.3f reached %.3f steps %s" % (what, edge, reached, np.bincount(o["steps"]).tolist()))
    assert 0.25 <= edge <= 0.75, (what, edge)
    assert reached >= 0.10 and 1.0 - reached >= 0.10, (what, reached)


def _solve(w, dt, gain, k, prm=PRM, precision=capi.F64, **kw):
    s = _handle(w["model"], w["B"], w["links"], w["q0"], w["A"], prm, precision=precision, box=w["box"], **kw)
    s.set_joint_limits(w["q_lo"], w["q_hi"])
    s.set_joint_accel_limits(w["a_max"])
    out = s.SolvePose(w["tg"], dt=dt, gain=gain, tol_pose=TOL, max_steps=k)
    out["velocity"] = s.get_applied_velocity()
    return s, out, s.get("q")


def _parity(w, out, q, o, idx, what):
    same = _gate(out, q, o, idx, what)
    _assert_contained(w, q, what)
    # (a flag is a comparison of two numbers that differ by the parity gate's 1e-7 at most between device and oracle)
    assert (out["limit_flags"][idx][same] != o["limit_flags"][same]).any(axis=1).mean() <= 0.01, what
    assert np.array_equal(out["status"][idx][same] & 9, o["status"][same] & 9)
    assert np.max(np.abs(out["velocity"][idx][same] - o["velocity"][same])) < 1e-7, what
    return same


# ---- 1. parity with the lock-step oracle: SolvePose ------------------------------------------------------------------------------
PARITY = [
    # (robot, nc, B, A per instance, base box per instance, percentiles of the position limits, seed)
    ("talos32", 1, 193, False, False, (2.0, 98.0), 5100),
    ("talos32", 2, 256, True, True, (2.0, 98.0), 5200),
    ("panda7", 1, 193, False, False, (5.0, 95.0), 5300),
    ("multidof", 2, 193, True, False, (5.0, 95.0), 5400),
]


@pytest.mark.parametrize("law", LAWS, ids=lambda l: "dt%g-g%g" % l)
@pytest.mark.parametrize("case", PARITY, ids=lambda c: "%s-nc%d-B%d-%s-%s" % (c[0], c[1], c[2], "Ainst" if c[3] else "Ash", "boxinst" if c[4] else "boxsh"))
def test_accel_limits_match_lockstep_oracle(case, law):
    dt, gain = law
    w = _accel_workload(case, dt)
    idx = _subset(w["B"])
    for k in (1, 4):
        s, out, q = _solve(w, dt, gain, k)
        s.close()
        o = _oracle(w, idx, dt, gain, k)
        _assert_binds(o, (case, law, k))
        same = _parity(w, out, q, o, idx, (case, law, k))
        assert (o["limit_flags"] & 12).any() and (out["limit_flags"] & 12).any()
        if k == 4:
            assert (o["limit_flags"] & 3).any()
        if case[0] == "multidof":   # a finite acceleration limit sits on a DoF that can carry no position limit (the free-flyer's)
            assert np.isfinite(w["a_max"][PL.limit_q_index(w["model"]) < 0]).any()


# ---- 2. parity with the lock-step oracle: TrackPose --------------------------------------------------------------------------------
def _track_problem(B, T, seed, dt, name="talos32", nc=1, adt=ADT):
    model = loik_amd.builtin_model(name)
    links = _links(model, nc)
    A = _nonsym_A(np.random.default_rng(seed), nc)
    q0, smp, q_path = _track_workload(model, links, B, T, seed=seed + 1)
    q_lo, q_hi, q0 = PL.binding_limits(model, q_path[:, T], q0, seed + 2)
    return dict(model=model, links=links, A=A, q0=q0, smp=smp, q_path=q_path, q_lo=q_lo, q_hi=q_hi, box=_box(model), B=B,
                a_max=PA.accel_limits(model, seed + 3, dt, BOUND, *adt))


def _track_oracle(w, idx, dt, gain, ff, v0=None, smp=None, q0=None):
    lb, ub = w["box"]
    return PA.lockstep_track_loop_accel(w["model"], PRM, (w["q0"] if q0 is None else q0)[idx], np.eye(6), np.zeros(6), w["links"], w["A"], lb, ub,
                                        _smp_of(w["smp"] if smp is None else smp, idx), dt, gain, TOL, w["q_lo"], w["q_hi"], w["a_max"], v0=v0,
                                        ff=TR.FF_NONE if ff == "none" else TR.FF_DIFFERENCE)


def _track_handle(w, limits=True, accel=True, precision=capi.F64, prm=PRM):
    s = _handle(w["model"], w["B"], w["links"], w["q0"], w["A"], prm, precision=precision, box=w["box"])
    if limits:
        s.set_joint_limits(w["q_lo"], w["q_hi"])
    if accel:
        s.set_joint_accel_limits(w["a_max"])
    return s


@pytest.mark.parametrize("ff", ["none", "difference"])
def test_track_with_accel_limits_matches_lockstep_oracle(ff):
    dt, gain, T = 0.5, 0.8, 6
    w = _track_problem(193, T, 5500, dt)
    s = _track_handle(w)
    out = s.TrackPose(w["smp"], dt=dt, gain=gain, tol_track=TOL, feedforward=ff)
    vel = s.get_applied_velocity()
    s.close()
    idx = _subset(w["B"])
    o = _track_oracle(w, idx, dt, gain, ff)
    edge = o["edge"].mean()
    print("track %s: oracle edge-active %.3f, inner & 12 on %.3f of the steps" % (ff, edge, ((o["inner"] & 12) != 0).mean()))
    assert edge >= 0.25 and ((o["inner"] & 8) != 0).any() and ((o["inner"] & 4) != 0).any()
    for key in ("q_traj", "z_traj"):
        assert np.array_equal(np.isnan(out[key][idx]), np.isnan(o[key])), key
        d = np.abs(out[key][idx] - o[key])
        print("track %s: max |d %s| %.3e" % (ff, key, np.nanmax(d)))
        assert np.nanmax(d) < 1e-7, (ff, key, np.nanmax(d))
    # (a flag is a comparison of two numbers that differ by 1e-7 at most between device and oracle: the allowance of the flags above)
    assert ((out["inner"][idx] & 12) != (o["inner"] & 12)).any(axis=1).mean() <= 0.01
    assert np.max(np.abs(vel[idx] - o["velocity"])) < 1e-7
    assert np.array_equal(vel, out["z_traj"][:, T - 1])


# ---- 3. the guarantee on the device's own output ------------------------------------------------------------------------------------
def _jump_problem(B, T, at, size, seed, dt):
    """_track_problem whose samples jump at sample `at`: the joint path from there on is moved by `size` (inf-norm) in joint space"""
    w = _track_problem(B, T, seed, dt)
    model, rng = w["model"], np.random.default_rng(seed + 4)
    v = rng.normal(size=(B, model.nv))
    v *= size / np.abs(v).max(axis=1, keepdims=True)
    qp = w["q_path"].copy()
    for b in range(B):
        for k in range(at, T + 1):
            qp[b, k] = P.integrate(model, qp[b, k], v[b])
    w["smp"] = np.stack([P.fk12(model, qp[:, k], w["links"]) for k in range(T + 1)], axis=1)
    return w


@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
def test_device_trajectory_obeys_the_bound_and_stays_in_range(precision):
    dt, gain, T = 0.5, 0.8, 8
    w = _jump_problem(193, T, 3, 0.1, 5600, dt)
    fin = np.isfinite(w["a_max"])
    s_lim = w["a_max"][fin] * dt
    ci, lo, hi = _limited(w)
    _assert_contained(w, w["q0"], "seeds")
    viol = {}
    for accel in (True, False):
        s = _track_handle(w, accel=accel, precision=precision)
        out = s.TrackPose(w["smp"], dt=dt, gain=gain, tol_track=TOL, feedforward="difference")
        s.close()
        assert not np.isnan(out["z_traj"]).any() and np.all(out["steps"] == T)
        z = np.concatenate([np.zeros((w["B"], 1, w["model"].nv)), out["z_traj"]], axis=1)[:, :, fin]
        dz, zp = np.abs(np.diff(z, axis=1)), np.abs(z[:, :-1])
        # fp64: rounding of the window's edges; fp32: each edge of the box is rounded to fp32 once
        bound = s_lim * (1.0 + 1e-12) if precision == capi.F64 else s_lim + 2.0 ** -22 * (zp + s_lim)
        viol[accel] = (dz > bound).any(axis=(1, 2))
        print("accel %s precision %d: worst dz / s %.15f, instances over the bound %.3f" % (accel, precision, (dz / s_lim).max(), viol[accel].mean()))
        qt = out["q_traj"][:, :, ci]
        assert np.all(lo <= qt) and np.all(qt <= hi), (accel, float(np.maximum(lo - qt, qt - hi).max()))   # exactly: plain <=
        if accel:
            assert (out["inner"] & capi.TRACK_IN_ACCEL).any() and (out["limit_flags"] & 12).any()
        else:
            assert not (out["inner"] & capi.TRACK_IN_ACCEL).any() and not (out["limit_flags"] & 12).any()
    assert not viol[True].any()
    assert viol[False].mean() >= 0.25, viol[False].mean()   # teeth: without the limits the same run breaks the bound


# ---- 4. every engine: one that captured the box-sharing mode before the launch would solve with the base box ---------------------
_ENGINE_CACHE = {}
ENGINE_CASE = ("talos32", 1, 193, False, False, (2.0, 98.0), 5100)
ENGINE_LAW = LAWS[0]


def _engine_problem():
    if not _ENGINE_CACHE:
        dt, gain = ENGINE_LAW
        w = _accel_workload(ENGINE_CASE, dt)
        idx = _subset(w["B"])
        o = _oracle(w, idx, dt, gain, 4)
        _assert_binds(o, "engines")
        _ENGINE_CACHE.update(w=w, idx=idx, o=o)
    return _ENGINE_CACHE["w"], _ENGINE_CACHE["idx"], _ENGINE_CACHE["o"]


@pytest.mark.parametrize("engine", list(ENGINES))
def test_every_engine_honours_the_dynamic_box(engine, monkeypatch):
    w, idx, o = _engine_problem()
    for v in ENGINE_ENV:
        monkeypatch.delenv(v, raising=False)
    env, kw = ENGINES[engine]
    for v, x in env.items():
        monkeypatch.setenv(v, x)
    s, out, q = _solve(w, *ENGINE_LAW, 4, **kw)
    s.close()
    _parity(w, out, q, o, idx, engine)
    assert np.any(out["steps"] > 1)


# ---- 5. chaining: one call over 8 samples is two calls over 4 + 4 -------------------------------------------------------------------
@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_two_chained_calls_are_one(warm, route):
    dt, gain, T = 0.5, 0.8, 8
    w = _jump_problem(193, T, 3, 0.1, 5700, dt)
    prm = dict(PRM, warm_start=warm)
    kw = dict(dt=dt, gain=gain, tol_track=TOL, feedforward="difference")
    s = _track_handle(w, prm=prm)
    whole = s.TrackPose(w["smp"], **kw)
    s.close()
    s = _track_handle(w, prm=prm)
    first = s.TrackPose(w["smp"][:, :5], **kw)
    if route == "device":   # anything with data_ptr() goes in and out
        dev = capi.DeviceArray(np.zeros((w["B"], w["model"].nv)))
        s.get_applied_velocity(out=dev)
        s.set_start_velocity(dev)
    else:
        v = s.get_applied_velocity()
        assert np.array_equal(v, first["z_traj"][:, 3])
        s.set_start_velocity(v)
    second = s.TrackPose(w["smp"][:, 4:], **kw)
    s.close()
    q2 = np.concatenate([first["q_traj"], second["q_traj"][:, 1:]], axis=1)
    z2 = np.concatenate([first["z_traj"], second["z_traj"]], axis=1)
    assert (whole["inner"][:, 4] & capi.TRACK_IN_ACCEL).any()   # the start velocity matters at the seam
    if warm:
        assert np.max(np.abs(q2 - whole["q_traj"])) < 1e-7 and np.max(np.abs(z2 - whole["z_traj"])) < 1e-7
    else:
        assert np.array_equal(q2, whole["q_traj"]) and np.array_equal(z2, whole["z_traj"])
    # ... and without the start velocity the seam shows: the second call starts from rest
    if route == "host" and not warm:
        s = _track_handle(w, prm=prm)
        s.TrackPose(w["smp"][:, :5], **kw)
        rest = s.TrackPose(w["smp"][:, 4:], **kw)
        s.close()
        assert np.max(np.abs(rest["z_traj"][:, 0] - whole["z_traj"][:, 4])) > 1e-4


def test_one_waypoint_path_is_solve_pose_bit_for_bit():
    """SolvePosePath goes through the same step: one waypoint without a per-waypoint bound is SolvePose, limits of both kinds on"""
    dt, gain = LAWS[0]
    w = _accel_workload(PARITY[0], dt)
    res = []
    for path in (False, True):
        s = _handle(w["model"], w["B"], w["links"], w["q0"], w["A"], PRM, box=w["box"])
        s.set_joint_limits(w["q_lo"], w["q_hi"])
        s.set_joint_accel_limits(w["a_max"])
        if path:
            out = s.SolvePosePath(w["tg"][:, None], dt=dt, gain=gain, tol_pose=TOL, max_steps=4)
        else:
            out = s.SolvePose(w["tg"], dt=dt, gain=gain, tol_pose=TOL, max_steps=4)
        res.append((out, s.get("q"), s.get_applied_velocity()))
        s.close()
    (a, qa, va), (b, qb, vb) = res
    for key in ("steps", "status", "err", "limit_flags"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(qa, qb) and np.array_equal(va, vb)
    assert (a["limit_flags"] & 12).any() and va.any() and not va[a["reached"]].any()


# ---- 6. no change where nothing is set -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limits", [False, True], ids=["nolimits", "limits"])
def test_cleared_accel_limits_change_nothing(limits):
    dt, gain, T = 0.5, 0.8, 4
    w = _track_problem(193, T, 5800, dt)
    tg = w["smp"][:, T]

    def run(mode):
        s = _track_handle(w, limits=limits, accel=False)
        if mode == "cleared":
            s.set_joint_accel_limits(w["a_max"])
            s.set_start_velocity(np.ones((w["B"], w["model"].nv)))
            s.set_joint_accel_limits(None)
        elif mode == "inf":
            s.set_joint_accel_limits(np.inf * np.ones(w["model"].nv))
        res = {}
        out = s.SolvePose(tg, dt=dt, gain=gain, tol_pose=TOL, max_steps=3)
        res.update({"pose_" + k: v for k, v in out.items()}, pose_q=s.get("q"), pose_z=s.get("z"), pose_iter=s.get("iter"))
        out = s.TrackPose(w["smp"], dt=dt, gain=gain, tol_track=TOL, feedforward="difference", q=w["q0"])
        res.update({"track_" + k: v for k, v in out.items()}, track_q=s.get("q"), track_z=s.get("z"), track_iter=s.get("iter"))
        with pytest.raises(capi.LoikError) as e:
            s.get_applied_velocity()
        assert e.value.code == -24
        s.close()
        return res

    ref = run("never")
    assert ("pose_limit_flags" in ref) == limits
    for mode in ("cleared", "inf"):
        got = run(mode)
        assert set(got) == set(ref)
        for key in ref:
            assert np.array_equal(got[key], ref[key], equal_nan=True), (mode, key)


# ---- 7. errors and states -----------------------------------------------------------------------------------------------------------
def _err(fn, code):
    with pytest.raises(capi.LoikError) as e:
        fn()
    assert e.value.code == code, e.value
    return str(e.value)


def test_arguments_and_states():
    dt = 0.5
    w = _track_problem(64, 2, 5900, dt, name="panda7")
    nv = w["model"].nv
    s = _track_handle(w, limits=False, accel=False)
    _err(lambda: s.set_joint_accel_limits(np.ones(nv + 1)), -20)
    bad = np.ones(nv); bad[2] = np.nan
    assert "DoF 2" in _err(lambda: s.set_joint_accel_limits(bad), -20)
    for x in (0.0, -1.0, -np.inf):
        bad = np.ones(nv); bad[3] = x
        assert "DoF 3" in _err(lambda: s.set_joint_accel_limits(bad), -20)
    _err(lambda: s.get_applied_velocity(), -24)          # before any loop
    _err(lambda: s.pose_limit_flags(), -24)
    with pytest.raises(ValueError):
        s.set_start_velocity(np.zeros(nv))
    s.set_joint_accel_limits(w["a_max"])                  # (the rejected calls above left nothing behind)
    _err(lambda: s.get_applied_velocity(), -24)          # set, but no loop ran with them yet
    msg = _err(lambda: s.SolvePoseMultiStart(w["smp"][::2, 0], 2, q0=w["q0"][::2]), -24)
    assert "acceleration" in msg and "teleported" in msg
    # a loop that moves nothing: the velocity is 0 whatever the start velocity was; the flags are valid with acceleration limits alone
    s.set_start_velocity(np.ones((w["B"], nv)))
    out = s.SolvePose(w["smp"][:, 2], dt=dt, max_steps=0)
    assert not s.get_applied_velocity().any() and not out["limit_flags"].any()
    # the start velocity is used once: the next loop starts from rest, so its first z is within s of 0, not of 1
    out = s.TrackPose(w["smp"], dt=dt, gain=0.8, tol_track=TOL)
    fin = np.isfinite(w["a_max"])
    assert np.all(np.abs(out["z_traj"][:, 0, fin]) <= w["a_max"][fin] * dt * (1 + 1e-12))
    assert out["limit_flags"].shape == (w["B"], nv) and (out["limit_flags"] & 12).any() and not (out["limit_flags"] & 3).any()
    v = s.get_applied_velocity()
    assert np.array_equal(v, out["z_traj"][:, 1])
    # a start velocity outside the base box is led back at the rate s, not rejected
    s.set_start_velocity(3.0 * BOUND * np.ones((w["B"], nv)))
    out = s.TrackPose(w["smp"], dt=dt, gain=0.8, tol_track=TOL, q=w["q0"])
    assert np.all(out["z_traj"][:, 0, fin] == BOUND) and np.all(out["steps"] == 2)
    # cleared: multistart works again, the velocity getter says the last loop ran without
    s.set_joint_accel_limits(None)
    s.set_seed_ranges(-np.ones(nv), np.ones(nv))
    s.SolvePoseMultiStart(w["smp"][::2, 0], 2, q0=w["q0"][::2], max_steps=1)
    _err(lambda: s.get_applied_velocity(), -24)
    s.close()


def _plan_core(s):
    import re
    return re.sub(r"; device buffers:.*?room\)", "", re.sub(r"; decades visited[^;]*", "", s.plan()))


@pytest.mark.parametrize("box_inst", [False, True], ids=["boxsh", "boxinst"])
def test_base_box_is_restored(box_inst):
    """test_pose_limits.test_base_box_is_restored with acceleration limits alone on the handle: after the loop the handle solves with
    its base box again, in the sharing mode it had -- the same calls on it and on a twin that never had limits, both put on the same
    q and started cold, give bit-identical z / iter, with a b large enough that the base box binds"""
    dt = 0.25
    w = _accel_workload(("talos32", 1, 256, False, box_inst, (2.0, 98.0), 6000), dt)
    s = _handle(w["model"], w["B"], w["links"], w["q0"], w["A"], PRM, box=w["box"])
    s.set_joint_accel_limits(w["a_max"])
    plan0 = _plan_core(s)
    out = s.SolvePose(w["tg"], dt=dt, gain=0.5, tol_pose=TOL, max_steps=3)
    assert _plan_core(s) == plan0
    assert (out["limit_flags"] & 12).any() and not (out["limit_flags"] & 3).any() and np.any(out["steps"] == 3)
    q = s.get("q")
    t = _handle(w["model"], w["B"], w["links"], w["q0"], w["A"], PRM, box=w["box"])
    t.SolvePose(w["tg"], dt=dt, gain=0.5, tol_pose=TOL, max_steps=3)
    assert np.max(np.abs(t.get("q") - q)) > 1e-3
    rng = np.random.default_rng(5)
    b = rng.choice([-1.0, 1.0], size=(w["B"], 6)) * (3.0 + rng.random((w["B"], 6)))
    for h in (s, t):   # (s keeps its limits: the call that moves nothing enters and leaves the per-instance mode once more)
        h.set_warm_start(False)
        h.SolvePose(w["tg"], dt=dt, gain=0.5, tol_pose=TOL, max_steps=0, q=q)
        h.UpdateEqConstraint(w["links"][0], b)
        h.Solve(None, -1, None, None)
        h.Solve()
    zs, its = s.get("z"), s.get("iter")
    zt, itt = t.get("z"), t.get("iter")
    assert _plan_core(s) == _plan_core(t)
    s.close()
    t.close()
    assert np.array_equal(its, itt) and np.array_equal(zs, zt)
    lb, ub = w["box"]
    assert np.all(zs >= lb) and np.all(zs <= ub)
    assert ((zs == np.broadcast_to(lb, zs.shape)) | (zs == np.broadcast_to(ub, zs.shape))).any(), "the base box never binds: the test shows nothing"
