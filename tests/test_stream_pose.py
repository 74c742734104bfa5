"""The pose layer on a caller's stream behind pending work (include/loik_amd.h at loikb_set_stream: the contract): SolvePose plain, with
tasks and tool frames, with joint and acceleration limits plus step control, and with collision avoidance latched; the multi-start
(sample_seeds, SolvePoseMultiStart, its clearance pick and its dexterity pick); SolvePosePath and TrackPose; every *_get of those loops
into a device array.

One sequence of calls per robot, run twice by stream_harness.run_both: on the null stream with host arrays, and on a handle moved to
a non-blocking stream (after a SolveInit on the null stream) with a gate in front of every call, the targets, waypoints, samples and
seeds in device arrays that hold the neighbouring instance's data until a copy queued behind the gate, and every getter into a
poisoned device array read back right after the call.  Byte for byte.  Robots: panda7 and the multi-DoF tree with nq != nv of
test_pose_ik._fk_models()[3], at B = 64, on the workloads of test_pose_parity, test_pose_path and test_pose_track."""
import ctypes as C

import numpy as np
import pytest

import clearance_numpy as CN
import loik_amd
import pose_limits_numpy as PL
import pose_tasks_numpy as PT
import stream_harness as H
import test_avoid_box as TA
import test_clearance as TC
from loik_amd import capi
from test_pose_ik import PRM, _fk_models, _links
from test_pose_parity import _box, _handle, _leaf_and_multidof, _nonsym_A, _seeds
from test_pose_path import _path_workload
from test_pose_track import _track_workload

pytestmark = pytest.mark.gpu

B, K, T_PATH, T_TRACK, TOL = 64, 8, 4, 6, 1e-4
F, I = np.float64, np.int32


def _robot(name):
    if name == "multidof13":
        model = _fk_models()[3]
        return model, _leaf_and_multidof(model)
    model = loik_amd.builtin_model(name)
    return model, _links(model, 2)


def _put(run, tag, d):
    """the arrays a pose loop's binding returns (its own getters into host arrays), but for the wall-clock timings"""
    for k, v in d.items():
        if v is not None and not isinstance(v, dict) and "timing" not in k:
            run.put("%s:%s" % (tag, k), v)


def _raw(s, fn, *head):
    """a getter of the C ABI with the arguments (handle, *head, out, out_flags) -> a call for Run.get_n"""
    def call(outs):
        o = outs[0]
        p, f = (o.ctypes.data_as(C.c_void_p), 0) if isinstance(o, np.ndarray) else (C.c_void_p(o.data_ptr()), capi.OUT_DEVICE)
        rc = fn(s.h, *head, p, f)
        assert rc == 0, s.L.loikb_last_error()
    return call


def _pose_gets(run, s, tag, nc, nv, limits=False, step=False, accel=False, avoid=False):
    L = s.L
    tag += " get"
    run.get_n([tag + ":status"], _raw(s, L.loikb_pose_get, capi.POSE_F_STATUS), [((B,), I)])
    run.get_n([tag + ":steps"], _raw(s, L.loikb_pose_get, capi.POSE_F_STEPS), [((B,), I)])
    run.get_n([tag + ":err"], _raw(s, L.loikb_pose_get, capi.POSE_F_ERR), [((B, nc, 6), F)])
    run.get(tag + ":q", lambda out: s.get("q", out=out))
    if limits:
        run.get_n([tag + ":limit_flags"], _raw(s, L.loikb_pose_get_limit_flags), [((B, nv), I)])
    if step:
        for fid, name, dt in ((capi.STEP_F_ALPHA, "alpha", F), (capi.STEP_F_BACKTRACKS, "backtracks", I), (capi.STEP_F_FAILED, "failed", I)):
            run.get_n(["%s:%s" % (tag, name)], _raw(s, L.loikb_step_get, fid), [((B,), dt)])
    if accel:
        run.get_n([tag + ":applied_velocity"], _raw(s, L.loikb_accel_get_velocity), [((B, nv), F)])
    if avoid:
        for fid, name, shape, dt in ((capi.AVOID_F_MIN_SEEN, "min_seen", (B,), F), (capi.AVOID_F_ACTIVE_STEPS, "active_steps", (B,), I),
                                     (capi.AVOID_F_FLAGS, "flags", (B, nv), I)):
            run.get_n(["%s:avoid %s" % (tag, name)], _raw(s, L.loikb_avoid_get_result, fid), [(shape, dt)])


def _case(name):
    model, links = _robot(name)
    nc, nv, nq = len(links), model.nv, model.nq
    rng = np.random.default_rng(6100 + nv)
    c = dict(model=model, links=links, nc=nc, A=_nonsym_A(rng, nc))   # (shared: set_pose_tasks asks for it)
    c["q0"], c["tg"] = _seeds(model, B, links, seed=6101, spread=(1e-3, 0.3))
    c["frames"] = PT.random_frames(rng, nc)
    q_t = model.random_configurations(np.random.default_rng(6101), B)   # (what _seeds drew the targets from)
    c["q_lo"], c["q_hi"], c["q0_in"] = PL.binding_limits(model, q_t, c["q0"], 6102)
    c["a_max"] = np.where(np.arange(nv) % 2 == 0, 4.0, np.inf)
    c["v0"] = 0.05 * rng.normal(size=(B, nv))
    c["clinks"], c["spheres"] = CN.make_spheres(model, 1, 6103)
    c["ws"], c["wb"] = TC._world(rng, 6, 5)
    c["q0p"], c["wp"], _ = _path_workload(model, links, B, T_PATH, seed=6104)
    c["q0t"], c["smp"], _ = _track_workload(model, links, B, T_TRACK, seed=6105)
    G = B // K
    c["goals"] = np.ascontiguousarray(c["tg"][:G])
    c["q0g"] = np.ascontiguousarray(c["q0_in"][:G])
    return c


def _sequence(c):
    model, nc = c["model"], c["nc"]
    nv, nq, G = model.nv, model.nq, B // K
    kw = dict(dt=0.5, gain=1.0, tol_pose=TOL, max_steps=5)

    def sequence(run, s):
        L = s.L
        # ---- 1. plain, the targets and the seeds on the device
        tg, q0 = run.inp(c["tg"].reshape(B, nc, 12)), run.inp(c["q0"])
        _put(run, "plain", run.do(s.SolvePose, tg, q=q0, **kw))
        _pose_gets(run, s, "plain", nc, nv)
        # ---- 2. tasks and tool frames (a formulation edit: every A becomes the task's own)
        run.do(s.set_pose_tasks, ["position", "pose"][:nc], c["frames"])
        tg, q0 = run.inp(c["tg"].reshape(B, nc, 12)), run.inp(c["q0"])
        _put(run, "tasks", run.do(s.SolvePose, tg, q=q0, **kw))
        _pose_gets(run, s, "tasks", nc, nv)
        run.do(s.clear_pose_tasks)
        # ---- 3. joint limits with acceleration limits and a start velocity on the device, then with step control (the two together
        #      are refused: a scaled step is not the velocity the braking box was built for)
        run.do(s.set_joint_limits, c["q_lo"], c["q_hi"])
        run.do(s.set_joint_accel_limits, c["a_max"])
        run.do(s.set_start_velocity, run.inp(c["v0"]))
        tg, q0 = run.inp(c["tg"].reshape(B, nc, 12)), run.inp(c["q0_in"])
        _put(run, "accel", run.do(s.SolvePose, tg, q=q0, **kw))
        _pose_gets(run, s, "accel", nc, nv, limits=True, accel=True)
        run.do(s.set_joint_accel_limits, None)
        run.do(s.set_step_control, shrink=0.5, sufficient=1e-4, max_backtracks=3, patience=2)
        tg, q0 = run.inp(c["tg"].reshape(B, nc, 12)), run.inp(c["q0_in"])
        _put(run, "limits", run.do(s.SolvePose, tg, q=q0, **kw))
        _pose_gets(run, s, "limits", nc, nv, limits=True, step=True)
        run.do(s.clear_step_control)
        # ---- 4. collision avoidance latched (the joint limits stay)
        run.do(s.set_collision_spheres, c["clinks"], c["spheres"])
        run.do(s.set_collision_world, c["ws"], c["wb"])
        run.do(s.set_self_collision, True)
        run.do(s.set_collision_avoidance, **TA.PRM)
        tg, q0 = run.inp(c["tg"].reshape(B, nc, 12)), run.inp(c["q0_in"])
        _put(run, "avoid", run.do(s.SolvePose, tg, q=q0, **kw))
        _pose_gets(run, s, "avoid", nc, nv, limits=True, avoid=True)
        run.do(s.clear_collision_avoidance)
        # ---- 5. the multi-start: the seeds alone, then the three picks
        run.do(s.set_seed_ranges, c["q_lo"], c["q_hi"])   # (the DoFs with a limit are the ones sampled)
        run.do(s.sample_seeds, K, seed=11, round=1, q0=run.inp(c["q0g"]))
        run.get("sampled:q", lambda out: s.get("q", out=out))
        for pick, extra in (("nearest", {}), ("first", dict(clearance_margin=0.0)), ("dexterous", dict(length=0.5))):
            goals, q0g = run.inp(c["goals"].reshape(G, nc, 12)), run.inp(c["q0g"])
            out = run.do(s.SolvePoseMultiStart, goals, K, rounds=2, seed=11, pick=pick, q0=q0g, **kw, **extra)
            _put(run, "ms " + pick, out)
            for fid, name, shape, dt in ((capi.MS_F_WINNER, "winner", (B,), I), (capi.MS_F_GOAL_STATUS, "goal_status", (B,), I), (capi.MS_F_Q, "q", (B, nq), F),
                                         (capi.MS_F_ERR, "err", (B, nc, 6), F), (capi.MS_F_COST, "cost", (B,), F), (capi.MS_F_NREACHED, "nreached", (B,), I),
                                         (capi.MS_F_ROUND, "round", (B,), I)):
                run.get_n(["ms %s goals:%s" % (pick, name)], _raw(s, L.loikb_multistart_get, fid), [(shape, dt)])
            if "clearance_margin" in extra:   # (the collision-aware selection's own getter: its results outlive the latch the binding puts back)
                for fid, name, shape, dt in ((capi.CLR_MS_F_CLEARANCE, "clearance", (B,), F), (capi.CLR_MS_F_WITNESS, "witness", (B, 3), I),
                                             (capi.CLR_MS_F_NCLEAR, "nclear", (B,), I), (capi.CLR_MS_F_INSTANCE, "instance", (B,), F)):
                    run.get_n(["ms %s clearance pick:%s" % (pick, name)], _raw(s, L.loikb_clearance_get_multistart_result, fid), [(shape, dt)])
            _pose_gets(run, s, "ms " + pick, nc, nv, limits=True)
        # ---- 6. a path of waypoints, a timed trajectory
        run.do(s.set_joint_limits, None, None)
        wp, q0 = run.inp(c["wp"].reshape(B, T_PATH, nc, 12)), run.inp(c["q0p"])
        _put(run, "path", run.do(s.SolvePosePath, wp, q=q0, max_steps_per_waypoint=3, **kw))
        for fid, name, shape, dt in ((capi.PATH_F_CURSOR, "cursor", (B,), I), (capi.PATH_F_STATUS, "path_status", (B,), I),
                                     (capi.PATH_F_WSTEPS, "wsteps", (B, T_PATH), I), (capi.PATH_F_Q, "q_path", (B, T_PATH, nq), F)):
            run.get_n(["path get:" + name], _raw(s, L.loikb_path_get, fid), [(shape, dt)])
        _pose_gets(run, s, "path", nc, nv)
        smp, q0 = run.inp(c["smp"].reshape(B, T_TRACK + 1, nc, 12)), run.inp(c["q0t"])
        _put(run, "track", run.do(s.TrackPose, smp, dt=0.5, gain=0.7, tol_track=1e-4, q=q0))
        for name in capi.TRACK_FIELD_ID:
            run.get("track get:" + name, lambda out, name=name: s.track_get(name, out=out))
        _pose_gets(run, s, "track", nc, nv)
    return sequence


@pytest.mark.parametrize("name", ["panda7", "multidof13"])
def test_pose_loops_behind_a_gate(name):
    c = _case(name)
    make = lambda: _handle(c["model"], B, c["links"], c["q0"], c["A"], PRM, box=_box(c["model"]))
    ref, gates = H.run_both(make, _sequence(c), what=name)
    assert gates >= 60
    # the loops did something: instances reached and others did not, limits bound, waypoints were passed, samples were tracked
    assert ref["plain:reached"].any() and (ref["plain:steps"] > 1).any()
    assert (ref["limits:limit_flags"] != 0).any()
    assert (ref["path:cursor"] > 0).any() and not np.isnan(ref["track:q_traj"][:, 0]).any()
    assert (ref["sampled:q"] != c["q0"]).any()
    G = B // K
    assert (ref["ms first clearance pick:nclear"][:G] >= 0).all() and not np.isnan(ref["ms first clearance pick:instance"]).all()
