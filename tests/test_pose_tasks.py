"""GPU: tool frames and position-only / orientation-only tasks in the pose loop (include/loik_amd_tasks.h) against the lock-step
CPU oracle with tasks (tests/pose_tasks_numpy.py, proven on the CPU by tests/test_pose_tasks_oracle.py), from first principles,
through every inner engine, on an f32 handle, with joint position limits, and the specification's lifetime and argument rules.
The parity gate is tests/test_pose_parity.py's: on the oracle's strided subset of at most 256 instances, the same reached / steps on
>= 99 % of them, |dq| < 1e-7 on those.  Every parity case prints what it measured ("pose_tasks_measured ...") before it asserts."""
import ctypes as C

import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from test_engines import ENGINES
from test_pose_ik import PRM, _fk_models, _links
from test_pose_parity import ENGINE_ENV, F32_STEP_REL, _box, _gate, _handle, _leaf_and_multidof, _nonsym_A, _seeds, _subset
from test_pose_tasks_oracle import KINDS, task_seeds
import pose_numpy as P
import pose_limits_numpy as PL
import pose_tasks_numpy as T

pytestmark = pytest.mark.gpu

TOL = 1e-4
DQ_BOUND = 1e-7   # the parity gate's, for every kind, the masked ones (a rank-3 A) included


def _robot(name, nc):
    if name == "multidof":
        model = _fk_models()[3]   # free-flyer root, a translation joint, two ZYX, a planar and three (cos, sin) joints
        return model, _leaf_and_multidof(model)[:nc]
    model = loik_amd.builtin_model(name)
    return model, _links(model, nc)


def _eye_A(nc):
    return np.tile(np.eye(6), (nc, 1, 1))


def _task_handle(model, B, links, q0, kinds, frames, prm=PRM, **kw):
    """SolveInit with a shared A = I and b = 0, then the tasks"""
    s = _handle(model, B, links, q0, _eye_A(len(links)), prm, **kw)
    s.set_pose_tasks(kinds, frames)
    return s


def _task_oracle(model, prm, q0, links, kinds, frames, tg, dt, gain, tol, k, idx, **kw):
    lb, ub = _box(model)
    tg_i = tg[idx] if tg.ndim == 3 else np.broadcast_to(tg, (len(idx),) + tg.shape)
    return T.lockstep_pose_loop_tasks(model, prm, q0[idx], np.eye(6), np.zeros(6), links, [KINDS[x] for x in kinds], frames, lb, ub,
                                      tg_i, dt, gain, tol, k, **kw)


def _measure(out, q, o, idx, what):
    """the parity gate with its figures printed first"""
    same = (out["reached"][idx] == o["reached"]) & (out["steps"][idx] == o["steps"])
    dq = np.abs(q[idx] - o["q"]).max(axis=1)
    print("pose_tasks_measured %s | same %.6f | dq_max %.3e | oracle reached %.3f steps %s"
          % (what, same.mean(), dq[same].max() if same.any() else np.nan, o["reached"].mean(), np.bincount(o["steps"]).tolist()))
    assert same.mean() >= 0.99, (what, same.mean())
    assert np.all(dq[same] < DQ_BOUND), (what, dq[same].max())
    return same


# ---- 1. identity: POSE tasks in the joint frame are the loop a handle without tasks runs, bit for bit -----------------------------
@pytest.mark.parametrize("name,B", [("talos32", 193), ("panda7", 64)])
def test_pose_tasks_with_identity_frames_change_nothing(name, B):
    model, links = _robot(name, 2)
    q0, tg = _seeds(model, B, links, seed=2100 + B)
    for k in (1, 3):
        res = []
        for tasks in (False, True):
            s = _handle(model, B, links, q0, _eye_A(2), PRM)
            if tasks:
                s.set_pose_tasks(["pose", "pose"])
                assert [t[0] for t in s.pose_tasks()] == ["pose", "pose"]
                assert all(np.array_equal(t[1], np.eye(4)) for t in s.pose_tasks())
            out = s.SolvePose(tg, dt=0.5, gain=0.8, tol_pose=TOL, max_steps=k)
            out["q"] = s.get("q")
            res.append(out)
            if tasks:
                assert np.array_equal(s.frame_placements(links), s.forward_kinematics(links))
                assert np.array_equal(s.frame_placements(links, np.tile(np.eye(4), (2, 1, 1))), s.forward_kinematics(links))
            s.close()
        for key in ("q", "steps", "status", "err"):
            assert np.array_equal(res[0][key], res[1][key]), (name, k, key)
        assert res[0]["steps"].any()


def test_frame_placements_match_numpy():
    for model in _fk_models()[:4]:
        B = 48
        rng = np.random.default_rng(2150)
        q = model.random_configurations(rng, B)
        links = list(range(model.njoints))
        frames = T.random_frames(rng, len(links))
        s = _handle(model, B, [model.njoints - 1], q, _eye_A(1), PRM)
        got = s.frame_placements(links, frames)
        s.close()
        want = T.frame_fk12(model, q, links, frames)
        assert np.max(np.abs(got[..., :3, :3].reshape(B, -1, 9) - want[..., :9])) < 1e-12, model.name
        assert np.max(np.abs(got[..., :3, 3] - want[..., 9:])) < 1e-12, model.name
        assert np.all(got[..., 3, :] == np.array([0, 0, 0, 1.0]))


# ---- 2. parity with the lock-step oracle ---------------------------------------------------------------------------------------
LAW0, LAW1 = (0.5, 0.25), (1.7, 2.0)   # (gain, dt) as in test_pose_parity.LAW_CASES
PARITY = [
    # (robot, kinds, B, (gain, dt), shared target)
    ("talos32", ("pose",), 193, LAW0, False),
    ("talos32", ("position",), 193, LAW0, False),
    ("talos32", ("orientation",), 193, LAW0, False),
    ("talos32", ("pose",), 193, LAW1, True),
    ("talos32", ("position",), 193, LAW1, True),
    ("talos32", ("orientation",), 193, LAW1, True),
    ("talos32", ("position", "orientation"), 193, LAW1, False),
    ("talos32", ("orientation", "pose"), 4096, LAW0, False),
    ("talos32", ("position", "pose"), 1, LAW0, False),
    ("talos32", ("orientation",), 1, LAW1, True),
    ("panda7", ("pose",), 193, LAW1, False),
    ("panda7", ("position",), 193, LAW1, False),
    ("panda7", ("orientation", "position"), 64, LAW0, True),
    ("multidof", ("pose", "pose"), 193, LAW0, False),
    ("multidof", ("position", "orientation"), 193, LAW0, False),
]


def _parity_id(c):
    return "%s-%s-B%d-g%g-dt%g-%s" % (c[0], "+".join(c[1]), c[2], c[3][0], c[3][1], "tgsh" if c[4] else "tginst")


def _parity_workload(case):
    """frames: a random rotation, |pf| in 0.1 .. 0.2; targets: the frames' FK at random configurations; seeds as test_pose_parity._seeds
    makes them.  The seed depends on the robot, B, the law and the target mode, NOT on the kinds: the POSE case beside a masked case
    runs on the same seeds and frames."""
    name, kinds, B, (gain, dt), shared_tg = case
    nc = len(kinds)
    model, links = _robot(name, nc)
    seed = 2200 + B + int(10 * gain) + 1000 * int(shared_tg) + sum(map(ord, name))
    frames = T.random_frames(np.random.default_rng(seed), 2)[:nc]
    q0, tg, _ = task_seeds(model, B, links, frames, seed=seed + 1, spread=(1e-5, 0.1) if shared_tg else (1e-4, 0.15))
    if shared_tg:   # (the seeds around the first target, as test_control_law_matches_lockstep_oracle has them)
        rng = np.random.default_rng(seed + 2)
        tg = tg[0]
        q0 = np.stack([P.integrate(model, q0[0], 0.02 * rng.normal(size=model.nv) * 10.0 ** rng.uniform(-3, 0)) for _ in range(B)])
    return model, links, frames, q0, tg


@pytest.mark.parametrize("case", PARITY, ids=_parity_id)
def test_tasks_match_lockstep_oracle(case):
    name, kinds, B, (gain, dt), shared_tg = case
    model, links, frames, q0, tg = _parity_workload(case)
    idx = _subset(B)
    for k in (1, 3):
        s = _task_handle(model, B, links, q0, kinds, frames)
        out = s.SolvePose(tg, dt=dt, gain=gain, tol_pose=TOL, max_steps=k)
        q = s.get("q")
        s.close()
        o = _task_oracle(model, PRM, q0, links, kinds, frames, tg, dt, gain, TOL, k, idx)
        same = _measure(out, q, o, idx, "%s k%d" % (_parity_id(case), k))
        assert np.all(out["steps"] <= k)
        assert np.max(np.abs(out["err"][idx][same] - o["err"][same])) < 1e-6
        for c, kind in enumerate(kinds):   # the masked-out entries of err are zeros, not small numbers
            assert not out["err"][:, c, ~T.mask(KINDS[kind]).astype(bool)].any()
        if k == 3 and B > 1:
            assert np.any(out["steps"] > 0) and np.max(np.abs(q - q0)) > 1e-4


# ---- 3. first principles, no oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pose", "position", "orientation"])
def test_reached_means_reached_and_the_masked_part_is_left_free(kind):
    """tolerance 1e-6, 20 steps: every reached instance's final q satisfies max |S e| <= tol, computed in numpy from pose_numpy.fk and
    iMf; >= 95 % reach (the oracle reaches all of them: tests/test_pose_tasks_oracle.py).  A position task leaves the orientation
    free: of the seeds whose frame orientation differs from the target's by more than 0.05 rad, most reached instances keep an
    orientation error above tol; an orientation task leaves the position free (0.05 there is metres)."""
    model, links = _robot("talos32", 1)
    B, tol = 1024, 1e-6
    frames = T.random_frames(np.random.default_rng(2300), 1)
    q0, tg, _ = task_seeds(model, B, links, frames, seed=2301, spread=(3e-2, 0.6))
    s = _task_handle(model, B, links, q0, [kind], frames)
    out = s.SolvePose(tg, dt=1.0, gain=1.0, tol_pose=tol, max_steps=20)
    q = s.get("q")
    s.close()
    r = out["reached"]
    print("first principles %s: reached %.4f, steps max %d" % (kind, r.mean(), out["steps"].max()))
    assert r.mean() >= 0.95, r.mean()
    e = T.task_errors(model, q, links, [KINDS[kind]], frames, tg)
    assert np.max(np.abs(e[r])) <= tol, np.max(np.abs(e[r]))
    assert np.max(np.abs(e - out["err"])) < 1e-10
    if kind == "pose":
        return
    free = slice(3, 6) if kind == "position" else slice(0, 3)
    full0 = T.task_errors(model, q0, links, [T.TASK_POSE], frames, tg)
    full1 = T.task_errors(model, q, links, [T.TASK_POSE], frames, tg)
    if kind == "orientation":   # (the linear part of log6 mixes in the rotation: measure the position error as a position task does)
        full0 = T.task_errors(model, q0, links, [T.TASK_POSITION], frames, tg)
        full1 = T.task_errors(model, q, links, [T.TASK_POSITION], frames, tg)
    off = (np.linalg.norm(full0[:, 0, free], axis=1) > 0.05) & r
    assert off.sum() >= 50, off.sum()
    still = np.abs(full1[off, 0, free]).max(axis=1) > tol
    print("first principles %s: %d reached seeds start more than 0.05 off in the free part, %.3f of them still are above tol" % (kind, off.sum(), still.mean()))
    assert still.mean() > 0.5, still.mean()


# ---- 4. every inner engine -----------------------------------------------------------------------------------------------------
_ENGINE_CACHE = {}
ENGINE_RUNS = list(ENGINES) + ["chunks3"]
ENGINE_KINDS = ("position", "orientation")


def _engine_problem():
    if not _ENGINE_CACHE:
        model, links = _robot("talos32", 2)
        B = 384   # (six tiles of 64: LOIKB_CHUNKS=3 gets three chunks of two)
        frames = T.random_frames(np.random.default_rng(2400), 2)
        q0, tg, _ = task_seeds(model, B, links, frames, seed=2401)
        idx = _subset(B)
        o = _task_oracle(model, PRM, q0, links, ENGINE_KINDS, frames, tg, 0.5, 0.7, TOL, 3, idx)
        _ENGINE_CACHE.update(w=(model, links, B, frames, q0, tg), idx=idx, o=o)
    return _ENGINE_CACHE["w"], _ENGINE_CACHE["idx"], _ENGINE_CACHE["o"]


@pytest.mark.parametrize("engine", ENGINE_RUNS)
def test_every_engine_matches_lockstep_oracle(engine, monkeypatch):
    (model, links, B, frames, q0, tg), idx, o = _engine_problem()
    for v in ENGINE_ENV:
        monkeypatch.delenv(v, raising=False)
    if engine == "chunks3":   # (the keywords of test_gpu_parity.test_concurrent_chunks_change_nothing)
        env, kw = dict(LOIKB_CHUNKS="3"), dict(compact_min_instances=128, max_launch_iters=5, tail_max_instances=900)
    else:
        env, kw = ENGINES[engine]
    for v, x in env.items():
        monkeypatch.setenv(v, x)
    s = _task_handle(model, B, links, q0, ENGINE_KINDS, frames, **kw)
    out = s.SolvePose(tg, dt=0.5, gain=0.7, tol_pose=TOL, max_steps=3)
    q = s.get("q")
    if engine == "chunks3":
        assert s.stats()["chunks"] == 3
    s.close()
    _measure(out, q, o, idx, "engine %s" % engine)
    assert np.any(out["steps"] > 1)


# ---- 5. f32 handle ------------------------------------------------------------------------------------------------------------
def test_f32_handle_err_is_fp64_and_one_step_matches_the_oracle():
    """err is the fp64 task-frame error whatever the handle's precision; one step of the f32 handle against the oracle's, relative to
    the step, within test_pose_parity.F32_STEP_REL (both run 40 ADMM iterations, no stopping test: the f32 solve's rounding alone)"""
    model, links = _robot("talos32", 2)
    B = 128
    kinds = ("position", "orientation")
    frames = T.random_frames(np.random.default_rng(2500), 2)
    q0, tg, _ = task_seeds(model, B, links, frames, seed=2501, spread=(1e-3, 0.1))
    prm = dict(PRM, max_iter=40, tol_abs=0.0, tol_rel=0.0, tol_primal_inf=0.0, tol_dual_inf=0.0)
    s = _task_handle(model, B, links, q0, kinds, frames, prm=prm, precision=capi.F32)
    out0 = s.SolvePose(tg, max_steps=0)
    want = T.task_errors(model, q0, links, [KINDS[x] for x in kinds], frames, tg)
    assert np.max(np.abs(out0["err"] - want)) <= 1e-10 and not out0["steps"].any()
    out = s.SolvePose(tg, dt=0.5, gain=0.7, tol_pose=1e-9, max_steps=1)
    q32 = s.get("q")
    s.close()
    o = _task_oracle(model, prm, q0, links, kinds, frames, tg, 0.5, 0.7, 1e-9, 1, np.arange(B))
    assert np.array_equal(out["steps"], o["steps"]) and o["steps"].all()
    rel = np.abs(q32 - o["q"]).max(axis=1) / np.abs(o["q"] - q0).max(axis=1)
    print("f32 task step vs oracle: max relative difference %.3e, median %.3e" % (rel.max(), np.median(rel)))
    assert rel.max() < F32_STEP_REL, rel.max()


# ---- 6. with joint position limits ----------------------------------------------------------------------------------------------
def test_tasks_with_joint_limits_match_the_combined_oracle():
    model, links = _robot("talos32", 2)
    B = 193
    kinds = ("position", "orientation")
    frames = T.random_frames(np.random.default_rng(2600), 2)
    q0, tg, q_t = task_seeds(model, B, links, frames, seed=2601, spread=(1e-7, 0.15))
    q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, 2602, (2.0, 98.0))
    qi = PL.limit_q_index(model)
    lim = np.isfinite(q_lo) | np.isfinite(q_hi)
    idx = _subset(B)
    for k in (1, 4):
        s = _task_handle(model, B, links, q0, kinds, frames)
        s.set_joint_limits(q_lo, q_hi)
        out = s.SolvePose(tg, dt=0.25, gain=0.5, tol_pose=TOL, max_steps=k)
        q = s.get("q")
        assert [t[0] for t in s.pose_tasks()] == list(kinds)
        s.close()
        assert "limit_flags" in out and out["limit_flags"].shape == (B, model.nv)
        assert np.all(q_lo[lim] <= q[:, qi[lim]]) and np.all(q[:, qi[lim]] <= q_hi[lim])
        o = _task_oracle(model, PRM, q0, links, kinds, frames, tg, 0.25, 0.5, TOL, k, idx, q_lo=q_lo, q_hi=q_hi)
        same = _measure(out, q, o, idx, "limits k%d" % k)
        assert (out["limit_flags"][idx][same] != o["limit_flags"][same]).any(axis=1).mean() <= 0.01
        if k == 4:
            assert (o["limit_flags"] != 0).any(axis=1).mean() > 0.1, "the limits never bound"


# ---- 7. lifetime of the specification ------------------------------------------------------------------------------------------
def _pose(s, tg):
    out = s.SolvePose(tg, dt=0.5, gain=0.9, tol_pose=TOL, max_steps=3)
    out["q"] = s.get("q")
    return out


def _assert_same_run(a, b, what):
    assert np.array_equal(a["steps"], b["steps"]) and np.array_equal(a["status"], b["status"]), what
    assert np.max(np.abs(a["q"] - b["q"])) <= 1e-12 and np.max(np.abs(a["err"] - b["err"])) <= 1e-12, what
    assert a["steps"].any(), what


DROPS = ["solve_init", "solve_full", "add_eq_constraint", "remove_eq_constraint", "update_eq_constraint_A", "solve_tailored_A", "clear"]


@pytest.mark.parametrize("drop", DROPS)
def test_calls_that_rewrite_A_drop_the_tasks(drop):
    """after each dropping call pose_tasks() is empty and SolvePose runs the plain loop on the A the handle then holds: the twin
    handle makes the same calls without ever setting tasks, from the A the tasks wrote (numpy's S X^-1) where that A survives"""
    model = loik_amd.builtin_model("talos32")
    l0, l1 = _links(model, 2)
    B = 96
    rng = np.random.default_rng(2700)
    frames = T.random_frames(rng, 2)
    kinds = ("position", "orientation")
    A_task = T.task_matrices([KINDS[x] for x in kinds], frames)
    A2 = _nonsym_A(rng, 2)
    q0, tg = _seeds(model, B, [l0, l1], seed=2701)
    lb, ub = _box(model)
    zeros = np.zeros((B, 2, 6))
    two = drop in ("solve_init", "solve_full", "remove_eq_constraint")
    links = [l0, l1] if two else [l0]
    n = len(links)
    prm = dict(PRM, num_eq_c=n, eq_c_capacity=2 if drop == "add_eq_constraint" else 0)
    ids = np.array(links, dtype=np.int32)
    pair = []
    for tasks in (True, False):
        s = loik_amd.BatchedLoik(model, B, **prm)
        if tasks:
            s.SolveInit(q0, np.eye(6), np.zeros(6), ids, _eye_A(n), zeros[:, :n], lb, ub)
            s.set_pose_tasks(kinds[:n], frames[:n])
            assert len(s.pose_tasks()) == n
        else:   # (the A the tasks wrote: what the dropping calls below leave in place, they leave in both)
            s.SolveInit(q0, np.eye(6), np.zeros(6), ids, A_task[:n], zeros[:, :n], lb, ub)
        if drop == "solve_init":
            s.SolveInit(q0, np.eye(6), np.zeros(6), ids, A2, zeros, lb, ub)
        elif drop == "solve_full":
            s.Solve(q0, np.eye(6), np.zeros(6), ids, A2, zeros, lb, ub)
        elif drop == "add_eq_constraint":
            s.AddEqConstraint(l1, A2[1], np.zeros(6))
        elif drop == "remove_eq_constraint":
            assert s.RemoveEqConstraint(l1)
        elif drop == "update_eq_constraint_A":
            s.UpdateEqConstraint(l0, A2[0], np.zeros(6))
        elif drop == "solve_tailored_A":
            s.Solve(None, l0, A2[0], np.zeros(6))
        elif tasks:
            s.clear_pose_tasks()
        assert s.pose_tasks() == []
        nc_now = len(s.active_task_constraint_ids())
        pair.append(_pose(s, tg[:, :nc_now]))
        s.close()
    _assert_same_run(pair[0], pair[1], drop)
    # and it is the plain loop: the oracle's on that A
    A_now = {"solve_init": A2, "solve_full": A2, "add_eq_constraint": np.stack([A_task[0], A2[1]]), "remove_eq_constraint": A_task[:1],
             "update_eq_constraint_A": A2[:1], "solve_tailored_A": A2[:1], "clear": A_task[:1]}[drop]
    if drop not in ("solve_full", "solve_tailored_A"):   # (those ran a solve first: the oracle would have to as well)
        idx = _subset(B)
        lk = [l0, l1][:A_now.shape[0]]
        o = P.lockstep_pose_loop(model, PRM, q0[idx], np.eye(6), np.zeros(6), lk, A_now, lb, ub, tg[idx][:, :len(lk)], 0.5, 0.9, TOL, 3)
        _gate(pair[0], pair[0]["q"], o, idx, drop)


def test_calls_that_leave_A_alone_keep_the_tasks():
    model, links = _robot("talos32", 2)
    B = 96
    kinds = ("position", "orientation")
    frames = T.random_frames(np.random.default_rng(2710), 2)
    q0, tg, _ = task_seeds(model, B, links, frames, seed=2711)
    runs = []
    for edits in (False, True):
        s = _task_handle(model, B, links, q0, kinds, frames)
        if edits:
            s.UpdateEqConstraint(links[0], np.ones(6))   # b only (the pose loop writes every b anyway)
            q_hi = np.inf * np.ones(model.nv)
            q_hi[int(np.flatnonzero(PL.limit_q_index(model) >= 0)[0])] = 1e3
            s.set_joint_limits(-np.inf * np.ones(model.nv), q_hi)
            assert len(s.pose_tasks()) == 2
            s.set_joint_limits(None, None)
            s.UpdateReferences(np.tile(np.eye(6), (model.njoints, 1, 1)), np.zeros((model.njoints, 6)))
            s.UpdateIneqConstraints(*_box(model))
            s.set_pose_tasks(kinds, frames)              # setting them twice is setting them once
        got = s.pose_tasks()
        assert [t[0] for t in got] == list(kinds)
        assert np.array_equal(np.stack([t[1] for t in got])[:, :3, :3].reshape(2, 9), frames[:, :9])
        assert np.array_equal(np.stack([t[1] for t in got])[:, :3, 3], frames[:, 9:])
        runs.append(_pose(s, tg))
        s.close()
    # (UpdateReferences puts the handle on its per-link reference table: the same numbers by another route, so the parity gate)
    a, b = runs
    same = (a["reached"] == b["reached"]) & (a["steps"] == b["steps"])
    assert same.mean() >= 0.99 and np.max(np.abs(a["q"] - b["q"])[same]) < 1e-7 and a["steps"].any()
    assert not b["err"][:, 0, 3:].any() and not b["err"][:, 1, :3].any()


# ---- 8. arguments ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_handle_as_it_was():
    model, links = _robot("panda7", 2)
    B = 32
    frames = T.random_frames(np.random.default_rng(2800), 2)
    kinds = ["position", "pose"]
    q0, tg, _ = task_seeds(model, B, links, frames, seed=2801)
    s = loik_amd.BatchedLoik(model, B, **dict(PRM, num_eq_c=2))
    with pytest.raises(loik_amd.LoikError) as e:   # before SolveInit
        s.set_pose_tasks(kinds, frames)
    assert e.value.code == -24
    s.close()
    s = _handle(model, B, links, q0, _nonsym_A(np.random.default_rng(1), 2, B), PRM)   # a per-instance A
    with pytest.raises(loik_amd.LoikError) as e:
        s.set_pose_tasks(kinds, frames)
    assert e.value.code == -24 and s.pose_tasks() == []
    s.close()

    ref = _task_handle(model, B, links, q0, kinds, frames)
    want = _pose(ref, tg)
    ref.close()
    s = _task_handle(model, B, links, q0, kinds, frames)
    skew = frames.copy()
    skew[1, 0] += 1e-6            # not orthonormal
    refl = frames.copy()
    refl[0, :3] *= -1             # orthonormal, determinant -1
    nan_R = frames.copy()
    nan_R[1, 4] = np.nan
    inf_p = frames.copy()
    inf_p[0, 10] = np.inf
    nan_p = frames.copy()
    nan_p[1, 11] = np.nan
    bad = [(["position"], frames[:1]), (["position", "pose", "pose"], np.tile(frames[:1], (3, 1))), ([0, 3], frames), ([-1, 0], frames),
           (kinds, skew), (kinds, refl), (kinds, nan_R), (kinds, inf_p), (kinds, nan_p)]
    for k, f in bad:
        with pytest.raises(loik_amd.LoikError) as e:
            s.set_pose_tasks(k, f)
        assert e.value.code == -20, (k, f)
        assert len(loik_amd.capi.lib().loikb_last_error()) > 0
    fr = np.ascontiguousarray(frames)
    rc = s.L.loikb_pose_set_tasks(s.h, 2, None, fr.ctypes.data_as(C.POINTER(C.c_double)))   # NULL kinds
    assert rc == -20
    with pytest.raises(ValueError):
        s.set_pose_tasks(["grasp", "pose"], frames)
    for lk, f in (([model.njoints], frames[:1]), ([-1], frames[:1]), (links, skew), (links, nan_p)):
        with pytest.raises(loik_amd.LoikError) as e:
            s.frame_placements(lk, f)
        assert e.value.code == -20
    got = s.pose_tasks()
    assert [t[0] for t in got] == kinds and np.array_equal(np.stack([t[1] for t in got])[:, :3, 3], frames[:, 9:])
    _assert_same_run(_pose(s, tg), want, "after the errors")
    s.close()
