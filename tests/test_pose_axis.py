"""GPU: axis-symmetric tool tasks in the pose loops (include/loik_amd_axis.h: LOIKB_TASK_POSE_AXIS, LOIKB_TASK_AXIS -- the rotation
about the task frame's z axis is free) against the lock-step CPU oracle with those kinds (tests/pose_axis_numpy.py, proven on the CPU
by tests/test_pose_axis_oracle.py), from first principles, the antiparallel rule, through every inner engine, on an f32 handle, with
joint position and acceleration limits, through SolvePosePath, TrackPose and SolvePoseMultiStart, and the argument rules.
The parity gate is tests/test_pose_tasks.py's (_measure): on at most 256 instances the same reached / steps on >= 99 %, |dq| < 1e-7 on
those.  Every case prints what it measured ("pose_axis_measured ...") before it asserts; profiles/axis_tasks_measured.md keeps the
figures of one run."""
import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from test_engines import ENGINES
from test_pose_ik import BOUND, PRM, _links
from test_pose_parity import ENGINE_ENV, F32_STEP_REL, _box, _handle, _subset
from test_pose_tasks import DQ_BOUND, ENGINE_RUNS, LAW0, LAW1, TOL, _eye_A, _parity_workload, _robot, _task_handle
from test_pose_tasks_oracle import task_seeds
from test_pose_track import _track_workload
import pose_numpy as P
import pose_limits_numpy as PL
import pose_tasks_numpy as T
import pose_axis_numpy as AX
import pose_accel_numpy as PA

pytestmark = pytest.mark.gpu

KINDS = AX.KINDS
AXIS = ("pose_axis", "axis")


def _spin(tg, kinds, seed, flip=False):
    """the targets of the constraints with a free-spin kind, spun about their own z by U(-pi, pi); tg [..][nc][12]"""
    out, ang = AX.spin_targets(np.random.default_rng(seed), tg, flip=flip)
    for c, kind in enumerate(kinds):
        if kind not in AXIS:
            out[..., c, :] = np.asarray(tg)[..., c, :]
    return out, ang


def _oracle(model, prm, q0, links, kinds, frames, tg, dt, gain, tol, k, idx, **kw):
    lb, ub = _box(model)
    tg_i = tg[idx] if tg.ndim == 3 else np.broadcast_to(tg, (len(idx),) + tg.shape)
    return AX.lockstep_pose_loop_axis(model, prm, q0[idx], np.eye(6), np.zeros(6), links, [KINDS[x] for x in kinds], frames, lb, ub,
                                      tg_i, dt, gain, tol, k, **kw)


def _measure(out, q, o, idx, what):
    """test_pose_tasks._measure: the parity gate with its figures printed first"""
    same = (out["reached"][idx] == o["reached"]) & (out["steps"][idx] == o["steps"])
    dq = np.abs(q[idx] - o["q"]).max(axis=1)
    print("pose_axis_measured %s | same %.6f | dq_max %.3e | oracle reached %.3f steps %s"
          % (what, same.mean(), dq[same].max() if same.any() else np.nan, o["reached"].mean(), np.bincount(o["steps"]).tolist()))
    assert same.mean() >= 0.99, (what, same.mean())
    assert np.all(dq[same] < DQ_BOUND), (what, dq[same].max())
    return same


def _masked_are_zero(err, kinds):
    for c, kind in enumerate(kinds):
        assert not err[:, c, ~AX.mask(KINDS[kind]).astype(bool)].any(), (c, kind)


# ---- 1. parity with the lock-step oracle ---------------------------------------------------------------------------------------------
PARITY = [
    # (robot, kinds, B, (gain, dt), shared target): test_pose_tasks.PARITY's layout, so _parity_workload builds them
    ("talos32", ("pose_axis",), 193, LAW0, False),
    ("talos32", ("axis",), 193, LAW0, False),
    ("talos32", ("pose_axis",), 193, LAW1, False),
    ("talos32", ("axis",), 193, LAW1, False),
    ("talos32", ("pose_axis",), 193, LAW0, True),
    ("talos32", ("axis",), 193, LAW0, True),
    ("talos32", ("pose_axis",), 193, LAW1, True),
    ("talos32", ("axis",), 193, LAW1, True),
    ("talos32", ("axis", "pose"), 193, LAW0, False),
    ("talos32", ("position", "pose_axis"), 193, LAW1, False),
    ("talos32", ("pose_axis",), 1, LAW0, False),
    ("panda7", ("pose_axis",), 64, LAW1, False),
    ("panda7", ("axis",), 64, LAW0, True),
    ("multidof", ("pose_axis", "axis"), 193, LAW0, False),
]


def _parity_id(c):
    return "%s-%s-B%d-g%g-dt%g-%s" % (c[0], "+".join(c[1]), c[2], c[3][0], c[3][1], "tgsh" if c[4] else "tginst")


@pytest.mark.parametrize("case", PARITY, ids=_parity_id)
def test_axis_tasks_match_lockstep_oracle(case):
    name, kinds, B, (gain, dt), shared_tg = case
    model, links, frames, q0, tg = _parity_workload(case)
    tg, _ = _spin(tg, kinds, 7000 + B)
    idx = _subset(B)
    for k in (1, 3):
        s = _task_handle(model, B, links, q0, kinds, frames)
        out = s.SolvePose(tg, dt=dt, gain=gain, tol_pose=TOL, max_steps=k)
        q = s.get("q")
        s.close()
        o = _oracle(model, PRM, q0, links, kinds, frames, tg, dt, gain, TOL, k, idx)
        same = _measure(out, q, o, idx, "%s k%d" % (_parity_id(case), k))
        assert np.all(out["steps"] <= k)
        assert np.max(np.abs(out["err"][idx][same] - o["err"][same])) < 1e-6
        _masked_are_zero(out["err"], kinds)
        if k == 3 and B > 1:
            assert np.any(out["steps"] > 0) and np.max(np.abs(q - q0)) > 1e-4


# ---- 2. first principles, no oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,flip", [("pose_axis", False), ("axis", False), ("axis", True)])
def test_reached_means_reached_and_the_spin_is_left_free(kind, flip):
    """tolerance 1e-6, 20 steps, the targets spun about their z by U(-pi, pi) (flip: turned upside down first, so the start is up to
    3.13 rad off): >= 95 % reach (the oracle reaches all of 256 such seeds: tests/test_pose_axis_oracle.py), every reached q
    satisfies max |S e| <= tol recomputed in numpy, and of the reached seeds whose target was spun by more than 0.05 rad more than
    half keep a full-orientation error above tol: nobody chased the spin"""
    model, links = _robot("talos32", 1)
    B, tol = 1024, 1e-6
    frames = T.random_frames(np.random.default_rng(2300), 1)
    q0, tg, _ = task_seeds(model, B, links, frames, seed=2301, spread=(3e-2, 0.6))
    tg, ang = _spin(tg, [kind], 2302, flip=flip)
    s = _task_handle(model, B, links, q0, [kind], frames)
    out = s.SolvePose(tg, dt=1.0, gain=1.0, tol_pose=tol, max_steps=20)
    q = s.get("q")
    s.close()
    r = out["reached"]
    print("pose_axis_measured first principles %s%s: reached %.4f, steps max %d" % (kind, " flipped" if flip else "", r.mean(), out["steps"].max()))
    assert r.mean() >= 0.95, r.mean()
    e = AX.task_errors(model, q, links, [KINDS[kind]], frames, tg)
    assert np.max(np.abs(e[r])) <= tol, np.max(np.abs(e[r]))
    assert np.max(np.abs(e - out["err"])) < 1e-10
    _masked_are_zero(out["err"], [kind])
    full = T.task_errors(model, q, links, [T.TASK_ORIENTATION], frames, tg)
    off = (np.abs(ang[:, 0]) > 0.05) & r
    assert off.sum() >= 50, off.sum()
    still = np.abs(full[off, 0, 3:]).max(axis=1) > tol
    print("pose_axis_measured first principles %s%s: %d reached seeds were spun by more than 0.05 rad, %.3f of them keep a full-orientation "
          "error above tol" % (kind, " flipped" if flip else "", off.sum(), still.mean()))
    assert still.mean() > 0.5, still.mean()


# ---- 3. the antiparallel rule ----------------------------------------------------------------------------------------------------------
def test_exactly_antiparallel_is_pi_about_x_and_the_loop_leaves_it():
    """one revolute joint about x at the origin, q = 0, identity frame, the target turned by pi about x: d = -z exactly"""
    eye12 = np.r_[np.eye(3).ravel(), np.zeros(3)]
    model = loik_amd.Model([0, 0], [0, 1], [[0, 0, 0], [1.0, 0, 0]], np.stack([eye12, eye12]), name="one_joint_x")
    tg = np.r_[np.diag([1.0, -1.0, -1.0]).ravel(), np.zeros(3)][None, None]
    for kind in AXIS:
        s = _task_handle(model, 1, [1], np.zeros((1, 1)), [kind], None)
        out = s.SolvePose(tg, max_steps=0)
        assert np.array_equal(out["err"][0, 0], np.array([0, 0, 0, np.pi, 0, 0])), out["err"]
        assert not out["reached"].any() and not out["steps"].any()
        out = s.SolvePose(tg, dt=1.0, gain=1.0, tol_pose=1e-6, max_steps=1)
        q = s.get("q")
        s.close()
        w = np.linalg.norm(out["err"][0, 0, 3:])
        print("pose_axis_measured antiparallel %s: after one step q = %.6f, |w| = %.6f" % (kind, q[0, 0], w))
        assert out["steps"][0] == 1 and w < np.pi and np.isfinite(w)
        assert not out["err"][0, 0, [0, 1, 2, 5]].any()


# ---- 4. every inner engine -----------------------------------------------------------------------------------------------------
_ENGINE_CACHE = {}


def _engine_problem():
    if not _ENGINE_CACHE:
        model, links = _robot("talos32", 2)
        B = 384   # (six tiles of 64: LOIKB_CHUNKS=3 gets three chunks of two)
        frames = T.random_frames(np.random.default_rng(2400), 2)
        q0, tg, _ = task_seeds(model, B, links, frames, seed=2401)
        tg, _ = _spin(tg, AXIS, 2402)
        idx = _subset(B)
        o = _oracle(model, PRM, q0, links, AXIS, frames, tg, 0.5, 0.7, TOL, 3, idx)
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
    s = _task_handle(model, B, links, q0, AXIS, frames, **kw)
    out = s.SolvePose(tg, dt=0.5, gain=0.7, tol_pose=TOL, max_steps=3)
    q = s.get("q")
    if engine == "chunks3":
        assert s.stats()["chunks"] == 3
    s.close()
    _measure(out, q, o, idx, "engine %s" % engine)
    assert np.any(out["steps"] > 1)


# ---- 5. f32 handle ------------------------------------------------------------------------------------------------------------
def test_f32_handle_err_is_fp64_and_one_step_matches_the_oracle():
    """the recipe of test_pose_tasks.test_f32_handle_err_is_fp64_and_one_step_matches_the_oracle with the two axis kinds"""
    model, links = _robot("talos32", 2)
    B = 128
    frames = T.random_frames(np.random.default_rng(2500), 2)
    q0, tg, _ = task_seeds(model, B, links, frames, seed=2501, spread=(1e-3, 0.1))
    tg, _ = _spin(tg, AXIS, 2502)
    prm = dict(PRM, max_iter=40, tol_abs=0.0, tol_rel=0.0, tol_primal_inf=0.0, tol_dual_inf=0.0)
    s = _task_handle(model, B, links, q0, AXIS, frames, prm=prm, precision=capi.F32)
    out0 = s.SolvePose(tg, max_steps=0)
    want = AX.task_errors(model, q0, links, [KINDS[x] for x in AXIS], frames, tg)
    print("pose_axis_measured f32 handle: max |err - numpy| = %.3e" % np.max(np.abs(out0["err"] - want)))
    assert np.max(np.abs(out0["err"] - want)) <= 1e-10 and not out0["steps"].any()
    out = s.SolvePose(tg, dt=0.5, gain=0.7, tol_pose=1e-9, max_steps=1)
    q32 = s.get("q")
    s.close()
    o = _oracle(model, prm, q0, links, AXIS, frames, tg, 0.5, 0.7, 1e-9, 1, np.arange(B))
    assert np.array_equal(out["steps"], o["steps"]) and o["steps"].all()
    rel = np.abs(q32 - o["q"]).max(axis=1) / np.abs(o["q"] - q0).max(axis=1)
    print("pose_axis_measured f32 step vs oracle: max relative difference %.3e, median %.3e" % (rel.max(), np.median(rel)))
    assert rel.max() < F32_STEP_REL, rel.max()


# ---- 6. with joint position limits, and with acceleration limits -------------------------------------------------------------------
def test_axis_tasks_with_joint_limits_match_the_combined_oracle():
    model, links = _robot("talos32", 2)
    B = 193
    frames = T.random_frames(np.random.default_rng(2600), 2)
    q0, tg, q_t = task_seeds(model, B, links, frames, seed=2601, spread=(1e-7, 0.15))
    tg, _ = _spin(tg, AXIS, 2603)
    q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, 2602, (2.0, 98.0))
    qi = PL.limit_q_index(model)
    lim = np.isfinite(q_lo) | np.isfinite(q_hi)
    idx = _subset(B)
    for k in (1, 4):
        s = _task_handle(model, B, links, q0, AXIS, frames)
        s.set_joint_limits(q_lo, q_hi)
        out = s.SolvePose(tg, dt=0.25, gain=0.5, tol_pose=TOL, max_steps=k)
        q = s.get("q")
        assert [t[0] for t in s.pose_tasks()] == list(AXIS)
        s.close()
        assert "limit_flags" in out and out["limit_flags"].shape == (B, model.nv)
        assert np.all(q_lo[lim] <= q[:, qi[lim]]) and np.all(q[:, qi[lim]] <= q_hi[lim])
        o = _oracle(model, PRM, q0, links, AXIS, frames, tg, 0.25, 0.5, TOL, k, idx, q_lo=q_lo, q_hi=q_hi)
        same = _measure(out, q, o, idx, "limits k%d" % k)
        assert (out["limit_flags"][idx][same] != o["limit_flags"][same]).any(axis=1).mean() <= 0.01
        _masked_are_zero(out["err"], AXIS)
        if k == 4:
            assert (o["limit_flags"] != 0).any(axis=1).mean() > 0.1, "the limits never bound"


def test_axis_tasks_with_acceleration_limits_match_the_combined_oracle():
    """joint-frame tasks (identity iMf, where pose_accel_numpy's law A (k e) is the task law to the bit: pose_axis_numpy says why),
    position limits and acceleration limits on half of the DoFs as tests/test_pose_accel.py draws them"""
    model, links = _robot("talos32", 2)
    B, dt, gain = 193, 0.25, 0.5
    q0, tg, q_t = task_seeds(model, B, links, np.tile(T.IDENTITY12, (2, 1)), seed=2651, spread=(1e-3, 0.15))
    tg, _ = _spin(tg, AXIS, 2653)
    q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, 2652, (2.0, 98.0))
    a_max = PA.accel_limits(model, 2654, dt, BOUND, 1e-4, 1e-3)
    lb, ub = _box(model)
    idx = _subset(B)
    for k in (1, 4):
        s = _task_handle(model, B, links, q0, AXIS, None)
        s.set_joint_limits(q_lo, q_hi)
        s.set_joint_accel_limits(a_max)
        out = s.SolvePose(tg, dt=dt, gain=gain, tol_pose=TOL, max_steps=k)
        q = s.get("q")
        s.close()
        o = AX.lockstep_pose_loop_axis_accel(model, PRM, q0[idx], np.eye(6), np.zeros(6), links, [KINDS[x] for x in AXIS], lb, ub, tg[idx],
                                             dt, gain, TOL, k, q_lo, q_hi, a_max)
        same = _measure(out, q, o, idx, "accel limits k%d (oracle edge-active %.3f)" % (k, o["edge"].mean()))
        assert (out["limit_flags"][idx][same] != o["limit_flags"][same]).any(axis=1).mean() <= 0.01
        _masked_are_zero(out["err"], AXIS)
        if k == 4:
            assert (o["limit_flags"] & 12).any() and (out["limit_flags"] & 12).any(), "the acceleration limits never bound"


# ---- 7. path: one waypoint and no budget is SolvePose ---------------------------------------------------------------------------------
def _pair_workload(B, seed):
    model, links = _robot("talos32", 2)
    frames = T.random_frames(np.random.default_rng(seed), 2)
    q0, tg, _ = task_seeds(model, B, links, frames, seed=seed + 1)
    tg, _ = _spin(tg, AXIS, seed + 2)
    return model, links, frames, q0, tg


def test_one_waypoint_path_is_solve_pose_bit_for_bit():
    B = 193
    model, links, frames, q0, tg = _pair_workload(B, 2900)
    res = []
    for path in (False, True):
        s = _task_handle(model, B, links, q0, AXIS, frames)
        kw = dict(dt=0.5, gain=0.8, tol_pose=TOL, max_steps=4)
        out = s.SolvePosePath(tg[:, None], **kw) if path else s.SolvePose(tg, **kw)
        res.append((out, s.get("q"), s.get("z")))
        s.close()
    (a, qa, za), (b, qb, zb) = res
    for key in ("steps", "status", "err"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(qa, qb) and np.array_equal(za, zb)
    assert a["steps"].any() and len(set(a["steps"].tolist())) > 1
    _masked_are_zero(b["err"], AXIS)


# ---- 8. track ----------------------------------------------------------------------------------------------------------------------------
def test_track_without_feedforward_on_constant_samples_is_solve_pose_bit_for_bit():
    B, Tn = 193, 4
    model, links, frames, q0, tg = _pair_workload(B, 2950)
    smp = np.repeat(tg[:, None], Tn + 1, axis=1)
    res = []
    for track in (False, True):
        s = _task_handle(model, B, links, q0, AXIS, frames)
        if track:
            out = s.TrackPose(smp, dt=0.5, gain=0.8, tol_track=0.0, feedforward="none")
        else:
            out = s.SolvePose(tg, dt=0.5, gain=0.8, tol_pose=0.0, max_steps=Tn)
        res.append((out, s.get("q"), s.get("z")))
        s.close()
    (a, qa, za), (b, qb, zb) = res
    for key in ("steps", "status", "err"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(qa, qb) and np.array_equal(za, zb)
    assert np.all(a["steps"] == Tn) and not a["reached"].any()


def test_one_feedforward_step_is_the_step_to_the_next_sample():
    """gain = 1: dt f + e against X_0 is the error against X_1, whatever X_0 is -- so one tracking step over (X_0, X_1) is
    SolvePose(X_1, max_steps=1) from the same q0, up to the rounding of the difference (|dq| < 1e-7, the parity gate's bound)"""
    B = 193
    model, links, frames, q0, x1 = _pair_workload(B, 3000)
    _, x0, _ = task_seeds(model, B, links, frames, seed=3005)   # other placements altogether
    x0, _ = _spin(x0, AXIS, 3006)
    smp = np.stack([x0, x1], axis=1)
    s = _task_handle(model, B, links, q0, AXIS, frames)
    a = s.TrackPose(smp, dt=0.5, gain=1.0, tol_track=0.0, feedforward="difference")
    qa = s.get("q")
    s.close()
    s = _task_handle(model, B, links, q0, AXIS, frames)
    b = s.SolvePose(x1, dt=0.5, gain=1.0, tol_pose=0.0, max_steps=1)
    qb = s.get("q")
    s.close()
    dq = np.abs(qa - qb).max()
    print("pose_axis_measured track one feed-forward step vs SolvePose to X_1: max |dq| = %.3e, step size %.3e" % (dq, np.abs(qb - q0).max()))
    assert np.all(a["steps"] == 1) and np.all(b["steps"] == 1) and np.abs(qb - q0).max() > 1e-3
    assert dq < DQ_BOUND, dq
    assert np.max(np.abs(a["err"] - b["err"])) < 1e-6


@pytest.mark.parametrize("kind", AXIS)
def test_feedforward_tracks_a_spinning_target_better(kind):
    """16 samples along smooth joint paths (a sample translates and tilts the frame by about 1e-2), the targets spinning about their
    own z by 0.5 rad per sample on top: the spin is nothing to these kinds, the feed-forward takes the lag out of the rest"""
    model, links = _robot("talos32", 1)
    B, Tn, dt, tol = 193, 15, 0.5, 1e-4
    frames = T.random_frames(np.random.default_rng(3100), 1)
    q0, smp, _ = _track_workload(model, links, B, Tn, seed=3101, frames=frames, on_path=True)
    for k in range(Tn + 1):
        smp[:, k, 0, :9] = (smp[:, k, 0, :9].reshape(B, 3, 3) @ AX.rot_z(0.5 * k)).reshape(B, 9)
    res = {}
    for ff in ("none", "difference"):
        s = _task_handle(model, B, links, q0, [kind], frames)
        res[ff] = s.TrackPose(smp, dt=dt, gain=1.0, tol_track=tol, feedforward=ff)
        s.close()
        assert np.all(res[ff]["errmax"][:, 0] < 1e-12) and not np.isnan(res[ff]["worst"]).any()
        assert not res[ff]["err"][..., 5].any()
    better = res["difference"]["worst"] < res["none"]["worst"]
    print("pose_axis_measured track %s: WORST median none %.3e, difference %.3e; better on %.4f"
          % (kind, np.median(res["none"]["worst"]), np.median(res["difference"]["worst"]), better.mean()))
    assert better.mean() >= 0.95, better.mean()


# ---- 9. multi-start -----------------------------------------------------------------------------------------------------------------------
def test_multistart_answers_axis_goals():
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 1)
    lo, hi = np.array(model.q_lo, dtype=float), np.array(model.q_hi, dtype=float)
    G, K, tol = 8, 16, 1e-6
    rng = np.random.default_rng(3200)
    frames = T.random_frames(rng, 1)
    q0g = rng.uniform(lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo), size=(G, model.nq))
    tg = T.frame_fk12(model, rng.uniform(lo, hi, size=(G, model.nq)), links, frames)
    tg, _ = _spin(tg, ["axis"], 3201)
    s = _handle(model, G * K, links, np.repeat(q0g, K, axis=0), _eye_A(1), PRM)
    s.set_joint_limits(lo, hi)
    s.set_pose_tasks(["axis"], frames)
    out = s.SolvePoseMultiStart(tg, K, seed=7, q0=q0g, tol_pose=tol, max_steps=20)
    s.close()
    e = AX.task_errors(model, out["q"], links, [AX.TASK_AXIS], frames, tg)
    got = out["nreached"] > 0
    print("pose_axis_measured multistart axis: %d of %d goals have a reached seed (nreached %s), max |S e| of their best q %.3e"
          % (got.sum(), G, out["nreached"].tolist(), np.abs(e[got]).max() if got.any() else np.nan))
    assert got.sum() >= G // 2, out["nreached"]
    assert np.abs(e[got]).max() <= tol
    assert np.max(np.abs(e - out["err"])) < 1e-10 and not out["err"][..., [0, 1, 2, 5]].any()


# ---- 10. arguments -----------------------------------------------------------------------------------------------------------------------
def test_kinds_accepted_and_refused():
    model, links = _robot("panda7", 2)
    B = 32
    frames = T.random_frames(np.random.default_rng(3300), 2)
    q0, tg, _ = task_seeds(model, B, links, frames, seed=3301)
    kw = dict(dt=0.5, gain=0.9, tol_pose=TOL, max_steps=3)
    ref = _task_handle(model, B, links, q0, ["axis", "pose_axis"], frames)
    want = ref.SolvePose(tg, **kw)
    want_q = ref.get("q")
    ref.close()
    s = _task_handle(model, B, links, q0, [capi.TASK_AXIS, capi.TASK_POSE_AXIS], frames)   # by number
    assert [t[0] for t in s.pose_tasks()] == ["axis", "pose_axis"]
    for bad in (3, 5, 7, 8, -1):
        with pytest.raises(loik_amd.LoikError) as e:
            s.set_pose_tasks([0, bad], frames)
        assert e.value.code == -20, bad
        assert b"unknown kind" in loik_amd.capi.lib().loikb_last_error()
    with pytest.raises(ValueError):
        s.set_pose_tasks(["axis", "free_z"], frames)
    got = s.pose_tasks()
    assert [t[0] for t in got] == ["axis", "pose_axis"] and np.array_equal(np.stack([t[1] for t in got])[:, :3, 3], frames[:, 9:])
    out = s.SolvePose(tg, **kw)
    assert np.array_equal(out["steps"], want["steps"]) and np.array_equal(out["status"], want["status"]) and out["steps"].any()
    assert np.array_equal(s.get("q"), want_q) and np.array_equal(out["err"], want["err"])
    s.set_pose_tasks(["pose_axis", "axis"], frames)   # by name, and the names come back
    assert [t[0] for t in s.pose_tasks()] == ["pose_axis", "axis"]
    s.set_pose_tasks(["position", capi.TASK_KINDS["orientation"]], frames)
    assert [t[0] for t in s.pose_tasks()] == ["position", "orientation"]
    s.close()
