"""GPU: backtracking step control and stall detection in the pose loop (include/loik_amd_step.h, k_pose_step_control) against the
lock-step CPU oracle with the same rule (tests/pose_step_numpy.py, proven on the CPU by tests/test_pose_step_oracle.py); the
identities with the plain loop on a second handle, bit for bit; the rescue at a gain the plain loop diverges at; the stall verdict;
every inner engine and an f32 handle; multi-start; and the argument / state rules.
The parity gate is tests/test_pose_parity.py's (_gate): the same reached / steps on >= 99 % of the instances, |dq| < 1e-7 on those.
Every parity case first asserts on the ORACLE alone that it means something (>= 25 % of the instances backtrack) and that a decision
flipped by rounding cannot consume the gate's 1 % (<= 0.5 % of the instances took a decision with a margin below 1e-2)."""
import ctypes as C

import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from test_engines import ENGINES
from test_pose_ik import PRM, _fk_models, _links
from test_pose_parity import ENGINE_ENV, F32_STEP_REL, _box, _gate, _handle, _leaf_and_multidof, _nonsym_A, _seeds, _subset
from test_pose_tasks_oracle import task_seeds
import pose_numpy as P
import pose_limits_numpy as PL
import pose_tasks_numpy as T
import pose_axis_numpy as AX
import pose_step_numpy as PS

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -20, -24
TOL = 1e-4
DEFAULTS = dict(PS.DEFAULTS)
KEYS = ("q", "steps", "status", "err")


def _workload(name):
    """dict(model, links, A, q0, tg, B, dt, gain) and, by the case, limits = (q_lo, q_hi) or tasks = (kind names, frames)"""
    w = dict(limits=None, tasks=None, dt=1.0, gain=3.0)
    if name == "talos32-nc1":
        model = loik_amd.builtin_model("talos32")
        links, B = _links(model, 1), 193
        A = np.eye(6)[None]
        q0, tg = _seeds(model, B, links, seed=3100, spread=(1e-3, 0.3))
    elif name == "talos32-nc2-Ainst":
        model = loik_amd.builtin_model("talos32")
        links, B = _links(model, 2), 256
        A = _nonsym_A(np.random.default_rng(3200), 2, B)
        q0, tg = _seeds(model, B, links, seed=3201, spread=(1e-3, 0.3))
        w["dt"] = 0.25
    elif name == "panda7-limits":
        model = loik_amd.builtin_model("panda7")
        links, B = _links(model, 1), 193
        A = np.eye(6)[None]
        q0, tg = _seeds(model, B, links, seed=3310, spread=(1e-3, 0.3))
        q_t = model.random_configurations(np.random.default_rng(3310), B)   # (what _seeds drew the targets from)
        # the limits are the range of the targets: every target is inside, and the limits bind through the overshoot -- at gain 3 the
        # full step goes twice as far beyond the target as the seed is short of it, so the box and the clamp cut the trials of the
        # instances whose target lies near an end of a range.  Limits that keep targets out of reach (narrower percentiles) leave
        # instances pinned at a limit with Phi(q_m) / Phi0 -> 1, and 2 to 30 % of the batch then decide within 1e-2 of the bound
        q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, seed=3311, pct=(0.0, 100.0))
        w["limits"] = (q_lo, q_hi)
    elif name == "multidof-tasks":
        model = _fk_models()[3]   # free-flyer root, a translation joint, two ZYX, a planar and three (cos, sin) joints
        links, B = _leaf_and_multidof(model), 193
        A = np.tile(np.eye(6), (2, 1, 1))
        frames = T.random_frames(np.random.default_rng(3400), 2)
        q0, tg, _ = task_seeds(model, B, links, frames, seed=3401, spread=(1e-3, 0.3))
        w["tasks"] = (("position", "pose_axis"), frames)
    else:
        raise ValueError(name)
    w.update(model=model, links=links, A=A, q0=q0, tg=tg, B=B)
    return w


def _mk(w, ctl=None, prm=PRM, precision=capi.F64, **kw):
    """a handle on the workload: SolveInit, the limits and tasks of the case, and step control when ctl is a dict"""
    s = _handle(w["model"], w["B"], w["links"], w["q0"], w["A"], prm, precision=precision, **kw)
    if w["limits"] is not None:
        s.set_joint_limits(*w["limits"])
    if w["tasks"] is not None:
        s.set_pose_tasks(list(w["tasks"][0]), w["tasks"][1])
    if ctl is not None:
        s.set_step_control(**ctl)
    return s


def _solve(w, k, ctl=None, gain=None, **kw):
    s = _mk(w, ctl, **kw)
    out = s.SolvePose(w["tg"], dt=w["dt"], gain=w["gain"] if gain is None else gain, tol_pose=TOL, max_steps=k)
    out["q"] = s.get("q")
    out["timing"] = s.pose_timing()
    s.close()
    return out


def _oracle(w, idx, k, ctl=DEFAULTS, prm=PRM, gain=None):
    lb, ub = _box(w["model"])
    A = w["A"]
    kw = dict(ctl)
    if w["limits"] is not None:
        kw.update(q_lo=w["limits"][0], q_hi=w["limits"][1])
    if w["tasks"] is not None:
        kw.update(tasks=([AX.KINDS[x] for x in w["tasks"][0]], w["tasks"][1]))
    return PS.lockstep_pose_loop_step(w["model"], prm, w["q0"][idx], np.eye(6), np.zeros(6), w["links"], A[idx] if A.ndim == 4 else A, lb, ub,
                                      w["tg"][idx], w["dt"], w["gain"] if gain is None else gain, TOL, k, **kw)


def _assert_means_something(o, what):
    """the two conditions on the oracle's result alone"""
    back = (o["backtracks"] > 0).mean()
    close = (o["margin"] < 1e-2).mean()
    print("pose_step_measured %s | oracle backtracked %.3f | margin < 1e-2 on %.4f, smallest %.3e | reached %.3f steps %s | failed %d"
          % (what, back, close, o["margin"].min(), o["reached"].mean(), np.bincount(o["steps"]).tolist(), int(o["failed"].sum())))
    assert back >= 0.25, (what, back)
    assert close <= 0.005, (what, close)


def _assert_parity(out, o, idx, what):
    same = _gate(out, out["q"], o, idx, what)
    dq = np.abs(out["q"][idx] - o["q"]).max(axis=1)
    print("pose_step_measured %s | same %.6f | dq_max %.3e" % (what, same.mean(), dq[same].max() if same.any() else np.nan))
    for key in ("alpha", "backtracks", "failed"):
        assert np.array_equal(out[key][idx][same], o[key][same]), (what, key)
    assert np.array_equal(out["stalled"][idx][same], (o["status"][same] & PS.POSE_STALLED) != 0), what
    assert np.array_equal(out["status"][idx][same] & 25, o["status"][same] & 25), what
    return same


# ---- 1. parity with the lock-step oracle ---------------------------------------------------------------------------------------------
PARITY = ["talos32-nc1", "talos32-nc2-Ainst", "panda7-limits", "multidof-tasks"]


@pytest.mark.parametrize("k", [1, 6])
@pytest.mark.parametrize("name", PARITY)
def test_step_control_matches_lockstep_oracle(name, k):
    w = _workload(name)
    idx = _subset(w["B"])
    o = _oracle(w, idx, k)
    _assert_means_something(o, (name, k))
    out = _solve(w, k, DEFAULTS)
    same = _assert_parity(out, o, idx, (name, k))
    assert np.all(out["steps"] <= k)
    assert np.max(np.abs(out["err"][idx][same] - o["err"][same])) < 1e-6
    if w["limits"] is not None:   # contained exactly, and the limits bind: without them some instances end elsewhere
        qi = PL.limit_q_index(w["model"])
        lim = np.isfinite(w["limits"][0])
        ql = out["q"][:, qi[lim]]
        assert np.all(w["limits"][0][lim] <= ql) and np.all(ql <= w["limits"][1][lim])
        free = _solve(dict(w, limits=None), k, DEFAULTS)
        moved = (np.abs(free["q"] - out["q"]).max(axis=1) > 1e-3).mean()
        print("pose_step_measured %s | the limits change %.3f of the instances" % ((name, k), moved))
        assert moved >= 0.02, moved
        assert o["limit_flags"].any()
        assert (out["limit_flags"][idx][same] != o["limit_flags"][same]).any(axis=1).mean() <= 0.01
    if w["tasks"] is not None:   # the masked-out entries of err are zeros, not small numbers
        for c, kind in enumerate(w["tasks"][0]):
            assert not out["err"][:, c, ~AX.mask(AX.KINDS[kind]).astype(bool)].any()


# ---- 2. identities on the device, against a second handle that runs the plain loop ------------------------------------------------
@pytest.mark.parametrize("name", ["talos32-nc2-Ainst", "panda7-limits", "multidof-tasks"])
def test_no_backtracks_no_patience_is_the_plain_loop_bit_for_bit(name):
    w = _workload(name)
    plain = _solve(w, 4, gain=2.5)
    got = _solve(w, 4, dict(max_backtracks=0, patience=0), gain=2.5)
    for key in KEYS:
        assert np.array_equal(got[key], plain[key]), (name, key)
    assert not got["backtracks"].any() and not got["stalled"].any()
    assert got["failed"].any(), "the case means nothing: no search failed"
    assert plain["steps"].max() == 4 and "alpha" not in plain


@pytest.mark.parametrize("name", ["talos32-nc2-Ainst", "panda7-limits"])
def test_gain_half_with_the_defaults_is_the_plain_loop_bit_for_bit(name):
    w = _workload(name)
    plain = _solve(w, 6, gain=0.5)
    got = _solve(w, 6, DEFAULTS, gain=0.5)
    for key in KEYS:
        assert np.array_equal(got[key], plain[key]), (name, key)
    assert not got["backtracks"].any() and not got["failed"].any()
    moved = got["steps"] > 0
    assert moved.any() and np.all(got["alpha"][moved] == 1.0) and np.all(got["alpha"][~moved] == 0.0)


def test_set_then_clear_is_the_plain_loop_bit_for_bit():
    w = _workload("talos32-nc2-Ainst")
    plain = _solve(w, 3)
    s = _mk(w, DEFAULTS)
    assert s.step_control() == DEFAULTS
    s.clear_step_control()
    assert s.step_control() is None
    out = s.SolvePose(w["tg"], dt=w["dt"], gain=w["gain"], tol_pose=TOL, max_steps=3)
    out["q"] = s.get("q")
    assert "alpha" not in out
    with pytest.raises(capi.LoikError) as e:
        s.step_get("alpha")
    assert e.value.code == ERR_STATE
    s.close()
    for key in KEYS:
        assert np.array_equal(out[key], plain[key]), key


# ---- 3. / 4. the rescue and the stall verdict on the device -----------------------------------------------------------------------
def _rescue_workload(B):
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 1)
    q0, tg = _seeds(model, B, links, seed=7, spread=(1e-3, 0.3))
    return dict(model=model, links=links, A=np.eye(6)[None], q0=q0, tg=tg, B=B, dt=1.0, gain=2.5, limits=None, tasks=None)


def test_rescue_at_gain_2p5():
    w = _rescue_workload(64)
    plain = _solve(w, 30)
    ctl = _solve(w, 30, DEFAULTS)
    print("pose_step_measured rescue | reached plain %.3f controlled %.3f | controlled steps max %d, loop steps %d | backtracks %d failed %d"
          % (plain["reached"].mean(), ctl["reached"].mean(), ctl["steps"].max(), ctl["timing"]["steps"], ctl["backtracks"].sum(), ctl["failed"].sum()))
    assert plain["reached"].mean() <= 0.10
    assert ctl["reached"].mean() >= 0.90
    e = P.pose_errors(w["model"], ctl["q"], w["links"], w["tg"])
    assert np.all(np.abs(e[ctl["reached"]]).max(axis=(1, 2)) <= TOL)
    assert ctl["backtracks"].any() and not ctl["stalled"].any()


def test_stall_after_three_failed_searches():
    w = _rescue_workload(32)
    got = _solve(w, 30, dict(max_backtracks=0, patience=3))
    two = _solve(w, 2)
    run = np.abs(P.pose_errors(w["model"], w["q0"], w["links"], w["tg"])).max(axis=(1, 2)) > TOL
    assert run.sum() >= 16
    assert np.all(got["stalled"][run]) and not got["stalled"][~run].any()
    assert np.all(got["steps"][run] == 2) and np.all(got["failed"][run] == 3) and not got["reached"][run].any()
    assert np.all(got["reached"][~run]) and not got["steps"][~run].any()
    assert np.array_equal(got["q"], two["q"])
    assert got["timing"]["steps"] == 3   # (max_steps = 30: the loop ends when nothing runs)
    # err is that of the final q: the plain two-step solve judged the same q last
    assert np.array_equal(got["err"], two["err"])
    assert np.max(np.abs(got["err"] - P.pose_errors(w["model"], got["q"], w["links"], w["tg"]))) < 1e-10
    # ... and the oracle says the same
    o = _oracle(w, np.arange(32), 30, dict(max_backtracks=0, patience=3))
    assert np.array_equal(got["status"] & 25, o["status"] & 25) and np.array_equal(got["steps"], o["steps"])
    assert np.array_equal(got["failed"], o["failed"]) and np.max(np.abs(got["q"] - o["q"])) < 1e-7


# ---- 5. every inner engine, and an f32 handle ---------------------------------------------------------------------------------------
_ENGINE_CACHE = {}


def _engine_problem():
    if not _ENGINE_CACHE:
        model = loik_amd.builtin_model("talos32")
        links, B = _links(model, 2), 64
        q0, tg = _seeds(model, B, links, seed=3501, spread=(1e-3, 0.3))
        w = dict(model=model, links=links, A=_nonsym_A(np.random.default_rng(3500), 2), q0=q0, tg=tg, B=B, dt=0.5, gain=3.0, limits=None, tasks=None)
        o = _oracle(w, np.arange(B), 3)
        _assert_means_something(o, "engines")
        _ENGINE_CACHE.update(w=w, o=o)
    return _ENGINE_CACHE["w"], _ENGINE_CACHE["o"]


@pytest.mark.parametrize("engine", list(ENGINES))
def test_every_engine_matches_lockstep_oracle(engine, monkeypatch):
    w, o = _engine_problem()
    for v in ENGINE_ENV:
        monkeypatch.delenv(v, raising=False)
    env, kw = ENGINES[engine]
    for v, x in env.items():
        monkeypatch.setenv(v, x)
    out = _solve(w, 3, DEFAULTS, **kw)
    _assert_parity(out, o, np.arange(w["B"]), engine)
    assert np.any(out["steps"] > 1) and out["backtracks"].any()


def test_f32_handle_step():
    """test_pose_parity.test_f32_handle_per_instance_A_step with step control: one controlled step on an f32 handle against an fp64
    handle given the same float32-rounded A, both inner solves running the same 40 iterations (F32_STEP_REL there says why that is the
    bound); the search is fp64 on both, so they settle on the same trial; and the fp64 handle against the oracle"""
    model = loik_amd.builtin_model("talos32")
    links, B = _links(model, 2), 64
    q0, tg = _seeds(model, B, links, seed=3601, spread=(1e-3, 0.1))
    A = _nonsym_A(np.random.default_rng(3602), 2, B).astype(np.float32).astype(np.float64)
    w = dict(model=model, links=links, A=A, q0=q0, tg=tg, B=B, dt=0.5, gain=3.0, limits=None, tasks=None)
    prm = dict(PRM, max_iter=40, tol_abs=0.0, tol_rel=0.0, tol_primal_inf=0.0, tol_dual_inf=0.0)
    o = _oracle(w, np.arange(B), 1, prm=prm)
    _assert_means_something(o, "f32")
    o32, o64 = (_solve(w, 1, DEFAULTS, prm=prm, precision=p) for p in (capi.F32, capi.F64))
    assert np.array_equal(o32["steps"], o64["steps"]) and o64["steps"].all()
    for key in ("alpha", "backtracks", "failed"):
        assert np.array_equal(o32[key], o64[key]), key
    dq64 = np.abs(o64["q"] - q0).max(axis=1)
    rel = np.abs(o32["q"] - o64["q"]).max(axis=1) / dq64
    print("pose_step_measured f32 vs f64 controlled step: max relative difference %.3e, median %.3e" % (rel.max(), np.median(rel)))
    assert rel.max() < F32_STEP_REL, rel.max()
    _assert_parity(o64, o, np.arange(B), "f64 anchor")


# ---- 6. multi-start -----------------------------------------------------------------------------------------------------------------
def _ms_workload():
    G, K = 16, 4
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 1)
    q0g, tg = _seeds(model, G, links, seed=7, spread=(1e-3, 0.3))   # seed 0 of every goal: the rescue case's seeds
    lo, hi = np.array(model.q_lo, dtype=float), np.array(model.q_hi, dtype=float)
    return model, links, G, K, q0g, tg, lo, hi


def _ms_handle(model, links, B, lo, hi, ctl):
    s = _handle(model, B, links, np.tile(0.5 * (lo + hi), (B, 1)), np.eye(6)[None], PRM)
    s.set_seed_ranges(lo, hi)   # (ranges for the sampler, no joint limits in the loop)
    if ctl is not None:
        s.set_step_control(**ctl)
    return s


def test_multistart_answers_goals_the_plain_call_does_not():
    model, links, G, K, q0g, tg, lo, hi = _ms_workload()
    res = {}
    for name, ctl in (("plain", None), ("ctl", DEFAULTS)):
        s = _ms_handle(model, links, G * K, lo, hi, ctl)
        res[name] = s.SolvePoseMultiStart(tg, K, rounds=2, seed=11, q0=q0g, gain=2.5, tol_pose=TOL, max_steps=30)
        s.close()
    frac = {n: ((r["goal_status"] & capi.MS_GOAL_REACHED) != 0).mean() for n, r in res.items()}
    print("pose_step_measured multistart | goals reached plain %.3f controlled %.3f" % (frac["plain"], frac["ctl"]))
    assert frac["plain"] <= 0.10
    assert frac["ctl"] >= 0.90


def test_multistart_resamples_the_stalled_instances():
    model, links, G, K, q0g, tg, lo, hi = _ms_workload()
    ctl = dict(max_backtracks=0, patience=3)
    # round 0 driven from the host on a second handle: the same seeds, the same loop
    a = _ms_handle(model, links, G * K, lo, hi, ctl)
    a.sample_seeds(K, seed=11, round=0, q0=q0g)
    r0 = a.SolvePose(np.repeat(tg, K, axis=0), gain=2.5, tol_pose=TOL, max_steps=30)
    a.close()
    assert r0["stalled"].mean() >= 0.5 and not (r0["stalled"] & r0["reached"]).any()
    s = _ms_handle(model, links, G * K, lo, hi, ctl)
    out = s.SolvePoseMultiStart(tg, K, rounds=2, seed=11, q0=q0g, gain=2.5, tol_pose=TOL, max_steps=30)
    s.close()
    assert out["rounds_run"] == 2
    assert np.all(out["round"][r0["stalled"]] == 1)
    assert np.all(out["round"][r0["reached"]] == 0)


# ---- 7. errors --------------------------------------------------------------------------------------------------------------------
BAD = [dict(shrink=0.0), dict(shrink=1.0), dict(shrink=-0.5), dict(shrink=1.5), dict(shrink=np.nan), dict(sufficient=-1e-9),
       dict(sufficient=1.0), dict(sufficient=np.nan), dict(max_backtracks=-1), dict(max_backtracks=31), dict(patience=-1), dict(flags=1)]


def _rc(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except capi.LoikError as e:
        return e.code
    return 0


def test_errors_leave_the_handle_as_it_was():
    w = _workload("panda7-limits")
    fresh = _solve(w, 3, gain=1.0)
    s = _mk(w)
    L = s.L
    # every argument error, on a handle without step control and on one with: nothing changes
    for armed in (False, True):
        if armed:
            s.set_step_control(shrink=0.25, sufficient=0.1, max_backtracks=3, patience=2)
        before = s.step_control()
        for bad in BAD:
            f = dict(shrink=0.5, sufficient=1e-4, max_backtracks=6, patience=0, flags=0)
            f.update(bad)
            prm = capi.StepParams(f["shrink"], f["sufficient"], f["max_backtracks"], f["patience"], f["flags"])
            assert L.loikb_pose_set_step_control(s.h, C.byref(prm)) == ERR_ARG, bad
            assert s.step_control() == before, bad
    assert before == dict(shrink=0.25, sufficient=0.1, max_backtracks=3, patience=2)
    # loikb_step_get before a controlled solve
    assert _rc(s.step_get, "alpha") == ERR_STATE
    # acceleration limits together with step control
    s.set_joint_accel_limits(np.full(w["model"].nv, 5.0))
    assert _rc(s.SolvePose, w["tg"], tol_pose=TOL, max_steps=3) == ERR_STATE
    assert b"loikb_pose_set_step_control" in L.loikb_last_error()
    s.set_joint_accel_limits(None)
    # the path and tracking loops name the setter to clear
    wp = w["tg"][:, None]
    assert _rc(s.SolvePosePath, wp, tol_pose=TOL, max_steps=3) == ERR_STATE
    assert b"loikb_pose_set_step_control(s, NULL)" in L.loikb_last_error()
    assert _rc(s.TrackPose, np.repeat(wp, 2, axis=1), tol_track=TOL) == ERR_STATE
    assert b"loikb_pose_set_step_control(s, NULL)" in L.loikb_last_error()
    assert _rc(s.step_get, "failed") == ERR_STATE
    # after all of them a plain solve is the fresh handle's, bit for bit
    s.clear_step_control()
    out = s.SolvePose(w["tg"], dt=w["dt"], gain=1.0, tol_pose=TOL, max_steps=3)
    out["q"] = s.get("q")
    for key in KEYS + ("limit_flags",):
        assert np.array_equal(out[key], fresh[key]), key
    assert _rc(s.step_get, "alpha") == ERR_STATE   # (the last solve ran without step control)
    # ... and a controlled solve afterwards has its results, the getter rejects an unknown field
    s.set_step_control()
    out = s.SolvePose(w["tg"], dt=w["dt"], gain=3.0, tol_pose=TOL, max_steps=2, q=w["q0"])
    assert out["backtracks"].any()
    buf = np.empty(w["B"])
    assert L.loikb_step_get(s.h, 7, buf.ctypes.data_as(C.c_void_p), 0) == ERR_ARG
    s.close()
