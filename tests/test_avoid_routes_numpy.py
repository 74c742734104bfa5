"""CPU: the `narrow` hook of the path, tracking and step-control oracles (avoid_numpy.narrower) proven against the oracles it extends,
and the conditions that make every input of tests/test_avoid_routes.py a test, on the reference alone: the share of near instances,
the narrowed share where a case claims one, the stall / complete / reach conditions, and for the ragged batches that no decision of
the oracle lies near its threshold.  Each `*_conditions` function returns the list of the conditions an input misses (empty: none)."""
import numpy as np
import pytest

import avoid_numpy as AN
import pose_limits_numpy as PL
import pose_numpy as P
import pose_path_numpy as PP
import pose_step_numpy as PS
import pose_track_numpy as TR
import test_avoid_pose as TP
import test_avoid_routes as R

NEAR_SHARE = 0.02
KEYS = ("q", "steps", "status", "err", "z", "iter")


# ---- 1. the hook ---------------------------------------------------------------------------------------------------------------------
def _args(w, idx, tg):
    return (w["model"], TP.PRM, w["q0"][idx], np.eye(6), np.zeros(6), w["links"], w["A"]) + w["box"] + (tg,)


def test_without_the_hook_the_three_oracles_are_what_they_were():
    """narrow=None: bit for bit the oracles this file's hook leaves alone -- on the branch without limits pose_numpy.lockstep_pose_loop, on
    the branch with limits pose_limits_numpy.lockstep_pose_loop_limits (one waypoint without a budget, constant samples without
    feed-forward and tol 0, no backtracks and no patience are those loops: the identities of test_pose_path_oracle.py,
    test_pose_track_oracle.py and test_pose_step_oracle.py)"""
    w = TP._workload("panda7", 1)
    idx = np.arange(4)
    tg, k, dt, gain = w["tg"][idx], 3, 0.25, 0.5
    lim = dict(q_lo=w["q_lo"], q_hi=w["q_hi"])
    plain = P.lockstep_pose_loop(*_args(w, idx, tg), dt, gain, TP.TOL, k)
    limits = PL.lockstep_pose_loop_limits(*_args(w, idx, tg), dt, gain, TP.TOL, k, w["q_lo"], w["q_hi"])
    assert limits["limit_flags"].any() and not np.array_equal(plain["q"], limits["q"])
    for want, kw in ((plain, {}), (limits, lim)):
        path = PP.lockstep_path_loop(*_args(w, idx, tg[:, None]), dt, gain, TP.TOL, k, narrow=None, **kw)
        step = PS.lockstep_pose_loop_step(*_args(w, idx, tg), dt, gain, TP.TOL, k, max_backtracks=0, patience=0, narrow=None, **kw)
        for key in KEYS + (("limit_flags",) if kw else ()):
            assert np.array_equal(path[key], want[key]), ("path", key)
            assert np.array_equal(step[key], want[key]), ("step", key)
        assert ("limit_flags" in path) == bool(kw) and ("limit_flags" in step) == bool(kw)
        zero = P.lockstep_pose_loop(*_args(w, idx, tg), dt, gain, 0.0, k) if not kw else \
            PL.lockstep_pose_loop_limits(*_args(w, idx, tg), dt, gain, 0.0, k, w["q_lo"], w["q_hi"])
        track = TR.lockstep_track_loop(*_args(w, idx, np.repeat(tg[:, None], k + 1, axis=1)), dt, gain, 0.0, ff=TR.FF_NONE, narrow=None, **kw)
        for key in KEYS + (("limit_flags",) if kw else ()):
            assert np.array_equal(track[key], zero[key]), ("track", key)


def test_an_identity_hook_is_the_limits_branch():
    """a hook that narrows nothing, without q_lo / q_hi: the limits branch with infinite limits, whose box is the base box -- the q, steps
    and status of the plain loop, and limit_flags that are all zero"""
    w = TP._workload("panda7", 0)
    idx = np.arange(4)
    tg, k, dt, gain = w["tg"][idx], 3, 0.25, 0.5
    calls = []
    same = lambda b, q_b, lo, hi: (calls.append(b), (lo, hi))[1]
    plain = P.lockstep_pose_loop(*_args(w, idx, tg), dt, gain, TP.TOL, k)
    path = PP.lockstep_path_loop(*_args(w, idx, tg[:, None]), dt, gain, TP.TOL, k, narrow=same)
    step = PS.lockstep_pose_loop_step(*_args(w, idx, tg), dt, gain, TP.TOL, k, max_backtracks=0, patience=0, narrow=same)
    assert len(calls) == 2 * int(plain["steps"].sum()) and plain["steps"].any()
    for got in (path, step):
        for key in ("q", "steps", "status", "err"):
            assert np.array_equal(got[key], plain[key]), key
        assert not got["limit_flags"].any()


def test_step_oracle_with_the_hook_is_the_avoid_oracle():
    """max_backtracks = 0 and patience = 0 take the plain step whatever the search says: with the hook, lockstep_pose_loop_avoid bit for bit"""
    w = TP._workload("panda7", 0)
    dt, gain, k = 0.25, 0.5, 4
    want = TP._oracle(w, dt, gain, k)
    hook = AN.narrower(w["model"], w["col"], TP.AVOID, dt, w["B"])
    got = PS.lockstep_pose_loop_step(*_args(w, np.arange(w["B"]), w["tg"]), dt, gain, TP.TOL, k, max_backtracks=0, patience=0, narrow=hook)
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
    for key in R.RESULTS + ("near",):
        assert np.array_equal(hook.results[key], want[key]), key
    assert (want["avoid_active_steps"] > 0).mean() >= 0.25 and want["steps"].max() == k


# ---- 2. the inputs of test_avoid_routes.py --------------------------------------------------------------------------------------------
def _narrowed(o):
    return float((o["avoid_active_steps"] > 0).mean())


def route_conditions(w, laws=TP.LAWS, steps=R.ROUTE_STEPS):
    miss = []
    for dt, gain in laws:
        for k in steps:
            o = TP._oracle(w, dt, gain, k)
            if o["near"].mean() > NEAR_SHARE:
                miss.append(("near", dt, k, float(o["near"].mean())))
            if _narrowed(o) < 0.25:
                miss.append(("narrowed", dt, k, _narrowed(o)))
    return miss


@pytest.mark.parametrize("case", R.ROUTES, ids=R.route_id)
def test_route_matrix_inputs(case):
    w = R.route_case(case)
    o = TP._oracle(w, *TP.LAWS[0], 4)
    print("avoid_routes_numpy %s: narrowed %.3f reached %.3f steps %s limit flags %d" % (R.route_id(case), _narrowed(o), o["reached"].mean(),
                                                                                       np.bincount(o["steps"]).tolist(), int((o["limit_flags"] != 0).any(axis=1).sum())))
    assert route_conditions(w) == []
    if case[1]:   # (the limits bind on some instance, so that the interval in the tiles is not the base box)
        assert (o["limit_flags"] != 0).any()


def ragged_conditions(w):
    dt, gain = R.RAGGED_LAW
    o = TP._oracle(w, dt, gain, R.RAGGED_STEPS)
    miss = []
    if o["near"].any():
        miss.append("near")
    margin = R.decision_margin(w, o)
    if margin < 1e-3:
        miss.append(("margin", margin))
    if not (o["avoid_active_steps"] > 0).any() or (w["B"] > 1 and _narrowed(o) < 0.25):
        miss.append(("narrowed", _narrowed(o)))
    if o["steps"].max() < 2:
        miss.append("steps")
    return miss


@pytest.mark.parametrize("case", R.RAGGED, ids=lambda c: "B%d-%s" % (c[0], "boxinst" if c[1] else "boxsh"))
def test_ragged_inputs(case):
    assert ragged_conditions(R.ragged_case(case)) == []


def back_conditions(w):
    o = R.back_oracle()
    early = float(o["idle"].mean())
    miss = [] if o["near"].mean() <= NEAR_SHARE else ["near"]
    if not (o["idle"] & ~o["near"] & (o["outside"] > 1e-4)).any():   # (1e-4: far above the gate's 1e-7, so the two boxes cannot be confused)
        miss.append(("idle z outside the last narrowed box", o["outside"].tolist()))
    if early < 0.10:
        miss.append(("reached before the last step", early))
    if _narrowed(o) < 0.25:
        miss.append(("narrowed", _narrowed(o)))
    return miss


def test_base_box_input():
    assert back_conditions(R.back_case()) == []


def contain_conditions(w):
    o = TP._oracle(w, *R.CONTAIN_LAW, R.CONTAIN_CALLS)
    miss = [] if o["near"].mean() <= NEAR_SHARE else ["near"]
    if _narrowed(o) < 0.25:
        miss.append(("narrowed", _narrowed(o)))
    if R.resting_on_narrowed(w, R.CONTAIN_LAW) < 8:   # (rounding to nearest rounds about half of them outward: enough that one is)
        miss.append(("resting on a narrowed side", R.resting_on_narrowed(w, R.CONTAIN_LAW)))
    return miss


@pytest.mark.parametrize("box_inst", [False, True])
def test_containment_inputs(box_inst):
    assert contain_conditions(R.contain_case(box_inst)) == []


def path_conditions(w):
    o = R.path_oracle(w)
    miss = [] if o["near"].mean() <= NEAR_SHARE else ["near"]
    if not (o["path_status"] == PP.PATH_STALLED).any():
        miss.append("stalled")
    if not (o["path_status"] == PP.PATH_COMPLETE).any():
        miss.append("complete")
    later = [b for b in range(w["B"]) if o["cursor"][b] >= 1 and any(o["calls"][b][int(o["wsteps"][b, 0]):])]
    if not later:
        miss.append("narrowed after the first waypoint")
    if w["q_lo"] is not None and not (o["limit_flags"] != 0).any():
        miss.append("limits")
    return miss


@pytest.mark.parametrize("case", R.PATHS, ids=lambda c: "%s-%s" % (c[0], "limits" if c[1] else "nolimits"))
def test_path_inputs(case):
    w = R.path_workload(*case)
    o = R.path_oracle(w)
    print("avoid_routes_numpy path %s: cursor %s path_status %s steps %s narrowed %.3f" % (case, np.bincount(o["cursor"], minlength=R.PATH_T + 1).tolist(),
                                                                                         np.bincount(o["path_status"], minlength=3).tolist(), np.bincount(o["steps"]).tolist(), _narrowed(o)))
    assert path_conditions(w) == []


def track_conditions(w, o):
    miss = [] if o["near"].mean() <= NEAR_SHARE else ["near"]
    if _narrowed(o) < 0.25:
        miss.append(("narrowed", _narrowed(o)))
    if w["q_lo"] is not None and not (o["inner"] & TR.IN_LIMIT).any():
        miss.append("limits")
    return miss


@pytest.mark.parametrize("case", R.TRACKS, ids=lambda c: "%s-%s" % (c[0], "limits" if c[1] else "nolimits"))
def test_track_inputs(case):
    w = R.track_workload(*case)
    assert track_conditions(w, R.track_oracle(w)) == []


def test_wall_track_input():
    o = R.wall_track_oracle()
    assert o["near"].mean() <= NEAR_SHARE and _narrowed(o) >= 0.5 and not (o["status"] & P.POSE_STOPPED).any()


def step_conditions(w, ctl):
    o = R.step_oracle(w, ctl)
    miss = [] if o["near"].mean() <= NEAR_SHARE else ["near"]
    keep = ~o["near"] & ~(o["margin"] < R.STEP_MARGIN)
    if keep.mean() < 0.75:
        miss.append(("kept", float(keep.mean())))
    if _narrowed(o) < 0.25:
        miss.append(("narrowed", _narrowed(o)))
    if ctl["patience"]:
        stalled = (o["status"] & PS.POSE_STALLED) != 0
        if not (stalled & keep & (o["avoid_active_steps"] > o["steps"])).any():
            miss.append("stalled with a constraint active")
    else:
        if (o["backtracks"][keep] > 0).mean() < 0.25:
            miss.append(("backtracked", float((o["backtracks"][keep] > 0).mean())))
        if not ((o["backtracks"] > 0) & (o["avoid_active_steps"] > 0) & keep).any():
            miss.append("backtracked and narrowed")
    return miss


@pytest.mark.parametrize("case", R.STEP_CASES, ids=R.step_id)
def test_step_control_inputs(case):
    w = R.step_workload(case[0], case[1])
    o = R.step_oracle(w, case[2])
    print("avoid_routes_numpy step %s: steps %s backtracks %s failed %s stalled %d narrowed %.3f margin min %.3e" % (
        R.step_id(case), o["steps"].tolist(), o["backtracks"].tolist(), o["failed"].tolist(), int(((o["status"] & PS.POSE_STALLED) != 0).sum()), _narrowed(o), o["margin"].min()))
    assert step_conditions(w, case[2]) == []


def multistart_conditions(w=None):
    o = R.multistart_oracle(w)
    last = o["last"]
    earlier = last["reached"] & (last["steps"] == 0)
    miss = [] if last["near"].mean() <= NEAR_SHARE else ["near"]
    if o["rounds_run"] != R.MS_ROUNDS or not o["answered"][0] < o["answered"][-1] < R.MS_G:
        miss.append(("answered", o["answered"]))
    if not earlier.any():
        miss.append("reached in an earlier round")
    if not (last["avoid_active_steps"][~earlier] > 0).any():
        miss.append("narrowed in the last round")
    return miss


def test_multistart_input():
    print("avoid_routes_numpy multistart: answered per round %s" % R.multistart_oracle()["answered"])
    assert multistart_conditions() == []
