"""CPU: the lock-step oracle with step control (tests/pose_step_numpy.py, the rule of include/loik_amd_step.h) is proven before it
referees the device.  With max_backtracks = 0 and patience = 0 it IS the plain lock-step loop -- np.array_equal, no tolerance --
with and without joint limits; at a gain that converges anyway it never backtracks; at gain 2.5, where the plain loop diverges, it
rescues the batch; the merit never rises across an accepted step; and with patience the instances stall where the rule says."""
import numpy as np
import pytest

import loik_amd

from test_pose_ik import PRM, _links
from test_pose_parity import _box, _nonsym_A, _seeds
import pose_numpy as P
import pose_limits_numpy as PL
import pose_step_numpy as PS

TOL = 1e-4
KEYS = ("q", "steps", "status", "err", "z", "iter")
CASES = [("talos32", 1, 32), ("panda7", 1, 64)]   # (robot, nc, B of the rescue / stall cases; the identities run 16 instances)
IDS = [c[0] for c in CASES]


def _problem(name, nc, B, spread=(1e-3, 0.3)):
    model = loik_amd.builtin_model(name)
    links = _links(model, nc)
    q0, tg = _seeds(model, B, links, seed=7, spread=spread)
    return model, links, q0, tg


def _plain(model, links, q0, tg, A, gain, k, dt=1.0):
    lb, ub = _box(model)
    return P.lockstep_pose_loop(model, PRM, q0, np.eye(6), np.zeros(6), links, A, lb, ub, tg, dt, gain, TOL, k)


def _step(model, links, q0, tg, A, gain, k, dt=1.0, **kw):
    lb, ub = _box(model)
    return PS.lockstep_pose_loop_step(model, PRM, q0, np.eye(6), np.zeros(6), links, A, lb, ub, tg, dt, gain, TOL, k, **kw)


# ---- 1. no backtracking, no patience: the plain loop --------------------------------------------------------------------------
@pytest.mark.parametrize("gain", [1.0, 2.5])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_backtracks_no_patience_is_the_plain_loop(case, gain):
    name, nc, B = case
    B = 16
    model, links, q0, tg = _problem(name, nc, B)
    A = _nonsym_A(np.random.default_rng(3), nc, B)
    want = _plain(model, links, q0, tg, A, gain, 4, dt=0.5)
    got = _step(model, links, q0, tg, A, gain, 4, dt=0.5, max_backtracks=0, patience=0)
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), (case, gain, key)
    # every search either accepted trial 0 or failed and took it all the same
    assert not got["backtracks"].any()
    searched = got["trial"] != -2
    assert np.array_equal(searched.sum(axis=1), want["steps"])
    assert np.array_equal(got["failed"], (got["trial"] == -1).sum(axis=1))
    if gain == 2.5:
        assert got["failed"].any(), "the case means nothing: no search failed"
        gone = got["failed"] == got["steps"]
        assert gone.any()   # instances every step of which raised the error


def test_no_backtracks_with_limits_is_the_limits_loop():
    B = 16
    model, links, q0, tg = _problem("panda7", 1, B)
    q_t = model.random_configurations(np.random.default_rng(7), B)
    assert np.array_equal(P.fk12(model, q_t, links), tg)
    q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, seed=11)
    A = np.eye(6)[None]
    lb, ub = _box(model)
    want = PL.lockstep_pose_loop_limits(model, PRM, q0, np.eye(6), np.zeros(6), links, A, lb, ub, tg, 1.0, 2.5, TOL, 4, q_lo, q_hi)
    got = PS.lockstep_pose_loop_step(model, PRM, q0, np.eye(6), np.zeros(6), links, A, lb, ub, tg, 1.0, 2.5, TOL, 4, max_backtracks=0,
                                     patience=0, q_lo=q_lo, q_hi=q_hi)
    for key in KEYS + ("limit_flags",):
        assert np.array_equal(got[key], want[key]), key
    assert want["limit_flags"].any()


# ---- 2. a gain that converges anyway: never a backtrack ------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gain_half_never_backtracks(case):
    name, nc, B = case
    B = 16
    model, links, q0, tg = _problem(name, nc, B)
    A = np.eye(6)[None]
    want = _plain(model, links, q0, tg, A, 0.5, 6)
    got = _step(model, links, q0, tg, A, 0.5, 6)
    assert not got["backtracks"].any() and not got["failed"].any()
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), (case, key)
    assert np.all(got["alpha"][got["steps"] > 0] == 1.0) and np.all(got["alpha"][got["steps"] == 0] == 0.0)


# ---- 3. / 4. the rescue at gain 2.5, and the merit across accepted steps --------------------------------------------------------
_RESCUE = {}


def _rescue():
    if not _RESCUE:
        model, links, q0, tg = _problem("talos32", 1, 32)
        A = np.eye(6)[None]
        _RESCUE["plain"] = _plain(model, links, q0, tg, A, 2.5, 30)
        _RESCUE["step"] = _step(model, links, q0, tg, A, 2.5, 30)
    return _RESCUE["plain"], _RESCUE["step"]


def test_rescue_at_gain_2p5():
    plain, ctl = _rescue()
    print("reached: plain %.3f, controlled %.3f; controlled steps max %d" % (plain["reached"].mean(), ctl["reached"].mean(), ctl["steps"].max()))
    assert plain["reached"].mean() <= 0.10
    assert ctl["reached"].mean() >= 0.90
    assert ctl["backtracks"].any()


def test_merit_never_rises_across_an_accepted_step():
    _, ctl = _rescue()
    phi, trial = ctl["phi"], ctl["trial"]
    before = np.concatenate([ctl["phi0"][:, None], phi[:, :-1]], axis=1)
    acc = trial >= 0
    assert acc.sum() > 32
    assert np.all(phi[acc] <= before[acc])
    # ... by the sufficient-decrease margin, with the alpha the search settled on
    a = 0.5 ** trial[acc]
    assert np.all(phi[acc] <= (1.0 - 1e-4 * a) * before[acc])


# ---- 5. patience: the stall verdict ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stall_after_three_failed_searches(case):
    name, nc, B = case
    model, links, q0, tg = _problem(name, nc, B)
    A = np.eye(6)[None]
    got = _step(model, links, q0, tg, A, 2.5, 30, max_backtracks=0, patience=3)
    two = _plain(model, links, q0, tg, A, 2.5, 2)
    start = np.abs(P.pose_errors(model, q0, links, tg)).max(axis=(1, 2)) <= TOL
    run = ~start
    assert run.sum() >= B // 2
    assert np.all(got["status"][run] & PS.POSE_STALLED) and not np.any(got["status"][start] & PS.POSE_STALLED)
    assert not got["reached"][run].any()
    assert np.all(got["steps"][run] == 2) and np.all(got["failed"][run] == 3)
    assert np.array_equal(got["q"][run], two["q"][run])
    assert np.array_equal(got["q"][start], q0[start]) and np.all(got["reached"][start])
