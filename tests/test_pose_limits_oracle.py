"""CPU: the lock-step oracle with joint position limits (tests/pose_limits_numpy.py) is proven before it referees the device.
RefSolver has no "replace the velocity box" call; the helper re-enters SolveInit every step (its docstring says why that keeps
every iterate).  Here: with all limits infinite it IS pose_numpy.lockstep_pose_loop -- np.array_equal, no tolerance -- on single-
and multi-DoF robots, shared and per-instance A, instances that leave the loop early (the idle b = 0 solves), tol_rel = 0 and
1e-3 (where bis_inf_norm_ enters the stopping test); and with limits that bind it keeps every limited coordinate in range exactly
and its reached instances satisfy tol_pose."""
import numpy as np
import pytest

import loik_amd

from test_pose_ik import PRM, _fk_models, _links
from test_pose_parity import _box, _leaf_and_multidof, _nonsym_A, _seeds
import pose_numpy as P
import pose_limits_numpy as PL

B = 16
TOL = 1e-4


def _problem(case):
    """(model, links, A) -- A non-symmetric by test_pose_parity's recipe, per instance where the case says so"""
    name, nc, per_inst = case
    if name == "multidof":
        model = _fk_models()[3]   # free-flyer root, a translation joint, two ZYX, a planar and three (cos, sin) joints
        links = _leaf_and_multidof(model)
    else:
        model = loik_amd.builtin_model(name)
        links = _links(model, nc)
    rng = np.random.default_rng(900 + 7 * nc + int(per_inst))
    return model, links, _nonsym_A(rng, len(links), B if per_inst else None)


CASES = [("talos32", 1, False), ("talos32", 2, True), ("panda7", 1, False), ("multidof", 2, True)]
IDS = ["%s-nc%d-%s" % (c[0], c[1], "Ainst" if c[2] else "Ash") for c in CASES]


@pytest.mark.parametrize("tol_rel", [0.0, 1e-3])
@pytest.mark.parametrize("max_steps", [1, 4])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_infinite_limits_reproduce_the_plain_lockstep_oracle(case, max_steps, tol_rel):
    model, links, A = _problem(case)
    prm = dict(PRM, tol_rel=tol_rel)
    q0, tg = _seeds(model, B, links, seed=910 + len(links))
    lb, ub = _box(model)
    inf = np.inf * np.ones(model.nv)
    for dt, gain in ((0.25, 0.5), (2.0, 1.7)):
        want = P.lockstep_pose_loop(model, prm, q0, np.eye(6), np.zeros(6), links, A, lb, ub, tg, dt, gain, TOL, max_steps)
        got = PL.lockstep_pose_loop_limits(model, prm, q0, np.eye(6), np.zeros(6), links, A, lb, ub, tg, dt, gain, TOL, max_steps, -inf, inf)
        for key in ("q", "steps", "status", "z", "iter", "err"):
            assert np.array_equal(got[key], want[key]), (case, max_steps, tol_rel, dt, key)
        assert not got["limit_flags"].any()
        if max_steps == 4:   # the case means something: instances leave the loop at different steps, some before the batch does
            assert len(set(want["steps"].tolist())) > 1 and want["steps"].min() < want["steps"].max() == 4


def test_limit_q_index_knows_which_dofs_can_carry_a_limit():
    model = _fk_models()[3]
    qi = PL.limit_q_index(model)
    assert qi.size == model.nv
    for i in range(1, model.njoints):
        jt, iq, iv = int(model.jtype[i]), int(model.idx_q[i]), int(model.idx_v[i])
        if jt == P.J_FREEFLYER:
            assert np.all(qi[iv:iv + 6] == -1)
        elif jt in (P.J_PLANAR, P.J_SPHERICAL):
            assert np.all(qi[iv:iv + 3] == -1)
        elif jt in (P.J_RUBX, P.J_RUBY, P.J_RUBZ, P.J_RUBU):
            assert qi[iv] == -1
        elif jt in (P.J_TRANSLATION, P.J_SPHERICAL_ZYX):
            assert list(qi[iv:iv + 3]) == [iq, iq + 1, iq + 2]
        else:
            assert qi[iv] == iq
    assert np.array_equal(PL.limit_q_index(loik_amd.builtin_model("panda7")), np.arange(7))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_binding_limits_hold_exactly_and_reached_means_reached(case):
    model, links, A = _problem(case)
    Bb = 48
    if A.ndim == 4:
        A = _nonsym_A(np.random.default_rng(5), len(links), Bb)
    q0, tg = _seeds(model, Bb, links, seed=930, spread=(1e-6, 0.15))
    q_t = model.random_configurations(np.random.default_rng(930), Bb)   # (the configurations _seeds drew its targets from)
    assert np.array_equal(P.fk12(model, q_t, links), tg)
    q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, seed=931, pct=(10.0, 90.0))
    lb, ub = _box(model)
    qi = PL.limit_q_index(model)
    lim = np.isfinite(q_lo)
    assert lim.any() and np.all(qi[lim] >= 0)
    o = PL.lockstep_pose_loop_limits(model, PRM, q0, np.eye(6), np.zeros(6), links, A, lb, ub, tg, 0.25, 0.5, TOL, 6, q_lo, q_hi)
    u = P.lockstep_pose_loop(model, PRM, q0, np.eye(6), np.zeros(6), links, A, lb, ub, tg, 0.25, 0.5, TOL, 6)
    ql = o["q"][:, qi[lim]]
    assert np.all(q_lo[lim] <= ql) and np.all(ql <= q_hi[lim])              # exactly: plain <=
    qu = u["q"][:, qi[lim]]
    assert np.any((qu < q_lo[lim]) | (qu > q_hi[lim])), "the limits never bound: the unlimited loop stays in range as well"
    assert np.max(np.abs(o["q"] - u["q"])) > 1e-3
    assert o["limit_flags"].any() and not o["limit_flags"][:, ~lim].any()
    assert o["reached"].any()
    e = P.pose_errors(model, o["q"], links, tg)
    assert np.all(np.abs(e[o["reached"]]).max(axis=(1, 2)) <= TOL)
    assert np.max(np.abs(e - o["err"])) < 1e-12   # (err is the last re-target's: the same q, evaluated row by row there)
