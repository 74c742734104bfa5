"""CPU: the lock-step path oracle (tests/pose_path_numpy.py) is proven before it referees the device.  With one waypoint and no
per-waypoint budget it IS pose_numpy.lockstep_pose_loop -- np.array_equal, no tolerance; on the asynchrony workload its loop is
as long as its longest instance, strictly shorter than waypoint-by-waypoint calls (the sum over waypoints of the batch maximum);
a per-waypoint budget stalls exactly the instances whose far leg needs more, at the right cursor; and a run of waypoints the seed
already satisfies is crossed in one re-target."""
import numpy as np
import pytest

import loik_amd

from test_pose_ik import PRM, _fk_models, _links
from test_pose_parity import _box, _leaf_and_multidof, _seeds
import pose_numpy as P
import pose_path_numpy as PP

# the asynchrony workload of the issue: A = I, box +-2, dt = 1, gain = 0.5, tol_pose = 1e-4, one constraint, 8 instances, 2 waypoints
# (the seed: one at which no panda7 configuration sits next to a singular posture, where a far leg takes 40 and more steps and
# dominates both ways of counting)
ASYNC = dict(dt=1.0, gain=0.5, tol=1e-4, B=8, T=2, max_steps=60, seed=1)
_ASYNC_RUNS = {}


def _async_run(name, budget=0):
    """the oracle on the asynchrony workload, computed once per (robot, budget) and shared"""
    key = (name, budget)
    if key not in _ASYNC_RUNS:
        model = loik_amd.builtin_model(name)
        links = _links(model, 1)
        q_a, wp, far_first = PP.asynchrony_workload(model, links, ASYNC["B"], ASYNC["T"], seed=ASYNC["seed"])
        lb, ub = _box(model)
        o = PP.lockstep_path_loop(model, PRM, q_a, np.eye(6), np.zeros(6), links, np.eye(6)[None], lb, ub, wp, ASYNC["dt"],
                                  ASYNC["gain"], ASYNC["tol"], ASYNC["max_steps"], budget=budget)
        _ASYNC_RUNS[key] = (model, links, q_a, wp, far_first, o)
    return _ASYNC_RUNS[key]


@pytest.mark.parametrize("max_steps", [0, 1, 4])
@pytest.mark.parametrize("name,nc", [("talos32", 2), ("panda7", 1)])
def test_one_waypoint_without_budget_is_the_plain_lockstep_oracle(name, nc, max_steps):
    model = loik_amd.builtin_model(name)
    links = _links(model, nc)
    B = 12
    q0, tg = _seeds(model, B, links, seed=1310 + nc)
    lb, ub = _box(model)
    A = np.tile(np.eye(6), (nc, 1, 1))
    for dt, gain in ((0.25, 0.5), (1.0, 1.0)):
        want = P.lockstep_pose_loop(model, PRM, q0, np.eye(6), np.zeros(6), links, A, lb, ub, tg, dt, gain, 1e-4, max_steps)
        got = PP.lockstep_path_loop(model, PRM, q0, np.eye(6), np.zeros(6), links, A, lb, ub, tg[:, None], dt, gain, 1e-4, max_steps)
        for key in want:
            assert np.array_equal(got[key], want[key]), (name, max_steps, dt, key)
        assert np.array_equal(got["cursor"], want["reached"].astype(np.int32))
        assert np.array_equal(got["wsteps"][:, 0], want["steps"])
        assert np.array_equal(got["path_status"], want["reached"].astype(np.int32) * PP.PATH_COMPLETE)
        r = want["reached"]
        assert np.array_equal(got["q_path"][r, 0], want["q"][r]) and np.all(np.isnan(got["q_path"][~r]))
    if max_steps == 4:   # (the case means something: instances leave the loop at different steps)
        assert len(set(want["steps"].tolist())) > 1


@pytest.mark.parametrize("name", ["talos32", "panda7"])
def test_asynchrony_loop_is_the_longest_instance_not_the_sum_of_waypoint_maxima(name):
    model, links, q_a, wp, far_first, o = _async_run(name)
    assert np.all(o["path_status"] == PP.PATH_COMPLETE) and o["reached"].all() and np.all(o["cursor"] == ASYNC["T"])
    assert np.array_equal(o["wsteps"].sum(axis=1), o["steps"])
    lockstep = int(o["wsteps"].max(axis=0).sum())
    print("%s: path loop %d inner solves, waypoint-by-waypoint %d" % (name, o["n_solves"], lockstep))
    assert o["n_solves"] == o["steps"].max()
    assert o["n_solves"] < lockstep, (o["n_solves"], lockstep)
    # the far leg costs more than the near one, whichever comes first
    far = np.where(far_first, o["wsteps"][:, 0], o["wsteps"][:, 1])
    near = np.where(far_first, o["wsteps"][:, 1], o["wsteps"][:, 0])
    assert np.all(far > near)
    # and waypoint-by-waypoint calls of the existing oracle cost what wsteps says they do: the per-waypoint batch maxima
    lb, ub = _box(model)
    q, total = q_a, 0
    for t in range(ASYNC["T"]):
        leg = P.lockstep_pose_loop(model, PRM, q, np.eye(6), np.zeros(6), links, np.eye(6)[None], lb, ub, wp[:, t], ASYNC["dt"],
                                   ASYNC["gain"], ASYNC["tol"], ASYNC["max_steps"])
        assert leg["reached"].all()
        total += int(leg["steps"].max())
        q = leg["q"]
    print("%s: chained lockstep_pose_loop calls: %d inner solves" % (name, total))
    assert o["n_solves"] < total


@pytest.mark.parametrize("name", ["talos32", "panda7"])
def test_budget_stalls_the_instances_whose_far_leg_needs_more(name):
    budget = 3
    model, links, q_a, wp, far_first, free = _async_run(name)
    _, _, _, _, _, o = _async_run(name, budget)
    over = free["wsteps"] > budget                       # [B][T]: legs that need more than the budget, on the unbudgeted run
    first_over = np.where(over.any(axis=1), over.argmax(axis=1), ASYNC["T"])
    stalled = (o["path_status"] & PP.PATH_STALLED) != 0
    assert over.any() and not over.all(axis=1).all()
    assert np.array_equal(stalled, over.any(axis=1))
    assert np.array_equal(o["cursor"], first_over)
    assert not (o["status"][stalled] & (P.POSE_REACHED | P.POSE_STOPPED)).any()
    assert np.all(o["path_status"][~stalled] == PP.PATH_COMPLETE)
    for b in np.flatnonzero(stalled):
        w = o["cursor"][b]
        assert o["wsteps"][b, w] == budget and not o["wsteps"][b, w + 1:].any()
        assert np.array_equal(o["wsteps"][b, :w], free["wsteps"][b, :w])
        assert np.all(np.isnan(o["q_path"][b, w:])) and np.all(np.isfinite(o["q_path"][b, :w]))
        assert np.max(np.abs(o["err"][b])) > ASYNC["tol"]
        # up to the stall the instance took the steps of the unbudgeted run: the waypoints it reached, it reached at the same q
        assert np.array_equal(o["q_path"][b, :w], free["q_path"][b, :w])
    assert np.array_equal(o["q"][~stalled], free["q"][~stalled])


def test_satisfied_waypoints_are_crossed_in_one_retarget():
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 1)
    B, T = 6, 4
    q0, tg = _seeds(model, B, links, seed=77, spread=(0.05, 0.1))
    here = P.fk12(model, q0, links)
    wp = np.stack([here, here, here, tg], axis=1)        # three waypoints at the seed, then a real one
    wp[1::2, 3] = here[1::2]                             # odd instances: the whole path is already satisfied
    lb, ub = _box(model)
    for max_steps in (0, 30):
        o = PP.lockstep_path_loop(model, PRM, q0, np.eye(6), np.zeros(6), links, np.eye(6)[None], lb, ub, wp, 1.0, 1.0, 1e-4, max_steps)
        assert not o["wsteps"][:, :3].any()
        assert np.array_equal(o["q_path"][:, :3], np.repeat(q0[:, None], 3, axis=1))
        assert np.all(o["cursor"][1::2] == T) and not o["steps"][1::2].any() and np.array_equal(o["q"][1::2], q0[1::2])
        if max_steps == 0:
            assert np.all(o["cursor"][0::2] == 3) and np.all(np.isnan(o["q_path"][0::2, 3]))
            assert np.max(np.abs(o["err"][0::2])) > 1e-4 and o["n_solves"] == 0
        else:
            assert np.all(o["cursor"][0::2] == T) and np.all(o["wsteps"][0::2, 3] > 0)
            assert np.array_equal(o["wsteps"][:, 3], o["steps"])


@pytest.mark.parametrize("variant", ["limits", "tasks", "tasks+limits"])
def test_one_waypoint_variants_are_the_limits_and_tasks_oracles(variant):
    """the variants with joint limits and with tasks, one waypoint: np.array_equal to the oracles whose rules they import"""
    import pose_limits_numpy as PL
    import pose_tasks_numpy as PT
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 2)
    B, nc = 10, 2
    q0, tg = _seeds(model, B, links, seed=1320)
    q_t = model.random_configurations(np.random.default_rng(1320), B)
    lb, ub = _box(model)
    kw = {}
    if "limits" in variant:
        q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, seed=5)
        kw.update(q_lo=q_lo, q_hi=q_hi)
    A = np.tile(np.eye(6), (nc, 1, 1))
    args = (model, PRM, q0, np.eye(6), np.zeros(6), links)
    if "tasks" in variant:
        kinds, frames = [PT.TASK_POSITION, PT.TASK_POSE], PT.random_frames(np.random.default_rng(6), nc)
        tg = PT.frame_fk12(model, q_t, links, frames)
        want = PT.lockstep_pose_loop_tasks(*args, kinds, frames, lb, ub, tg, 0.5, 0.8, 1e-4, 4, **kw)
        kw.update(kinds=kinds, frames=frames)
    else:
        want = PL.lockstep_pose_loop_limits(*args, A, lb, ub, tg, 0.5, 0.8, 1e-4, 4, kw["q_lo"], kw["q_hi"])
    got = PP.lockstep_path_loop(*args, A, lb, ub, tg[:, None], 0.5, 0.8, 1e-4, 4, **kw)
    for key in want:
        assert np.array_equal(got[key], want[key]), (variant, key)
    assert want["steps"].any()


def test_single_instance_path_on_a_free_flyer_tree_is_chained_lockstep_pose_loops():
    """nq != nv: a free-flyer root with ZYX, planar and (cos, sin) joints.  One instance never idles, so a path is the chain of
    lockstep_pose_loop calls, each from where the last one ended.  A chained call starts a fresh solver: without warm starts the
    inner solves are the same arithmetic and the two are np.array_equal; with them (PRM) the steps per waypoint are equal and q
    differs by what two inner solves stopped at tol_abs = 1e-6 from different starts differ by, carried over at most 16 steps"""
    from test_pose_path import _path_workload
    model = _fk_models()[3]
    assert model.nq > model.nv
    links = _leaf_and_multidof(model)
    T = 4
    q0, wp, _ = _path_workload(model, links, 1, T, seed=1403, spread=(0.1, 0.15))
    lb, ub = _box(model)
    A = np.tile(np.eye(6), (2, 1, 1))
    for warm in (False, True):
        prm = dict(PRM, warm_start=warm)
        o = PP.lockstep_path_loop(model, prm, q0, np.eye(6), np.zeros(6), links, A, lb, ub, wp, 1.0, 0.8, 1e-4, 100)
        assert o["cursor"][0] == T and o["path_status"][0] == PP.PATH_COMPLETE and o["wsteps"].sum() == o["steps"][0] > T
        assert o["q_path"].shape == (1, T, model.nq) and np.all(np.isfinite(o["q_path"]))
        q = q0
        for t in range(T):
            leg = P.lockstep_pose_loop(model, prm, q, np.eye(6), np.zeros(6), links, A, lb, ub, wp[:, t], 1.0, 0.8, 1e-4, 100)
            q = leg["q"]
            assert leg["reached"][0] and leg["steps"][0] == o["wsteps"][0, t], (warm, t, leg["steps"], o["wsteps"])
            if warm:
                assert np.max(np.abs(q - o["q_path"][:, t])) < 1e-5, (t, np.max(np.abs(q - o["q_path"][:, t])))
            else:
                assert np.array_equal(q, o["q_path"][:, t]), (t, np.max(np.abs(q - o["q_path"][:, t])))
        assert np.array_equal(q, o["q"]) or warm
