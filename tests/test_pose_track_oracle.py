"""CPU: the lock-step tracking oracle (tests/pose_track_numpy.py) is proven before it referees the device.  Without feed-forward
and on constant samples it IS pose_numpy.lockstep_pose_loop with tol = 0 and max_steps = T -- np.array_equal, no tolerance; on a
smooth joint path the feed-forward law tracks strictly better than pure feedback at every sample, for both gains and all three
task kinds; for position tasks at gain 1 a feed-forward step is the feedback step aimed at the next sample; and the transport
of the desired frame's twist to the actual frame is checked against exp6 / log6 compositions."""
import numpy as np
import pytest

import loik_amd

from test_pose_ik import PRM, _fk_models, _links
from test_pose_parity import _box, _leaf_and_multidof, _seeds
import pose_numpy as P
import pose_tasks_numpy as PT
import pose_track_numpy as TR

T_PATH = 5
_RUNS = {}


def _on_path_run(name, kind, gain, ff):
    """the oracle on the on-path workload of the issue (A = I, the +-2 box, B = 4, dt = 0.5), computed once per case and shared"""
    key = (name, kind, gain, ff)
    if key not in _RUNS:
        model = loik_amd.builtin_model(name)
        links = _links(model, 1)
        frames = PT.random_frames(np.random.default_rng(11), 1)
        q_a, smp, q_path = TR.joint_path_workload(model, links, 4, T_PATH, seed=2100, frames=frames)
        lb, ub = _box(model)
        _RUNS[key] = TR.lockstep_track_loop(model, PRM, q_a, np.eye(6), np.zeros(6), links, np.eye(6)[None], lb, ub, smp, 0.5, gain, 1e-4,
                                            ff=ff, kinds=[kind], frames=frames)
    return _RUNS[key]


@pytest.mark.parametrize("name,nc", [("talos32", 2), ("panda7", 1)])
def test_no_feedforward_on_constant_samples_is_the_plain_lockstep_oracle(name, nc):
    model = loik_amd.builtin_model(name)
    _check_no_feedforward_is_the_plain_lockstep_oracle(model, _links(model, nc))


def test_no_feedforward_on_constant_samples_is_the_plain_lockstep_oracle_on_a_free_flyer_tree():
    """nq != nv: a free-flyer root with a spherical and a translation joint"""
    model = _fk_models()[2]
    assert model.nq > model.nv
    _check_no_feedforward_is_the_plain_lockstep_oracle(model, _leaf_and_multidof(model))


def _check_no_feedforward_is_the_plain_lockstep_oracle(model, links):
    name, nc = model.name, len(links)
    B, T = 8, 4
    q0, tg = _seeds(model, B, links, seed=2000 + nc)
    lb, ub = _box(model)
    A = np.tile(np.eye(6), (nc, 1, 1))
    smp = np.repeat(tg[:, None], T + 1, axis=1)
    for dt, gain in ((0.25, 0.5), (1.0, 1.0)):
        want = P.lockstep_pose_loop(model, PRM, q0, np.eye(6), np.zeros(6), links, A, lb, ub, tg, dt, gain, 0.0, T)
        got = TR.lockstep_track_loop(model, PRM, q0, np.eye(6), np.zeros(6), links, A, lb, ub, smp, dt, gain, 0.0, ff=TR.FF_NONE)
        for key in want:
            assert np.array_equal(got[key], want[key]), (name, dt, key)
        assert np.all(want["steps"] == T) and np.array_equal(got["q_traj"][:, T], want["q"]) and np.array_equal(got["q_traj"][:, 0], q0)
        assert np.array_equal(got["errmax"][:, T], np.abs(want["err"]).max(axis=(1, 2))) and not got["ontrack"].any()
        assert np.array_equal(got["z_traj"][:, T - 1], want["z"])


@pytest.mark.parametrize("kind", [PT.TASK_POSE, PT.TASK_POSITION, PT.TASK_ORIENTATION], ids=["pose", "position", "orientation"])
@pytest.mark.parametrize("gain", [1.0, 0.5])
@pytest.mark.parametrize("name", ["panda7", "talos32"])
def test_feedforward_tracks_strictly_better_at_every_sample(name, gain, kind):
    none, diff = _on_path_run(name, kind, gain, TR.FF_NONE), _on_path_run(name, kind, gain, TR.FF_DIFFERENCE)
    assert np.all(none["steps"] == T_PATH) and np.all(diff["steps"] == T_PATH)
    print("%s gain %g kind %d: errmax none %s, difference %s" % (name, gain, kind, none["errmax"].max(axis=0), diff["errmax"].max(axis=0)))
    assert np.all(none["errmax"][:, 0] < 1e-12) and np.array_equal(none["errmax"][:, 0], diff["errmax"][:, 0])   # both start ON the path
    assert np.all(diff["errmax"][:, 1:] < none["errmax"][:, 1:])
    assert np.all(diff["worst"] < none["worst"])
    w, at = TR.worst_of(diff["errmax"])
    assert np.array_equal(w, diff["errmax"][:, 1:].max(axis=1)) and np.array_equal(at, diff["errmax"][:, 1:].argmax(axis=1) + 1)


@pytest.mark.parametrize("name", ["panda7", "talos32"])
def test_position_feedforward_step_is_the_feedback_step_aimed_at_the_next_sample(name):
    """position tasks, gain 1: dt f + e is the error against X_{k+1}, so one FF_DIFFERENCE step from X_0 is one pure-feedback step of
    pose_tasks_numpy.lockstep_pose_loop_tasks aimed at X_1 (the seeds are displaced off the path, so that e is not 0)"""
    model = loik_amd.builtin_model(name)
    links = _links(model, 2)
    B, dt = 4, 0.5
    rng = np.random.default_rng(2200)
    frames = PT.random_frames(rng, 2)
    kinds = [PT.TASK_POSITION] * 2
    q_a, smp, _ = TR.joint_path_workload(model, links, B, 3, seed=2201, frames=frames)
    q0 = np.stack([P.integrate(model, q_a[b], 0.01 * rng.normal(size=model.nv)) for b in range(B)])
    lb, ub = _box(model)
    args = (model, PRM, q0, np.eye(6), np.zeros(6), links)
    got = TR.lockstep_track_loop(*args, None, lb, ub, smp[:, :2], dt, 1.0, 1e-4, ff=TR.FF_DIFFERENCE, kinds=kinds, frames=frames)
    want = PT.lockstep_pose_loop_tasks(*args, kinds, frames, lb, ub, smp[:, 1], dt, 1.0, 0.0, 1)
    assert np.all(want["steps"] == 1) and np.all(got["steps"] == 1)
    assert np.max(np.abs(got["q"] - want["q"])) <= 1e-12 and np.max(np.abs(got["z_traj"][:, 0] - want["z"])) <= 1e-12
    assert np.max(np.abs(got["err"] - want["err"])) <= 1e-12
    assert np.max(np.abs(want["q"] - q0)) > 1e-3


def _compose(A, B):
    return A[0] @ B[0], A[1] + A[0] @ B[1]


def _inverse(A):
    return A[0].T, -A[0].T @ A[1]


def test_transport_against_exp6_log6_compositions():
    """M = (Re, pe) = the desired frame seen from the actual one.  The actual frame moved by exp6(h f) and the desired one by
    exp6(h u) keep their relative placement iff f is u transported by M: exp6(h f)^-1 M exp6(h u) = M.  Checked at a finite h
    (the identity is exact), by the finite difference of the error log6(.) at a small one, and against the same with the pe term
    of the transport left out."""
    rng = np.random.default_rng(2300)
    for _ in range(20):
        M = P.exp6(rng.normal(size=6) * np.r_[0.3, 0.3, 0.3, 0.8, 0.8, 0.8])
        u = rng.normal(size=6)
        f = TR.transport(M[0], M[1], u)
        e0 = P.log6(*M)
        for h in (0.3, 1e-4):
            Mh = _compose(_compose(_inverse(P.exp6(h * f)), M), P.exp6(h * u))
            assert np.max(np.abs(Mh[0] - M[0])) < 1e-12 and np.max(np.abs(Mh[1] - M[1])) < 1e-12
        h = 1e-4
        de = (P.log6(*_compose(_compose(_inverse(P.exp6(h * f)), M), P.exp6(h * u))) - e0) / h
        assert np.max(np.abs(de)) < 1e-8, de
        f_bad = np.r_[M[0] @ u[:3], M[0] @ u[3:]]
        de_bad = (P.log6(*_compose(_compose(_inverse(P.exp6(h * f_bad)), M), P.exp6(h * u))) - e0) / h
        assert np.max(np.abs(de_bad)) > 1e-2, de_bad
    # the same through feedforward(): the actual frame ON the desired one (Re = I, pe = 0) moves with the desired frame's own twist
    X0, X1 = P.exp6(rng.normal(size=6)), P.exp6(rng.normal(size=6))
    x0, x1 = P.to12(*X0)[0], P.to12(*X1)[0]
    f = TR.feedforward(PT.TASK_POSE, X0[0], X0[1], x0, x1, 0.5)
    assert np.max(np.abs(f - P.log6(*_compose(_inverse(X0), X1)) / 0.5)) < 1e-12
    moved = _compose(X0, P.exp6(0.5 * f))
    assert np.max(np.abs(moved[0] - X1[0])) < 1e-12 and np.max(np.abs(moved[1] - X1[1])) < 1e-12
