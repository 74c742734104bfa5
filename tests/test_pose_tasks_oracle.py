"""CPU: the lock-step oracle with tool frames and task kinds (tests/pose_tasks_numpy.py) is proven before it referees the device.
With every kind POSE and identity frames it IS pose_numpy.lockstep_pose_loop with A = I -- np.array_equal, no tolerance; the
motion transform X^-1 it puts into A is checked against a finite difference of the numpy FK; and the masked formulation converges:
A_c = S_c X_c^-1 has three zero rows for a position or an orientation task, which the ADMM takes in its stride."""
import numpy as np
import pytest

import loik_amd

from test_pose_ik import PRM, _fk_models, _links
from test_pose_parity import _box, _leaf_and_multidof, _seeds
import pose_numpy as P
import pose_tasks_numpy as T

KINDS = {"pose": T.TASK_POSE, "position": T.TASK_POSITION, "orientation": T.TASK_ORIENTATION}


def task_seeds(model, B, links, frames, seed, spread=(1e-4, 0.15)):
    """test_pose_parity._seeds with the targets taken at the task frames: (q0, targets [B][nc][12], q_t)"""
    q0, _ = _seeds(model, B, links, seed, spread=spread)
    q_t = model.random_configurations(np.random.default_rng(seed), B)   # (the configurations _seeds drew its targets from)
    return q0, T.frame_fk12(model, q_t, links, frames), q_t


def _model(name):
    if name == "multidof":
        model = _fk_models()[3]
        return model, _leaf_and_multidof(model)
    model = loik_amd.builtin_model(name)
    return model, _links(model, 2)


@pytest.mark.parametrize("tol_rel", [0.0, 1e-3])
@pytest.mark.parametrize("max_steps", [1, 4])
@pytest.mark.parametrize("name", ["talos32", "panda7", "multidof"])
def test_pose_kind_with_identity_frames_reproduces_the_plain_lockstep_oracle(name, max_steps, tol_rel):
    model, links = _model(name)
    B, nc = 16, len(links)
    prm = dict(PRM, tol_rel=tol_rel)
    q0, tg = _seeds(model, B, links, seed=1210 + nc)
    lb, ub = _box(model)
    A = np.tile(np.eye(6), (nc, 1, 1))
    for dt, gain in ((0.25, 0.5), (2.0, 1.7)):
        want = P.lockstep_pose_loop(model, prm, q0, np.eye(6), np.zeros(6), links, A, lb, ub, tg, dt, gain, 1e-4, max_steps)
        for frames in (None, np.tile(T.IDENTITY12, (nc, 1))):
            got = T.lockstep_pose_loop_tasks(model, prm, q0, np.eye(6), np.zeros(6), links, [T.TASK_POSE] * nc, frames, lb, ub, tg, dt,
                                             gain, 1e-4, max_steps)
            assert set(got) == set(want)
            for key in want:
                assert np.array_equal(got[key], want[key]), (name, max_steps, tol_rel, dt, key)
        if max_steps == 4:   # (the case means something: instances leave the loop at different steps)
            assert len(set(want["steps"].tolist())) > 1


def test_task_matrices_are_masked_motion_transforms():
    rng = np.random.default_rng(3)
    F = T.random_frames(rng, 3)
    A = T.task_matrices([T.TASK_POSE, T.TASK_POSITION, T.TASK_ORIENTATION], F)
    Rf, pf = F[0, :9].reshape(3, 3), F[0, 9:]
    v, w = rng.normal(size=3), rng.normal(size=3)
    # the velocity of the frame origin, in frame axes: Rf^T (v + w x pf), Rf^T w
    assert np.allclose(A[0] @ np.r_[v, w], np.r_[Rf.T @ (v + np.cross(w, pf)), Rf.T @ w], rtol=0, atol=1e-15)
    assert np.array_equal(A[1][:3], T.x_inv(F[1])[:3]) and not A[1][3:].any()
    assert np.array_equal(A[2][3:], T.x_inv(F[2])[3:]) and not A[2][:3].any()
    assert np.linalg.matrix_rank(A[0]) == 6 and np.linalg.matrix_rank(A[1]) == 3 and np.linalg.matrix_rank(A[2]) == 3
    assert np.array_equal(T.task_matrices([T.TASK_POSE], [T.IDENTITY12])[0], np.eye(6))


@pytest.mark.parametrize("name", ["talos32", "panda7", "multidof"])
def test_x_inv_against_a_finite_difference_of_the_numpy_fk(name):
    """move q by a small dq: the body twist of the task frame, log6(oMf(q)^-1 oMf(q + dq)), is X^-1 applied to the link's,
    log6(oMi(q)^-1 oMi(q + dq)).  Both are O(h); the identity holds to O(h^2) (log6 is the exact twist of the displacement only to
    first order in a moving frame): h = 1e-5 leaves 1e-10 against twists of 1e-5 -- a dropped -Rf^T [pf]x block is |pf| h = 1e-6."""
    model, links = _model(name)
    rng = np.random.default_rng(17)
    B, h = 8, 1e-5
    q = model.random_configurations(rng, B)
    frames = T.random_frames(rng, len(links))
    for c, l in enumerate(links):
        X = T.x_inv(frames[c])
        seen = 0.0
        for b in range(B):
            q1 = P.integrate(model, q[b], h * rng.normal(size=model.nv))[None]
            (R0, t0), (R1, t1) = P.fk(model, q[b:b + 1], l), P.fk(model, q1, l)
            (S0, s0), (S1, s1) = T.frame_fk(model, q[b:b + 1], l, frames[c]), T.frame_fk(model, q1, l, frames[c])
            nu_i = P.log6(R0[0].T @ R1[0], R0[0].T @ (t1[0] - t0[0]))
            nu_f = P.log6(S0[0].T @ S1[0], S0[0].T @ (s1[0] - s0[0]))
            assert np.max(np.abs(nu_f - X @ nu_i)) < 1e-9, (name, l, b, np.max(np.abs(nu_f - X @ nu_i)))
            Xd = X.copy()
            Xd[:3, 3:] = 0.0   # (the check can tell: without the lever-arm block the two differ by |pf| |w|)
            seen = max(seen, np.max(np.abs(nu_f - Xd @ nu_i)))
        assert seen > 1e-7, (name, l, seen)


@pytest.mark.parametrize("kind", ["pose", "position", "orientation"])
@pytest.mark.parametrize("name", ["talos32", "panda7"])
def test_masked_tasks_converge_on_the_oracle(name, kind):
    """24 seeds, one constraint, a rotated and translated frame (|pf| = 0.15), tolerance 1e-6, box +-2, test_pose_ik.PRM, dt = gain =
    1: every instance of the masked kinds reaches within 10 steps (the zero rows of A are nothing the ADMM minds); the full pose
    takes more steps.  The final q of the reached instances is then checked from first principles."""
    model = loik_amd.builtin_model(name)
    links = _links(model, 1)
    B, tol = 24, 1e-6
    frames = T.random_frames(np.random.default_rng(41), 1, offset=(0.15, 0.15))
    assert abs(np.linalg.norm(frames[0, 9:]) - 0.15) < 1e-12 and np.max(np.abs(frames[0, :9] - np.eye(3).ravel())) > 0.1
    q0, tg, _ = task_seeds(model, B, links, frames, seed=1240)
    lb, ub = _box(model)
    kinds = [KINDS[kind]]
    max_steps = 10 if kind != "pose" else 40
    o = T.lockstep_pose_loop_tasks(model, PRM, q0, np.eye(6), np.zeros(6), links, kinds, frames, lb, ub, tg, 1.0, 1.0, tol, max_steps)
    print("%s %s: reached %d/%d, steps max %d, inner solves not converged on %d instances"
          % (name, kind, o["reached"].sum(), B, o["steps"].max(), ((o["status"] & P.POSE_NOT_CONVERGED) != 0).sum()))
    if kind != "pose":
        assert o["reached"].all(), (name, kind, o["reached"].mean(), o["steps"])
    else:   # (the plain loop's own behaviour, not this interface's: a 6-D task on a 7-DoF arm stalls on a seed now and then; the
        #    share test_pose_ik.test_pose_end_to_end_many_seeds asks of it)
        assert o["reached"].mean() > 0.5, (name, o["reached"].mean(), o["steps"])
    assert o["steps"].max() >= 1
    r = o["reached"]
    e = T.task_errors(model, o["q"], links, kinds, frames, tg)
    assert np.max(np.abs(e[r])) <= tol
    m = T.mask(kinds[0]).astype(bool)
    assert not e[..., ~m].any() and not o["err"][..., ~m].any()


def test_infinite_joint_limits_reproduce_the_oracle_without_limits():
    """the combination with pose_limits_numpy's box rule (SolveInit per step, the running-maximum b): with every limit infinite it is
    the loop without limits, np.array_equal"""
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 2)
    B = 16
    kinds = [T.TASK_POSITION, T.TASK_ORIENTATION]
    frames = T.random_frames(np.random.default_rng(51), 2)
    q0, tg, _ = task_seeds(model, B, links, frames, seed=1250)
    lb, ub = _box(model)
    inf = np.inf * np.ones(model.nv)
    for tol_rel in (0.0, 1e-3):
        prm = dict(PRM, tol_rel=tol_rel)
        want = T.lockstep_pose_loop_tasks(model, prm, q0, np.eye(6), np.zeros(6), links, kinds, frames, lb, ub, tg, 0.25, 0.5, 1e-4, 4)
        got = T.lockstep_pose_loop_tasks(model, prm, q0, np.eye(6), np.zeros(6), links, kinds, frames, lb, ub, tg, 0.25, 0.5, 1e-4, 4,
                                         q_lo=-inf, q_hi=inf)
        for key in want:
            assert np.array_equal(got[key], want[key]), (tol_rel, key)
        assert not got["limit_flags"].any() and len(set(want["steps"].tolist())) > 1
