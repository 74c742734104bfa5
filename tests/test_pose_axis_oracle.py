"""CPU: the numpy restatement of the axis-symmetric task kinds (tests/pose_axis_numpy.py, include/loik_amd_axis.h) is proven before
it referees the device: w_axis is the rotation it claims to be, it does not see a spin of the target about its own z, its two
exact cases and its behaviour next to pi; the constraint matrices are the masked motion transforms; and the lock-step loop with the
two kinds converges where the full pose, asked to match an arbitrary spin, does not."""
import numpy as np
import pytest

import loik_amd

from test_pose_ik import PRM, _links
from test_pose_parity import _box
from test_pose_tasks_oracle import task_seeds
import pose_numpy as P
import pose_tasks_numpy as T
import pose_axis_numpy as AX

Z = np.array([0.0, 0.0, 1.0])


def _random_rotations(rng, n):
    out = []
    for _ in range(n):
        a = rng.normal(size=3)
        out.append(P.exp3(rng.uniform(0.0, np.pi) * a / np.linalg.norm(a)))
    return out


def test_w_axis_rotates_z_onto_d_and_has_no_z_component():
    worst = 0.0
    for Re in _random_rotations(np.random.default_rng(5), 500):
        w = AX.w_axis(Re)
        assert w[2] == 0.0
        worst = max(worst, np.max(np.abs(P.exp3(w) @ Z - Re[:, 2])))
        assert np.linalg.norm(w) <= np.pi
    print("w_axis: max |exp3(w) z - d| = %.3e" % worst)
    assert worst < 1e-14


def test_w_axis_does_not_see_a_spin_of_the_target():
    """w_axis(Re Rz(a)) == w_axis(Re): Rz leaves the third column of the product alone, entry for entry"""
    rng = np.random.default_rng(6)
    worst = 0.0
    for Re in _random_rotations(rng, 300):
        a = rng.uniform(-np.pi, np.pi)
        worst = max(worst, np.max(np.abs(AX.w_axis(Re @ AX.rot_z(a)) - AX.w_axis(Re))))
    print("w_axis: max change under a spin of the target = %.3e" % worst)
    assert worst <= 1e-15


def test_exactly_parallel_and_antiparallel():
    assert np.array_equal(AX.w_axis(np.eye(3)), np.zeros(3))
    assert np.array_equal(AX.w_axis(AX.rot_z(0.7)), np.zeros(3))
    assert np.array_equal(AX.w_axis(np.diag([1.0, -1.0, -1.0])), np.array([np.pi, 0.0, 0.0]))
    assert np.array_equal(AX.w_axis(np.diag([-1.0, 1.0, -1.0])), np.array([np.pi, 0.0, 0.0]))
    bad = np.eye(3)
    bad[2, 2] = np.nan
    assert not np.all(np.isfinite(AX.w_axis(bad)))
    bad = np.eye(3)
    bad[0, 2] = np.inf
    assert not np.all(np.isfinite(AX.w_axis(bad)))


def test_norm_next_to_pi():
    """|w_axis(exp3((0, pi - eps, 0)))| = pi - eps with no loss next to pi, where a formula through asin or acos of one entry would
    lose half the digits.  The bound is four ulps of pi (4.44e-16 each): exp3's sine and cosine, the atan2, the division by s and the
    norm each round once."""
    for k in range(3, 13):
        eps = 10.0 ** -k
        w = AX.w_axis(P.exp3(np.array([0.0, np.pi - eps, 0.0])))
        diff = abs(np.linalg.norm(w) - (np.pi - eps))
        print("w_axis next to pi: eps %.0e, | |w| - (pi - eps) | = %.3e" % (eps, diff))
        assert diff <= 4 * np.spacing(np.pi), (eps, diff)
        assert w[2] == 0.0 and abs(w[0]) < 1e-15 and w[1] > 0


def test_task_matrices_have_rank_five_and_two():
    F = T.random_frames(np.random.default_rng(3), 2)
    A = AX.task_matrices([AX.TASK_POSE_AXIS, AX.TASK_AXIS], F)
    assert np.linalg.matrix_rank(A[0]) == 5 and np.linalg.matrix_rank(A[1]) == 2
    assert np.array_equal(A[0][:5], T.x_inv(F[0])[:5]) and not A[0][5].any()
    assert np.array_equal(A[1][3:5], T.x_inv(F[1])[3:5]) and not A[1][:3].any() and not A[1][5].any()
    assert np.array_equal(AX.mask(AX.TASK_POSE_AXIS), [1, 1, 1, 1, 1, 0]) and np.array_equal(AX.mask(AX.TASK_AXIS), [0, 0, 0, 1, 1, 0])
    # the older kinds are pose_tasks_numpy's, and that module is as it was once a call is over
    assert np.array_equal(AX.task_matrices([T.TASK_POSE, T.TASK_POSITION], F), T.task_matrices([T.TASK_POSE, T.TASK_POSITION], F))
    assert sorted(T._MASK) == [0, 1, 2] and T.task_error is AX._tasks_task_error


def test_errors_of_the_older_kinds_are_unchanged_and_err_5_is_zero():
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 1)
    frames = T.random_frames(np.random.default_rng(8), 1)
    q0, tg, _ = task_seeds(model, 8, links, frames, seed=9)
    for kind in (T.TASK_POSE, T.TASK_POSITION, T.TASK_ORIENTATION):
        assert np.array_equal(AX.task_errors(model, q0, links, [kind], frames, tg), T.task_errors(model, q0, links, [kind], frames, tg))
    e5 = AX.task_errors(model, q0, links, [AX.TASK_POSE_AXIS], frames, tg)
    e2 = AX.task_errors(model, q0, links, [AX.TASK_AXIS], frames, tg)
    assert np.array_equal(e5[..., :3], T.task_errors(model, q0, links, [T.TASK_POSITION], frames, tg)[..., :3])
    assert np.array_equal(e5[..., 3:], e2[..., 3:]) and not e2[..., :3].any() and not e5[..., 5].any()
    assert np.abs(e2[..., 3:5]).min() > 0


# ---- convergence: the set-up of tests/test_pose_tasks_oracle.test_masked_tasks_converge_on_the_oracle, the targets spun about their z
def _spun_setup(name):
    model = loik_amd.builtin_model(name)
    links = _links(model, 1)
    frames = T.random_frames(np.random.default_rng(41), 1, offset=(0.15, 0.15))
    q0, tg, _ = task_seeds(model, 24, links, frames, seed=1240)
    tg, _ = AX.spin_targets(np.random.default_rng(1241), tg)
    return model, links, frames, q0, tg


@pytest.mark.parametrize("kind", ["pose_axis", "axis"])
@pytest.mark.parametrize("name", ["talos32", "panda7"])
def test_axis_tasks_converge_on_spun_targets(name, kind):
    model, links, frames, q0, tg = _spun_setup(name)
    lb, ub = _box(model)
    tol, kinds = 1e-6, [AX.KINDS[kind]]
    o = AX.lockstep_pose_loop_axis(model, PRM, q0, np.eye(6), np.zeros(6), links, kinds, frames, lb, ub, tg, 1.0, 1.0, tol, 20)
    print("%s %s: reached %d/24, steps max %d" % (name, kind, o["reached"].sum(), o["steps"].max()))
    need = 22 if (name, kind) == ("panda7", "pose_axis") else 24   # (a 5-D task on a 7-DoF arm stalls on a seed, as the pose test tolerates)
    assert o["reached"].sum() >= need, (name, kind, o["reached"].sum(), o["steps"])
    r = o["reached"]
    e = AX.task_errors(model, o["q"], links, kinds, frames, tg)
    assert np.max(np.abs(e[r])) <= tol and o["steps"].max() >= 1
    m = AX.mask(kinds[0]).astype(bool)
    assert not e[..., ~m].any() and not o["err"][..., ~m].any() and not o["err"][..., 5].any()


def test_axis_converges_from_upside_down():
    """targets flipped as well: the start error is up to 3.13 rad, right next to the antiparallel rule"""
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 1)
    B, tol = 256, 1e-6
    frames = T.random_frames(np.random.default_rng(2300), 1)
    q0, tg, _ = task_seeds(model, B, links, frames, seed=2301, spread=(3e-2, 0.6))
    tg, _ = AX.spin_targets(np.random.default_rng(2302), tg, flip=True)
    lb, ub = _box(model)
    e0 = AX.task_errors(model, q0, links, [AX.TASK_AXIS], frames, tg)
    o = AX.lockstep_pose_loop_axis(model, PRM, q0, np.eye(6), np.zeros(6), links, [AX.TASK_AXIS], frames, lb, ub, tg, 1.0, 1.0, tol, 20)
    print("flipped axis: start error up to %.4f rad, reached %d/%d, steps max %d"
          % (np.linalg.norm(e0[:, 0, 3:], axis=1).max(), o["reached"].sum(), B, o["steps"].max()))
    assert np.linalg.norm(e0[:, 0, 3:], axis=1).max() > 3.0
    assert o["reached"].all(), (o["reached"].sum(), o["steps"].max())
    assert not o["err"][..., 5].any() and not o["err"][..., :3].any()


def test_feedforward_difference_rule_lands_on_the_next_sample():
    """the feed-forward of loik_amd_track.h for the axis kinds: with gain = 1, dt f + e against X_0 is the error against X_1"""
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 1)
    frames = T.random_frames(np.random.default_rng(61), 1)
    q0, x0, _ = task_seeds(model, 16, links, frames, seed=62)
    _, x1, _ = task_seeds(model, 16, links, frames, seed=63)
    x0, _ = AX.spin_targets(np.random.default_rng(64), x0)
    x1, _ = AX.spin_targets(np.random.default_rng(65), x1)
    R, t = T.frame_fk(model, q0, links[0], frames[0])
    for kind in (AX.TASK_POSE_AXIS, AX.TASK_AXIS):
        for b in range(16):
            f = AX.feedforward(kind, R[b], t[b], x0[b, 0], x1[b, 0], 0.25)
            e0, e1 = AX.task_error(R[b], t[b], x0[b, 0], kind), AX.task_error(R[b], t[b], x1[b, 0], kind)
            assert np.max(np.abs(0.25 * f + e0 - e1)) < 1e-14 and f[5] == 0.0
            assert kind == AX.TASK_POSE_AXIS or not f[:3].any()
