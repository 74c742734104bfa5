"""The numpy restatement of the axis-symmetric task kinds (include/loik_amd_axis.h) beside pose_tasks_numpy: the rotation about the
task frame's z axis is free.  Notation as there: (Re, pe) = oMf^-1 oMdes, d = the third column of Re (the desired z axis seen from
the task frame);

    w_axis(Re):  s = sqrt(d_x^2 + d_y^2), theta = atan2(s, d_z)
                 s == 0:  (pi, 0, 0) if d_z < 0 else (0, 0, 0)
                 else:    (theta / s) (-d_y, d_x, 0)
    pose_axis    e = [pe; w_axis(Re)]      S = diag(1,1,1,1,1,0)
    axis         e = [0;  w_axis(Re)]      S = diag(0,0,0,1,1,0)

The lock-step loop is pose_tasks_numpy.lockstep_pose_loop_tasks itself: `installed()` puts this module's error and masks into that
module for the duration of a call and restores it afterwards, so the three older kinds run what they always ran."""
import contextlib

import numpy as np

import pose_numpy as P
import pose_tasks_numpy as T

TASK_FREE_Z = 4
TASK_POSE_AXIS, TASK_AXIS = T.TASK_POSE | TASK_FREE_Z, T.TASK_ORIENTATION | TASK_FREE_Z
KINDS = {"pose": T.TASK_POSE, "position": T.TASK_POSITION, "orientation": T.TASK_ORIENTATION, "pose_axis": TASK_POSE_AXIS, "axis": TASK_AXIS}
_AXIS_MASK = {TASK_POSE_AXIS: np.array([1.0, 1, 1, 1, 1, 0]), TASK_AXIS: np.array([0.0, 0, 0, 1, 1, 0])}


def w_axis(Re):
    """the minimal rotation, in frame axes, that carries the frame's z axis onto d = Re[:, 2]; w_z is 0 identically"""
    Re = np.asarray(Re, dtype=float)
    dx, dy, dz = Re[0, 2], Re[1, 2], Re[2, 2]
    s = np.sqrt(dx * dx + dy * dy)
    if not (np.isfinite(s) and np.isfinite(dz)):
        return np.array([np.nan, np.nan, 0.0])
    if s == 0.0:
        return np.array([np.pi if dz < 0 else 0.0, 0.0, 0.0])
    f = np.arctan2(s, dz) / s
    return np.array([-(f * dy), f * dx, 0.0])


def mask(kind):
    """the diagonal of S for any of the five kinds"""
    kind = int(kind)
    return _AXIS_MASK[kind].copy() if kind in _AXIS_MASK else T.mask(kind)


_tasks_task_error = T.task_error


def task_error(Rw, tw, target12, kind):
    """pose_tasks_numpy.task_error with the two axis kinds"""
    kind = int(kind)
    if kind not in _AXIS_MASK:
        return _tasks_task_error(Rw, tw, target12, kind)
    D = np.asarray(target12, dtype=float)
    Rd, td = D[:9].reshape(3, 3), D[9:]
    w = w_axis(Rw.T @ Rd)
    return np.r_[Rw.T @ (td - tw) if kind == TASK_POSE_AXIS else np.zeros(3), w]


@contextlib.contextmanager
def installed():
    """pose_tasks_numpy knows the axis kinds while this is open: its task_error is this module's, its mask table has their rows"""
    saved = T.task_error
    T.task_error = task_error
    T._MASK.update(_AXIS_MASK)
    try:
        yield
    finally:
        T.task_error = saved
        for k in _AXIS_MASK:
            T._MASK.pop(k, None)


def task_matrices(kinds, frames):
    """[nc][6][6]: A_c = S_c X_c^-1"""
    with installed():
        return T.task_matrices(kinds, frames)


def task_errors(model, q, links, kinds, frames, targets):
    """[B][nc][6] masked task-frame errors, any of the five kinds"""
    with installed(), np.errstate(invalid="ignore"):
        return T.task_errors(model, q, links, kinds, frames, targets)


def lockstep_pose_loop_axis(*args, **kw):
    """pose_tasks_numpy.lockstep_pose_loop_tasks, same arguments, with the axis kinds known"""
    with installed():
        return T.lockstep_pose_loop_tasks(*args, **kw)


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def spin_targets(rng, targets, flip=False):
    """targets [..., 12] with every rotation spun about its own z axis by an angle from U(-pi, pi) (returned too, same leading
    shape); flip: turned upside down first, R diag(1, -1, -1), so the z axis points the other way"""
    tg = np.array(targets, dtype=float)
    flat = tg.reshape(-1, 12)
    ang = rng.uniform(-np.pi, np.pi, size=flat.shape[0])
    F = np.diag([1.0, -1.0, -1.0]) if flip else np.eye(3)
    for i in range(flat.shape[0]):
        flat[i, :9] = (flat[i, :9].reshape(3, 3) @ F @ rot_z(ang[i])).ravel()
    return tg, ang.reshape(tg.shape[:-1])


def feedforward(kind, R, t, X0, X1, dt):
    """the feed-forward of loik_amd_track.h for the axis kinds, the difference rule in the actual frame (R, t):
    f_w = (w_axis(R^T R1) - w_axis(R^T R0)) / dt, f_v = R^T (t1 - t0) / dt for pose_axis and 0 for axis"""
    X0, X1 = np.asarray(X0, dtype=float), np.asarray(X1, dtype=float)
    fw = (w_axis(R.T @ X1[:9].reshape(3, 3)) - w_axis(R.T @ X0[:9].reshape(3, 3))) / dt
    fv = R.T @ (X1[9:] - X0[9:]) / dt if int(kind) == TASK_POSE_AXIS else np.zeros(3)
    return np.r_[fv, fw]


def lockstep_pose_loop_axis_accel(model, prm, q0, H_ref, v_ref, links, kinds, lb, ub, targets, dt, gain, tol, max_steps, q_lo, q_hi, a_max):
    """pose_accel_numpy.lockstep_pose_loop_accel (position and acceleration limits) with task kinds in the JOINT frame (identity
    iMf): there A_c = S_c is a diagonal of ones and zeros, so that function's b_c = A_c (k e_c) is the task law's k S_c e_c to the
    bit, and its error is this module's for the duration of the call"""
    import pose_accel_numpy as PA
    nc = len(links)
    frames = np.tile(T.IDENTITY12, (nc, 1))
    A = task_matrices(kinds, frames)
    saved = P.pose_errors
    P.pose_errors = lambda m, q, l, tg: task_errors(m, q, l, kinds, frames, tg)
    try:
        return PA.lockstep_pose_loop_accel(model, prm, q0, H_ref, v_ref, links, A, lb, ub, targets, dt, gain, tol, max_steps, q_lo, q_hi, a_max)
    finally:
        P.pose_errors = saved
