"""numpy restatement of the pose layer (loik_amd/csrc/loik_pose.hpp) for the tests: forward kinematics over the model tables,
exp6 / log6 (Pinocchio's conventions: 6-vectors [linear; angular], twists in the local frame), the pose error, the configuration
integrator, and the pose loop on the CPU oracle: host-driven one instance at a time, and lock-step as the device runs it."""
import numpy as np

from loik_amd import workloads as W

J_RX, J_RY, J_RZ, J_PX, J_PY, J_PZ, J_RU, J_PU = 1, 2, 3, 4, 5, 6, 7, 8
J_FREEFLYER, J_SPHERICAL, J_TRANSLATION, J_SPHERICAL_ZYX, J_PLANAR = 9, 10, 11, 12, 13
J_RUBX, J_RUBY, J_RUBZ, J_COMPOSITE, J_RUBU = 14, 15, 16, 17, 18
J_HX, J_HY, J_HZ, J_HU = 19, 20, 21, 22


def skew(w):
    w = np.asarray(w, dtype=float)
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -w[..., 2], w[..., 1], -w[..., 0]
    K[..., 1, 0], K[..., 2, 0], K[..., 2, 1] = w[..., 2], -w[..., 1], w[..., 0]
    return K


def _axis_rot(a, c, s):
    """[B,3,3] rotation about the unit axis a by the angle with cosine c, sine s"""
    a = np.asarray(a, dtype=float)
    return (c[:, None, None] * np.eye(3)[None] + (1 - c)[:, None, None] * np.outer(a, a)[None]
            + s[:, None, None] * skew(a)[None])


def joint_motion(model, i, q):
    """M(q) of joint i of a model without composites, batched: (R [B,3,3], t [B,3])"""
    B = q.shape[0]
    jt, iq = int(model.jtype[i]), int(model.idx_q[i])
    R, t = np.broadcast_to(np.eye(3), (B, 3, 3)).copy(), np.zeros((B, 3))
    unit = lambda k: np.eye(3)[k]
    if jt in (J_RX, J_RY, J_RZ, J_RU, J_HX, J_HY, J_HZ, J_HU):
        a = np.asarray(model.axis[i], dtype=float) if jt in (J_RU, J_HU) else unit((jt - (J_RX if jt <= J_RZ else J_HX)) % 3)
        R = _axis_rot(a, np.cos(q[:, iq]), np.sin(q[:, iq]))
        if jt >= J_HX:
            t = (float(model.pitch[i]) * q[:, iq])[:, None] * a[None]
    elif jt in (J_PX, J_PY, J_PZ, J_PU):
        a = np.asarray(model.axis[i], dtype=float) if jt == J_PU else unit(jt - J_PX)
        t = q[:, iq:iq + 1] * a[None]
    elif jt in (J_RUBX, J_RUBY, J_RUBZ, J_RUBU):
        a = np.asarray(model.axis[i], dtype=float) if jt == J_RUBU else unit(jt - J_RUBX)
        R = _axis_rot(a, q[:, iq], q[:, iq + 1])
    elif jt == J_FREEFLYER:
        R, t = W.quat_rot(q[:, iq + 3:iq + 7]), q[:, iq:iq + 3].copy()
    elif jt == J_SPHERICAL:
        R = W.quat_rot(q[:, iq:iq + 4])
    elif jt == J_TRANSLATION:
        t = q[:, iq:iq + 3].copy()
    elif jt == J_SPHERICAL_ZYX:   # Rz(q0) Ry(q1) Rx(q2)
        ez, ey, ex = unit(2), unit(1), unit(0)
        R = (_axis_rot(ez, np.cos(q[:, iq]), np.sin(q[:, iq])) @ _axis_rot(ey, np.cos(q[:, iq + 1]), np.sin(q[:, iq + 1]))
             @ _axis_rot(ex, np.cos(q[:, iq + 2]), np.sin(q[:, iq + 2])))
    elif jt == J_PLANAR:          # (x, y, cos, sin)
        R = _axis_rot(unit(2), q[:, iq + 2], q[:, iq + 3])
        t[:, :2] = q[:, iq:iq + 2]
    else:
        raise ValueError("joint type %d" % jt)
    return R, t


def fk(model, q, link):
    """world placement oMi of `link` (the caller's joint id) for configurations q [B][nq]: (R [B,3,3], t [B,3])"""
    q = np.atleast_2d(np.asarray(q, dtype=float))
    if getattr(model, "composite", None):
        ch = getattr(model, "_chain_cache", None)
        if ch is None:
            ch = model._chain_cache = W._Chain(model)
        return fk(ch, q, ch.link_of[int(link)])
    B = q.shape[0]
    path, i = [], int(link)
    while i > 0:
        path.append(i)
        i = int(model.parents[i])
    R, t = np.broadcast_to(np.eye(3), (B, 3, 3)).copy(), np.zeros((B, 3))
    for i in reversed(path):
        P = np.asarray(model.placement[i], dtype=float)
        Rp, tp = P[:9].reshape(3, 3), P[9:]
        Rj, tj = joint_motion(model, i, q)
        Rl, tl = Rp[None] @ Rj, tp[None] + tj @ Rp.T            # liMi = jointPlacement * M(q)
        t = t + np.einsum("bij,bj->bi", R, tl)
        R = R @ Rl
    return R, t


def fk12(model, q, links):
    """[B][n][12] placements (R row-major, t) of `links`"""
    out = []
    for l in links:
        R, t = fk(model, q, l)
        out.append(np.concatenate([R.reshape(-1, 9), t], axis=1))
    return np.stack(out, axis=1)


def to12(R, t):
    return np.concatenate([np.asarray(R).reshape(-1, 9), np.asarray(t).reshape(-1, 3)], axis=1)


def exp3(w):
    w = np.asarray(w, dtype=float)
    th = np.linalg.norm(w)
    K = skew(w)
    t2 = th * th
    if th < 1e-2:
        a, b = 1 - t2 / 6 + t2 * t2 / 120, 0.5 - t2 / 24 + t2 * t2 / 720
    else:
        a, b = np.sin(th) / th, (1 - np.cos(th)) / th ** 2
    return np.eye(3) + a * K + b * K @ K


def exp6(nu):
    """pinocchio::exp6 of one twist [v; w]: (R, p)"""
    nu = np.asarray(nu, dtype=float)
    v, w = nu[:3], nu[3:]
    th = np.linalg.norm(w)
    K = skew(w)
    t2 = th * th
    if th < 1e-2:
        b, c = 0.5 - t2 / 24 + t2 * t2 / 720, 1.0 / 6 - t2 / 120 + t2 * t2 / 5040
    else:
        b, c = (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    return exp3(w), (np.eye(3) + b * K + c * K @ K) @ v


def log3(R):
    """pinocchio::log3 with the branches of loik_pose.hpp's pose_log3 (series for theta -> 0, the symmetric part for theta -> pi)"""
    R = np.asarray(R, dtype=float)
    vee = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = 0.5 * np.sqrt(vee @ vee)
    c = 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, c)
    if c < -0.8:
        k = int(np.argmax(np.diag(R)))
        omc = 1.0 - c
        a = np.empty(3)
        a[k] = np.sqrt(max(0.0, (R[k, k] - c) / omc))
        for j in range(3):
            if j != k:
                a[j] = 0.5 * (R[k, j] + R[j, k]) / (omc * a[k])
        return (-th if a @ vee < 0 else th) * a
    t2 = th * th
    f = 0.5 * (1 + t2 / 6 + 7 * t2 * t2 / 360) if th < 1e-4 else 0.5 * th / s
    return f * vee


def log6(R, p):
    """pinocchio::log6 of (R, p): [v; w]"""
    w = log3(R)
    t2 = w @ w
    th = np.sqrt(t2)
    if th < 1e-3:
        beta = 1.0 / 12 + t2 / 720 + t2 * t2 / 30240
    else:
        beta = (1 - 0.5 * th * np.cos(0.5 * th) / np.sin(0.5 * th)) / t2
    p = np.asarray(p, dtype=float)
    wp = np.cross(w, p)
    return np.concatenate([p - 0.5 * wp + beta * np.cross(w, wp), w])


def pose_error(R, t, target12):
    """e = log6(oMi^-1 oMdes) for one placement (R, t) and a target [12]"""
    D = np.asarray(target12, dtype=float)
    Rd, td = D[:9].reshape(3, 3), D[9:]
    return log6(R.T @ Rd, R.T @ (td - t))


def pose_errors(model, q, links, targets):
    """[B][nc][6] errors of configurations q [B][nq] against targets [B][nc][12]"""
    B = q.shape[0]
    e = np.empty((B, len(links), 6))
    for c, l in enumerate(links):
        R, t = fk(model, q, l)
        for b in range(B):
            e[b, c] = pose_error(R[b], t[b], targets[b, c])
    return e


def host_pose_loop(model, prm, q0, H_ref, v_ref, links, A, lb, ub, targets, dt, gain, tol, max_steps, integrate):
    """the pose loop driven from the host on the CPU oracle, one instance at a time: numpy FK and log6 -> b_c = A_c (gain / dt) e_c ->
    UpdateEqConstraint -> tailored Solve (warm_start) -> integrate.  A: [nc][6][6] shared.  Returns (q, steps, reached)."""
    from oracle import ref
    B, nc = q0.shape[0], len(links)
    q = q0.copy()
    steps = np.zeros(B, dtype=np.int32)
    reached = np.zeros(B, dtype=bool)
    k = gain / dt
    for b in range(B):
        r = ref.RefSolver(model, **dict(prm, warm_start=True))
        r.SolveInit(q[b], H_ref, v_ref, np.asarray(links, dtype=np.int32), A, np.zeros((nc, 6)), lb, ub)
        for step in range(max_steps + 1):
            e = pose_errors(model, q[b:b + 1], links, targets[b:b + 1])[0]
            if np.max(np.abs(e)) <= tol:
                reached[b] = True
                break
            if step == max_steps:
                break
            for c, l in enumerate(links):
                r.UpdateEqConstraint(l, A[c] @ (k * e[c]))
            r.Solve(q[b], -1, None, None)
            q[b] = integrate(model, q[b], dt * r.field("z"))
            steps[b] += 1
    return q, steps, reached


POSE_REACHED, POSE_NOT_CONVERGED, POSE_INFEASIBLE, POSE_STOPPED = 1, 2, 4, 8


def integrate(model, q, v):
    """pinocchio::integrate of one configuration for every joint the device integrates (k_advance_q): the free-flyer, spherical and
    translation joints as test_multidof._np_integrate has them, the planar joint on SE(2), the (cos, sin) joints on SO(2), plain
    sums for the others (ZYX angles, prismatic, revolute, helical); a composite integrates sub-joint by sub-joint"""
    from test_multidof import _np_integrate
    if getattr(model, "composite", None):
        return integrate(W._Chain(model), q, v)
    out = _np_integrate(model, q, v)
    for i in range(1, model.njoints):
        jt, iq, iv = int(model.jtype[i]), int(model.idx_q[i]), int(model.idx_v[i])
        if jt == J_SPHERICAL_ZYX:
            out[iq:iq + 3] = q[iq:iq + 3] + v[iv:iv + 3]
        elif jt == J_PLANAR:
            vx, vy, w = v[iv:iv + 3]
            c0, s0 = q[iq + 2], q[iq + 3]
            sw, cw = np.sin(w), np.cos(w)
            # sin(w) / w and (1 - cos(w)) / w = sin(w / 2) sinc(w / 2): no quotient of rounded differences, exact at w = 0
            a, b = np.sinc(w / np.pi), np.sin(0.5 * w) * np.sinc(0.5 * w / np.pi)
            tx, ty = a * vx - b * vy, b * vx + a * vy
            out[iq], out[iq + 1] = q[iq] + c0 * tx - s0 * ty, q[iq + 1] + s0 * tx + c0 * ty
            c1, s1 = c0 * cw - s0 * sw, s0 * cw + c0 * sw
            n = 0.5 * (3 - (c1 * c1 + s1 * s1))
            out[iq + 2], out[iq + 3] = c1 * n, s1 * n
        elif jt in (J_RUBX, J_RUBY, J_RUBZ, J_RUBU):
            c0, s0, w = q[iq], q[iq + 1], v[iv]
            c1, s1 = c0 * np.cos(w) - s0 * np.sin(w), s0 * np.cos(w) + c0 * np.sin(w)
            n = 0.5 * (3 - (c1 * c1 + s1 * s1))
            out[iq], out[iq + 1] = c1 * n, s1 * n
    return out


def lockstep_pose_loop(model, prm, q0, H_ref, v_ref, links, A, lb, ub, targets, dt, gain, tol, max_steps, integrate=integrate):
    """the pose loop as the device runs it, step-major on the CPU oracle: each step computes the errors of every instance and marks
    it reached (max_c |e_c|_inf <= tol) or stopped (e or q not finite); the loop ends at max_steps or when none is running; otherwise
    EVERY instance runs the tailored Solve (warm_start as prm says), with b_c = A_c (gain / dt) e_c when running and b = 0 when not,
    and only the running ones integrate q <- q (+) dt z and take the inner solve's outcome into their status.
    A: [nc][6][6] shared or [B][nc][6][6] per instance; targets [B][nc][12].  Instances are independent but for the number of solves,
    which is the batch's: run the oracle on the whole batch for `z` / `iter`.
    Returns dict(q, steps, status (POSE_* bits), reached, err [B][nc][6] (of the last re-target each instance took part in),
    z [B][nv], iter [B] (the oracle's after its last inner solve; 0 / zeros when there was none))."""
    from oracle import ref
    B, nc = q0.shape[0], len(links)
    A = np.asarray(A, dtype=float)
    A_of = (lambda b: A[b]) if A.ndim == 4 else (lambda b: A)
    k = gain / dt
    q = np.array(q0, dtype=float)
    steps = np.zeros(B, dtype=np.int32)
    status = np.zeros(B, dtype=np.int32)
    err = np.zeros((B, nc, 6))
    z = np.zeros((B, model.nv))
    it = np.zeros(B, dtype=np.int32)
    solvers, end = [], np.zeros(B, dtype=np.int32)
    for b in range(B):   # each instance until it leaves the loop: the retarget at which it is reached / stopped, or max_steps
        r = ref.RefSolver(model, **dict(prm, num_eq_c=nc))
        r.SolveInit(q[b], H_ref, v_ref, np.asarray(links, dtype=np.int32), A_of(b), np.zeros((nc, 6)), lb, ub)
        solvers.append(r)
        for step in range(max_steps + 1):
            end[b] = step
            with np.errstate(all="ignore"):
                e = pose_errors(model, q[b:b + 1], links, targets[b:b + 1])[0]
            err[b] = e
            if not (np.all(np.isfinite(e)) and np.all(np.isfinite(q[b]))):
                status[b] |= POSE_STOPPED
                break
            if np.max(np.abs(e)) <= tol:
                status[b] |= POSE_REACHED
                break
            if step == max_steps:
                break
            for c, l in enumerate(links):
                r.UpdateEqConstraint(l, A_of(b)[c] @ (k * e[c]))
            r.Solve(q[b], -1, None, None)
            if not r.get_convergence_status():
                status[b] |= POSE_NOT_CONVERGED
            if r.get_primal_infeasibility_status():
                status[b] |= POSE_INFEASIBLE
            q[b] = integrate(model, q[b], dt * r.field("z"))
            steps[b] += 1
    n_solves = int(end.max()) if B else 0   # the step at which none is running any more (or max_steps)
    for b in range(B):   # the idle b = 0 solves at the final q of the instances that left the loop before the batch did
        r = solvers[b]
        if end[b] < n_solves and not status[b] & POSE_STOPPED:
            for l in links:
                r.UpdateEqConstraint(l, np.zeros(6))
            for _ in range(n_solves - end[b]):
                r.Solve(q[b], -1, None, None)
        if n_solves > 0 and not status[b] & POSE_STOPPED:
            z[b], it[b] = r.field("z"), r.get_iter()
    return dict(q=q, steps=steps, status=status, reached=(status & POSE_REACHED) != 0, err=err, z=z, iter=it)
