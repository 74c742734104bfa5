"""The lock-step CPU oracle of the pose loop TRACKING TIMED TRAJECTORIES (include/loik_amd_track.h), in the structure of
pose_numpy.lockstep_pose_loop: T + 1 samples X_0 .. X_T per instance, and for step k = 0 .. T - 1 a running instance does

    1. e against X_k (pose_numpy.pose_errors, or pose_tasks_numpy.task_errors with kinds / frames);
    2. e or q not finite                        -> STOPPED;
    3. errmax[b][k] = max |e|, ontrack counts it when <= tol;
    4. f = the feed-forward twist (feedforward below), 0 with ff = FF_NONE;
    5. b_c = A_c ((gain / dt) e_c + f_c), with tasks (gain / dt) e_c + f_c;
    6. the tailored Solve, q <- q (+) dt z (clamped with limits); z_traj[b][k] = z, q_traj[b][k + 1] = q, inner[b][k] = the bits.

The re-target after step T - 1 judges against X_T and runs nothing.  No instance is ever "reached", so no instance idles: the
loop is T steps for every instance that is not stopped.  The limits variant takes its box rule from pose_limits_numpy.step_box
and the tasks variant its error from pose_tasks_numpy.task_errors: nothing of either is restated."""
import numpy as np

import pose_numpy as P
import pose_tasks_numpy as PT
from pose_numpy import POSE_INFEASIBLE, POSE_NOT_CONVERGED, POSE_STOPPED

FF_NONE, FF_DIFFERENCE = 0, 1
IN_NOT_CONVERGED, IN_INFEASIBLE, IN_LIMIT = 1, 2, 4


def split12(X):
    X = np.asarray(X, dtype=float)
    return X[:9].reshape(3, 3), X[9:]


def transport(Re, pe, u):
    """the action of the placement (Re, pe) on the twist u = [v; w]: [Re v + pe x (Re w); Re w]"""
    w = Re @ u[3:]
    return np.r_[Re @ u[:3] + np.cross(pe, w), w]


def feedforward(kind, R, t, X0, X1, dt):
    """rule 4. of loik_amd_track.h for one constraint: (R, t) = the world placement of the task (or joint) frame, X0 / X1 [12] the
    samples k and k + 1.  [linear; angular] in the frame of the error, masked by the kind as the error is."""
    (R0, t0), (R1, t1) = split12(X0), split12(X1)
    kind = int(kind)
    if kind == PT.TASK_POSITION:
        return np.r_[R.T @ (t1 - t0) / dt, np.zeros(3)]
    Re, pe = R.T @ R0, R.T @ (t0 - t)
    if kind == PT.TASK_ORIENTATION:
        return np.r_[np.zeros(3), Re @ P.log3(R0.T @ R1) / dt]
    return transport(Re, pe, P.log6(R0.T @ R1, R0.T @ (t1 - t0)) / dt)


def lockstep_track_loop(model, prm, q0, H_ref, v_ref, links, A, lb, ub, samples, dt, gain, tol, ff=FF_DIFFERENCE,
                        integrate=P.integrate, q_lo=None, q_hi=None, kinds=None, frames=None, narrow=None):
    """samples [B][T+1][nc][12]; A [nc][6][6] shared or [B][nc][6][6] (ignored with kinds: A_c = S_c X_c^-1 then).  q_lo / q_hi
    [nv]: joint position limits, step for step as pose_limits_numpy.lockstep_pose_loop_limits has them (SolveInit with the
    step's box and the running-maximum b: its docstring says why).  narrow(b, q_b, lo, hi) -> (lo2, hi2): applied to the step's box
    right behind step_box (avoid_numpy.narrower); given without q_lo / q_hi the loop takes the limits branch with infinite limits.
    kinds [nc] (+ frames [nc][12], None = identity): the task law of pose_tasks_numpy.
    Returns lockstep_pose_loop's dict (err = against X_T, reached all False) plus q_traj [B][T+1][nq] and z_traj [B][T][nv] (NaN
    rows after a stop), errmax [B][T+1] (NaN from a stop on), inner [B][T], ontrack [B], worst [B] / worst_at [B] (the first
    maximum of errmax[b][1:] over its finite entries; NaN / -1 without one), and limit_flags [B][nv] with limits."""
    from oracle import ref
    samples = np.asarray(samples, dtype=float)
    B, T, nc = q0.shape[0], samples.shape[1] - 1, len(links)
    tasks = kinds is not None
    if tasks:
        frames = np.tile(PT.IDENTITY12, (nc, 1)) if frames is None else np.asarray(frames, dtype=float).reshape(nc, 12)
        A = PT.task_matrices(kinds, frames)
        errors = lambda qb, tg: PT.task_errors(model, qb, links, kinds, frames, tg)[0]
        placement = lambda qb, c: PT.frame_fk(model, qb, links[c], frames[c])
        kind_of = lambda c: kinds[c]
    else:
        errors = lambda qb, tg: P.pose_errors(model, qb, links, tg)[0]
        placement = lambda qb, c: P.fk(model, qb, links[c])
        kind_of = lambda c: PT.TASK_POSE
    A = np.asarray(A, dtype=float)
    A_of = (lambda b: A[b]) if A.ndim == 4 else (lambda b: A)
    limits = q_lo is not None or narrow is not None
    if limits:
        import pose_limits_numpy as PL
        if q_lo is None:   # (the hook alone: the limits branch with no limit, so that the base box is the step box)
            q_lo, q_hi = np.full(model.nv, -np.inf), np.full(model.nv, np.inf)
        q_lo, q_hi = np.asarray(q_lo, dtype=float), np.asarray(q_hi, dtype=float)
        qidx = PL.limit_q_index(model)
        flags = np.zeros((B, model.nv), dtype=np.int32)
    ids = np.asarray(links, dtype=np.int32)
    kg = gain / dt
    q = np.array(q0, dtype=float)
    steps = np.zeros(B, dtype=np.int32)
    status = np.zeros(B, dtype=np.int32)
    err = np.zeros((B, nc, 6))
    z = np.zeros((B, model.nv))
    it = np.zeros(B, dtype=np.int32)
    q_traj = np.full((B, T + 1, q.shape[1]), np.nan)
    z_traj = np.full((B, T, model.nv), np.nan)
    errmax = np.full((B, T + 1), np.nan)
    inner = np.zeros((B, T), dtype=np.int32)
    ontrack = np.zeros(B, dtype=np.int32)
    for b in range(B):
        r = ref.RefSolver(model, **dict(prm, num_eq_c=nc))
        r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), np.zeros((nc, 6)), lb, ub)
        bis_max, norm_max = np.zeros((nc, 6)), 0.0
        q_traj[b, 0] = q[b]
        for k in range(T + 1):
            with np.errstate(all="ignore"):
                e = errors(q[b:b + 1], samples[b:b + 1, k])
            err[b] = e
            if not (np.all(np.isfinite(e)) and np.all(np.isfinite(q[b]))):
                status[b] |= POSE_STOPPED
                break
            errmax[b, k] = np.max(np.abs(e))
            ontrack[b] += errmax[b, k] <= tol
            if k == T:
                break
            if ff == FF_NONE:   # (the statement of lockstep_pose_loop: no "+ 0")
                u = [kg * e[c] for c in range(nc)]
            else:
                u = []
                for c in range(nc):
                    R, t = placement(q[b:b + 1], c)
                    u.append(kg * e[c] + feedforward(kind_of(c), R[0], t[0], samples[b, k, c], samples[b, k + 1, c], dt))
            bs = np.stack([u[c] if tasks else A_of(b)[c] @ u[c] for c in range(nc)])
            if limits:
                if np.max(np.abs(bs)) > norm_max:
                    bis_max, norm_max = bs, float(np.max(np.abs(bs)))
                lo, hi, flags[b], inside = PL.step_box(q[b], q_lo, q_hi, lb, ub, dt, qidx)
                if narrow is not None:
                    lo, hi = narrow(b, q[b], lo, hi)
                r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), bis_max, lo, hi)
                if flags[b].any():
                    inner[b, k] |= IN_LIMIT
            for c, l in enumerate(links):
                r.UpdateEqConstraint(l, bs[c])
            r.Solve(q[b], -1, None, None)
            if not r.get_convergence_status():
                status[b] |= POSE_NOT_CONVERGED
                inner[b, k] |= IN_NOT_CONVERGED
            if r.get_primal_infeasibility_status():
                status[b] |= POSE_INFEASIBLE
                inner[b, k] |= IN_INFEASIBLE
            z_traj[b, k] = r.field("z")
            qn = integrate(model, q[b], dt * z_traj[b, k])
            if limits:
                ci = qidx[inside]
                qn[ci] = np.clip(qn[ci], q_lo[inside], q_hi[inside])
            q[b] = q_traj[b, k + 1] = qn
            steps[b] += 1
        if steps[b] and not status[b] & POSE_STOPPED:
            z[b], it[b] = r.field("z"), r.get_iter()
    worst, worst_at = worst_of(errmax)
    out = dict(q=q, steps=steps, status=status, reached=np.zeros(B, dtype=bool), err=err, z=z, iter=it, q_traj=q_traj, z_traj=z_traj,
               errmax=errmax, inner=inner, ontrack=ontrack, worst=worst, worst_at=worst_at)
    if limits:
        out["limit_flags"] = flags
    return out


def worst_of(errmax):
    """(worst [B], worst_at [B]) of errmax [B][T+1]: the first maximum of errmax[b][1:] over its finite entries; NaN / -1 without one"""
    B = errmax.shape[0]
    worst, worst_at = np.full(B, np.nan), -np.ones(B, dtype=np.int32)
    for b in range(B):
        fin = np.flatnonzero(np.isfinite(errmax[b, 1:])) + 1
        if fin.size:
            worst_at[b] = fin[np.argmax(errmax[b, fin])]
            worst[b] = errmax[b, worst_at[b]]
    return worst, worst_at


def joint_path_workload(model, links, B, T, seed, move=1e-2, frames=None):
    """a smooth joint path per instance and its poses: q_k = integrate(q_a, (k / T) v) with |v|_inf = T * move, so that a sample
    moves the joints by about `move`; X_k = FK(q_k) (of the task frames with `frames`).
    Returns (q_a [B][nq] = the start, ON the path, samples [B][T+1][nc][12], q_path [B][T+1][nq])."""
    rng = np.random.default_rng(seed)
    q_a = model.random_configurations(rng, B)
    v = rng.normal(size=(B, model.nv))
    v *= T * move / np.abs(v).max(axis=1, keepdims=True)
    q_path = np.stack([np.stack([P.integrate(model, q_a[b], (k / T) * v[b]) for k in range(T + 1)]) for b in range(B)])
    fk = (lambda q: P.fk12(model, q, links)) if frames is None else (lambda q: PT.frame_fk12(model, q, links, frames))
    samples = np.stack([fk(q_path[:, k]) for k in range(T + 1)], axis=1)
    return q_a, samples, q_path
