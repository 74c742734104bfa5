"""The lock-step CPU oracle of the pose loop WITH tool frames and task kinds (include/loik_amd_tasks.h), in the structure of
pose_numpy.lockstep_pose_loop.  Pinocchio's public conventions, restated: (R, t) = oMi of the constrained link, (Rf, pf) = iMf,
(Rd, td) the target, twists [linear; angular];

    oMf  = (R Rf, t + R pf)
    X^-1 = [[Rf^T, -Rf^T [pf]x], [0, Rf^T]]          v_f = X^-1 v_i
    pose         e = log6(oMf^-1 oMdes)              S = I
    position     e = [(R Rf)^T (td - t - R pf); 0]   S = diag(1,1,1,0,0,0)
    orientation  e = [0; log3((R Rf)^T Rd)]          S = diag(0,0,0,1,1,1)

A_c = S_c X_c^-1 goes into SolveInit, b_c = (gain / dt) S_c e_c, reached when max_c |S_c e_c|_inf <= tol.  pose_numpy supplies
fk / log3 / log6 / integrate; pose_limits_numpy the box rule when joint position limits are given as well."""
import numpy as np

import pose_numpy as P
from pose_numpy import POSE_INFEASIBLE, POSE_NOT_CONVERGED, POSE_REACHED, POSE_STOPPED

TASK_POSE, TASK_POSITION, TASK_ORIENTATION = 0, 1, 2
IDENTITY12 = np.r_[np.eye(3).ravel(), np.zeros(3)]
_MASK = {TASK_POSE: np.ones(6), TASK_POSITION: np.r_[np.ones(3), np.zeros(3)], TASK_ORIENTATION: np.r_[np.zeros(3), np.ones(3)]}


def mask(kind):
    """the diagonal of S for a kind"""
    return _MASK[int(kind)].copy()


def x_inv(frame12):
    """the motion transform joint frame -> task frame of iMf = frame12 [12]: v_f = X^-1 v_i"""
    F = np.asarray(frame12, dtype=float)
    Rf, pf = F[:9].reshape(3, 3), F[9:]
    X = np.zeros((6, 6))
    X[:3, :3] = Rf.T
    X[3:, 3:] = Rf.T
    X[:3, 3:] = -Rf.T @ P.skew(pf)
    return X


def task_matrices(kinds, frames):
    """[nc][6][6]: A_c = S_c X_c^-1"""
    return np.stack([mask(k)[:, None] * x_inv(f) for k, f in zip(kinds, frames)])


def frame_fk(model, q, link, frame12):
    """oMf = oMi(link) iMf for configurations q [B][nq]: (R [B,3,3], t [B,3])"""
    F = np.asarray(frame12, dtype=float)
    R, t = P.fk(model, q, link)
    return R @ F[:9].reshape(3, 3), t + R @ F[9:]


def frame_fk12(model, q, links, frames):
    """[B][n][12] placements (R row-major, t) of the frames on `links`"""
    out = []
    for l, f in zip(links, frames):
        R, t = frame_fk(model, q, l, f)
        out.append(np.concatenate([R.reshape(-1, 9), t], axis=1))
    return np.stack(out, axis=1)


def task_error(Rw, tw, target12, kind):
    """S e of one task-frame placement (Rw, tw) = oMf against a target [12], zeros in the masked-out entries"""
    D = np.asarray(target12, dtype=float)
    Rd, td = D[:9].reshape(3, 3), D[9:]
    kind = int(kind)
    if kind == TASK_POSITION:
        return np.r_[Rw.T @ (td - tw), np.zeros(3)]
    if kind == TASK_ORIENTATION:
        return np.r_[np.zeros(3), P.log3(Rw.T @ Rd)]
    return P.log6(Rw.T @ Rd, Rw.T @ (td - tw))


def task_errors(model, q, links, kinds, frames, targets):
    """[B][nc][6] masked task-frame errors of configurations q [B][nq] against targets [B][nc][12]"""
    B = q.shape[0]
    e = np.empty((B, len(links), 6))
    for c, l in enumerate(links):
        R, t = frame_fk(model, q, l, frames[c])
        for b in range(B):
            e[b, c] = task_error(R[b], t[b], targets[b, c], kinds[c])
    return e


def lockstep_pose_loop_tasks(model, prm, q0, H_ref, v_ref, links, kinds, frames, lb, ub, targets, dt, gain, tol, max_steps,
                             integrate=P.integrate, q_lo=None, q_hi=None):
    """pose_numpy.lockstep_pose_loop on a handle with tasks: A_c = S_c X_c^-1 in SolveInit, the masked task-frame error,
    b_c = (gain / dt) S_c e_c, reached on max_c |S_c e_c|_inf.  kinds [nc], frames [nc][12] (None: the identity), targets
    [B][nc][12].  Returns lockstep_pose_loop's dict.
    With q_lo / q_hi [nv] the box rule of pose_limits_numpy.lockstep_pose_loop_limits is combined with it, step for step as that
    function does it (SolveInit with the step's box and the running-maximum b, its docstring says why), and limit_flags [B][nv]
    is returned too."""
    from oracle import ref
    B, nc = q0.shape[0], len(links)
    frames = np.tile(IDENTITY12, (nc, 1)) if frames is None else np.asarray(frames, dtype=float).reshape(nc, 12)
    A = task_matrices(kinds, frames)
    limits = q_lo is not None
    if limits:
        import pose_limits_numpy as PL
        q_lo, q_hi = np.asarray(q_lo, dtype=float), np.asarray(q_hi, dtype=float)
        qidx = PL.limit_q_index(model)
        flags = np.zeros((B, model.nv), dtype=np.int32)
    ids = np.asarray(links, dtype=np.int32)
    k = gain / dt
    q = np.array(q0, dtype=float)
    steps = np.zeros(B, dtype=np.int32)
    status = np.zeros(B, dtype=np.int32)
    err = np.zeros((B, nc, 6))
    z = np.zeros((B, model.nv))
    it = np.zeros(B, dtype=np.int32)
    solvers, end, bmax = [], np.zeros(B, dtype=np.int32), []
    for b in range(B):
        r = ref.RefSolver(model, **dict(prm, num_eq_c=nc))
        r.SolveInit(q[b], H_ref, v_ref, ids, A, np.zeros((nc, 6)), lb, ub)
        solvers.append(r)
        bis_max, norm_max = np.zeros((nc, 6)), 0.0
        for step in range(max_steps + 1):
            end[b] = step
            with np.errstate(all="ignore"):
                e = task_errors(model, q[b:b + 1], links, kinds, frames, targets[b:b + 1])[0]
            err[b] = e
            if not (np.all(np.isfinite(e)) and np.all(np.isfinite(q[b]))):
                status[b] |= POSE_STOPPED
                break
            if np.max(np.abs(e)) <= tol:
                status[b] |= POSE_REACHED
                break
            if step == max_steps:
                break
            bs = np.stack([k * e[c] for c in range(nc)])
            if limits:
                if np.max(np.abs(bs)) > norm_max:
                    bis_max, norm_max = bs, float(np.max(np.abs(bs)))
                lo, hi, flags[b], inside = PL.step_box(q[b], q_lo, q_hi, lb, ub, dt, qidx)
                r.SolveInit(q[b], H_ref, v_ref, ids, A, bis_max, lo, hi)
            for c, l in enumerate(links):
                r.UpdateEqConstraint(l, bs[c])
            r.Solve(q[b], -1, None, None)
            if not r.get_convergence_status():
                status[b] |= POSE_NOT_CONVERGED
            if r.get_primal_infeasibility_status():
                status[b] |= POSE_INFEASIBLE
            qn = integrate(model, q[b], dt * r.field("z"))
            if limits:
                ci = qidx[inside]
                qn[ci] = np.clip(qn[ci], q_lo[inside], q_hi[inside])
            q[b] = qn
            steps[b] += 1
        bmax.append(bis_max)
    n_solves = int(end.max()) if B else 0
    for b in range(B):   # the idle b = 0 solves at the final q of the instances that left the loop before the batch did
        r = solvers[b]
        if end[b] < n_solves and not status[b] & POSE_STOPPED:
            if limits:
                r.SolveInit(q[b], H_ref, v_ref, ids, A, bmax[b], lb, ub)
            for l in links:
                r.UpdateEqConstraint(l, np.zeros(6))
            for _ in range(n_solves - end[b]):
                r.Solve(q[b], -1, None, None)
        if n_solves > 0 and not status[b] & POSE_STOPPED:
            z[b], it[b] = r.field("z"), r.get_iter()
    out = dict(q=q, steps=steps, status=status, reached=(status & POSE_REACHED) != 0, err=err, z=z, iter=it)
    if limits:
        out["limit_flags"] = flags
    return out


def random_frames(rng, n, offset=(0.1, 0.2)):
    """[n][12]: a uniformly random rotation and a translation of a length uniform in `offset`, per frame"""
    out = np.empty((n, 12))
    for i in range(n):
        a = rng.normal(size=3)
        R = P.exp3(rng.uniform(0.3, np.pi - 0.3) * a / np.linalg.norm(a))
        p = rng.normal(size=3)
        out[i] = np.r_[R.ravel(), rng.uniform(*offset) * p / np.linalg.norm(p)]
    return out
