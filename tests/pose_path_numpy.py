"""The lock-step CPU oracle of the pose loop ALONG WAYPOINT PATHS (include/loik_amd_path.h), in the structure of
pose_numpy.lockstep_pose_loop: each instance carries a cursor w and a count ws of the steps spent on waypoint w, and a re-target of
a running instance repeats

    1. e against waypoint w (pose_numpy.pose_errors, or pose_tasks_numpy.task_errors with kinds / frames);
    2. e or q not finite                        -> STOPPED;
    3. max |e| <= tol                           -> q_path[b][w] = q, wsteps[b][w] = ws, w += 1, ws = 0; w == T -> REACHED, else 1. again
                                                   with the next waypoint, in the same re-target;
    4. budget > 0 and ws == budget              -> STALLED (leaves the loop; neither REACHED nor STOPPED);
    5. otherwise the instance runs: b_c = A_c (gain / dt) e_c, the tailored Solve, q <- q (+) dt z, steps and ws count one.

The re-target after max_steps steps applies 1. to 4. and runs nothing.  The loop is as long as its longest instance; the others
take the idle b = 0 solves at their final q, as in lockstep_pose_loop.  The limits variant takes its box rule from
pose_limits_numpy.step_box and the tasks variant its error from pose_tasks_numpy.task_errors: nothing of either is restated."""
import numpy as np

import pose_numpy as P
from pose_numpy import POSE_INFEASIBLE, POSE_NOT_CONVERGED, POSE_REACHED, POSE_STOPPED

PATH_COMPLETE, PATH_STALLED = 1, 2


def lockstep_path_loop(model, prm, q0, H_ref, v_ref, links, A, lb, ub, waypoints, dt, gain, tol, max_steps, budget=0,
                       integrate=P.integrate, q_lo=None, q_hi=None, kinds=None, frames=None, narrow=None):
    """waypoints [B][T][nc][12]; A [nc][6][6] shared or [B][nc][6][6] (ignored with kinds: A_c = S_c X_c^-1 then); budget = steps per
    waypoint at most (0: none).  q_lo / q_hi [nv]: joint position limits, step for step as
    pose_limits_numpy.lockstep_pose_loop_limits has them (SolveInit with the step's box and the running-maximum b: its docstring
    says why).  narrow(b, q_b, lo, hi) -> (lo2, hi2): applied to the step's box right behind step_box (avoid_numpy.narrower); given
    without q_lo / q_hi the loop takes the limits branch with infinite limits.  kinds [nc] (+ frames [nc][12], None = identity): the
    task law of pose_tasks_numpy.
    Returns lockstep_pose_loop's dict (steps = the total, err = against waypoint min(cursor, T - 1)) plus cursor [B], wsteps [B][T]
    (at the cursor: the steps so far), path_status [B], q_path [B][T][nq] (NaN rows from the cursor on), n_solves = the length
    of the loop, and limit_flags [B][nv] with limits."""
    from oracle import ref
    waypoints = np.asarray(waypoints, dtype=float)
    B, T, nc = q0.shape[0], waypoints.shape[1], len(links)
    tasks = kinds is not None
    if tasks:
        import pose_tasks_numpy as PT
        frames = np.tile(PT.IDENTITY12, (nc, 1)) if frames is None else np.asarray(frames, dtype=float).reshape(nc, 12)
        A = PT.task_matrices(kinds, frames)
        errors = lambda qb, tg: PT.task_errors(model, qb, links, kinds, frames, tg)[0]
    else:
        errors = lambda qb, tg: P.pose_errors(model, qb, links, tg)[0]
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
    k = gain / dt
    q = np.array(q0, dtype=float)
    steps = np.zeros(B, dtype=np.int32)
    status = np.zeros(B, dtype=np.int32)
    pstatus = np.zeros(B, dtype=np.int32)
    cursor = np.zeros(B, dtype=np.int32)
    wsteps = np.zeros((B, T), dtype=np.int32)
    q_path = np.full((B, T, q.shape[1]), np.nan)
    err = np.zeros((B, nc, 6))
    z = np.zeros((B, model.nv))
    it = np.zeros(B, dtype=np.int32)
    solvers, end, bmax = [], np.zeros(B, dtype=np.int32), []
    for b in range(B):   # each instance until it leaves the loop: complete, stopped, stalled, or max_steps
        r = ref.RefSolver(model, **dict(prm, num_eq_c=nc))
        r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), np.zeros((nc, 6)), lb, ub)
        solvers.append(r)
        bis_max, norm_max = np.zeros((nc, 6)), 0.0
        w = ws = 0
        for step in range(max_steps + 1):
            end[b] = step
            left = False
            while True:   # the rule, until the instance runs or leaves
                with np.errstate(all="ignore"):
                    e = errors(q[b:b + 1], waypoints[b:b + 1, w])
                err[b] = e
                if not (np.all(np.isfinite(e)) and np.all(np.isfinite(q[b]))):
                    status[b] |= POSE_STOPPED
                    left = True
                    break
                if np.max(np.abs(e)) <= tol:
                    q_path[b, w] = q[b]
                    wsteps[b, w] = ws
                    w, ws = w + 1, 0
                    if w == T:
                        status[b] |= POSE_REACHED
                        pstatus[b] |= PATH_COMPLETE
                        left = True
                        break
                    continue
                if budget > 0 and ws == budget:
                    pstatus[b] |= PATH_STALLED
                    left = True
                break
            if left or step == max_steps:
                break
            bs = np.stack([(k * e[c]) if tasks else A_of(b)[c] @ (k * e[c]) for c in range(nc)])
            if limits:
                if np.max(np.abs(bs)) > norm_max:
                    bis_max, norm_max = bs, float(np.max(np.abs(bs)))
                lo, hi, flags[b], inside = PL.step_box(q[b], q_lo, q_hi, lb, ub, dt, qidx)
                if narrow is not None:
                    lo, hi = narrow(b, q[b], lo, hi)
                r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), bis_max, lo, hi)
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
            ws += 1
        cursor[b] = w
        if w < T:
            wsteps[b, w] = ws
        bmax.append(bis_max)
    n_solves = int(end.max()) if B else 0   # the step at which none is running any more (or max_steps)
    for b in range(B):   # the idle b = 0 solves at the final q of the instances that left the loop before the batch did
        r = solvers[b]
        if end[b] < n_solves and not status[b] & POSE_STOPPED:
            if limits:
                r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), bmax[b], lb, ub)
            for l in links:
                r.UpdateEqConstraint(l, np.zeros(6))
            for _ in range(n_solves - end[b]):
                r.Solve(q[b], -1, None, None)
        if n_solves > 0 and not status[b] & POSE_STOPPED:
            z[b], it[b] = r.field("z"), r.get_iter()
    out = dict(q=q, steps=steps, status=status, reached=(status & POSE_REACHED) != 0, err=err, z=z, iter=it, cursor=cursor,
               wsteps=wsteps, path_status=pstatus, q_path=q_path, n_solves=n_solves)
    if limits:
        out["limit_flags"] = flags
    return out


def asynchrony_workload(model, links, B, T, seed, far=0.30, near=0.0005):
    """the workload on which a per-instance cursor pays: even instances get a far first leg and a near second leg, odd instances
    the reverse, alternating on along the path.  Instance b moves along one direction d_b (normal noise scaled to |d|_inf = 1):
    waypoint t = fk12(integrate(q_a, s_t d)) with s_t the leg lengths added up.  Returns (q_a [B][nq], waypoints [B][T][nc][12],
    far_first [B] bool)."""
    rng = np.random.default_rng(seed)
    q_a = model.random_configurations(rng, B)
    wp = np.empty((B, T, len(links), 12))
    for b in range(B):
        d = rng.normal(size=model.nv)
        d /= np.max(np.abs(d))
        s = 0.0
        for t in range(T):
            s += far if (b + t) % 2 == 0 else near
            wp[b, t] = P.fk12(model, P.integrate(model, q_a[b], s * d)[None], links)[0]
    return q_a, wp, np.arange(B) % 2 == 0
