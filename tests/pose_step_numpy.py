"""The lock-step CPU oracle of the pose loop WITH step control (include/loik_amd_step.h): pose_numpy.lockstep_pose_loop -- with joint
position limits pose_limits_numpy.lockstep_pose_loop_limits, with tasks pose_tasks_numpy.lockstep_pose_loop_tasks' error and law --
where the step's integrate is the backtracking search of that header.  The errors, the integrator, the box and the task matrices
are those modules' functions; what is stated here is the rule alone:

    Phi(q) = sum_c sum_r e_c[r]^2                      (c-major, then r; the square rounded before the add)
    Phi0   = Phi of the errors the step's re-target formed
    trial m = 0..M:  alpha_0 = 1, alpha_{m+1} = alpha_m * shrink;  q_m = q (+) (alpha_m dt) z, clamped as the step's clamp does it
    accept the first m with q_m and its errors finite and Phi(q_m) <= (1 - sufficient * alpha_m) * Phi0
    none accepted: failed += 1; with patience > 0 and `patience` failures in a row STALLED (q stays, the step is not counted),
    otherwise the plain step q_0."""
import numpy as np

import pose_numpy as P
from pose_numpy import POSE_INFEASIBLE, POSE_NOT_CONVERGED, POSE_REACHED, POSE_STOPPED

POSE_STALLED = 16
DEFAULTS = dict(shrink=0.5, sufficient=1e-4, max_backtracks=6, patience=0)


def merit(e):
    """Phi of one instance's errors [nc][6]: one product and one add per entry, in order"""
    phi = 0.0
    for x in np.asarray(e, dtype=float).reshape(-1):
        sq = x * x
        phi = phi + sq
    return float(phi)


def lockstep_pose_loop_step(model, prm, q0, H_ref, v_ref, links, A, lb, ub, targets, dt, gain, tol, max_steps, shrink=0.5,
                            sufficient=1e-4, max_backtracks=6, patience=0, q_lo=None, q_hi=None, tasks=None, integrate=P.integrate, narrow=None):
    """pose_numpy.lockstep_pose_loop with the rule above.  q_lo / q_hi [nv]: joint position limits, the loop is then
    pose_limits_numpy.lockstep_pose_loop_limits (its per-step SolveInit and why: that function's docstring).  tasks = (kinds [nc],
    frames [nc][12] or None): the handle has tasks, A is ignored (A_c = S_c X_c^-1), the error is the masked task-frame error and
    b_c = (gain / dt) e_c, as pose_tasks_numpy.lockstep_pose_loop_tasks has it (axis kinds included).  narrow(b, q_b, lo, hi) ->
    (lo2, hi2): applied to the step's box right behind step_box (avoid_numpy.narrower), once per step whose inner solve ran -- a
    search that ends STALLED included, since the box is narrowed before the search; given without q_lo / q_hi the loop takes the
    limits branch with infinite limits.
    Returns those functions' dict plus
      alpha [B]       alpha of the last step that moved the instance, 0 if none
      backtracks [B]  sum over the accepted searches of the accepted m
      failed [B]      searches in which no trial was accepted
      margin [B]      the smallest |Phi(q_m) - (1 - sufficient alpha_m) Phi0| / Phi0 over every decision the instance took, inf if none
      phi [B][max_steps]   the merit after each step (NaN: the step did not run, or stalled)
      trial [B][max_steps] the accepted m of each step, -1 for a failed search, -2 for a step that did not run
      phi0 [B]        the merit of the seed (NaN for an instance stopped at once)"""
    from oracle import ref
    import pose_limits_numpy as PL
    B, nc = q0.shape[0], len(links)
    if tasks is not None:
        import pose_axis_numpy as PA
        kinds = [int(k) for k in tasks[0]]
        frames = np.tile(PA.T.IDENTITY12, (nc, 1)) if tasks[1] is None else np.asarray(tasks[1], dtype=float).reshape(nc, 12)
        A = PA.task_matrices(kinds, frames)
        errors = lambda qs, tg: PA.task_errors(model, qs, links, kinds, frames, tg)
        law = lambda b, c, ke: ke
    else:
        A = np.asarray(A, dtype=float)
        errors = lambda qs, tg: P.pose_errors(model, qs, links, tg)
        law = lambda b, c, ke: A_of(b)[c] @ ke
    A_of = (lambda b: A[b]) if A.ndim == 4 else (lambda b: A)
    lb, ub = np.asarray(lb, dtype=float), np.asarray(ub, dtype=float)
    box_of = (lambda b: (lb[b], ub[b])) if lb.ndim == 2 else (lambda b: (lb, ub))
    limits = q_lo is not None or narrow is not None
    if limits:
        if q_lo is None:   # (the hook alone: the limits branch with no limit, so that the base box is the step box)
            q_lo, q_hi = np.full(model.nv, -np.inf), np.full(model.nv, np.inf)
        q_lo, q_hi = np.asarray(q_lo, dtype=float), np.asarray(q_hi, dtype=float)
        qidx = PL.limit_q_index(model)
    ids = np.asarray(links, dtype=np.int32)
    k = gain / dt
    q = np.array(q0, dtype=float)
    steps = np.zeros(B, dtype=np.int32)
    status = np.zeros(B, dtype=np.int32)
    err = np.zeros((B, nc, 6))
    z = np.zeros((B, model.nv))
    it = np.zeros(B, dtype=np.int32)
    flags = np.zeros((B, model.nv), dtype=np.int32)
    alpha, backtracks, failed = np.zeros(B), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    margin = np.full(B, np.inf)
    phi = np.full((B, max_steps), np.nan)
    trial = np.full((B, max_steps), -2, dtype=np.int32)
    phi_seed = np.full(B, np.nan)
    solvers, end, bmax = [], np.zeros(B, dtype=np.int32), []

    def moved(b, a, zb, inside):
        qn = integrate(model, q[b], (a * dt) * zb)
        if limits:
            ci = qidx[inside]
            qn[ci] = np.clip(qn[ci], q_lo[inside], q_hi[inside])
        return qn

    for b in range(B):
        r = ref.RefSolver(model, **dict(prm, num_eq_c=nc))
        lb_b, ub_b = box_of(b)
        r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), np.zeros((nc, 6)), lb_b, ub_b)
        solvers.append(r)
        bis_max, norm_max, run = np.zeros((nc, 6)), 0.0, 0
        for step in range(max_steps + 1):
            end[b] = step
            with np.errstate(all="ignore"):
                e = errors(q[b:b + 1], targets[b:b + 1])[0]
            err[b] = e
            if not (np.all(np.isfinite(e)) and np.all(np.isfinite(q[b]))):
                status[b] |= POSE_STOPPED
                break
            if step == 0:
                phi_seed[b] = merit(e)
            if np.max(np.abs(e)) <= tol:
                status[b] |= POSE_REACHED
                break
            if step == max_steps:
                break
            bs = np.stack([law(b, c, k * e[c]) for c in range(nc)])
            inside = None
            if limits:
                if np.max(np.abs(bs)) > norm_max:
                    bis_max, norm_max = bs, float(np.max(np.abs(bs)))
                lo, hi, flags[b], inside = PL.step_box(q[b], q_lo, q_hi, lb_b, ub_b, dt, qidx)
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
            steps[b] += 1
            # ---- the search of loik_amd_step.h
            zb = r.field("z")
            phi0 = merit(e)
            alphas = [1.0]
            for _ in range(max_backtracks):
                alphas.append(alphas[-1] * shrink)
            with np.errstate(all="ignore"):
                q_trials = [moved(b, alphas[0], zb, inside)]
                e_trials = list(errors(np.stack(q_trials), targets[b:b + 1]))
            accepted = -1
            for m, a in enumerate(alphas):
                if m == 1:   # (trial 0 failed: the others in one batch of forward kinematics; they are judged in order all the same)
                    with np.errstate(all="ignore"):
                        q_trials += [moved(b, x, zb, inside) for x in alphas[1:]]
                        e_trials += list(errors(np.stack(q_trials[1:]), np.repeat(targets[b:b + 1], len(alphas) - 1, axis=0)))
                if not (np.all(np.isfinite(q_trials[m])) and np.all(np.isfinite(e_trials[m]))):
                    continue
                sa = sufficient * a
                bound = (1.0 - sa) * phi0
                phi_m = merit(e_trials[m])
                margin[b] = min(margin[b], abs(phi_m - bound) / phi0)
                if phi_m <= bound:
                    accepted = m
                    break
            if accepted >= 0:
                q[b], alpha[b], run = q_trials[accepted], alphas[accepted], 0
                backtracks[b] += accepted
                trial[b, step], phi[b, step] = accepted, merit(e_trials[accepted])
                continue
            failed[b] += 1
            run += 1
            trial[b, step] = -1
            if patience > 0 and run >= patience:
                status[b] |= POSE_STALLED
                steps[b] -= 1
                end[b] = step + 1   # (its solve of this step ran; at the next re-target it no longer runs)
                break
            q[b], alpha[b] = q_trials[0], 1.0
            phi[b, step] = merit(e_trials[0])
        bmax.append(bis_max)
    n_solves = int(end.max()) if B else 0
    for b in range(B):   # the idle b = 0 solves (with limits: in the base box) of the instances that left the loop before the batch did
        r = solvers[b]
        if end[b] < n_solves and not status[b] & POSE_STOPPED:
            if limits:
                lb_b, ub_b = box_of(b)
                r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), bmax[b], lb_b, ub_b)
            for l in links:
                r.UpdateEqConstraint(l, np.zeros(6))
            for _ in range(n_solves - end[b]):
                r.Solve(q[b], -1, None, None)
        if n_solves > 0 and not status[b] & POSE_STOPPED:
            z[b], it[b] = r.field("z"), r.get_iter()
    out = dict(q=q, steps=steps, status=status, reached=(status & POSE_REACHED) != 0, err=err, z=z, iter=it, alpha=alpha,
               backtracks=backtracks, failed=failed, margin=margin, phi=phi, trial=trial, phi0=phi_seed)
    if limits:
        out["limit_flags"] = flags
    return out
