"""The lock-step CPU oracle of the pose loops WITH joint acceleration limits (include/loik_amd_accel.h): dyn_box is the rule of
that header, the two loops are pose_limits_numpy.lockstep_pose_loop_limits and pose_track_numpy.lockstep_track_loop(q_lo=...)
with dyn_box in place of step_box and the velocity state zp carried from step to step (the SolveInit-per-step construction is
explained in lockstep_pose_loop_limits' docstring and not again here).  tests/test_pose_accel_oracle.py proves both: with
a_max = inf they are np.array_equal to the loops they were written over."""
import numpy as np

import pose_numpy as P
import pose_limits_numpy as PL
import pose_track_numpy as PK
from pose_numpy import POSE_INFEASIBLE, POSE_NOT_CONVERGED, POSE_REACHED, POSE_STOPPED

LIMIT_LOWER, LIMIT_UPPER, LIMIT_ACCEL_LOWER, LIMIT_ACCEL_UPPER = 1, 2, 4, 8
IN_ACCEL = 8
_TINY = np.finfo(float).tiny


def vmax(d, s, dt):
    """the largest velocity from which q += dt z still stops within distance d when the velocity drops by s per step (arrays d, s
    of one shape).  d < 0, d or s infinite, dt s below the normal range: d / dt.  An estimate n >= 2^31 is used uncorrected."""
    d, s = np.array(d, dtype=float), np.array(s, dtype=float)
    with np.errstate(all="ignore"):
        out = d / dt
        ds = dt * s
        m = (d >= 0) & np.isfinite(d) & np.isfinite(s) & (ds >= _TINY)
        if m.any():
            dm, sm, dsm = d[m], s[m], ds[m]
            n = np.floor((np.sqrt(1.0 + 8.0 * (dm / dsm)) - 1.0) / 2.0)
            n = np.minimum(n, 2.0 ** 52)
            fix = n < 2.0 ** 31
            while True:
                dec = fix & (n > 0) & (dsm * n * (n + 1.0) / 2.0 > dm)
                if not dec.any():
                    break
                n[dec] -= 1.0
            while True:
                inc = fix & (dsm * (n + 1.0) * (n + 2.0) / 2.0 <= dm)
                if not inc.any():
                    break
                n[inc] += 1.0
            out[m] = (dm / dt + sm * n * (n + 1.0) / 2.0) / (n + 1.0)
    return out


def dyn_box(q, zp, a, q_lo, q_hi, lb, ub, dt, qidx):
    """the box of one step for one configuration by the rule of loik_amd_accel.h.  q [nq]; zp, a, q_lo, q_hi, lb, ub [nv]; qidx =
    pose_limits_numpy.limit_q_index(model).  Returns (lo, hi, flags, inside) as pose_limits_numpy.step_box does, flags with the
    two acceleration bits beside the position bits."""
    zp, a = np.asarray(zp, dtype=float), np.asarray(a, dtype=float)
    lb, ub = np.asarray(lb, dtype=float), np.asarray(ub, dtype=float)
    nv = lb.size
    s = a * dt
    lim = (qidx >= 0) & (np.isfinite(q_lo) | np.isfinite(q_hi))
    qj = q[qidx[lim]]
    U, Lw = np.full(nv, np.inf), np.full(nv, -np.inf)
    with np.errstate(all="ignore"):
        U[lim] = vmax(q_hi[lim] - qj, s[lim], dt)
        Lw[lim] = -vmax(qj - q_lo[lim], s[lim], dt)
        wlo, whi = zp - s, zp + s
        hi = np.minimum(np.maximum(U, wlo), whi)
        lo = np.minimum(np.minimum(np.maximum(Lw, wlo), whi), hi)
    flags = np.zeros(nv, dtype=np.int32)
    flags[(Lw > lb) & (Lw >= wlo)] |= LIMIT_LOWER
    flags[(U < ub) & (U <= whi)] |= LIMIT_UPPER
    flags[(wlo > lb) & (wlo > Lw)] |= LIMIT_ACCEL_LOWER
    flags[(whi < ub) & (whi < U)] |= LIMIT_ACCEL_UPPER
    lo = np.minimum(np.maximum(lo, lb), ub)
    hi = np.minimum(np.maximum(hi, lb), ub)
    inside = np.zeros(nv, dtype=bool)
    inside[lim] = (q_lo[lim] <= qj) & (qj <= q_hi[lim])
    return lo, hi, flags, inside


def _edge(z, zp, a, dt):
    """some DoF's z sits on an edge of its acceleration window"""
    fin = np.isfinite(a)
    return bool(np.any(np.abs(z - zp)[fin] >= (a[fin] * dt) * (1.0 - 1e-9)))


def lockstep_pose_loop_accel(model, prm, q0, H_ref, v_ref, links, A, lb, ub, targets, dt, gain, tol, max_steps, q_lo, q_hi, a_max,
                             v0=None, integrate=P.integrate):
    """pose_limits_numpy.lockstep_pose_loop_limits with acceleration limits a_max [nv] (+inf: none) and the start velocity v0
    [B][nv] (None: rest).  q_lo / q_hi may be all infinite.  Returns its dict plus velocity [B][nv] (the z of the last step that
    moved the instance; 0 for one that never moved, reached or stopped) and edge [B] (in some step some DoF's z sat on an edge of
    its acceleration window)."""
    from oracle import ref
    B, nc = q0.shape[0], len(links)
    A = np.asarray(A, dtype=float)
    A_of = (lambda b: A[b]) if A.ndim == 4 else (lambda b: A)
    lb, ub = np.asarray(lb, dtype=float), np.asarray(ub, dtype=float)
    box_of = (lambda b: (lb[b], ub[b])) if lb.ndim == 2 else (lambda b: (lb, ub))
    q_lo, q_hi, a_max = np.asarray(q_lo, dtype=float), np.asarray(q_hi, dtype=float), np.asarray(a_max, dtype=float)
    qidx = PL.limit_q_index(model)
    assert qidx.size == model.nv == q_lo.size == q_hi.size == a_max.size
    assert not np.any((qidx < 0) & (np.isfinite(q_lo) | np.isfinite(q_hi))), "a finite limit on a DoF that cannot carry one"
    ids = np.asarray(links, dtype=np.int32)
    k = gain / dt
    q = np.array(q0, dtype=float)
    steps = np.zeros(B, dtype=np.int32)
    status = np.zeros(B, dtype=np.int32)
    err = np.zeros((B, nc, 6))
    z = np.zeros((B, model.nv))
    it = np.zeros(B, dtype=np.int32)
    flags = np.zeros((B, model.nv), dtype=np.int32)
    vel = np.zeros((B, model.nv))
    edge = np.zeros(B, dtype=bool)
    solvers, end, bmax = [], np.zeros(B, dtype=np.int32), []
    for b in range(B):
        r = ref.RefSolver(model, **dict(prm, num_eq_c=nc))
        lb_b, ub_b = box_of(b)
        r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), np.zeros((nc, 6)), lb_b, ub_b)
        solvers.append(r)
        bis_max, norm_max = np.zeros((nc, 6)), 0.0
        zp = np.zeros(model.nv) if v0 is None else np.array(v0[b], dtype=float)
        moved = False
        for step in range(max_steps + 1):
            end[b] = step
            with np.errstate(all="ignore"):
                e = P.pose_errors(model, q[b:b + 1], links, targets[b:b + 1])[0]
            err[b] = e
            if not (np.all(np.isfinite(e)) and np.all(np.isfinite(q[b]))):
                status[b] |= POSE_STOPPED
                break
            if np.max(np.abs(e)) <= tol:
                status[b] |= POSE_REACHED
                break
            if step == max_steps:
                break
            bs = np.stack([A_of(b)[c] @ (k * e[c]) for c in range(nc)])
            if np.max(np.abs(bs)) > norm_max:
                bis_max, norm_max = bs, float(np.max(np.abs(bs)))
            lo, hi, flags[b], inside = dyn_box(q[b], zp, a_max, q_lo, q_hi, lb_b, ub_b, dt, qidx)
            r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), bis_max, lo, hi)
            for c, l in enumerate(links):
                r.UpdateEqConstraint(l, bs[c])
            r.Solve(q[b], -1, None, None)
            if not r.get_convergence_status():
                status[b] |= POSE_NOT_CONVERGED
            if r.get_primal_infeasibility_status():
                status[b] |= POSE_INFEASIBLE
            zn = np.array(r.field("z"), dtype=float)
            edge[b] = edge[b] or _edge(zn, zp, a_max, dt)
            qn = integrate(model, q[b], dt * zn)
            ci = qidx[inside]
            qn[ci] = np.clip(qn[ci], q_lo[inside], q_hi[inside])
            q[b] = qn
            zp, moved = zn, True
            steps[b] += 1
        if moved and not status[b] & (POSE_REACHED | POSE_STOPPED):
            vel[b] = zp
        bmax.append(bis_max)
    n_solves = int(end.max()) if B else 0
    for b in range(B):   # the idle b = 0 solves, with the base box, of the instances that left the loop before the batch did
        r = solvers[b]
        if end[b] < n_solves and not status[b] & POSE_STOPPED:
            lb_b, ub_b = box_of(b)
            r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), bmax[b], lb_b, ub_b)
            for l in links:
                r.UpdateEqConstraint(l, np.zeros(6))
            for _ in range(n_solves - end[b]):
                r.Solve(q[b], -1, None, None)
        if n_solves > 0 and not status[b] & POSE_STOPPED:
            z[b], it[b] = r.field("z"), r.get_iter()
    return dict(q=q, steps=steps, status=status, reached=(status & POSE_REACHED) != 0, err=err, z=z, iter=it, limit_flags=flags,
                velocity=vel, edge=edge)


def lockstep_track_loop_accel(model, prm, q0, H_ref, v_ref, links, A, lb, ub, samples, dt, gain, tol, q_lo, q_hi, a_max, v0=None,
                              ff=PK.FF_DIFFERENCE, integrate=P.integrate):
    """pose_track_numpy.lockstep_track_loop(q_lo=..., q_hi=...) in the joint frame, with acceleration limits a_max [nv] and the
    start velocity v0 [B][nv] (None: rest); lb / ub [nv].  inner carries IN_LIMIT for a position flag of the step and IN_ACCEL for
    an acceleration flag.  Returns its dict plus velocity [B][nv] and edge [B] as lockstep_pose_loop_accel."""
    from oracle import ref
    samples = np.asarray(samples, dtype=float)
    B, T, nc = q0.shape[0], samples.shape[1] - 1, len(links)
    A = np.asarray(A, dtype=float)
    A_of = (lambda b: A[b]) if A.ndim == 4 else (lambda b: A)
    q_lo, q_hi, a_max = np.asarray(q_lo, dtype=float), np.asarray(q_hi, dtype=float), np.asarray(a_max, dtype=float)
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
    vel = np.zeros((B, model.nv))
    edge = np.zeros(B, dtype=bool)
    for b in range(B):
        r = ref.RefSolver(model, **dict(prm, num_eq_c=nc))
        r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), np.zeros((nc, 6)), lb, ub)
        bis_max, norm_max = np.zeros((nc, 6)), 0.0
        q_traj[b, 0] = q[b]
        zp = np.zeros(model.nv) if v0 is None else np.array(v0[b], dtype=float)
        for k in range(T + 1):
            with np.errstate(all="ignore"):
                e = P.pose_errors(model, q[b:b + 1], links, samples[b:b + 1, k])[0]
            err[b] = e
            if not (np.all(np.isfinite(e)) and np.all(np.isfinite(q[b]))):
                status[b] |= POSE_STOPPED
                break
            errmax[b, k] = np.max(np.abs(e))
            ontrack[b] += errmax[b, k] <= tol
            if k == T:
                break
            if ff == PK.FF_NONE:
                u = [kg * e[c] for c in range(nc)]
            else:
                u = []
                for c in range(nc):
                    R, t = P.fk(model, q[b:b + 1], links[c])
                    u.append(kg * e[c] + PK.feedforward(0, R[0], t[0], samples[b, k, c], samples[b, k + 1, c], dt))
            bs = np.stack([A_of(b)[c] @ u[c] for c in range(nc)])
            if np.max(np.abs(bs)) > norm_max:
                bis_max, norm_max = bs, float(np.max(np.abs(bs)))
            lo, hi, flags[b], inside = dyn_box(q[b], zp, a_max, q_lo, q_hi, lb, ub, dt, qidx)
            r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), bis_max, lo, hi)
            if (flags[b] & 3).any():
                inner[b, k] |= PK.IN_LIMIT
            if (flags[b] & 12).any():
                inner[b, k] |= IN_ACCEL
            for c, l in enumerate(links):
                r.UpdateEqConstraint(l, bs[c])
            r.Solve(q[b], -1, None, None)
            if not r.get_convergence_status():
                status[b] |= POSE_NOT_CONVERGED
                inner[b, k] |= PK.IN_NOT_CONVERGED
            if r.get_primal_infeasibility_status():
                status[b] |= POSE_INFEASIBLE
                inner[b, k] |= PK.IN_INFEASIBLE
            z_traj[b, k] = r.field("z")
            edge[b] = edge[b] or _edge(z_traj[b, k], zp, a_max, dt)
            qn = integrate(model, q[b], dt * z_traj[b, k])
            ci = qidx[inside]
            qn[ci] = np.clip(qn[ci], q_lo[inside], q_hi[inside])
            q[b] = q_traj[b, k + 1] = qn
            zp = z_traj[b, k].copy()
            steps[b] += 1
        if steps[b] and not status[b] & POSE_STOPPED:
            z[b], it[b] = r.field("z"), r.get_iter()
            vel[b] = zp
    worst, worst_at = PK.worst_of(errmax)
    return dict(q=q, steps=steps, status=status, reached=np.zeros(B, dtype=bool), err=err, z=z, iter=it, q_traj=q_traj, z_traj=z_traj,
                errmax=errmax, inner=inner, ontrack=ontrack, worst=worst, worst_at=worst_at, limit_flags=flags, velocity=vel, edge=edge)


def accel_limits(model, seed, dt, bound, lo=1e-4, hi=1e-3):
    """acceleration limits for the tests: finite on a seeded random half of the DoFs, with a dt uniform in [lo, hi] * bound (bound =
    the velocity box of the workload), +inf on the others"""
    rng = np.random.default_rng(seed)
    pick = np.sort(rng.choice(model.nv, size=max(1, model.nv // 2), replace=False))
    a = np.full(model.nv, np.inf)
    a[pick] = rng.uniform(lo, hi, size=pick.size) * bound / dt
    return a
