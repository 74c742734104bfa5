"""The lock-step CPU oracle of the pose loop WITH joint position limits (include/loik_amd_limits.h), assembled from what
oracle/ref.py offers: RefSolver changes its velocity box only through SolveInit.  pose_numpy supplies fk / pose_errors /
integrate; nothing of it is restated here."""
import numpy as np

from loik_amd import workloads as W

import pose_numpy as P
from pose_numpy import POSE_INFEASIBLE, POSE_NOT_CONVERGED, POSE_REACHED, POSE_STOPPED

LIMIT_LOWER, LIMIT_UPPER = 1, 2
_PLAIN_1DOF = {P.J_RX, P.J_RY, P.J_RZ, P.J_PX, P.J_PY, P.J_PZ, P.J_RU, P.J_PU, P.J_HX, P.J_HY, P.J_HZ, P.J_HU}


def limit_q_index(model):
    """[nv] int: where the configuration coordinate of each DoF sits in q when the integrator advances it by a plain sum (bounded
    revolute, prismatic, helical, the coordinates of a translation joint, the ZYX angles; sub-joints of a composite alike), -1
    for every other DoF (free-flyer, spherical, planar, (cos, sin) revolute): the DoFs that may carry a position limit"""
    if getattr(model, "composite", None):
        return limit_q_index(W._Chain(model))
    out = -np.ones(int(max(int(model.idx_v[i]) for i in range(1, model.njoints))) + 6, dtype=int)
    nv = 0
    for i in range(1, model.njoints):
        jt, iq, iv = int(model.jtype[i]), int(model.idx_q[i]), int(model.idx_v[i])
        n = 6 if jt == P.J_FREEFLYER else 3 if jt in (P.J_SPHERICAL, P.J_TRANSLATION, P.J_SPHERICAL_ZYX, P.J_PLANAR) else 1
        if jt in _PLAIN_1DOF:
            out[iv] = iq
        elif jt in (P.J_TRANSLATION, P.J_SPHERICAL_ZYX):
            out[iv:iv + 3] = np.arange(iq, iq + 3)
        nv = max(nv, iv + n)
    return out[:nv]


def step_box(q, q_lo, q_hi, lb, ub, dt, qidx):
    """the box of one step for one configuration: lo = clamp((q_lo - q) / dt, lb, ub), hi likewise, on the DoFs that have a finite
    limit; the base box, untouched, on the others.  Returns (lo, hi, flags, inside): flags bit 0 = lo > lb, bit 1 = hi < ub;
    inside = the coordinate is within [q_lo, q_hi]"""
    lo, hi = np.array(lb, dtype=float), np.array(ub, dtype=float)
    lim = (qidx >= 0) & (np.isfinite(q_lo) | np.isfinite(q_hi))
    qj = q[qidx[lim]]
    with np.errstate(all="ignore"):
        lo[lim] = np.minimum(np.maximum((q_lo[lim] - qj) / dt, lb[lim]), ub[lim])
        hi[lim] = np.minimum(np.maximum((q_hi[lim] - qj) / dt, lb[lim]), ub[lim])
    flags = np.zeros(lo.size, dtype=np.int32)
    flags[lo > lb] |= LIMIT_LOWER
    flags[hi < ub] |= LIMIT_UPPER
    inside = np.zeros(lo.size, dtype=bool)
    inside[lim] = (q_lo[lim] <= qj) & (qj <= q_hi[lim])
    return lo, hi, flags, inside


def lockstep_pose_loop_limits(model, prm, q0, H_ref, v_ref, links, A, lb, ub, targets, dt, gain, tol, max_steps, q_lo, q_hi,
                              integrate=P.integrate):
    """pose_numpy.lockstep_pose_loop with joint position limits q_lo / q_hi [nv] (+-inf: none): per step and running instance the
    inner solve sees the box step_box gives, and after the integrate a limited coordinate that was inside its range before the
    step is clamped to it.  lb / ub: [nv] or [B][nv].  Returns lockstep_pose_loop's dict plus limit_flags [B][nv] (of the last
    step that moved the instance).

    The oracle has no "replace the box" call, so every step is
        SolveInit(q, H_ref, v_ref, links, A, bis_max, lo, hi);  UpdateEqConstraint(l_c, b_c) for every c;  Solve(q, -1, None, None)
    ref_solve_init = problem_reset + data_reset(warm_start) + reset_solver + references + box + constraints + FwdPassInit: with
    warm_start on, data_reset keeps w, z, nu, vis, fis, g and nothing touches yis / Aty, and the tailored Solve repeats the same
    data_reset / reset_solver / FwdPassInit anyway.  The one member of the reference's state that SolveInit disturbs is
    bis_inf_norm_, which only grows under UpdateEqConstraint (the quirk the device keeps) but which SolveInit recomputes from the
    bis it is given: hence bis_max, the b of the step with the largest max_c |b_c|_inf so far (0 before the first step, as the
    handle's own SolveInit has it) -- the UpdateEqConstraint calls that follow cannot raise the norm above that running maximum,
    and they leave Ais / AtA / Atb / bis as the plain loop has them.  With warm_start off every solve starts cold in both loops.
    tests/test_pose_limits_oracle.py proves the construction: with infinite limits it is np.array_equal to lockstep_pose_loop."""
    from oracle import ref
    B, nc = q0.shape[0], len(links)
    A = np.asarray(A, dtype=float)
    A_of = (lambda b: A[b]) if A.ndim == 4 else (lambda b: A)
    lb, ub = np.asarray(lb, dtype=float), np.asarray(ub, dtype=float)
    box_of = (lambda b: (lb[b], ub[b])) if lb.ndim == 2 else (lambda b: (lb, ub))
    q_lo, q_hi = np.asarray(q_lo, dtype=float), np.asarray(q_hi, dtype=float)
    qidx = limit_q_index(model)
    assert qidx.size == model.nv == q_lo.size == q_hi.size
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
    solvers, end, bmax = [], np.zeros(B, dtype=np.int32), []
    for b in range(B):
        r = ref.RefSolver(model, **dict(prm, num_eq_c=nc))
        lb_b, ub_b = box_of(b)
        r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), np.zeros((nc, 6)), lb_b, ub_b)
        solvers.append(r)
        bis_max, norm_max = np.zeros((nc, 6)), 0.0
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
            lo, hi, flags[b], inside = step_box(q[b], q_lo, q_hi, lb_b, ub_b, dt, qidx)
            r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), bis_max, lo, hi)
            for c, l in enumerate(links):
                r.UpdateEqConstraint(l, bs[c])
            r.Solve(q[b], -1, None, None)
            if not r.get_convergence_status():
                status[b] |= POSE_NOT_CONVERGED
            if r.get_primal_infeasibility_status():
                status[b] |= POSE_INFEASIBLE
            qn = integrate(model, q[b], dt * r.field("z"))
            ci = qidx[inside]
            qn[ci] = np.clip(qn[ci], q_lo[inside], q_hi[inside])
            q[b] = qn
            steps[b] += 1
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
    return dict(q=q, steps=steps, status=status, reached=(status & POSE_REACHED) != 0, err=err, z=z, iter=it, limit_flags=flags)


def binding_limits(model, q_t, q0, seed, pct=(20.0, 80.0)):
    """limits that bind, for the tests: for a seeded random half of the DoFs that can carry a limit, [q_lo, q_hi] = the interval
    between the pct percentiles of the TARGET configurations q_t over the batch -- so about 40 % of the targets need that
    coordinate outside its range -- and +-inf on every other DoF.  The seeds q0 sit next to their targets (test_pose_parity._seeds),
    so widening the interval until it holds every seed would leave nothing to bind; instead the seeds' limited coordinates are
    clipped into the interval: every instance starts in range.  Returns (q_lo, q_hi, q0 clipped)."""
    rng = np.random.default_rng(seed)
    qidx = limit_q_index(model)
    can = np.flatnonzero(qidx >= 0)
    pick = np.sort(rng.choice(can, size=max(1, can.size // 2), replace=False))
    q_lo, q_hi = -np.inf * np.ones(model.nv), np.inf * np.ones(model.nv)
    q_lo[pick] = np.percentile(q_t[:, qidx[pick]], pct[0], axis=0)
    q_hi[pick] = np.percentile(q_t[:, qidx[pick]], pct[1], axis=0)
    q0 = np.array(q0, dtype=float)
    q0[:, qidx[pick]] = np.clip(q0[:, qidx[pick]], q_lo[pick], q_hi[pick])
    return q_lo, q_hi, q0
