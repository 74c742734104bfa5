"""The numpy reference of include/loik_amd_avoid.h: each sphere's nearest world object and nearest self partner, the unit normal and
the gradient row of a pair clearance, the inscribed velocity box, and the lock-step pose loop with that box.

Centres and the three distance formulas are clearance_numpy's; Jc is the linear part of jacobian_numpy.frame_jacobians
(local_world_aligned) of a frame at the sphere's centre; the step box under the avoidance box and the loop around it are
pose_limits_numpy's.  The normals, m, r and the box rule are restated from the header.  test_avoid_numpy.py proves them from first
principles without a GPU.

Every decision of the rule that hangs on a comparison of floating-point numbers is reported in a `near` mask: a configuration is near
when a reference decision lies within NEAR of its threshold, so that a correctly rounded device may decide the other way."""
import numpy as np

import clearance_numpy as CN
import jacobian_numpy as JN
import pose_limits_numpy as PL
import pose_numpy as P
import qp_numpy as QP
from pose_numpy import POSE_INFEASIBLE, POSE_NOT_CONVERGED, POSE_REACHED, POSE_STOPPED

NEAR = 1e-9
_PATHS = {}


def path_dofs(model, link):
    """bool [nv]: the DoFs structurally on the root path of `link` -- the columns of its 6-row joint Jacobian at a generic
    configuration that are not zero (the twist of a joint never vanishes)"""
    if id(model) not in _PATHS:   # (every link in one call)
        q = model.random_configurations(np.random.default_rng(7), 1)
        _PATHS[id(model)] = (model, np.any(QP.jacobians(model, q)[0] != 0.0, axis=1))
    return _PATHS[id(model)][1][int(link)]


def pair_dofs(model, la, lb=None):
    """the DoFs on the pair's path: the root path of la (a world pair), or the symmetric difference of the two root paths"""
    return path_dofs(model, la) if lb is None else path_dofs(model, la) ^ path_dofs(model, lb)


def normal_sphere(c, w):
    """(n, |c - w|): n = (c - w) / |c - w|, 0 at coincidence"""
    e = np.asarray(c, dtype=float) - np.asarray(w, dtype=float)
    d = float(np.sqrt((e * e).sum()))
    return (e / d if d != 0.0 else np.zeros(3)), d


def normal_box(c, box15):
    """(n, gap): the outward normal of the signed distance of c to the oriented box; gap = inside the box the distance between the
    largest and the second largest of d = |p| - h (the argmax decision), +inf outside"""
    box15 = np.asarray(box15, dtype=float)
    R, t, h = box15[:9].reshape(3, 3), box15[9:12], box15[12:15]
    p = R.T @ (np.asarray(c, dtype=float) - t)
    d = np.abs(p) - h
    sgn = np.where(p >= 0.0, 1.0, -1.0)
    if np.any(d > 0.0):
        o = np.maximum(d, 0.0)
        return R @ (sgn * o / np.sqrt((o * o).sum())), np.inf
    k = int(np.argmax(d))   # (the lowest index that attains the maximum)
    v = np.zeros(3)
    v[k] = sgn[k]
    s = np.sort(d)
    return R @ v, float(s[2] - s[1])


def nearest(model, q, links, spheres, ws=(), wb=(), pairs=()):
    """each sphere's nearest world object and nearest listed self partner (first index = the sphere), in the total order (clearance,
    ordinal).  Returns dict(pairs [n][ns][2] (+inf: empty set, NaN: q not finite), partner [n][ns][2] int (world sphere o, nws + box o, the
    other sphere; -1), second [n][ns][2] the runner-up clearance (+inf: none), centres [n][ns][3])"""
    q = np.atleast_2d(np.asarray(q, dtype=float))
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    ws = np.asarray(ws, dtype=float).reshape(-1, 4)
    wb = np.asarray(wb, dtype=float).reshape(-1, 15)
    n, ns = q.shape[0], spheres.shape[0]
    bad = ~np.isfinite(q).all(axis=1)
    with np.errstate(all="ignore"):
        cen = CN.centres(model, np.where(bad[:, None], 0.0, q), links, spheres)
    val = np.full((n, ns, 2), np.inf)
    par = -np.ones((n, ns, 2), dtype=np.int32)
    sec = np.full((n, ns, 2), np.inf)
    firsts = {}
    for a, b in pairs:
        firsts.setdefault(int(a), []).append(int(b))
    for a in range(ns):
        cols = [CN.sphere_sphere(cen[:, a], spheres[a, 3], ws[o, :3], ws[o, 3]) for o in range(ws.shape[0])]
        cols += [CN.sphere_box(cen[:, a], spheres[a, 3], wb[o]) for o in range(wb.shape[0])]
        for kind, cols, names in ((0, cols, None), (1, [CN.sphere_sphere(cen[:, a], spheres[a, 3], cen[:, b], spheres[b, 3]) for b in firsts.get(a, [])],
                                                    firsts.get(a, []))):
            if not cols:
                continue
            v = np.stack(cols, axis=1)
            k = np.argmin(v, axis=1)   # (the first of equal minima: the lowest ordinal)
            val[:, a, kind] = v[np.arange(n), k]
            par[:, a, kind] = k if names is None else np.asarray(names)[k]
            if v.shape[1] > 1:
                sec[:, a, kind] = np.partition(v, 1, axis=1)[:, 1]
    val[bad] = np.nan
    par[bad] = -1
    return dict(pairs=val, partner=par, second=sec, centres=cen, bad=bad)


def centre_jacobians(model, q_row, links, spheres, which):
    """{a: the 3 x nv linear part of the local_world_aligned Jacobian of a frame at the centre of sphere a} for the spheres `which`, from
    one call of jacobian_numpy.frame_jacobians; a sphere on link 0 moves with no DoF"""
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    out = {int(a): np.zeros((3, model.nv)) for a in which if int(links[a]) == 0}
    todo = sorted({int(a) for a in which} - set(out))
    if todo:
        frames = np.stack([np.concatenate([np.eye(3).reshape(9), spheres[a, :3]]) for a in todo])
        J = JN.frame_jacobians(model, q_row[None], [int(links[a]) for a in todo], frames=frames, reference="local_world_aligned")[0]
        out.update({a: J[k, :3] for k, a in enumerate(todo)})
    return out


def _jc(model, q_row, links, spheres, a, jc=None):
    return jc[int(a)] if jc is not None and int(a) in jc else centre_jacobians(model, q_row, links, spheres, [a])[int(a)]


def pair_gradient(model, q_row, links, spheres, ws, wb, jc, a, kind, partner, cen_row):
    """(n, g [nv], m, near) of the pair of sphere a with `partner` (kind 0: a world object, 1: the other sphere); jc: centre_jacobians of
    the row when the caller has them"""
    ws = np.asarray(ws, dtype=float).reshape(-1, 4)
    wb = np.asarray(wb, dtype=float).reshape(-1, 15)
    near = False
    if kind == 1:
        nrm, dist = normal_sphere(cen_row[a], cen_row[partner])
        near = dist < NEAR
        g = nrm @ (_jc(model, q_row, links, spheres, a, jc) - _jc(model, q_row, links, spheres, partner, jc))
        g[path_dofs(model, links[a]) & path_dofs(model, links[partner])] = 0.0
        on = pair_dofs(model, links[a], links[partner])
    else:
        if partner < ws.shape[0]:
            nrm, dist = normal_sphere(cen_row[a], ws[partner, :3])
            near = dist < NEAR
        else:
            nrm, gap = normal_box(cen_row[a], wb[partner - ws.shape[0]])
            near = gap < NEAR
        g = nrm @ _jc(model, q_row, links, spheres, a, jc)
        on = pair_dofs(model, links[a])
    return nrm, g, int(on.sum()), bool(near)


def constraints(model, q, links, spheres, ws, wb, pairs, d_influence, table=None, d_safe=None):
    """the active constraints of every configuration: a list per row of dict(a, kind, partner, d, n, g, m), and near [n] bool"""
    q = np.atleast_2d(np.asarray(q, dtype=float))
    t = nearest(model, q, links, spheres, ws, wb, pairs) if table is None else table
    out, near = [], np.zeros(q.shape[0], dtype=bool)
    for i in range(q.shape[0]):
        row = []
        if not t["bad"][i]:
            v, s = t["pairs"][i], t["second"][i]
            with np.errstate(invalid="ignore"):   # (inf - inf where a sphere has no object or no partner)
                near[i] = bool(np.any(np.abs(v - d_influence) < NEAR)) or bool(np.any((v < d_influence) & (s < d_influence) & (s - v < NEAR)))
            act = [(a, kind) for a in range(v.shape[0]) for kind in (0, 1) if v[a, kind] < d_influence]
            jc = centre_jacobians(model, q[i], links, spheres, [a for a, _ in act] + [int(t["partner"][i, a, 1]) for a, kind in act if kind == 1])
            for a in range(v.shape[0]):
                for kind in (0, 1):
                    if v[a, kind] < d_influence:
                        nrm, g, m, nr = pair_gradient(model, q[i], links, spheres, ws, wb, jc, a, kind, int(t["partner"][i, a, kind]), t["centres"][i])
                        # (two more comparisons of the rule: max(d - d_safe, 0) when the caller names d_safe, and the sign of g_kj)
                        near[i] |= nr or bool(np.any((g != 0.0) & (np.abs(g) < NEAR))) or (d_safe is not None and abs(v[a, kind] - d_safe) < NEAR)
                        row.append(dict(a=a, kind=kind, partner=int(t["partner"][i, a, kind]), d=float(v[a, kind]), n=nrm, g=g, m=m))
        out.append(row)
    return out, near, t


def narrow(cons, lo, hi, d_safe, kappa, dt):
    """the box rule for one configuration: (lo', hi', A_lo, A_hi, r [k]) from its active constraints and the step's interval [lo, hi]"""
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    A_lo, A_hi = np.full(lo.size, -np.inf), np.full(lo.size, np.inf)
    rs = []
    for c in cons:
        r = kappa * max(c["d"] - d_safe, 0.0) / dt
        rs.append(r)
        g = c["g"]
        pos, neg = g > 0.0, g < 0.0
        A_lo[pos] = np.maximum(A_lo[pos], -r / (c["m"] * g[pos]))
        A_hi[neg] = np.minimum(A_hi[neg], r / (c["m"] * np.abs(g[neg])))
    return np.minimum(np.maximum(A_lo, lo), hi), np.minimum(np.maximum(A_hi, lo), hi), A_lo, A_hi, np.array(rs)


def avoidance_box(model, q, links, spheres, ws, wb, pairs, dt, lb, ub, d_safe, d_influence, kappa):
    """BatchedLoik.avoidance_box: dict(lo [n][nv], hi [n][nv], pairs, partner, near [n], cons)"""
    q = np.atleast_2d(np.asarray(q, dtype=float))
    lb, ub = np.broadcast_to(np.asarray(lb, dtype=float), (model.nv,)), np.broadcast_to(np.asarray(ub, dtype=float), (model.nv,))
    cons, near, t = constraints(model, q, links, spheres, ws, wb, pairs, d_influence, d_safe=d_safe)
    lo, hi = np.empty((q.shape[0], model.nv)), np.empty((q.shape[0], model.nv))
    for i in range(q.shape[0]):
        lo[i], hi[i] = narrow(cons[i], lb, ub, d_safe, kappa, dt)[:2]
    return dict(lo=lo, hi=hi, pairs=t["pairs"], partner=t["partner"], near=near, cons=cons, centres=t["centres"])


def clearance_gradient(model, q, links, spheres, ws=(), wb=(), pairs=()):
    """BatchedLoik.clearance_gradient: clearance_numpy.clearance plus grad [n][nv] of the witness pair, and near [n]: the runner-up of the
    overall minimum is within NEAR, or the pair's own decision (|c - w|, the argmax inside a box) is"""
    q = np.atleast_2d(np.asarray(q, dtype=float))
    out = CN.clearance(model, q, links, spheres, ws, wb, pairs)
    nws = np.asarray(ws, dtype=float).reshape(-1, 4).shape[0]
    grad, near = np.zeros((q.shape[0], model.nv)), np.zeros(q.shape[0], dtype=bool)
    v = out["table"][0]
    for i in range(q.shape[0]):
        kind, a, b = (int(x) for x in out["witness"][i])
        if not np.isfinite(q[i]).all():
            grad[i] = np.nan
            continue
        if kind == CN.NONE:
            continue
        partner = b if kind != CN.WORLD_BOX else nws + b
        _, grad[i], _, nr = pair_gradient(model, q[i], links, spheres, ws, wb, None, a, 1 if kind == CN.SELF else 0, partner, out["centres"][i])
        s = np.sort(v[i])
        near[i] = nr or (s.size > 1 and s[1] - s[0] < NEAR)
    out.update(grad=grad, near=near)
    return out


def constraints_of(model, q, col, avoid):
    """constraints() of a pose loop's collision model col = dict(links, spheres, ws, wb, pairs[, grid]).  With a voxel grid in it
    (col["grid"], a gridnear_numpy.Grid): gridnear_numpy.constraints, the grid one more world object, clamped as a pose loop clamps.
    Without one, or with grid = None, the very call this function replaced"""
    if col.get("grid") is not None:
        import gridnear_numpy as NN   # (it imports this module)
        return NN.constraints(model, q, col["links"], col["spheres"], col["ws"], col["wb"], col["pairs"], avoid["d_influence"], col["grid"],
                              d_safe=avoid["d_safe"], clamped=True)
    return constraints(model, q, col["links"], col["spheres"], col["ws"], col["wb"], col["pairs"], avoid["d_influence"], d_safe=avoid["d_safe"])


def narrower(model, col, avoid, dt, B):
    """the `narrow` hook of pose_path_numpy.lockstep_path_loop, pose_track_numpy.lockstep_track_loop and
    pose_step_numpy.lockstep_pose_loop_step: a callable narrow(b, q_b, lo, hi) -> (lo2, hi2) that narrows the step's interval as
    lockstep_pose_loop_avoid does and accumulates, in its attribute `results`, that function's avoid_min_seen [B], avoid_active_steps
    [B], avoid_flags [B][nv] (of the last call for the instance) and near [B].  One call = one step the instance ran."""
    res = dict(avoid_min_seen=np.full(B, np.inf), avoid_active_steps=np.zeros(B, dtype=np.int32),
               avoid_flags=np.zeros((B, model.nv), dtype=np.int32), near=np.zeros(B, dtype=bool))

    def narrow_step(b, q_b, lo, hi):
        cons, nr, t = constraints_of(model, q_b[None], col, avoid)
        res["near"][b] |= bool(nr[0])
        res["avoid_min_seen"][b] = min(res["avoid_min_seen"][b], float(np.min(t["pairs"][0])))
        nlo, nhi = narrow(cons[0], lo, hi, avoid["d_safe"], avoid["kappa"], dt)[:2]
        res["avoid_flags"][b] = (nlo > lo).astype(np.int32) | ((nhi < hi).astype(np.int32) << 1)
        res["avoid_active_steps"][b] += int(np.any(res["avoid_flags"][b] != 0))
        return nlo, nhi

    narrow_step.results = res
    return narrow_step


def lockstep_pose_loop_avoid(model, prm, q0, H_ref, v_ref, links, A, lb, ub, targets, dt, gain, tol, max_steps, q_lo, q_hi, col, avoid,
                             a_max=None, integrate=P.integrate):
    """pose_limits_numpy.lockstep_pose_loop_limits with the avoidance box of include/loik_amd_avoid.h behind the step box: per step and
    running instance the inner solve sees narrow(constraints(q), step_box(q)).  col = dict(links, spheres, ws, wb, pairs), avoid =
    dict(d_safe, d_influence, kappa); with a_max [nv] the step box is pose_accel_numpy.dyn_box from rest instead.  Every step re-enters SolveInit, as lockstep_pose_loop_limits does and for the reason its
    docstring gives.  Returns its dict plus avoid_min_seen [B], avoid_active_steps [B], avoid_flags [B][nv], near [B] (the run touched a
    near configuration) and q_path: a list per instance of the step-start configurations (the final one included)."""
    from oracle import ref
    B, nc = q0.shape[0], len(links)
    A = np.asarray(A, dtype=float)
    A_of = (lambda b: A[b]) if A.ndim == 4 else (lambda b: A)
    lb, ub = np.asarray(lb, dtype=float), np.asarray(ub, dtype=float)
    box_of = (lambda b: (lb[b], ub[b])) if lb.ndim == 2 else (lambda b: (lb, ub))
    q_lo, q_hi = np.asarray(q_lo, dtype=float), np.asarray(q_hi, dtype=float)
    qidx = PL.limit_q_index(model)
    ids = np.asarray(links, dtype=np.int32)
    k = gain / dt
    q = np.array(q0, dtype=float)
    steps, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    err, z, it = np.zeros((B, nc, 6)), np.zeros((B, model.nv)), np.zeros(B, dtype=np.int32)
    flags, aflags = np.zeros((B, model.nv), dtype=np.int32), np.zeros((B, model.nv), dtype=np.int32)
    min_seen, asteps, near, paths = np.full(B, np.inf), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=bool), []
    solvers, end, bmax = [], np.zeros(B, dtype=np.int32), []
    for b in range(B):
        r = ref.RefSolver(model, **dict(prm, num_eq_c=nc))
        lb_b, ub_b = box_of(b)
        r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), np.zeros((nc, 6)), lb_b, ub_b)
        solvers.append(r)
        bis_max, norm_max = np.zeros((nc, 6)), 0.0
        path = []
        zp = np.zeros(model.nv)
        for step in range(max_steps + 1):
            end[b] = step
            path.append(q[b].copy())
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
            if a_max is None:
                lo, hi, flags[b], inside = PL.step_box(q[b], q_lo, q_hi, lb_b, ub_b, dt, qidx)
            else:
                import pose_accel_numpy as PA
                lo, hi, flags[b], inside = PA.dyn_box(q[b], zp, np.asarray(a_max, dtype=float), q_lo, q_hi, lb_b, ub_b, dt, qidx)
            cons, nr, t = constraints_of(model, q[b:b + 1], col, avoid)
            near[b] |= bool(nr[0])
            min_seen[b] = min(min_seen[b], float(np.min(t["pairs"][0])))
            nlo, nhi = narrow(cons[0], lo, hi, avoid["d_safe"], avoid["kappa"], dt)[:2]
            aflags[b] = (nlo > lo).astype(np.int32) | ((nhi < hi).astype(np.int32) << 1)
            asteps[b] += int(np.any(aflags[b] != 0))
            r.SolveInit(q[b], H_ref, v_ref, ids, A_of(b), bis_max, nlo, nhi)
            for c, l in enumerate(links):
                r.UpdateEqConstraint(l, bs[c])
            r.Solve(q[b], -1, None, None)
            if not r.get_convergence_status():
                status[b] |= POSE_NOT_CONVERGED
            if r.get_primal_infeasibility_status():
                status[b] |= POSE_INFEASIBLE
            zp = np.array(r.field("z"), dtype=float)
            qn = integrate(model, q[b], dt * zp)
            ci = qidx[inside]
            qn[ci] = np.clip(qn[ci], q_lo[inside], q_hi[inside])
            q[b] = qn
            steps[b] += 1
        bmax.append(bis_max)
        paths.append(np.array(path))
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
                avoid_min_seen=min_seen, avoid_active_steps=asteps, avoid_flags=aflags, near=near, q_path=paths)
