"""The numpy reference of include/loik_amd_plan.h: the RRT-Connect rule of the header restated on motion_numpy.difference and
motion_numpy.advance (the certified check of an edge), pose_numpy.integrate (a step towards a target) and pose_multistart_numpy.words
(the samples).

Every query is a generator that yields the edge it wants checked, (from, to), and is sent the advancement's answer; the driver runs the
queries of a batch side by side, so that one batched advancement serves the pending edge of every query that still runs, edge by edge
as alone.  test_plan_numpy.py proves the rule's claims without a GPU."""
import numpy as np

import grid_numpy as GN
import motion_numpy as MN
import pose_limits_numpy as PL
import pose_multistart_numpy as MS
import pose_numpy as P

FOUND, EXHAUSTED_ITERS, EXHAUSTED_NODES, START_BLOCKED, GOAL_BLOCKED, TOO_LONG, INVALID = range(7)
INT_MAX = 2 ** 31 - 1


def diff(model, x, y):
    """difference(x, y) [nv]; two finite rows that are equal entry by entry are exactly 0 apart"""
    if np.array_equal(x, y):
        return np.zeros(int(model.nv))
    return MN.difference(model, x, y)[0]


def dist2(dv):
    """the squares summed in DoF order, one by one"""
    dv = np.atleast_2d(dv)
    return np.cumsum(dv * dv, axis=1)[:, -1]


def sample(model, seed, r, b, q_start, s_lo, s_hi):
    """q_rand of iteration r of query b: the multi-start sampler's arithmetic on the DoFs with a finite pair, the start row elsewhere"""
    j, c = MS.sampled_dofs(model, s_lo, s_hi)
    q = np.array(q_start, dtype=float)
    u = MS.uniforms(seed, r, b, j)
    prod = u * (s_hi[j] - s_lo[j])          # (numpy rounds the product: it is an array of doubles)
    q[c] = np.minimum(s_lo[j] + prod, s_hi[j])
    return q


def nearest(model, nodes, target):
    """(index, near) of the node with the least dist2 to the target, the lowest index among equals"""
    rows = np.stack(nodes)
    d2 = dist2(MN.difference(model, rows, np.tile(target, (rows.shape[0], 1))))
    d2[np.all(rows == target[None], axis=1)] = 0.0
    k = int(np.argmin(d2))
    rest = np.delete(d2, k)
    return k, bool(rest.size and rest.min() - d2[k] <= MN.NEAR * d2[k])


def _query(model, b, q_start, q_goal, s_lo, s_hi, T, step, max_iters, max_nodes, seed, out):
    """the rule for one query; yields (from, to) per edge and is sent dict(status, s_free, evals, near) of its advancement"""
    info = out["info"][b]
    if not (np.isfinite(q_start).all() and np.isfinite(q_goal).all() and np.isfinite(diff(model, q_start, q_goal)).all()):
        info[0] = INVALID
        return
    nodes, parent = [[q_start.copy()], [q_goal.copy()]], [[-1], [-1]]

    def count(res):
        info[5] += 1
        info[6] += int(res["status"] == MN.FREE)
        info[7] = min(int(info[7]) + int(res["evals"]), INT_MAX)
        out["near"][b] |= bool(res["near"])
        out["edges"][b].append((res["from"], res["to"], int(res["status"])))
        return res["status"] == MN.FREE

    def finish(status, b0=0, b1=0):
        info[0], info[3], info[4] = status, len(nodes[0]), len(nodes[1])
        if status != FOUND:
            return
        chain0, chain1 = [b0], [b1]
        while parent[0][chain0[-1]] >= 0:
            chain0.append(parent[0][chain0[-1]])
        while parent[1][chain1[-1]] >= 0:
            chain1.append(parent[1][chain1[-1]])
        rows = [nodes[0][i] for i in reversed(chain0)] + [nodes[1][i] for i in chain1]
        info[1] = len(rows)
        if len(rows) > T:
            info[0] = TOO_LONG
            return
        out["q_path"][b] = np.stack(rows + [rows[-1]] * (T - len(rows)))

    # 0. the direct segment, then the goal itself
    res = yield (q_start, q_goal)
    if count(res):
        return finish(FOUND)
    if res["status"] == MN.BLOCKED and res["s_free"] == 0.0:
        return finish(START_BLOCKED)
    res = yield (q_goal, q_goal)
    count(res)
    if res["status"] == MN.BLOCKED:
        return finish(GOAL_BLOCKED)

    def extend(t, k, target):
        """step 3 without the check: (the new configuration, reach) of tree t from node k"""
        dv = diff(model, nodes[t][k], target)
        d = float(np.sqrt(dist2(dv)[0]))
        out["near"][b] |= abs(d - step) <= MN.NEAR * (1.0 + step)
        if d <= step:
            return target, True
        return P.integrate(model, nodes[t][k], (step / d) * dv), False

    for r in range(max_iters):
        info[2] = r + 1
        a = r % 2
        q_rand = sample(model, seed, r, b, q_start, s_lo, s_hi)
        k, near = nearest(model, nodes[a], q_rand)
        out["near"][b] |= near
        new, reach = extend(a, k, q_rand)
        if len(nodes[a]) >= max_nodes:
            return finish(EXHAUSTED_NODES)
        if not count((yield (nodes[a][k], new) if a == 0 else (new, nodes[a][k]))):
            continue
        nodes[a].append(np.array(new))
        parent[a].append(k)
        goal, t = nodes[a][-1], 1 - a
        k, near = nearest(model, nodes[t], goal)
        out["near"][b] |= near
        while True:      # (every trip but the last adds a node: at most max_nodes trips)
            new, reach = extend(t, k, goal)
            if not reach and len(nodes[t]) >= max_nodes:
                return finish(EXHAUSTED_NODES)
            if not count((yield (nodes[t][k], new) if t == 0 else (new, nodes[t][k]))):
                break
            if reach:
                return finish(FOUND, *((k, len(nodes[1]) - 1) if t == 0 else (len(nodes[0]) - 1, k)))
            nodes[t].append(np.array(new))
            parent[t].append(k)
            k = len(nodes[t]) - 1
    finish(EXHAUSTED_ITERS)


def plan(model, q_start, q_goal, links, spheres, s_lo, s_hi, T, wspheres=(), wboxes=(), pairs=(), step=0.5, max_iters=256, max_nodes=256, seed=0,
         margin=0.0, tol=1e-3, max_evals=256, grid=None):
    """the rule for q_start, q_goal [B][nq]; grid: a grid_numpy.Grid, whose pairs then join the check of an edge (grid_numpy.advance).  Returns dict(q_path [B][T][nq], status, n_waypoints, iterations [B], nodes [B][2],
    edges_checked, edges_free, evals [B], length [B], near [B] = some decision of the query lay within motion_numpy.NEAR of its threshold,
    edges = per query the list of (from, to, status) checked, in order)"""
    import shortcut_numpy as SN
    q_start, q_goal = np.atleast_2d(np.asarray(q_start, dtype=float)), np.atleast_2d(np.asarray(q_goal, dtype=float))
    s_lo, s_hi = np.broadcast_to(np.asarray(s_lo, dtype=float), (model.nv,)), np.broadcast_to(np.asarray(s_hi, dtype=float), (model.nv,))
    assert np.all(PL.limit_q_index(model)[np.isfinite(s_lo) | np.isfinite(s_hi)] >= 0) and np.any(np.isfinite(s_lo) & np.isfinite(s_hi))
    B, nq = q_start.shape
    out = dict(q_path=np.full((B, T, nq), np.nan), info=np.zeros((B, 8), dtype=np.int64), near=np.zeros(B, dtype=bool), edges=[[] for _ in range(B)])
    gens, pending = {}, {}
    for b in range(B):
        g = _query(model, b, q_start[b], q_goal[b], s_lo, s_hi, T, float(step), max_iters, max_nodes, seed, out)
        try:
            pending[b] = next(g)
            gens[b] = g
        except StopIteration:
            pass
    while pending:
        order = sorted(pending)
        qa = np.stack([pending[b][0] for b in order])
        dv = np.stack([diff(model, *pending[b]) for b in order])
        res = GN.advance_of(grid)(model, qa, dv, links, spheres, wspheres, wboxes, pairs, margin=margin, tol=tol, max_evals=max_evals)
        for i, b in enumerate(order):
            one = {k: res[k][i] for k in ("status", "s_free", "evals", "near")}
            one["from"], one["to"] = pending.pop(b)
            try:
                pending[b] = gens[b].send(one)
            except StopIteration:
                del gens[b]
    info = out.pop("info")
    out.update(status=info[:, 0].astype(np.int32), n_waypoints=info[:, 1].astype(np.int32), iterations=info[:, 2].astype(np.int32),
               nodes=info[:, 3:5].astype(np.int32), edges_checked=info[:, 5].astype(np.int32), edges_free=info[:, 6].astype(np.int32),
               evals=info[:, 7].astype(np.int32))
    out["length"] = np.array([SN._length(model, out["q_path"][b, :out["n_waypoints"][b]]) if out["status"][b] == FOUND else np.nan for b in range(B)])
    return out
