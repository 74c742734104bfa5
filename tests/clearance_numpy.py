"""The numpy reference of include/loik_amd_collision.h: the clearance of a sphere model against a world of spheres and oriented boxes
and against itself, the self-pair list, the ordered minimum with its witness, and the selection rule of the collision-aware multi-start.

Forward kinematics is pose_numpy.fk; the three distance formulas, the pair-list rule and the total order (clearance, ordinal) are
restated from the header.  test_clearance_numpy.py proves them from first principles without a GPU."""
import numpy as np

import pose_numpy as P
import pose_multistart_numpy as M

NONE, WORLD_SPHERE, WORLD_BOX, SELF = 0, 1, 2, 3
MS_GOAL_IN_COLLISION = 8


def sphere_sphere(c1, r1, c2, r2):
    """|c1 - c2| - r1 - r2 (broadcasting over leading axes)"""
    d = np.asarray(c1, dtype=float) - np.asarray(c2, dtype=float)
    return np.sqrt((d * d).sum(axis=-1)) - r1 - r2


def sphere_box(c, r, box15):
    """the signed distance of the centre c [..., 3] to the oriented box (R row-major, t, h), less r: negative inside"""
    box15 = np.asarray(box15, dtype=float)
    R, t, h = box15[:9].reshape(3, 3), box15[9:12], box15[12:15]
    p = (np.asarray(c, dtype=float) - t) @ R          # R^T (c - t), row-wise
    d = np.abs(p) - h
    out = np.maximum(d, 0.0)
    return np.sqrt((out * out).sum(axis=-1)) + np.minimum(d.max(axis=-1), 0.0) - r


def box15(T44, h):
    T44 = np.asarray(T44, dtype=float)
    return np.concatenate([T44[:3, :3].reshape(9), T44[:3, 3], np.asarray(h, dtype=float).reshape(3)])


def self_pairs(parents, links, ignore=()):
    """the list of sphere pairs (a < b), lexicographic: the links differ, neither is the other's parent in `parents` (the caller's
    tree, parents[0] unused), the link pair is not in ignore (either order)"""
    skip = {(int(i), int(j)) for i, j in ignore} | {(int(j), int(i)) for i, j in ignore}
    par = [-1] + [int(p) for p in list(parents)[1:]]
    out = []
    for a in range(len(links)):
        for b in range(a + 1, len(links)):
            la, lb = int(links[a]), int(links[b])
            if la == lb or par[la] == lb or par[lb] == la or (la, lb) in skip:
                continue
            out.append((a, b))
    return out


def make_spheres(model, k, seed, links=None):
    """k spheres per link (all links of the model but the universe, or `links`), deterministic: offsets within 0.1 of the link origin,
    radii 0.02 .. 0.08.  Returns (links [ns] int32, spheres [ns][4])"""
    rng = np.random.default_rng(seed)
    links = list(range(1, model.njoints)) if links is None else [int(l) for l in links]
    lk, sph = [], []
    for l in links:
        for _ in range(k):
            v = rng.normal(size=3)
            v *= 0.1 * rng.uniform() ** (1.0 / 3.0) / np.linalg.norm(v)
            lk.append(l)
            sph.append([v[0], v[1], v[2], rng.uniform(0.02, 0.08)])
    return np.array(lk, dtype=np.int32), np.array(sph, dtype=float).reshape(-1, 4)


def centres(model, q, links, spheres):
    """world centres [n][ns][3] of the spheres for configurations q [n][nq]"""
    q = np.atleast_2d(np.asarray(q, dtype=float))
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    out = np.empty((q.shape[0], len(links), 3))
    cache = {}
    for s, l in enumerate(links):
        l = int(l)
        if l not in cache:
            cache[l] = (np.broadcast_to(np.eye(3), (q.shape[0], 3, 3)), np.zeros((q.shape[0], 3))) if l == 0 else P.fk(model, q, l)
        R, t = cache[l]
        out[:, s] = t + np.einsum("bij,j->bi", R, spheres[s, :3])
    return out


def pair_table(cen, radii, wspheres, wboxes, pairs):
    """every pair clearance in ordinal order: (values [n][npairs_total], kinds [..], a [..], b [..]).  World spheres first, a major and
    b minor, then world boxes likewise, then the self pairs in list order"""
    n, ns = cen.shape[:2]
    wspheres = np.asarray(wspheres, dtype=float).reshape(-1, 4)
    wboxes = np.asarray(wboxes, dtype=float).reshape(-1, 15)
    vals, kinds, ia, ib = [], [], [], []
    for a in range(ns):
        for o in range(wspheres.shape[0]):
            vals.append(sphere_sphere(cen[:, a], radii[a], wspheres[o, :3], wspheres[o, 3]))
            kinds.append(WORLD_SPHERE); ia.append(a); ib.append(o)
    for a in range(ns):
        for o in range(wboxes.shape[0]):
            vals.append(sphere_box(cen[:, a], radii[a], wboxes[o]))
            kinds.append(WORLD_BOX); ia.append(a); ib.append(o)
    for a, b in pairs:
        vals.append(sphere_sphere(cen[:, a], radii[a], cen[:, b], radii[b]))
        kinds.append(SELF); ia.append(a); ib.append(b)
    v = np.stack(vals, axis=1) if vals else np.zeros((n, 0))
    return v, np.array(kinds, dtype=np.int32), np.array(ia, dtype=np.int32), np.array(ib, dtype=np.int32)


def ordered_min(values):
    """the index of the minimum of a row in (value, ordinal), a NaN after every number; -1 for an empty row"""
    values = np.asarray(values, dtype=float)
    if values.size == 0:
        return -1
    key = np.where(np.isnan(values), np.inf, values)
    nan = np.isnan(values)
    order = sorted(range(values.size), key=lambda i: (bool(nan[i]), float(key[i]), i))
    return order[0]


def clearance(model, q, links, spheres, wspheres=(), wboxes=(), pairs=()):
    """dict(min [n], min_world [n], min_self [n], witness [n][3], table = pair_table) as BatchedLoik.clearance returns it"""
    q = np.atleast_2d(np.asarray(q, dtype=float))
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    n = q.shape[0]
    cen = centres(model, q, links, spheres)
    v, kinds, ia, ib = pair_table(cen, spheres[:, 3], wspheres, wboxes, list(pairs))
    out = dict(min=np.full(n, np.inf), min_world=np.full(n, np.inf), min_self=np.full(n, np.inf),
               witness=np.tile(np.array([NONE, -1, -1], dtype=np.int32), (n, 1)), table=(v, kinds, ia, ib), centres=cen)
    world = kinds != SELF
    bad = ~np.isfinite(q).all(axis=1)
    for i in range(n):
        if bad[i]:
            out["min"][i] = out["min_world"][i] = out["min_self"][i] = np.nan
            continue
        k = ordered_min(v[i])
        if k >= 0:
            out["min"][i] = v[i, k]
            out["witness"][i] = (kinds[k], ia[k], ib[k])
        if world.any():
            out["min_world"][i] = v[i, world].min()
        if (~world).any():
            out["min_self"][i] = v[i, ~world].min()
    return out


def witness_value(table, i, wit):
    """the oracle's clearance of the pair a witness names, for configuration i"""
    v, kinds, ia, ib = table
    k = np.flatnonzero((kinds == wit[0]) & (ia == wit[1]) & (ib == wit[2]))
    assert k.size == 1, wit
    return float(v[i, k[0]])


# ---- the collision-aware multi-start ---------------------------------------------------------------------------------------------
# classes as sort keys: 0 reached and clear, 0.5 reached in collision (0c), 1 out of steps, 2 stopped
def ms_keys(cls, cost, status, clr, margin):
    """(class [B], cost [B]) of the latched selection from those of pose_multistart_numpy.instance_keys: a REACHED, not STOPPED instance
    with !(clr >= margin) moves to class 0.5 with the cost -clr"""
    cls, cost = np.array(cls, dtype=float), np.array(cost, dtype=float)
    clr = np.asarray(clr, dtype=float)
    with np.errstate(invalid="ignore"):
        colliding = (cls == 0) & ~(clr >= margin)
    cls[colliding] = 0.5
    cost[colliding] = -clr[colliding]
    return cls, cost


def ms_select(cls, cost, K):
    """the lexicographic minimum of (class, cost, b) per goal, a NaN after every number, ties to the lowest b.  Returns dict(winner [G],
    goal_status [G], cost [G], nclear [G])"""
    cls, cost = np.asarray(cls, dtype=float), np.asarray(cost, dtype=float)
    G = cls.size // K
    out = dict(winner=np.zeros(G, dtype=np.int32), goal_status=np.zeros(G, dtype=np.int32), cost=np.zeros(G), nclear=np.zeros(G, dtype=np.int32))
    status_of = {0.0: M_GOAL[0], 0.5: MS_GOAL_IN_COLLISION, 1.0: M_GOAL[1], 2.0: M_GOAL[2]}
    for g in range(G):
        keys = []
        for b in range(g * K, (g + 1) * K):
            nan = bool(np.isnan(cost[b]))
            keys.append((float(cls[b]), nan, 0.0 if nan else float(cost[b]), b))
        keys.sort()
        b = keys[0][3]
        out["winner"][g], out["goal_status"][g], out["cost"][g] = b, status_of[float(cls[b])], cost[b]
        out["nclear"][g] = int((cls[g * K:(g + 1) * K] == 0).sum())
    return out


M_GOAL = (1, 2, 4)   # LOIKB_MS_GOAL_REACHED / BEST_EFFORT / FAILED


def ms_loop_status(status, clr, margin):
    """the loop-private status word of the re-sampler: REACHED cleared on class 0c"""
    status = np.array(status)
    clr = np.asarray(clr, dtype=float)
    with np.errstate(invalid="ignore"):
        colliding = ((status & M.POSE_REACHED) != 0) & ((status & M.POSE_STOPPED) == 0) & ~(clr >= margin)
    status[colliding] &= ~M.POSE_REACHED
    return status
