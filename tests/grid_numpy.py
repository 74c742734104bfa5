"""The numpy reference of include/loik_amd_grid.h: the distance field of an occupancy grid (by brute force over the occupied voxels and by
the three min-plus passes of the header), the pair of a robot sphere against the grid, the exact distance to the union of the occupied
cubes that the pair bounds from below, and the clearance and the conservative advancement with the grid pairs in their place in the
ordinal order.

Centres, the motion bound, the interpolation and the values of every other pair are clearance_numpy's and motion_numpy's;
test_grid_numpy.py proves the claims of the header about the field and the pair without a GPU."""
import numpy as np

import clearance_numpy as CN
import motion_numpy as MN

WORLD_GRID = 4
EMPTY = 0xFFFFFFFF
FACE = MN.NEAR   # a centre this close (in voxels) to a voxel face may read the voxel on its other side on the device


class Grid:
    """occ [nz][ny][nx] (nonzero = occupied), origin [3] the low corner of voxel (0, 0, 0), h the edge; G the field (brute force)"""

    def __init__(self, occ, origin, h, G=None):
        self.occ = (np.asarray(occ) != 0)
        assert self.occ.ndim == 3
        self.origin = np.asarray(origin, dtype=float).reshape(3)
        self.h = float(h)
        self.inv_h = 1.0 / self.h
        self.n = np.array(self.occ.shape[::-1], dtype=np.int64)            # nx, ny, nz
        self.hi = self.origin + self.n.astype(float) * self.h              # product first, then the sum
        self.G = field_brute(self.occ) if G is None else np.asarray(G, dtype=np.uint32)


def g(d):
    d = np.abs(np.asarray(d, dtype=np.int64))
    return np.where(d == 0, 0, (2 * d - 1) ** 2)


def field_brute(occ):
    """G [nz][ny][nx] uint32: the minimum over all occupied voxels, one by one"""
    occ = np.asarray(occ) != 0
    nz, ny, nx = occ.shape
    out = np.full(occ.shape, EMPTY, dtype=np.int64)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    for uz, uy, ux in np.argwhere(occ):
        out = np.minimum(out, g(z - uz) + g(y - uy) + g(x - ux))
    return out.astype(np.uint32)


def field_passes(occ):
    """the same by the three min-plus passes of the header, along x, then y, then z, in integers"""
    occ = np.asarray(occ) != 0
    far = np.int64(1) << 40
    G = np.where(occ, 0, far).astype(np.int64)
    for axis in (2, 1, 0):
        n = G.shape[axis]
        k = np.arange(n)
        cost = g(k[:, None] - k[None, :])                                   # [out][in]
        Gm = np.moveaxis(G, axis, -1)
        G = np.moveaxis((Gm[..., None, :] + cost).min(axis=-1), -1, axis)
    return np.where(G >= far, EMPTY, G).astype(np.uint32)


def sphere_grid(c, r, grid):
    """(v, voxel): the pair of the header for centres c [..., 3] and radii r (broadcast), and the linear index of the voxel read"""
    c = np.asarray(c, dtype=float)
    p = np.minimum(np.maximum(c, grid.origin), grid.hi)
    with np.errstate(invalid="ignore"):
        i = np.minimum(np.maximum(np.floor((p - grid.origin) * grid.inv_h), 0.0), (grid.n - 1).astype(float))
    i = np.where(np.isnan(i), 0, i).astype(np.int64)
    x = grid.origin + (i + 0.5) * grid.h
    Gv = grid.G[i[..., 2], i[..., 1], i[..., 0]]
    with np.errstate(invalid="ignore"):
        m = np.where(Gv == EMPTY, np.inf, (0.5 * grid.h) * np.sqrt(Gv.astype(float)) - np.sqrt(((p - x) ** 2).sum(axis=-1)))
        dout = np.sqrt(((c - p) ** 2).sum(axis=-1))
        mp = np.maximum(m, 0.0)
        v = np.where(dout > 0, np.sqrt(dout * dout + mp * mp), m) - r
    vox = (i[..., 2] * grid.n[1] + i[..., 1]) * grid.n[0] + i[..., 0]
    return v, vox


def near_face(c, grid):
    """[...]: some centre of c [..., ns, 3] has a component whose clamped value, measured in voxels from the origin, lies within FACE of
    an integer k with 0 < k < n: a face between two voxels, where a rounding difference reads the other voxel and the pair jumps.  The
    two faces of the grid's box (k = 0 and k = n, where every clamped component of a centre outside the box lies) are no such place: the
    index is clamped to 0 and to n - 1 on both sides of them"""
    c = np.asarray(c, dtype=float)
    with np.errstate(invalid="ignore"):
        t = (np.minimum(np.maximum(c, grid.origin), grid.hi) - grid.origin) * grid.inv_h
        k = np.rint(t)
        hit = (np.abs(t - k) <= FACE) & (k > 0) & (k < grid.n)
    return hit.any(axis=(-1, -2))


def advance_of(grid):
    """the advancement that shortcut_numpy and plan_numpy call: motion_numpy.advance without a grid, advance (below) with one, under
    motion_numpy.advance's signature"""
    if grid is None:
        return MN.advance
    return lambda model, qa, dv, links, spheres, wspheres=(), wboxes=(), pairs=(), **kw: advance(model, qa, dv, links, spheres, wspheres, wboxes, grid, pairs, **kw)


def cubes(grid):
    """the occupied voxels as boxes [k][15] of clearance_numpy.sphere_box"""
    out = []
    for uz, uy, ux in np.argwhere(grid.occ):
        ctr = grid.origin + (np.array([ux, uy, uz]) + 0.5) * grid.h
        out.append(np.concatenate([np.eye(3).reshape(9), ctr, np.full(3, 0.5 * grid.h)]))
    return np.array(out).reshape(-1, 15)


def exact_distance(c, grid, boxes=None):
    """the signed distance of centres c [..., 3] to the union of the occupied cubes: positive outside, where it is the exact distance;
    <= 0 inside.  +inf without an occupied voxel"""
    boxes = cubes(grid) if boxes is None else boxes
    c = np.asarray(c, dtype=float)
    out = np.full(c.shape[:-1], np.inf)
    for b in boxes:
        out = np.minimum(out, CN.sphere_box(c, 0.0, b))
    return out


def pair_values(cen, radii, ws, wb, grid, pairs):
    """every pair clearance [B][npairs_total] in ordinal order: world spheres, world boxes, the ns grid pairs, the self pairs.  Also the
    voxel each grid pair read, [B][ns]"""
    B, ns = cen.shape[:2]
    world = MN.pair_values(cen, radii, ws, wb, [])
    self_ = MN.pair_values(cen, radii, ws[:0], wb[:0], pairs)
    if grid is None:
        return np.concatenate([world, self_], axis=1), np.zeros((B, 0), dtype=np.int64)
    gv, vox = sphere_grid(cen, radii[None, :], grid)
    return np.concatenate([world, gv, self_], axis=1), vox


def pair_names(ns, nws, nwb, grid, pairs):
    """(kind, a, b) [npairs_total][3] of every ordinal; b of a grid pair is -1 here: the voxel depends on the configuration"""
    rows = [(CN.WORLD_SPHERE, a, o) for a in range(ns) for o in range(nws)] + [(CN.WORLD_BOX, a, o) for a in range(ns) for o in range(nwb)]
    if grid is not None:
        rows += [(WORLD_GRID, a, -1) for a in range(ns)]
    rows += [(CN.SELF, int(a), int(b)) for a, b in pairs]
    return np.array(rows, dtype=np.int32).reshape(-1, 3)


def _name(names, o, vox_row):
    if o < 0:
        return (CN.NONE, -1, -1)
    k, a, b = names[o]
    return (k, a, int(vox_row[a])) if k == WORLD_GRID else (k, a, b)


def clearance(model, q, links, spheres, wspheres=(), wboxes=(), grid=None, pairs=()):
    """dict(min [n], min_world [n], min_self [n], witness [n][3], values [n][npairs_total], names, voxels [n][ns], centres) as
    BatchedLoik.clearance returns it with a grid set"""
    q = np.atleast_2d(np.asarray(q, dtype=float))
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    ws, wb = np.asarray(wspheres, dtype=float).reshape(-1, 4), np.asarray(wboxes, dtype=float).reshape(-1, 15)
    pairs = list(pairs)
    n, ns = q.shape[0], spheres.shape[0]
    bad = ~np.isfinite(q).all(axis=1)
    cen = MN.centres(model, np.where(bad[:, None], 0.0, q), links, spheres)
    V, vox = pair_values(cen, spheres[:, 3], ws, wb, grid, pairs)
    names = pair_names(ns, ws.shape[0], wb.shape[0], grid, pairs)
    world = names[:, 0] != CN.SELF
    out = dict(min=np.full(n, np.inf), min_world=np.full(n, np.inf), min_self=np.full(n, np.inf),
               witness=np.tile(np.array([CN.NONE, -1, -1], dtype=np.int32), (n, 1)), values=V, names=names, voxels=vox, centres=cen)
    for i in range(n):
        if bad[i]:
            out["min"][i] = out["min_world"][i] = out["min_self"][i] = np.nan
            continue
        o = CN.ordered_min(V[i])
        if o >= 0:
            out["min"][i] = V[i, o]
            out["witness"][i] = _name(names, o, vox[i] if grid is not None else None)
        if world.any():
            out["min_world"][i] = V[i, world].min()
        if (~world).any():
            out["min_self"][i] = V[i, ~world].min()
    return out


def advance(model, qa, dv, links, spheres, wspheres=(), wboxes=(), grid=None, pairs=(), margin=0.0, tol=1e-3, max_evals=256):
    """motion_numpy.advance with the grid pairs in the table: the same loop, decision for decision.  Returns dict(status [n], evals [n],
    s_free [n], min_sampled [n], s_at_min [n], witness [n][3], near [n] (motion_numpy.advance's, or near_face at some sample), samples)"""
    qa, dv = np.atleast_2d(np.asarray(qa, dtype=float)), np.atleast_2d(np.asarray(dv, dtype=float))
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    ws, wb = np.asarray(wspheres, dtype=float).reshape(-1, 4), np.asarray(wboxes, dtype=float).reshape(-1, 15)
    pairs = list(pairs)
    n, ns = qa.shape[0], spheres.shape[0]
    names = pair_names(ns, ws.shape[0], wb.shape[0], grid, pairs)
    world = names[:, 0] != CN.SELF
    out = dict(status=np.full(n, MN.UNDECIDED, dtype=np.int32), evals=np.zeros(n, dtype=np.int32), s_free=np.zeros(n), min_sampled=np.full(n, np.inf),
               s_at_min=np.zeros(n), witness=np.tile(np.array([CN.NONE, -1, -1], dtype=np.int32), (n, 1)), near=np.zeros(n, dtype=bool),
               samples=[[] for _ in range(n)])
    for i in range(n):
        if not (np.isfinite(qa[i]).all() and np.isfinite(dv[i]).all()):
            out["status"][i] = MN.INVALID
            out["s_free"][i] = out["min_sampled"][i] = out["s_at_min"][i] = np.nan
            continue
        L = MN.motion_bound(model, qa[i], dv[i], links, spheres)
        lam = np.where(world, L[names[:, 1]], L[names[:, 1]] + L[np.maximum(names[:, 2], 0)])
        s = 0.0
        for k in range(max_evals):
            q = MN.interpolate(model, qa[i], dv[i], s)[None]
            cen = MN.centres(model, q, links, spheres)
            V, vox = pair_values(cen, spheres[:, 3], ws, wb, grid, pairs)
            if grid is not None:
                out["near"][i] |= bool(near_face(cen[0], grid))
            v = V[0]
            o = int(np.argmin(v)) if v.size else -1
            m = float(v[o]) if o >= 0 else np.inf
            out["evals"][i] = k + 1
            out["samples"][i].append((s, m))
            out["s_free"][i] = s
            if k == 0 or m < out["min_sampled"][i]:
                out["min_sampled"][i], out["s_at_min"][i] = m, s
                out["witness"][i] = _name(names, o, vox[0] if grid is not None else None)
            out["near"][i] |= abs(m - margin - tol) <= MN.NEAR
            if m < margin + tol:
                out["status"][i] = MN.BLOCKED
                break
            if s == 1.0:
                out["status"][i] = MN.FREE
                break
            if k + 1 == max_evals:
                break
            pos = lam > 0
            delta = float(np.min((v[pos] - margin) / lam[pos])) if pos.any() else np.inf
            out["near"][i] |= abs(s + delta - 1.0) <= MN.NEAR
            s = min(s + delta, 1.0)
    return out


def exact_clearance(model, q, links, spheres, grid, boxes=None):
    """[n]: the least exact clearance of the spheres of configurations q against the union of the occupied cubes"""
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    cen = MN.centres(model, np.atleast_2d(q), links, spheres)
    return (exact_distance(cen, grid, boxes) - spheres[None, :, 3]).min(axis=1)


def random_occupancy(dims, frac, seed):
    """[nz][ny][nx] uint8 with about frac of the voxels occupied"""
    nx, ny, nz = dims
    return (np.random.default_rng(seed).uniform(size=(nz, ny, nx)) < frac).astype(np.uint8)
