"""The numpy reference of include/loik_amd_gridnear.h: the nearest-voxel transform of an occupancy grid (by brute force over the occupied
voxels and by the three passes over 64-bit keys), the eight candidates, the chosen cube and its normal, the query, and collision avoidance
with the grid as one more world object of every sphere: nearest / constraints / avoidance_box / clearance_gradient and the hook of the
lock-step pose loops.

The field, the pair's lower bound and the exact distance are grid_numpy's; the normals of the other pairs, m, the box rule and the centre
Jacobians are avoid_numpy's; both modules are imported unchanged.  test_gridnear_numpy.py proves the claims of the header without a GPU."""
import numpy as np

import avoid_numpy as AN
import clearance_numpy as CN
import grid_numpy as GN

NO_VOXEL = 0xFFFFFFFF
FACE = GN.FACE
NEAR = AN.NEAR


# ---- the transform ----------------------------------------------------------------------------------------------------------------
def feature_brute(occ):
    """F [nz][ny][nx] uint32: the occupied voxel that attains grid_numpy.field_brute, one by one in ascending linear index; a later voxel
    replaces an earlier one only when it is strictly nearer, so ties go to the lowest index"""
    occ = np.asarray(occ) != 0
    nz, ny, nx = occ.shape
    best = np.full(occ.shape, np.int64(1) << 40, dtype=np.int64)
    F = np.full(occ.shape, NO_VOXEL, dtype=np.int64)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    for uz, uy, ux in np.argwhere(occ):   # (argwhere: row-major, the ascending linear index)
        d = GN.g(z - uz) + GN.g(y - uy) + GN.g(x - ux)
        take = d < best
        best[take] = d[take]
        F[take] = (uz * ny + uy) * nx + ux
    return F.astype(np.uint32)


def feature_passes(occ):
    """(G, F): the same by three min-plus passes over the keys (G << 32) | F, along x, then y, then z: the device's build"""
    occ = np.asarray(occ) != 0
    far = (np.int64(1) << 62) | np.int64(NO_VOXEL)   # (above every sum, and three more costs cannot wrap it)
    lin = np.arange(occ.size, dtype=np.int64).reshape(occ.shape)
    K = np.where(occ, lin, far)
    for axis in (2, 1, 0):
        n = K.shape[axis]
        k = np.arange(n)
        cost = GN.g(k[:, None] - k[None, :]).astype(np.int64) << 32              # [out][in]
        Km = np.moveaxis(K, axis, -1)
        K = np.moveaxis((Km[..., None, :] + cost).min(axis=-1), -1, axis)
    empty = K >= (np.int64(1) << 62)
    return np.where(empty, GN.EMPTY, K >> 32).astype(np.uint32), np.where(empty, NO_VOXEL, K & 0xFFFFFFFF).astype(np.uint32)


class Grid(GN.Grid):
    """grid_numpy.Grid with the transform F (brute force unless given)"""

    def __init__(self, occ, origin, h, G=None, F=None):
        super().__init__(occ, origin, h, G)
        self.F = feature_brute(self.occ) if F is None else np.asarray(F, dtype=np.uint32)


def of(grid):
    """a grid_numpy.Grid with the transform beside it"""
    return Grid(grid.occ, grid.origin, grid.h, grid.G)


# ---- the pair with a direction ------------------------------------------------------------------------------------------------------
def _index(c, grid):
    """(p, i, x) of loik_amd_grid.h for centres c [..., 3]"""
    p = np.minimum(np.maximum(c, grid.origin), grid.hi)
    i = np.minimum(np.maximum(np.floor((p - grid.origin) * grid.inv_h), 0.0), (grid.n - 1).astype(float)).astype(np.int64)
    return p, i, grid.origin + (i + 0.5) * grid.h


def candidates(c, grid):
    """[..., 8] the features of the up to eight voxels whose centres surround the clamped centre (NO_VOXEL in an empty grid)"""
    c = np.asarray(c, dtype=float)
    p, i, x = _index(c, grid)
    j = i - (p < x)
    lo, hi = np.maximum(j, 0), np.minimum(j + 1, grid.n - 1)
    out = []
    for s in range(8):
        w = [np.where((s >> k) & 1, hi[..., k], lo[..., k]) for k in range(3)]
        out.append(grid.F[w[2], w[1], w[0]].astype(np.int64))
    return np.stack(out, axis=-1)


def cube_centre(u, grid):
    u = np.asarray(u, dtype=np.int64)
    idx = np.stack([u % grid.n[0], (u // grid.n[0]) % grid.n[1], u // (grid.n[0] * grid.n[1])], axis=-1)
    return grid.origin + (idx + 0.5) * grid.h


def cube_distance(c, u, grid):
    """| max(|c - t_u| - h / 2, 0) | of centres c [..., 3] to the cubes u [...]"""
    e = np.asarray(c, dtype=float) - cube_centre(u, grid)
    o = np.maximum(np.abs(e) - 0.5 * grid.h, 0.0)
    return np.sqrt((o * o).sum(axis=-1))


def cube_normal(c, u, grid):
    """(n [..., 3], gap [...]): avoid_numpy.normal_box with R = I, t = t_u, half extents h / 2, vectorised; gap as there"""
    e = np.asarray(c, dtype=float) - cube_centre(u, grid)
    d = np.abs(e) - 0.5 * grid.h
    sgn = np.where(e >= 0.0, 1.0, -1.0)
    o = np.maximum(d, 0.0)
    ln = np.sqrt((o * o).sum(axis=-1))
    outside = np.any(d > 0.0, axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        n_out = sgn * o / ln[..., None]
    k = np.argmax(d, axis=-1)   # (the lowest index that attains the maximum)
    n_in = np.zeros_like(e)
    np.put_along_axis(n_in, k[..., None], np.take_along_axis(sgn, k[..., None], axis=-1), axis=-1)
    s = np.sort(d, axis=-1)
    return np.where(outside[..., None], n_out, n_in), np.where(outside, np.inf, s[..., 2] - s[..., 1])


def pair(c, r, grid):
    """the pair of the header for centres c [..., 3] (finite) and radii r (broadcast): dict(v, upper = d_u - r, vox, u (-1: an empty grid),
    normal, du, near): near = the choice among the candidates, or the face inside a cube, is decided by less than NEAR"""
    c = np.asarray(c, dtype=float)
    v, vox = GN.sphere_grid(c, r, grid)
    cand = candidates(c, grid)
    none = cand == NO_VOXEL
    d = np.where(none, np.inf, cube_distance(c[..., None, :], np.where(none, 0, cand), grid))
    dmin = d.min(axis=-1)
    u = np.where(d == dmin[..., None], cand, np.int64(1) << 40).min(axis=-1)     # the lowest index among the least d
    empty = none.all(axis=-1)
    us = np.where(empty, 0, u)
    n, gap = cube_normal(c, us, grid)
    with np.errstate(invalid="ignore"):
        other = (cand != u[..., None]) & ~none & (d - dmin[..., None] < NEAR)
    return dict(v=v, upper=np.where(empty, np.inf, dmin) - r, vox=vox, u=np.where(empty, -1, u), normal=np.where(empty[..., None], 0.0, n),
                du=np.where(empty, np.inf, dmin), near=~empty & (other.any(axis=-1) | (gap < NEAR)))


def query(spheres, grid):
    """BatchedLoik.grid_nearest: dict(val [n][2], vox [n][2], normal [n][3]); a row that is not finite: NaN, (-1, -1), NaN"""
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    bad = ~np.isfinite(spheres).all(axis=1)
    sp = np.where(bad[:, None], 0.0, spheres)
    pr = pair(sp[:, :3], sp[:, 3], grid)
    val = np.stack([pr["v"], pr["upper"]], axis=1)
    vox = np.stack([pr["vox"], pr["u"]], axis=1).astype(np.int32)
    normal = np.array(pr["normal"])
    val[bad], vox[bad], normal[bad] = np.nan, -1, np.nan
    return dict(val=val, vox=vox, normal=normal, near=pr["near"] & ~bad)


def near_plane(c, grid):
    """[...]: some component of the clamped centre, in voxels from the origin, lies within FACE of a voxel face inside the grid (where the
    voxel read changes) or of a mid-plane through voxel centres (where the candidates change)"""
    c = np.asarray(c, dtype=float)
    t = (np.minimum(np.maximum(c, grid.origin), grid.hi) - grid.origin) * grid.inv_h
    k = np.rint(t)
    face = (np.abs(t - k) <= FACE) & (k > 0) & (k < grid.n)
    mid = np.abs(t - 0.5 - np.rint(t - 0.5)) <= FACE
    return (face | mid).any(axis=-1)


# ---- avoidance with the grid as one more world object --------------------------------------------------------------------------------
def nearest(model, q, links, spheres, ws=(), wb=(), pairs=(), grid=None):
    """avoid_numpy.nearest with the grid pair of every sphere at ordinal nws + nwb among its world objects, at the lower bound v; also
    gridpair: pair() of every centre, and near_grid [n]: some centre is near_plane"""
    t = AN.nearest(model, q, links, spheres, ws, wb, pairs)
    if grid is None:
        return t
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    nwo = np.asarray(ws, dtype=float).reshape(-1, 4).shape[0] + np.asarray(wb, dtype=float).reshape(-1, 15).shape[0]
    pr = pair(t["centres"], spheres[None, :, 3], grid)
    old, v = t["pairs"][:, :, 0], pr["v"]
    with np.errstate(invalid="ignore"):
        take = (t["partner"][:, :, 0] < 0) | (v < old)   # (the last ordinal: an equal value stays with the object before it)
        three = np.sort(np.stack([np.where(np.isnan(old), np.inf, old), t["second"][:, :, 0], v], axis=-1), axis=-1)
    t["second"][:, :, 0] = three[..., 1]
    t["pairs"][:, :, 0] = np.where(take, v, old)
    t["partner"][:, :, 0] = np.where(take, nwo, t["partner"][:, :, 0])
    t["pairs"][t["bad"]] = np.nan
    t["partner"][t["bad"]] = -1
    t.update(gridpair=pr, nwo=nwo, near_grid=near_plane(t["centres"], grid).any(axis=-1))
    return t


def constraints(model, q, links, spheres, ws, wb, pairs, d_influence, grid=None, d_safe=None, clamped=False):
    """avoid_numpy.constraints with the grid: the active constraints of every row as dict(a, kind, partner, d, n, g, m), near [n], the
    table.  A grid constraint has d = v, n = the normal of the chosen cube and g = n^T Jc.  The table gains tiny [n][nv]: DoF j of row i
    has a grid constraint with 0 < |g_j| < NEAR.  The normal of a cube's face is a world axis, so a joint about that axis (the first of
    panda7 under a z face) has a derivative that is 0 by structure, which the reference's Jacobian returns as rounding noise of either
    sign and the device may return as 0: neither answer is wrong, so it does not make the row near; the caller leaves those entries of
    an unbounded box out.  clamped = True is for a caller that clamps into a finite base box (the pose loops): there both answers give the
    same bound and nothing is left out -- except at or below d_safe, where r = 0 and the sign of g alone decides between a bound of 0 and
    none: such an entry then does make the row near"""
    q = np.atleast_2d(np.asarray(q, dtype=float))
    t = nearest(model, q, links, spheres, ws, wb, pairs, grid)
    if grid is None:
        return AN.constraints(model, q, links, spheres, ws, wb, pairs, d_influence, table=t, d_safe=d_safe)
    out, near = [], np.array(t["near_grid"])
    t["tiny"] = np.zeros((q.shape[0], model.nv), dtype=bool)
    for i in range(q.shape[0]):
        row = []
        if not t["bad"][i]:
            v, s = t["pairs"][i], t["second"][i]
            with np.errstate(invalid="ignore"):
                near[i] |= bool(np.any(np.abs(v - d_influence) < NEAR)) or bool(np.any((v < d_influence) & (s < d_influence) & (s - v < NEAR)))
            act = [(a, kind) for a in range(v.shape[0]) for kind in (0, 1) if v[a, kind] < d_influence]
            jc = AN.centre_jacobians(model, q[i], links, spheres, [a for a, _ in act] + [int(t["partner"][i, a, 1]) for a, kind in act if kind == 1])
            for a, kind in act:
                partner = int(t["partner"][i, a, kind])
                if kind == 0 and partner == t["nwo"]:
                    nrm = t["gridpair"]["normal"][i, a]
                    g = nrm @ jc[a]
                    m, nr = int(AN.pair_dofs(model, links[a]).sum()), bool(t["gridpair"]["near"][i, a])
                else:
                    nrm, g, m, nr = AN.pair_gradient(model, q[i], links, spheres, ws, wb, jc, a, kind, partner, t["centres"][i])
                small = (g != 0.0) & (np.abs(g) < NEAR)
                if kind == 0 and partner == t["nwo"] and not (clamped and d_safe is not None and v[a, kind] <= d_safe):
                    t["tiny"][i] |= small
                    small = np.zeros_like(small)
                near[i] |= nr or bool(np.any(small)) or (d_safe is not None and abs(v[a, kind] - d_safe) < NEAR)
                row.append(dict(a=a, kind=kind, partner=partner, d=float(v[a, kind]), n=nrm, g=g, m=m))
        out.append(row)
    return out, near, t


def avoidance_box(model, q, links, spheres, ws, wb, pairs, dt, lb, ub, d_safe, d_influence, kappa, grid=None):
    """BatchedLoik.avoidance_box with a grid set and the transform latched: avoid_numpy.avoidance_box's dict"""
    q = np.atleast_2d(np.asarray(q, dtype=float))
    lb, ub = np.broadcast_to(np.asarray(lb, dtype=float), (model.nv,)), np.broadcast_to(np.asarray(ub, dtype=float), (model.nv,))
    cons, near, t = constraints(model, q, links, spheres, ws, wb, pairs, d_influence, grid, d_safe=d_safe)
    lo, hi = np.empty((q.shape[0], model.nv)), np.empty((q.shape[0], model.nv))
    for i in range(q.shape[0]):
        lo[i], hi[i] = AN.narrow(cons[i], lb, ub, d_safe, kappa, dt)[:2]
    return dict(lo=lo, hi=hi, pairs=t["pairs"], partner=t["partner"], near=near, cons=cons, centres=t["centres"],
                tiny=t.get("tiny", np.zeros(lo.shape, dtype=bool)))


def clearance_gradient(model, q, links, spheres, ws=(), wb=(), pairs=(), grid=None):
    """BatchedLoik.clearance_gradient with a grid: grid_numpy.clearance plus grad [n][nv] of the witness pair, near [n], and for a grid
    witness cube [n] (the chosen cube, -1 otherwise)"""
    q = np.atleast_2d(np.asarray(q, dtype=float))
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    out = GN.clearance(model, q, links, spheres, ws, wb, grid, pairs)
    nws = np.asarray(ws, dtype=float).reshape(-1, 4).shape[0]
    grad, near, cube = np.zeros((q.shape[0], model.nv)), np.zeros(q.shape[0], dtype=bool), -np.ones(q.shape[0], dtype=np.int64)
    for i in range(q.shape[0]):
        kind, a, b = (int(x) for x in out["witness"][i])
        if not np.isfinite(q[i]).all():
            grad[i] = np.nan
            continue
        if kind == CN.NONE:
            continue
        if kind == GN.WORLD_GRID:
            pr = pair(out["centres"][i, a], spheres[a, 3], grid)
            grad[i] = pr["normal"] @ AN.centre_jacobians(model, q[i], links, spheres, [a])[a]
            nr, cube[i] = bool(pr["near"]) or bool(near_plane(out["centres"][i, a], grid)), int(pr["u"])
        else:
            partner = b if kind != CN.WORLD_BOX else nws + b
            _, grad[i], _, nr = AN.pair_gradient(model, q[i], links, spheres, ws, wb, None, a, 1 if kind == CN.SELF else 0, partner, out["centres"][i])
        s = np.sort(out["values"][i])
        near[i] = nr or (s.size > 1 and s[1] - s[0] < NEAR)
    out.update(grad=grad, near=near, cube=cube)
    return out


def narrower(model, col, avoid, dt, B):
    """avoid_numpy.narrower with col["grid"]: the `narrow` hook of the lock-step loops (pose_step_numpy.lockstep_pose_loop_step with
    max_backtracks = 0 and patience = 0 is SolvePose; pose_path_numpy, pose_track_numpy), with the same `results`"""
    res = dict(avoid_min_seen=np.full(B, np.inf), avoid_active_steps=np.zeros(B, dtype=np.int32),
               avoid_flags=np.zeros((B, model.nv), dtype=np.int32), near=np.zeros(B, dtype=bool))

    def narrow_step(b, q_b, lo, hi):
        cons, nr, t = constraints(model, q_b[None], col["links"], col["spheres"], col["ws"], col["wb"], col["pairs"], avoid["d_influence"],
                                  col.get("grid"), d_safe=avoid["d_safe"], clamped=True)
        res["near"][b] |= bool(nr[0])
        res["avoid_min_seen"][b] = min(res["avoid_min_seen"][b], float(np.min(t["pairs"][0])))
        nlo, nhi = AN.narrow(cons[0], lo, hi, avoid["d_safe"], avoid["kappa"], dt)[:2]
        res["avoid_flags"][b] = (nlo > lo).astype(np.int32) | ((nhi < hi).astype(np.int32) << 1)
        res["avoid_active_steps"][b] += int(np.any(res["avoid_flags"][b] != 0))
        return nlo, nhi

    narrow_step.results = res
    return narrow_step


def voxelise_box(box15, origin, h, dims):
    """occ [nz][ny][nx]: the voxels whose centre lies in the oriented box [15] of clearance_numpy"""
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ctr = np.asarray(origin, dtype=float) + (np.stack([x, y, z], axis=-1) + 0.5) * h
    return (CN.sphere_box(ctr, 0.0, np.asarray(box15, dtype=float)) <= 0.0).astype(np.uint8)
