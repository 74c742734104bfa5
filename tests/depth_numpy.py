"""The numpy reference of include/loik_amd_depth.h: steps 1 to 5 in the header's arithmetic (every operation one rounded fp64 operation, in
the order written there; the field through grid_numpy.field_brute), a tiny renderer that makes depth images of analytic planes, boxes
and spheres, and the decisions of a case that lie so close to their threshold that the device may take them the other way.

test_depth_numpy.py proves the header's claims on this reference alone, without a GPU."""
import numpy as np

import grid_numpy as GN
import motion_numpy as MN

NEAR = MN.NEAR
REPLACE, FUSE = "replace", "fuse"
COVER = 0.5 * np.sqrt(3.0)   # times h: what band and filter_pad must at least cover


class Camera:
    """a pinhole camera: R [3][3] and p [3] place the camera frame (x right, y down, z forward) in the world"""

    def __init__(self, width, height, fx, fy, cx, cy, R, p, z_min, z_max, depth_scale=1.0):
        self.width, self.height = int(width), int(height)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.R, self.p = np.asarray(R, dtype=float).reshape(3, 3), np.asarray(p, dtype=float).reshape(3)
        self.z_min, self.z_max, self.depth_scale = float(z_min), float(z_max), float(depth_scale)

    def as_dict(self):
        return dict(fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy, T_world_cam=np.concatenate([self.R.reshape(9), self.p]), z_min=self.z_min,
                    z_max=self.z_max, depth_scale=self.depth_scale)


def returns(depth, cam):
    """(d [H][W] metric z-depth, ret [H][W]: the pixel is a return)"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.asarray(depth).astype(np.float64) * cam.depth_scale
        ret = np.isfinite(d) & (d >= cam.z_min) & (d <= cam.z_max)
    return d, ret


def back_project(depth, cam):
    """(x_w [H W][3], ret [H W]) of every pixel, in the header's order of operations"""
    d, ret = returns(depth, cam)
    v, u = np.meshgrid(np.arange(cam.height, dtype=float), np.arange(cam.width, dtype=float), indexing="ij")
    d = np.where(ret, d, 1.0)
    xc = np.stack([((u - cam.cx) / cam.fx) * d, ((v - cam.cy) / cam.fy) * d, d], axis=-1).reshape(-1, 3)
    R, p = cam.R, cam.p
    xw = np.stack([((R[k, 0] * xc[:, 0] + R[k, 1] * xc[:, 1]) + R[k, 2] * xc[:, 2]) + p[k] for k in range(3)], axis=-1)
    return xw, ret.reshape(-1)


def voxel_coords(xw, origin, h):
    """t [n][3] = (x_w - origin) inv_h: the voxel is floor(t)"""
    return (np.asarray(xw, dtype=float) - np.asarray(origin, dtype=float)) * (1.0 / float(h))


def centres_of(dims, origin, h):
    """(x [nx], y [ny], z [nz]): the voxel centres along each axis, origin + (i + 0.5) h with the product rounded first"""
    return [float(origin[k]) + (np.arange(dims[k]) + 0.5) * float(h) for k in range(3)]


def _project(cam, dims, origin, h):
    """of every voxel centre: (x_c [nz][ny][nx][3], a_u, a_v: the pixel coordinates before the floor)"""
    X, Y, Z = centres_of(dims, origin, h)
    e2, e1, e0 = np.meshgrid(Z - cam.p[2], Y - cam.p[1], X - cam.p[0], indexing="ij")
    R = cam.R
    xc = np.stack([(R[0, j] * e0 + R[1, j] * e1) + R[2, j] * e2 for j in range(3)], axis=-1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        au = ((cam.fx * xc[..., 0]) / xc[..., 2] + cam.cx) + 0.5
        av = ((cam.fy * xc[..., 1]) / xc[..., 2] + cam.cy) + 0.5
    return xc, au, av


def carve(P, depth, cam, dims, origin, h, band):
    """dict(cleared [nz][ny][nx], and what ambiguous() reads): step 2 of the header for the prior P"""
    d, ret = returns(depth, cam)
    xc, au, av = _project(cam, dims, origin, h)
    front = xc[..., 2] > 0
    with np.errstate(invalid="ignore"):
        u, v = np.floor(au), np.floor(av)
        inimg = front & (u >= 0) & (u < cam.width) & (v >= 0) & (v < cam.height)
    ui, vi = np.where(inimg, u, 0).astype(np.int64), np.where(inimg, v, 0).astype(np.int64)
    dpix = np.where(inimg & ret[vi, ui], d[vi, ui], np.nan)
    with np.errstate(invalid="ignore"):
        seen = (xc[..., 2] + band) < dpix
    P = np.asarray(P) != 0
    return dict(cleared=P & seen, z=xc[..., 2], au=au, av=av, inimg=inimg, dpix=dpix, front=front, band=band)


def filter_mask(cen, rad, dims, origin, h):
    """(mask [nz][ny][nx]: the voxel's centre lies within rad of some centre; dist2 - rad2 margins for ambiguous())"""
    X, Y, Z = centres_of(dims, origin, h)
    mask = np.zeros((dims[2], dims[1], dims[0]), dtype=bool)
    near = np.zeros_like(mask)
    tests = 0
    for c, R in zip(np.asarray(cen, dtype=float).reshape(-1, 3), np.asarray(rad, dtype=float).reshape(-1)):
        if not np.isfinite(c).all():
            continue
        dz, dy, dx = np.meshgrid(Z - c[2], Y - c[1], X - c[0], indexing="ij")
        s = (dx * dx + dy * dy) + dz * dz
        mask |= s <= R * R
        near |= np.abs(np.sqrt(s) - R) <= NEAR * max(1.0, R)
        tests += int((s <= 4.0 * R * R + 3.0 * h * h).sum())
    return mask, near, tests


def integrate(cam=None, depth=None, points=None, dims=None, origin=None, h=None, mode=REPLACE, carve_on=False, band=0.0, prior=None,
              filter_centres=(), filter_radii=(), filter_pad=0.0, field=True):
    """steps 1 to 5.  prior: the occupancy [nz][ny][nx] of the grid that is set (None: none is).  filter_centres [m][3] and filter_radii [m]:
    the world centres and radii of the robot's spheres at every filter configuration.  Returns dict(occ uint8, stats [4], G (field=True),
    ambiguous: dict step -> (count, decisions), touched [nz][ny][nx]: the voxels an ambiguous decision may change)"""
    nx, ny, nz = (int(n) for n in dims)
    origin = np.asarray(origin, dtype=float).reshape(3)
    shape = (nz, ny, nx)
    P = np.zeros(shape, dtype=bool) if (mode == REPLACE or prior is None) else (np.asarray(prior) != 0)
    assert P.shape == shape
    occ = P.copy()
    touched = np.zeros(shape, dtype=bool)
    amb = {}
    if carve_on:
        assert mode == FUSE and cam is not None
        cv = carve(P, depth, cam, dims, origin, h, band)
        occ &= ~cv["cleared"]
        with np.errstate(invalid="ignore"):
            a = P & (np.abs(cv["z"]) <= NEAR)
            for t in (cv["au"], cv["av"]):
                a |= P & cv["front"] & np.isfinite(t) & (np.abs(t - np.rint(t)) <= NEAR * np.maximum(1.0, np.abs(t)))
            b = P & np.isfinite(cv["dpix"]) & (np.abs(cv["z"] + band - cv["dpix"]) <= NEAR * np.maximum(1.0, np.abs(cv["dpix"])))
        touched |= a | b
        amb["carve_pixel"] = (int(a.sum()), int((P & cv["front"]).sum()))
        amb["carve_depth"] = (int(b.sum()), int((P & cv["inimg"]).sum()))
    if cam is not None:
        xw, ret = back_project(depth, cam)
    else:
        xw = np.asarray(points, dtype=float).reshape(-1, 3)
        ret = np.isfinite(xw).all(axis=1)
    xw = xw[ret]
    t = voxel_coords(xw, origin, h)
    i = np.floor(t)
    n = np.array([nx, ny, nz], dtype=float)
    inside = ((i >= 0) & (i < n)).all(axis=1)
    ii = i[inside].astype(np.int64)
    occ[ii[:, 2], ii[:, 1], ii[:, 0]] = True
    # a point near a face between two voxels (or a face of the grid's box) may fall on its other side: every voxel around it is touched
    face = np.abs(t - np.rint(t)) <= NEAR * np.maximum(1.0, np.abs(t))
    reach = ((np.rint(t) >= -1) & (np.rint(t) <= n + 1)).all(axis=1)
    amb_pts = face.any(axis=1) & reach
    for k in np.flatnonzero(amb_pts):
        lo = np.clip(np.rint(t[k]).astype(np.int64) - 1, 0, None)
        hi = np.minimum(np.rint(t[k]).astype(np.int64) + 1, np.array([nx, ny, nz]) - 1)
        touched[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    amb["points"] = (int(amb_pts.sum()), int(ret.sum()))
    cen = np.asarray(filter_centres, dtype=float).reshape(-1, 3)
    if cen.shape[0]:
        rad = np.asarray(filter_radii, dtype=float).reshape(-1) + filter_pad
        mask, near, tests = filter_mask(cen, rad, dims, origin, h)
        occ &= ~mask
        touched |= near
        amb["filter"] = (int(near.sum()), tests)
    out = dict(occ=occ.astype(np.uint8), stats=np.array([int(ret.sum()), int(inside.sum()), int(P.sum()), int(occ.sum())], dtype=np.int64),
               ambiguous=amb, touched=touched, points=xw, inside=inside)
    if field:
        out["G"] = GN.field_brute(occ)
    return out


def ambiguous_share(res):
    """the largest share of ambiguous decisions among the steps of an integrate() result"""
    return max((a / max(n, 1) for a, n in res["ambiguous"].values()), default=0.0)


# ---- the renderer ------------------------------------------------------------------------------------------------------------------------
def render(cam, planes=(), boxes=(), spheres=(), dtype=np.float32, miss=0.0):
    """a depth image [height][width] of the nearest hit along every pixel's ray: planes [k][4] = (n, d) with n . x = d, boxes [k][15] =
    (R row-major, centre, half extents), spheres [k][4] = (centre, radius), all in the world.  The z-depth of a hit is the ray parameter,
    since the ray's direction has z = 1 in the camera frame.  A miss is `miss`; dtype uint16 stores depth / depth_scale, rounded"""
    v, u = np.meshgrid(np.arange(cam.height, dtype=float), np.arange(cam.width, dtype=float), indexing="ij")
    dc = np.stack([(u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy, np.ones_like(u)], axis=-1)
    dw = dc @ cam.R.T
    o = cam.p
    best = np.full(u.shape, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for pl in np.asarray(planes, dtype=float).reshape(-1, 4):
            t = (pl[3] - pl[:3] @ o) / (dw @ pl[:3])
            best = np.where((t > 0) & (t < best), t, best)
        for s in np.asarray(spheres, dtype=float).reshape(-1, 4):
            oc = o - s[:3]
            a, b, c = (dw * dw).sum(axis=-1), 2.0 * (dw @ oc), oc @ oc - s[3] * s[3]
            disc = b * b - 4.0 * a * c
            t = (-b - np.sqrt(np.where(disc >= 0, disc, np.nan))) / (2.0 * a)
            best = np.where((t > 0) & (t < best), t, best)
        for bx in np.asarray(boxes, dtype=float).reshape(-1, 15):
            Rb = bx[:9].reshape(3, 3)
            ol, dl = (o - bx[9:12]) @ Rb, dw @ Rb
            t1, t2 = (-bx[12:15] - ol) / dl, (bx[12:15] - ol) / dl
            tn, tf = np.minimum(t1, t2).max(axis=-1), np.maximum(t1, t2).min(axis=-1)
            best = np.where((tn <= tf) & (tn > 0) & (tn < best), tn, best)
    if dtype == np.uint16:
        units = np.where(np.isfinite(best), np.rint(best / cam.depth_scale), miss)
        return np.clip(units, 0, 65535).astype(np.uint16)
    return np.where(np.isfinite(best), best, miss).astype(dtype)
