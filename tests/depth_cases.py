"""The inputs of tests/test_depth_integrate.py and tests/test_depth_routes.py (GPU), and of the CPU test that checks every one of them
against the cap on ambiguous decisions (test_depth_numpy.py): cameras, images, grids and a robot to filter, each with the numpy answer
of tests/depth_numpy.py, computed once.

Exact cases: fx = fy = 64, cx and cy half-integers, depths multiples of 1 / 32 (uint16: units of 1 / 1024 m), h = 1 / 16, a dyadic camera
position, R a signed permutation -- every product and sum of steps 2 and 3 is exact in fp64, so the device's occupancy, stats and field
equal the reference's bit for bit.  The grid's origin is off the voxel lattice of the points by 1 / 8192, so that no point lies on a face.
General cases: a 3-4-5 rotation about z composed with a rotation about x, fx = fy = 525, random depths."""
import numpy as np

import clearance_numpy as CN
import depth_numpy as DN
import motion_numpy as MN
import qp_cases as QC

H_EXACT = 1.0 / 16.0
CAP = 0.005   # ambiguous decisions per step, at most (the issue's cap)
# the camera looks along world +x: its x axis is world -y, its y axis world -z (the columns of R are the camera's axes in the world)
LOOK_X = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
# grids (nx, ny, nz): one voxel; two line lengths that are no multiple of the four voxels of a thread; one large
GRIDS = {"one": (1, 1, 1), "thin": (65, 3, 9), "odd": (130, 67, 5), "large": (256, 256, 64)}
IMAGES = {"1x1": (1, 1), "65x3": (65, 3), "vga": (640, 480)}

_MEMO = {}


def _memo(fn):
    def wrapped(*key):
        k = (fn.__name__,) + key
        if k not in _MEMO:
            _MEMO[k] = fn(*key)
        return _MEMO[k]
    wrapped.__doc__ = fn.__doc__
    return wrapped


def rot(axis, c, s):
    R = np.eye(3)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def general_R():
    """a 3-4-5 rotation about z, then one about the camera's x, of the camera that looks along +x"""
    return rot(2, 0.8, 0.6) @ LOOK_X @ rot(0, np.cos(0.2), np.sin(0.2))


def camera(kind, size, p=(-0.5, 0.25, 0.5), scale=1.0):
    W, H = IMAGES[size] if isinstance(size, str) else size
    if kind == "exact":
        return DN.Camera(W, H, 64.0, 64.0, 0.5 * (W - 1) + (0.5 if W % 2 else 0.0), 0.5 * (H - 1) + (0.5 if H % 2 else 0.0), LOOK_X, p, 0.25, 8.0, scale)
    return DN.Camera(W, H, 525.0, 525.0, 0.5 * W - 0.37, 0.5 * H + 0.21, general_R(), np.asarray(p) + np.array([0.013, -0.007, 0.004]), 0.3, 6.0, scale)


def image(kind, cam, seed, dtype=np.float32, holes=True):
    """random depths (exact: multiples of 1 / 32 m); with holes, every kind of pixel that is no return"""
    rng = np.random.default_rng(seed)
    shape = (cam.height, cam.width)
    d = rng.integers(16, 96, size=shape) / 32.0 if kind == "exact" else rng.uniform(0.4, 2.8, size=shape)
    if dtype == np.uint16:
        img = np.rint(d / cam.depth_scale).astype(np.uint16)
        if holes and img.size >= 8:
            flat = img.reshape(-1)
            flat[rng.choice(img.size, size=4, replace=False)] = [0, 1, 65535, int(0.2 / cam.depth_scale)]   # none, below z_min twice, above z_max
        return img
    img = d.astype(np.float32)
    if holes and img.size >= 8:
        flat = img.reshape(-1)
        flat[rng.choice(img.size, size=6, replace=False)] = [0.0, np.nan, np.inf, -np.inf, 0.5 * cam.z_min, 2.0 * cam.z_max]
    return img


def grid_for(cam, dims, h, ahead=0.5):
    """the origin of a grid of `dims` that starts `ahead` in front of the camera and is centred on its axis, off the lattice by 1 / 8192"""
    n = np.array(dims, dtype=float)
    axis = cam.R[:, 2]
    lo = cam.p + axis * (ahead + 0.5 * n[0] * h) - 0.5 * n * h
    return np.round(lo * 16.0) / 16.0 + 1.0 / 8192.0


@_memo
def robot():
    """panda7 with two spheres a link, three configurations"""
    model = QC.model_of("panda7")
    links, spheres = CN.make_spheres(model, 2, 2210)
    q = model.random_configurations(np.random.default_rng(2211), 3)
    return dict(model=model, links=links, spheres=spheres, q=q, centres=MN.centres(model, q, links, spheres))


# name -> (kind, image, grid, dtype, depth_scale, filter configurations).  The GPU tests integrate every one of them in REPLACE mode and
# once more in FUSE onto the result of another seed, with the carve
CASES = {
    "exact-65x3-thin": ("exact", "65x3", "thin", np.float32, 1.0, 0),
    "exact-1x1-one": ("exact", "1x1", "one", np.float32, 1.0, 0),
    "exact-65x3-odd-u16": ("exact", "65x3", "odd", np.uint16, 1.0 / 1024.0, 1),
    "exact-vga-odd": ("exact", "vga", "odd", np.float32, 1.0, 3),
    "general-vga-odd": ("general", "vga", "odd", np.float32, 1.0, 3, dict(p=(-1.1, -0.85, 0.25), ahead=-1.5)),   # (the robot stands in this grid)
    "general-65x3-thin-u16": ("general", "65x3", "thin", np.uint16, 0.001, 1),
    "general-65x3-large": ("general", "65x3", "large", np.float32, 1.0, 1),
    "general-1x1-one": ("general", "1x1", "one", np.float32, 1.0, 0),
}


@_memo
def case(name):
    """dict(cam, img, prev (the image of the frame before, for FUSE), dims, origin, h, nf, centres, radii, pad, band, replace, fuse): the two
    numpy answers; fuse is the frame onto the occupancy of `prev` alone, carved with the recommended band"""
    kind, size, grid, dtype, scale, nf = CASES[name][:6]
    over = CASES[name][6] if len(CASES[name]) > 6 else {}
    seed = 2300 + 10 * list(CASES).index(name)
    h = H_EXACT if kind == "exact" else 0.05
    cam = camera(kind, size, scale=scale, **({"p": over["p"]} if "p" in over else {}))
    dims = GRIDS[grid]
    origin = grid_for(cam, dims, h, ahead=over.get("ahead", 0.6))
    if grid == "one":   # the one voxel sits where the central pixel's point falls
        cam_d = 1.03125
        origin = DN.back_project(np.full((cam.height, cam.width), cam_d, dtype=np.float32), cam)[0][0] - 0.5 * h + 1.0 / 8192.0
        img = prev = np.full((cam.height, cam.width), cam_d, dtype=np.float32)
    else:
        img, prev = image(kind, cam, seed, dtype), image(kind, cam, seed + 1, dtype)
        if grid == "large":   # (few returns, so that the brute-force field of the reference stays cheap)
            keep = np.zeros(img.size, dtype=bool)
            keep[np.random.default_rng(seed + 2).choice(img.size, size=9, replace=False)] = True
            img, prev = np.where(keep.reshape(img.shape), img, 0).astype(dtype), np.where(keep.reshape(img.shape)[::-1], prev, 0).astype(dtype)
    r = robot()
    c = dict(name=name, kind=kind, cam=cam, img=img, prev=prev, dims=dims, origin=origin, h=h, nf=nf, pad=DN.COVER * h + 0.01, band=DN.COVER * h)
    c["centres"], c["radii"] = r["centres"][:nf].reshape(-1, 3), np.tile(r["spheres"][:, 3], nf)
    kw = dict(dims=dims, origin=origin, h=h, filter_centres=c["centres"], filter_radii=c["radii"], filter_pad=c["pad"])
    c["replace"] = DN.integrate(cam=cam, depth=img, **kw)
    before = DN.integrate(cam=cam, depth=prev, dims=dims, origin=origin, h=h, field=False)
    c["prior"] = before["occ"]
    c["fuse"] = DN.integrate(cam=cam, depth=img, mode=DN.FUSE, carve_on=True, band=c["band"], prior=before["occ"], **kw)
    return c
