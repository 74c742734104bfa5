"""Measurements for profiles/depth_measured.md: a 640 x 480 float image into grids of 256 x 256 x 64 and 512 x 512 x 256 voxels.

`python scripts/measure_depth.py` times whole calls with hipEvent pairs on the handle's stream (a non-blocking stream of the caller's,
set_stream): integrate_depth in its modes from a host and from a device image, and for comparison the only route there was before,
set_collision_grid from a host occupancy (upload included) and from a device occupancy (the field build alone).  Every call is complete
on return, so a pair brackets the upload, the kernels and the drain.  One line of JSON per grid.

`python scripts/measure_depth.py kernels` makes the same calls a few times and nothing else: run it under
`rocprofv3 --kernel-trace --stats` for the time of each kernel."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GRIDS = (((256, 256, 64), 0.02), ((512, 512, 256), 0.01))   # dims, voxel: 5.12 x 5.12 x 1.28 m and 5.12 x 5.12 x 2.56 m
REPEAT = 12


def scene(dims, h):
    import depth_cases as DC
    import depth_numpy as DN
    cam = DN.Camera(640, 480, 525.0, 525.0, 319.5, 239.5, DC.LOOK_X, [-2.4, 0.0, 0.6], 0.3, 6.0)
    origin = np.array([-2.56, -2.56, -0.2])
    boxes = [np.concatenate([np.eye(3).reshape(9), c, e]) for c, e in (([0.6, 0.4, 0.5], [0.2, 0.3, 0.5]), ([0.2, -0.7, 0.3], [0.3, 0.2, 0.3]), ([1.4, 0.0, 0.9], [0.1, 0.8, 0.1]))]
    img = DN.render(cam, boxes=boxes, planes=[[1.0, 0.0, 0.0, 2.2], [0.0, 0.0, 1.0, 0.0]], spheres=[[0.0, 0.0, 0.5, 0.25]])
    return cam, img, origin


def main(kernels_only):
    import depth_cases as DC
    from loik_amd import capi
    from stream_harness import DevBuf, Lane, hip
    from test_clearance import _open
    h = hip()
    h.hipEventSynchronize.argtypes = [C.c_void_p]
    h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    r = DC.robot()
    lane = Lane()
    s = _open(r["model"], r["q"])
    s.set_collision_spheres(r["links"], r["spheres"])
    s.set_stream(lane.ptr)
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert h.hipEventCreate(C.byref(e)) == 0

    def timed(fn):
        """milliseconds between two events on the handle's stream around fn()"""
        assert h.hipEventRecord(ev[0], lane.stream) == 0
        out = fn()
        assert h.hipEventRecord(ev[1], lane.stream) == 0 and h.hipEventSynchronize(ev[1]) == 0
        ms = C.c_float()
        assert h.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        return ms.value, out

    for dims, voxel in GRIDS:
        cam, img, origin = scene(dims, voxel)
        cd = cam.as_dict()
        dimg = DevBuf(img)
        kw = dict(dims=dims, origin=origin, voxel=voxel)
        calls = {
            "replace, host image": lambda: s.integrate_depth(img, cd, **kw),
            "replace, device image": lambda: s.integrate_depth(dimg, cd, **kw),
            "fuse, host image": lambda: s.integrate_depth(img, cd, mode="fuse", **kw),
            "fuse + carve, host image": lambda: s.integrate_depth(img, cd, mode="fuse", carve=True, **kw),
            "fuse + carve + filter (1 q), host image": lambda: s.integrate_depth(img, cd, mode="fuse", carve=True, filter_q=1, **kw),
            "fuse + carve + filter (1 q), device image": lambda: s.integrate_depth(dimg, cd, mode="fuse", carve=True, filter_q=1, **kw),
        }
        st = s.integrate_depth(img, cd, mode="replace", **kw)
        occ = s.collision_occupancy()
        docc = DevBuf(occ)
        calls["set_collision_grid, host occupancy (the route before)"] = lambda: s.set_collision_grid(occ, origin, voxel)
        calls["set_collision_grid, device occupancy (the build alone)"] = lambda: s.set_collision_grid(docc, origin, voxel)
        out = dict(dims=dims, voxel=voxel, stats=st, occupied=int(occ.sum()), ms={})
        for rnd in range(3 if kernels_only else REPEAT):   # (the calls alternate: a drift of the machine lands on all of them)
            for name, fn in calls.items():
                ms, _ = timed(fn)
                out["ms"].setdefault(name, []).append(ms)
        if not kernels_only:
            out["ms"] = {k: dict(median=float(np.median(v[2:])), lo=float(min(v[2:])), hi=float(max(v[2:]))) for k, v in out["ms"].items()}
            print(json.dumps(out))
        dimg.free()
        docc.free()
    s.close()
    lane.close()


if __name__ == "__main__":
    main(len(sys.argv) > 1 and sys.argv[1] == "kernels")
