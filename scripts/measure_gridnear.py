"""Measurements for profiles/gridnear_measured.md: the time of set_collision_grid with and without the nearest-voxel transform latched, and
the time of a SolvePose step with collision avoidance at B = 4096 on panda7 -- without a grid, with a grid read through the transform, and
with the grid's cubes given as world boxes.  `python scripts/measure_gridnear.py` runs the set-time part in this process and the step part
in child processes, three rounds; with LOIKB_PARENT_LIB=<a libloik_amd.so built from the parent commit> the rounds alternate between that
library and this tree's for the step without a grid.  Everything timed ends in a synchronous call."""
import ctypes as C
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PARENT = os.environ.get("LOIKB_PARENT_LIB")


def _load(lib):
    from loik_amd import capi
    if lib:
        class Lenient(C.CDLL):
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if name.startswith("loikb_"):
                        return types.SimpleNamespace()
                    raise
        capi._LIB_PATH = lib
        capi.C.CDLL = Lenient
    return capi


def step(lib, mode):
    """one line of JSON: seconds per SolvePose step at B = 4096 on panda7; mode: nogrid / grid / boxes"""
    import numpy as np
    capi = _load(lib)
    import gridnear_cases as GC
    import grid_numpy as GN
    from test_avoid_pose import AVOID, TOL, _latched
    w = dict(GC.pose_workload("panda7"))
    rep = 4096 // w["B"]
    for k in ("q0", "tg"):
        w[k] = np.ascontiguousarray(np.tile(w[k], (rep,) + (1,) * (w[k].ndim - 1)))
    w["B"] = w["q0"].shape[0]
    col = dict(w["col"])
    g = col["grid"]
    if mode == "boxes":
        col["wb"] = np.concatenate([col["wb"], GN.cubes(g)])
    w["col"] = col
    s = _latched(w, avoid=None)
    if mode == "grid":
        s.set_collision_grid_nearest(True)
        s.set_collision_grid(g.occ, g.origin, g.h)
    s.set_collision_avoidance(**AVOID)
    K, CALLS = 20, 40   # a timed window is 40 calls of 20 steps, about 0.3 s
    times = []
    for i in range(7):
        t0 = time.perf_counter()
        for _ in range(CALLS if i >= 2 else 1):
            out = s.SolvePose(w["tg"], dt=0.05, gain=0.2, tol_pose=1e-9, max_steps=K, q=w["q0"])
        times.append((time.perf_counter() - t0) / (K * (CALLS if i >= 2 else 1)))
    q = s.get("q")
    s.close()
    print(json.dumps(dict(lib="parent" if lib else "this", mode=mode, B=int(w["B"]), step_s=sorted(times[2:]), narrowed=float((out["avoid_active_steps"] > 0).mean()),
                          qsum=float(np.abs(q).sum()), nwb=int(col["wb"].shape[0]))))


def hbm(lib):
    """one line of JSON: seconds per avoidance_box call on the 330-joint tree (the HBM instantiation of k_avoid_box), 2048 configurations,
    100 spheres, 3 world spheres and 2 boxes, self pairs, no grid"""
    import numpy as np
    capi = _load(lib)
    import gridnear_cases as GC
    from test_avoid_box import DT, PRM
    from test_clearance import _open
    c = GC.avoid_case("tree330")
    q = c["model"].random_configurations(np.random.default_rng(5), 2048)
    s = _open(c["model"], q)
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    dq = capi.DeviceArray(q)
    n, nv, ns = q.shape[0], c["model"].nv, len(c["links"])
    outs = (capi.DeviceArray(np.zeros((n, nv))), capi.DeviceArray(np.zeros((n, nv))), capi.DeviceArray(np.zeros((n, ns, 2))), capi.DeviceArray(np.zeros((n * ns * 2 + 1) // 2)))
    CALLS = 100
    times = []
    for i in range(7):
        t0 = time.perf_counter()
        for _ in range(CALLS if i >= 2 else 1):
            s.avoidance_box(dq, DT, -1.0, 1.0, out=outs, **PRM)
        times.append((time.perf_counter() - t0) / (CALLS if i >= 2 else 1))
    s.close()
    print(json.dumps(dict(lib="parent" if lib else "this", mode="hbm", n=n, ns=ns, call_s=sorted(times[2:]))))


def sets():
    import numpy as np
    capi = _load(None)
    import grid_numpy as GN
    import qp_cases as QC
    from test_clearance import _open
    from test_grid_build import _DeviceBytes
    model = QC.model_of("panda7")
    for dims, frac in (((256, 256, 256), 0.005), ((25, 21, 17), 0.002)):
        occ = GN.random_occupancy(dims, frac, 7)
        dev = _DeviceBytes(occ)
        a, b = (_open(model, model.random_configurations(np.random.default_rng(1), 2)) for _ in range(2))
        b.set_collision_grid_nearest(True)
        ta, tb = [], []
        for i in range(12):
            for s, t in ((a, ta), (b, tb)):
                t0 = time.perf_counter()
                s.set_collision_grid(dev, (0.0, 0.0, 0.0), 0.01)
                t.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        a.set_collision_grid_nearest(True)
        latch = time.perf_counter() - t0
        same = bool(np.array_equal(a.collision_grid_nearest(), b.collision_grid_nearest()))
        print(json.dumps(dict(dims=dims, occupied=int(occ.sum()), set_unlatched_s=sorted(ta[2:]), set_latched_s=sorted(tb[2:]), latch_on_existing_grid_s=latch, same=same)))
        a.close(); b.close()


if __name__ == "__main__":
    if len(sys.argv) > 1:
        lib = PARENT if sys.argv[1] == "parent" else None
        hbm(lib) if sys.argv[2] == "hbm" else step(lib, sys.argv[2])
    else:
        sets()
        for rnd in range(3):
            for lib, mode in ((("parent", "nogrid"), ("parent", "hbm")) if PARENT else ()) + (("this", "nogrid"), ("this", "grid"), ("this", "boxes"), ("this", "hbm")):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), lib, mode], capture_output=True, text=True, timeout=240)
                print(r.stdout.strip().splitlines()[-1] if r.returncode == 0 and r.stdout.strip() else "FAILED %s %s rc=%d %s" % (lib, mode, r.returncode, r.stderr[-800:]))
                if r.returncode != 0:
                    sys.exit(1)
