"""Voxel worlds (include/loik_amd_grid.h) on one MI355X: the time to build the distance field at three sizes, motion_clearance over the
segments of tests/test_motion_clearance.motion_case("panda7") against a world of one box per occupied voxel of a 32^3 grid at 5 % and
against the same world as a grid, and -- with --parent DIR, a directory that holds the parent commit's loik_amd package with its built
library -- the same N-box timing from the parent's build, alternated with this one's, and a byte comparison of what clearance,
motion_clearance, shortcut_paths, plan_paths and blend_paths return without a grid from the two builds.

The parent process starts one worker process per build and round (a library is loaded once per process); a worker prints one JSON line
and writes its raw outputs to a file.  Host clock around calls that end in a device synchronise, host inputs and outputs (device ones for the two clearance
calls that fill the chip), profiler off.
Writes profiles/grid_measured.md (or --out PATH).  Run it under a timeout."""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ROUNDS, REPS, TILE = 3, 20, 64
FILL = 32768      # configurations of a clearance call that fills the chip: 256 CUs x 4 SIMDs x 8 wavefronts is 8192
SIZES = ((64, 64, 64), (128, 128, 128), (256, 256, 128))
GRID_N, GRID_H, GRID_FRAC, GRID_ORIGIN = 32, 0.05, 0.05, (-0.8, -0.8, -0.4)


def _arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def _times(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(out)), float(np.min(out)), float(np.max(out))]


def voxel_world():
    """the occupancy [32][32][32] and the same world as boxes [N][15], one per occupied voxel"""
    occ = (np.random.default_rng(2024).uniform(size=(GRID_N,) * 3) < GRID_FRAC).astype(np.uint8)
    boxes = []
    for z, y, x in np.argwhere(occ):
        ctr = np.array(GRID_ORIGIN) + (np.array([x, y, z]) + 0.5) * GRID_H
        boxes.append(np.concatenate([np.eye(3).reshape(9), ctr, np.full(3, 0.5 * GRID_H)]))
    return occ, np.array(boxes)


def worker(dump):
    """runs in a process of its own with the package of one build on its path"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_motion_clearance as TM
    import test_plan as TPL
    import test_shortcut as TS
    c = TM.motion_case("panda7")
    model = c["model"]
    res, raw = {}, []

    def keep(r):
        raw.extend(np.ascontiguousarray(r[k]).tobytes() for k in sorted(r) if r[k] is not None)

    # 1. one small case per kernel without a grid: the bytes
    s = TM._open(c)
    keep(s.clearance(c["q"]))
    keep(s.motion_clearance(c["qa"], dv=c["dv"], margin=c["margin"], tol=TM.TOL, max_evals=TM.MAX_EVALS))
    paths = TS.make_paths(model, c["q"][:16], TM.SIZE["panda7"], 8, np.random.default_rng(77))
    keep(s.shortcut_paths(paths, rounds=16, seed=5, margin=c["margin"], tol=TM.TOL, max_evals=TM.MAX_EVALS))
    keep(s.blend_paths(paths, np.full(model.nv, 1.0), np.full(model.nv, 2.0), 0.05, 0.2, margin=c["margin"], tol=TM.TOL, max_evals=TM.MAX_EVALS))
    s.close()
    pc = TPL.case("panda7")
    s = TM._open(pc)
    keep(TPL._plan(s, pc))
    s.close()
    # 1b. the two instantiations that lose a wavefront per SIMD to the grid branch (models whose records do not fit the LDS): tree330
    import test_clearance as TC
    c3 = TC._case("tree330")
    s = TM._open(c3)
    from loik_amd import capi as _capi
    outs = (_capi.DeviceArray(np.zeros(3 * FILL)), _capi.DeviceArray(np.zeros(3 * FILL // 2)))      # min [n][3] doubles, witness [n][3] ints
    q3 = _capi.DeviceArray(np.tile(c3["q"], (FILL // 3 + 1, 1))[:FILL])      # (device inputs and outputs: the call is the kernels' time)
    res["t_clearance_tree330"] = _times(lambda: s.clearance(q3, out=outs), reps=10)
    s.close()
    q3.free()
    # ... and a 700-joint tree with 64 spheres: k_clearance<true> again (12 * 700 doubles of records alone pass 64 KB), with 2 KB of LDS a
    # wavefront, so that the registers, not the LDS, decide how many wavefronts a SIMD holds
    from helpers import random_tree
    import clearance_numpy as CN
    big = random_tree(54, 700)
    rng = np.random.default_rng(55)
    lk = np.linspace(1, big.njoints - 1, 64).astype(np.int32)
    _, sph = CN.make_spheres(big, 1, 56, links=lk)
    qb = big.random_configurations(rng, 8)
    s = TC._open(big, qb)
    s.set_collision_spheres(lk, sph)
    s.set_collision_world(*TC._world(rng, 33, 32))
    keep(s.clearance(qb))
    qfill = _capi.DeviceArray(np.tile(qb, (FILL // 8, 1)))
    res["t_clearance_tree700"] = _times(lambda: s.clearance(qfill, out=outs), reps=10)
    s.close()
    qfill.free()
    pc3 = TPL.case("tree330")
    s = TM._open(pc3)
    start3, goal3 = np.tile(pc3["start"], (64, 1)), np.tile(pc3["goal"], (64, 1))
    res["t_plan_tree330"] = _times(lambda: s.plan_paths(start3, goal3, pc3["lo"], pc3["hi"], TPL.T_PLAN, **pc3["kw"]), reps=10)
    s.close()
    res["bytes"] = int(sum(len(b) for b in raw))
    res["sha256"] = hashlib.sha256(b"".join(raw)).hexdigest()
    with open(dump, "wb") as f:
        f.write(b"".join(raw))

    # 2. motion_clearance against the voxels as boxes, and as a grid
    occ, boxes = voxel_world()
    qa, dv = np.tile(c["qa"], (TILE, 1)), np.tile(c["dv"], (TILE, 1))
    margin = -1.0      # (below every clearance: no segment ends at its first sample)
    s = TM._open(c)
    s.set_self_collision(False)
    s.set_collision_world(None, boxes)
    kw = dict(margin=margin, tol=TM.TOL, max_evals=TM.MAX_EVALS)
    r_box = s.motion_clearance(c["qa"], dv=c["dv"], **kw)
    clr_box = s.clearance(c["q"])["min"]
    res["n_boxes"], res["n_spheres"], res["segments"] = int(boxes.shape[0]), int(len(c["links"])), [int(c["qa"].shape[0]), int(qa.shape[0])]
    res["boxes_status"] = np.bincount(r_box["status"], minlength=4).tolist()
    res["boxes_evals"] = int(r_box["evals"].sum())
    res["t_boxes"] = _times(lambda: s.motion_clearance(c["qa"], dv=c["dv"], **kw))
    res["t_boxes_tiled"] = _times(lambda: s.motion_clearance(qa, dv=dv, **kw))
    if hasattr(s, "set_collision_grid"):
        s.set_collision_world(None, None)
        s.set_collision_grid(occ, GRID_ORIGIN, GRID_H)
        r_grid = s.motion_clearance(c["qa"], dv=c["dv"], **kw)
        res["grid_status"] = np.bincount(r_grid["status"], minlength=4).tolist()
        res["grid_evals"] = int(r_grid["evals"].sum())
        # the grid's bound never exceeds the boxes' exact clearance, and stays within sqrt(3) h of it inside the grid
        clr_grid = s.clearance(c["q"])["min"]
        res["grid_above_boxes"] = int(np.sum(clr_grid > clr_box + 1e-12))
        res["grid_below_boxes_max"] = float(np.max(clr_box - clr_grid))
        res["t_grid"] = _times(lambda: s.motion_clearance(c["qa"], dv=c["dv"], **kw))
        res["t_grid_tiled"] = _times(lambda: s.motion_clearance(qa, dv=dv, **kw))
        res["t_set_32"] = _times(lambda: s.set_collision_grid(occ, GRID_ORIGIN, GRID_H))
        # 3. the builder
        from loik_amd import capi
        res["build"] = {}
        for dims in SIZES:
            big = (np.random.default_rng(sum(dims)).uniform(size=dims[::-1]) < 0.05).astype(np.uint8)
            raw8 = np.zeros((big.size + 7) // 8 * 8, dtype=np.uint8)
            raw8[:big.size] = big.ravel()
            dev = capi.DeviceArray(raw8.view(np.float64))

            class Dev:
                shape, is_cuda = big.shape, True
                data_ptr = staticmethod(dev.data_ptr)
                element_size = staticmethod(lambda: 1)
            res["build"]["x".join(str(d) for d in dims)] = dict(
                host=_times(lambda: s.set_collision_grid(big, (0, 0, 0), 0.02), reps=10),
                device=_times(lambda: s.set_collision_grid(Dev, (0, 0, 0), 0.02), reps=10))
            dev.free()
    s.close()
    print("MEASURE_GRID " + json.dumps(res))


def run_worker(pkg_dir, dump):
    env = dict(os.environ, PYTHONPATH=pkg_dir + os.pathsep + ROOT)      # (the tests import oracle/ from the root; the package comes from pkg_dir)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", dump], env=env, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
        raise SystemExit("worker for %s ended with %d" % (pkg_dir, out.returncode))
    line = [l for l in out.stdout.splitlines() if l.startswith("MEASURE_GRID ")][-1]
    return json.loads(line[len("MEASURE_GRID "):])


def fmt(t):
    return "%.3f (%.3f .. %.3f)" % tuple(t)


def main():
    parent = _arg("--parent")
    out_path = _arg("--out", os.path.join(ROOT, "profiles", "grid_measured.md"))
    tmp = _arg("--tmp", "/tmp")
    regs = _arg("--registers")
    new, old = [], []
    for r in range(ROUNDS):      # alternating: the two builds see the same neighbours on the machine
        if parent:
            old.append(run_worker(os.path.abspath(parent), os.path.join(tmp, "grid_parent.bin")))
        new.append(run_worker(ROOT, os.path.join(tmp, "grid_this.bin")))
    n = new[-1]
    L = ["# Voxel worlds: the builder, the query, and what stayed as it was", "",
         "One MI355X, fp64.  Recorded, not gated.  `python scripts/measure_grid.py --parent DIR` took the figures and wrote this file: every call is",
         "warmed up three times and timed %d times (the builder 10) with the host clock around calls that are complete on return; %d worker" % (REPS, ROUNDS),
         "processes per build, this build's and the parent commit's alternating.  Times are median (min .. max) in ms.", "",
         "## The builder (`loikb_collision_set_world_grid`, 5 % of the voxels occupied)", "",
         "| nx x ny x nz | host occupancy (upload included) | device occupancy (`LOIKB_IN_DEVICE`) |", "|---|---|---|"]
    for k, v in n.get("build", {}).items():
        L.append("| %s | %s | %s |" % (k, fmt(v["host"]), fmt(v["device"])))
    L += ["", "The 32^3 grid of the next section, host occupancy: %s." % fmt(n["t_set_32"]), "",
          "## `motion_clearance`: one box per occupied voxel against the grid", "",
          "panda7 with the %d spheres of tests/test_clearance._case, self pairs off, the segments of tests/test_motion_clearance.motion_case(\"panda7\")" % n["n_spheres"],
          "(%d; and tiled %d times, %d), margin -1 so that no segment ends at its first sample, tol 1e-3, max_evals %d.  The world is a %d^3 grid of" % (
              n["segments"][0], TILE, n["segments"][1], 12, GRID_N),
          "%.2f m voxels, 5 %% occupied: %d boxes, or one grid." % (GRID_H, n["n_boxes"]), "",
          "| world | build | %d segments | %d segments |" % tuple(n["segments"]), "|---|---|---|---|"]
    for i, r in enumerate(new):
        L.append("| %d boxes | this, run %d | %s | %s |" % (r["n_boxes"], i + 1, fmt(r["t_boxes"]), fmt(r["t_boxes_tiled"])))
    for i, r in enumerate(old):
        L.append("| %d boxes | parent, run %d | %s | %s |" % (r["n_boxes"], i + 1, fmt(r["t_boxes"]), fmt(r["t_boxes_tiled"])))
    for i, r in enumerate(new):
        L.append("| the grid | this, run %d | %s | %s |" % (i + 1, fmt(r["t_grid"]), fmt(r["t_grid_tiled"])))
    med = lambda rs, k: float(np.median([r[k][0] for r in rs]))
    L += ["", "Samples taken over the %d segments: %d against the boxes (statuses free / blocked / undecided / invalid %s), %d against the grid (%s):" % (
        n["segments"][0], n["boxes_evals"], n["boxes_status"], n["grid_evals"], n["grid_status"]),
          "the grid's bound is below the boxes' distance by up to sqrt(3) h, so its steps can be shorter and its samples more.  Of the %d start configurations, those whose" % n["segments"][0],
          "clearance against the grid exceeds the one against the boxes: %d; the largest amount by which it is below: %.4f m (sqrt(3) h = %.4f)." % (
              n["grid_above_boxes"], n["grid_below_boxes_max"], 3 ** 0.5 * GRID_H), "",
          "Boxes over grid, medians of the runs' medians: %.2f at %d segments, %.2f at %d." % (
              med(new, "t_boxes") / med(new, "t_grid"), n["segments"][0], med(new, "t_boxes_tiled") / med(new, "t_grid_tiled"), n["segments"][1])]
    if old:
        L += ["This build over the parent's on the boxes: %.3f at %d segments, %.3f at %d; the runs of one build differ by up to %.1f %% and %.1f %%." % (
            med(new, "t_boxes") / med(old, "t_boxes"), n["segments"][0], med(new, "t_boxes_tiled") / med(old, "t_boxes_tiled"), n["segments"][1],
            100 * max(np.ptp([r["t_boxes"][0] for r in rs]) / med(rs, "t_boxes") for rs in (new, old)),
            100 * max(np.ptp([r["t_boxes_tiled"][0] for r in rs]) / med(rs, "t_boxes_tiled") for rs in (new, old))), "",
              "## Without a grid, against the parent commit's build", "",
              "clearance, motion_clearance, shortcut_paths, blend_paths (the panda7 case of tests/test_motion_clearance.py, 16 paths of 8 waypoints) and",
              "plan_paths (tests/test_plan.case(\"panda7\")), every output array dumped raw: %d bytes from this build, %d from the parent's, sha256" % (n["bytes"], old[-1]["bytes"]),
              "%s and %s: %s." % (n["sha256"][:16], old[-1]["sha256"][:16], "identical byte for byte" if n["sha256"] == old[-1]["sha256"] and n["bytes"] == old[-1]["bytes"] else "THEY DIFFER")]
    if old:
        L += ["", "## The two instantiations that lose a wavefront per SIMD, no grid set", "",
              "Device inputs and outputs for the clearance calls, so that the time is the kernels'.", "", "| call | build | time |", "|---|---|---|"]
        for name, rs in (("this", new), ("parent", old)):
            for i, r in enumerate(rs):
                L.append("| `clearance`, tree330, 330 spheres, %d configurations (`k_clearance<true>`) | %s, run %d | %s |" % (FILL, name, i + 1, fmt(r["t_clearance_tree330"])))
        for name, rs in (("this", new), ("parent", old)):
            for i, r in enumerate(rs):
                L.append("| `clearance`, a 700-joint tree, 64 spheres, %d configurations (`k_clearance<true>`) | %s, run %d | %s |" % (FILL, name, i + 1, fmt(r["t_clearance_tree700"])))
        for name, rs in (("this", new), ("parent", old)):
            for i, r in enumerate(rs):
                L.append("| `plan_paths`, 128 queries of tests/test_plan.case(\"tree330\") (`k_plan_paths<true>`) | %s, run %d | %s |" % (name, i + 1, fmt(r["t_plan_tree330"])))
        L += ["", "This build over the parent's, medians of the runs' medians: clearance on tree330 %.3f, on the 700-joint tree %.3f, plan_paths %.3f." % (
            med(new, "t_clearance_tree330") / med(old, "t_clearance_tree330"), med(new, "t_clearance_tree700") / med(old, "t_clearance_tree700"),
            med(new, "t_plan_tree330") / med(old, "t_plan_tree330"))]
    if regs and os.path.exists(regs):
        L += ["", open(regs).read().rstrip()]
    with open(out_path, "w") as f:
        f.write("\n".join(L) + "\n")
    print(json.dumps(dict(this=new, parent=old)))


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker(_arg("--worker"))
    else:
        main()
