"""Talos-32, 4096 instances, 2 spheres per link, self pairs on, the world of tests/test_clearance.py (33 spheres, 32 boxes): one SolvePose
with collision avoidance set, then one clearance query of the same 4096 configurations (k_clearance, the yardstick of stages 1-3 of
k_avoid_box).  Meant to run under a kernel trace of its own,
    rocprofv3 --kernel-trace --stats -d OUT -o avoid -- python scripts/measure_avoidance.py
whose per-kernel totals go into profiles/avoidance_measured.md.  Prints the pose loop's own timing and results as one JSON line.  One
process; run it under a timeout."""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loik_amd
from test_pose_ik import _handle, _links
from test_pose_parity import _seeds
import clearance_numpy as CN
import test_clearance as TC

B, STEPS = 4096, 8
AVOID = dict(d_safe=0.02, d_influence=0.15, kappa=0.5)


def main():
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 1)
    q0, tg = _seeds(model, B, links, seed=3, spread=(1e-2, 0.3))
    s, _ = _handle(model, B, links, q0)
    lk, sph = CN.make_spheres(model, 2, 410)
    c = TC._case("talos32")
    s.set_collision_spheres(lk, sph)
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    s.set_collision_avoidance(**AVOID)
    out = s.SolvePose(tg, dt=0.25, gain=0.5, tol_pose=1e-4, max_steps=STEPS)
    t = s.pose_timing()
    clr = s.clearance()
    res = dict(robot="talos32", B=B, nv=model.nv, spheres=int(lk.size), self_pairs=s.num_self_pairs(), world="33 spheres, 32 boxes", avoid=AVOID,
               steps=t["steps"], total_ms=t["total_ms"], solve_ms=t["solve_ms"], narrowed=float((out["avoid_active_steps"] > 0).mean()),
               reached=float(out["reached"].mean()), min_seen=float(np.nanmin(out["avoid_min_seen"])), final_min=float(clr["min"].min()))
    s.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
