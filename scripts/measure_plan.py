"""Talos-32 in the world of tests/test_clearance._case (two spheres per link, 33 world spheres, 32 boxes, the self pairs), B = 4096 queries
between random configurations, margin = the 10 % quantile of the clearance over the ends, step 0.5, 64 iterations, 64 nodes per tree, 64
samples per edge, T = 32: the outcomes of one plan_paths call by status, its time with device pointers, the same with a budget of 16
iterations and with none (the direct checks alone), the checks per second, and the registers, LDS and scratch of the kernel read from the
library's gfx950 code object.  Host clock around calls that end in a device synchronise; --short: 3 timed calls per figure and 1024
queries.  Prints one JSON line and writes profiles/plan_measured.md (or --out PATH); --accuracy FILE adds the lines tests/test_plan.py
prints.  One process; run it under a timeout."""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import loik_amd
from loik_amd import capi
import measure_clearance as MC
import test_clearance as TC

SHORT = "--short" in sys.argv
REPS = 3 if SHORT else 10
B, T = (1024 if SHORT else 4096), 32
NAMES = ("FOUND", "EXHAUSTED_ITERS", "EXHAUSTED_NODES", "START_BLOCKED", "GOAL_BLOCKED", "TOO_LONG", "INVALID")


def main():
    import torch
    c = TC._case("talos32")
    model = c["model"]
    nq = model.nq
    rng = np.random.default_rng(1300)
    start, goal = model.random_configurations(rng, B), model.random_configurations(rng, B)
    s = TC._open(model, c["q"])
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    ends = np.concatenate([start, goal])
    margin = float(np.quantile(s.clearance(ends)["min"], 0.1))
    lo, hi = ends.min(axis=0) - 0.5, ends.max(axis=0) + 0.5      # (talos32: every DoF a plain sum, coordinate j is DoF j)
    kw = dict(step=0.5, max_iters=64, max_nodes=64, seed=4242, margin=margin, tol=1e-3, max_evals=64)
    ref = s.plan_paths(start, goal, lo, hi, T, **kw)
    found = ref["status"] == capi.PLAN_FOUND
    chk = s.path_clearance(np.ascontiguousarray(ref["q_path"][found]), margin=margin, tol=1e-3, max_evals=64)
    assert np.all(chk["status"] == capi.MOTION_FREE) and np.array_equal(s.path_length(np.ascontiguousarray(ref["q_path"][found])), ref["length"][found])
    dev = torch.device("cuda:0")
    ds, dg = torch.from_numpy(start).to(dev), torch.from_numpy(goal).to(dev)
    outs = (torch.empty((B, T, nq), dtype=torch.float64, device=dev), torch.empty((B, 8), dtype=torch.int32, device=dev),
            torch.empty(B, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    full = MC.timed(lambda: s.plan_paths(ds, dg, lo, hi, T, out=outs, **kw), lambda: None, reps=REPS)
    assert np.array_equal(outs[0].cpu().numpy(), ref["q_path"], equal_nan=True) and np.array_equal(outs[1].cpu().numpy()[:, 0], ref["status"])
    sixteen = MC.timed(lambda: s.plan_paths(ds, dg, lo, hi, T, out=outs, **dict(kw, max_iters=16)), lambda: None, reps=REPS)
    r16 = outs[1].cpu().numpy()
    direct = MC.timed(lambda: s.plan_paths(ds, dg, lo, hi, T, out=outs, **dict(kw, max_iters=0)), lambda: None, reps=REPS)
    r0 = outs[1].cpu().numpy()
    host = MC.timed(lambda: s.plan_paths(start, goal, lo, hi, T, **kw), lambda: None, reps=REPS)
    res = MC.code_object_resources(r"k_plan_paths|k_shortcut_paths")
    by = lambda st: {n: int((st == k).sum()) for k, n in enumerate(NAMES)}
    out = dict(B=B, T=T, margin=margin, kw={k: v for k, v in kw.items()}, outcomes=by(ref["status"]), outcomes_16=by(r16[:, 0]), outcomes_0=by(r0[:, 0]),
               iterations_of_found=dict(median=float(np.median(ref["iterations"][found])), max=int(ref["iterations"][found].max())),
               waypoints_of_found=dict(median=float(np.median(ref["n_waypoints"][found])), max=int(ref["n_waypoints"][found].max())),
               nodes_max=int(ref["nodes"].max()), edges_checked=int(ref["edges_checked"].sum()), edges_free=int(ref["edges_free"].sum()),
               evals=int(ref["evals"].astype(np.int64).sum()), full=full, sixteen=sixteen, direct=direct, host_pointers=host, resources=res)
    print(json.dumps(out))
    s.close()
    tail_ms = full["median_ms"] - sixteen["median_ms"]
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    row = lambda what, r: "| %s | %.3f | %.3f .. %.3f |" % (what, r["median_ms"], r["min_ms"], r["max_ms"])
    cnt = lambda d: ", ".join("%s %d" % (n, d[n]) for n in NAMES if d[n])
    md = ["# Planning: batched RRT-Connect with certified edges", "",
          "One MI355X, talos32 (nq = nv = 32), fp64.  Recorded, not gated.  `python scripts/measure_plan.py` took the figures and wrote this file:",
          "every call is warmed up three times and timed %d times.  %d queries between random configurations in the world of" % (REPS, B),
          "`tests/test_clearance._case` (64 robot spheres, 33 world spheres, 32 boxes, the self pairs); margin = %.4f, the 10 %% quantile of the" % margin,
          "clearance over the ends; ranges = the box of the ends widened by 0.5; step 0.5, 64 nodes per tree, at most 64 samples per edge, T = %d." % T, "",
          "## Outcomes", "",
          "| budget | outcomes |", "|---|---|",
          "| 64 iterations | %s |" % cnt(out["outcomes"]), "| 16 iterations | %s |" % cnt(out["outcomes_16"]), "| 0 iterations (the direct checks) | %s |" % cnt(out["outcomes_0"]), "",
          "With 64 iterations the found paths took a median of %.0f iterations (at most %d) and have a median of %.0f waypoints (at most %d); the largest" % (
              out["iterations_of_found"]["median"], out["iterations_of_found"]["max"], out["waypoints_of_found"]["median"], out["waypoints_of_found"]["max"]),
          "tree holds %d nodes.  The call checked %d edges (%d FREE) with %d samples.  Every segment of every found path is `MOTION_FREE` under" % (
              out["nodes_max"], out["edges_checked"], out["edges_free"], out["evals"]),
          "`path_clearance` and every length equals `path_length`'s, bit for bit (asserted by the script).", "",
          "## Call times (host clock around calls that end in a device synchronise; profiler off)", "",
          "| what | median (ms) | min .. max (ms) |", "|---|---|---|",
          row("`plan_paths`, 64 iterations, device pointers", full), row("the same, 16 iterations", sixteen),
          row("the same, 0 iterations: two checks per query", direct), row("64 iterations, host pointers", host), "",
          "That is %.2f million certified edges and %.1f million samples (forward kinematics of 32 joints, 64 centres, %d pairs) per second." % (
              out["edges_checked"] / full["median_ms"] / 1e3, out["evals"] / full["median_ms"] / 1e3, 64 * 65 + len(c["pairs"])),
          "A query is one wavefront, so the call lasts as long as its slowest queries: after 16 iterations %d of %d queries still run, and the 48" % (out["outcomes_16"]["EXHAUSTED_ITERS"], B),
          "further iterations they may use cost %.1f ms, about %.2f ms per iteration of a lone wavefront: a few edges of up to 64 samples each." % (tail_ms, tail_ms / 48.0),
          "Nobody has tuned this kernel; no time is promised.", "",
          "## Registers, LDS and scratch (the notes of the gfx950 code object in libloik_amd.so)", "",
          "| kernel symbol | VGPRs | SGPRs | static LDS (bytes) | scratch (bytes/lane) |", "|---|---|---|---|---|"]
    md += ["| `%s` | %d | %d | %d | %d |" % (k, v["vgpr"], v["sgpr"], v["lds"], v["scratch"]) for k, v in sorted(res.items())]
    md += ["", "`k_plan_paths` sits where `k_shortcut_paths` sits: the advancement (`motion_advance`, inlined once) sets the register count, and the",
           "80 bytes of scratch per lane are `difference_joint`'s dynamically indexed rotation, as in `k_shortcut_paths` and `k_difference`.  The",
           "two checks of step 0 and every extension of an iteration are trips of one loop body, so the kernel holds one copy of the advancement, one",
           "of the nearest-node search and three of `difference_joint` (the search, `dv` towards the target, `dv` of the edge) plus `path_length_wave`'s.",
           "Two wavefronts per SIMD fit the registers; dynamic LDS is what `k_shortcut_paths` takes (talos32: 64 centres, the records and `dv`:",
           "%d bytes), the trees are global: per resident wavefront 2 x max_nodes rows of nq doubles, the sample and the parents." % (8 * (4 * 64 + 64 + 12 * 32 + 12 * 32 + 32)), "",
           "## The layout of the nearest-node search", "",
           "The trees are row-major `[node][nq]`, the row the check reads; there is no coordinate-major copy.  A lane owns a node and walks its row",
           "front to back, so a load instruction of the wavefront touches up to 64 cache lines, but each of those lines is used up by the same lane's next",
           "loads (16 doubles per 128-byte line), and the trees of this workload are small (at most %d nodes, %d KB per tree: L2-resident, mostly" % (out["nodes_max"], out["nodes_max"] * nq * 8 // 1024 + 1),
           "one trip of the lane loop).  A search is one pass over n rows, for talos32 32 subtractions and multiply-adds per lane, against an",
           "advancement of up to max_evals samples of the whole sphere model per edge; an iteration of a lone wavefront costs about %.2f ms (above)." % (tail_ms / 48.0),
           "The search was not timed on its own.  A coordinate-major copy would double the scratch and add a scattered store per new node; it was",
           "not built and not measured, and is worth measuring once trees reach thousands of nodes."]
    if arg("--accuracy"):
        lines = [l.lstrip(".").strip() for l in open(arg("--accuracy"), errors="replace") if l.lstrip(".").startswith("plan_measured")]   # (pytest -s puts its dots in front)
        md += ["", "## What the tests print (tests/test_plan.py, one MI355X)", "", "```"] + lines + ["```", "",
               "The bound of test 1, `PLAN_BOUND`, is 16 times the largest of the errors above."]
    path = arg("--out", os.path.join(ROOT, "profiles", "plan_measured.md"))
    open(path, "w").write("\n".join(md) + "\n")


if __name__ == "__main__":
    main()
