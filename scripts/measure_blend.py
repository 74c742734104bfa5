"""Talos-32, the 4096 paths of 32 waypoints, the limits and the period of scripts/measure_retime.py, the spheres and the world of
test_clearance._case: the time of one blend_paths call with device pointers beside retime_paths on the same paths, the ratio of the
durations, how the corners end, and the registers, LDS and scratch of the new kernel read from the library's gfx950 code object.  Host
clock around calls that end in a device synchronise; --short: 3 timed calls per figure.  Prints one JSON line and writes
profiles/blend_measured.md (or --out PATH); --accuracy FILE adds the error lines tests/test_blend.py prints.  Recorded, not gated.  One
process; run it under a timeout."""
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
B, T, S, SIZE = 4096, 32, 256, 0.08
MAX_EVALS, MAX_TRIES, TOL = 64, 3, 1e-3


def main():
    import torch
    c = TC._case("talos32")
    model = c["model"]
    nq, nv = model.nq, model.nv
    rng = np.random.default_rng(900)
    rows = [model.random_configurations(rng, B)]
    for _ in range(T - 1):
        rows.append(rows[-1] + SIZE * rng.uniform(-1.0, 1.0, size=(B, nv)))
    paths = np.ascontiguousarray(np.stack(rows, axis=1))
    j = np.arange(nv)
    v_max, a_max = SIZE * (2.0 + 0.25 * (j % 5)), SIZE * (4.0 + 1.5 * (j % 3))
    s = TC._open(model, c["q"])
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    longest = float(s.retime_paths(paths, v_max, a_max, 1.0, max_samples=0)["duration"].max())
    dt = longest / (S - 1.5)
    margin = float(np.quantile(s.clearance(paths.reshape(-1, nq))["min"], 0.1))
    reach = 0.2 * SIZE * np.sqrt(nv)
    kw = dict(v_max=v_max, a_max=a_max, dt=dt, max_samples=S)
    bkw = dict(kw, reach=reach, margin=margin, tol=TOL, max_evals=MAX_EVALS, max_tries=MAX_TRIES)
    ref = s.retime_paths(paths, **kw)
    got = s.blend_paths(paths, **bkw)
    assert np.all(ref["flags"] == 0) and np.all(got["flags"] == 0)
    dev = torch.device("cuda:0")
    paths_t = torch.from_numpy(paths).to(dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    routs = (f64(B, S, nq), f64(B, S, nv), f64(B, T - 1, 4), f64(B), i32(B, 4))
    bouts = (f64(B, S, nq), f64(B, S, nv), f64(B), i32(B, 4), f64(B, T - 2, 5), i32(B, T - 2, 6), f64(B, 2 * T - 3, 4))
    torch.cuda.synchronize()
    retime = MC.timed(lambda: s.retime_paths(paths_t, out=routs, **kw), lambda: None, reps=REPS)
    blend = MC.timed(lambda: s.blend_paths(paths_t, out=bouts, **bkw), lambda: None, reps=REPS)
    assert np.array_equal(bouts[0].cpu().numpy(), got["q_traj"])
    off = MC.timed(lambda: s.blend_paths(paths_t, out=bouts, **dict(bkw, max_tries=0)), lambda: None, reps=REPS)
    timing = MC.timed(lambda: s.blend_paths(paths_t, out=(None, None) + bouts[2:], **bkw), lambda: None, reps=REPS)
    st = got["corner_info"][:, :, 0]
    counts = {k: int(np.sum(st == getattr(capi, "BLEND_" + k))) for k in ("TAKEN", "BLOCKED", "UNDECIDED", "COUPLED", "ZERO_LEG", "OFF")}
    ratio = got["duration"] / ref["duration"]
    res = MC.code_object_resources(r"k_blend_paths|k_retime_paths")
    out = dict(B=B, T=T, S=S, dt=dt, margin=margin, reach=reach, retime=retime, blend=blend, blend_no_tries=off, blend_timing_only=timing, corners=counts,
               evals_mean=float(got["corner_info"][:, :, 2].mean()), ratio_mean=float(ratio.mean()), ratio_min=float(ratio.min()), ratio_max=float(ratio.max()),
               resources=res)
    print(json.dumps(out))
    s.close()
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    row = lambda what, r: "| %s | %.3f | %.3f .. %.3f |" % (what, r["median_ms"], r["min_ms"], r["max_ms"])
    md = ["# Blending: retiming through certified corners beside the stop at every waypoint", "",
          "One MI355X, talos32 (nq = nv = 32), fp64.  Recorded, not gated.  `python scripts/measure_blend.py` took the figures and wrote this file:",
          "every call is warmed up three times and timed %d times.  The %d paths of %d waypoints, the limits and dt = %.6f s of" % (REPS, B, T, dt),
          "`profiles/retime_measured.md`; the spheres, the world and the self pairs of the clearance tests; margin %.4f (the 10 %% quantile of the" % margin,
          "clearance over all waypoints), tol %g, reach %.4f, max_evals %d, max_tries %d." % (TOL, reach, MAX_EVALS, MAX_TRIES), "",
          "## Call times (host clock around calls that end in a device synchronise; device inputs and outputs; profiler off)", "",
          "| what | median (ms) | min .. max (ms) |", "|---|---|---|",
          row("`retime_paths`", retime), row("`blend_paths`", blend), row("`blend_paths`, timing only (`out_traj` NULL)", timing),
          row("`blend_paths` with `max_tries = 0` (no corner is tried)", off), "",
          "## What the corners came to, and what it buys", "",
          "Corners: %s; %.1f samples of the advancement per corner on average." % (", ".join("%s %d" % kv for kv in counts.items()), out["evals_mean"]),
          "Duration of the blended trajectory over the duration of `retime_paths`, per path: mean %.3f, least %.3f, largest %.3f." % (out["ratio_mean"], out["ratio_min"], out["ratio_max"]), "",
          "## Registers, LDS and scratch (the notes of the gfx950 code object in libloik_amd.so)", "",
          "| kernel symbol | VGPRs | SGPRs | static LDS (bytes) | scratch (bytes/lane) |", "|---|---|---|---|---|"]
    md += ["| `%s` | %d | %d | %d | %d |" % (k, v["vgpr"], v["sgpr"], v["lds"], v["scratch"]) for k, v in sorted(res.items())]
    if arg("--accuracy"):
        lines = [l.lstrip(".F").strip() for l in open(arg("--accuracy"), errors="replace") if l.lstrip(".F").startswith("blend_measured")]   # (pytest -s puts its dots in front)
        md += ["", "## What the tests print (tests/test_blend.py, one MI355X)", "", "```"] + lines + ["```"]
    path = arg("--out", os.path.join(ROOT, "profiles", "blend_measured.md"))
    open(path, "w").write("\n".join(md) + "\n")


if __name__ == "__main__":
    main()
