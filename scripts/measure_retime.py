"""Talos-32, 4096 paths of 32 waypoints (random starts, each next waypoint the last plus 0.08 * uniform(-1, 1) per DoF), limits
v_max_j = 0.08 (2 + 0.25 (j mod 5)), a_max_j = 0.08 (4 + 1.5 (j mod 3)) and the period that makes the longest path 256 samples: the time of
one retime_paths call with device pointers beside (a) the same work driven from the host through the older entry point (difference with
device pointers, the timing and the profile in numpy, the samples as plain sums in numpy -- talos32 has nq == nv -- and the upload of the
result), (b) the time the output bytes take at the HBM rate, and (c) shortcut_paths / path_length as scripts/measure_shortcut.py times
them, whose kernels share the fin / same helper with this one; and the registers, LDS and scratch of the kernels read from the library's
gfx950 code object.  Host clock around calls that end in a device synchronise; --short: 3 timed calls per figure.  Prints one JSON line
and writes profiles/retime_measured.md (or --out PATH); --accuracy FILE adds the error lines tests/test_retime.py prints, --bytes FILE the
outcome of the byte comparison of k_path_length's and k_shortcut_paths' outputs with the parent commit's.  One process; run it under a
timeout."""
import json
import os
import sys
import time

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
HBM_BYTES_PER_S = 6.3e12      # MI355X: what a streaming copy reaches of the 8 TB/s of HBM3E
PARENT = {"shortcut_paths": 115.194, "path_length": 0.096}     # profiles/shortcut_measured.md, the parent commit's medians (ms)


def host_retime(s, torch, paths_t, v_max, a_max, dt):
    """the rule of loik_amd_retime.h without SNAP for a robot whose (+) is a sum, the batch side by side: difference on the device, the
    rest in numpy; returns device tensors (q_traj [B][S][nq], v_traj [B][S][nv]) and the durations"""
    nq, nv = s.model.nq, s.model.nv
    dv_t = torch.empty((B * (T - 1), nv), dtype=torch.float64, device=paths_t.device)
    s.difference(paths_t[:, :-1].reshape(-1, nq).contiguous(), paths_t[:, 1:].reshape(-1, nq).contiguous(), out=dv_t)
    dv = dv_t.cpu().numpy().reshape(B, T - 1, nv)
    q = paths_t.cpu().numpy()
    cv, ca = np.max(np.abs(dv) / v_max, axis=2), np.max(np.abs(dv) / a_max, axis=2)
    tri = ca >= cv * cv
    rt = np.sqrt(ca)
    t_acc = np.where(tri, rt, ca / cv)
    D = np.where(tri, 2.0 * rt, cv + ca / cv)
    peak = np.where(tri, 1.0 / rt, 1.0 / cv)
    A = 1.0 / ca
    start = np.concatenate([np.zeros((B, 1)), np.cumsum(D, axis=1)], axis=1)
    total = start[:, -1]
    t = np.arange(S) * dt
    k = np.minimum((start[:, None, 1:] <= t[None, :, None]).sum(axis=2), T - 2)      # [B][S]: the last segment that has started
    rows = np.arange(B)[:, None]
    tau = t[None] - start[rows, k]
    Dk, ta, pk, Ak = D[rows, k], t_acc[rows, k], peak[rows, k], A[rows, k]
    rem = np.maximum(Dk - tau, 0.0)
    sv = np.where(tau < ta, 0.5 * Ak * tau * tau, np.where(tau <= Dk - ta, pk * (tau - 0.5 * ta), 1.0 - 0.5 * Ak * rem * rem))
    sd = np.where(tau < ta, Ak * tau, np.where(tau <= Dk - ta, pk, Ak * rem))
    past = t[None] >= total[:, None]
    sv, sd = np.where(past, 1.0, sv), np.where(past, 0.0, sd)
    traj = q[rows, k] + sv[:, :, None] * dv[rows, k]
    traj[past] = np.broadcast_to(q[:, None, -1], traj.shape)[past]
    vel = sd[:, :, None] * dv[rows, k]
    out = torch.from_numpy(traj).to(paths_t.device), torch.from_numpy(vel).to(paths_t.device)
    torch.cuda.synchronize()
    return out[0], out[1], total


def main():
    import torch
    c = TC._case("talos32")
    model = c["model"]
    assert model.nq == model.nv      # (plain sums: the host recipe's (+) is an addition)
    nq, nv = model.nq, model.nv
    rng = np.random.default_rng(900)
    rows = [model.random_configurations(rng, B)]
    for _ in range(T - 1):
        rows.append(rows[-1] + SIZE * rng.uniform(-1.0, 1.0, size=(B, nv)))
    paths = np.ascontiguousarray(np.stack(rows, axis=1))
    j = np.arange(nv)
    v_max, a_max = SIZE * (2.0 + 0.25 * (j % 5)), SIZE * (4.0 + 1.5 * (j % 3))
    s = TC._open(model, c["q"])
    longest = float(s.retime_paths(paths, v_max, a_max, 1.0, max_samples=0)["duration"].max())
    dt = longest / (S - 1.5)      # the longest path ends between samples S - 2 and S - 1: n_samples = S
    ref = s.retime_paths(paths, v_max, a_max, dt, max_samples=S)
    assert int(ref["n_samples"].max()) == S and np.all(ref["flags"] == 0)
    dev = torch.device("cuda:0")
    paths_t = torch.from_numpy(paths).to(dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    outs = (f64(B, S, nq), f64(B, S, nv), f64(B, T - 1, 4), f64(B), torch.empty((B, 4), dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    kw = dict(v_max=v_max, a_max=a_max, dt=dt, max_samples=S)
    fused = MC.timed(lambda: s.retime_paths(paths_t, out=outs, **kw), lambda: None, reps=REPS)
    assert np.array_equal(outs[0].cpu().numpy(), ref["q_traj"]) and np.array_equal(outs[1].cpu().numpy(), ref["v_traj"])
    snap = MC.timed(lambda: s.retime_paths(paths_t, out=outs, snap=True, **kw), lambda: None, reps=REPS)
    timing = MC.timed(lambda: s.retime_paths(paths_t, out=(None, None) + outs[2:], **kw), lambda: None, reps=REPS)
    no_vel = MC.timed(lambda: s.retime_paths(paths_t, out=(outs[0], None) + outs[2:], **kw), lambda: None, reps=REPS)
    hq, hv, hd = host_retime(s, torch, paths_t, v_max, a_max, dt)
    host_err = max(float(np.abs(hq.cpu().numpy() - ref["q_traj"]).max()), float(np.abs(hv.cpu().numpy() - ref["v_traj"]).max()),
                   float(np.abs(hd - ref["duration"]).max()))
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter(); host_retime(s, torch, paths_t, v_max, a_max, dt); t.append((time.perf_counter() - t0) * 1e3)
    host = dict(median_ms=float(np.median(t)), min_ms=float(min(t)), max_ms=float(max(t)), reps=REPS)
    out_bytes = 8 * B * (S * (nq + nv) + 4 * (T - 1) + 1) + 16 * B
    hbm_ms = out_bytes / HBM_BYTES_PER_S * 1e3
    # the two older calls that share rows_fin_same with the new kernel, as scripts/measure_shortcut.py times them
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    margin = float(np.quantile(s.clearance(paths.reshape(-1, nq))["min"], 0.1))
    souts = (f64(B, T, nq), torch.empty((B, T), dtype=torch.int32, device=dev), torch.empty((B, 6), dtype=torch.int32, device=dev), f64(B, 2))
    skw = dict(rounds=64, seed=4242, margin=margin, tol=1e-3, max_evals=256)
    shortcut = MC.timed(lambda: s.shortcut_paths(paths_t, out=souts, **skw), lambda: None, reps=REPS)
    length = MC.timed(lambda: s.path_length(paths_t, out=souts[3]), lambda: None, reps=REPS)
    res = MC.code_object_resources(r"k_retime_paths|k_shortcut_paths|k_path_length|k_difference")
    out = dict(B=B, T=T, S=S, dt=dt, longest_s=longest, n_samples_mean=float(ref["n_samples"].mean()), fused=fused, snap=snap, timing_only=timing,
               no_velocities=no_vel, host_driven=host, host_max_abs_diff=host_err, out_bytes=out_bytes, hbm_ms=hbm_ms, shortcut_paths=shortcut,
               path_length=length, parent=PARENT, resources=res)
    print(json.dumps(out))
    s.close()
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    row = lambda what, r: "| %s | %.3f | %.3f .. %.3f |" % (what, r["median_ms"], r["min_ms"], r["max_ms"])
    md = ["# Retiming: one fused call against the host-driven recipe", "",
          "One MI355X, talos32 (nq = nv = 32), fp64.  Recorded, not gated.  `python scripts/measure_retime.py` took the figures and wrote this file:",
          "every call is warmed up three times and timed %d times.  %d paths of %d waypoints: random starts, each next waypoint the last plus" % (REPS, B, T),
          "%.2f * uniform(-1, 1) per DoF; v_max_j = %.2f (2 + 0.25 (j mod 5)), a_max_j = %.2f (4 + 1.5 (j mod 3)); dt = %.6f s, which makes the" % (SIZE, SIZE, SIZE, dt),
          "longest path (%.3f s) %d samples; the mean path has %.1f.  S = %d rows per path." % (longest, S, out["n_samples_mean"], S), "",
          "## Call times (host clock around calls that end in a device synchronise; device inputs and outputs; profiler off)", "",
          "| what | median (ms) | min .. max (ms) |", "|---|---|---|",
          row("`retime_paths`, positions, velocities and records in one launch", fused),
          row("the same with `snap=True`", snap),
          row("positions only (`out_vel` NULL)", no_vel),
          row("timing only (`out_traj` NULL): phases 1 and 2", timing),
          row("the same work from the host: `difference` on the device, timing, profile and sums in numpy, upload of the result", host),
          row("`shortcut_paths`, 64 rounds (parent commit: %.3f)" % PARENT["shortcut_paths"], shortcut),
          row("`path_length` of the %d paths (parent commit: %.3f)" % (B, PARENT["path_length"]), length), "",
          "The host-driven recipe and the fused call agree within %.1e (largest absolute difference over positions, velocities and durations)." % host_err,
          "Ratio of the medians, host-driven over fused: %.1f." % (host["median_ms"] / fused["median_ms"]), "",
          "## Against the memory system", "",
          "The call writes %d bytes (%.1f MB).  At the 6.3 TB/s a streaming kernel reaches of HBM3E's 8 TB/s that is %.4f ms; the fused call takes %.1f times as long." % (out_bytes, out_bytes / 1e6, hbm_ms, fused["median_ms"] / hbm_ms),
          "A lane owns a sample and writes its row coordinate by coordinate, so one store instruction of a wavefront touches 64 rows that are",
          "nq doubles apart; the rows of a wavefront are contiguous, so every cache line it touches is filled by the lanes' later stores and L2 merges",
          "them, but each store instruction occupies 64 lines.  The difference between the first and the fourth row of the table is what the samples",
          "cost; between the first and the third, what the velocity rows cost.  A lane-per-coordinate store (the rows staged in LDS, then written",
          "with consecutive lanes on consecutive doubles) was not tried.  The velocity rows are as many bytes as the position rows and cost",
          "%.1f times as much (%.3f ms against %.3f ms beyond the timing-only call); the cause was not looked for." % ((fused["median_ms"] - no_vel["median_ms"]) / (no_vel["median_ms"] - timing["median_ms"]), fused["median_ms"] - no_vel["median_ms"], no_vel["median_ms"] - timing["median_ms"]), "",
          "## Registers, LDS and scratch (the notes of the gfx950 code object in libloik_amd.so)", "",
          "| kernel symbol | VGPRs | SGPRs | static LDS (bytes) | scratch (bytes/lane) |", "|---|---|---|---|---|"]
    md += ["| `%s` | %d | %d | %d | %d |" % (k, v["vgpr"], v["sgpr"], v["lds"], v["scratch"]) for k, v in sorted(res.items())]
    md += ["", "`k_retime_paths<false>` takes its tables from dynamic LDS, (T - 1) (5 + nv) doubles; `<true>` from a slab of global memory per resident",
           "wavefront, at most 512 of them.  `difference_joint` brings the same 80 bytes of scratch per lane that it brought to `k_shortcut_paths` and",
           "`k_difference` (the dynamically indexed rotation of `pose_log3`); it is touched once per segment, never per sample.  The register count",
           "leaves room for two wavefronts per SIMD."]
    if arg("--bytes"):
        md += ["", "## k_path_length and k_shortcut_paths after the fin / same test moved into rows_fin_same", "",
               "`shortcut_paths` and `path_length` on panda7, talos32, multidof13 and tree330 (the slab instantiation), with and without counts, and a path",
               "with repeated and NaN waypoints, from the parent commit's library and from this one, on one MI355X, every output array dumped raw:",
               open(arg("--bytes")).read().strip() + ".  The instruction streams of the three kernels differ from the parent's only in the layout of the",
               "scalar branches around that loop; every vector instruction is the same."]
    if arg("--accuracy"):
        lines = [l.lstrip(".").strip() for l in open(arg("--accuracy"), errors="replace") if l.lstrip(".").startswith("retime_measured")]   # (pytest -s puts its dots in front)
        md += ["", "## What the tests print (tests/test_retime.py, one MI355X)", "", "```"] + lines + ["```"]
    path = arg("--out", os.path.join(ROOT, "profiles", "retime_measured.md"))
    open(path, "w").write("\n".join(md) + "\n")


if __name__ == "__main__":
    main()
