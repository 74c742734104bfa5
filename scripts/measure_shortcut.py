"""Talos-32 with the spheres, world and self pairs of tests/test_clearance._case, 4096 paths of 32 waypoints (random starts, each next
waypoint the last plus 0.08 * uniform(-1, 1) per DoF), 64 shortcut rounds: the time of one shortcut_paths call with device pointers
beside the same 64 rounds driven from the host through the older entry points (difference and motion_clearance per round with device
pointers, the draws in numpy, the splice in torch), the outcome totals, the samples per tried segment, and the registers, LDS and scratch
of the kernels read from the library's gfx950 code object.  Host clock around calls that end in a device synchronise; --short: 3 timed
calls per figure.  Prints one JSON line and writes profiles/shortcut_measured.md (or --out PATH); --accuracy FILE adds the error maxima
from the lines tests/test_shortcut.py prints, --bytes FILE the outcome of the byte comparison of k_motion_clearance's outputs.  One
process; run it under a timeout."""
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
import pose_multistart_numpy as MS
import test_clearance as TC

SHORT = "--short" in sys.argv
REPS = 3 if SHORT else 10
B, T, ROUNDS, SEED, SIZE, TOL, MAX_EVALS = 4096, 32, 64, 4242, 0.08, 1e-3, 256


def host_loop(s, torch, paths_t, margin):
    """the rule of loik_amd_shortcut.h with the whole batch in lock step: returns (keep [B][T], L [B], totals, evals of the tried segments)"""
    dev = paths_t.device
    nq, nv = s.model.nq, s.model.nv
    keep = torch.arange(T, device=dev).repeat(B, 1)
    L = np.full(B, T, dtype=np.int64)
    rows, pos = torch.arange(B, device=dev), torch.arange(T, device=dev)[None]
    dv, val, info = torch.empty((B, nv), dtype=torch.float64, device=dev), torch.empty((B, 3), dtype=torch.float64, device=dev), torch.empty((B, 5), dtype=torch.int32, device=dev)
    totals, evals = np.zeros(4, dtype=np.int64), []
    ids = np.arange(B, dtype=np.uint64)
    for r in range(ROUNDS):
        act = L >= 3
        if not act.any():
            break
        span = np.where(act, L - 2, 1).astype(np.uint64)
        i = (MS.words(SEED, r, ids, 0) % span).astype(np.int64)
        j = i + 2 + (MS.words(SEED, r, ids, 1) % np.where(act, L - 2 - i, 1).astype(np.uint64)).astype(np.int64)
        i, j = np.where(act, i, 0), np.where(act, j, 1)
        it, jt = torch.from_numpy(i).to(dev), torch.from_numpy(j).to(dev)
        qa = paths_t[rows, keep[rows, it]].contiguous()
        qb = paths_t[rows, keep[rows, jt]].contiguous()
        torch.cuda.synchronize()
        s.difference(qa, qb, out=dv)
        s.motion_clearance(qa, dv=dv, margin=margin, tol=TOL, max_evals=MAX_EVALS, out=(val, info))
        st = info[:, 0].cpu().numpy()      # (the sync of the round: the draws of the next one need L)
        evals.append(info[:, 1].cpu().numpy()[act])
        totals += np.bincount(st[act], minlength=4)[:4]
        free = act & (st == capi.MOTION_FREE)
        cut = torch.from_numpy(np.where(free, j - i - 1, 0)).to(dev)[:, None]
        keep = torch.where(pos <= it[:, None], keep, torch.gather(keep, 1, torch.clamp(pos + cut, max=T - 1)))
        L = L - np.where(free, j - i - 1, 0)
    torch.cuda.synchronize()
    return keep.cpu().numpy(), L, totals, np.concatenate(evals) if evals else np.zeros(0, dtype=np.int32)


def main():
    import torch
    c = TC._case("talos32")
    model = c["model"]
    assert model.nq == model.nv      # (plain sums: the recipe's (+) is an addition)
    rng = np.random.default_rng(900)
    rows = [model.random_configurations(rng, B)]
    for _ in range(T - 1):
        rows.append(rows[-1] + SIZE * rng.uniform(-1.0, 1.0, size=(B, model.nv)))
    paths = np.ascontiguousarray(np.stack(rows, axis=1))
    s = TC._open(model, c["q"])
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    margin = float(np.quantile(s.clearance(paths.reshape(-1, model.nq))["min"], 0.1))
    kw = dict(rounds=ROUNDS, seed=SEED, margin=margin, tol=TOL, max_evals=MAX_EVALS)
    ref = s.shortcut_paths(paths, **kw)
    dev = torch.device("cuda:0")
    paths_t = torch.from_numpy(paths).to(dev)
    outs = (torch.empty((B, T, model.nq), dtype=torch.float64, device=dev), torch.empty((B, T), dtype=torch.int32, device=dev),
            torch.empty((B, 6), dtype=torch.int32, device=dev), torch.empty((B, 2), dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    fused = MC.timed(lambda: s.shortcut_paths(paths_t, out=outs, **kw), lambda: None, reps=REPS)
    assert np.array_equal(outs[1].cpu().numpy(), ref["keep"]) and np.array_equal(outs[2].cpu().numpy()[:, 0], ref["n_waypoints"])
    length = MC.timed(lambda: s.path_length(paths_t, out=outs[3]), lambda: None, reps=REPS)
    keep_h, L_h, totals, evals = host_loop(s, torch, paths_t, margin)
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter(); host_loop(s, torch, paths_t, margin); t.append((time.perf_counter() - t0) * 1e3)
    host = dict(median_ms=float(np.median(t)), min_ms=float(min(t)), max_ms=float(max(t)), reps=REPS)
    agree = int(np.sum((L_h == ref["n_waypoints"]) & np.all(np.where(np.arange(T)[None] < L_h[:, None], keep_h, -1) == ref["keep"], axis=1)))
    res = MC.code_object_resources(r"k_shortcut_paths|k_path_length|k_motion_clearance")
    tot = {k: int(ref[k].sum()) for k in ("tried", "accepted", "blocked", "undecided", "invalid")}
    out = dict(B=B, T=T, rounds=ROUNDS, margin=margin, fused=fused, host_loop=host, path_length=length, totals=tot, host_totals=totals.tolist(),
               paths_agreeing=agree, evals_median=float(np.median(evals)), evals_max=int(evals.max()), evals_mean=float(evals.mean()),
               waypoints_left_mean=float(ref["n_waypoints"].mean()), length_in_mean=float(ref["length_in"].mean()),
               length_out_mean=float(ref["length_out"].mean()), resources=res)
    print(json.dumps(out))
    s.close()
    arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    md = ["# Certified shortcutting: one fused call against the host-driven loop", "",
          "One MI355X, talos32 (nv = 32) with the spheres (%d), self pairs (%d) and world (33 spheres, 32 boxes) of tests/test_clearance._case, fp64.  Recorded, not"
          % (len(c["links"]), len(c["pairs"])),
          "gated.  `python scripts/measure_shortcut.py` took the figures and wrote this file: every call is warmed up three times and timed %d times." % REPS,
          "%d paths of %d waypoints: random starts, each next waypoint the last plus %.2f * uniform(-1, 1) per DoF; %d rounds, seed %d, margin %.4f (the" % (B, T, SIZE, ROUNDS, SEED, margin),
          "10 %% quantile of the clearance over all waypoints), tol %.0e, max_evals %d." % (TOL, MAX_EVALS), "",
          "## Outcomes", "",
          "tried %(tried)d, accepted %(accepted)d, blocked %(blocked)d, undecided %(undecided)d, invalid %(invalid)d." % tot
          + "  Waypoints left per path: mean %.2f of %d; length mean %.3f -> %.3f." % (out["waypoints_left_mean"], T, out["length_in_mean"], out["length_out_mean"]),
          "Samples per tried segment (from the host-driven loop's motion_clearance rows): median %d, mean %.2f, largest %d." % (out["evals_median"], out["evals_mean"], out["evals_max"]),
          "The host-driven loop ends with the same keep list as the fused call on %d of %d paths (outcome totals free / blocked / undecided / invalid %s)." % (agree, B, totals.tolist()), "",
          "## Call times (host clock around calls that end in a device synchronise; device inputs and outputs; profiler off)", "",
          "| what | median (ms) | min .. max (ms) |", "|---|---|---|",
          "| `shortcut_paths`, %d rounds in one launch | %.3f | %.3f .. %.3f |" % (ROUNDS, fused["median_ms"], fused["min_ms"], fused["max_ms"]),
          "| the same rounds from the host: `difference` + `motion_clearance` per round, draws in numpy, splice in torch | %.3f | %.3f .. %.3f |" % (host["median_ms"], host["min_ms"], host["max_ms"]),
          "| `path_length` of the %d paths | %.3f | %.3f .. %.3f |" % (B, length["median_ms"], length["min_ms"], length["max_ms"]), "",
          "The host-driven loop pays two launches, the gathers and a synchronise per round, and every round waits for its longest segment; the fused",
          "call keeps a wavefront on a path until the path is done.  Ratio of the medians: %.2f." % (host["median_ms"] / fused["median_ms"]), "",
          "## Registers, LDS and scratch (the notes of the gfx950 code object in libloik_amd.so)", "",
          "| kernel symbol | VGPRs | SGPRs | static LDS (bytes) | scratch (bytes/lane) |", "|---|---|---|---|---|"]
    md += ["| `%s` | %d | %d | %d | %d |" % (k, v["vgpr"], v["sgpr"], v["lds"], v["scratch"]) for k, v in sorted(res.items())]
    md += ["", "`k_shortcut_paths` takes its LDS dynamically as `k_motion_clearance` does, plus the dv row: 4 ns doubles for the centres and, in the `false`",
           "(LDS) instantiation, ns + 12 nb + 12 ncar + nb doubles beside them; the `true` instantiation keeps those in a slab of global memory per",
           "resident wavefront.  The 80 bytes of scratch per lane are `difference_joint`'s dynamically indexed rotation (`pose_log3`), the same 80 bytes",
           "`k_difference` has: the aim of no scratch is missed by that much, on a path taken once per round and once per segment of a length.",
           "254 VGPRs leave room for two wavefronts per SIMD, 2048 on the chip: the 4096 paths of this measurement go through in two shifts, and",
           "within a shift a path's rounds and samples follow one another, so the call time is the longest chains' time, not the sample count's.  A budget of",
           "three wavefronts per SIMD (`__launch_bounds__(64, 3)`) crashes the ROCm 7.2 compiler on this kernel and was not pursued."]
    if arg("--bytes"):
        md += ["", "## k_motion_clearance after the advancement moved into motion_advance", "",
               "`motion_clearance` and `path_clearance` on the eight cases of tests/test_motion_clearance.motion_case, from the parent commit's library and",
               "from this one, on one MI355X, every output array dumped raw: " + open(arg("--bytes")).read().strip() + "."]
    if arg("--accuracy"):
        lines = [l.lstrip(".").strip() for l in open(arg("--accuracy"), errors="replace") if l.lstrip(".").startswith("shortcut_measured")]   # (pytest -s puts its dots in front)
        md += ["", "## What the tests print (tests/test_shortcut.py, one MI355X)", "", "```"] + lines + ["```"]
    path = arg("--out", os.path.join(ROOT, "profiles", "shortcut_measured.md"))
    open(path, "w").write("\n".join(md) + "\n")


if __name__ == "__main__":
    main()
