"""Talos-32, 65 536 configurations, 2 spheres per link, self pairs on, a world of 0, 16 and 64 objects: the call time of the clearance
query beside forward kinematics of all links on the same batch (the placements alone) and a device copy of the query's output bytes, the
select time of a collision-aware multi-start beside the unlatched one on the same handle, and the registers, LDS and scratch of every
instantiation of k_clearance read from the library's gfx950 code object.  Host clock around calls that end in a device synchronise;
--short: 5 timed calls per figure.  Prints one JSON line and writes profiles/clearance_measured.md (or --out PATH); --accuracy FILE adds
the error maxima from the lines tests/test_clearance.py prints.  One process; run it under a timeout."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loik_amd
from loik_amd import capi
from test_pose_ik import _handle, _links
import clearance_numpy as CN
import pose_numpy as P

SHORT = "--short" in sys.argv
REPS = 5 if SHORT else 30
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def _arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def timed(fn, sync, reps=REPS, warm=3):
    for _ in range(warm):
        fn(); sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); sync(); t.append((time.perf_counter() - t0) * 1e3)
    t = np.array(t)
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), reps=reps)


def code_object_resources(pattern):
    """{kernel symbol: dict(vgpr, sgpr, lds, scratch)} of the kernels whose symbol matches `pattern`, from the notes of every gfx950 code
    object bundled in the library"""
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, capi._LIB_PATH, os.path.join(tmp, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)] + [len(blob)]
        for k in range(len(starts) - 1):
            part, co = os.path.join(tmp, "bundle%d" % k), os.path.join(tmp, "co%d" % k)
            open(part, "wb").write(blob[starts[k]:starts[k + 1]])
            subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   "--input=" + part, "--output=" + co])
            notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
            for rec in notes.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", rec)
                if not name or not re.search(pattern, name.group(1)):
                    continue
                f = {key: int(re.search(r"\.%s:\s+(\d+)" % key, rec).group(1)) for key in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")}
                # the mangled symbol by hand: _ZN5loikb<len><name>[ILb<0|1>E]E...
                m = re.match(r"_ZN5loikb\d+([a-z_0-9]+?)(?:ILb([01])E)?E", name.group(1))
                plain = name.group(1) if not m else m.group(1) + ("" if m.group(2) is None else "<%s>" % ("true" if m.group(2) == "1" else "false"))
                out[plain] = dict(vgpr=f["vgpr_count"], sgpr=f["sgpr_count"], lds=f["group_segment_fixed_size"], scratch=f["private_segment_fixed_size"])
    return out


def _world(rng, nw):
    nws, nwb = nw // 2, nw - nw // 2
    ws = np.concatenate([rng.uniform(-1.0, 1.0, size=(nws, 3)), rng.uniform(0.05, 0.3, size=(nws, 1))], axis=1)
    wb = np.array([np.concatenate([np.eye(3).reshape(9), rng.uniform(-1.0, 1.0, size=3), rng.uniform(0.05, 0.4, size=3)]) for _ in range(nwb)]).reshape(nwb, 15)
    return ws, wb


def main():
    model = loik_amd.builtin_model("talos32")
    B = 65536
    links = _links(model, 1)
    rng = np.random.default_rng(1)
    q = model.random_configurations(rng, B)
    s, _ = _handle(model, B, links, q)
    hip = capi.DeviceArray.hip()
    sync = s.synchronize
    lk, sph = CN.make_spheres(model, 2, 410)
    s.set_collision_spheres(lk, sph)
    s.set_self_collision(True)
    res = dict(robot="talos32", B=B, nv=model.nv, spheres=int(lk.size), self_pairs=s.num_self_pairs())
    out_bytes = B * (3 * 8 + 3 * 4)
    res["output_bytes"] = out_bytes
    dm, dw = capi.DeviceArray(np.zeros(3 * B)), capi.DeviceArray(np.zeros((3 * B + 1) // 2))
    src, dst = capi.DeviceArray(np.zeros(out_bytes // 8)), capi.DeviceArray(np.zeros(out_bytes // 8))
    res["device_copy_output_bytes"] = timed(lambda: hip.hipMemcpy(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), out_bytes, 3), sync)
    all_links = np.arange(1, model.njoints, dtype=np.int32)
    dfk = capi.DeviceArray(np.zeros(B * all_links.size * 12))
    lp = all_links.ctypes.data_as(C.POINTER(C.c_int))
    res["forward_kinematics_all_links"] = timed(lambda: s.L.loikb_forward_kinematics(s.h, lp, int(all_links.size), C.c_void_p(dfk.data_ptr()), capi.OUT_DEVICE), sync)
    res["forward_kinematics_bytes"] = int(B * all_links.size * 12 * 8)
    res["clearance"] = {}
    for nw in (0, 16, 64):
        s.set_collision_world(*_world(rng, nw))
        res["clearance"][str(nw)] = timed(lambda: s.clearance(out=(dm, dw)), sync)
    # the collision-aware multi-start beside the unlatched one: G = 1024 goals of K = 64 seeds, three steps, the world of 64 objects
    G, K = 1024, 64
    lo, hi = np.array(model.q_lo, dtype=float), np.array(model.q_hi, dtype=float)
    s.set_joint_limits(lo, hi)
    q0g = rng.uniform(lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo), size=(G, model.nq))
    tg = P.fk12(model, rng.uniform(lo, hi, size=(G, model.nq)), links)
    # the margin: the median clearance of the batch's random configurations, so that about half of the seeds that reach are clear (with
    # random spheres of up to 0.08 within 0.1 of every link origin the model collides with itself at any q: the margin is negative)
    margin = float(np.median(s.clearance()["min"]))
    res["multistart_margin"] = margin
    sel = {"unlatched": [], "latched": []}
    for rep in range(2 if SHORT else 6):
        for mode in ("unlatched", "latched"):
            out = s.SolvePoseMultiStart(tg, K, seed=7, q0=q0g, pick="first", tol_pose=1e-3, max_steps=3, clearance_margin=margin if mode == "latched" else None)
            if rep:
                sel[mode].append(out["timing"]["select_ms"])
            res["multistart_%s_total_ms" % mode] = out["timing"]["total_ms"]
            res["multistart_%s_nreached_mean" % mode] = float(out["nreached"].mean())
            if mode == "latched":
                res["multistart_latched_nclear_mean"] = float(out["nclear"].mean())
                res["multistart_latched_goals_in_collision"] = int((out["goal_status"] == capi.MS_GOAL_IN_COLLISION).sum())
    res["multistart_select_ms"] = {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v)) for k, v in sel.items()}
    s.close()
    res["resources"] = code_object_resources(r"k_clearance|k_ms_select|k_ms_loop_status")
    acc = _arg("--accuracy")
    if acc and os.path.exists(acc):
        res["accuracy"] = dict(re.findall(r"clearance_measured (\S+) worst relative (\S+)", open(acc).read()))
    print("CLEARANCE_MEASURED " + json.dumps(res))
    write_report(res, _arg("--out", os.path.join(ROOT, "profiles", "clearance_measured.md")))


def write_report(r, path):
    def row(name, t):
        return "| %s | %.3f | %.3f .. %.3f |" % (name, t["median_ms"], t["min_ms"], t["max_ms"])
    fk, cp = r["forward_kinematics_all_links"], r["device_copy_output_bytes"]
    L = ["# Collision clearance: what the query and the collision-aware selection cost", "",
         "One MI355X, talos32 (nv = %d), B = %d resident configurations, %d spheres (2 per link), self pairs on (%d pairs), fp64.  Recorded, not"
         % (r["nv"], r["B"], r["spheres"], r["self_pairs"]),
         "gated.  `python scripts/measure_clearance.py` took the figures and wrote this file: every call is warmed up three times and timed %d times."
         % r["clearance"]["0"]["reps"], "",
         "## Call times (host clock around a call that ends in a device synchronise; profiler off)", "",
         "| what | median (ms) | min .. max (ms) |", "|---|---|---|"]
    for nw in ("0", "16", "64"):
        L.append(row("`clearance(out=device)`, %s world objects (half spheres, half boxes) -- %d bytes of output" % (nw, r["output_bytes"]), r["clearance"][nw]))
    L += [row("`loikb_forward_kinematics` of all %d links, `LOIKB_OUT_DEVICE` -- %d bytes of output" % (r["nv"], r["forward_kinematics_bytes"]), fk),
          row("`hipMemcpy` device to device of the query's %d output bytes + synchronise" % r["output_bytes"], cp), "",
          "As measured: the query with 0 / 16 / 64 world objects takes %.2f / %.2f / %.2f times the forward kinematics of all links alone, and %.1f / %.1f / %.1f"
          % tuple([r["clearance"][k]["median_ms"] / fk["median_ms"] for k in ("0", "16", "64")] + [r["clearance"][k]["median_ms"] / cp["median_ms"] for k in ("0", "16", "64")]),
          "times a device copy of its output bytes.", "",
          "## The collision-aware selection in a multi-start", "",
          "G = 1 024 goals of K = 64 seeds (B = 65 536), joint limits as ranges, one round, 3 steps, tol_pose 1e-3, pick first, the world of 64",
          "objects, margin %.4f (the median clearance of the batch's random configurations).  `select_ms` of" % r["multistart_margin"],
          "`LOIKB_MS_F_TIMING`, the two modes in alternation on one handle, the first call of each dropped:", "",
          "| mode | select_ms median | min .. max | calls | total_ms of the last call |", "|---|---|---|---|---|"]
    for mode in ("unlatched", "latched"):
        m = r["multistart_select_ms"][mode]
        L.append("| %s | %.3f | %.3f .. %.3f | %d | %.1f |" % (mode, m["median"], m["min"], m["max"], m["n"], r["multistart_%s_total_ms" % mode]))
    L += ["", "The latched selection includes its clearance launch over all B rows.  Of the 64 seeds of a goal %.1f reached on average and %.1f were"
          % (r["multistart_latched_nreached_mean"], r["multistart_latched_nclear_mean"]),
          "clear; %d of the 1 024 goals had only colliding answers." % r["multistart_latched_goals_in_collision"], "",
          "## Registers, LDS and scratch (the notes of the gfx950 code object in libloik_amd.so)", "",
          "| kernel symbol | VGPRs | SGPRs | static LDS (bytes) | scratch (bytes/lane) |", "|---|---|---|---|---|"]
    for name in sorted(r["resources"]):
        x = r["resources"][name]
        L.append("| `%s` | %d | %d | %d | %d |" % (name, x["vgpr"], x["sgpr"], x["lds"], x["scratch"]))
    L += ["", "`k_clearance` takes its LDS dynamically: per wavefront 4 ns doubles for the centres and, in the `false` (LDS) instantiation, 12 nb + 12 ncar",
          "doubles for the joint transforms and the carriers' placements (talos32 with 64 spheres: 8 192 bytes a wavefront, four wavefronts a workgroup)."]
    if r.get("accuracy"):
        L += ["", "## Error maxima the tests print (tests/test_clearance.py, one MI355X)", "",
              "`max |min - oracle| / (1 + max |centre| + max r)` over min, min_world and min_self, a world of 33 spheres and 32 boxes, self pairs on",
              "(bound 1e-13): " + ", ".join("%s %.1e" % (k, float(v)) for k, v in r["accuracy"].items()) + "."]
    open(path, "w").write("\n".join(L) + "\n")


if __name__ == "__main__":
    main()
