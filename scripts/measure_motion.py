"""Talos-32, 65 536 segments, 2 spheres per link, self pairs on, the world of tests/test_clearance.py (33 spheres, 32 boxes): the call time
of the certified motion check, the samples it takes, the time of the clearance query on as many configurations times the median number
of samples (the yardstick of the cost of one sample), the time of difference, and the registers, LDS and scratch of the new kernels read
from the library's gfx950 code object.  Host clock around calls that end in a device synchronise; --short: 5 timed calls per figure.
Prints one JSON line and writes profiles/motion_measured.md (or --out PATH); --accuracy FILE adds the error maxima from the lines
tests/test_motion_clearance.py prints.  One process; run it under a timeout."""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loik_amd
from loik_amd import capi
from measure_clearance import _arg, code_object_resources, timed
from test_pose_ik import _handle, _links
import clearance_numpy as CN
import test_clearance as TC

TOL, MAX_EVALS, SIZE = 1e-3, 256, 0.08


def main():
    model = loik_amd.builtin_model("talos32")
    n = 65536
    rng = np.random.default_rng(2)
    qa = model.random_configurations(rng, n)
    dv = SIZE * rng.uniform(-1.0, 1.0, size=(n, model.nv))
    s, _ = _handle(model, n, _links(model, 1), qa)
    sync = s.synchronize
    lk, sph = CN.make_spheres(model, 2, 410)
    c = TC._case("talos32")
    s.set_collision_spheres(lk, sph)
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    start = s.clearance()["min"]
    margin = float(np.quantile(start, 0.4))   # (the dense world leaves few random configurations clear of everything: see the tests)
    res = dict(robot="talos32", n=n, nv=model.nv, spheres=int(lk.size), self_pairs=s.num_self_pairs(), world="33 spheres, 32 boxes", margin=margin,
               tol=TOL, max_evals=MAX_EVALS, dv_size=SIZE)
    got = s.motion_clearance(qa, dv=dv, margin=margin, tol=TOL, max_evals=MAX_EVALS)
    res["outcomes"] = [int((got["status"] == k).sum()) for k in range(4)]
    res["evals"] = dict(median=float(np.median(got["evals"])), mean=float(got["evals"].mean()), largest=int(got["evals"].max()), total=int(got["evals"].sum()))
    dqa, ddv = capi.DeviceArray(qa), capi.DeviceArray(dv)
    val, info = capi.DeviceArray(np.zeros(3 * n)), capi.DeviceArray(np.zeros((5 * n + 1) // 2))
    res["motion_clearance"] = timed(lambda: s.motion_clearance(dqa, dv=ddv, margin=margin, tol=TOL, max_evals=MAX_EVALS, out=(val, info)), sync)
    res["motion_clearance_one_sample"] = timed(lambda: s.motion_clearance(dqa, dv=ddv, margin=margin, tol=TOL, max_evals=1, out=(val, info)), sync)
    dm, dw = capi.DeviceArray(np.zeros(3 * n)), capi.DeviceArray(np.zeros((3 * n + 1) // 2))
    res["clearance"] = timed(lambda: s.clearance(dqa, out=(dm, dw)), sync)
    dq1, dvo = capi.DeviceArray(model.random_configurations(rng, n)), capi.DeviceArray(np.zeros((n, model.nv)))
    res["difference"] = timed(lambda: s.difference(dqa, dq1, out=dvo), sync)
    s.close()
    res["resources"] = code_object_resources(r"k_motion_clearance|k_difference|k_clearance")
    acc = _arg("--accuracy")
    if acc and os.path.exists(acc):
        text = open(acc).read()
        res["accuracy_s"] = dict(re.findall(r"^\.*motion_measured (.+?): max \|s - oracle\| (\d\S*),", text, flags=re.M))
        res["accuracy_min"] = dict(re.findall(r"^\.*motion_measured (.+?): max \|s .*?relative (\d\S*)", text, flags=re.M))
    print("MOTION_MEASURED " + json.dumps(res))
    write_report(res, _arg("--out", os.path.join(ROOT, "profiles", "motion_measured.md")))


def write_report(r, path):
    def row(name, t):
        return "| %s | %.3f | %.3f .. %.3f |" % (name, t["median_ms"], t["min_ms"], t["max_ms"])
    mc, cl, ev = r["motion_clearance"], r["clearance"], r["evals"]
    L = ["# Certified motion checks: what a segment costs", "",
         "One MI355X, talos32 (nv = %d), %d segments, %d spheres (2 per link), self pairs on (%d pairs), a world of %s, fp64.  Recorded, not"
         % (r["nv"], r["n"], r["spheres"], r["self_pairs"], r["world"]),
         "gated.  `python scripts/measure_motion.py` took the figures and wrote this file: every call is warmed up three times and timed %d times." % mc["reps"],
         "Starts are random configurations, dv = %.2f * uniform(-1, 1) per DoF, margin %.4f (the 40 %% quantile of the clearance at the starts),"
         % (r["dv_size"], r["margin"]),
         "tol %.0e, max_evals %d." % (r["tol"], r["max_evals"]), "",
         "## Outcomes and samples", "",
         "FREE %d, BLOCKED %d, UNDECIDED %d, INVALID %d.  Samples per segment: median %.0f, mean %.2f, largest %d; %d in all." %
         (r["outcomes"][0], r["outcomes"][1], r["outcomes"][2], r["outcomes"][3], ev["median"], ev["mean"], ev["largest"], ev["total"]), "",
         "## Call times (host clock around a call that ends in a device synchronise; device inputs and outputs; profiler off)", "",
         "| what | median (ms) | min .. max (ms) |", "|---|---|---|",
         row("`motion_clearance`, max_evals %d" % r["max_evals"], mc),
         row("`motion_clearance`, max_evals 1 (the bound, one sample, the store)", r["motion_clearance_one_sample"]),
         row("`clearance` of the %d start configurations (the parent commit's query)" % r["n"], cl),
         row("`difference` of %d pairs of configurations" % r["n"], r["difference"]), "",
         "The yardstick of the cost of a sample: the clearance query on %d configurations times the median number of samples is %.3f ms, times the"
         % (r["n"], cl["median_ms"] * ev["median"]),
         "mean number %.3f ms; the check took %.3f ms.  A wavefront runs as long as its segment takes samples, so the call ends with the" %
         (cl["median_ms"] * ev["mean"], mc["median_ms"]),
         "longest segments of the batch (largest %d samples against a mean of %.2f)." % (ev["largest"], ev["mean"]), "",
         "## Registers, LDS and scratch (the notes of the gfx950 code object in libloik_amd.so)", "",
         "| kernel symbol | VGPRs | SGPRs | static LDS (bytes) | scratch (bytes/lane) |", "|---|---|---|---|---|"]
    for name in sorted(r["resources"]):
        x = r["resources"][name]
        L.append("| `%s` | %d | %d | %d | %d |" % (name, x["vgpr"], x["sgpr"], x["lds"], x["scratch"]))
    L += ["", "`k_motion_clearance` takes its LDS dynamically, one wavefront a workgroup: 4 ns doubles for the centres and, in the `false` (LDS)",
          "instantiation, ns + 12 nb + 12 ncar doubles for Lambda, the joint transforms and the carriers' placements (talos32 with 64 spheres: 8 704",
          "bytes); the `true` instantiation keeps those in a slab of global memory per resident wavefront."]
    if r.get("accuracy_s"):
        worst = max(float(v) for v in r["accuracy_s"].values())
        L += ["", "## Error maxima the tests print (tests/test_motion_clearance.py, one MI355X)", "",
              "`max |s_free - oracle|` and `max |s_at_min - oracle|` together, per case: " + ", ".join("%s %.1e" % (k, float(v)) for k, v in r["accuracy_s"].items()) + ".",
              "The largest is %.3e; tests/test_motion_clearance.py asserts 16 times that." % worst, "",
              "`max |min_sampled - oracle| / (1 + max |centre| + max r)` (bound 1e-13): " + ", ".join("%s %.1e" % (k, float(v)) for k, v in r["accuracy_min"].items()) + "."]
    open(path, "w").write("\n".join(L) + "\n")


if __name__ == "__main__":
    main()
