"""Talos-32, 65 536 instances, one frame: call times of the Jacobian / dexterity getters beside a device copy and an inner Solve,
and the select time of a dexterous multi-start beside pick="first" (profiles/jacobian_measured.md).  Host clock around calls that end
in a device synchronise; --short: 5 timed calls per figure, for a run under a kernel trace.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loik_amd
from loik_amd import capi
from test_pose_ik import PRM, _handle, _links
import pose_numpy as P

SHORT = "--short" in sys.argv
REPS = 5 if SHORT else 30


def timed(fn, sync, reps=REPS, warm=3):
    for _ in range(warm):
        fn(); sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); sync(); t.append((time.perf_counter() - t0) * 1e3)
    t = np.array(t)
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), reps=reps)


def main():
    model = loik_amd.builtin_model("talos32")
    B = 65536
    links = _links(model, 1)
    rng = np.random.default_rng(1)
    q = model.random_configurations(rng, B)
    s, _ = _handle(model, B, links, q)
    hip = capi.DeviceArray.hip()
    sync = s.synchronize
    res = dict(robot="talos32", B=B, nv=model.nv)
    nJ = B * 6 * model.nv
    dJ, dJ2 = capi.DeviceArray(np.zeros(nJ)), capi.DeviceArray(np.zeros(nJ))
    res["jacobian_bytes"] = nJ * 8
    for ref in ("local", "world"):
        res["frame_jacobians_%s" % ref] = timed(lambda: s.frame_jacobians(links, None, reference=ref, out=dJ), sync)
    res["device_copy_same_bytes"] = timed(lambda: hip.hipMemcpy(C.c_void_p(dJ2.data_ptr()), C.c_void_p(dJ.data_ptr()), nJ * 8, 3), sync)
    dD = capi.DeviceArray(np.zeros(B * 8))
    prm = capi.DexterityParams(1.0, 0)
    la = np.array(links, dtype=np.int32)
    lp = la.ctypes.data_as(C.POINTER(C.c_int))
    res["frame_dexterity"] = timed(lambda: s.L.loikb_frame_dexterity(s.h, lp, None, None, 1, C.byref(prm), C.c_void_p(dD.data_ptr()), capi.OUT_DEVICE), sync)
    res["inner_solve"] = timed(lambda: s.Solve(), sync, reps=max(3, REPS // 3))
    # a dexterous multi-start beside pick="first": G = 1024 goals of K = 64 seeds, three steps
    G, K = 1024, 64
    lo, hi = np.array(model.q_lo, dtype=float), np.array(model.q_hi, dtype=float)
    s.set_joint_limits(lo, hi)
    q0g = rng.uniform(lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo), size=(G, model.nq))
    tg = P.fk12(model, rng.uniform(lo, hi, size=(G, model.nq)), links)
    sel = {"first": [], "dexterous": []}
    for rep in range(2 if SHORT else 5):
        for pick in ("first", "dexterous"):
            out = s.SolvePoseMultiStart(tg, K, seed=7, q0=q0g, pick=pick, tol_pose=1e-3, max_steps=3)
            if rep:
                sel[pick].append(out["timing"]["select_ms"])
            res["multistart_%s_nreached_mean" % pick] = float(out["nreached"].mean())
            res["multistart_%s_total_ms" % pick] = out["timing"]["total_ms"]
    res["multistart_select_ms"] = {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in sel.items()}
    s.close()
    print("JACOBIAN_MEASURED " + json.dumps(res))


if __name__ == "__main__":
    main()
