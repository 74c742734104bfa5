"""The two-run agreement of the lock-step oracles behind profiles/pose_multidof_parity.md: every parity case of
tests/test_pose_path_multidof.py and tests/test_pose_track_multidof.py on the CPU oracle, as given and with q0 scaled by 1 + 1e-13.
A case tests the device and not itself when the two runs agree on every instance.  python scripts/pose_multidof_seed_agreement.py [path|track]"""
import os
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from multiprocessing import Pool
import test_pose_path_multidof as TP, test_pose_track_multidof as TT

def agree(kind, case):
    mod = TP if kind == "path" else TT
    t = time.time()
    w = mod._inputs(case)
    idx = np.arange(mod.B)
    a = mod._oracle(w, idx)
    b = mod._oracle(w, idx, q0=w["q0"] * (1 + 1e-13))
    if kind == "path":
        same = (a["reached"] == b["reached"]) & (a["steps"] == b["steps"]) & (a["cursor"] == b["cursor"]) & (a["wsteps"] == b["wsteps"]).all(axis=1)
        dq = np.abs(a["q"] - b["q"]).max(axis=1)
        info = "cursor %s pstat %s steps %s status %s" % (np.bincount(a["cursor"], minlength=w["T"] + 1).tolist(), np.bincount(a["path_status"], minlength=3).tolist(),
                                                np.bincount(a["steps"]).tolist(), np.bincount(a["status"], minlength=8).tolist())
    else:
        same = (a["steps"] == b["steps"]) & (a["inner"] == b["inner"]).all(axis=1) & (a["status"] == b["status"])
        dq = np.nan_to_num(np.abs(a["q_traj"] - b["q_traj"])).max(axis=(1, 2))
        info = "status %s inner-any %s errmax med %s" % (np.bincount(a["status"], minlength=8).tolist(), np.bincount(a["inner"].max(axis=1), minlength=8).tolist(),
                                            ["%.1e" % x for x in np.nanmedian(a["errmax"], axis=0)])
    if "limit_flags" in a:
        info += " flagged %.2f" % (a["limit_flags"] != 0).any(axis=1).mean()
    ok = same & (dq < 1e-8)
    return kind, case, ok.mean(), dq.max(), info, time.time() - t

if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    jobs = []
    if which in ("path", "both"): jobs += [("path", c) for c in TP.PARITY]
    if which in ("track", "both"): jobs += [("track", c) for c in TT.PARITY]
    with Pool(8) as p:
        for r in p.starmap(agree, jobs):
            print("%s %s | agree %.4f | max dq %.2e | %s | %.1fs" % (r[0], (TP if r[0] == "path" else TT)._case_id(r[1]) + "-seed%d" % r[1][-1], r[2], r[3], r[4], r[5]), flush=True)
