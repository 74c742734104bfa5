"""Regenerates tests/golden/qp_optimum_measured.json: how far the C oracle (oracle/loik_ref.c; oracle/dense.py for the dense_* cases),
stopped at the tight settings of tests/qp_cases.py, lies from the certified optimum of tests/qp_numpy.py -- per (case, batch) the maximum
over the compared instances of |z - x*|_inf, |nu - x*|_inf, |vis - J x*|_inf and the stationarity residual.  CPU only; no kernel is run.

    python tests/golden/make_qp_optimum_measured.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import qp_cases as C  # noqa: E402


def main():
    keys = [(n, C.CPU_BATCH, "ref") for n in C.CASES] + [(n, 3, "dense") for n in C.DENSE_CASES] + [(n, 3, "ref") for n in C.DENSE_CASES]
    keys += [(n, B, "ref") for n, B in C.GPU_KEYS]
    out = {"_provenance": dict(settings={k: C.TIGHT[k] for k in ("tol_abs", "tol_rel", "tol_primal_inf", "tol_dual_inf", "max_iter", "rho", "mu",
                                                                     "mu_equality_scale_factor")},
                               solver="oracle/loik_ref.c (entries ending in :dense: oracle/dense.py), fp64, CPU",
                               reference="tests/qp_numpy.py: primal active set + KKT certificate",
                               cases="tests/qp_cases.py: every seed is in CASES / DENSE_CASES; instances: all of a batch up to 64, else qp_cases.sample(B)",
                               figures="max over the certified instances of the inf-norm distances z, nu, vis and of the stationarity residual")}
    for name, B, solver in keys:
        wl = C.problem(name, B)
        idx = C.sample(B)
        opt = C.reference(wl, idx)
        C.check_conditions(name, wl, opt)
        stalled = C.stalled_instances(wl) if (name, B) in C.GPU_KEYS else np.zeros(0, dtype=int)
        live = ~np.isin(idx, stalled)
        got = C.oracle_solve(wl, idx, solver)
        assert got["converged"][live].all() and not got["infeasible"].any(), (name, B, got["iter"])
        assert name not in C.DENSE_CASES and B != C.CPU_BATCH or stalled.size == 0
        f = {m: v[live] for m, v in C.figures(opt, got).items()}
        k = C.key(name, B) + (":dense" if solver == "dense" else "")
        out[k] = dict({m: C.worst(f[m]) for m in C.FIGURES}, instances=int(idx.size), certified=int(opt["certified"].sum()),
                      with_active_bound=int((opt["n_active"][opt["certified"]] >= 1).sum()), max_iter_seen=int(got["iter"][live].max()),
                      not_converged=[int(b) for b in stalled],
                      cond_P=float(max(c["cond_P"] for c in opt["certs"] if "cond_P" in c)))
        print(k, out[k], flush=True)
    # the fp64 oracle at the fp32 accuracy contract's settings (tol_abs = 1e-3): its distance to x* on the sampled instances it converges on
    for fam in C.FP32_FAMILIES:
        model, wl, prm, idx, opt, z, conv = C.fp32_reference(fam)
        ok = opt["certified"] & conv
        assert opt["certified"].mean() >= 0.95 and ok.mean() > 0.5, (fam, opt["certified"].mean(), ok.mean())
        dz = np.abs(z - opt["x"]).max(axis=1)[ok]
        out["fp32:" + fam] = dict(z_max=float(dz.max()), z_p99=float(np.quantile(dz, 0.99)), instances=int(idx.size), certified=int(opt["certified"].sum()),
                                  oracle_converged=int(conv.sum()), tol_abs=prm["tol_abs"], max_iter=prm["max_iter"])
        print("fp32:" + fam, out["fp32:" + fam], flush=True)
    with open(C.MEASURED_PATH, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
