"""Route census: which launch sequence every kind of handle takes through the on-chip engines (run_tail, loik_host.hip).

The answers of these handles are tested elsewhere; this records what no other test observes -- WHICH kernels ran.  Per handle,
for two consecutive solves: the integer fields of loikb_stats that depend only on the route and the arithmetic, the sum of the
iteration counts, and plan().  (lean_requeues and the times depend on timing and are left out.)

    python tests/golden/make_route_census.py OUT.json      # needs a GPU

route_census_parent.json is the record of the commit BEFORE run_tail was split by engine (fields that repeated over two runs of
the recorder); tests/test_route_census.py replays the handles and requires equality.  A refactor of the dispatch must not
re-record it: a difference is a change of behaviour.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIELDS = ["launches", "tail_launches", "lean_launches", "flat_launches", "flat_split_launches", "flat_ordered", "flat_built",
          "lean_escaped", "n_unfinished"]


def _spd(seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((6, 6))
    return M @ M.T + 6.0 * np.eye(6)


def _t32(B, **kw):
    return dict(robot="talos32", B=B, **kw)


def _t44(B, **kw):
    return dict(robot="talos44", B=B, **kw)


# name -> the handle: robot, batch, environment at create, constructor keywords, reference weight, second solve's inputs
CASES = {
    "talos32_b1": _t32(1),
    "talos32_b63": _t32(63),
    "talos32_b2049": _t32(2049),   # (just past the short sequence)
    "talos32_b4096_slice8": _t32(4096, env={"LOIKB_FLAT_SLICE": "8"}),
    "talos32_b4096_build1_window": _t32(4096, env={"LOIKB_FLAT_BUILD": "1", "LOIKB_FLAT_WINDOW": "0,2"}),
    "talos44_b300": _t44(300),
    "talos44_b300_slice8": _t44(300, env={"LOIKB_FLAT_SLICE": "8"}),
    "talos32_href_diagonal": _t32(300, href="diagonal"),
    "talos32_href_general": _t32(300, href="general"),
    "talos32_href_per_link": _t32(300, href="per_link"),
    "talos32_logging": _t32(96, prm=dict(logging=True)),
    "talos44_logging": _t44(96, prm=dict(logging=True)),
    "talos32_osqp": _t32(300, prm=dict(mu_update_strat=1)),
    "talos44_osqp": _t44(300, prm=dict(mu_update_strat=1)),
    "talos32_fp32": _t32(300, prm=dict(precision=1, tol_abs=1e-3)),
    "talos32_flat_off": _t32(300, env={"LOIKB_FLAT": "0"}),
    "talos32_flat_split_off": _t32(300, env={"LOIKB_FLAT_SPLIT": "0"}),
    "panda7_b4096": dict(robot="panda7", B=4096),
    "talos32_fixed_iters": _t32(300, prm=dict(flags=1, max_iter=30)),
    "talos32_order_from_previous": _t32(2049, prm=dict(flags=32), second_seed=99),
}

ENV_KEYS = ["LOIKB_FLAT", "LOIKB_FLAT_SPLIT", "LOIKB_FLAT_SLICE", "LOIKB_FLAT_BUILD", "LOIKB_FLAT_WINDOW"]


def _workload(case, seed):
    from loik_amd import workloads
    if case["robot"] == "talos32":
        return workloads.talos_c3(case["B"], seed=seed)
    if case["robot"] == "talos44":
        return workloads.talos_wholebody(case["B"], seed=seed)
    return workloads.panda_c5(case["B"], seed=seed)


def record(name):
    """Runs the handle `name` for two solves; returns {"plan": [..], "stats": [{field: int}, ..], "iters": [sum, sum]}."""
    import loik_amd
    case = CASES[name]
    saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    os.environ.update(case.get("env", {}))
    try:
        wl = _workload(case, 7)
        prm = dict(wl["params"], **case.get("prm", {}))
        s = loik_amd.BatchedLoik(wl["model"], case["B"], **prm)
    finally:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    href = case.get("href")
    H = np.diag([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]) if href == "diagonal" else _spd(3) if href == "general" else wl["H_ref"]
    out = dict(plan=[], stats=[], iters=[])
    for k in range(2):
        w = wl if k == 0 or "second_seed" not in case else _workload(case, case["second_seed"])
        args = (w["q"], H, w["v_ref"], w["c_ids"], w["Ais"], w["bis"], w["lb"], w["ub"])
        if href == "per_link":
            nj = wl["model"].njoints
            s.SolveInit(*args)
            s.UpdateReferences(np.stack([_spd(10 + i) for i in range(nj)]), np.zeros((nj, 6)))
            s.Solve()
        else:
            s.Solve(*args)
        st = s.stats()
        out["stats"].append({f: int(st[f]) for f in FIELDS})
        out["iters"].append(int(s.get("iter").astype(np.int64).sum()))
        out["plan"].append(s.plan())
    s.close()
    return out


if __name__ == "__main__":
    census = {}
    for name in CASES:
        census[name] = record(name)
        print(name, json.dumps(census[name]["stats"]), census[name]["iters"], flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(census, f, indent=1, sort_keys=True)
        f.write("\n")
