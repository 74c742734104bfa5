"""The problems of tests/test_qp_optimum_cpu.py and tests/test_qp_optimum_gpu.py: model families x formulations, paired (not the full
product), each a deterministic function of (case name, batch).  Also the tight solver settings, the oracle-side solve and the distance
figures both files and tests/golden/make_qp_optimum_measured.py share.

Settings: tol_abs = 1e-10, tol_rel = 0, tol_primal_inf = tol_dual_inf = 1e-14 (no certificate fires on a feasible problem), max_iter =
50000 (every compared instance converges; one that does not is a failure, not an exclusion).

Instances the solver never converges on.  Under the reference's penalty rule (mu x 10 / / 10 on a residual ratio of 10, at every
iteration) a few well-posed instances of the headline workload stall: mu flips between two decades and the residuals stay at 1e-2 for
50000 iterations (workloads.talos_c3(63): instances 23 and 42; about 3 % of a larger batch).  The CPU batches (24) hold none and assert
that all converge.  The batches of the GPU file (63, 300 of the headline workload, as the device is used) do hold some.  They are not
dropped: stalled_instances() runs the C oracle on the WHOLE batch, the record names the stalled instances, and the GPU file asserts
that an engine converges on every other one, flags none infeasible, and compares whatever it converges on with x*."""
import json
import os

import numpy as np

import loik_amd
from loik_amd import workloads as W
from helpers import FIXTURE, composite_tree, helical_tree, random_tree, random_tree_multidof, renumber_breadth_first
import pose_tasks_numpy as T
import qp_numpy as Q

TIGHT = dict(FIXTURE, tol_abs=1e-10, tol_rel=0.0, tol_primal_inf=1e-14, tol_dual_inf=1e-14, max_iter=50000)
FLOOR = 1e-12
FIGURES = ("z", "nu", "vis", "stationarity", "y", "w")
MEASURED_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qp_optimum_measured.json")

_MODELS = {}


def model_of(name):
    if name not in _MODELS:
        if name in ("panda7", "talos32", "talos44"):
            m = loik_amd.builtin_model(name)
        elif name == "tree20":
            m = random_tree(6, 20)
        elif name == "tree31":
            m = random_tree(12, 31, branch_prob=0.3)   # (31 joints, at most four children, a tree the flat schedule takes; depth 14, 13 ancestors: too deep for k_flat2, and k_flat<double, 16> is refused by the plan -- tests/flat_census.py -- so the level-by-level engines run it)
        elif name == "tree35":
            m = random_tree(8, 35)
        elif name == "deep60":
            m = random_tree(15, 60, branch_prob=0.45)   # (depth 15: the deepest of these seeds the flat schedule takes)
        elif name == "bushy42":
            from test_bushy_trees import bushy_tree
            m = bushy_tree(77, 42, 2, 10)
        elif name == "helical24":
            m = helical_tree(21, 24, 5)
        elif name == "multidof20":   # free-flyer root, spherical, translation, ZYX, planar, (cos, sin) revolutes
            m = random_tree_multidof(5, 20, root_freeflyer=True, n_spherical=1, n_translation=1, n_zyx=1, n_planar=1, n_rub=1, n_rubu=1)
        elif name == "composite20":  # a universal joint (two unaligned revolutes), a 3- and a 4-sub-joint composite
            m = composite_tree(41, 20, [1, 5, 9], kinds=[[7, 7], [4, 15, 8], [2, 18, 5, 7]])
        elif name == "talos32_bfs":
            m = renumber_breadth_first(loik_amd.builtin_model("talos32"))[0]
        elif name == "multidof9":
            m = random_tree_multidof(seed=5, nb=9, root_freeflyer=True, n_spherical=1, n_translation=1)
        else:
            raise KeyError(name)
        _MODELS[name] = m
    return _MODELS[name]


def _spd(rng):
    Qm = np.linalg.qr(rng.normal(size=(6, 6)))[0]
    H = Qm @ np.diag(rng.uniform(0.3, 3.0, size=6)) @ Qm.T
    return 0.5 * (H + H.T)


# name -> model, task links (joint names or ids; negative: from the end), A, H_ref, v_ref, bounds, penalty rule
#   A: identity | general | per_instance | position | orientation (the rank-3 masks of set_pose_tasks, with a tool frame)
#   H: identity | scalar | diagonal | general | per_link;   v: zero | nonzero | per_link
#   bounds: loose | active | per_instance (active too)
CASES = {
    "panda7":            dict(model="panda7", links=[-1], A="identity", H="identity", v="zero", bounds="loose", mu=0, seed=101),
    "panda7_active":     dict(model="panda7", links=[-1], A="position", H="diagonal", v="nonzero", bounds="active", mu=1, seed=102),
    "talos32_c3":        dict(model="talos32", workload="talos_c3", bounds="active", mu=0),
    "talos32_general":   dict(model="talos32", links=["arm_left_7_joint", "leg_right_6_joint"], A="general", H="general", v="nonzero",
                              bounds="active", mu=0, seed=103),
    "talos44_wholebody": dict(model="talos44", workload="talos_wholebody", bounds="active", mu=0),
    "talos44_osqp":      dict(model="talos44", workload="talos_wholebody", bounds="active", mu=1),
    "tree20":            dict(model="tree20", links=[-1, 9], A="general", H="diagonal", v="zero", bounds="per_instance", mu=0, seed=104),
    "tree31":            dict(model="tree31", links=[-1], A="identity", H="scalar", v="nonzero", bounds="active", mu=0, seed=112),
    "tree35":            dict(model="tree35", links=[-1], A="per_instance", H="general", v="nonzero", bounds="loose", mu=1, seed=105),
    "deep60":            dict(model="deep60", links=[-1, 30], A="identity", H="per_link", v="per_link", bounds="active", mu=0, seed=106),
    "bushy42":           dict(model="bushy42", links=[-1, 20, 3, 11], A="general", H="scalar", v="zero", bounds="loose", mu=0, seed=107),
    "helical24":         dict(model="helical24", links=[-1], A="position", H="scalar", v="zero", bounds="active", mu=0, seed=108),
    "multidof20":        dict(model="multidof20", links=[-1, 8], A="general", H="identity", v="nonzero", bounds="active", mu=0, seed=109),
    "composite20":       dict(model="composite20", links=[-1], A="orientation", H="per_link", v="per_link", bounds="per_instance", mu=0,
                              seed=110),
    "talos32_bfs":       dict(model="talos32_bfs", links=["arm_left_7_joint"], A="per_instance", H="identity", v="zero",
                              bounds="per_instance", mu=1, seed=111),
}
ACTIVE = [n for n, c in CASES.items() if c["bounds"] != "loose"]
# what oracle/dense.py takes: 1-DoF, free-flyer, spherical and translation joints, the default penalty rule, few joints (it is dense)
DENSE_CASES = {
    "dense_panda7":    dict(model="panda7", links=[-1], A="general", H="general", v="nonzero", bounds="loose", mu=0, seed=201),
    "dense_multidof9": dict(model="multidof9", links=[-1, 4], A="identity", H="per_link", v="per_link", bounds="loose", mu=0, seed=202),
}


def _link(model, l):
    if isinstance(l, str):
        return model.getJointId(l)
    return model.njoints + l if l < 0 else int(l)


def problem(name, B):
    """the workload of a case: dict(model, prm, q, H_ref, v_ref, c_ids, Ais, bis, lb, ub, refs = (H_refs, v_refs) or None, nu_star)"""
    c = dict(CASES, **DENSE_CASES)[name]
    model = model_of(c["model"])
    nv, nj = model.nv, model.njoints
    if "workload" in c:
        wl = getattr(W, c["workload"])(B, model=model)
        wl = {k: wl[k] for k in ("q", "H_ref", "v_ref", "c_ids", "Ais", "bis", "lb", "ub", "nu_star")}
        nc = len(wl["c_ids"])
        return dict(wl, model=model, refs=None, prm=dict(TIGHT, num_eq_c=nc, mu_update_strat=c["mu"]), name=name)
    rng = np.random.default_rng(c["seed"])
    links = [_link(model, l) for l in c["links"]]
    nc = len(links)
    q = model.random_configurations(rng, B)
    bound = 4.0 if c["bounds"] == "loose" else 0.5
    lb, ub = -bound * np.ones(nv), bound * np.ones(nv)
    if c["bounds"] == "per_instance":
        lb = -bound * (1 + 0.2 * rng.random((B, nv)))
        ub = bound * (1 + 0.2 * rng.random((B, nv)))
    # a feasible point: inside the box, a quarter of its components ON the box where the bounds are to be active
    lo, hi = np.broadcast_to(lb, (B, nv)), np.broadcast_to(ub, (B, nv))
    scale = 0.125 if c["bounds"] == "loose" else 1.0
    nu_star = scale * rng.uniform(lo, hi)
    if c["bounds"] != "loose":
        snap = rng.random((B, nv)) < 0.25
        nu_star = np.where(snap, np.where(nu_star > 0, hi, lo), nu_star)
    if c["A"] == "identity":
        A = np.tile(np.eye(6), (nc, 1, 1))
    elif c["A"] == "general":
        A = np.eye(6)[None] + 0.3 * rng.normal(size=(nc, 6, 6))
    elif c["A"] == "per_instance":
        A = np.eye(6)[None, None] + 0.3 * rng.normal(size=(B, nc, 6, 6))
    else:
        kind = T.TASK_POSITION if c["A"] == "position" else T.TASK_ORIENTATION
        A = T.task_matrices([kind] * nc, T.random_frames(rng, nc))
    b = np.empty((B, nc, 6))
    for k, l in enumerate(links):
        v = W.link_velocity(model, q, nu_star, l)
        b[:, k] = np.einsum("bij,bj->bi", A[:, k], v) if A.ndim == 4 else v @ A[k].T   # (in the range of A_c by construction)
    H = {"identity": np.eye(6), "scalar": 2.5 * np.eye(6), "diagonal": np.diag([0.4, 1.5, 0.7, 3.0, 0.2, 2.2])}.get(c["H"])
    if c["H"] in ("general", "per_link"):
        H = _spd(rng)
    vref = np.zeros(6) if c["v"] == "zero" else 0.05 * rng.normal(size=6)
    refs = None
    if c["H"] == "per_link" or c["v"] == "per_link":
        Hs = np.stack([_spd(rng) for _ in range(nj)]) if c["H"] == "per_link" else np.tile(H, (nj, 1, 1))
        vs = 0.05 * rng.normal(size=(nj, 6)) if c["v"] == "per_link" else np.tile(vref, (nj, 1))
        refs = (Hs, vs)
    return dict(model=model, prm=dict(TIGHT, num_eq_c=nc, mu_update_strat=c["mu"]), q=q, H_ref=H, v_ref=vref,
                c_ids=np.array(links, dtype=np.int32), Ais=A, bis=b, lb=lb, ub=ub, refs=refs, nu_star=nu_star, name=name)


def solve_args(wl):
    return (wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])


def reference(wl, idx=None):
    """qp_numpy.optimum of (a sample of) a workload, its per-link references included"""
    a = list(solve_args(wl))
    if wl["refs"] is not None:
        a[1], a[2] = wl["refs"]
    return Q.optimum(wl["model"], *a, idx=idx)


def _one(wl, b):
    pick = lambda a, nd: a if np.asarray(a).ndim == nd else a[b]
    return (wl["q"][b], wl["H_ref"], wl["v_ref"], wl["c_ids"], pick(wl["Ais"], 3), wl["bis"][b], pick(wl["lb"], 1), pick(wl["ub"], 1))


def oracle_solve(wl, idx, solver="ref"):
    """the CPU oracle (oracle/loik_ref.c, or oracle/dense.py) on instances idx: dict(z, nu, vis [n][njoints][6], yis [n][nc][6], w,
    converged, infeasible, iter)"""
    from oracle import dense, ref
    model, prm = wl["model"], wl["prm"]
    out = {k: [] for k in ("z", "nu", "vis", "yis", "w", "converged", "infeasible", "iter")}
    for b in idx:
        if solver == "ref":
            s = ref.RefSolver(model, **prm)
        else:
            s = dense.DenseSolver(model, **{k: v for k, v in prm.items() if k != "eq_c_capacity"})
        if wl["refs"] is None:
            s.Solve(*_one(wl, b))
        else:
            s.SolveInit(*_one(wl, b)); s.UpdateReferences(*wl["refs"]); s.Solve()
        yis = np.asarray(s.yis)
        if solver != "ref":
            yis = yis[[int(c) for c in wl["c_ids"]]]   # (the plain solver keeps one dual per joint)
        for k, v in (("z", s.z), ("nu", s.nu), ("vis", s.vis), ("yis", yis), ("w", s.w)):
            out[k].append(np.array(v, dtype=float))
        out["converged"].append(bool(s.get_convergence_status() if solver == "ref" else s.converged))
        out["infeasible"].append(bool(s.get_primal_infeasibility_status() if solver == "ref" else s.primal_infeasible))
        out["iter"].append(int(s.get_iter()))
    return {k: np.array(v) for k, v in out.items()}


def figures(opt, got):
    """per instance of opt["idx"] (nan where the reference is not certified; y, w: nan where the multipliers are not unique): |z - x*|_inf, |nu - x*|_inf, max_i |vis_i - J_i x*|_inf and
    the stationarity residual |P z + c + sum_c J_c^T A_c^T y_c + w|_inf built from the SOLVER's duals and the independent Jacobians.
    got: z, nu [n][nv], vis [n][njoints][6] (row 0 = the universe), yis [n][nc][6], w [n][nv] of the same instances."""
    n = opt["idx"].size
    f = {k: np.full(n, np.nan) for k in FIGURES}
    for k in np.flatnonzero(opt["certified"]):
        f["z"][k] = np.abs(got["z"][k] - opt["x"][k]).max()
        f["nu"][k] = np.abs(got["nu"][k] - opt["x"][k]).max()
        f["vis"][k] = np.abs(got["vis"][k] - opt["vis"][k]).max()
        f["stationarity"][k] = np.abs(Q.stationarity_residual(opt["qp"], k, got["z"][k], got["yis"][k], got["w"][k])).max()
        # the duals in value where the reference's are unique: every task block of full row rank (a rank-3 mask leaves yis free along
        # the zero rows) -- w = -(P x + c + E^T y) on the active set then is, too
        if opt["certs"][k]["rank_E"] == 6 * opt["y"].shape[1]:
            f["y"][k] = np.abs(got["yis"][k] - opt["y"][k]).max()
            f["w"][k] = np.abs(got["w"][k] - opt["w"][k]).max()
    return f


def check_conditions(name, wl, opt):
    """what keeps a case from being hollowed out: at most 5 % of the instances uncertified and never all; a quarter of the certified
    instances of an "active bounds" case with an active bound; every constraint block of a multi-constraint case nonzero"""
    cert = opt["certified"]
    why = [c for c in opt["certs"] if not c["certified"]][:3]
    assert cert.any() and (~cert).mean() <= 0.05, (name, int(cert.sum()), cert.size, why)
    if name in ACTIVE:
        assert (opt["n_active"][cert] >= 1).mean() >= 0.25, (name, opt["n_active"])
    nc = len(wl["c_ids"])
    E, d = opt["qp"]["E"], opt["qp"]["d"]
    for c in range(nc):
        assert np.all(np.abs(E[:, 6 * c:6 * c + 6]).max(axis=(1, 2)) > 1e-3), (name, "constraint block", c)
        assert np.all(np.abs(d[:, 6 * c:6 * c + 6]).max(axis=1) > 1e-6), (name, "constraint target", c)


def measured():
    with open(MEASURED_PATH) as f:
        return json.load(f)


def sample(B, n=64, seed=2024):
    """the instances of a batch of B whose x* is computed: all of a small batch, else a fixed seeded sample of n"""
    return np.arange(B) if B <= n else np.sort(np.random.default_rng(seed + B).choice(B, size=n, replace=False))


CPU_BATCH = 24
# (case, batch) of the GPU file: batches of 1, 63 and a few hundred that cross the tiles of 64 instances
GPU_KEYS = [("tree31", 1), ("tree31", 130), ("talos32_c3", 63), ("talos32_c3", 300), ("talos32_general", 130), ("talos44_wholebody", 300),
            ("talos44_osqp", 63), ("tree20", 63), ("tree35", 63), ("deep60", 130), ("bushy42", 130), ("panda7", 63),
            ("panda7_active", 63), ("helical24", 130), ("multidof20", 130), ("composite20", 63), ("talos32_bfs", 63)]


def stalled_instances(wl):
    """the instances of the WHOLE batch the C oracle does not converge on within max_iter (sorted indices), none flagged infeasible"""
    from oracle import ref
    out = ref.solve_batch(wl["model"], *solve_args(wl), nthreads=8, refs=wl["refs"], **wl["prm"])
    assert not out["primal_infeasible"].any(), (wl["name"], np.flatnonzero(out["primal_infeasible"]))
    return np.flatnonzero(~out["converged"])


def key(name, B):
    return "%s@%d" % (name, B)


def worst(values):
    """the largest of a figure over the instances that have one; None when none has (y, w of a case with rank-3 task matrices)"""
    v = np.asarray(values, dtype=float)
    v = v[np.isfinite(v)]
    return float(v.max()) if v.size else None


# ---- single precision: the families whose converged fp32 distance the project already pins (test_fp32_parity.CONTRACT_PINS, tol 1e-3) ----
FP32_FAMILIES = ("talos32", "talos44_wholebody", "multidof")
FP32_SAMPLE = 400


def fp32_problem(family):
    """(model, workload with fp32-exact inputs, params at tol_abs = 1e-3) of test_fp32_parity's accuracy contract, the sampled instances"""
    from test_fp32_parity import _contract_problem
    model, wl, prm = _contract_problem(family, loik_amd.builtin_model("talos32"))
    return model, wl, prm, sample(wl["q"].shape[0], n=FP32_SAMPLE)


def fp32_reference(family):
    """x* of the sample and the fp64 C oracle at the contract's settings on it: (model, wl, prm, idx, opt, oracle z [n][nv], converged [n])"""
    from oracle import ref
    model, wl, prm, idx = fp32_problem(family)
    a = solve_args(wl)
    opt = Q.optimum(model, *a, idx=idx)
    out = ref.solve_batch(model, wl["q"][idx], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"][idx], wl["lb"], wl["ub"], nthreads=8, **prm)
    return model, wl, prm, idx, opt, out["z"], out["converged"]
