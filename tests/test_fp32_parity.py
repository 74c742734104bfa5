"""Single-precision handles (precision = F32: the `float` instantiation of every device kernel) against the fp64 oracle.

The oracle is given the problem as the fp32 tiles hold it (helpers.f32_exact: every input rounded to float32 and widened back, the
device gets the same arrays), so input rounding is out of the comparison and what is measured is the device's own fp32 arithmetic.
Fixed-iteration runs (tol_abs = 0, tol_rel = 1e-30, tol_primal_inf = 0: no stopping decision) are compared per instance and per
field, normwise (helpers.normwise_error), against ten times what each case and field measured (max and median over the batch: a
bias shared by every instance shows in the median).  Then: every engine a float handle can take, problem
shapes (several constraints, A per instance, general references, multi-DoF / helical / composite joints, the penalty rules, odd
batch sizes), the set-up / edit / getter kernels, and the accuracy contract of LOIKB_OPT_F32_ACCURATE beyond Panda-7."""
import json
import os

import numpy as np
import pytest

import loik_amd
from loik_amd import capi, workloads
from helpers import (FIXTURE, U32, composite_tree, f32_exact, feasible_batch, helical_tree, multi_task_batch, normwise_error,
                     problem_args, random_tree, random_tree_multidof)
from oracle import ref

pytestmark = pytest.mark.gpu

FIELDS = ["nu", "z", "w", "vis", "fis", "g", "yis", "Aty", "Stf_plus_w", "primal_residual_vec", "dual_residual_vec", "liMi"]
SCALARS = ["primal_residual", "dual_residual", "primal_residual_task", "primal_residual_slack", "dual_residual_v",
           "dual_residual_nu", "mu", "delta_fis_inf_norm", "delta_yis_inf_norm", "delta_w_inf_norm", "delta_vis_inf_norm",
           "delta_nu_inf_norm", "Av_inf_norm", "nu_inf_norm", "Href_v_inf_norm", "g_inf_norm", "Stf_plus_w_inf_norm",
           "tol_primal", "tol_dual"]
# Fixed runs of k = 1, 2, 5, 12 iterations.  From the third iteration on the fp32 residual ratio takes the other branch of the penalty
# rule (mu x 10 / 10) than fp64 for many instances -- measured on an MI355X: 12-17 % at k = 5, 27-76 % at k = 12 (Panda-7, the bushy
# tree) -- and those follow another trajectory.  At k = 1, 2 no instance does (the ones within BORDER of the threshold are left out);
# at k = 5, 12 the instances whose mu differs from the oracle's at the end are left out too, and at least MIN_LATE_SHARE must remain.
KS = (1, 2, 5, 12)
EARLY = 2
MIN_LATE_SHARE = 0.2

# The bounds, per case and per field: the maximum over the compared instances of normwise_error(field) may be at most BOUND_FACTOR times
# what it measured on an MI355X for that case and field, the median at most BOUND_FACTOR times the measured median (a bias that shifts
# every instance shows there), neither below FLOOR_ULPS k u32 (fields the device reproduces exactly).  The measurements are the table
# tests/golden/fp32_parity_measured.json ({case: {field: [max, median]}}, His per 6x6 block of a joint); a case missing from it fails.
# Why one constant for every field would not do: the normwise error of a k = 1 run spans 1e-8 (w) to 1e-2 (Stf_plus_w of the 80-joint
# tree) -- mu_eq = 1e4 mu makes the constraint blocks of H badly conditioned -- and a bound set by the worst of them misses a 1e-3 error
# in the others.  LOIKB_FP32_MEASURE=<file> re-measures: the bounds are not asserted, each (case, field, max, median) is appended to
# <file> as a JSON line -- what the table was made from.
BOUND_FACTOR = 10.0
FLOOR_ULPS = 4.0
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fp32_parity_measured.json")) as _f:
    MEASURED = json.load(_f)
FLOOR = 1e-6          # (the norm below which a field is compared absolutely)
# Residuals, duals and the differences of iterates are small differences of O(1) terms (velocities of 0.1-1, forces of 1-50): fp32
# resolves them to u32 times the terms, not to u32 times themselves (dual_residual_v of the first iteration is 1e-8..1e-6 in fp64),
# so they are measured against the problem's unit scale.  tol_primal / tol_dual are tol_rel (1e-30 here) times norms: relative.
UNIT_SCALE = ("w", "Stf_plus_w", "primal_residual_vec", "dual_residual_vec", "primal_residual", "dual_residual", "primal_residual_task",
              "primal_residual_slack", "dual_residual_v", "dual_residual_nu", "delta_fis_inf_norm", "delta_yis_inf_norm", "delta_w_inf_norm",
              "delta_vis_inf_norm", "delta_nu_inf_norm", "Stf_plus_w_inf_norm")
RELATIVE = ("tol_primal", "tol_dual")


def _floor(name):
    return 1.0 if name in UNIT_SCALE else 1e-300 if name in RELATIVE else FLOOR


# The penalty rule multiplies mu by 10 when primal > 10 dual (divides when dual > 10 primal): an instance whose residual ratio comes
# within BORDER of a threshold at some iteration may take the other branch in fp32 and follow another trajectory -- a discontinuity,
# not an error.  Such instances (from the oracle's own residual lists) are left out, at most MAX_BORDER_SHARE of a sample.
BORDER = 0.01
MAX_BORDER_SHARE = 0.1
K_FK, K_FK_MEDIAN = 16.0, 4.0   # liMi of the fp32 tiles against the numpy kinematics, normwise per instance, in u32 (measured: max 2.8, median 1.4)

ENV_KEYS = ("LOIKB_LEAN", "LOIKB_FLAT", "LOIKB_FLAT_SPLIT", "LOIKB_FLAT_SLICE", "LOIKB_LEAN_WG_PER_CU", "LOIKB_LEAN_KLO",
            "LOIKB_LEAN_DECADES", "LOIKB_LEAN_ADAPT", "LOIKB_FLAT_BUILD")


def _env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _margin(what, err, bound):
    """a record of how much of each bound is used (LOIKB_TEST_MARGINS, as helpers.assert_end_to_end keeps it)"""
    if os.environ.get("LOIKB_TEST_MARGINS"):
        with open(os.environ["LOIKB_TEST_MARGINS"], "a") as f:
            f.write("%-70s n %5d  max %.3e  median %.3e  bound %.3e  used %.3f\n" % (
                what, np.size(err), float(np.max(err)), float(np.median(err)), bound, float(np.max(err)) / bound if bound > 0 else float("inf")))


def _args(wl):
    return (wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])


def _oracle_state(r, model, his=True):
    """the oracle's values of FIELDS / SCALARS / His, shaped as the device's getters return them"""
    out = {}
    for n in FIELDS:
        w = r.field(n)
        out[n] = w[1:] if n in ("vis", "fis", "g", "liMi") else w
    for n in SCALARS:
        out[n] = r.scalar(n)
    if his:
        out["His"] = r.His[1:]
    return out


def borderline(r, rule=0):
    """did the oracle's penalty rule come within BORDER of its threshold in the last solve (its SolverInfo lists)?"""
    if rule == 1:   # (OSQP: a change by more than a factor of 5 -- not visible in the lists; mu is compared like any field)
        return False
    p, d = r.solver_info(2), r.solver_info(5)
    ratio = np.abs(np.log10(np.maximum(p, 1e-300) / np.maximum(d, 1e-300)))
    return bool(np.any(np.abs(ratio - 1.0) < np.log10(1.0 + BORDER)))


def assert_within_bound(got, want, idx, iters, what, skip=(), border=None, late=None):
    """got: {name: [B, ...]} of the fp32 handle; want: {name: [len(idx), ...]} of the oracle for instances idx; the normwise error of
    every field against BOUND_FACTOR times its measurement for this case (max, median); border: [len(idx)] bool, instances left out
    (borderline penalty decisions); late: for k > EARLY, [len(idx)] bool, instances whose final mu is not the oracle's (left out).
    Returns {name: max error} for the message."""
    keep = np.ones(idx.size, dtype=bool) if border is None else ~np.asarray(border, dtype=bool)
    assert (~keep).sum() <= max(1, MAX_BORDER_SHARE * idx.size), (what, "borderline penalty decisions", int((~keep).sum()), idx.size)
    if late is not None:   # (k > EARLY: the instances whose final mu is the oracle's)
        keep &= ~np.asarray(late, dtype=bool)
        assert keep.mean() >= MIN_LATE_SHARE, (what, "instances that kept the oracle's mu", keep.mean())
    worst, bad = {}, []
    for n in want:
        if n in skip:
            continue
        floor_ = FLOOR_ULPS * iters * U32
        meas = MEASURED.get(what, {}).get(n) if not os.environ.get("LOIKB_FP32_MEASURE") else (0.0, 0.0)
        assert meas is not None, (what, n, "no measurement in tests/golden/fp32_parity_measured.json")
        bound, bound_med = max(BOUND_FACTOR * meas[0], floor_), max(BOUND_FACTOR * meas[1], floor_)
        if n == "His":   # (per 6x6 block of a joint: the blocks of the constrained links, mu_eq A^T A, are 1e4 times the others)
            g_, w_ = np.asarray(got[n])[idx], np.asarray(want[n])
            err = normwise_error(g_.reshape(-1, 36), w_.reshape(-1, 36), FLOOR).reshape(idx.size, -1).max(axis=1)[keep]
        else:
            err = normwise_error(np.asarray(got[n])[idx], want[n], _floor(n))[keep]
        worst[n] = float(err.max())
        _margin("%s %s" % (what, n), err, bound)
        if os.environ.get("LOIKB_FP32_MEASURE"):
            with open(os.environ["LOIKB_FP32_MEASURE"], "a") as f:
                f.write(json.dumps([what, n, float(err.max()), float(np.median(err))]) + "\n")
            continue
        if err.max() > bound or np.median(err) > bound_med:
            bad.append((n, float(err.max()), float(np.median(err)), int(idx[keep][int(np.argmax(err))])))
    assert not bad, (what, "bound %.2e" % bound, bad)
    return worst


def fixed_iterations(model, wl, prm_base, what, ks=KS, stride=1, handle_kw=None, his=True, check=None):
    """k fixed iterations on an fp32 handle (a fresh handle per k), every FIELD / SCALAR (+ His) of a strided sample against the oracle
    fed the same fp32-exact problem; check(s, k) runs on each handle before it is closed"""
    B = wl["q"].shape[0]
    idx = np.arange(0, B, stride)
    for k in ks:
        prm = dict(prm_base, max_iter=k + 1, tol_abs=0.0, tol_rel=1e-30, tol_primal_inf=0.0)
        s = loik_amd.BatchedLoik(model, B, precision=capi.F32, **prm, **(handle_kw or {}))
        s.Solve(*_args(wl))
        got = {n: s.get(n) for n in FIELDS + SCALARS}
        if his:
            got["His"] = s.His_full()
        assert np.all(s.get("iter") == k), (k, np.unique(s.get("iter")))
        if check is not None:
            check(s, k)
        want, border = {}, np.zeros(idx.size, dtype=bool)
        for j, b in enumerate(idx):
            r = ref.RefSolver(model, **prm)
            r.Solve(*problem_args(wl, b))
            border[j] = borderline(r, prm["mu_update_strat"])
            for n, v in _oracle_state(r, model, his).items():
                want.setdefault(n, np.empty((idx.size,) + np.shape(v)))[j] = v
        if prm["mu_update_strat"] == 3 and k <= EARLY:   # (MAXEIGENVALUE: mu0 is 10^(n/4) of an fp32 eigenvalue estimate -- a grid, with borders too)
            border |= np.abs(np.log(np.asarray(got["mu"])[idx] / want["mu"])) > 0.1
        late = None if k <= EARLY else np.abs(np.log(np.asarray(got["mu"])[idx] / want["mu"])) > 1e-3
        assert_within_bound(got, want, idx, k, "%s %s k%d" % (what, model.name, k), border=border, late=late)
        s.close()


# reasons the plan gives for no flat engine AFTER "fp32 solver" (loikb_plan_string): where the fp64 twin of a handle runs the flat engine
# or gives one of these, the float handle must say "fp32 solver"
AFTER_FP32 = ("LOIKB_OPT_NO_H_CACHE", "OSQP penalty rule", "a small robot", "more task constraints", "constraint blocks leave")


def _no_flat(s, twin=None):
    """a float handle never reaches the flat engines (fp64 only); with twin (the same handle in fp64, its plan made by the same SolveInit)
    the plan says why: "fp32 solver" wherever that is the first reason, else the fp64 handle's own"""
    st = s.stats()
    assert st["flat_launches"] == 0 and st["flat_split_launches"] == 0, (s.plan(), st)
    if twin is not None:
        p64, p32 = twin.plan(), s.plan()
        why64 = p64.split("; no k_flat: ")[1] if "; no k_flat: " in p64 else None
        if why64 is None or why64.startswith(AFTER_FP32):
            assert "; no k_flat: fp32 solver" in p32, (p64, p32)
        else:
            assert "; no k_flat: " + why64.split(";")[0] in p32, (p64, p32)


def _twin64(model, B, prm, kw, wl):
    t = loik_amd.BatchedLoik(model, B, **prm, **kw)
    t.SolveInit(*_args(wl))
    return t


# ---- 2. every engine a float handle can take -------------------------------------------------------------------------------------------

def _talos_wl(talos, B, seed=91):
    return feasible_batch(talos, B, talos.getJointId("arm_left_7_joint"), seed, nu_scale=0.5)


# engine -> (env, handle kw, robot, check(stats, B) of the run to convergence)
def _lean(st, B):
    return st["lean_launches"] >= 1 and st["lean_escaped"] == 0 and st["tail_instances"] == B


def _tail(st, B):
    return st["lean_launches"] == 0 and st["tail_instances"] > 0


def _solve(st, B):
    return st["tail_instances"] == 0 and st["lean_launches"] == 0


ENGINES32 = {
    "lean-talos32": (dict(), dict(), "talos32", _lean),
    "lean-tree21": (dict(), dict(), "tree21", _lean),
    "lean-talos44": (dict(), dict(), "talos44", _lean),
    "tail-talos32": (dict(LOIKB_LEAN="0"), dict(tail_max_instances=1 << 20), "talos32", _tail),
    "solve-talos32": (dict(), dict(tail_max_instances=-1), "talos32", _solve),
    "solve-tree80": (dict(), dict(), "tree80", _solve),
    "hybrid-talos32": (dict(LOIKB_LEAN="0"), dict(tail_max_instances=120, max_launch_iters=2), "talos32",
                       lambda st, B: st["lean_launches"] == 0 and 0 < st["tail_instances"] < B),
    "hybrid_lean-talos32": (dict(), dict(tail_max_instances=120, max_launch_iters=2), "talos32",
                            lambda st, B: st["lean_launches"] >= 1 and 0 < st["tail_instances"] < B),
    "lean_escapes-talos32": (dict(LOIKB_LEAN_KLO="0", LOIKB_LEAN_DECADES="2"), dict(), "talos32",
                             lambda st, B: st["lean_launches"] >= 1 and st["lean_escaped"] > 0),
    "default-panda7": (dict(), dict(), "panda7", _tail),
    "accurate-panda7": (dict(), dict(flags=capi.OPT_F32_ACCURATE), "panda7", _lean),
    "pass-talos32": (dict(), dict(logging=True), "talos32", _solve),
    "bushy-42x10": (dict(), dict(), "bushy", lambda st, B: st["lean_launches"] == 0 and st["tail_instances"] == B),
}


def _engine_problem(robot, B, request):
    if robot in ("talos32", "talos44"):
        model = request.getfixturevalue("talos") if robot == "talos32" else loik_amd.builtin_model("talos44")
        return model, _talos_wl(model, B), dict(FIXTURE)
    if robot == "panda7":
        model = request.getfixturevalue("panda7")
        return model, feasible_batch(model, B, model.njoints - 1, 92, bound=1.0, nu_scale=0.8), dict(FIXTURE)
    if robot == "bushy":
        from test_bushy_trees import bushy_tree
        model = bushy_tree(77, 42, 2, 10, depth_first=False)
        links = [model.njoints - 1, model.njoints - 1 - 42 // 10]
        return model, multi_task_batch(model, B, links, 13, nu_scale=0.3), dict(FIXTURE, num_eq_c=2)
    nb = int(robot[4:])
    model = random_tree(6, 21) if nb == 21 else random_tree(3, 80, branch_prob=0.3)
    if nb == 80:
        return model, multi_task_batch(model, B, [nb // 3, nb], 7, nu_scale=0.3), dict(FIXTURE, num_eq_c=2)
    return model, feasible_batch(model, B, model.njoints - 1, 91, nu_scale=0.5), dict(FIXTURE)


@pytest.mark.parametrize("engine", list(ENGINES32))
def test_fp32_engine_matches_the_oracle(engine, request, monkeypatch):
    env, kw, robot, ran = ENGINES32[engine]
    _env(monkeypatch, env)
    B = 600
    model, wl, prm = _engine_problem(robot, B, request)
    wl = f32_exact(wl)
    fixed_iterations(model, wl, prm, engine, stride=3, handle_kw=kw, check=lambda s, k: _no_flat(s))
    # to convergence: the engine this case names is the one that ran, and the answer stays in the box
    prm_e = dict(prm, max_iter=300, tol_abs=1e-4, tol_rel=0.0)
    s = loik_amd.BatchedLoik(model, B, precision=capi.F32, **prm_e, **kw)
    s.Solve(*_args(wl))
    st = s.stats()
    assert ran(st, B), (engine, s.plan(), st)
    twin = _twin64(model, B, prm_e, kw, wl)
    _no_flat(s, twin)
    twin.close()
    if engine.startswith("pass"):
        assert "k_pass_solve" in s.plan(), s.plan()
    z = s.get("z")
    assert np.all(z <= wl["ub"] + 1e-6) and np.all(z >= wl["lb"] - 1e-6)
    if not engine.startswith("pass"):   # (k_pass_solve does not count them)
        assert st["instance_iterations"] == int(s.get("iter").sum())
    s.close()


# ---- 3. problem shapes on the default fp32 engine --------------------------------------------------------------------------------------

def _shape_problem(case, talos, B):
    la, ra, ll = (talos.getJointId(n) for n in ("arm_left_7_joint", "arm_right_7_joint", "leg_left_6_joint"))
    if case == "nc3_A_per_instance":
        return talos, multi_task_batch(talos, B, [la, ra, ll], 21, per_instance_A=True), dict(FIXTURE, num_eq_c=3), True
    if case == "general_H_ref_v_ref":
        wl = _talos_wl(talos, B, seed=22)
        Q = np.linalg.qr(np.random.default_rng(4).normal(size=(6, 6)))[0]
        H = Q @ np.diag([0.4, 1.5, 0.7, 3.0, 0.2, 2.2]) @ Q.T
        wl["H_ref"], wl["v_ref"] = 0.5 * (H + H.T), np.array([0.02, -0.01, 0.03, 0.05, -0.04, 0.01])
        return talos, wl, dict(FIXTURE), True
    if case == "multidof":
        m = random_tree_multidof(5, 20, root_freeflyer=True, n_spherical=1, n_translation=1, n_zyx=1, n_planar=1, n_rub=1, n_rubu=1)
        return m, workloads.make_workload(m, B, m.njoints - 1, 23, bound=0.5, snap_prob=0.2, nu_scale=0.4), dict(FIXTURE), True
    if case == "helical":
        m = helical_tree(122, 22, 4, branch_prob=0.5)
        return m, workloads.make_workload(m, B, m.njoints - 1, 24, bound=0.5, snap_prob=0.0, nu_scale=0.4), dict(FIXTURE), True
    if case == "composite":
        m = composite_tree(41, 20, [1, 5, 9])
        return m, workloads.make_workload(m, B, m.njoints - 1, 25, bound=0.5, snap_prob=0.0, nu_scale=0.4), dict(FIXTURE), False
    if case in ("osqp", "maxeigenvalue"):
        rule = 1 if case == "osqp" else 3   # (LOIKB_MU_OSQP, LOIKB_MU_MAXEIGENVALUE)
        return talos, _talos_wl(talos, B, seed=26), dict(FIXTURE, mu_update_strat=rule), True
    raise KeyError(case)


@pytest.mark.parametrize("case", ["nc3_A_per_instance", "general_H_ref_v_ref", "multidof", "helical", "composite", "osqp", "maxeigenvalue"])
def test_fp32_problem_shapes_match_the_oracle(case, talos, monkeypatch):
    _env(monkeypatch, {})
    B = 400
    model, wl, prm, his = _shape_problem(case, talos, B)
    wl = f32_exact(wl)
    twin = _twin64(model, B, prm, {}, wl)
    fixed_iterations(model, wl, prm, case, stride=2, his=his, check=lambda s, k: _no_flat(s, twin))
    twin.close()


@pytest.mark.parametrize("B", [1, 5, 63, 65, 4097])
def test_fp32_batch_sizes_match_the_oracle(B, talos, monkeypatch):
    """one instance, part of a wavefront, a wavefront and one more, a ragged last tile: SolveInit's small-batch path (k_set_q_fk_small)
    and the bulk one (k_fk_init)"""
    _env(monkeypatch, {})
    wl = f32_exact(_talos_wl(talos, B, seed=27))
    twin = _twin64(talos, B, dict(FIXTURE), {}, wl)
    fixed_iterations(talos, wl, dict(FIXTURE), "B%d" % B, stride=max(1, B // 200), check=lambda s, k: _no_flat(s, twin))
    twin.close()


# ---- 4. set-up, edit and getter kernels in fp32 ----------------------------------------------------------------------------------------

def _local_placements(model, q):
    """liMi = jointPlacement * M(q) of every joint, [B][nb][12] (numpy, fp64)"""
    from pose_numpy import joint_motion
    out = np.empty((q.shape[0], model.njoints - 1, 12))
    for i in range(1, model.njoints):
        P = np.asarray(model.placement[i], dtype=float)
        Rp, tp = P[:9].reshape(3, 3), P[9:]
        Rj, tj = joint_motion(model, i, q)
        out[:, i - 1, :9] = (Rp[None] @ Rj).reshape(-1, 9)
        out[:, i - 1, 9:] = tp[None] + tj @ Rp.T
    return out


@pytest.mark.parametrize("which", ["multidof", "helical"])
def test_fp32_kinematics_before_and_after_integrate(which):
    """FwdPassInit's pairs (k_fk_init / k_set_q_fk_small<float>) and the liMi getter (k_limi<float>) against the numpy kinematics,
    over every joint type of the tree; integrate (k_advance_q<float>: q <- q (+) dt z with z read from the fp32 tiles) against the numpy
    integrator; the next solve's kinematics on the integrated q"""
    from pose_numpy import fk12, integrate
    if which == "multidof":
        model = random_tree_multidof(5, 20, root_freeflyer=True, n_spherical=1, n_translation=1, n_zyx=1, n_planar=1, n_rub=1, n_rubu=1)
        assert {9, 10, 11, 12, 13, 14, 18} <= set(int(t) for t in model.jtype)
    else:
        model = helical_tree(122, 22, 4, branch_prob=0.5)
        assert {19, 20, 21, 22} & set(int(t) for t in model.jtype)
    link = model.njoints - 1
    links = np.arange(1, model.njoints)
    dt = 0.05
    for B in (3, 300):   # (the small-batch set-up launch and the bulk one)
        wl = f32_exact(workloads.make_workload(model, B, link, 31, bound=0.5, snap_prob=0.0, nu_scale=0.4))
        prm = dict(FIXTURE, max_iter=6, tol_abs=0.0, tol_rel=1e-30, tol_primal_inf=0.0)
        s = loik_amd.BatchedLoik(model, B, precision=capi.F32, **prm)
        s.Solve(*_args(wl))
        q0 = wl["q"]
        assert np.array_equal(s.get("q"), q0)
        err = normwise_error(s.get("liMi"), _local_placements(model, q0), FLOOR)
        _margin("%s B%d liMi" % (model.name, B), err, K_FK * U32)
        assert err.max() <= K_FK * U32 and np.median(err) <= K_FK_MEDIAN * U32, ("liMi", err.max(), np.median(err))
        M = s.forward_kinematics(links)           # (fp64 from the resident q whatever the precision)
        M12 = np.concatenate([M[..., :3, :3].reshape(B, -1, 9), M[..., :3, 3]], axis=-1)
        assert np.abs(M12 - fk12(model, q0, links)).max() < 1e-12
        z = s.get("z")
        s.integrate(dt)
        q1 = s.get("q")
        want = np.stack([integrate(model, q0[b], dt * z[b]) for b in range(B)])
        assert np.abs(q1 - want).max() < 1e-9, np.abs(q1 - want).max()   # (fp64 both: the free-flyer's series / closed forms differ at 1.6e-10)
        Ai = wl["Ais"][0]
        s.Solve(None, link, Ai, wl["bis"][:, 0])        # (the tailored entry on the resident, integrated q)
        err = normwise_error(s.get("liMi"), _local_placements(model, q1), FLOOR)
        _margin("%s B%d liMi after integrate" % (model.name, B), err, K_FK * U32)
        assert err.max() <= K_FK * U32 and np.median(err) <= K_FK_MEDIAN * U32, ("liMi after integrate", err.max())
        s.close()


def _three_links(talos):
    return [talos.getJointId(n) for n in ("arm_left_7_joint", "arm_right_7_joint", "leg_left_6_joint")]


@pytest.mark.parametrize("shared_A", [True, False])
def test_fp32_constraint_edits_equal_a_fresh_handle(talos, shared_A, monkeypatch):
    """Add / Remove / Update on an fp32 handle (k_upload_rows<float>, k_edit_constraints<float>: the remaining constraints shift down a
    slot), then a solve: bit for bit what a fresh fp32 handle built with the final constraint set returns, and within the bound of the
    oracle driven through the same edits"""
    _env(monkeypatch, {})
    a, b_, c = _three_links(talos)
    B, k = 96, 2
    full = f32_exact(multi_task_batch(talos, B, [a, b_, c], 3, per_instance_A=not shared_A))
    A = {l: (full["Ais"][j] if shared_A else full["Ais"][:, j]) for j, l in enumerate((a, b_, c))}
    bv = {l: full["bis"][:, j] for j, l in enumerate((a, b_, c))}
    b_new = np.asarray(0.8 * bv[a], dtype=np.float32).astype(np.float64)
    prm = dict(FIXTURE, max_iter=k + 1, tol_abs=0.0, tol_rel=1e-30, tol_primal_inf=0.0, num_eq_c=2, eq_c_capacity=3)
    st = lambda ls: np.stack([A[l] for l in ls], axis=-3)
    s = loik_amd.BatchedLoik(talos, B, precision=capi.F32, **prm)
    s.Solve(full["q"], full["H_ref"], full["v_ref"], np.array([b_, a], dtype=np.int32), st([b_, a]), np.stack([bv[b_], bv[a]], axis=1),
            full["lb"], full["ub"])
    s.AddEqConstraint(c, A[c], bv[c])
    assert s.RemoveEqConstraint(b_)              # (slot 0 goes: a and c shift down)
    assert s.active_task_constraint_ids() == [a, c]
    s.UpdateEqConstraint(a, b_new)               # (c_id, bi): A kept -- a, not c: c's bi in its new slot is k_edit_constraints' copy alone
    s.Solve(full["q"], -1, None, None)
    names = ["iter", "z", "nu", "w", "vis", "fis", "g", "yis", "Aty", "mu", "primal_residual", "dual_residual", "Stf_plus_w"]
    got = {n: s.get(n) for n in names}
    fresh = loik_amd.BatchedLoik(talos, B, precision=capi.F32, **dict(prm, eq_c_capacity=0))
    fresh.Solve(full["q"], full["H_ref"], full["v_ref"], np.array([a, c], dtype=np.int32), st([a, c]), np.stack([b_new, bv[c]], axis=1),
                full["lb"], full["ub"])
    for n in names:
        assert np.array_equal(got[n], fresh.get(n)), n
    # the oracle through the same edits
    idx = np.arange(0, B, 4)
    want, border = {}, np.zeros(idx.size, dtype=bool)
    for j, b in enumerate(idx):
        pick = (lambda x: x) if shared_A else (lambda x: x[b])
        r = ref.RefSolver(talos, **prm)
        r.Solve(full["q"][b], full["H_ref"], full["v_ref"], np.array([b_, a], dtype=np.int32), np.stack([pick(A[b_]), pick(A[a])]),
                np.stack([bv[b_][b], bv[a][b]]), full["lb"], full["ub"])
        r.AddEqConstraint(c, pick(A[c]), bv[c][b])
        r.RemoveEqConstraint(b_)
        r.UpdateEqConstraint(a, b_new[b])
        r.Solve(full["q"][b], -1, None, None)
        border[j] = borderline(r)
        for n, v in _oracle_state(r, talos).items():
            want.setdefault(n, np.empty((idx.size,) + np.shape(v)))[j] = v
    got = {n: s.get(n) for n in FIELDS + SCALARS}
    got["His"] = s.His_full()
    assert_within_bound(got, want, idx, k, "edits shared_A=%s" % shared_A, border=border)
    s.close(); fresh.close()


def test_fp32_update_references_match_the_oracle(talos, monkeypatch):
    """per-link references (UpdateReferences: the per-link tables of an fp32 handle) between SolveInit and a fixed-iteration solve"""
    from test_formulation_editing import per_link_references
    _env(monkeypatch, {})
    B, k = 200, 2
    wl = f32_exact(_talos_wl(talos, B, seed=41))
    H, v = per_link_references(talos, 7)
    H, v = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (H, v))
    prm = dict(FIXTURE, max_iter=k + 1, tol_abs=0.0, tol_rel=1e-30, tol_primal_inf=0.0)
    s = loik_amd.BatchedLoik(talos, B, precision=capi.F32, **prm)
    s.SolveInit(*_args(wl))
    s.UpdateReferences(H, v)
    s.Solve()
    got = {n: s.get(n) for n in FIELDS + SCALARS}
    got["His"] = s.His_full()
    idx = np.arange(0, B, 2)
    want, border = {}, np.zeros(idx.size, dtype=bool)
    for j, b in enumerate(idx):
        r = ref.RefSolver(talos, **prm)
        r.SolveInit(*problem_args(wl, b))
        r.UpdateReferences(H, v)
        r.Solve()
        border[j] = borderline(r)
        for n, x in _oracle_state(r, talos).items():
            want.setdefault(n, np.empty((idx.size,) + np.shape(x)))[j] = x
    assert_within_bound(got, want, idx, k, "per-link references", border=border)
    _no_flat(s)
    s.close()


@pytest.mark.parametrize("robot,B,nc", [("talos32", 1, 1), ("talos32", 300, 1), ("talos44", 5, 4)])
def test_fp32_results_in_one_call_are_the_getters_values(robot, B, nc):
    """loikb_get_results on an fp32 handle (one gather of the fp32 tiles) against the single getters, bit for bit"""
    wl = (workloads.talos_c3 if robot == "talos32" else workloads.talos_wholebody)(B, seed=55)
    prm = dict(wl["params"], max_iter=120, tol_abs=1e-4)
    s = loik_amd.BatchedLoik(wl["model"], B, precision=capi.F32, **prm)
    s.Solve(*_args(wl))
    assert len(wl["c_ids"]) == nc
    names = ("z", "nu", "w", "vis", "fis", "yis")
    one = {k: s.get(k) for k in names}
    allr = s.get_results(names + ("scalars",))
    for k in names:
        assert allr[k].shape == one[k].shape and np.array_equal(allr[k], one[k]), k
    from loik_amd.capi import _SCALAR_FIELDS
    for j, name in enumerate(_SCALAR_FIELDS):
        assert np.array_equal(allr["scalars"][:, j], np.asarray(s.get(name))), name
    assert np.array_equal(allr["scalars"][:, s.SCALAR_ITER], np.asarray(s.get("iter")).astype(float))
    assert np.array_equal(allr["scalars"][:, s.SCALAR_STATUS], np.asarray(s.get("status")).astype(float))
    if nc > 1:
        s.RemoveEqConstraint(int(wl["c_ids"][-1]))
        s.Solve()
        r = s.get_results()
        assert r["yis"].shape == (B, nc - 1, 6)
        for k in names:
            assert np.array_equal(r[k], s.get(k)), k
    s.close()


@pytest.mark.parametrize("B", [1, 40])
def test_fp32_handle_reused_for_other_problems_answers_as_a_fresh_one(talos, B):
    """one fp32 handle through problems that differ in the task link, shared / per-instance A and bounds, the entry point (Solve(args),
    SolveInit + Solve(), the tailored Solve): bit for bit what a fresh fp32 handle returns"""
    la, lb_ = talos.getJointId("arm_left_7_joint"), talos.getJointId("leg_right_6_joint")
    probs = [feasible_batch(talos, B, la, 501, nu_scale=0.5), feasible_batch(talos, B, lb_, 502, nu_scale=0.5),
             feasible_batch(talos, B, la, 503, nu_scale=0.5, per_instance_A=True),
             feasible_batch(talos, B, lb_, 504, nu_scale=0.5, per_instance_bounds=True)]
    prm = dict(FIXTURE, max_iter=150, tol_abs=1e-4, tol_rel=0.0)
    keys = ("iter", "converged", "primal_infeasible", "z", "nu", "w", "yis", "fis", "vis")
    one = loik_amd.BatchedLoik(talos, B, precision=capi.F32, **prm)
    for k, wl in enumerate(probs):
        if k % 2 == 0:
            one.Solve(*_args(wl))
        else:
            one.SolveInit(*_args(wl)); one.Solve()
        fresh = loik_amd.BatchedLoik(talos, B, precision=capi.F32, **prm)
        fresh.Solve(*_args(wl))
        for f in keys:
            assert np.array_equal(one.get(f), fresh.get(f)), (k, f)
        wl2 = feasible_batch(talos, B, int(wl["c_ids"][0]), 600 + k, nu_scale=0.5)
        Ai = wl["Ais"][0] if np.asarray(wl["Ais"]).ndim == 3 else wl["Ais"][:, 0]
        one.Solve(wl2["q"], int(wl["c_ids"][0]), Ai, wl2["bis"][:, 0])
        fresh.Solve(wl2["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl2["bis"], wl["lb"], wl["ub"])
        for f in keys:
            assert np.array_equal(one.get(f), fresh.get(f)), (k, "tailored", f)
        fresh.close()
    one.close()


def test_fp32_tailored_warm_start_sequence_matches_the_oracle(talos, monkeypatch):
    """SolveInit, then Solve(q, c_id, Ai, bi) for T = 3 targets with warm_start (loikb_solve_tailored and the fp32 warm start), k fixed
    iterations a step: the state carries over, so step t is held to the bound of (t + 1) k iterations"""
    _env(monkeypatch, {})
    B, T, k = 400, 3, 2
    wl = f32_exact(workloads.talos_c4(B, T, model=talos))
    steps = [tuple(np.asarray(x, dtype=np.float32).astype(np.float64) for x in st) for st in wl["steps"]]
    link = int(wl["c_ids"][0])
    prm = dict(wl["params"], max_iter=k + 1, tol_abs=0.0, tol_rel=1e-30, tol_primal_inf=0.0)
    assert prm["warm_start"]
    s = loik_amd.BatchedLoik(talos, B, precision=capi.F32, **prm)
    s.SolveInit(*_args(wl))
    idx = np.arange(0, B, 2)
    refs = []
    for b in idx:
        r = ref.RefSolver(talos, **prm)
        r.SolveInit(*problem_args(wl, b))
        refs.append(r)
    border = np.zeros(idx.size, dtype=bool)   # (a borderline decision carries over to the later steps: the state is warm)
    for t, (q_t, b_t) in enumerate(steps):
        s.Solve(q_t, link, wl["Ais"][0], b_t[:, 0])
        assert np.all(s.get("iter") == k)
        got = {n: s.get(n) for n in FIELDS + SCALARS}
        got["His"] = s.His_full()
        want = {}
        for j, (b, r) in enumerate(zip(idx, refs)):
            r.Solve(q_t[b], link, wl["Ais"][0], b_t[b, 0])
            border[j] |= borderline(r)
            for n, x in _oracle_state(r, talos).items():
                want.setdefault(n, np.empty((idx.size,) + np.shape(x)))[j] = x
        late = None if (t + 1) * k <= EARLY else np.abs(np.log(np.asarray(got["mu"])[idx] / want["mu"])) > 1e-3
        assert_within_bound(got, want, idx, (t + 1) * k, "warm-started step %d" % t, border=border, late=late)
    assert s.stats()["lean_launches"] >= 1
    _no_flat(s)
    s.close()


# ---- 5. the fp32 accuracy contract beyond Panda-7 --------------------------------------------------------------------------------------

def _contract_problem(robot, talos):
    if robot == "talos32":
        wl = workloads.talos_c3(4096, seed=71, model=talos)
    elif robot == "talos44_wholebody":
        wl = workloads.talos_wholebody(2048, seed=72)
    else:
        m = random_tree_multidof(5, 20, root_freeflyer=True, n_spherical=1, n_translation=1, n_zyx=1, n_planar=1, n_rub=1, n_rubu=1)
        wl = workloads.make_workload(m, 2048, m.njoints - 1, 73, bound=0.5, snap_prob=0.0, nu_scale=0.4)
        wl["model"], wl["params"] = m, dict(workloads.FIXTURE_PARAMS, max_iter=1000)
    wl = f32_exact(wl)
    return wl["model"], wl, dict(wl["params"], tol_abs=1e-3, tol_rel=0.0)


CONTRACT_PINS = {"talos32": (8e-3, 0.02), "talos44_wholebody": (8e-3, 0.06), "multidof": (3e-3, 0.02)}   # (p99 of |dz|_inf, flag share)


@pytest.mark.parametrize("robot", ["talos32", "talos44_wholebody", "multidof"])
def test_fp32_accuracy_contract(robot, talos, monkeypatch):
    """LOIKB_OPT_F32_ACCURATE's contract (include/loik_amd.h: |z_f32 - z_f64|_inf <= tol_abs for 99 % of the instances that converge in
    both, tol_abs = 1e-3) beyond Panda-7, for the option and for the default fp32 handle: it does not hold there, and what does is pinned"""
    _env(monkeypatch, {})
    model, wl, prm = _contract_problem(robot, talos)
    B, tol = wl["q"].shape[0], prm["tol_abs"]
    out = ref.solve_batch(model, *_args(wl), nthreads=16, **prm)
    rows = {}
    for name, flags in (("default", 0), ("accurate", capi.OPT_F32_ACCURATE)):
        s = loik_amd.BatchedLoik(model, B, precision=capi.F32, flags=flags, **prm)
        s.Solve(*_args(wl))
        st = s.stats()
        assert st["lean_launches"] >= 1 and st["flat_launches"] == 0, (name, s.plan(), st)
        z, nu = s.get("z"), s.get("nu")
        c32, i32 = s.get("converged").astype(bool), s.get("primal_infeasible").astype(bool)
        both = c32 & out["converged"]
        dz = np.abs(z - out["z"]).max(axis=1)[both]
        rows[name] = dict(median=float(np.median(dz)), p99=float(np.quantile(dz, 0.99)), max=float(dz.max()), share=float(both.mean()),
                          conv_mismatch=float((c32 != out["converged"]).mean()), inf_mismatch=float((i32 != out["primal_infeasible"]).mean()))
        print("%s %s: %s" % (robot, name, rows[name]))
        if os.environ.get("LOIKB_TEST_MARGINS"):
            with open(os.environ["LOIKB_TEST_MARGINS"], "a") as f:
                f.write("contract %s %s %s\n" % (robot, name, rows[name]))
        assert both.mean() > 0.5, rows[name]
        # The header's contract (p99 <= tol_abs) holds on Panda-7 only (test_gpu_parity.test_c5_fp32_accuracy_contract).  Measured here on
        # an MI355X, the same for both handles (more than 16 joints: k_lean either way): p99 5.7e-3 (Talos-32), 5.0e-3 (whole body),
        # 2.0e-3 (multi-DoF tree); converged / infeasible flags differ on 1.9 / 1.6 %, 4.1 / 3.6 %, 0.05 / 0 %.  Pinned, and the header
        # says so: a change of either path shows.
        p99_pin, flag_pin = CONTRACT_PINS[robot]
        assert rows[name]["p99"] <= p99_pin, (name, rows[name])
        assert rows[name]["conv_mismatch"] < flag_pin and rows[name]["inf_mismatch"] < flag_pin, (name, rows[name])
        assert np.all(z <= wl["ub"] + 1e-6) and np.all(z >= wl["lb"] - 1e-6)
        assert np.abs(nu - z)[c32].max() < tol                                   # the slack closed
        for c, l in enumerate(wl["c_ids"]):                                      # the task met
            A = wl["Ais"][c] if np.asarray(wl["Ais"]).ndim == 3 else wl["Ais"][:, c]
            v = workloads.link_velocity(model, wl["q"], nu, int(l))
            Av = np.einsum("ij,bj->bi", A, v) if A.ndim == 2 else np.einsum("bij,bj->bi", A, v)
            assert np.abs(Av - wl["bis"][:, c])[c32].max() < 2 * tol, (name, c, np.abs(Av - wl["bis"][:, c])[c32].max())
        s.close()
