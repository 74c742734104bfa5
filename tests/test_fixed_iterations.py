"""LOIKB_OPT_FIXED_ITERS (include/loik_amd.h): exactly max_iter - 1 ADMM iterations, mu frozen at the solve's start value, no stopping logic --
on every route a solve can take.  Each engine has its own fixed-mode branch (k_flat2, k_flat, k_lean, k_tail, k_solve, k_pass_solve) and the
planner changes its decisions for the flag (one decade, no ordering / slicing / adaptation, no compaction, no hand-over to k_tail), so every
route is run and proved by stats() / plan().

The oracle: the same entry point with max_iter = 1 (the solve's resets and start mu, no iteration), then max_iter - 1 bare iteration bodies
(oracle/loik_ref.c ref_iteration_body: no CheckConvergence, CheckFeasibility, tail solve or UpdateMu).  The tolerances are the fixture's
(1e-3 / 1e-3, 1e-2) with max_iter = 60, and each case first solves without the flag to show that the flag matters there: instances stop
early and mu moves."""
import json
import os

import numpy as np
import pytest

import loik_amd
from loik_amd import capi, workloads
from helpers import FIXTURE, assert_close, f32_exact, feasible_batch, helical_tree, multi_task_batch, normwise_error, problem_args
from oracle import ref

MAX_ITER = 60
FIELDS = ["z", "nu", "w", "vis", "fis", "g", "yis", "Aty", "Stf_plus_w", "primal_residual_vec", "dual_residual_vec"]
# the residuals and the norms every iteration body recomputes
SCALARS = ["primal_residual", "dual_residual", "primal_residual_task", "primal_residual_slack", "dual_residual_v", "dual_residual_nu",
           "delta_fis_inf_norm", "delta_yis_inf_norm", "delta_w_inf_norm", "delta_vis_inf_norm", "delta_nu_inf_norm", "Av_inf_norm",
           "nu_inf_norm", "Href_v_inf_norm", "g_inf_norm", "Stf_plus_w_inf_norm"]
# what only the stopping logic sets -- CheckConvergence's tolerances, CheckFeasibility's certificate, the tail solve's count: not
# evaluated in fixed mode, so every instance on every route reports the solve's reset values, 0 (include/loik_amd.h, FIXED_ITERS).
UNEVALUATED = ["tol_primal", "tol_dual", "tail_solve_iter"]
# (the certificate's getters of the oracle recompute it from the current norms at every call, as upstream's debug getters do: the
#  library's report the values of the last CheckFeasibility, which a fixed solve never runs -- compared with 0, not with the oracle)
CERTIFICATE = ["delta_y_qp_inf_norm", "A_qp_T_delta_y_qp_inf_norm", "ub_qp_T_delta_y_qp_plus", "lb_qp_T_delta_y_qp_minus",
               "primal_infeasibility_cond_1", "primal_infeasibility_cond_2"]
ENV_KEYS = ("LOIKB_LEAN", "LOIKB_FLAT", "LOIKB_FLAT_SPLIT")
MU_RULES = {"default": 0, "osqp": 1, "maxeig": 3, "strat2": 2}   # (2: no such rule -- fixed mode applies none, so it is accepted)

_MODELS = {}


def _model(name):
    if name not in _MODELS:
        if name in ("talos32", "talos44", "panda7"):
            _MODELS[name] = loik_amd.builtin_model(name)
        elif name == "bushy42":
            from test_bushy_trees import bushy_tree
            _MODELS[name] = bushy_tree(77, 42, 2, 10)
        elif name == "bushy100":
            from test_bushy_trees import bushy_tree
            _MODELS[name] = bushy_tree(77, 100, 3, 9)
        else:
            _MODELS[name] = helical_tree(21, 24, 5)
    return _MODELS[name]


def _workload(robot, B, seed):
    """(workload, params) of a robot's problems"""
    m = _model(robot)
    if robot == "talos44":
        return workloads.talos_wholebody(B, seed=seed, model=m), dict(FIXTURE, num_eq_c=4)
    if robot == "panda7":
        return feasible_batch(m, B, m.njoints - 1, seed, bound=1.0, nu_scale=0.8), dict(FIXTURE)
    if robot == "talos32":
        return feasible_batch(m, B, m.getJointId("arm_left_7_joint"), seed, nu_scale=0.5), dict(FIXTURE)
    return multi_task_batch(m, B, [m.njoints - 1], seed, nu_scale=0.3), dict(FIXTURE)


def _flat2(s, st, B, n):
    assert "k_flat2" in s.plan() and st["flat_split_launches"] >= 1 and st["tail_instances"] == B, (s.plan(), st)


def _flat1(s, st, B, n):
    assert "k_flat1" in s.plan() and st["flat_launches"] >= 1 and st["tail_instances"] == B, (s.plan(), st)


def _osqp_off_flat(s, st, B):
    """OSQP's rule is k_flat2's / k_flat1's only: one lane per joint and k_lean leave such a solve to k_solve / k_tail"""
    assert "OSQP penalty rule" in s.plan() and st["flat_launches"] == 0 and st["lean_launches"] == 0, (s.plan(), st)


def _flat_one_lane(s, st, B, n):
    if "OSQP" in s.plan():
        return _osqp_off_flat(s, st, B)
    if B < 64:   # (a small batch: k_flat's plan, the short sequence of the one-instance-per-wavefront engines)
        assert "k_flat " in s.plan() and st["tail_instances"] == B, (s.plan(), st)
        return
    assert st["flat_launches"] >= 1 and st["flat_split_launches"] == 0 and st["tail_instances"] == B, (s.plan(), st)


def _lean(s, st, B, n):
    if "OSQP" in s.plan():
        return _osqp_off_flat(s, st, B)
    if B < 64:   # (a small batch: k_lean's plan, the short sequence of the one-instance-per-wavefront engines)
        assert "k_lean" in s.plan() and st["tail_instances"] == B, (s.plan(), st)
        return
    assert st["lean_launches"] >= 1 and st["flat_launches"] == 0 and st["tail_instances"] == B, (s.plan(), st)


def _tail(s, st, B, n):
    assert st["lean_launches"] == 0 and st["flat_launches"] == 0 and st["tail_instances"] == B, (s.plan(), st)


def _solve(s, st, B, n):
    assert st["lean_launches"] == 0 and st["flat_launches"] == 0 and st["tail_instances"] == 0, (s.plan(), st)
    assert "k_pass_solve" not in s.plan(), s.plan()


def _solve_launches(s, st, B, n):   # (launches of 3 iterations: boundaries in the middle of the count, no hand-over to k_tail)
    _solve(s, st, B, n)
    assert st["launches"] >= -(-n // 3), (n, st)


def _pass(s, st, B, n):
    assert "k_pass_solve" in s.plan() and st["tail_instances"] == 0 and st["launches"] == 1, (s.plan(), st)


def _on_chip(s, st, B, n):
    assert "too bushy for k_solve" in s.plan() and "whole batches go to the on-chip engines" in s.plan(), s.plan()
    assert st["tail_instances"] == B and st["launches"] >= 1, (s.plan(), st)


# route -> (robot, env, handle keywords, H_ref override, check(s, stats, B, iterations))
ROUTES = {
    "flat2": ("talos32", {}, {}, None, _flat2),
    "flat1": ("talos44", {}, {}, None, _flat1),
    "flat_one_lane": ("talos32", dict(LOIKB_FLAT_SPLIT="0"), {}, 2.0 * np.eye(6), _flat_one_lane),
    "lean": ("talos32", dict(LOIKB_FLAT="0"), {}, None, _lean),
    "tail": ("talos32", dict(LOIKB_LEAN="0"), dict(tail_max_instances=1 << 20), None, _tail),
    "solve": ("talos32", {}, dict(tail_max_instances=-1), None, _solve),
    "solve_launches": ("talos32", {}, dict(max_launch_iters=3), None, _solve_launches),
    "panda7": ("panda7", {}, {}, None, _tail),
    "helical_solve": ("helical", {}, dict(tail_max_instances=-1), None, _solve),
    "bushy_on_chip": ("bushy42", {}, {}, None, _on_chip),
    "bushy_pass": ("bushy42", {}, dict(flags=capi.OPT_NO_H_CACHE), None, _pass),
    "over_64_joints": ("bushy100", {}, {}, None, _pass),
    "logged": ("talos32", {}, dict(logging=True), None, _pass),
}
ENTRIES = ["full", "split", "tailored"]
BATCHES = [1, 130, 4096]


def _pairwise():
    """every (route, mu rule) pair once; entry point and batch size rotate so that every pair of any two of the four factors occurs"""
    out = []
    for i, r in enumerate(ROUTES):
        for j, mu in enumerate(MU_RULES):
            out.append((r, mu, ENTRIES[(i + j) % 3], BATCHES[(i + 2 * j) % 3]))
    return out


def _handle(monkeypatch, route, B, prm, fixed=True):
    robot, env, kw, _, _ = ROUTES[route]
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(kw)
    kw["flags"] = kw.get("flags", 0) | (capi.OPT_FIXED_ITERS if fixed else 0)
    return loik_amd.BatchedLoik(_model(robot), B, **prm, **kw)


def _problems_of(robot, B, n, href=None):
    wls = []
    for t in range(n):
        wl, prm = _workload(robot, B, 31 + 7 * t)
        if href is not None:
            wl["H_ref"] = href
        wls.append(wl)
    return wls, prm


def _problems(route, B, entry):
    """the workloads of a case: one, or the targets of a warm-started tailored sequence"""
    robot, _, _, href, _ = ROUTES[route]
    return _problems_of(robot, B, 2 if entry == "tailored" else 1, href)


def _run(s, wls, entry, link):
    """the entry point on the device; yields after each solve"""
    args = lambda wl: (wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])
    if entry == "full":
        s.Solve(*args(wls[0])); yield 0
    elif entry == "split":
        s.SolveInit(*args(wls[0])); s.Solve(); yield 0
    else:
        s.SolveInit(*args(wls[0]))
        for t, wl in enumerate(wls):
            s.Solve(wl["q"], link, wl["Ais"][0], wl["bis"][:, 0]); yield t


def _oracle(model, prm, wls, entry, b, link, n):
    """RefSolver after each solve of the sequence: the entry point's resets and start mu (max_iter = 1: no iteration), then n bare
    iteration bodies"""
    r = ref.RefSolver(model, **dict(prm, max_iter=1))
    if entry == "split":
        r.SolveInit(*problem_args(wls[0], b)); r.Solve()
    elif entry == "full":
        r.Solve(*problem_args(wls[0], b))
    else:
        r.SolveInit(*problem_args(wls[0], b))
    for t, wl in enumerate(wls):
        if entry == "tailored":
            r.Solve(wl["q"][b], link, np.asarray(wl["Ais"])[0], wl["bis"][b, 0])
        mu0 = r.scalar("mu")
        for _ in range(n):
            r.IterationBody()
        yield r, mu0


def _check_fixed(s, model, prm, wls, entry, link, stride, check_route=None, logged=False):
    B = wls[0]["q"].shape[0]
    n = prm["max_iter"] - 1
    idx = list(range(0, B, stride)) + ([B - 1] if (B - 1) % stride else [])
    oracles = {b: _oracle(model, prm, wls, entry, b, link, n) for b in idx}
    for t in _run(s, wls, entry, link):
        st = s.stats()
        if check_route is not None:
            check_route(s, st, B, n)
        it = s.get("iter")
        assert np.all(it == n), (t, np.unique(it))
        assert st["instance_iterations"] == B * n, (t, st["instance_iterations"], B * n)
        assert st["n_unfinished"] == B, st   # (neither converged nor flagged: every instance stopped at max_iter)
        assert not np.any(s.get("converged")) and not np.any(s.get("primal_infeasible")), t
        got = {k: s.get(k) for k in FIELDS + SCALARS + UNEVALUATED + CERTIFICATE + ["mu", "mu_eq", "mu_ineq"]}
        for k in UNEVALUATED + CERTIFICATE:
            assert np.all(got[k] == 0), (t, k, np.flatnonzero(got[k] != 0)[:10], np.unique(got[k])[:5])
        info = s.solver_info() if logged else None
        for b in idx:
            r, mu0 = next(oracles[b])
            assert got["mu"][b] == mu0, (t, b, got["mu"][b], mu0)   # frozen at the start value, exactly
            if n > 0:   # (mu_eq / mu_ineq and the residual vectors of the last iteration: none ran)
                assert_close(got["mu_eq"][b], prm["mu_equality_scale_factor"] * mu0, 1e-12, "mu_eq")
                assert got["mu_ineq"][b] == mu0
            for k in FIELDS if n > 0 else FIELDS[:-2]:
                want = r.field(k)
                if k in ("vis", "fis", "g"):
                    want = want[1:]
                assert_close(got[k][b], want, 1e-9, "%s t%d b%d" % (k, t, b))
            for k in SCALARS + UNEVALUATED:
                assert_close(got[k][b], r.scalar(k), 1e-9, "%s t%d b%d" % (k, t, b))
            if logged and n > 0:
                assert info["rows"][b] == n, (b, info["rows"][b])
                assert np.all(info["mu_list"][b, :n] == mu0)
                assert_close(info["primal_residual_list"][b, n - 1], r.scalar("primal_residual"), 1e-9, "logged primal")
                assert_close(info["dual_residual_list"][b, n - 1], r.scalar("dual_residual"), 1e-9, "logged dual")
        if logged:
            assert np.all(info["rows"] == n), np.unique(info["rows"])



def test_pairwise_cases_cover_every_pair():
    cases = _pairwise()
    factors = [list(ROUTES), list(MU_RULES), ENTRIES, BATCHES]
    for a in range(4):
        for b in range(a + 1, 4):
            seen = {(c[a], c[b]) for c in cases}
            assert len(seen) == len(factors[a]) * len(factors[b]), (a, b)


@pytest.mark.parametrize("robot", ["talos32", "talos44", "panda7", "helical", "bushy42", "bushy100"])
def test_oracle_tolerances_make_the_flag_matter(robot):
    """CPU: with the fixture's tolerances the oracle's own solves stop early and move mu on every robot of the routes, and its fixed
    construction (an entry point with max_iter = 1, then bare iteration bodies) is another solve -- for all three entry points"""
    wls, prm = _problems_of(robot, 12, 2)
    prm = dict(prm, max_iter=MAX_ITER, warm_start=True)
    wl = wls[0]
    out = ref.solve_batch(_model(robot), wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"],
                          nthreads=4, **dict(prm, warm_start=False))
    assert np.any(out["iters"] < MAX_ITER - 1), out["iters"]
    link = int(wl["c_ids"][0])
    zs = {}
    for entry in ENTRIES:
        rs = list(_oracle(_model(robot), prm, wls if entry == "tailored" else wls[:1], entry, 3, link, MAX_ITER - 1))
        zs[entry] = rs[0][0].z.copy() if entry != "tailored" else None
        assert all(r.scalar("mu") == mu0 for r, mu0 in rs)
    assert np.array_equal(zs["full"], zs["split"])
    r = ref.RefSolver(_model(robot), **dict(prm, warm_start=False))
    r.Solve(*problem_args(wl, 3))
    assert r.get_iter() < MAX_ITER - 1 or r.scalar("mu") != prm["mu"], "instance 3 neither stops early nor moves mu"
    assert np.abs(r.z - zs["full"]).max() > 1e-12

@pytest.mark.gpu
@pytest.mark.parametrize("route,mu,entry,B", _pairwise())
def test_fixed_iterations_on_every_route(route, mu, entry, B, monkeypatch):
    robot = ROUTES[route][0]
    model = _model(robot)
    wls, prm = _problems(route, B, entry)
    prm = dict(prm, max_iter=MAX_ITER, mu_update_strat=MU_RULES[mu], warm_start=entry == "tailored")
    link = int(wls[0]["c_ids"][0])
    # precondition: without the flag (same handle settings; rule 2 does not exist outside fixed mode -> DEFAULT's), instances of this
    # route stop early and mu moves -- an engine that ignored the flag would be seen
    pre_wls, _ = _problems(route, 130, "full")
    pre = _handle(monkeypatch, route, 130, dict(prm, mu_update_strat=0 if mu == "strat2" else prm["mu_update_strat"], warm_start=False),
                  fixed=False)
    next(_run(pre, pre_wls, "full", link))
    mu0 = next(_oracle(model, dict(prm, warm_start=False), pre_wls, "full", 0, link, 0))[1]   # (the start mu: H_ref is the batch's)
    it, mus = pre.get("iter"), pre.get("mu")
    assert np.any(it < MAX_ITER - 1) and np.any(mus != mu0), (route, mu, np.unique(it), mu0, np.unique(mus))
    pre.close()
    s = _handle(monkeypatch, route, B, prm)
    _check_fixed(s, model, prm, wls, entry, link, stride=17 if B > 1 else 1, check_route=ROUTES[route][4], logged=route == "logged")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [1, 2])
@pytest.mark.parametrize("route", list(ROUTES))
def test_fixed_iterations_edges(route, max_iter, monkeypatch):
    """max_iter = 1: no iteration -- the state is SolveInit's (the engines' guard at entry); max_iter = 2: one iteration"""
    robot = ROUTES[route][0]
    wls, prm = _problems(route, 130, "full")
    prm = dict(prm, max_iter=max_iter)
    s = _handle(monkeypatch, route, 130, prm)
    _check_fixed(s, _model(robot), prm, wls, "full", int(wls[0]["c_ids"][0]), stride=13, logged=route == "logged")
    if max_iter == 2:
        ROUTES[route][4](s, s.stats(), 130, 1)
    s.close()


# ---- fp32: the float builds of k_lean, k_tail and k_solve against the fp64 oracle, inputs rounded to fp32 ----------------------------------
# Bounds: ten times what each case measured on an MI355X (tests/golden/fixed_iterations_fp32_measured.json, {case: {field: max}}).
# LOIKB_FIXED_FP32_MEASURE=<file> re-measures: nothing is asserted, each (case, field, max) is appended to <file> as a JSON line.
# mu is frozen: no instance can follow another penalty trajectory, none is left out.
# The k_lean and k_tail rows of a robot are equal because the two engines return the same bits in fixed mode: on these inputs (B = 130,
# seed 57, max_iter = 60) z, nu, w, vis, fis, yis, iter and mu of every instance were bitwise equal on an MI355X, Talos-32 and Panda-7
# (k_lean with OPT_F32_ACCURATE) alike -- one decade, so k_lean's precomputed H of mu0 is the H k_tail builds -- while the same solves
# with the adaptive rule differ (Talos-32 |dz| up to 9.8e-2, 41 iterations).  k_solve's rows, another summation order, differ.
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fixed_iterations_fp32_measured.json")) as _f:
    MEASURED32 = json.load(_f)
FIELDS32 = ["z", "nu", "w", "vis", "fis", "yis", "primal_residual", "dual_residual", "mu"]
UNIT_SCALE32 = ("w", "primal_residual", "dual_residual")   # (small differences of O(1) terms: against the problem's unit scale)
ENGINES32 = {
    "lean-talos32": ("talos32", {}, {}, lambda st, B: st["lean_launches"] >= 1 and st["tail_instances"] == B),
    "lean-panda7": ("panda7", {}, dict(flags=capi.OPT_F32_ACCURATE), lambda st, B: st["lean_launches"] >= 1 and st["tail_instances"] == B),
    "tail-talos32": ("talos32", dict(LOIKB_LEAN="0"), dict(tail_max_instances=1 << 20), lambda st, B: st["lean_launches"] == 0 and st["tail_instances"] == B),
    "tail-panda7": ("panda7", {}, {}, lambda st, B: st["lean_launches"] == 0 and st["tail_instances"] == B),
    "solve-talos32": ("talos32", {}, dict(tail_max_instances=-1), lambda st, B: st["lean_launches"] == 0 and st["tail_instances"] == 0),
    "solve-panda7": ("panda7", {}, dict(tail_max_instances=-1), lambda st, B: st["lean_launches"] == 0 and st["tail_instances"] == 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("engine", list(ENGINES32))
def test_fixed_iterations_fp32(engine, monkeypatch):
    robot, env, kw, check = ENGINES32[engine]
    model = _model(robot)
    B = 130
    wl, prm = _workload(robot, B, 57)
    wl = f32_exact(wl)
    prm = dict(prm, max_iter=MAX_ITER)
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(kw)
    kw["flags"] = kw.get("flags", 0) | capi.OPT_FIXED_ITERS
    s = loik_amd.BatchedLoik(model, B, precision=capi.F32, **prm, **kw)
    s.Solve(wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])
    st = s.stats()
    assert check(st, B) and st["flat_launches"] == 0, (s.plan(), st)
    n = MAX_ITER - 1
    assert np.all(s.get("iter") == n) and st["instance_iterations"] == B * n, st
    assert not np.any(s.get("converged")) and not np.any(s.get("primal_infeasible"))
    got = {k: s.get(k) for k in FIELDS32}
    idx = np.arange(0, B, 13)
    want = {k: [] for k in FIELDS32}
    for b in idx:
        r = next(_oracle(model, prm, [wl], "full", b, None, n))[0]
        for k in FIELDS32:
            v = r.field(k) if k in ("z", "nu", "w", "vis", "fis", "yis") else r.scalar(k)
            want[k].append(v[1:] if k in ("vis", "fis") else v)
    bad = []
    for k in FIELDS32:
        floor = 1.0 if k in UNIT_SCALE32 else 1e-300 if k == "mu" else 1e-6
        err = normwise_error(np.asarray(got[k])[idx].reshape(idx.size, -1), np.asarray(want[k]).reshape(idx.size, -1), floor)
        if os.environ.get("LOIKB_FIXED_FP32_MEASURE"):
            with open(os.environ["LOIKB_FIXED_FP32_MEASURE"], "a") as f:
                f.write(json.dumps([engine, k, float(err.max())]) + "\n")
            continue
        meas = MEASURED32.get(engine, {}).get(k)
        assert meas is not None, (engine, k, "no measurement in tests/golden/fixed_iterations_fp32_measured.json")
        if err.max() > max(10.0 * meas, 4 * n * 2.0 ** -24):
            bad.append((k, float(err.max()), meas))
    assert not bad, (engine, bad)
    s.close()
