"""GPU: joint position limits in the pose loop (include/loik_amd_limits.h) against the lock-step CPU oracle with limits
(tests/pose_limits_numpy.py, proven on the CPU by tests/test_pose_limits_oracle.py), and loikb_update_ineq_constraints.
The parity gate is tests/test_pose_parity.py's: on the oracle's strided subset, the same reached / steps on >= 99 % of the
instances, |dq| < 1e-7 on those.  Every parity workload is built so that the limits bind, which is asserted on the ORACLE's
output (_assert_binds): >= 25 % of the instances with a nonzero limit flag, >= 25 % with none, >= 10 % reached, >= 10 % not."""
import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from helpers import FIXTURE, assert_end_to_end, feasible_batch, fetch_end_to_end
from test_engines import ENGINES
from test_pose_ik import BOUND, PRM, _fk_models, _links
from test_pose_parity import ENGINE_ENV, _box, _gate, _handle, _leaf_and_multidof, _nonsym_A, _seeds, _subset
import pose_numpy as P
import pose_limits_numpy as PL

pytestmark = pytest.mark.gpu

TOL = 1e-4
LAWS = [(0.25, 0.5), (2.0, 1.7)]   # (dt, gain) as in test_pose_parity.LAW_CASES
SPREAD = (1e-7, 0.15)              # seeds this far from their targets, log-uniform: about half start within tol_pose


def _workload(name, nc, B, a_inst, box_inst, pct, seed):
    """seeds and targets as test_pose_parity._seeds makes them, limits and in-range seeds by pose_limits_numpy.binding_limits,
    A non-symmetric (shared or per instance), the base box BOUND (shared) or a seeded [B][nv] box in [0.5, 2] BOUND"""
    if name == "multidof":
        model = _fk_models()[3]   # free-flyer root (no limit possible), a translation joint and two ZYX joints (limited)
        links = _leaf_and_multidof(model)
    else:
        model = loik_amd.builtin_model(name)
        links = _links(model, nc)
    rng = np.random.default_rng(seed)
    A = _nonsym_A(rng, len(links), B if a_inst else None)
    q0, tg = _seeds(model, B, links, seed=seed + 1, spread=SPREAD)
    q_t = model.random_configurations(np.random.default_rng(seed + 1), B)   # (what _seeds drew the targets from)
    q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, seed + 2, pct)
    if box_inst:
        w = rng.uniform(0.5, 2.0, size=(2, B, model.nv)) * BOUND
        box = (-w[0], w[1])
    else:
        box = _box(model)
    return dict(model=model, links=links, A=A, q0=q0, tg=tg, q_lo=q_lo, q_hi=q_hi, box=box, B=B)


def _oracle(w, idx, dt, gain, k, prm=PRM):
    A, (lb, ub) = w["A"], w["box"]
    return PL.lockstep_pose_loop_limits(w["model"], prm, w["q0"][idx], np.eye(6), np.zeros(6), w["links"], A[idx] if A.ndim == 4 else A,
                                        lb[idx] if lb.ndim == 2 else lb, ub[idx] if ub.ndim == 2 else ub, w["tg"][idx], dt, gain, TOL, k,
                                        w["q_lo"], w["q_hi"])


def _assert_binds(o, what):
    """the conditions on the oracle's result that make a parity case mean something"""
    flagged = (o["limit_flags"] != 0).any(axis=1).mean()
    reached = o["reached"].mean()
    print("%s: oracle flagged %.3f reached %.3f steps %s" % (what, flagged, reached, np.bincount(o["steps"]).tolist()))
    assert flagged >= 0.25 and 1.0 - flagged >= 0.25, (what, flagged)
    assert reached >= 0.10 and 1.0 - reached >= 0.10, (what, reached)


def _limited(w):
    qi = PL.limit_q_index(w["model"])
    lim = np.isfinite(w["q_lo"]) | np.isfinite(w["q_hi"])
    return qi[lim], w["q_lo"][lim], w["q_hi"][lim]


def _assert_contained(w, q, what):
    ci, lo, hi = _limited(w)
    assert np.all(lo <= q[:, ci]) and np.all(q[:, ci] <= hi), (what, float(np.maximum(lo - q[:, ci], q[:, ci] - hi).max()))


def _solve(w, dt, gain, k, prm=PRM, precision=capi.F64, limits=True, **kw):
    s = _handle(w["model"], w["B"], w["links"], w["q0"], w["A"], prm, precision=precision, box=w["box"], **kw)
    if limits:
        s.set_joint_limits(w["q_lo"], w["q_hi"])
    out = s.SolvePose(w["tg"], dt=dt, gain=gain, tol_pose=TOL, max_steps=k)
    return s, out, s.get("q")


# ---- 1. parity with the lock-step oracle ---------------------------------------------------------------------------------------
PARITY = [
    # (robot, nc, B, A per instance, base box per instance, percentiles of the limits, seed)
    ("talos32", 1, 193, False, False, (2.0, 98.0), 1100),
    ("talos32", 2, 256, True, True, (2.0, 98.0), 1200),
    ("panda7", 1, 193, False, False, (5.0, 95.0), 1300),
    ("multidof", 2, 193, True, False, (5.0, 95.0), 1400),
]


@pytest.mark.parametrize("law", LAWS, ids=lambda l: "dt%g-g%g" % l)
@pytest.mark.parametrize("case", PARITY, ids=lambda c: "%s-nc%d-B%d-%s-%s" % (c[0], c[1], c[2], "Ainst" if c[3] else "Ash", "boxinst" if c[4] else "boxsh"))
def test_limits_match_lockstep_oracle(case, law):
    w = _workload(*case)
    dt, gain = law
    idx = _subset(w["B"])
    for k in (1, 4):
        s, out, q = _solve(w, dt, gain, k)
        s.close()
        o = _oracle(w, idx, dt, gain, k)
        _assert_binds(o, (case, law, k))
        same = _gate(out, q, o, idx, (case, law, k))
        _assert_contained(w, q, (case, law, k))
        # (a flag is a comparison of two numbers that differ by the parity gate's 1e-7 at most between device and oracle)
        assert (out["limit_flags"][idx][same] != o["limit_flags"][same]).any(axis=1).mean() <= 0.01, (case, law, k)
        assert np.array_equal(out["status"][idx][same] & 9, o["status"][same] & 9)
        if case[0] == "multidof":   # the free-flyer carries no limit and moves; a translation / ZYX coordinate is limited
            m = w["model"]
            jt = [int(t) for t in m.jtype]
            ff = jt.index(9)
            assert not np.isfinite(w["q_lo"][int(m.idx_v[ff]):int(m.idx_v[ff]) + 6]).any()
            multi_v = [int(m.idx_v[i]) + d for i in range(1, m.njoints) if jt[i] in (11, 12) for d in range(3)]
            assert np.isfinite(w["q_lo"][multi_v]).any()


@pytest.mark.parametrize("law", LAWS, ids=lambda l: "dt%g-g%g" % l)
def test_single_instance_matches_lockstep_oracle(law):
    """B = 1 (fractions of a batch mean nothing here: the instance is one whose limits bind in the B = 193 oracle run)"""
    big = _workload("talos32", 1, 193, False, False, (2.0, 98.0), 1100)
    dt, gain = law
    ob = _oracle(big, np.arange(193), dt, gain, 4)
    pick = np.flatnonzero((ob["limit_flags"] != 0).any(axis=1) & (ob["steps"] == 4))
    assert pick.size
    b = int(pick[0])
    w = dict(big, B=1, q0=big["q0"][b:b + 1], tg=big["tg"][b:b + 1])
    for k in (1, 4):
        s, out, q = _solve(w, dt, gain, k)
        s.close()
        o = _oracle(w, np.arange(1), dt, gain, k)
        assert o["limit_flags"].any()
        assert out["reached"][0] == o["reached"][0] and out["steps"][0] == o["steps"][0]
        assert np.max(np.abs(q - o["q"])) < 1e-7
        assert np.array_equal(out["limit_flags"], o["limit_flags"])
        _assert_contained(w, q, (law, k))


# ---- 2. every engine: one that captured the box-sharing mode before the launch would solve with the base box --------------------
_ENGINE_CACHE = {}
ENGINE_LAW = (0.5, 0.5, 3)   # dt, gain, max_steps (gain 1 closes the error in one step: nine in ten reach, nothing left to rest on a limit)
ENGINE_RUNS = list(ENGINES) + ["chunks3"]


def _engine_problem():
    if not _ENGINE_CACHE:
        w = _workload("talos32", 2, 384, False, False, (2.0, 98.0), 1500)   # (six tiles: LOIKB_CHUNKS=3 gets three chunks of two)
        idx = _subset(w["B"])
        o = _oracle(w, idx, *ENGINE_LAW)
        _assert_binds(o, "engines")
        _ENGINE_CACHE.update(w=w, idx=idx, o=o)
    return _ENGINE_CACHE["w"], _ENGINE_CACHE["idx"], _ENGINE_CACHE["o"]


@pytest.mark.parametrize("engine", ENGINE_RUNS)
def test_every_engine_honours_the_step_box(engine, monkeypatch):
    w, idx, o = _engine_problem()
    for v in ENGINE_ENV:
        monkeypatch.delenv(v, raising=False)
    if engine == "chunks3":
        env, kw = dict(LOIKB_CHUNKS="3"), dict(compact_min_instances=128, max_launch_iters=5, tail_max_instances=900)
    else:
        env, kw = ENGINES[engine]
    for v, x in env.items():
        monkeypatch.setenv(v, x)
    s, out, q = _solve(w, *ENGINE_LAW, **kw)
    if engine == "chunks3":
        assert s.stats()["chunks"] == 3
    s.close()
    _gate(out, q, o, idx, engine)
    _assert_contained(w, q, engine)
    assert np.any(out["steps"] > 1)


# ---- 3. containment on a full batch, no oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
def test_containment_full_batch(precision):
    w = _workload("talos32", 1, 4096, False, False, (2.0, 98.0), 1600)
    _assert_contained(w, w["q0"], "seeds")
    s, out, q = _solve(w, 0.25, 0.5, 4, precision=precision)
    s.close()
    _assert_contained(w, q, precision)
    ci, lo, hi = _limited(w)
    moved = out["steps"] > 0
    assert moved.mean() > 0.25 and np.max(np.abs(q - w["q0"])) > 1e-3
    assert ((q[:, ci] == lo) | (q[:, ci] == hi)).any(axis=1).mean() > 0.25   # instances resting on a limit
    assert (out["limit_flags"] != 0).any(axis=1)[moved].any() and not out["limit_flags"][~moved].any()


def test_f32_handle_contains_and_flags_are_consistent():
    """an fp32 handle on panda7: containment (as the fp64 oracle has it) and flags consistent with the handle's OWN q; no fp32
    trajectory claim.  The flags are those of the box of the last step, computed from the q before it: lo > lb <=> q_prev - q_lo <
    dt BOUND, and the step moved the coordinate by dt BOUND at most.  So a limit farther than 2 dt BOUND from the final coordinate
    cannot be flagged, and a limit the final coordinate of a moved instance rests on must be."""
    w = _workload("panda7", 1, 193, False, False, (5.0, 95.0), 1300)
    dt, gain = 0.25, 0.5
    s, out, q = _solve(w, dt, gain, 4, precision=capi.F32)
    s.close()
    _assert_contained(w, q, "f32")
    o = _oracle(w, np.arange(w["B"]), dt, gain, 4)
    ci, lo, hi = _limited(w)
    assert np.all(lo <= o["q"][:, ci]) and np.all(o["q"][:, ci] <= hi)
    f = out["limit_flags"]
    lim = np.isfinite(w["q_lo"])
    assert not f[:, ~lim].any() and not f[out["steps"] == 0].any()
    # q_prev of the last step is within dt BOUND of the final q: lo > lb <=> q_prev - q_lo < dt BOUND
    qq = q[:, ci]
    far_lo, far_hi = qq - lo > 2.001 * dt * BOUND, hi - qq > 2.001 * dt * BOUND
    near_lo, near_hi = qq == lo, qq == hi
    fl = f[:, lim]
    assert not (fl[far_lo] & capi.LIMIT_LOWER).any() and not (fl[far_hi] & capi.LIMIT_UPPER).any()
    mv = (out["steps"] > 0)[:, None]
    assert np.all((fl & capi.LIMIT_LOWER)[near_lo & mv] != 0) and np.all((fl & capi.LIMIT_UPPER)[near_hi & mv] != 0)
    assert (fl != 0).any()


# ---- 4. no limits = today ------------------------------------------------------------------------------------------------------
def test_without_finite_limits_nothing_changes():
    w = _workload("talos32", 2, 256, True, True, (2.0, 98.0), 1700)
    inf = np.inf * np.ones(w["model"].nv)

    def run(mode):
        s = _handle(w["model"], w["B"], w["links"], w["q0"], w["A"], PRM, box=w["box"])
        if mode == "inf":
            s.set_joint_limits(-inf, inf)
        elif mode == "cleared":
            s.set_joint_limits(w["q_lo"], w["q_hi"])
            s.set_joint_limits(None, None)
        out = s.SolvePose(w["tg"], dt=0.5, gain=1.0, tol_pose=TOL, max_steps=3)
        res = dict(out, q=s.get("q"), z=s.get("z"), iter=s.get("iter"))
        if mode != "never":
            with pytest.raises(capi.LoikError) as e:
                s.pose_limit_flags()
            assert e.value.code == -24
        s.close()
        return res

    ref = run("never")
    assert set(ref) == {"reached", "steps", "err", "status", "q", "z", "iter"}
    for mode in ("inf", "cleared"):
        got = run(mode)
        assert set(got) == set(ref)
        for key in ref:
            assert np.array_equal(got[key], ref[key]), (mode, key)


# ---- 5. the base box is back in force afterwards ----------------------------------------------------------------------------------
def _plan_core(s):
    """plan() without the parts that record a handle's solve history (decades visited so far, buffer sizes): the engine plan"""
    import re
    return re.sub(r"; device buffers:.*?room\)", "", re.sub(r"; decades visited[^;]*", "", s.plan()))


@pytest.mark.parametrize("box_inst", [False, True], ids=["boxsh", "boxinst"])
def test_base_box_is_restored(box_inst):
    """after a SolvePose with limits the handle solves with its base box again, in the sharing mode it had: the same calls on it and
    on a twin whose SolvePose ran without limits, both put on the same q and started cold, give bit-identical z / iter -- with a b
    large enough that the base box binds (and dominates bis_inf_norm_, which keeps each handle's own history otherwise)"""
    w = _workload("talos32", 1, 256, False, box_inst, (2.0, 98.0), 1800)
    s = _handle(w["model"], w["B"], w["links"], w["q0"], w["A"], PRM, box=w["box"])
    s.set_joint_limits(w["q_lo"], w["q_hi"])
    plan0 = _plan_core(s)
    out = s.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=3)
    assert _plan_core(s) == plan0
    assert (out["limit_flags"] != 0).any() and np.any(out["steps"] == 3)
    q = s.get("q")
    t = _handle(w["model"], w["B"], w["links"], w["q0"], w["A"], PRM, box=w["box"])
    assert _plan_core(t) == plan0
    t.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=3)
    assert np.max(np.abs(t.get("q") - q)) > 1e-3
    rng = np.random.default_rng(5)
    b = rng.choice([-1.0, 1.0], size=(w["B"], 6)) * (3.0 + rng.random((w["B"], 6)))
    for h in (s, t):   # (s keeps its limits: the call that moves nothing enters and leaves the per-instance mode once more)
        h.set_warm_start(False)
        h.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=0, q=q)
        h.UpdateEqConstraint(w["links"][0], b)
        h.Solve(None, -1, None, None)
        h.Solve()
    zs, its = s.get("z"), s.get("iter")
    zt, itt = t.get("z"), t.get("iter")
    assert _plan_core(s) == _plan_core(t)
    s.close()
    t.close()
    assert np.array_equal(its, itt) and np.array_equal(zs, zt)
    lb, ub = w["box"]
    assert np.all(zs >= lb) and np.all(zs <= ub)
    assert ((zs == np.broadcast_to(lb, zs.shape)) | (zs == np.broadcast_to(ub, zs.shape))).any(), "the base box never binds: the test shows nothing"


# ---- 6. UpdateIneqConstraints ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared,device", [(True, False), (False, False), (False, True)], ids=["boxsh-host", "boxinst-host", "boxinst-device"])
def test_update_ineq_constraints_matches_solve_init(shared, device):
    """warm_start off: SolveInit(box1), UpdateIneqConstraints(box2), Solve() is the oracle's SolveInit(box2), Solve() (a shared box is a
    host array, as every shared input)"""
    from oracle import ref
    model = loik_amd.builtin_model("talos32")
    B = 192
    link = _links(model, 1)[0]
    wl = feasible_batch(model, B, link, seed=2100, bound=0.5, per_instance_bounds=not shared)
    rng = np.random.default_rng(2101)
    box1 = (wl["lb"], wl["ub"])
    if shared:
        box2 = (-0.08 * (1 + rng.random(model.nv)), 0.08 * (1 + rng.random(model.nv)))
    else:
        box2 = (-0.08 * (1 + rng.random((B, model.nv))), 0.08 * (1 + rng.random((B, model.nv))))
    prm = dict(FIXTURE, max_iter=200, warm_start=False)
    s = loik_amd.BatchedLoik(model, B, **prm)
    # the other sharing mode first: the update switches the mode as SolveInit would
    first = (box1[0][0], box1[1][0]) if not shared else (np.tile(box1[0], (B, 1)), np.tile(box1[1], (B, 1)))
    s.SolveInit(wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], *first)
    keep = [capi.DeviceArray(x) for x in box2] if device and not shared else None
    s.UpdateIneqConstraints(*(keep if keep else box2))
    s.Solve()
    got = fetch_end_to_end(s, residuals=True)
    out = ref.solve_batch(model, wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], box2[0], box2[1], nthreads=4, **prm)
    assert_end_to_end(got, out, prm, what="UpdateIneqConstraints %s %s" % (shared, device))
    z = got["z"]
    assert np.all(z >= box2[0] - 1e-12) and np.all(z <= box2[1] + 1e-12)
    assert (np.isclose(z, np.broadcast_to(box2[0], z.shape)) | np.isclose(z, np.broadcast_to(box2[1], z.shape))).mean() > 0.01
    s.close()


def test_update_ineq_constraints_errors():
    model = loik_amd.builtin_model("panda7")
    B = 8
    s = loik_amd.BatchedLoik(model, B, **FIXTURE)
    lb, ub = _box(model)
    with pytest.raises(capi.LoikError) as e:
        s.UpdateIneqConstraints(lb, ub)
    assert e.value.code == -24
    q0 = model.random_configurations(np.random.default_rng(0), B)
    s.SolveInit(q0, np.eye(6), np.zeros(6), np.array([7], dtype=np.int32), np.eye(6)[None], np.zeros((B, 1, 6)), lb, ub)
    with pytest.raises(capi.LoikError) as e:
        s.UpdateIneqConstraints(np.ones(model.nv + 1), np.ones(model.nv + 1))
    assert e.value.code == -3
    s.UpdateIneqConstraints(lb, ub)
    s.close()


# ---- 7. argument checking --------------------------------------------------------------------------------------------------------
def _err(fn, code):
    with pytest.raises(capi.LoikError) as e:
        fn()
    assert e.value.code == code, e.value
    return str(e.value)


def test_set_joint_limits_arguments():
    import ctypes as C
    model = _fk_models()[3]
    B = 4
    s = loik_amd.BatchedLoik(model, B, **FIXTURE)
    nv = model.nv
    inf = np.inf * np.ones(nv)
    qi = PL.limit_q_index(model)
    ok = int(np.flatnonzero(qi >= 0)[0])
    lo, hi = -inf.copy(), inf.copy()
    lo[ok], hi[ok] = -0.5, 0.5
    s.set_joint_limits(lo, hi)            # accepted; one-sided as well
    hi[ok] = np.inf
    s.set_joint_limits(lo, hi)
    _err(lambda: s.set_joint_limits(-np.inf * np.ones(nv + 1), np.inf * np.ones(nv + 1)), -20)
    bad = lo.copy(); bad[ok] = np.nan
    assert "DoF %d" % ok in _err(lambda: s.set_joint_limits(bad, hi), -20)
    bad = lo.copy(); bad[ok] = 1.0
    hi2 = hi.copy(); hi2[ok] = 0.5
    assert "DoF %d" % ok in _err(lambda: s.set_joint_limits(bad, hi2), -20)
    one = np.ascontiguousarray(lo)
    assert s.L.loikb_set_joint_limits(s.h, one.ctypes.data_as(C.POINTER(C.c_double)), None, nv) == -20
    assert s.L.loikb_set_joint_limits(s.h, None, one.ctypes.data_as(C.POINTER(C.c_double)), nv) == -20
    # every kind of DoF that cannot carry a limit is refused, by name
    jt = [int(t) for t in model.jtype]
    kinds = {9: "free-flyer", 13: "planar", 14: "unbounded", 15: "unbounded", 16: "unbounded", 18: "unbounded", 10: "spherical"}
    seen = set()
    for i in range(1, model.njoints):
        if jt[i] in kinds:
            v = int(model.idx_v[i])
            bad = -inf.copy(); bad[v] = -1.0
            msg = _err(lambda: s.set_joint_limits(bad, inf), -20)
            assert "DoF %d" % v in msg and "joint %d" % i in msg and kinds[jt[i]] in msg, msg
            seen.add(kinds[jt[i]])
    assert {"free-flyer", "planar", "unbounded"} <= seen
    # a rejected call leaves the limits that were in force; the flags getter needs a pose solve with limits
    _err(lambda: s.pose_limit_flags(), -24)
    s.close()
    sph = _fk_models()[2]
    s = loik_amd.BatchedLoik(sph, B, **FIXTURE)
    i = [int(t) for t in sph.jtype].index(10)
    bad = -np.inf * np.ones(sph.nv); bad[int(sph.idx_v[i]) + 1] = 0.0
    assert "spherical" in _err(lambda: s.set_joint_limits(bad, np.inf * np.ones(sph.nv)), -20)
    s.close()


def test_limit_flags_getter_state_and_device_output():
    w = _workload("panda7", 1, 64, False, False, (5.0, 95.0), 1300)
    s = _handle(w["model"], w["B"], w["links"], w["q0"], w["A"], PRM, box=w["box"])
    _err(lambda: s.pose_limit_flags(), -24)
    s.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=2)
    _err(lambda: s.pose_limit_flags(), -24)          # the last solve_pose ran without limits
    s.set_joint_limits(w["q_lo"], w["q_hi"])
    out = s.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=2, q=w["q0"])
    assert out["limit_flags"].shape == (w["B"], w["model"].nv) and out["limit_flags"].dtype == np.int32 and out["limit_flags"].any()
    d = capi.DeviceArray(np.zeros((w["B"] * w["model"].nv + 1) // 2))   # room for B * nv ints
    import ctypes as C
    assert s.L.loikb_pose_get_limit_flags(s.h, C.c_void_p(d.data_ptr()), capi.OUT_DEVICE) == 0
    back = np.zeros((w["B"] * w["model"].nv + 1) // 2)
    assert capi.DeviceArray.hip().hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(d.data_ptr()), back.nbytes, 2) == 0
    assert np.array_equal(back.view(np.int32)[:w["B"] * w["model"].nv].reshape(w["B"], -1), out["limit_flags"])
    s.set_joint_limits(None, None)
    s.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=1)
    _err(lambda: s.pose_limit_flags(), -24)
    s.close()
