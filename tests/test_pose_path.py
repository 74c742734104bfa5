"""GPU: waypoint paths in the pose loop (include/loik_amd_path.h, loikb_solve_pose_path) -- one waypoint IS SolvePose, bit for
bit; parity with the lock-step path oracle (tests/pose_path_numpy.py, proven on the CPU by tests/test_pose_path_oracle.py) under
the gate of tests/test_pose_parity.py (the same reached / steps on >= 99 % of the oracle's subset, |dq| < 1e-7 on those) plus
equal cursor / wsteps and every recorded q_path row within 1e-7; the asynchrony on the device's own counts; the status
arithmetic; a B = 1 path against chained SolvePose calls; and the argument errors."""
import ctypes as C

import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from test_pose_ik import PRM, _links
from test_pose_parity import F32_STEP_REL, _box, _gate, _handle, _nonsym_A, _subset
import pose_numpy as P
import pose_limits_numpy as PL
import pose_path_numpy as PP
import pose_tasks_numpy as PT

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _path_workload(model, links, B, T, seed, spread=(1e-3, 0.3), shared=False, frames=None):
    """targets = FK of random configurations q_t, seeds = those moved by a velocity v of a size log-uniform in `spread`
    (test_pose_parity._seeds), and T waypoints on the way back: waypoint t = FK(integrate(q_t, (1 - f_t) v)) with f_{T-1} = 1, the
    last one the target.  The legs f_t - f_{t-1} of an instance are log-uniform over three decades (normalised), so that some are
    crossed in the re-target that reaches the waypoint before and others take several steps: the cursors spread over the path.
    shared: the path of instance 0 for the batch, the seeds scattered around its start.
    Returns (q0 [B][nq], waypoints [B][T][nc][12] or [T][nc][12], q_t)."""
    rng = np.random.default_rng(seed)
    q_t = model.random_configurations(rng, B)
    size = np.exp(rng.uniform(np.log(spread[0]), np.log(spread[1]), size=B))
    v = size[:, None] * rng.normal(size=(B, model.nv)) / np.sqrt(model.nv)
    legs = 10.0 ** rng.uniform(-3, 0, size=(B, T))
    f = np.cumsum(legs, axis=1) / legs.sum(axis=1, keepdims=True)
    f[:, -1] = 1.0
    fk = (lambda q: P.fk12(model, q, links)) if frames is None else (lambda q: PT.frame_fk12(model, q, links, frames))
    q0 = np.stack([P.integrate(model, q_t[b], v[b]) for b in range(B)])
    wp = np.stack([fk(np.stack([P.integrate(model, q_t[b], (1.0 - f[b, t]) * v[b]) for b in range(B)])) for t in range(T)], axis=1)
    if shared:
        wp = wp[0]
        q0 = np.stack([P.integrate(model, q0[0], 0.02 * rng.normal(size=model.nv) * 10.0 ** rng.uniform(-3, 0)) for _ in range(B)])
    return q0, wp, q_t


def _path_gate(out, q, o, idx, what):
    """test_pose_parity._gate, then the path's own: cursor and wsteps equal on the instances the gate accepted, every recorded
    q_path row within 1e-7 of the oracle's and the same rows NaN"""
    same = _gate(out, q, o, idx, what)
    assert np.array_equal(out["cursor"][idx][same], o["cursor"][same]), what
    assert np.array_equal(out["wsteps"][idx][same], o["wsteps"][same]), what
    assert np.array_equal(out["path_status"][idx][same], o["path_status"][same]), what
    got, want = out["q_path"][idx][same], o["q_path"][same]
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    rec = ~np.isnan(want)
    if rec.any():
        assert np.max(np.abs(got[rec] - want[rec])) < 1e-7, (what, np.max(np.abs(got[rec] - want[rec])))
    return same


def _wp_of(wp, idx):
    return wp[idx] if wp.ndim == 4 else np.broadcast_to(wp, (len(idx),) + wp.shape)


# ---- 1. one waypoint, no budget: SolvePose bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["Ash", "Ainst", "tasks", "limits", "f32"])
@pytest.mark.parametrize("name,nc,B", [("talos32", 2, 193), ("panda7", 1, 64), ("talos32", 1, 1)])
def test_one_waypoint_is_solve_pose_bit_for_bit(name, nc, B, form):
    model = loik_amd.builtin_model(name)
    _check_one_waypoint_is_solve_pose(model, _links(model, nc), B, form)


def _check_one_waypoint_is_solve_pose(model, links, B, form):
    nc = len(links)
    rng = np.random.default_rng(3000 + B)
    frames = PT.random_frames(rng, nc) if form == "tasks" else None
    q0, wp, q_t = _path_workload(model, links, B, 1, seed=3001 + B + nc, frames=frames)
    A = _nonsym_A(rng, nc, B) if form == "Ainst" else np.tile(np.eye(6), (nc, 1, 1)) if form == "tasks" else _nonsym_A(rng, nc)
    if form == "limits":
        q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, 3002)
    res = []
    for path in (False, True):
        s = _handle(model, B, links, q0, A, PRM, precision=capi.F32 if form == "f32" else capi.F64)
        if form == "tasks":
            s.set_pose_tasks(["position", "pose"][:nc], frames)
        if form == "limits":
            s.set_joint_limits(q_lo, q_hi)
        kw = dict(dt=0.5, gain=0.8, tol_pose=TOL, max_steps=4)
        out = s.SolvePosePath(wp, **kw) if path else s.SolvePose(wp[:, 0], **kw)
        res.append((out, s.get("q"), s.get("z")))
        s.close()
    (a, qa, za), (b, qb, zb) = res
    for key in ("steps", "status", "err") + (("limit_flags",) if form == "limits" else ()):
        assert np.array_equal(a[key], b[key]), (form, key)
    assert np.array_equal(qa, qb) and np.array_equal(za, zb)
    assert np.array_equal(b["cursor"], a["reached"].astype(np.int32)) and np.array_equal(b["wsteps"][:, 0], a["steps"])
    r = a["reached"]
    assert np.array_equal(b["q_path"][r, 0], qa[r]) and np.all(np.isnan(b["q_path"][~r]))
    if B > 1:
        assert a["steps"].any() and len(set(a["steps"].tolist())) > 1


# ---- 2. parity with the lock-step path oracle -------------------------------------------------------------------------------------
PARITY = [
    # (robot, nc, T, B, waypoints shared, A per instance, (gain, dt), variant, max_steps, budget); max_steps is chosen on the oracle
    # so that the loop ends with the cursors spread over the path: some paths complete, most instances under way
    ("talos32", 1, 2, 193, False, False, (1.0, 1.0), "plain", 2, 0),
    ("talos32", 2, 5, 193, True, False, (1.0, 1.0), "plain", 4, 0),
    ("talos32", 2, 5, 193, False, True, (0.5, 0.25), "plain", 6, 0),
    ("panda7", 1, 5, 64, False, True, (0.5, 0.25), "plain", 6, 3),
    ("panda7", 2, 2, 1, False, False, (1.0, 1.0), "plain", 6, 0),
    ("talos32", 1, 1, 64, False, False, (1.0, 1.0), "plain", 4, 2),
    ("talos32", 2, 2, 193, False, True, (1.0, 0.5), "limits", 4, 0),
    ("panda7", 1, 5, 64, False, False, (1.0, 1.0), "limits", 4, 2),
    ("talos32", 2, 2, 193, False, False, (1.0, 0.5), "tasks", 2, 0),
    ("panda7", 1, 5, 64, True, False, (1.0, 1.0), "tasks", 6, 0),
    ("talos32", 2, 5, 193, False, True, (1.0, 1.0), "device", 4, 0),
    ("panda7", 1, 2, 64, True, False, (1.0, 1.0), "device", 2, 0),
]


@pytest.mark.parametrize("case", PARITY, ids=lambda c: "%s-nc%d-T%d-B%d-%s-%s-g%g-dt%g-%s-k%d-m%d" % (
    c[0], c[1], c[2], c[3], "wpsh" if c[4] else "wpinst", "Ainst" if c[5] else "Ash", c[6][0], c[6][1], c[7], c[8], c[9]))
def test_path_matches_lockstep_path_oracle(case):
    name, nc, T, B, shared, a_inst, (gain, dt), variant, k, budget = case
    model = loik_amd.builtin_model(name)
    links = _links(model, nc)
    rng = np.random.default_rng(3100 + B + 10 * nc + T)
    tasks, limits = variant == "tasks", variant == "limits"
    frames = PT.random_frames(rng, nc) if tasks else None
    kinds = ["position"] * nc if tasks else None
    A = np.tile(np.eye(6), (nc, 1, 1)) if tasks else _nonsym_A(rng, nc, B if a_inst else None)
    q0, wp, q_t = _path_workload(model, links, B, T, seed=3101 + B + nc + T, shared=shared, frames=frames)
    okw = {}
    if limits:
        q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, 3102)
        okw.update(q_lo=q_lo, q_hi=q_hi)
    if tasks:
        okw.update(kinds=[PT.TASK_POSITION] * nc, frames=frames)
    s = _handle(model, B, links, q0, A, PRM)
    if tasks:
        s.set_pose_tasks(kinds, frames)
    if limits:
        s.set_joint_limits(q_lo, q_hi)
    kw = dict(dt=dt, gain=gain, tol_pose=TOL, max_steps=k, max_steps_per_waypoint=budget)
    if variant == "device":
        out = s.SolvePosePath(capi.DeviceArray(wp), q=capi.DeviceArray(q0), **kw)
    else:
        out = s.SolvePosePath(wp, **kw)
    q = s.get("q")
    timing = s.path_get("timing")
    s.close()
    idx = _subset(B)
    lb, ub = _box(model)
    o = PP.lockstep_path_loop(model, PRM, q0[idx], np.eye(6), np.zeros(6), links, A[idx] if A.ndim == 4 else A, lb, ub, _wp_of(wp, idx), dt,
                              gain, TOL, k, budget=budget, **okw)
    print("pose_path_measured %s | oracle cursor %s | path_status %s | steps %s | loop %d (device %d)"
          % (case, np.bincount(o["cursor"], minlength=T + 1).tolist(), np.bincount(o["path_status"], minlength=3).tolist(),
             np.bincount(o["steps"]).tolist(), o["n_solves"], timing["steps"]))
    same = _path_gate(out, q, o, idx, case)
    assert np.array_equal(out["wsteps"].sum(axis=1), out["steps"])
    assert timing["steps"] == out["steps"].max()
    if limits:
        assert (out["limit_flags"][idx][same] != o["limit_flags"][same]).any(axis=1).mean() <= 0.01, case
        lim = np.isfinite(q_lo) | np.isfinite(q_hi)
        ci = PL.limit_q_index(model)[lim]
        assert np.all(q_lo[lim] <= q[:, ci]) and np.all(q[:, ci] <= q_hi[lim])
    if B > 1:   # the case means something: instances are spread over the path
        assert len(set(o["cursor"].tolist())) > 1 or T == 1, o["cursor"]
        assert o["steps"].any()
    if budget and B > 1:
        assert (o["path_status"] == PP.PATH_STALLED).any()


def test_f32_handle_step_and_fp64_error():
    """an fp32 handle with a per-instance A (the re-target reads A from the f32 tiles): the first waypoint is already satisfied, one
    step towards the second against an fp64 handle given the same float32-rounded A (F32_STEP_REL of test_pose_parity: both inner
    solves run the same 40 iterations), err is fp64, and the fp64 handle is anchored to the oracle"""
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 2)
    B, T = 128, 2
    q0, wp, _ = _path_workload(model, links, B, 1, seed=3201, spread=(1e-3, 0.1))
    wp = np.concatenate([P.fk12(model, q0, links)[:, None], wp], axis=1)
    A = _nonsym_A(np.random.default_rng(3202), 2, B).astype(np.float32).astype(np.float64)
    prm = dict(PRM, max_iter=40, tol_abs=0.0, tol_rel=0.0, tol_primal_inf=0.0, tol_dual_inf=0.0)
    res = {}
    for prec in (capi.F32, capi.F64):
        s = _handle(model, B, links, q0, A, prm, precision=prec)
        z = s.SolvePosePath(wp, dt=0.5, gain=0.7, tol_pose=1e-9, max_steps=0)
        assert np.all(z["cursor"] == 1) and not z["steps"].any()
        assert np.max(np.abs(z["err"] - P.pose_errors(model, q0, links, wp[:, 1]))) <= 1e-10
        out = s.SolvePosePath(wp, dt=0.5, gain=0.7, tol_pose=1e-9, max_steps=1)
        res[prec] = (out, s.get("q"))
        s.close()
    (o32, q32), (o64, q64) = res[capi.F32], res[capi.F64]
    for key in ("steps", "cursor", "wsteps"):
        assert np.array_equal(o32[key], o64[key]), key
    assert o64["steps"].all() and np.all(o64["cursor"] == 1) and np.array_equal(o64["wsteps"], np.tile([0, 1], (B, 1)))
    assert np.array_equal(o32["q_path"][:, 0], q0) and np.all(np.isnan(o32["q_path"][:, 1]))
    rel = np.abs(q32 - q64).max(axis=1) / np.abs(q64 - q0).max(axis=1)
    print("f32 vs f64 path step: max relative difference %.3e, median %.3e" % (rel.max(), np.median(rel)))
    assert rel.max() < F32_STEP_REL, rel.max()
    idx = _subset(B)
    lb, ub = _box(model)
    o = PP.lockstep_path_loop(model, prm, q0[idx], np.eye(6), np.zeros(6), links, A[idx], lb, ub, wp[idx], 0.5, 0.7, 1e-9, 1)
    assert np.abs(q64[idx] - o["q"]).max() < 1e-7


# ---- 3. asynchrony, on the device's own counts -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["talos32", "panda7"])
def test_asynchrony_loop_is_as_long_as_its_longest_instance(name):
    model = loik_amd.builtin_model(name)
    links = _links(model, 1)
    B, T = 64, 2
    q_a, wp, far_first = PP.asynchrony_workload(model, links, B, T, seed=1)
    s = _handle(model, B, links, q_a, np.eye(6)[None], PRM)
    out = s.SolvePosePath(wp, dt=1.0, gain=0.5, tol_pose=TOL, max_steps=200)
    timing = s.path_get("timing")
    s.close()
    lockstep = int(out["wsteps"].max(axis=0).sum())
    print("pose_path_measured asynchrony %s: loop %d, sum of per-waypoint maxima %d, complete %d / %d"
          % (name, timing["steps"], lockstep, int((out["path_status"] == capi.PATH_ST_COMPLETE).sum()), B))
    assert np.all(out["path_status"] == capi.PATH_ST_COMPLETE) and out["reached"].all() and np.all(out["cursor"] == T)
    assert timing["steps"] == out["steps"].max()
    assert timing["steps"] < lockstep, (timing["steps"], lockstep)


# ---- 4. status arithmetic ----------------------------------------------------------------------------------------------------------
def test_stalled_instances_stop_moving():
    """a budget of 4 on the asynchrony workload: a near leg fits, a far leg does not, so the even instances stall on their first
    waypoint and the odd ones, later, on their second.  A stalled instance sits where its last counted step left it -- the q of
    the same path without a budget, cut at max_steps = its step count -- while the rest of the batch goes on"""
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 1)
    B, T, budget = 193, 2, 4
    q_a, wp, _ = PP.asynchrony_workload(model, links, B, T, seed=5)
    kw = dict(dt=1.0, gain=0.5, tol_pose=TOL)
    s = _handle(model, B, links, q_a, np.eye(6)[None], PRM)
    out = s.SolvePosePath(wp, max_steps=40, max_steps_per_waypoint=budget, **kw)
    q = s.get("q")
    s.close()
    stalled = out["path_status"] == capi.PATH_ST_STALLED
    assert stalled.any() and not (out["status"][stalled] & (capi.POSE_ST_REACHED | capi.POSE_ST_STOPPED)).any()
    assert not (out["path_status"] == (capi.PATH_ST_STALLED | capi.PATH_ST_COMPLETE)).any()
    b = np.arange(B)[stalled]
    assert np.all(out["wsteps"][b, out["cursor"][b]] == budget) and np.all(out["cursor"][b] < T)
    assert np.all(np.abs(out["err"][stalled]).max(axis=(1, 2)) > TOL)
    assert len(np.unique(out["cursor"][stalled])) == 2 and len(np.unique(out["steps"][stalled])) > 1
    for n in np.unique(out["steps"][stalled]):   # the same path without a budget, cut at n steps: where the instances with n steps were
        s = _handle(model, B, links, q_a, np.eye(6)[None], PRM)
        cut = s.SolvePosePath(wp, max_steps=int(n), **kw)
        qn = s.get("q")
        s.close()
        m = stalled & (out["steps"] == n)
        assert np.all(cut["steps"][m] == n)
        assert np.max(np.abs(q[m] - qn[m])) <= 1e-12, (n, np.max(np.abs(q[m] - qn[m])))


def test_nan_seed_zero_steps_unreached_rows_and_record_off():
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 2)
    B, T, bad = 64, 5, 37
    q0, wp, _ = _path_workload(model, links, B, T, seed=3301)
    wp[::4, 0] = P.fk12(model, q0[::4], links)   # every fourth instance starts on its first waypoint
    qs = q0.copy()
    qs[bad, 2] = np.nan
    A = np.tile(np.eye(6), (2, 1, 1))
    s = _handle(model, B, links, qs, A, PRM)
    # max_steps = 0 fills err and cursor only
    z = s.SolvePosePath(wp, tol_pose=TOL, max_steps=0)
    assert not z["steps"].any() and not z["wsteps"].any() and np.array_equal(s.get("q"), qs, equal_nan=True)
    keep = np.arange(B) != bad
    errs = np.stack([np.abs(P.pose_errors(model, q0, links, wp[:, t])).max(axis=(1, 2)) for t in range(T)], axis=1)   # [B][T]
    want_cursor = np.where((errs > TOL).any(axis=1), (errs > TOL).argmax(axis=1), T)   # the waypoints q0 satisfies, from the first on
    want_cursor[bad] = 0
    assert np.array_equal(z["cursor"], want_cursor) and np.all(want_cursor[::4][np.arange(0, B, 4) != bad] >= 1) and (want_cursor == 0).any()
    assert z["status"][bad] == capi.POSE_ST_STOPPED and z["path_status"][bad] == 0
    want = P.pose_errors(model, q0, links, wp[np.arange(B), np.minimum(z["cursor"], T - 1)])
    assert np.max(np.abs(z["err"][keep] - want[keep])) < 1e-10
    crossed = np.arange(T)[None, :] < want_cursor[:, None]
    assert np.array_equal(z["q_path"][crossed], np.repeat(q0[:, None], T, axis=1)[crossed]) and np.all(np.isnan(z["q_path"][~crossed]))
    # a NaN seed: STOPPED with cursor 0, the others as without it
    out = s.SolvePosePath(wp, tol_pose=TOL, max_steps=6)
    s.close()
    assert out["status"][bad] == capi.POSE_ST_STOPPED and out["cursor"][bad] == 0 and out["steps"][bad] == 0
    assert out["path_status"][bad] == 0 and np.all(np.isnan(out["q_path"][bad]))
    s = _handle(model, B, links, q0, A, PRM)
    ref = s.SolvePosePath(wp, tol_pose=TOL, max_steps=6, record=False)
    assert ref["q_path"] is None
    for key in ("steps", "status", "cursor", "wsteps", "path_status"):
        assert np.array_equal(out[key][keep], ref[key][keep]), key
    # unreached rows are NaN, reached rows are not
    reached_rows = np.arange(T)[None, :] < out["cursor"][:, None]
    assert np.array_equal(np.isnan(out["q_path"]).all(axis=2), ~reached_rows) and not np.isnan(out["q_path"][reached_rows]).any()
    assert 0 < reached_rows.mean() < 1
    # record = 0: LOIKB_PATH_F_Q is a state error, the other fields are there
    buf = np.empty((B, T, model.nq))
    assert s.L.loikb_path_get(s.h, capi.PATH_F_Q, buf.ctypes.data_as(C.c_void_p), 0) == -24
    assert np.array_equal(s.path_get("cursor"), ref["cursor"])
    s.close()


def test_path_get_before_the_first_path_call():
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 1)
    q0, wp, _ = _path_workload(model, links, 4, 2, seed=3401)
    s = _handle(model, 4, links, q0, np.eye(6)[None], PRM)
    buf = np.empty(4, dtype=np.int32)
    assert s.L.loikb_path_get(s.h, capi.PATH_F_CURSOR, buf.ctypes.data_as(C.c_void_p), 0) == -24
    s.SolvePose(wp[:, 0], max_steps=1)
    assert s.L.loikb_path_get(s.h, capi.PATH_F_CURSOR, buf.ctypes.data_as(C.c_void_p), 0) == -24
    s.close()


# ---- 5. B = 1: a path is T chained SolvePose calls ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nc,T", [("talos32", 2, 5), ("panda7", 1, 2)])
def test_single_instance_path_is_chained_solve_pose(name, nc, T):
    """one instance: the path loop runs the inner solves of T chained SolvePose(q=None) calls in the same order from the same
    states (a lone instance never idles), so per-waypoint steps are equal and q is expected bit-equal; the bound is 1e-7"""
    model = loik_amd.builtin_model(name)
    links = _links(model, nc)
    q0, wp, _ = _path_workload(model, links, 1, T, seed=3501 + T, spread=(0.1, 0.15))
    A = np.tile(np.eye(6), (nc, 1, 1))
    kw = dict(dt=1.0, gain=0.8, tol_pose=TOL)
    s = _handle(model, 1, links, q0, A, PRM)
    out = s.SolvePosePath(wp, max_steps=100, **kw)
    q = s.get("q")
    s.close()
    assert out["path_status"][0] == capi.PATH_ST_COMPLETE and out["cursor"][0] == T
    s = _handle(model, 1, links, q0, A, PRM)
    for t in range(T):
        leg = s.SolvePose(wp[:, t], max_steps=100, **kw)
        assert leg["reached"][0] and leg["steps"][0] == out["wsteps"][0, t], (t, leg["steps"], out["wsteps"])
        qt = s.get("q")
        assert np.max(np.abs(qt[0] - out["q_path"][0, t])) < 1e-7
        print("pose_path_measured chain %s t=%d: steps %d, bit-equal %s" % (name, t, leg["steps"][0], np.array_equal(qt[0], out["q_path"][0, t])))
    s.close()
    assert np.max(np.abs(qt - q)) < 1e-7 and out["wsteps"].sum() == out["steps"][0] > T


# ---- 6. argument errors leave the handle as it was -----------------------------------------------------------------------------------
def test_argument_errors_leave_the_handle_unchanged():
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 1)
    B, T = 16, 2
    q0, wp, _ = _path_workload(model, links, B, T, seed=3601)
    A = np.eye(6)[None]
    kw = dict(dt=0.5, gain=0.9, tol_pose=TOL, max_steps=3)
    s = _handle(model, B, links, q0, A, PRM)
    fresh = s.SolvePose(wp[:, 1], **kw)
    fresh["q"], fresh["z"] = s.get("q"), s.get("z")
    s.close()
    flat = np.ascontiguousarray(wp.reshape(B, T, 1, 12))
    bad_rot = flat.copy()
    bad_rot[5, 1, 0, 0] += 1e-6          # the LAST waypoint of an instance: the check covers all of them
    nan_wp = flat.copy()
    nan_wp[2, 0, 0, 10] = np.nan
    pose_ok = capi.PoseParams(0.5, 0.9, TOL, 3, 0)

    def raw(s, w, pose, path):
        return s.L.loikb_solve_pose_path(s.h, None, w.ctypes.data_as(C.c_void_p), 0, C.byref(pose), C.byref(path))

    cases = {
        "T = 0": lambda s: raw(s, flat, pose_ok, capi.PathParams(0, 0, 1, 0)),
        "T < 0": lambda s: raw(s, flat, pose_ok, capi.PathParams(-1, 0, 1, 0)),
        "budget < 0": lambda s: raw(s, flat, pose_ok, capi.PathParams(T, -1, 1, 0)),
        "record 2": lambda s: raw(s, flat, pose_ok, capi.PathParams(T, 0, 2, 0)),
        "record -1": lambda s: raw(s, flat, pose_ok, capi.PathParams(T, 0, -1, 0)),
        "flags": lambda s: raw(s, flat, pose_ok, capi.PathParams(T, 0, 1, 1)),
        "dt": lambda s: raw(s, flat, capi.PoseParams(0.0, 0.9, TOL, 3, 0), capi.PathParams(T, 0, 1, 0)),
        "gain": lambda s: raw(s, flat, capi.PoseParams(0.5, -1.0, TOL, 3, 0), capi.PathParams(T, 0, 1, 0)),
        "tol": lambda s: raw(s, flat, capi.PoseParams(0.5, 0.9, -1.0, 3, 0), capi.PathParams(T, 0, 1, 0)),
        "max_steps": lambda s: raw(s, flat, capi.PoseParams(0.5, 0.9, TOL, -1, 0), capi.PathParams(T, 0, 1, 0)),
        "rotation": lambda s: raw(s, bad_rot, pose_ok, capi.PathParams(T, 0, 1, 0)),
        "nan": lambda s: raw(s, nan_wp, pose_ok, capi.PathParams(T, 0, 1, 0)),
        "null waypoints": lambda s: s.L.loikb_solve_pose_path(s.h, None, None, 0, C.byref(pose_ok), C.byref(capi.PathParams(T, 0, 1, 0))),
        "null path": lambda s: s.L.loikb_solve_pose_path(s.h, None, flat.ctypes.data_as(C.c_void_p), 0, C.byref(pose_ok), None),
    }
    for what, call in cases.items():
        s = _handle(model, B, links, q0, A, PRM)
        assert call(s) == -20, what
        got = s.SolvePose(wp[:, 1], **kw)
        for key in ("steps", "status", "err"):
            assert np.array_equal(got[key], fresh[key]), (what, key)
        assert np.array_equal(s.get("q"), fresh["q"]) and np.array_equal(s.get("z"), fresh["z"]), what
        s.close()
    # the binding's own checks, and a handle before SolveInit
    s = _handle(model, B, links, q0, A, PRM)
    with pytest.raises(ValueError):
        s.SolvePosePath(wp[:, :, 0])          # [B][T][12]: no constraint axis
    with pytest.raises(loik_amd.LoikError) as e:
        s.SolvePosePath(bad_rot)
    assert e.value.code == -20 and "waypoint" in str(e.value)
    s.close()
    s = loik_amd.BatchedLoik(model, B, **dict(PRM))
    with pytest.raises(loik_amd.LoikError) as e:
        s.SolvePosePath(flat)
    assert e.value.code == -24
    s.close()
