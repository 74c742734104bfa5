"""GPU: certified RRT-Connect planning of include/loik_amd_plan.h against the numpy reference of tests/plan_numpy.py (proven on the CPU by
test_plan_numpy.py): five robots and tree330 (which takes its records and dv from the global slab) in the world of test_clearance._case,
the result's own consistency with path_clearance and path_length bit for bit, the wall a direct segment cannot pass, the chain into
shortcut_paths and retime_paths, the edge cases, determinism and the pointer routes, neutrality towards the solves, the validation."""
import ctypes as C

import numpy as np
import pytest

import loik_amd
from loik_amd import capi

import motion_numpy as MN
import plan_numpy as PN
import pose_numpy as P
import test_clearance as TC
import test_motion_clearance as TM
import test_plan_numpy as TP
from test_shortcut import _back, _device_i32

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -20, -24
T_PLAN, TOL, MAX_EVALS = TP.T_PLAN, TP.TOL, TP.MAX_EVALS
# |got - numpy| / (1 + |numpy|) over the rows of the found paths and their lengths: 16 times the largest error measured on one MI355X over
# the six robots of test 1 (profiles/plan_measured.md), the allowance for another compiler's rounding, as RETIME_BOUND of test_retime.py was set
PLAN_MEASURED = 3.741e-16   # (multidof13; the others between 8.9e-17 and 1.5e-16)
PLAN_BOUND = 16 * PLAN_MEASURED
# name -> (queries, goals near the starts, what differs from test_plan_numpy.plan_case's parameters).  composite20: the world leaves edges of
# 0.5 no room, so it steps by 0.1, fills trees of 60 nodes and finds paths that are TOO_LONG for T = 32.  tree330, the slab instantiation:
# 24 samples decide no edge of 330 joints longer than about 0.05, so its goals lie 0.3 from the starts and the margin is far below the
# clearance: the direct segment is UNDECIDED, and one iteration of seven edges finds a path of 9 waypoints
ROBOTS = {"panda7": (16, None, {}), "talos32": (16, None, {}), "multidof13": (16, None, {}), "composite20": (16, None, dict(step=0.1)),
          "helical24": (16, None, {}), "tree330": (2, 0.03, dict(max_iters=4, step=0.05, margin=-1.0))}
SMALL = [n for n in ROBOTS if n != "tree330"]
FIELDS = ("status", "n_waypoints", "iterations", "nodes", "edges_checked", "edges_free", "evals")


def case(name):
    B, near, over = ROBOTS[name]
    return TP.plan_case(name, B, near=near, **over)


def _plan(s, c, start=None, goal=None, T=T_PLAN, **over):
    return s.plan_paths(c["start"] if start is None else start, c["goal"] if goal is None else goal, c["lo"], c["hi"], T, **dict(c["kw"], **over))


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def _rows(r, rows):
    return {k: v[rows] for k, v in r.items()}


def _check_self(s, got, start, goal, margin, tol, max_evals):
    """2. what holds for every result, bit for bit: the found paths FREE under path_clearance (padding included), the length path_length's,
    the ends the inputs, the padding the last row, NaN everywhere else"""
    B, T = got["q_path"].shape[:2]
    found = got["status"] == capi.PLAN_FOUND
    assert np.isnan(got["q_path"][~found]).all() and np.isnan(got["length"][~found]).all()
    assert np.all(got["n_waypoints"][~found & (got["status"] != capi.PLAN_TOO_LONG)] == 0)
    assert np.all(got["edges_free"] <= got["edges_checked"])
    if not found.any():
        return
    paths = np.ascontiguousarray(got["q_path"][found])
    chk = s.path_clearance(paths, margin=margin, tol=tol, max_evals=max_evals)
    assert np.all(chk["status"] == MN.FREE), chk["status"]
    assert np.array_equal(s.path_length(paths), got["length"][found])
    for i, b in enumerate(np.flatnonzero(found)):
        L = int(got["n_waypoints"][b])
        assert 2 <= L <= T and np.array_equal(paths[i, 0], start[b]) and np.array_equal(paths[i, L - 1], goal[b])
        assert np.array_equal(paths[i, L:], np.tile(goal[b], (T - L, 1)))
        assert (L == 2) == (got["iterations"][b] == 0)


# ---- 1. against numpy, 2. self-consistency -------------------------------------------------------------------------------------------------
# No query of the six references has a decision within 1e-9 of its threshold (checked here on the CPU; at most 1 in 16 is allowed), so
# test_clearance's rng and seed 4242 stand for every robot.  The references take 1 to 3 s of numpy each, composite20's 7 s and tree330's,
# which walks every root path in Python, 9 s
@pytest.mark.parametrize("name", list(ROBOTS))
def test_plan_matches_numpy_and_is_consistent(name):
    c = case(name)
    model, want, B = c["model"], c["want"], c["B"]
    print("plan_measured %s: status %s, L %s, iterations %s, nodes up to %d, queries with near %d" % (
        name, want["status"].tolist(), want["n_waypoints"].tolist(), want["iterations"].tolist(), int(want["nodes"].max()), int(want["near"].sum())))
    assert want["near"].sum() <= B // 16
    s = TM._open(c)
    got = _plan(s, c)
    _check_self(s, got, c["start"], c["goal"], c["kw"]["margin"], TOL, MAX_EVALS)
    sure = ~want["near"]
    for k in FIELDS:
        assert np.array_equal(got[k][sure], want[k][sure]), (name, k, got[k], want[k])
    found = sure & (want["status"] == PN.FOUND)
    err = 0.0
    for k in ("q_path", "length"):
        err = max(err, float(np.max(np.abs(got[k][found] - want[k][found]) / (1.0 + np.abs(want[k][found])), initial=0.0)))
    print("plan_measured %s: max |got - numpy| / (1 + |numpy|) over rows and lengths %.3e" % (name, err))
    assert err <= PLAN_BOUND, (name, err)
    s.close()


def test_the_small_robots_see_every_kind_of_outcome():
    seen = {"direct": 0, "tree": 0, "exhausted": 0}
    for name in SMALL:
        w = case(name)["want"]
        seen["direct"] += int(((w["status"] == PN.FOUND) & (w["iterations"] == 0)).sum())
        seen["tree"] += int(((w["status"] == PN.FOUND) & (w["iterations"] > 0)).sum())
        seen["exhausted"] += int((w["status"] == PN.EXHAUSTED_ITERS).sum())
    print("plan_measured outcomes on the small robots: %s" % seen)
    assert min(seen.values()) > 0, seen
    c = case("talos32")      # one robot has all three: its device answer has them too
    s = TM._open(c)
    got = _plan(s, c)
    assert ((got["status"] == capi.PLAN_FOUND) & (got["iterations"] == 0)).any() and ((got["status"] == capi.PLAN_FOUND) & (got["iterations"] > 0)).any()
    assert (got["status"] == capi.PLAN_EXHAUSTED_ITERS).any()
    s.close()


# ---- 3. the wall ---------------------------------------------------------------------------------------------------------------------------
def test_a_thin_box_across_the_direct_segment_is_planned_around():
    w = TP.wall_case()
    model, A, Bq = w["model"], w["A"], w["Bq"]
    s = TC._open(model, np.stack([A, Bq]))
    s.set_collision_spheres(w["links"], w["spheres"])
    s.set_collision_world(None, w["box"][None])
    assert np.all(s.clearance(np.stack([A, Bq]))["min"] >= TOL)
    assert s.motion_clearance(A[None], qb=Bq[None], margin=0.0, tol=TOL)["status"][0] == MN.BLOCKED
    kw = dict(step=0.5, max_iters=16, max_nodes=16, seed=1, margin=0.0, tol=TOL)
    got = s.plan_paths(A[None], Bq[None], w["lo"], w["hi"], 16, **kw)
    want = PN.plan(model, A, Bq, w["links"], w["spheres"], w["lo"], w["hi"], 16, wboxes=w["box"][None], **kw)
    assert got["status"][0] == capi.PLAN_FOUND and got["n_waypoints"][0] >= 3 and got["iterations"][0] >= 1
    assert want["near"][0] or all(np.array_equal(got[k], want[k]) for k in FIELDS)
    _check_self(s, got, A[None], Bq[None], 0.0, TOL, 256)
    s.set_collision_world(None, None)
    got = s.plan_paths(A[None], Bq[None], w["lo"], w["hi"], 16, **kw)
    assert got["status"][0] == capi.PLAN_FOUND and got["n_waypoints"][0] == 2 and got["iterations"][0] == 0 and got["edges_checked"][0] == 1
    assert np.array_equal(got["q_path"][0, 0], A) and np.all(got["q_path"][0, 1:] == Bq) and got["nodes"][0].tolist() == [1, 1]
    s.close()


# ---- 4. the chain --------------------------------------------------------------------------------------------------------------------------
def test_a_planned_path_goes_through_shortcut_and_retime():
    c = case("panda7")
    model = c["model"]
    s = TM._open(c)
    got = _plan(s, c)
    found = got["status"] == capi.PLAN_FOUND
    assert (got["n_waypoints"][found] >= 3).any()
    paths, n = np.ascontiguousarray(got["q_path"][found]), got["n_waypoints"][found].astype(np.int32)
    kw = dict(margin=c["margin"], tol=TOL, max_evals=MAX_EVALS)
    for cnt in (None, n):
        cut = s.shortcut_paths(paths, n_waypoints=cnt, rounds=16, seed=7, **kw)
        assert np.all(cut["invalid"] == 0) and np.all(cut["n_waypoints"] >= 2) and np.all(cut["n_waypoints"] <= (T_PLAN if cnt is None else n))
        assert np.all(s.path_clearance(cut["q_path"], **kw)["status"] == MN.FREE)
        assert np.array_equal(cut["length_in"], got["length"][found])
        assert np.array_equal(cut["q_path"][:, 0], c["start"][found]) and np.array_equal(cut["q_path"][:, -1], c["goal"][found])
        timed = s.retime_paths(cut["q_path"], 1.0, 2.0, 0.05, n_waypoints=cut["n_waypoints"])
        assert np.all(timed["flags"] == 0) and np.all(timed["duration"] > 0.0) and np.all(timed["n_samples"] >= 2)
    assert cut["accepted"].sum() > 0
    s.close()


# ---- 5. the edge cases ---------------------------------------------------------------------------------------------------------------------
def test_edges():
    c = case("panda7")
    model, want, B = c["model"], c["want"], c["B"]
    start, goal = c["start"], c["goal"]
    s = TM._open(c)
    full = _plan(s, c)
    tree = np.flatnonzero((full["status"] == capi.PLAN_FOUND) & (full["n_waypoints"] >= 3))
    blocked_s, blocked_g = np.flatnonzero(full["status"] == capi.PLAN_START_BLOCKED), np.flatnonzero(full["status"] == capi.PLAN_GOAL_BLOCKED)
    free_ends = np.flatnonzero(~np.isin(full["status"], (capi.PLAN_START_BLOCKED, capi.PLAN_GOAL_BLOCKED)))
    assert tree.size and blocked_s.size and blocked_g.size
    assert np.all(full["edges_checked"][blocked_s] == 1) and np.all(full["edges_checked"][blocked_g] == 2) and np.all(full["nodes"][blocked_s] == 1)
    # start == goal: the zero segment is FREE where the start is, L = 2 in 0 iterations
    still = _plan(s, c, goal=start)
    assert np.all(still["status"][free_ends] == capi.PLAN_FOUND) and np.all(still["n_waypoints"][free_ends] == 2)
    assert np.all(still["iterations"] == 0) and np.all(still["length"][free_ends] == 0.0) and np.all(still["status"][blocked_s] == capi.PLAN_START_BLOCKED)
    _check_self(s, still, start, start, c["margin"], TOL, MAX_EVALS)
    # max_iters = 0: the checks of step 0 alone
    zero = _plan(s, c, max_iters=0)
    direct = (full["status"] == capi.PLAN_FOUND) & (full["iterations"] == 0)
    settled = np.isin(full["status"], (capi.PLAN_START_BLOCKED, capi.PLAN_GOAL_BLOCKED)) | direct
    assert _same(_rows(zero, settled), _rows(full, settled)) and np.all(zero["status"][~settled] == capi.PLAN_EXHAUSTED_ITERS)
    assert np.all(zero["iterations"] == 0) and np.all(zero["nodes"] == 1) and np.all(zero["edges_checked"][~settled] == 2)
    # max_nodes = 2: the second addition to a tree ends the query
    few = _plan(s, c, max_nodes=2)
    assert np.all(few["status"][tree] == capi.PLAN_EXHAUSTED_NODES) and np.all(few["nodes"] <= 2) and np.all(few["nodes"][tree].max(axis=1) == 2)
    assert np.isnan(few["q_path"][tree]).all() and np.all(few["n_waypoints"][tree] == 0)
    # T too small: TOO_LONG with the true L, everything else as found
    short = _plan(s, c, T=2)
    assert np.all(short["status"][tree] == capi.PLAN_TOO_LONG) and np.array_equal(short["n_waypoints"], full["n_waypoints"])
    assert np.isnan(short["q_path"][tree]).all() and np.isnan(short["length"][tree]).all()
    assert all(np.array_equal(short[k], full[k]) for k in FIELDS[2:])
    # a NaN start and a NaN goal: INVALID, all counters 0, the neighbours untouched
    b0, b1 = int(tree[0]), int(tree[-1] if tree.size > 1 else free_ends[0])
    bad_s, bad_g = start.copy(), goal.copy()
    bad_s[b0, 1] = np.nan
    bad_g[b1, 0] = np.inf
    inv = _plan(s, c, start=bad_s, goal=bad_g)
    others = ~np.isin(np.arange(B), (b0, b1))
    assert _same(_rows(inv, others), _rows(full, others))
    for b in {b0, b1}:
        assert inv["status"][b] == capi.PLAN_INVALID and all(np.all(inv[k][b] == 0) for k in FIELDS[1:]) and np.isnan(inv["q_path"][b]).all()
    # one batch that holds all of them: every row is the row of its own run (a query's words depend on its index, so a row runs alone
    # behind NaN rows, which are INVALID at once)
    rows = [b0, int(blocked_s[0]), int(blocked_g[0]), int(np.flatnonzero(full["status"] == capi.PLAN_EXHAUSTED_ITERS)[0])]
    mixed_s, mixed_g = start.copy(), goal.copy()
    mixed_s[free_ends[-1]] = np.nan
    mixed = _plan(s, c, start=mixed_s, goal=mixed_g)
    assert mixed["status"][free_ends[-1]] == capi.PLAN_INVALID
    for b in rows:
        alone_s, alone_g = np.full((b + 1, model.nq), np.nan), np.full((b + 1, model.nq), np.nan)
        alone_s[b], alone_g[b] = start[b], goal[b]
        assert _same(_rows(_plan(s, c, start=alone_s, goal=alone_g), [b]), _rows(mixed, [b])), b
    # B = 0
    none = _plan(s, c, start=start[:0], goal=goal[:0])
    assert none["q_path"].shape == (0, T_PLAN, model.nq) and none["status"].shape == (0,) and none["nodes"].shape == (0, 2)
    s.close()


# ---- 6. determinism, the routes, neutrality ------------------------------------------------------------------------------------------------
def test_determinism_and_pointer_routes():
    c = case("talos32")
    model, B = c["model"], c["B"]
    nq = model.nq
    s = TM._open(c)
    host = _plan(s, c)
    assert _same(host, _plan(s, c))                                      # the same call twice
    s32 = TM._open(c, capi.F32)
    assert _same(host, _plan(s32, c))                                    # fp64 whatever the handle's precision
    s32.close()
    ds, dg = capi.DeviceArray(c["start"]), capi.DeviceArray(c["goal"])
    assert _same(host, _plan(s, c, start=ds, goal=dg))                   # device in, host out
    for a, g in ((c["start"], c["goal"]), (ds, dg)):                     # host in and device in, device out
        bufs = (capi.DeviceArray(np.full(B * T_PLAN * nq, -1.0)), _device_i32(np.zeros(8 * B)), capi.DeviceArray(np.zeros(B)))
        _plan(s, c, start=a, goal=g, out=bufs)
        got = capi.BatchedLoik._plan_result(_back(bufs[0], (B, T_PLAN, nq), np.float64), _back(bufs[1], (B, 8), np.int32), _back(bufs[2], (B,), np.float64))
        assert _same(host, got)
        _plan(s, c, start=a, goal=g, out=(bufs[0], bufs[1], None))      # without the lengths
        assert np.array_equal(_back(bufs[0], (B, T_PLAN, nq), np.float64), host["q_path"], equal_nan=True)
        for d in bufs:
            d.free()
    ds.free(); dg.free()
    # another seed draws other samples: the queries that ran iterations change, the others do not
    other = _plan(s, c, seed=c["kw"]["seed"] + 1)
    ran = host["iterations"] > 0
    assert ran.any() and not _same(_rows(other, ran), _rows(host, ran)) and _same(_rows(other, ~ran), _rows(host, ~ran))
    s.close()


def test_the_call_changes_no_solve_and_no_resident_q():
    c = case("talos32")
    model = c["model"]
    qa = c["q"]
    links = TC._links(model, 1)
    tg = P.fk12(model, np.clip(qa + 0.05, model.q_lo, model.q_hi), links)
    res = []
    for with_calls in (False, True):
        s, _ = TC._handle(model, c["n"], links, qa)
        s.set_collision_spheres(c["links"], c["spheres"])
        s.set_collision_world(c["ws"], c["wb"])
        s.set_self_collision(True)

        def calls():
            if with_calls:
                _plan(s, c)
        q0 = s.get("q")
        calls()
        assert np.array_equal(q0, s.get("q"))
        s.Solve()
        out = [s.get("z"), s.get("iter")]
        calls()
        out += [s.get("z"), s.get("iter"), s.get("q")]
        p = s.SolvePose(tg, tol_pose=1e-4, max_steps=6)
        calls()
        out += [s.get("q"), p["status"], p["err"], s.clearance()["min"]]
        res.append(out)
        s.close()
    assert all(np.array_equal(a, b) for a, b in zip(*res))


# ---- 7. validation -------------------------------------------------------------------------------------------------------------------------
def test_errors():
    c = case("multidof13")      # (a free-flyer root: DoFs that cannot carry a range)
    model, start, goal = c["model"], c["start"], c["goal"]
    B, nq, nv, T = c["B"], model.nq, model.nv, 8
    lo, hi = np.ascontiguousarray(c["lo"]), np.ascontiguousarray(c["hi"])
    s = TC._open(model, c["q"])
    with pytest.raises(capi.LoikError) as e:      # no spheres: the state error, B = 0 included
        _plan(s, c)
    assert e.value.code == ERR_STATE and "no spheres" in str(e.value)
    with pytest.raises(capi.LoikError) as e:
        _plan(s, c, start=start[:0], goal=goal[:0])
    assert e.value.code == ERR_STATE
    s.close()
    s = TM._open(c)
    before = _plan(s, c, T=T)
    L, h, vp, dp = s.L, s.h, C.c_void_p, C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(vp)
    dptr = lambda a: a.ctypes.data_as(dp)
    outs = [np.full((B, T, nq), -7.0), np.full((B, 8), -7, dtype=np.int32), np.full(B, -7.0)]
    P_ = lambda margin=0.0, tol=1e-3, step=0.5, seed=1, max_evals=8, max_iters=4, max_nodes=8, flags=0: capi.PlanParams(margin, tol, step, seed, max_evals, max_iters, max_nodes, flags)
    good = P_()
    untouched = lambda: all(np.all(o == -7) for o in outs)

    def call(prm=good, qs_=ptr(start), qg_=ptr(goal), B_=B, T_=T, lo_=dptr(lo), hi_=dptr(hi), path_=ptr(outs[0]), info_=ptr(outs[1]), len_=ptr(outs[2]), h_=h):
        return L.loikb_plan_paths(h_, qs_, qg_, B_, 0, lo_, hi_, C.byref(prm) if prm is not None else None, T_, path_, info_, len_, 0)
    for bad, text in ((P_(margin=np.nan), b"margin"), (P_(margin=np.inf), b"margin"), (P_(tol=np.nan), b"tol"), (P_(tol=0.5e-9), b"tol"),
                      (P_(max_evals=0), b"max_evals"), (P_(max_evals=65537), b"max_evals"), (P_(step=0.0), b"step"), (P_(step=-1.0), b"step"),
                      (P_(step=np.inf), b"step"), (P_(step=np.nan), b"step"), (P_(max_iters=-1), b"max_iters"), (P_(max_iters=1048577), b"max_iters"),
                      (P_(max_nodes=1), b"max_nodes"), (P_(max_nodes=65537), b"max_nodes"), (P_(flags=1), b"flags"), (None, b"p == NULL")):
        assert call(bad) == ERR_ARG and text in L.loikb_last_error(), text
        assert call(bad, B_=0) == ERR_ARG       # the arguments are checked before anything else
    assert call(h_=None) == ERR_ARG
    assert call(path_=None) == ERR_ARG and b"out_path" in L.loikb_last_error() and call(info_=None) == ERR_ARG and b"out_info" in L.loikb_last_error()
    assert call(qs_=None) == ERR_ARG and b"q_start" in L.loikb_last_error() and call(qg_=None) == ERR_ARG
    assert call(B_=-1) == ERR_ARG and b"B >= 0" in L.loikb_last_error()
    assert call(T_=1) == ERR_ARG and b"T >= 2" in L.loikb_last_error() and call(T_=1, B_=0) == ERR_ARG
    assert call(B_=1 << 20, T_=1 << 11) == ERR_ARG and b"2^31" in L.loikb_last_error()
    assert call(lo_=None) == ERR_ARG and call(hi_=None) == ERR_ARG and b"s_lo and s_hi" in L.loikb_last_error()
    assert call(path_=ptr(start)) == ERR_ARG and b"out_path == q_start" in L.loikb_last_error() and call(path_=ptr(goal)) == ERR_ARG
    # the ranges: lo > hi, a NaN, a finite entry on the free-flyer, nothing to sample
    j = int(np.flatnonzero(np.isfinite(lo))[0])
    free = int(np.flatnonzero(~np.isfinite(lo))[0])
    for edit, text in (((j, 1.0, -1.0), b"s_lo > s_hi"), ((j, np.nan, 1.0), b"NaN"), ((free, -1.0, 1.0), b"cannot carry a position limit"),
                       ((free, -1.0, np.inf), b"cannot carry a position limit")):
        l2, h2 = lo.copy(), hi.copy()
        l2[edit[0]], h2[edit[0]] = edit[1], edit[2]
        assert call(lo_=dptr(l2), hi_=dptr(h2)) == ERR_ARG and text in L.loikb_last_error(), text
    l2, h2 = np.full(nv, -np.inf), hi.copy()
    assert call(lo_=dptr(l2), hi_=dptr(h2)) == ERR_ARG and b"no DoF to sample" in L.loikb_last_error()
    assert untouched()
    assert call(B_=0, qs_=None, qg_=None, path_=None, info_=None) == 0 and untouched()
    assert call(P_(tol=1e-9, max_evals=65536, max_iters=1048576, max_nodes=65536, seed=2 ** 64 - 1), B_=0) == 0 and untouched()
    # the handle is as it was: the same call gives the same answer, with and without the lengths
    assert _same(before, _plan(s, c, T=T))
    assert call(len_=None) == 0 and np.all(outs[2] == -7.0) and np.array_equal(outs[1][:, 0], _plan(s, c, T=T, **dict(seed=1, max_evals=8, max_iters=4, max_nodes=8, margin=0.0, step=0.5))["status"])
    # spheres gone: the state error again
    outs[0][:] = -7.0; outs[1][:] = -7
    s.set_collision_spheres([], np.zeros((0, 4)))
    assert call() == ERR_STATE and call(B_=0) == ERR_STATE and untouched()
    s.close()
