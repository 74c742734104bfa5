"""GPU: multi-start pose IK (include/loik_amd_multistart.h) -- the device sampler against its numpy restatement bit for bit, the
restart loop against the same loop driven from the host on a second handle (bit for bit: both run loikb_solve_pose on the same
seeds), the selection against the numpy rule, what the feature is for (more goals answered with K = 16 than with K = 1), and
the argument / state rules.  fp64 handles with joint limits unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from test_pose_ik import BOUND, PRM, _links
from test_pose_limits import _workload
from test_pose_parity import _box, _handle, _seeds
import pose_numpy as P
import pose_limits_numpy as PL
import pose_multistart_numpy as M
import pose_tasks_numpy as T

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -20, -24
TOL = 1e-4
SEED = 7


def _robot(name, nc=1):
    """model, constrained links, joint limits [nv] (= the ranges the seeds are drawn from), one valid configuration"""
    if name == "multidof":
        w = _workload("multidof", 2, 8, False, False, (5.0, 95.0), 1400)   # free-flyer root (never sampled), a translation and two ZYX joints
        return w["model"], w["links"][:nc], w["q_lo"], w["q_hi"], w["q0"]
    model = loik_amd.builtin_model(name)
    lo, hi = np.array(model.q_lo, dtype=float), np.array(model.q_hi, dtype=float)
    assert model.nq == model.nv and np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))
    return model, _links(model, nc), lo, hi, None


def _goal_rows(name, model, lo, hi, valid, G, seed):
    """[G][nq] distinct q0 rows inside the limits (multidof: valid rows of the workload, so the quaternion is one)"""
    rng = np.random.default_rng(seed)
    if name == "multidof":
        return np.array(valid[rng.integers(0, valid.shape[0], size=G)]) + 0.0
    return rng.uniform(lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo), size=(G, model.nq))


def _mk(model, B, links, q_init, lo, hi, limits=True, precision=capi.F64):
    s = _handle(model, B, links, q_init, np.tile(np.eye(6), (len(links), 1, 1)), PRM, precision=precision)
    if limits:
        s.set_joint_limits(lo, hi)
    return s


def _pose_fields(s):
    """status, steps, err of the last loikb_solve_pose, per instance"""
    B, nc = s.batch, int(s.L.loikb_num_eq_c(s.h))
    status, steps, err = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32), np.empty((B, nc, 6))
    for f, a in ((capi.POSE_F_STATUS, status), (capi.POSE_F_STEPS, steps), (capi.POSE_F_ERR, err)):
        assert s.L.loikb_pose_get(s.h, f, a.ctypes.data_as(C.c_void_p), 0) == 0
    return status, steps, err


def _rc(fn, *a, **kw):
    """the status a binding call ends with (0: none raised)"""
    try:
        fn(*a, **kw)
    except capi.LoikError as e:
        return e.code
    return 0


# ---- 1. K = 1, R = 1 is SolvePose ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["talos32", "panda7"])
def test_one_seed_one_round_is_solve_pose(name):
    model, links, lo, hi, _ = _robot(name)
    G = 193
    q0, tg = _seeds(model, G, links, seed=40)
    q0 = np.clip(q0, lo, hi)
    a, b = _mk(model, G, links, q0, lo, hi), _mk(model, G, links, q0, lo, hi)
    out = a.SolvePoseMultiStart(tg, 1, q0=q0, tol_pose=TOL, max_steps=2)   # (two steps: some seeds need a third)
    ref = b.SolvePose(tg, tol_pose=TOL, max_steps=2, q=q0)
    status, steps, err = _pose_fields(a)
    qa, qb = a.get("q"), b.get("q")
    a.close(); b.close()
    assert np.array_equal(qa, qb) and np.array_equal(status, ref["status"]) and np.array_equal(steps, ref["steps"])
    assert np.array_equal(err, ref["err"])
    assert np.any(steps > 0) and np.any(ref["reached"]) and not np.all(ref["reached"])
    assert np.array_equal(out["winner"], np.arange(G)) and out["rounds_run"] == 1 and np.array_equal(out["q"], qa)
    assert np.array_equal(out["round"], np.zeros(G, dtype=np.int32))


# ---- 2. the sampler, bit for bit ---------------------------------------------------------------------------------------------------
SHAPES = [(1, 5), (3, 70), (2, 64)]


def _check_sampler(name, precision, shapes):
    model, links, lo, hi, valid = _robot(name, 1)
    for G, K in shapes:
        B = G * K
        q0g = _goal_rows(name, model, lo, hi, valid, G, seed=50 + G)
        tg = P.fk12(model, q0g, links)
        s = _mk(model, B, links, np.repeat(q0g, K, axis=0), lo, hi, precision=precision)
        for rnd in (0, 3):
            forms = [("goal", q0g, q0g), ("shared", q0g[0], np.tile(q0g[0], (G, 1)))]
            for form, arg, rows in forms + [("resident", None, None)]:
                if form == "resident":   # the resident q of instance g * K: put known rows there first
                    res = np.repeat(_goal_rows(name, model, lo, hi, valid, G, seed=60 + rnd), K, axis=0)
                    res[1::K] += 0.0625 if K > 1 else 0.0   # (the rows of the other seeds must not be the ones that are read)
                    s.SolvePose(np.repeat(tg, K, axis=0), max_steps=0, q=res)
                    rows = res[::K]
                s.sample_seeds(K, seed=SEED + G, round=rnd, q0=arg)
                q = s.get("q")
                want = M.sample(model, rows, K, SEED + G, rnd, lo, hi)
                what = (name, G, K, rnd, form)
                assert np.array_equal(q, want), (what, np.argwhere(q != want)[:4])
                _, cols = M.sampled_dofs(model, lo, hi)
                rest = np.setdiff1d(np.arange(model.nq), cols)
                assert np.array_equal(q[:, rest], np.repeat(rows, K, axis=0)[:, rest]), what
                assert np.all(q[:, cols] >= lo[np.isfinite(lo) & np.isfinite(hi)]) and np.all(q[:, cols] <= hi[np.isfinite(lo) & np.isfinite(hi)])
                if rnd == 0:
                    assert np.array_equal(q[::K], rows), what
                elif cols.size:
                    assert np.all(q[::K][:, cols] != rows[:, cols]), what
                if name == "multidof":   # the free-flyer's translation and quaternion are the goal's q0, exactly
                    iq = int(model.idx_q[[int(t) for t in model.jtype].index(9)])
                    assert iq not in cols and np.array_equal(q[:, iq:iq + 7], np.repeat(rows, K, axis=0)[:, iq:iq + 7]), what
        s.close()


@pytest.mark.parametrize("name", ["panda7", "talos32", "multidof"])
def test_sampler_matches_numpy_bit_for_bit(name):
    _check_sampler(name, capi.F64, SHAPES)


def test_sampler_on_an_f32_handle_is_fp64():
    _check_sampler("panda7", capi.F32, [(3, 70)])


# ---- 3. / 5. one round: the loop against SolvePose on the numpy seeds, the selection against numpy --------------------------------
def _check_selection(s, out, q0g, K, pick, weights, model, what):
    """winner / goal_status / nreached / cost / the winner's rows of `out` against the numpy rule on the handle's own fields"""
    status, _, err = _pose_fields(s)
    q = s.get("q")
    o = M.select(status, err, q, q0g, K, pick, PL.limit_q_index(model), weights)
    clear = o["margin"] > 1e-9
    print("multistart_measured %s | goals %d clear %d | status %s | nreached %s" % (what, clear.size, int(clear.sum()),
                                                                                   o["goal_status"].tolist(), o["nreached"].tolist()))
    assert np.array_equal(out["winner"][clear], o["winner"][clear]), what
    assert np.array_equal(out["goal_status"], o["goal_status"]) and np.array_equal(out["nreached"], o["nreached"]), what
    cls, cost = M.instance_keys(status, err, q, q0g, K, pick, PL.limit_q_index(model), weights)
    w = out["winner"]
    assert np.all(w // K == np.arange(w.size)) and np.array_equal(cls[w], cls[o["winner"]]), what
    ok = ~np.isnan(o["cost"])
    assert np.all(cost[w][ok] <= o["cost"][ok] * (1 + 1e-12)), what          # (the device's winner, costed by numpy)
    assert np.all(np.abs(out["cost"][ok] - cost[w][ok]) <= 1e-12 * cost[w][ok]), what
    assert np.array_equal(out["q"], q[w]) and np.array_equal(out["err"], err[w]), what
    return o


# (robot, G, K, tasks, max_steps: chosen on the CPU oracle so that every goal has reached seeds and seeds that are not, several of each)
# multidof: _robot("multidof", 2) -- nq = 31, nv = 26, both links constrained; the seeds cost through the DoF-to-coordinate table.
# Its sixth entry is the seed of the targets: at that seed and max_steps = 6 the oracle has 28, 25 and 15 of the 64 seeds of the three
# goals reached
LOOP_CASES = [("talos32", 3, 70, True, 3), ("panda7", 6, 16, False, 12), ("multidof", 3, 64, False, 6, 75)]


def _multidof_targets(model, lo, hi, valid, G, seed, rng):
    """FK of valid rows (unit quaternion and (cos, sin) pairs) whose sampled coordinates are redrawn inside their ranges"""
    q_t = _goal_rows("multidof", model, lo, hi, valid, G, seed=seed)
    j, c = M.sampled_dofs(model, lo, hi)
    q_t[:, c] = rng.uniform(lo[j], hi[j], size=(G, j.size))
    return q_t


@pytest.mark.parametrize("case", LOOP_CASES, ids=lambda c: "%s-G%d-K%d%s" % (c[0], c[1], c[2], "-tasks" if c[3] else ""))
def test_one_round_matches_solve_pose_on_the_numpy_seeds(case):
    name, G, K, tasks, max_steps = case[:5]
    nc = 2 if tasks or name == "multidof" else 1
    model, links, lo, hi, valid = _robot(name, nc)
    B = G * K
    rng = np.random.default_rng(70 + G)
    q0g = _goal_rows(name, model, lo, hi, valid, G, seed=71)
    q_t = _multidof_targets(model, lo, hi, valid, G, case[5], rng) if name == "multidof" else rng.uniform(lo, hi, size=(G, model.nq))
    frames = T.random_frames(rng, nc) if tasks else None
    tg = T.frame_fk12(model, q_t, links, frames) if tasks else P.fk12(model, q_t, links)
    q_init = np.repeat(q0g, K, axis=0)
    a, b = _mk(model, B, links, q_init, lo, hi), _mk(model, B, links, q_init, lo, hi)
    if tasks:
        a.set_pose_tasks(["position", "orientation"], frames)
        b.set_pose_tasks(["position", "orientation"], frames)
    weights = rng.uniform(0.2, 3.0, size=model.nv)
    a.set_seed_ranges(weights=weights)
    kw = dict(tol_pose=TOL, max_steps=max_steps)
    out = a.SolvePoseMultiStart(tg, K, seed=SEED, q0=q0g, **kw)
    seeds = M.sample(model, q0g, K, SEED, 0, lo, hi)
    ref = b.SolvePose(np.repeat(tg, K, axis=0), q=seeds, **kw)
    status, steps, err = _pose_fields(a)
    assert np.array_equal(a.get("q"), b.get("q")) and np.array_equal(status, ref["status"]) and np.array_equal(steps, ref["steps"])
    assert np.array_equal(err, ref["err"])
    assert out["rounds_run"] == 1 and not out["round"].any()
    assert np.any(ref["reached"]) and not np.all(ref["reached"]), ref["reached"].mean()
    _check_selection(a, out, q0g, K, M.PICK_NEAREST, weights, model, (case, "nearest"))
    out = a.SolvePoseMultiStart(tg, K, seed=SEED, q0=q0g, pick="first", **kw)
    o = _check_selection(a, out, q0g, K, M.PICK_FIRST, weights, model, (case, "first"))
    assert np.array_equal(out["winner"], o["winner"]) and not out["cost"][o["goal_status"] == M.GOAL_REACHED].any()
    if name == "multidof":
        # every goal has several seeds that reach and several that do not; out["q"] has nq columns; and with no step taken the
        # winners' free-flyer blocks (never sampled, so moved by the solve alone) are the goals' q0
        reached = ref["reached"].reshape(G, K).sum(axis=1)
        assert np.all(reached >= 3) and np.all(K - reached >= 3), reached
        assert model.nq > model.nv and out["q"].shape == (G, model.nq) and a.get("q").shape == (B, model.nq)
        iq = int(model.idx_q[[int(t) for t in model.jtype].index(9)])
        moved = np.abs(out["q"][:, iq:iq + 7] - q0g[:, iq:iq + 7]).max(axis=1)
        assert np.all((moved > 0) == (steps[out["winner"]] > 0)), (moved, steps[out["winner"]])
        for pick, rule in (("nearest", M.PICK_NEAREST), ("first", M.PICK_FIRST)):
            out0 = a.SolvePoseMultiStart(tg, K, seed=SEED, q0=q0g, pick=pick, tol_pose=TOL, max_steps=0)
            _check_selection(a, out0, q0g, K, rule, weights, model, (case, pick, "no step"))
            assert out0["q"].shape == (G, model.nq) and np.array_equal(out0["q"][:, iq:iq + 7], q0g[:, iq:iq + 7])
            assert np.array_equal(a.get("q"), M.sample(model, q0g, K, SEED, 0, lo, hi))
    a.close(); b.close()


# ---- 4. / 5. three rounds against the host-driven sequence ---------------------------------------------------------------------------
_R3 = {}


def _r3_workload():
    """panda7, (6, 16), few steps: the ORACLE leaves goals unanswered after round 0 and answers more of them later"""
    if not _R3:
        model, links, lo, hi, _ = _robot("panda7")
        G, K, steps = 6, 16, 5
        q_t = np.random.default_rng(101).uniform(lo, hi, size=(G, model.nq))
        tg = P.fk12(model, q_t, links)
        q0g = np.tile(0.5 * (lo + hi), (G, 1))
        lb, ub = _box(model)
        o = M.multistart_loop(model, PRM, q0g, K, 3, SEED, lo, hi, links, np.tile(np.eye(6), (1, 1, 1)), lb, ub, tg, 1.0, 1.0, TOL, steps, lo, hi)
        print("multistart_measured r3 oracle answered per round %s" % o["answered"])
        assert G - o["answered"][0] >= 2 and len(o["answered"]) == 3 and o["answered"][2] > o["answered"][0], o["answered"]
        _R3.update(model=model, links=links, lo=lo, hi=hi, G=G, K=K, steps=steps, tg=tg, q0g=q0g)
    return _R3


def _host_driven(w, s, rounds, tg=None, q0g=None):
    """the loop of loikb_solve_pose_multistart from the host on handle s: SolvePose, re-seed the rows without REACHED with the
    numpy sampler, SolvePose(q = ...), ...  Returns (q, round [B], rounds run)"""
    model, G, K, lo, hi = w["model"], w["G"], w["K"], w["lo"], w["hi"]
    tg = w["tg"] if tg is None else tg
    q0g = w["q0g"] if q0g is None else q0g
    q = M.sample(model, q0g, K, SEED, 0, lo, hi)
    rnd = np.zeros(G * K, dtype=np.int32)
    for r in range(rounds):
        out = s.SolvePose(np.repeat(tg, K, axis=0), tol_pose=TOL, max_steps=w["steps"], q=q)
        ok = out["reached"] & ((out["status"] & capi.POSE_ST_STOPPED) == 0)
        if r == rounds - 1 or ok.reshape(G, K).any(axis=1).all():
            return s.get("q"), rnd, r + 1
        q, fresh = M.resample(model, s.get("q"), out["status"], q0g, K, SEED, r + 1, lo, hi)
        rnd[fresh] = r + 1


def test_three_rounds_match_the_host_driven_sequence():
    w = _r3_workload()
    model, links, lo, hi, G, K = w["model"], w["links"], w["lo"], w["hi"], w["G"], w["K"]
    q_init = np.repeat(w["q0g"], K, axis=0)
    a, b = _mk(model, G * K, links, q_init, lo, hi), _mk(model, G * K, links, q_init, lo, hi)
    weights = np.linspace(0.5, 2.0, model.nv)
    a.set_seed_ranges(weights=weights)
    out = a.SolvePoseMultiStart(w["tg"], K, rounds=3, seed=SEED, q0=w["q0g"], tol_pose=TOL, max_steps=w["steps"])
    q, rnd, rounds_run = _host_driven(w, b, 3)
    sa, sb = _pose_fields(a), _pose_fields(b)
    assert np.array_equal(a.get("q"), q) and out["rounds_run"] == rounds_run and np.array_equal(out["round"], rnd)
    assert all(np.array_equal(x, y) for x, y in zip(sa, sb))
    assert rounds_run >= 2 and rnd.max() == rounds_run - 1 and (rnd == 0).any()
    assert out["timing"]["rounds"] == rounds_run and out["timing"]["solve_ms"] > 0
    _check_selection(a, out, w["q0g"], K, M.PICK_NEAREST, weights, model, "r3 nearest")
    out = a.SolvePoseMultiStart(w["tg"], K, rounds=3, seed=SEED, q0=w["q0g"], pick="first", tol_pose=TOL, max_steps=w["steps"])
    _check_selection(a, out, w["q0g"], K, M.PICK_FIRST, weights, model, "r3 first")
    a.close(); b.close()


def test_zero_steps_two_rounds_leave_the_round_one_seeds():
    w = _r3_workload()
    model, links, lo, hi, G, K = w["model"], w["links"], w["lo"], w["hi"], w["G"], w["K"]
    s = _mk(model, G * K, links, np.repeat(w["q0g"], K, axis=0), lo, hi)
    tg = np.array(w["tg"])
    tg[0] = P.fk12(model, w["q0g"][:1], links)[0]   # goal 0's seed 0 (= q0) sits at its target: reached with no step
    out = s.SolvePoseMultiStart(tg, K, rounds=2, seed=SEED, q0=w["q0g"], tol_pose=TOL, max_steps=0)
    status, steps, _ = _pose_fields(s)
    at = (status & capi.POSE_ST_REACHED) != 0
    assert out["rounds_run"] == 2 and at[0] and not at[1:].any() and not steps.any()
    want = M.sample(model, w["q0g"], K, SEED, 1, lo, hi)
    want[at] = M.sample(model, w["q0g"], K, SEED, 0, lo, hi)[at]
    assert np.array_equal(s.get("q"), want) and np.array_equal(out["round"], np.where(at, 0, 1))
    assert out["goal_status"].tolist() == [M.GOAL_REACHED] + [M.GOAL_BEST_EFFORT] * (G - 1) and out["winner"][0] == 0
    s.close()


# ---- 5. the selection's corner cases -------------------------------------------------------------------------------------------------
def test_identical_seeds_tie_to_the_first_instance():
    w = _r3_workload()
    model, links, lo, hi, G, K = w["model"], w["links"], w["lo"], w["hi"], w["G"], w["K"]
    q0 = w["q0g"][0]
    s = _mk(model, G * K, links, np.repeat(w["q0g"], K, axis=0), lo, hi)
    s.set_seed_ranges(q0, q0)   # every seed is q0: the K instances of a goal are the same problem
    for pick in ("nearest", "first"):
        out = s.SolvePoseMultiStart(w["tg"], K, rounds=2, seed=SEED, q0=q0, pick=pick, tol_pose=TOL, max_steps=12)
        q = s.get("q").reshape(G, K, -1)
        assert np.array_equal(q, np.repeat(q[:, :1], K, axis=1))
        assert np.array_equal(out["winner"], np.arange(G) * K), (pick, out["winner"])
        assert np.all((out["nreached"] == 0) | (out["nreached"] == K))
    s.close()


def test_a_far_target_is_best_effort_and_a_nan_goal_fails():
    w = _r3_workload()
    model, links, lo, hi, G, K = w["model"], w["links"], w["lo"], w["hi"], w["G"], w["K"]
    kw = dict(seed=SEED, tol_pose=TOL, max_steps=12)
    s = _mk(model, G * K, links, np.repeat(w["q0g"], K, axis=0), lo, hi)
    base = s.SolvePoseMultiStart(w["tg"], K, q0=w["q0g"], **kw)
    s.close()
    assert (base["goal_status"] == M.GOAL_REACHED).sum() >= 3
    others = np.arange(G) != 2
    # goal 2's target 10 m away
    tg = np.array(w["tg"])
    tg[2, :, 9] += 10.0
    s = _mk(model, G * K, links, np.repeat(w["q0g"], K, axis=0), lo, hi)
    out = s.SolvePoseMultiStart(tg, K, q0=w["q0g"], **kw)
    o = _check_selection(s, out, w["q0g"], K, M.PICK_NEAREST, None, model, "far target")
    s.close()
    assert out["goal_status"][2] == M.GOAL_BEST_EFFORT and out["nreached"][2] == 0 and out["winner"][2] == o["winner"][2]
    assert out["cost"][2] > 5.0
    for f in ("winner", "goal_status", "q", "err", "nreached", "cost"):
        assert np.array_equal(out[f][others], base[f][others]), f
    # goal 2's q0 NaN in a coordinate that is not sampled: every seed of the goal is stopped
    s_lo, s_hi = lo.copy(), hi.copy()
    s_lo[6], s_hi[6] = -np.inf, np.inf
    q0g = np.array(w["q0g"])
    q0g[2, 6] = np.nan
    s = _mk(model, G * K, links, np.repeat(w["q0g"], K, axis=0), lo, hi)
    s.set_seed_ranges(s_lo, s_hi)
    out = s.SolvePoseMultiStart(w["tg"], K, rounds=2, q0=q0g, **kw)
    status, _, _ = _pose_fields(s)
    s.close()
    assert np.all(status.reshape(G, K)[2] & capi.POSE_ST_STOPPED)
    assert out["goal_status"][2] == M.GOAL_FAILED and out["winner"][2] == 2 * K and out["nreached"][2] == 0 and out["cost"][2] == 0.0
    assert not (out["goal_status"][others] == M.GOAL_FAILED).any() and np.all(np.isfinite(out["q"][others]))


# ---- 6. what it is for ---------------------------------------------------------------------------------------------------------------
def test_sixteen_seeds_answer_more_goals_than_one():
    model, links, lo, hi, _ = _robot("panda7")
    G, steps, tol = 24, 10, 1e-6
    q_t = np.random.default_rng(0).uniform(lo, hi, size=(G, model.nq))   # targets: FK of in-range configurations
    tg = P.fk12(model, q_t, links)
    q0g = np.tile(0.5 * (lo + hi), (G, 1))
    lb, ub = _box(model)
    A = np.tile(np.eye(6), (1, 1, 1))
    o1 = M.multistart_loop(model, PRM, q0g, 1, 1, SEED, lo, hi, links, A, lb, ub, tg, 1.0, 1.0, tol, steps, lo, hi)
    o16 = M.multistart_loop(model, PRM, q0g, 16, 1, SEED, lo, hi, links, A, lb, ub, tg, 1.0, 1.0, tol, steps, lo, hi)
    n1, n16 = o1["answered"][-1], o16["answered"][-1]
    assert G - n1 >= 3 and n16 > n1, (n1, n16)
    got = {}
    for K in (1, 16):
        s = _mk(model, G * K, links, np.repeat(q0g, K, axis=0), lo, hi)
        got[K] = s.SolvePoseMultiStart(tg, K, seed=SEED, q0=q0g, tol_pose=tol, max_steps=steps)
        s.close()
    r1, r16 = [(got[K]["goal_status"] == M.GOAL_REACHED) for K in (1, 16)]
    print("multistart_measured goals reached: oracle K=1 %d K=16 %d | device K=1 %d K=16 %d" % (n1, n16, r1.sum(), r16.sum()))
    assert r16.sum() >= r1.sum() and r16.sum() >= n16 - 1
    qw = got[16]["q"]
    e = P.pose_errors(model, qw, links, tg)
    assert np.all(np.abs(e[r16]).max(axis=(1, 2)) <= tol * (1 + 1e-9))
    assert np.all(qw >= lo) and np.all(qw <= hi)


# ---- 7. arguments and state ------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_as_it_was():
    model, links, lo, hi, _ = _robot("panda7")
    G, K = 4, 8
    B = G * K
    q0, tg = _seeds(model, B, links, seed=90)
    q0 = np.clip(q0, lo, hi)
    a, b = _mk(model, B, links, q0, lo, hi), _mk(model, B, links, q0, lo, hi)
    assert _rc(a.multistart_get, "winner") == ERR_STATE
    tgg, q0g = tg[::K], q0[::K]
    bad_R = np.array(tgg)
    bad_R[1, 0, 0] += 1e-3
    nan, inf = np.nan, np.inf
    one = lambda j, v: np.where(np.arange(model.nv) == j, v, 0.0)
    calls = [
        (ERR_ARG, lambda: a.SolvePoseMultiStart(tg[0], 5, q0=q0[0])),                  # B % K != 0 (the binding passes it on)
        (ERR_ARG, lambda: a.SolvePoseMultiStart(tg[0], 0, q0=q0[0])),                  # K < 1
        (ERR_ARG, lambda: a.SolvePoseMultiStart(tgg, K, rounds=0, q0=q0g)),
        (ERR_ARG, lambda: a.SolvePoseMultiStart(tgg, K, pick=2, q0=q0g)),
        (ERR_ARG, lambda: a.SolvePoseMultiStart(tgg, K, pick=-1, q0=q0g)),
        (ERR_ARG, lambda: a.SolvePoseMultiStart(tgg, K, q0=q0g, dt=0.0)),
        (ERR_ARG, lambda: a.SolvePoseMultiStart(bad_R, K, q0=q0g)),                    # a target rotation that is none
        (ERR_ARG, lambda: a.sample_seeds(K, round=-1)),
        (ERR_ARG, lambda: a.sample_seeds(5)),
        (ERR_ARG, lambda: a.sample_seeds(0)),
        (ERR_ARG, lambda: a.set_seed_ranges(lo[:-1], hi[:-1])),                        # n != nv
        (ERR_ARG, lambda: a.set_seed_ranges(lo + one(3, nan), hi)),
        (ERR_ARG, lambda: a.set_seed_ranges(hi, lo)),                                  # s_lo > s_hi
        (ERR_ARG, lambda: a.set_seed_ranges(lo, None)),
        (ERR_ARG, lambda: a.set_seed_ranges(None, hi)),
        (ERR_ARG, lambda: a.set_seed_ranges(lo, hi, -np.ones(model.nv))),
        (ERR_ARG, lambda: a.set_seed_ranges(lo, hi, np.ones(model.nv) + one(2, inf))),
        (ERR_ARG, lambda: a.set_seed_ranges(weights=np.ones(model.nv) + one(2, nan))),
    ]
    ms = capi.MultiStartParams(K, 1, 0, 0, 1)   # flags != 0: only the C entry point can be given one
    prm = capi.PoseParams(1.0, 1.0, TOL, 2, 0)
    t12 = np.ascontiguousarray(tgg)
    calls.append((ERR_ARG, lambda: capi._check(a.L.loikb_solve_pose_multistart(a.h, None, t12.ctypes.data_as(C.c_void_p), 0, C.byref(prm), C.byref(ms)))))
    for k, (code, call) in enumerate(calls):
        assert _rc(call) == code, k
        assert _rc(a.multistart_get, "winner") == ERR_STATE, k
        ra, rb = a.SolvePose(tg, tol_pose=TOL, max_steps=2, q=q0), b.SolvePose(tg, tol_pose=TOL, max_steps=2, q=q0)
        assert np.array_equal(a.get("q"), b.get("q")) and all(np.array_equal(ra[f], rb[f]) for f in ("status", "steps", "err")), k
    # s_lo == s_hi is legal; the ranges that failed above did not replace the joint limits as the default
    a.sample_seeds(K, seed=3, round=2, q0=q0g)
    assert np.array_equal(a.get("q"), M.sample(model, q0g, K, 3, 2, lo, hi))
    a.set_seed_ranges(lo, lo)
    a.sample_seeds(K, seed=3, round=2, q0=q0g)
    assert np.array_equal(a.get("q"), np.tile(lo, (B, 1)))
    a.close(); b.close()


def test_state_errors():
    model, links, lo, hi, _ = _robot("panda7")
    G, K = 4, 8
    B = G * K
    q0, tg = _seeds(model, B, links, seed=91)
    fresh = loik_amd.BatchedLoik(model, B, **dict(PRM, num_eq_c=1))   # no SolveInit yet
    fresh.set_seed_ranges(lo, hi)
    assert _rc(fresh.sample_seeds, K, q0=q0[::K]) == ERR_STATE
    ms, prm, t12 = capi.MultiStartParams(K, 1, 0, 0, 0), capi.PoseParams(1.0, 1.0, TOL, 2, 0), np.ascontiguousarray(tg[::K])
    q12 = np.ascontiguousarray(q0[::K])
    assert fresh.L.loikb_solve_pose_multistart(fresh.h, q12.ctypes.data_as(C.c_void_p), t12.ctypes.data_as(C.c_void_p), 0, C.byref(prm),
                                               C.byref(ms)) == ERR_STATE
    fresh.close()
    # nothing to sample: no limits and no ranges, then ranges without a finite pair, then one-sided pairs only
    a, b = _mk(model, B, links, q0, lo, hi, limits=False), _mk(model, B, links, q0, lo, hi, limits=False)
    inf = np.full(model.nv, np.inf)
    for setup in (lambda: None, lambda: a.set_seed_ranges(-inf, inf), lambda: a.set_seed_ranges(lo, inf)):
        setup()
        assert _rc(a.sample_seeds, K, q0=q0[::K]) == ERR_STATE
        assert _rc(a.sample_seeds, 1, round=1) == ERR_STATE
        assert _rc(a.SolvePoseMultiStart, tg[::K], K, q0=q0[::K]) == ERR_STATE
        assert _rc(a.SolvePoseMultiStart, tg, 1, rounds=2) == ERR_STATE
        ra, rb = a.SolvePose(tg, tol_pose=TOL, max_steps=2, q=q0), b.SolvePose(tg, tol_pose=TOL, max_steps=2, q=q0)
        assert np.array_equal(a.get("q"), b.get("q")) and np.array_equal(ra["status"], rb["status"])
    # K = 1, R = 1 needs no range at all
    out = a.SolvePoseMultiStart(tg, 1, q0=q0, tol_pose=TOL, max_steps=2)
    rb = b.SolvePose(tg, tol_pose=TOL, max_steps=2, q=q0)
    assert np.array_equal(a.get("q"), b.get("q")) and np.array_equal(out["winner"], np.arange(B))
    a.close(); b.close()


def test_a_range_on_a_free_flyer_dof_is_refused_by_name():
    model, links, lo, hi, valid = _robot("multidof", 2)
    s = _mk(model, 8, links, valid, lo, hi)
    iv = int(model.idx_v[[int(t) for t in model.jtype].index(9)])
    s_lo, s_hi = lo.copy(), hi.copy()
    s_lo[iv + 4], s_hi[iv + 4] = -1.0, 1.0
    assert _rc(s.set_seed_ranges, s_lo, s_hi) == ERR_ARG
    msg = s.L.loikb_last_error().decode()
    assert "DoF %d " % (iv + 4) in msg and "free-flyer" in msg, msg
    s.sample_seeds(4, seed=1, round=1)   # the limits are still the ranges
    s.close()
