"""GPU: the step mode of k_avoid_box (include/loik_amd_avoid.h) on every route a pose loop can hand it -- the three places the step's
interval comes from (the home tiles after k_pose_limit_box / k_pose_dyn_box, the shared base box, the per-instance base box), ragged
batches whose last workgroup holds idle wavefronts, the per-instance base box coming back, exact containment of z without limits on
every engine, and the loops beside SolvePose: SolvePosePath with a budget (its loop-private status word), TrackPose with feed-forward,
step control and a multi-start of three rounds.

The referees are the lock-step oracles of tests/*_numpy.py with the `narrow` hook of avoid_numpy.narrower; the gates are the ones
the corresponding tests already use (test_pose_parity._gate: the same reached / steps on >= 99 % -- at B <= 16 that is all of them --
and |dq| < 1e-7; a 1 % flag share; 1e-7 on avoid_min_seen; exact where stated).  Every input is built by a function of this file that
needs no GPU, and tests/test_avoid_routes_numpy.py asserts on the oracle alone the conditions that make each case mean something."""
import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from test_engines import ENGINES
from test_pose_ik import BOUND, PRM, _fk_models, _links
from test_pose_parity import ENGINE_ENV, _box, _gate, _handle, _leaf_and_multidof, _nonsym_A, _seeds
from test_avoid_pose import AVOID, LAWS, TOL, WALL, WALL_DT, WALL_GAIN, _latched, _wall_case
import test_avoid_pose as TP
import avoid_numpy as AN
import clearance_numpy as CN
import pose_accel_numpy as PA
import pose_limits_numpy as PL
import pose_multistart_numpy as M
import pose_numpy as P
import pose_path_numpy as PP
import pose_step_numpy as PS
import pose_track_numpy as TR
import test_clearance as TC

pytestmark = pytest.mark.gpu

B_MAX = 16
RESULTS = ("avoid_min_seen", "avoid_active_steps", "avoid_flags")
_WORK, _ORACLE = {}, {}


# ---- the inputs (no GPU) ---------------------------------------------------------------------------------------------------------
def _robot(name):
    if name == "multidof":
        model = _fk_models()[3]
        return model, _leaf_and_multidof(model)
    model = loik_amd.builtin_model(name)
    return model, _links(model, 1)


def _collision(model, rng, seed):
    lk, spheres = CN.make_spheres(model, 1, seed)
    ws, wb = TC._world(rng, 6, 5)
    return dict(links=lk, spheres=spheres, ws=ws, wb=wb, pairs=CN.self_pairs(model.parents, lk))


def _inst_box(rng, B, nv, f32):
    """the seeded [B][nv] box of test_pose_limits._workload: uniform(0.5, 2) BOUND on each side, asymmetric; f32: drawn on the fp32 grid,
    so that an fp32 handle holds the very numbers the test clamps with"""
    w = rng.uniform(0.5, 2.0, size=(2, B, nv)) * BOUND
    if f32:
        w = w.astype(np.float32).astype(np.float64)
    return -w[0], w[1]


def route_workload(name, variant, box_inst, a_inst=False, B=B_MAX, seed=0, f32_box=False):
    """test_avoid_pose._workload with the route as a parameter: variant 0 no limits, 1 binding position limits, 2 position and
    acceleration limits; the base box shared (BOUND) or per instance (_inst_box); A shared or per instance"""
    key = ("route", name, variant, box_inst, a_inst, B, seed, f32_box)
    if key in _WORK:
        return _WORK[key]
    model, links = _robot(name)
    rng = np.random.default_rng(seed)
    A = _nonsym_A(rng, len(links), B if a_inst else None)
    q0, tg = _seeds(model, B, links, seed=seed + 1, spread=(1e-5, 0.3))
    q_lo, q_hi = -np.inf * np.ones(model.nv), np.inf * np.ones(model.nv)
    a_max = None
    if variant >= 1:
        q_t = model.random_configurations(np.random.default_rng(seed + 1), B)   # (what _seeds drew the targets from)
        q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, seed + 2, (10.0, 90.0))
    if variant == 2:
        a_max = PA.accel_limits(model, seed + 3, 0.25, BOUND, lo=0.05, hi=0.5)
    col = _collision(model, rng, seed + 4)
    box = _inst_box(rng, B, model.nv, f32_box) if box_inst else _box(model)
    _WORK[key] = dict(model=model, links=links, A=A, q0=q0, tg=tg, q_lo=q_lo, q_hi=q_hi, a_max=a_max, box=box, B=B, col=col)
    return _WORK[key]


# a. (robot, variant, per-instance box, per-instance A, seed): {shared, per-instance} x {none, position, position + acceleration} minus
# the two of test_avoid_pose.PARITY_CASES; the seeds are the first for which the oracle alone meets the conditions of
# test_avoid_routes_numpy.test_route_matrix_inputs on both laws and both step counts
ROUTES = [
    ("panda7", 1, False, False, 2000),
    ("panda7", 0, True, True, 2010),
    ("panda7", 1, True, False, 2020),
    ("panda7", 2, True, True, 2030),
    ("multidof", 1, False, True, 2040),
    ("multidof", 0, True, False, 2050),
    ("multidof", 1, True, True, 2060),
    ("multidof", 2, True, False, 2070),
]
ROUTE_STEPS = (1, 4)


def route_id(c):
    return "%s-%s-%s-%s" % (c[0], ("nolimits", "limits", "limits-accel")[c[1]], "boxinst" if c[2] else "boxsh", "Ainst" if c[3] else "Ash")


def route_case(c):
    return route_workload(c[0], c[1], c[2], c[3], B_MAX, c[4])


# b. (B, per-instance box, seed): 5 leaves three idle wavefronts in the last workgroup of CLR_WAVES = 4, 13 one, 1 is one live wavefront
RAGGED = [(1, False, 2101), (5, False, 2110), (13, False, 2120), (1, True, 2131), (5, True, 2140), (13, True, 2150)]
RAGGED_LAW, RAGGED_STEPS = LAWS[0], 4


def ragged_case(c):
    return route_workload("panda7", 0, c[1], False, c[0], c[2])


def decision_margin(w, o, tol=TOL):
    """the least relative distance of max |e| from tol over every step-start configuration of the oracle's run (q_path, the final one
    included): the reached / steps decisions of the loop"""
    worst = np.inf
    for b, path in enumerate(o["q_path"]):
        e = np.abs(P.pose_errors(w["model"], path, w["links"], np.repeat(w["tg"][b:b + 1], len(path), axis=0))).max(axis=(1, 2))
        worst = min(worst, float(np.min(np.abs(e - tol) / tol)))
    return worst


# c. / d. the per-instance and the shared box without limits, on the fp32 grid
BACK_SEED, BACK_STEPS, BACK_LAW = 2200, 4, (0.25, 1.0)   # (gain 1: most instances reach within the loop, at different steps)
# a reference velocity that is not zero: the idle b = 0 solves of an instance that has reached then have an optimum away from 0, which
# the box decides -- the base box k_avoid_box puts back, not the narrowed box of the instance's last step
BACK_VREF = 0.5 * np.array([0.3, -0.5, 0.8, 1.0, -0.7, 0.4])
CONTAIN_SEED, CONTAIN_CALLS, CONTAIN_LAW = 2311, 3, LAWS[1]


def back_case():
    return route_workload("panda7", 0, True, False, B_MAX, BACK_SEED, f32_box=True)


def back_oracle():
    """lockstep_pose_loop_avoid with BACK_VREF, plus idle [B] (reached before the last step, after at least one) and outside [B]: by how
    much the final z of an idle instance, which its idle solves found in the base box, lies outside the narrowed box of its last step"""
    if "back" not in _ORACLE:
        w, c = back_case(), back_case()["col"]
        dt, gain = BACK_LAW
        lb, ub = w["box"]
        o = AN.lockstep_pose_loop_avoid(w["model"], PRM, w["q0"], np.eye(6), BACK_VREF, w["links"], w["A"], lb, ub, w["tg"], dt, gain, TOL, BACK_STEPS,
                                        w["q_lo"], w["q_hi"], w["col"], AVOID)
        idle = o["reached"] & (o["steps"] > 0) & (o["steps"] < BACK_STEPS)
        outside = np.zeros(w["B"])
        for b in np.flatnonzero(idle):
            box = AN.avoidance_box(w["model"], o["q_path"][b][-2][None], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], dt, lb[b], ub[b], **AVOID)
            outside[b] = max(0.0, float(np.maximum(box["lo"][0] - o["z"][b], o["z"][b] - box["hi"][0]).max()))
        _ORACLE["back"] = dict(o, idle=idle, outside=outside)
    return _ORACLE["back"]


def resting_on_narrowed(w, law):
    """how many entries of the oracle's z of the first step rest (within 1e-9: the inner solve's tolerance) on a narrowed side that is not 0"""
    lo_hi = resting_entries(w, law, sides=True)
    return int(lo_hi[0].sum() + lo_hi[1].sum())


def resting_entries(w, law, sides=False):
    """[B][nv] bool: the entries resting_on_narrowed counts (`sides`: those on the lower and those on the upper side, apart)"""
    dt, gain = law
    o, c, nv = TP._oracle(w, dt, gain, 1), w["col"], w["model"].nv
    lb, ub = (np.broadcast_to(x, (w["B"], nv)) for x in w["box"])
    box = AN.avoidance_box(w["model"], w["q0"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], dt, -np.inf * np.ones(nv), np.inf * np.ones(nv), **AVOID)
    lo, hi = np.minimum(np.maximum(box["lo"], lb), ub), np.minimum(np.maximum(box["hi"], lb), ub)
    ran = (o["steps"] == 1)[:, None]
    on_lo, on_hi = (np.abs(o["z"] - lo) < 1e-9) & (lo > lb) & (lo != 0.0) & ran, (np.abs(o["z"] - hi) < 1e-9) & (hi < ub) & (hi != 0.0) & ran
    return (on_lo, on_hi) if sides else on_lo | on_hi


def contain_case(box_inst):
    return route_workload("panda7", 0, box_inst, False, B_MAX, CONTAIN_SEED, f32_box=True)


# e. SolvePosePath: (robot, limits, seed); T = 3 waypoints, a budget of 2 steps a waypoint, 6 steps
PATHS = [("panda7", False, 2400), ("panda7", True, 2410), ("multidof", False, 2420), ("multidof", True, 2430)]
PATH_T, PATH_STEPS, PATH_BUDGET, PATH_LAW = 3, 6, 2, (1.0, 1.0)


def path_workload(name, limits, seed):
    key = ("path", name, limits, seed)
    if key not in _WORK:
        from test_pose_path import _path_workload
        model, links = _robot(name)
        rng = np.random.default_rng(seed)
        A = _nonsym_A(rng, len(links))
        q0, wp, q_t = _path_workload(model, links, B_MAX, PATH_T, seed=seed + 1, spread=(1e-2, 0.3))
        q_lo = q_hi = None
        if limits:
            q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, seed + 2, (10.0, 90.0))
        _WORK[key] = dict(model=model, links=links, A=A, q0=q0, wp=wp, q_lo=q_lo, q_hi=q_hi, box=_box(model), B=B_MAX, col=_collision(model, rng, seed + 4))
    return _WORK[key]


def _recorded(hook, B):
    """the hook, keeping per instance whether each of its calls narrowed"""
    calls = [[] for _ in range(B)]

    def f(b, q_b, lo, hi):
        out = hook(b, q_b, lo, hi)
        calls[b].append(bool(hook.results["avoid_flags"][b].any()))
        return out

    f.results, f.calls = hook.results, calls
    return f


def _limit_kw(w):
    return dict(q_lo=w["q_lo"], q_hi=w["q_hi"]) if w["q_lo"] is not None else {}


def path_oracle(w):
    key = ("path", id(w))
    if key not in _ORACLE:
        dt, gain = PATH_LAW
        hook = _recorded(AN.narrower(w["model"], w["col"], AVOID, dt, w["B"]), w["B"])
        lb, ub = w["box"]
        o = PP.lockstep_path_loop(w["model"], PRM, w["q0"], np.eye(6), np.zeros(6), w["links"], w["A"], lb, ub, w["wp"], dt, gain, TOL, PATH_STEPS,
                                  budget=PATH_BUDGET, narrow=hook, **_limit_kw(w))
        o.update(hook.results, calls=hook.calls)
        _ORACLE[key] = o
    return _ORACLE[key]


# f. TrackPose: (robot, limits, seed); T = 4 steps, FF_DIFFERENCE
TRACKS = [("panda7", False, 2500), ("panda7", True, 2510), ("multidof", False, 2520), ("multidof", True, 2530)]
TRACK_T, TRACK_LAW, TRACK_TOL = 4, (0.25, 0.5), 1e-4


def track_workload(name, limits, seed):
    key = ("track", name, limits, seed)
    if key not in _WORK:
        from test_pose_track import _track_workload
        model, links = _robot(name)
        rng = np.random.default_rng(seed)
        A = _nonsym_A(rng, len(links))
        q0, smp, q_path = _track_workload(model, links, B_MAX, TRACK_T, seed=seed + 1)
        q_lo = q_hi = None
        if limits:
            q_lo, q_hi, q0 = PL.binding_limits(model, q_path[:, TRACK_T], q0, seed + 2, (10.0, 90.0))
        _WORK[key] = dict(model=model, links=links, A=A, q0=q0, smp=smp, q_lo=q_lo, q_hi=q_hi, box=_box(model), B=B_MAX, col=_collision(model, rng, seed + 4))
    return _WORK[key]


def track_oracle(w):
    key = ("track", id(w))
    if key not in _ORACLE:
        dt, gain = TRACK_LAW
        hook = AN.narrower(w["model"], w["col"], AVOID, dt, w["B"])
        lb, ub = w["box"]
        o = TR.lockstep_track_loop(w["model"], PRM, w["q0"], np.eye(6), np.zeros(6), w["links"], w["A"], lb, ub, w["smp"], dt, gain, TRACK_TOL,
                                   ff=TR.FF_DIFFERENCE, narrow=hook, **_limit_kw(w))
        o.update(hook.results)
        _ORACLE[key] = o
    return _ORACLE[key]


def wall_track_case():
    """the first B_MAX instances of test_avoid_pose._wall_case and TRACK_T + 1 samples on the straight joint-space line through the wall"""
    if "walltrack" not in _WORK:
        w = _wall_case()
        B, T = B_MAX, TRACK_T
        qs = np.stack([[P.integrate(w["model"], w["q0"][b], (k / T) * TP._way(w, b)) for k in range(T + 1)] for b in range(B)])
        smp = P.fk12(w["model"], qs.reshape(-1, w["model"].nq), w["links"]).reshape(B, T + 1, len(w["links"]), 12)
        # (a handle checks the self pairs of its spheres as well: the oracle of this case is told of them, test_avoid_pose's is not)
        col = dict(w["col"], pairs=CN.self_pairs(w["model"].parents, w["col"]["links"]))
        _WORK["walltrack"] = dict(w, B=B, q0=w["q0"][:B], tg=w["tg"][:B], smp=smp, q_lo=None, q_hi=None, col=col)
    return _WORK["walltrack"]


def wall_track_oracle():
    if "walltrack" not in _ORACLE:
        w = wall_track_case()
        hook = AN.narrower(w["model"], w["col"], WALL, WALL_DT, w["B"])
        lb, ub = w["box"]
        o = TR.lockstep_track_loop(w["model"], PRM, w["q0"], np.eye(6), np.zeros(6), w["links"], w["A"], lb, ub, w["smp"], WALL_DT, WALL_GAIN, 1e-3,
                                   ff=TR.FF_DIFFERENCE, narrow=hook)
        o.update(hook.results)
        _ORACLE["walltrack"] = o
    return _ORACLE["walltrack"]


# g. step control at gain 2.5 (test_pose_step.test_rescue_at_gain_2p5): (robot, seed, control); the last one stalls with a constraint active
STEP_GAIN, STEP_DT, STEP_STEPS, STEP_MARGIN = 2.5, 1.0, 4, 1e-2
STEP_CASES = [("panda7", 2603, dict(PS.DEFAULTS)), ("multidof", 2610, dict(PS.DEFAULTS)),
              ("panda7", 2620, dict(PS.DEFAULTS, max_backtracks=0, patience=2))]


def step_id(c):
    return "%s-%s" % (c[0], "patience%d" % c[2]["patience"] if c[2]["patience"] else "defaults")


def step_workload(name, seed):
    key = ("step", name, seed)
    if key not in _WORK:
        model, links = _robot(name)
        rng = np.random.default_rng(seed)
        A = _nonsym_A(rng, len(links))
        q0, tg = _seeds(model, B_MAX, links, seed=seed + 1, spread=(1e-3, 0.3))
        inf = np.inf * np.ones(model.nv)
        _WORK[key] = dict(model=model, links=links, A=A, q0=q0, tg=tg, q_lo=-inf, q_hi=inf, a_max=None, box=_box(model), B=B_MAX,
                          col=_collision(model, rng, seed + 4))
    return _WORK[key]


def step_oracle(w, ctl):
    key = ("step", id(w), tuple(sorted(ctl.items())))
    if key not in _ORACLE:
        hook = AN.narrower(w["model"], w["col"], AVOID, STEP_DT, w["B"])
        lb, ub = w["box"]
        o = PS.lockstep_pose_loop_step(w["model"], PRM, w["q0"], np.eye(6), np.zeros(6), w["links"], w["A"], lb, ub, w["tg"], STEP_DT, STEP_GAIN, TOL,
                                       STEP_STEPS, narrow=hook, **ctl)
        o.update(hook.results)
        _ORACLE[key] = o
    return _ORACLE[key]


# h. the multi-start: G = 4 goals of K = 4 seeds, three rounds of 4 steps
MS_SEED, MS_G, MS_K, MS_ROUNDS, MS_STEPS, MS_DRAW = 2700, 4, 4, 3, 4, 7


def multistart_workload():
    """panda7 with its own joint limits; goal g < 3 has its target next to a seed that round g draws for it (not the goal's q0), so that it
    is answered in round g and not before -- the oracle says whether it is -- and goal 3 has a target no seed is near"""
    if "ms" not in _WORK:
        model, links = _robot("panda7")
        lo, hi = np.array(model.q_lo, dtype=float), np.array(model.q_hi, dtype=float)
        rng = np.random.default_rng(MS_SEED)
        G, K = MS_G, MS_K
        q0g = np.tile(0.5 * (lo + hi), (G, 1))
        near = np.stack([M.sample(model, q0g, K, MS_DRAW, min(g, 2), lo, hi)[g * K + 1 + g % (K - 1)] for g in range(G)])
        q_t = np.clip(near + 0.05 * rng.uniform(-1.0, 1.0, size=near.shape), lo, hi)
        q_t[3] = rng.uniform(lo, hi)
        _WORK["ms"] = dict(model=model, links=links, lo=lo, hi=hi, G=G, K=K, B=G * K, steps=MS_STEPS, q0g=q0g, tg=P.fk12(model, q_t, links),
                           A=np.tile(np.eye(6), (1, 1, 1)), box=_box(model), col=_collision(model, rng, MS_SEED + 4))
    return _WORK["ms"]


def multistart_oracle(w=None):
    """pose_multistart_numpy.multistart_loop with lockstep_pose_loop_avoid as the round: dict(q, round, rounds_run, answered, last = the
    last round's result); of multistart_workload(), or of that workload with another collision model"""
    w = multistart_workload() if w is None else w
    key = ("ms", id(w))
    if key not in _ORACLE:
        model, G, K, lo, hi = w["model"], w["G"], w["K"], w["lo"], w["hi"]
        lb, ub = w["box"]
        tg = np.repeat(w["tg"], K, axis=0)
        q = M.sample(model, w["q0g"], K, MS_DRAW, 0, lo, hi)
        rnd, answered = np.zeros(G * K, dtype=np.int32), []
        for r in range(MS_ROUNDS):
            o = AN.lockstep_pose_loop_avoid(model, PRM, q, np.eye(6), np.zeros(6), w["links"], w["A"], lb, ub, tg, 1.0, 1.0, TOL, MS_STEPS, lo, hi, w["col"], AVOID)
            ok = o["reached"] & ((o["status"] & P.POSE_STOPPED) == 0)
            answered.append(int(ok.reshape(G, K).any(axis=1).sum()))
            if r == MS_ROUNDS - 1 or answered[-1] == G:
                break
            q, fresh = M.resample(model, o["q"], o["status"], w["q0g"], K, MS_DRAW, r + 1, lo, hi)
            rnd[fresh] = r + 1
        _ORACLE[key] = dict(q=o["q"], round=rnd, rounds_run=len(answered), answered=answered, last=o)
    return _ORACLE[key]


# ---- what the tests share ----------------------------------------------------------------------------------------------------------
def _arm(s, w, avoid=AVOID):
    c = w["col"]
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    TP._latch_grid(s, c)
    if avoid is not None:
        s.set_collision_avoidance(**avoid)
    return s


def _loop_handle(w, avoid=AVOID, precision=capi.F64, **kw):
    """a handle on a path / track workload (q_lo None: no limits)"""
    s = _arm(_handle(w["model"], w["B"], w["links"], w["q0"], w["A"], PRM, precision=precision, box=w["box"], **kw), w, avoid)
    if w.get("q_lo") is not None and np.isfinite(w["q_lo"]).any():
        s.set_joint_limits(w["q_lo"], w["q_hi"])
    return s


def _assert_results(out, o, keep, same, what, exact=False):
    """the three avoidance results on the instances keep[same]: active steps equal, min_seen within the gate's 1e-7 (through FK), the flags
    equal but for a 1 % share (a flag is a comparison of two numbers that differ by 1e-7 at most) -- `exact`: on every one"""
    got = {f: out[f][keep][same] for f in RESULTS}
    want = {f: o[f][keep][same] for f in RESULTS}
    bad = (got["avoid_flags"] != want["avoid_flags"]).any(axis=1).mean() if same.any() else 0.0
    assert bad <= (0.0 if exact else 0.01), (what, bad)
    assert np.array_equal(got["avoid_active_steps"], want["avoid_active_steps"]), (what, got["avoid_active_steps"], want["avoid_active_steps"])
    ms, ws = got["avoid_min_seen"], want["avoid_min_seen"]
    assert np.array_equal(np.isinf(ms), np.isinf(ws)), what
    fin = np.isfinite(ws)
    assert np.all(np.abs(ms[fin] - ws[fin]) <= 1e-7), what
    return bad


def _measured(what, out_q, o_q, same, keep, bad, o):
    dq = np.abs(out_q[keep] - o_q[keep]).max(axis=1)
    print("avoid_routes_measured %s | max |q - oracle| %.3e | equal instances %.4f | flag mismatch %.4f | narrowed %.4f | left out %d"
          % (what, dq[same].max() if same.any() else np.nan, same.mean(), bad, (o["avoid_active_steps"] > 0).mean(), int((~keep).sum())))


def _solve_pose_parity(w, dt, gain, k, what, limits, exact=False):
    """the body of test_avoid_pose.test_solve_pose_matches_lockstep_oracle"""
    idx = np.arange(w["B"])
    s = _latched(w, grid=True)   # (a workload of test_gridnear_routes.py names a grid in its collision model; the others none)
    out = s.SolvePose(w["tg"], dt=dt, gain=gain, tol_pose=TOL, max_steps=k)
    q = s.get("q")
    s.close()
    o = TP._oracle(w, dt, gain, k)
    keep = ~o["near"]
    assert (~keep).mean() <= 0.02, (what, o["near"])
    sub = {f: v[keep] for f, v in o.items() if f != "q_path"}
    same = _gate(out, q, sub, idx[keep], what)
    assert np.array_equal(out["status"][keep][same] & 9, sub["status"][same] & 9)
    bad = _assert_results(out, o, keep, same, what, exact)
    if limits:
        assert (out["limit_flags"][keep][same] != sub["limit_flags"][same]).any(axis=1).mean() <= 0.01, what
    _measured(what, q, o["q"], same, keep, bad, o)
    return out, q, o, same


# ---- a. the route matrix ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", LAWS, ids=lambda l: "dt%g-g%g" % l)
@pytest.mark.parametrize("case", ROUTES, ids=route_id)
def test_route_matrix_matches_lockstep_oracle(case, law):
    """every (base box, limits) pair test_avoid_pose.py leaves out: the interval from the tiles after k_pose_limit_box alone, and every
    kernel over the per-instance base box"""
    w = route_case(case)
    for k in ROUTE_STEPS:
        out, q, o, same = _solve_pose_parity(w, law[0], law[1], k, (route_id(case), law, k), case[1] > 0)
        assert (o["avoid_active_steps"] > 0).mean() >= 0.25   # (the condition that makes the case mean something)
        assert np.all(out["avoid_active_steps"] <= out["steps"])


# ---- b. ragged batches -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RAGGED, ids=lambda c: "B%d-%s" % (c[0], "boxinst" if c[1] else "boxsh"))
def test_ragged_batches_store_nothing_past_the_end(case):
    """the idle wavefronts of the last workgroup walk configuration B - 1 and store nothing: at these sizes a share means nothing, so the
    oracle's run has no near instance and no decision near its threshold, and every instance is held to it"""
    w = ragged_case(case)
    dt, gain = RAGGED_LAW
    out, q, o, same = _solve_pose_parity(w, dt, gain, RAGGED_STEPS, ("ragged",) + case[:2], False, exact=True)
    assert not o["near"].any() and same.all()
    assert (o["avoid_active_steps"] > 0).any() and np.all(out["avoid_active_steps"] <= out["steps"])
    assert np.array_equal(out["avoid_flags"], o["avoid_flags"])


# ---- c. the per-instance base box comes back ---------------------------------------------------------------------------------------------
def _back_handle(w, precision, avoid):
    """test_pose_parity._handle with BACK_VREF, armed"""
    nc = len(w["links"])
    s = loik_amd.BatchedLoik(w["model"], w["B"], precision=precision, **dict(PRM, num_eq_c=nc))
    s.SolveInit(w["q0"], np.eye(6), BACK_VREF, np.array(w["links"], dtype=np.int32), w["A"], np.zeros((w["B"], nc, 6)), *w["box"])
    return _arm(s, w, avoid)


@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
def test_per_instance_base_box_comes_back(precision):
    """the route of test_avoid_pose.test_f32_box_is_inside_the_f64_box_and_the_base_box_comes_back with a per-instance box.  In the loop:
    an instance that has reached idles in ITS base box, which k_avoid_box puts back itself -- its idle solves (BACK_VREF: an optimum away
    from 0) end on the oracle's z, outside the narrowed box of its last step.  After it: the latch cleared, a cold start with a b large
    enough that the base box binds, against a twin that never had the latch"""
    w = back_case()
    dt, gain = BACK_LAW
    lb, ub = w["box"]
    s, t = _back_handle(w, precision, AVOID), _back_handle(w, precision, None)
    out = s.SolvePose(w["tg"], dt=dt, gain=gain, tol_pose=TOL, max_steps=BACK_STEPS)
    t.SolvePose(w["tg"], dt=dt, gain=gain, tol_pose=TOL, max_steps=BACK_STEPS)
    q, z = s.get("q"), s.get("z").astype(np.float64)
    assert (out["reached"] & (out["steps"] > 0) & (out["steps"] < BACK_STEPS)).any() and (out["avoid_active_steps"] > 0).any()
    if precision == capi.F64:
        o = back_oracle()
        keep = ~o["near"]
        same = _gate(out, q, {f: o[f][keep] for f in ("reached", "steps", "q")}, np.arange(w["B"])[keep], "base box")
        _assert_results(out, o, keep, same, "base box")
        told = o["idle"][keep][same] & (o["outside"][keep][same] > 1e-4)
        dz = np.abs(z - o["z"])[keep][same].max(axis=1)
        print("avoid_routes_measured base box | idle instances %d, %d of them with z outside their last narrowed box (by %s) | max |z - oracle| on those %.3e"
              % (int(o["idle"].sum()), int(told.sum()), o["outside"][keep][same][told], dz[told].max() if told.any() else np.nan))
        assert told.any() and np.all(dz[told] < 1e-7), dz[told]
    assert not np.array_equal(q, t.get("q"))
    _cold_solve_in_the_base_box(s, t, w, q, dt, gain)
    s.close(); t.close()


def _cold_solve_in_the_base_box(s, t, w, q, dt, gain):
    """s ran with the latch, its twin t never had it: the latch cleared, both put on q and started cold with a b large enough that the
    per-instance base box binds -- z and iter bit-equal, z inside the box and on it in half the instances"""
    lb, ub = w["box"]
    rng = np.random.default_rng(6)
    b = rng.choice([-1.0, 1.0], size=(w["B"], 6)) * (3.0 + rng.random((w["B"], 6)))
    s.clear_collision_avoidance()
    for h in (s, t):
        h.set_warm_start(False)
        h.SolvePose(w["tg"], dt=dt, gain=gain, tol_pose=TOL, max_steps=0, q=q)
        h.UpdateEqConstraint(w["links"][0], b)
        h.Solve(None, -1, None, None)
        h.Solve()
    zs, zt = s.get("z").astype(np.float64), t.get("z").astype(np.float64)
    assert np.array_equal(s.get("iter"), t.get("iter")) and np.array_equal(zs, zt)
    assert np.all(zs >= lb) and np.all(zs <= ub)
    assert ((zs == lb) | (zs == ub)).any(axis=1).mean() >= 0.5, "the per-instance base box does not bind: the test shows nothing"


# ---- d. exact containment without limits -------------------------------------------------------------------------------------------------
def _toward_zero_f32(x):
    """the fp32 number next to the fp64 x on the side of zero (x itself when it is one)"""
    y = x.astype(np.float32)
    return np.where(np.abs(y.astype(np.float64)) > np.abs(x), np.nextafter(y, np.float32(0.0)), y)


def _check_containment(w, precision, what, calls=CONTAIN_CALLS, **kw):
    """SolvePose one step a call: the z of every instance that ran lies in clamp(A, lb_b, ub_b) with A the unclamped interval of the
    query at the configuration before the call, exactly, and the flags are the clamp's"""
    dt, gain = CONTAIN_LAW
    B, nv = w["B"], w["model"].nv
    lb, ub = (np.broadcast_to(x, (B, nv)) for x in w["box"])
    s = _loop_handle(w, precision=precision, **kw)   # (no limits on these workloads: _latched with the engine's options)
    ref = s if precision == capi.F64 else _latched(w, grid=True)   # (the query does not round; an fp64 handle answers it from the same fp64 q)
    inf = np.inf * np.ones(nv)
    q, rests, narrowed, inexact = w["q0"], 0, 0, 0
    for call in range(calls):
        box = ref.avoidance_box(q, dt, -inf, inf, **AVOID)
        lo, hi = np.minimum(np.maximum(box["lo"], lb), ub), np.minimum(np.maximum(box["hi"], lb), ub)
        out = s.SolvePose(w["tg"], dt=dt, gain=gain, tol_pose=TOL, max_steps=1, q=q if call == 0 else None)
        ran = out["steps"] == 1
        z = s.get("z").astype(np.float64)
        assert np.all(z[ran] >= lo[ran]) and np.all(z[ran] <= hi[ran]), (what, call, float(np.maximum(lo - z, z - hi)[ran].max()))
        want = (lo > lb).astype(np.int32) | ((hi < ub).astype(np.int32) << 1)
        assert np.array_equal(out["avoid_flags"][ran], want[ran]), (what, call)
        assert not out["avoid_flags"][~ran].any() and np.array_equal(out["avoid_active_steps"][ran], want[ran].any(axis=1).astype(np.int32))
        on_lo, on_hi = ((want & 1) != 0) & ran[:, None], ((want & 2) != 0) & ran[:, None]
        narrowed += int((on_lo | on_hi).any(axis=1).sum())
        if precision == capi.F32:   # the number the kernel stored is the fp64 bound rounded toward zero
            tl, th = _toward_zero_f32(lo), _toward_zero_f32(hi)
            rests += int(((z == tl) & on_lo).sum() + ((z == th) & on_hi).sum())
            # ... among them the bounds whose nearest fp32 number lies outside the fp64 box: rounding to nearest would let z out
            inexact += int(((z == tl) & on_lo & (lo.astype(np.float32) < lo)).sum() + ((z == th) & on_hi & (hi.astype(np.float32) > hi)).sum())
        else:
            rests += int(((z == lo) & on_lo).sum() + ((z == hi) & on_hi).sum())
        q = s.get("q")
    if ref is not s:
        ref.close()
    s.close()
    print("avoid_routes_measured containment %s | narrowed instance-steps %d | z entries resting on a narrowed side %d" % (what, narrowed, rests))
    assert narrowed > 0 and rests > 0, (what, narrowed, rests)
    if precision == capi.F32:
        print("avoid_routes_measured containment %s | of those, on a bound whose nearest fp32 number is outside the box %d" % (what, inexact))
        assert inexact > 0, what


@pytest.mark.parametrize("box_inst", [False, True], ids=["boxsh", "boxinst"])
@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
def test_z_is_inside_the_clamped_query_exactly(precision, box_inst):
    _check_containment(contain_case(box_inst), precision, ("f64" if precision == capi.F64 else "f32", "boxinst" if box_inst else "boxsh"))


@pytest.mark.parametrize("engine", list(ENGINES))
def test_every_engine_honours_the_narrowed_box(engine, monkeypatch):
    """in the manner of test_pose_limits.test_every_engine_honours_the_step_box (its three-chunk run needs six tiles, more than B <= 16
    gives): an engine that captured the box-sharing mode before the launch would solve in the base box"""
    for v in ENGINE_ENV:
        monkeypatch.delenv(v, raising=False)
    env, kw = ENGINES[engine]
    for v, x in env.items():
        monkeypatch.setenv(v, x)
    _check_containment(contain_case(False), capi.F64, ("engine", engine), calls=2, **kw)


# ---- e. SolvePosePath ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PATHS, ids=lambda c: "%s-%s" % (c[0], "limits" if c[1] else "nolimits"))
def test_path_with_a_budget_matches_the_path_oracle(case):
    """avoid_step is handed the path loop's own status word: an instance the budget stalled is idle, one that reached a waypoint but not
    the last still runs and is narrowed"""
    _check_path(path_workload(*case), case)


def _check_path(w, case):
    from test_pose_path import _path_gate
    dt, gain = PATH_LAW
    s = _loop_handle(w)
    out = s.SolvePosePath(w["wp"], dt=dt, gain=gain, tol_pose=TOL, max_steps=PATH_STEPS, max_steps_per_waypoint=PATH_BUDGET)
    q = s.get("q")
    s.close()
    o = path_oracle(w)
    keep = ~o["near"]
    assert (~keep).mean() <= 0.02, (case, o["near"])
    idx = np.arange(w["B"])[keep]
    sub = {f: (v[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (w["B"],) else v) for f, v in o.items() if f != "calls"}
    same = _path_gate(out, q, sub, idx, case)
    bad = _assert_results(out, o, keep, same, case)
    if case[1]:
        assert (out["limit_flags"][keep][same] != sub["limit_flags"][same]).any(axis=1).mean() <= 0.01, case
    _measured(("path",) + case[:2], q, o["q"], same, keep, bad, o)
    assert (out["path_status"] == PP.PATH_STALLED).any() and (out["path_status"] == PP.PATH_COMPLETE).any()


# ---- f. TrackPose ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TRACKS, ids=lambda c: "%s-%s" % (c[0], "limits" if c[1] else "nolimits"))
def test_track_with_feedforward_matches_the_track_oracle(case):
    _check_track(track_workload(*case), case)


def _check_track(w, case):
    from test_pose_track import _track_gate
    dt, gain = TRACK_LAW
    s = _loop_handle(w)
    out = s.TrackPose(w["smp"], dt=dt, gain=gain, tol_track=TRACK_TOL, feedforward="difference")
    s.close()
    o = track_oracle(w)
    keep = ~o["near"]
    assert (~keep).mean() <= 0.02, (case, o["near"])
    idx = np.arange(w["B"])[keep]
    sub = {f: v[keep] for f, v in o.items()}
    same = _track_gate(out, sub, idx, case)
    with np.errstate(invalid="ignore"):
        dz = np.nan_to_num(np.abs(out["z_traj"][idx] - sub["z_traj"])).max(axis=(1, 2))
    print("avoid_routes_measured track %s | max |z_traj - oracle| %.3e" % (case[:2], dz[same].max() if same.any() else np.nan))
    assert np.all(dz[same] < 1e-7), (case, dz[same].max())   # (the gate's bound on q_traj, on z_traj)
    bad = _assert_results(out, o, keep, same, case)
    if case[1]:
        assert (out["limit_flags"][keep][same] != sub["limit_flags"][same]).any(axis=1).mean() <= 0.01, case
    _measured(("track",) + case[:2], out["q_traj"][:, TRACK_T], o["q"], same, keep, bad, o)


def test_track_through_the_wall_keeps_every_z_inside_the_clamped_query():
    """every recorded z_traj[b, k] lies exactly inside clamp(A(q_traj[b, k]), lb, ub), and z_traj reproduces q_traj"""
    w = wall_track_case()
    B, T, nv = w["B"], TRACK_T, w["model"].nv
    lb, ub = w["box"]
    s = _loop_handle(w, avoid=WALL)
    out = s.TrackPose(w["smp"], dt=WALL_DT, gain=WALL_GAIN, tol_track=1e-3, feedforward="difference")
    qt, zt = out["q_traj"], out["z_traj"]
    assert np.isfinite(qt).all() and np.isfinite(zt).all()
    inf = np.inf * np.ones(nv)
    box = s.avoidance_box(qt[:, :T].reshape(B * T, -1), WALL_DT, -inf, inf, **WALL)
    s.close()
    lo = np.minimum(np.maximum(box["lo"], lb), ub).reshape(B, T, nv)
    hi = np.minimum(np.maximum(box["hi"], lb), ub).reshape(B, T, nv)
    assert np.all(zt >= lo) and np.all(zt <= hi), float(np.maximum(lo - zt, zt - hi).max())
    narrowed = (lo > lb) | (hi < ub)
    assert np.array_equal(out["avoid_active_steps"], narrowed.any(axis=2).sum(axis=1))
    assert np.array_equal(out["avoid_flags"], (lo[:, T - 1] > lb).astype(np.int32) | ((hi[:, T - 1] < ub).astype(np.int32) << 1))
    rests = int((((zt == lo) & (lo > lb)) | ((zt == hi) & (hi < ub))).sum())
    worst = max(np.max(np.abs(P.integrate(w["model"], qt[b, k], WALL_DT * zt[b, k]) - qt[b, k + 1])) for b in range(B) for k in range(T))
    print("avoid_routes_measured wall track | narrowed instance-steps %d | z entries resting on a narrowed side %d | max |integrate(q_k, dt z_k) - q_{k+1}| %.3e"
          % (int(narrowed.any(axis=2).sum()), rests, worst))
    assert narrowed.any(axis=2).any(axis=1).mean() >= 0.5 and rests > 0
    assert worst <= 1e-12, worst   # (test_pose_track._check_trajectories_and_feedforward)
    o = wall_track_oracle()
    keep = ~o["near"]
    dq = np.abs(qt - o["q_traj"]).max(axis=(1, 2))
    assert np.all(dq[keep] < 1e-7), dq
    _assert_results(out, o, keep, np.ones(int(keep.sum()), dtype=bool), "wall track")


# ---- g. step control ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STEP_CASES, ids=step_id)
def test_step_control_with_the_latch_matches_the_step_oracle(case):
    """the narrowed box under the backtracking search; with patience, a search that ends STALLED after the box was narrowed counts in the
    avoidance results (the sentence of loik_amd_avoid.h)"""
    _check_step(step_workload(case[0], case[1]), case)


def _check_step(w, case):
    from test_pose_step import _assert_parity
    name, seed, ctl = case
    s = _latched(w, grid=True)
    s.set_step_control(**ctl)
    out = s.SolvePose(w["tg"], dt=STEP_DT, gain=STEP_GAIN, tol_pose=TOL, max_steps=STEP_STEPS)
    out["q"] = s.get("q")
    s.close()
    o = step_oracle(w, ctl)
    keep = ~o["near"] & ~(o["margin"] < STEP_MARGIN)
    idx = np.arange(w["B"])[keep]
    skip = ("phi", "trial", "phi0")
    sub = {f: v[keep] for f, v in o.items() if f not in skip}
    same = _assert_parity(out, sub, idx, step_id(case))
    bad = _assert_results(out, o, keep, same, step_id(case))
    _measured(("step", step_id(case)), out["q"], o["q"], same, keep, bad, o)
    if ctl["patience"]:
        stalled = out["stalled"] & keep
        assert (stalled & (out["avoid_active_steps"] > out["steps"])).any(), (out["stalled"], out["avoid_active_steps"], out["steps"])
    else:
        assert (out["backtracks"][keep] > 0).any() and ((out["backtracks"] > 0) & (out["avoid_active_steps"] > 0) & keep).any()


# ---- h. the multi-start ---------------------------------------------------------------------------------------------------------------------
def test_multistart_three_rounds_match_the_host_driven_sequence_with_the_latch():
    """test_multistart.test_three_rounds_match_the_host_driven_sequence with the latch on both handles: q, the winners and the three
    avoidance results -- those of the last round -- bit for bit"""
    _check_multistart(multistart_workload())


def _check_multistart(w):
    from test_multistart import _check_selection, _mk, _pose_fields
    model, links, lo, hi, G, K = w["model"], w["links"], w["lo"], w["hi"], w["G"], w["K"]
    q_init = np.repeat(w["q0g"], K, axis=0)
    a, b = _arm(_mk(model, G * K, links, q_init, lo, hi), w), _arm(_mk(model, G * K, links, q_init, lo, hi), w)
    weights = np.linspace(0.5, 2.0, model.nv)
    a.set_seed_ranges(weights=weights)
    out = a.SolvePoseMultiStart(w["tg"], K, rounds=MS_ROUNDS, seed=MS_DRAW, q0=w["q0g"], tol_pose=TOL, max_steps=MS_STEPS)
    # the same loop from the host on b (test_multistart._host_driven, keeping each round's result)
    q = M.sample(model, w["q0g"], K, MS_DRAW, 0, lo, hi)
    rnd, earlier = np.zeros(G * K, dtype=np.int32), np.zeros(G * K, dtype=bool)
    for r in range(MS_ROUNDS):
        ref = b.SolvePose(np.repeat(w["tg"], K, axis=0), tol_pose=TOL, max_steps=MS_STEPS, q=q)
        ok = ref["reached"] & ((ref["status"] & capi.POSE_ST_STOPPED) == 0)
        rounds_run = r + 1
        if r == MS_ROUNDS - 1 or ok.reshape(G, K).any(axis=1).all():
            break
        earlier = ref["reached"].copy()
        q, fresh = M.resample(model, b.get("q"), ref["status"], w["q0g"], K, MS_DRAW, r + 1, lo, hi)
        rnd[fresh] = r + 1
    assert np.array_equal(a.get("q"), b.get("q")) and out["rounds_run"] == rounds_run == MS_ROUNDS and np.array_equal(out["round"], rnd)
    assert all(np.array_equal(x, y) for x, y in zip(_pose_fields(a), _pose_fields(b)))
    for f in RESULTS:
        assert np.array_equal(out[f], ref[f]), f
    o = _check_selection(a, out, w["q0g"], K, M.PICK_NEAREST, weights, model, "avoid routes multistart")
    assert np.array_equal(out["winner"], o["winner"])
    # instances that reached in an earlier round never ran in the last one
    assert earlier.any() and np.all(np.isposinf(out["avoid_min_seen"][earlier])) and not out["avoid_active_steps"][earlier].any()
    assert not out["avoid_flags"][earlier].any()
    assert (out["avoid_active_steps"][~earlier] > 0).any()
    want = multistart_oracle(w)
    assert np.array_equal(out["round"], want["round"]) and np.array_equal(earlier, want["last"]["reached"] & (want["last"]["steps"] == 0))
    a.close(); b.close()
