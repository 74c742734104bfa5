"""GPU: the pose loops with the latch of include/loik_amd_avoid.h -- SolvePose against the lock-step oracle of tests/avoid_numpy.py
(proven on the CPU by test_avoid_numpy.py), a wall that the loops run into without the latch and keep away from with it (SolvePose step
by step, SolvePosePath, TrackPose), SolvePoseMultiStart against SolvePose, the inward rounding of an fp32 handle, and neutrality: a
handle that set and cleared the latch runs what one that never set it runs."""
import ctypes as C

import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from test_pose_ik import BOUND, PRM, _fk_models, _links
from test_pose_parity import _box, _gate, _handle, _leaf_and_multidof, _nonsym_A, _seeds
import avoid_numpy as AN
import clearance_numpy as CN
import pose_accel_numpy as PA
import pose_limits_numpy as PL
import pose_numpy as P
import test_clearance as TC

pytestmark = pytest.mark.gpu

ERR_STATE = -24
TOL = 1e-4
LAWS = [(0.25, 0.5), (2.0, 1.7)]   # (dt, gain) as in test_pose_limits.LAWS
AVOID = dict(d_safe=0.02, d_influence=0.15, kappa=0.5)
B_PARITY = 16
PARITY_CASES = [("panda7", 0), ("talos32", 0), ("multidof", 0), ("panda7", 1)]   # (robot, variant of _workload)
PARITY_STEPS = (1, 4)
_WORK, _ORACLE = {}, {}


def _workload(name, variant):
    """16 seeds next to their targets (test_pose_parity._seeds), a sphere on every link, a world of 6 spheres and 5 boxes and the self
    pairs; variant 1: binding joint limits (pose_limits_numpy.binding_limits) and acceleration limits on half the DoFs beside them"""
    key = (name, variant)
    if key in _WORK:
        return _WORK[key]
    if name == "multidof":
        model = _fk_models()[3]
        links = _leaf_and_multidof(model)
    else:
        model = loik_amd.builtin_model(name)
        links = _links(model, 1)
    seed = 1500 + 10 * ["panda7", "talos32", "multidof"].index(name) + variant
    rng = np.random.default_rng(seed)
    B = B_PARITY
    A = _nonsym_A(rng, len(links))
    q0, tg = _seeds(model, B, links, seed=seed + 1, spread=(1e-5, 0.3))
    q_lo, q_hi = -np.inf * np.ones(model.nv), np.inf * np.ones(model.nv)
    a_max = None
    if variant == 1:
        q_t = model.random_configurations(np.random.default_rng(seed + 1), B)   # (what _seeds drew the targets from)
        q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, seed + 2, (10.0, 90.0))
        a_max = PA.accel_limits(model, seed + 3, 0.25, BOUND, lo=0.05, hi=0.5)
    lk, spheres = CN.make_spheres(model, 1, seed + 4)
    ws, wb = TC._world(rng, 6, 5)
    col = dict(links=lk, spheres=spheres, ws=ws, wb=wb, pairs=CN.self_pairs(model.parents, lk))
    _WORK[key] = dict(model=model, links=links, A=A, q0=q0, tg=tg, q_lo=q_lo, q_hi=q_hi, a_max=a_max, box=_box(model), B=B, col=col)
    return _WORK[key]


def _latched(w, precision=capi.F64, avoid=AVOID, limits=True, q0=None, grid=False):
    s = _handle(w["model"], w["B"], w["links"], w["q0"] if q0 is None else q0, w["A"], PRM, precision=precision, box=w["box"])
    c = w["col"]
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    if limits and np.isfinite(w["q_lo"]).any():
        s.set_joint_limits(w["q_lo"], w["q_hi"])
    if limits and w.get("a_max") is not None:
        s.set_joint_accel_limits(w["a_max"])
    if grid:
        _latch_grid(s, c)
    if avoid is not None:
        s.set_collision_avoidance(**avoid)
    return s


def _latch_grid(s, col):
    """_latched(grid=True) on a workload with a voxel grid (col["grid"], gridnear_cases.pose_workload): the nearest-voxel transform
    latched and the grid set, before avoidance is (the order of test_gridnear_pose._with_grid).  Without one: nothing"""
    g = col.get("grid")
    if g is not None:
        s.set_collision_grid_nearest(True)
        s.set_collision_grid(g.occ, g.origin, g.h)


def _oracle(w, dt, gain, k, avoid=AVOID):
    key = (id(w), dt, gain, k, tuple(sorted(avoid.items())))
    if key not in _ORACLE:
        lb, ub = w["box"]
        _ORACLE[key] = AN.lockstep_pose_loop_avoid(w["model"], PRM, w["q0"], np.eye(6), np.zeros(6), w["links"], w["A"], lb, ub, w["tg"], dt, gain, TOL, k,
                                                   w["q_lo"], w["q_hi"], w["col"], avoid, a_max=w.get("a_max"))
    return _ORACLE[key]


def _scale(w, q):
    c = w["col"]
    return 1.0 + float(np.max(np.abs(CN.centres(w["model"], q, c["links"], c["spheres"])))) + float(np.max(c["spheres"][:, 3]))


# ---- 1. parity with the lock-step oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", LAWS, ids=lambda l: "dt%g-g%g" % l)
@pytest.mark.parametrize("case", PARITY_CASES, ids=lambda c: "%s%s" % (c[0], "-limits-accel" if c[1] else ""))
def test_solve_pose_matches_lockstep_oracle(case, law):
    """the comparison of test_pose_limits.test_limits_match_lockstep_oracle on the instances whose oracle run touched no near
    configuration (at most 2 % are left out: test_avoid_numpy.py asserts that share for these workloads without a GPU); the avoidance
    results beside it"""
    w = _workload(*case)
    dt, gain = law
    idx = np.arange(w["B"])
    for k in PARITY_STEPS:
        s = _latched(w)
        out = s.SolvePose(w["tg"], dt=dt, gain=gain, tol_pose=TOL, max_steps=k)
        q = s.get("q")
        s.close()
        o = _oracle(w, dt, gain, k)
        keep = ~o["near"]
        assert (~keep).mean() <= 0.02, (case, law, k, o["near"])
        narrowed = (o["avoid_active_steps"] > 0).mean()
        print("avoidance %s %s k=%d: oracle narrowed %.3f reached %.3f steps %s" % (case, law, k, narrowed, o["reached"].mean(), np.bincount(o["steps"]).tolist()))
        assert narrowed >= 0.25, (case, law, k, narrowed)   # (the condition that makes the case mean something)
        sub = {f: v[keep] for f, v in o.items() if f != "q_path"}
        same = _gate(out, q, sub, idx[keep], (case, law, k))
        assert np.array_equal(out["status"][keep][same] & 9, sub["status"][same] & 9)
        # (a flag is a comparison of two numbers that differ by the parity gate's 1e-7 at most between device and oracle)
        assert (out["avoid_flags"][keep][same] != sub["avoid_flags"][same]).any(axis=1).mean() <= 0.01, (case, law, k)
        assert np.array_equal(out["avoid_active_steps"][keep][same], sub["avoid_active_steps"][same])
        ms, want = out["avoid_min_seen"][keep][same], sub["avoid_min_seen"][same]
        assert np.array_equal(np.isinf(ms), np.isinf(want))
        fin = np.isfinite(want)
        assert np.all(np.abs(ms[fin] - want[fin]) <= 1e-7), (case, law, k)   # (the gate's 1e-7 on q, through FK)
        if case[1]:
            assert (out["limit_flags"][keep][same] != sub["limit_flags"][same]).any(axis=1).mean() <= 0.01, (case, law, k)


# ---- 2. a wall ----------------------------------------------------------------------------------------------------------------------
WALL = dict(d_safe=0.05, d_influence=0.25, kappa=0.25)   # (chosen on the CPU oracle: test_avoid_numpy.py asserts both conditions)
WALL_DT, WALL_GAIN, WALL_STEPS, WALL_B = 0.25, 0.5, 10, 64


def _wall_case():
    """panda7, 64 instances: seeds around one configuration, targets around another, and a slab across the straight line between the
    two hand positions, placed from the reference's FK; spheres on the last three links"""
    if "wall" in _WORK:
        return _WORK["wall"]
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 1)
    rng = np.random.default_rng(1600)
    qa = np.array([0.0, -0.4, 0.0, -2.0, 0.0, 1.6, 0.8])
    qb = np.array([1.6, -0.4, 0.0, -2.0, 0.0, 1.6, 0.8])
    q0 = qa + 0.05 * rng.uniform(-1.0, 1.0, size=(WALL_B, model.nv))
    q_t = qb + 0.05 * rng.uniform(-1.0, 1.0, size=(WALL_B, model.nv))
    tg = P.fk12(model, q_t, links)
    pa, pb = P.fk(model, qa[None], links[0])[1][0], P.fk(model, qb[None], links[0])[1][0]
    x = (pb - pa) / np.linalg.norm(pb - pa)
    y = np.cross([0.0, 0.0, 1.0], x)
    y /= np.linalg.norm(y)
    T = np.eye(4)
    T[:3, :3] = np.stack([x, y, np.cross(x, y)], axis=1)
    T[:3, 3] = 0.5 * (pa + pb)
    wb = CN.box15(T, [0.02, 0.5, 0.5])[None]
    lk, spheres = CN.make_spheres(model, 1, 1601, links=[5, 6, 7])
    col = dict(links=lk, spheres=spheres, ws=np.zeros((0, 4)), wb=wb, pairs=[])
    inf = np.inf * np.ones(model.nv)
    _WORK["wall"] = dict(model=model, links=links, A=np.tile(np.eye(6), (1, 1, 1)), q0=q0, q_t=q_t, tg=tg, q_lo=-inf, q_hi=inf, a_max=None,
                         box=_box(model), B=WALL_B, col=col)
    return _WORK["wall"]


def _path_clearance(w, paths):
    """the least clearance_numpy clearance over each instance's recorded configurations"""
    c = w["col"]
    return np.array([CN.clearance(w["model"], p, c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"])["min"].min() for p in paths])


def wall_oracle_paths():
    """(least clearance per instance without the latch, with it) over the oracle's recorded paths: test_avoid_numpy.py asserts the two
    conditions that make the wall a test, without a GPU"""
    w = _wall_case()
    free = _oracle(w, WALL_DT, WALL_GAIN, WALL_STEPS, dict(d_safe=-1e9, d_influence=-1e8, kappa=0.5))
    held = _oracle(w, WALL_DT, WALL_GAIN, WALL_STEPS, WALL)
    return _path_clearance(w, free["q_path"]), _path_clearance(w, held["q_path"])


WALL_PROGRESS = 0.75   # with the latch every instance still closes a quarter of its pose error before the wall holds it (measured on the
                        # CPU oracle: 0.65 in the median, 0.71 at most; test_avoid_numpy.py asserts it there)


def wall_errors(w, q):
    """max_c |e_c|_inf of the configurations q [B][nq] against the wall case's targets"""
    return np.abs(P.pose_errors(w["model"], q, w["links"], w["tg"])).max(axis=(1, 2))


def _device_clearance(s, w, rows):
    return s.clearance(np.ascontiguousarray(rows).reshape(-1, w["model"].nq))["min"]


def test_wall_solve_pose_step_by_step_and_path():
    w = _wall_case()
    cfree, cheld = wall_oracle_paths()
    assert (cfree < 0.0).mean() >= 0.5 and np.all(cheld >= WALL["d_safe"] / 2)
    B, nq = w["B"], w["model"].nq
    kw = dict(dt=WALL_DT, gain=WALL_GAIN, tol_pose=TOL)
    scale = _scale(w, w["q0"])
    # SolvePose, one step a call: the configuration before each call is the step-start configuration avoid_min_seen speaks of
    s = _latched(w, avoid=WALL)
    q, least = w["q0"], np.full(B, np.inf)
    for step in range(WALL_STEPS):
        before = _device_clearance(s, w, q)
        out = s.SolvePose(w["tg"], max_steps=1, q=q if step == 0 else None, **kw)
        ran = out["steps"] == 1
        assert np.all(np.abs(out["avoid_min_seen"][ran] - before[ran]) <= TC.BOUND * scale), step
        assert np.all(np.isposinf(out["avoid_min_seen"][~ran])) and not out["avoid_active_steps"][~ran].any()
        assert np.all((out["avoid_active_steps"] > 0) == (out["avoid_flags"] != 0).any(axis=1))
        q = s.get("q")
        least = np.minimum(least, _device_clearance(s, w, q))
    print("avoidance wall: step-by-step least clearance %.4f (oracle %.4f; without the latch %.4f)" % (least.min(), cheld.min(), cfree.min()))
    assert np.all(least >= WALL["d_safe"] / 2 - 1e-9)
    # ... and the same loop in one call ends where the step-by-step one did (warm starts carry over alike)
    one = s.SolvePose(w["tg"], max_steps=WALL_STEPS, q=w["q0"], **kw)
    assert np.all(_device_clearance(s, w, s.get("q")) >= WALL["d_safe"] / 2 - 1e-9)
    assert np.all(one["avoid_min_seen"] >= WALL["d_safe"] / 2 - 1e-9) and (one["avoid_active_steps"] > 0).mean() >= 0.5
    # ... and it is no freeze: every instance moves up to the wall, the target behind it stays out of reach (WALL_PROGRESS, as the oracle)
    e0, e1 = wall_errors(w, w["q0"]), np.abs(one["err"]).max(axis=(1, 2))
    assert np.all(e1 <= WALL_PROGRESS * e0) and np.all(np.abs(s.get("q") - w["q0"]).max(axis=1) > 0.2)
    # SolvePosePath.  q_path records the configurations at which a waypoint was reached, not every step start, so for a path of several
    # waypoints avoid_min_seen can only be bounded: every recorded configuration keeps its distance, and avoid_min_seen is no more than the
    # least clearance over the step starts among them (the seed and the waypoints reached before the last).  The exact referee of the path
    # loop is the path of ONE waypoint, which is SolvePose bit for bit (test_pose_path.test_one_waypoint_is_solve_pose_bit_for_bit), whose
    # avoid_min_seen the one-step calls above pin to clearance(): fresh handles, the same q and the same three results
    res = []
    for path in (False, True):
        h = _latched(w, avoid=WALL)
        o = h.SolvePosePath(w["tg"][:, None], max_steps=WALL_STEPS, **kw) if path else h.SolvePose(w["tg"], max_steps=WALL_STEPS, **kw)
        res.append((o, h.get("q")))
        h.close()
    assert np.array_equal(res[0][1], res[1][1]) and (res[0][0]["avoid_active_steps"] > 0).any()
    for f in ("avoid_min_seen", "avoid_active_steps", "avoid_flags"):
        assert np.array_equal(res[0][0][f], res[1][0][f]), f
    tgm = P.fk12(w["model"], np.stack([P.integrate(w["model"], w["q0"][b], f * _way(w, b)) for b in range(B) for f in (0.4, 0.7, 1.0)]), w["links"])
    wp = tgm.reshape(B, 3, len(w["links"]), 12)
    pout = s.SolvePosePath(wp, max_steps=3 * WALL_STEPS, q=w["q0"], **kw)
    rec = pout["q_path"]
    got = ~np.isnan(rec).any(axis=2)
    cl = np.full((B, 3), np.inf)
    cl[got] = _device_clearance(s, w, rec[got])
    assert np.all(cl >= WALL["d_safe"] / 2 - 1e-9)
    starts = np.minimum(_device_clearance(s, w, w["q0"]), np.where(got[:, :2], cl[:, :2], np.inf).min(axis=1))
    assert np.all(pout["avoid_min_seen"] <= starts + TC.BOUND * scale)
    assert np.all(pout["avoid_min_seen"] >= WALL["d_safe"] / 2 - 1e-9) and (pout["avoid_active_steps"] > 0).any()
    # without the latch SolvePose runs into the wall as the oracle does: one step a call again, clearance() after each
    s.clear_collision_avoidance()
    least = np.full(B, np.inf)
    for step in range(WALL_STEPS):
        free = s.SolvePose(w["tg"], max_steps=1, q=w["q0"] if step == 0 else None, **kw)
        assert "avoid_min_seen" not in free
        least = np.minimum(least, _device_clearance(s, w, s.get("q")))
    assert (least < 0.0).mean() >= 0.5, least
    # ... and so does SolvePosePath over the three waypoints, at the waypoints it records
    pfree = s.SolvePosePath(wp, max_steps=3 * WALL_STEPS, q=w["q0"], **kw)
    got = ~np.isnan(pfree["q_path"]).any(axis=2)
    cl = np.full((B, 3), np.inf)
    cl[got] = _device_clearance(s, w, pfree["q_path"][got])
    print("avoidance wall: without the latch SolvePose reaches %.4f, the recorded waypoints of SolvePosePath %.4f" % (least.min(), cl.min()))
    s.close()


def _way(w, b):
    """the joint-space step from seed b to the configuration its target was drawn from (panda7: nq == nv, a plain difference)"""
    return w["q_t"][b] - w["q0"][b]


def test_wall_track_pose():
    """a trajectory through the wall, T = 10 samples: q_traj holds every step-start configuration, so avoid_min_seen is its minimum"""
    w = _wall_case()
    B, T = w["B"], WALL_STEPS
    qs = np.stack([[P.integrate(w["model"], w["q0"][b], (k / T) * _way(w, b)) for k in range(T + 1)] for b in range(B)])
    smp = P.fk12(w["model"], qs.reshape(-1, w["model"].nq), w["links"]).reshape(B, T + 1, len(w["links"]), 12)
    s = _latched(w, avoid=WALL)
    out = s.TrackPose(smp, dt=WALL_DT, gain=WALL_GAIN, tol_track=1e-3, q=w["q0"])
    traj = out["q_traj"]
    assert np.isfinite(traj).all()
    cl = _device_clearance(s, w, traj).reshape(B, T + 1)
    scale = _scale(w, w["q0"])
    print("avoidance wall: tracked least clearance %.4f, narrowed instances %.3f" % (cl.min(), (out["avoid_active_steps"] > 0).mean()))
    assert np.all(cl >= WALL["d_safe"] / 2 - 1e-9)
    assert np.all(np.abs(out["avoid_min_seen"] - cl[:, :T].min(axis=1)) <= TC.BOUND * scale)
    assert (out["avoid_active_steps"] > 0).mean() >= 0.5 and np.all(out["avoid_active_steps"] <= T)
    # the same trajectory without the latch goes through
    s.clear_collision_avoidance()
    free = s.TrackPose(smp, dt=WALL_DT, gain=WALL_GAIN, tol_track=1e-3, q=w["q0"])
    assert (_device_clearance(s, w, free["q_traj"]).reshape(B, T + 1).min(axis=1) < 0.0).mean() >= 0.5
    s.close()


# ---- 3. the multi-start, fp32, neutrality -----------------------------------------------------------------------------------------
def test_multistart_one_round_is_solve_pose_with_the_latch():
    """the route of test_multistart.test_one_seed_one_round_is_solve_pose: K = 1, one round, the goals' q0 rows as the seeds"""
    w = _workload("panda7", 0)
    a, b = _latched(w), _latched(w)
    out = a.SolvePoseMultiStart(w["tg"], 1, q0=w["q0"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=3)
    ref = b.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=3, q=w["q0"])
    assert np.array_equal(a.get("q"), b.get("q"))
    for f in ("avoid_min_seen", "avoid_active_steps", "avoid_flags"):
        assert np.array_equal(out[f], ref[f]), f
    assert (ref["avoid_active_steps"] > 0).any()
    a.close(); b.close()


def _plan_core(s):
    """plan() without the parts that record a handle's solve history (test_pose_limits._plan_core)"""
    import re
    return re.sub(r"; device buffers:.*?room\)", "", re.sub(r"; decades visited[^;]*", "", s.plan()))


def test_f32_box_is_inside_the_f64_box_and_the_base_box_comes_back():
    """one step from the same q: the z of an fp32 handle, which its inner solve projects onto the box it was handed, lies inside the fp64
    box of the query (which does not round) on both sides, exactly: rounding to nearest would let it out by half an ulp of fp32.  Then the
    route of test_pose_limits.test_base_box_is_restored: the handle and a twin that never had the latch, put on the same q and started
    cold with a b large enough that the base box binds, give bit-identical z / iter"""
    w = _workload("talos32", 0)
    lb, ub = w["box"]
    s, t = _latched(w, precision=capi.F32), _latched(w, precision=capi.F32, avoid=None)
    ref = _latched(w)
    box = ref.avoidance_box(w["q0"], 0.25, lb, ub, **AVOID)
    ref.close()
    out = s.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=1)
    t.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=1)
    ran = out["steps"] == 1
    z = s.get("z").astype(np.float64)
    assert ran.any() and np.all(z[ran] >= box["lo"][ran]) and np.all(z[ran] <= box["hi"][ran])
    on_lo, on_hi = (out["avoid_flags"] & 1) != 0, (out["avoid_flags"] & 2) != 0
    assert np.array_equal(on_lo[ran], (box["lo"] > lb)[ran]) and np.array_equal(on_hi[ran], (box["hi"] < ub)[ran])
    assert ((on_lo | on_hi) & ran[:, None]).any()
    # ... and some z rests on a narrowed side: the fp32 number the kernel stored, which is the fp64 bound rounded toward zero
    lo_in = np.where(box["lo"].astype(np.float32) < box["lo"], np.nextafter(box["lo"].astype(np.float32), np.float32(0.0)), box["lo"].astype(np.float32))
    hi_in = np.where(box["hi"].astype(np.float32) > box["hi"], np.nextafter(box["hi"].astype(np.float32), np.float32(0.0)), box["hi"].astype(np.float32))
    assert ((z == lo_in) & on_lo & ran[:, None]).any() or ((z == hi_in) & on_hi & ran[:, None]).any()
    assert not np.array_equal(z, t.get("z").astype(np.float64))
    q = s.get("q")
    rng = np.random.default_rng(6)
    b = rng.choice([-1.0, 1.0], size=(w["B"], 6)) * (3.0 + rng.random((w["B"], 6)))
    s.clear_collision_avoidance()
    for h in (s, t):
        h.set_warm_start(False)
        h.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=0, q=q)
        h.UpdateEqConstraint(w["links"][0], b)
        h.Solve(None, -1, None, None)
        h.Solve()
    zs, zt = s.get("z"), t.get("z")
    assert np.array_equal(s.get("iter"), t.get("iter")) and np.array_equal(zs, zt)
    assert ((zs == np.broadcast_to(lb, zs.shape)) | (zs == np.broadcast_to(ub, zs.shape))).any(), "the base box never binds: the test shows nothing"
    s.close(); t.close()


def test_a_cleared_latch_is_no_latch():
    w = _workload("panda7", 0)
    a, b = _latched(w, avoid=None), _latched(w, avoid=None)
    plan = b.plan()
    a.set_collision_avoidance(**AVOID)
    assert a.plan() != plan and "k_avoid_box" in a.plan()
    a.clear_collision_avoidance()
    assert a.plan() == plan
    ra = a.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=4)
    rb = b.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=4)
    assert set(ra) == set(rb) and "avoid_min_seen" not in ra
    assert all(np.array_equal(ra[f], rb[f]) for f in ra)
    for f in ("q", "z", "iter"):
        assert np.array_equal(a.get(f), b.get(f)), f
    assert a.plan() == b.plan()
    buf = np.zeros(w["B"])
    for s in (a, b):
        assert s.L.loikb_avoid_get_result(s.h, capi.AVOID_F_MIN_SEEN, buf.ctypes.data_as(C.c_void_p), 0) == ERR_STATE
    # ... and with the latch the same handle does something else, and says so
    a.set_collision_avoidance(**AVOID)
    rc = a.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=4, q=w["q0"])
    assert (rc["avoid_active_steps"] > 0).any() and not np.array_equal(a.get("q"), b.get("q"))
    assert _plan_core(a) != _plan_core(b)
    a.close(); b.close()
