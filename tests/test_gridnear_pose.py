"""GPU: the pose loops with collision avoidance reading a voxel grid (include/loik_amd_gridnear.h) -- SolvePose against the lock-step
reference of tests/gridnear_numpy.py in fp64, an fp32 handle against the fp64 one over the same steps, its inward rounding, a wall of
voxels that the loops keep away from (SolvePose step by step and in one call, SolvePosePath, TrackPose), and neutrality of the latch in
a pose loop."""
import numpy as np
import pytest

from loik_amd import capi

from test_avoid_pose import AVOID, TOL, WALL, WALL_DT, WALL_GAIN, WALL_STEPS, _device_clearance, _latched, _scale, _way, wall_errors
from test_clearance import BOUND
from test_pose_ik import PRM
from test_fp32_parity import CONTRACT_PINS
from test_pose_parity import _gate, _handle
import gridnear_cases as GC
import pose_numpy as P
from test_gridnear_numpy import WALL_FLOOR, WALL_PROGRESS, exact_path_clearance

pytestmark = pytest.mark.gpu

F32_Z = max(p[0] for p in CONTRACT_PINS.values())   # 8e-3: the recorded p99 of |z_f32 - z_f64|_inf on the largest robot
LAW = (0.25, 0.5)
STEPS = (1, 4)


def _with_grid(w, precision=capi.F64, avoid=AVOID, q0=None):
    """test_avoid_pose._latched with the transform latched and the grid set before avoidance is"""
    s = _latched(w, precision=precision, avoid=None, q0=q0)
    s.set_collision_grid_nearest(True)
    g = w["col"]["grid"]
    s.set_collision_grid(g.occ, g.origin, g.h)
    if avoid is not None:
        s.set_collision_avoidance(**avoid)
    return s


@pytest.mark.parametrize("name", ["panda7", "talos32"])
def test_solve_pose_matches_lockstep_oracle(name):
    w = GC.pose_workload(name)
    dt, gain = LAW
    idx = np.arange(w["B"])
    for k in STEPS:
        s = _with_grid(w)
        out = s.SolvePose(w["tg"], dt=dt, gain=gain, tol_pose=TOL, max_steps=k)
        q = s.get("q")
        s.close()
        o = GC.pose_oracle(w, dt, gain, k, AVOID, TOL)
        keep = ~o["near"]
        assert (~keep).mean() <= GC.NEAR_SHARE, (name, k, o["near"])
        sub = {f: v[keep] for f, v in o.items() if f != "q_path" and isinstance(v, np.ndarray) and v.shape[:1] == (w["B"],)}
        same = _gate(out, q, sub, idx[keep], (name, k))
        assert np.array_equal(out["status"][keep][same] & 9, sub["status"][same] & 9)
        assert (out["avoid_flags"][keep][same] != sub["avoid_flags"][same]).any(axis=1).mean() <= 0.01, (name, k)
        assert np.array_equal(out["avoid_active_steps"][keep][same], sub["avoid_active_steps"][same])
        ms, want = out["avoid_min_seen"][keep][same], sub["avoid_min_seen"][same]
        assert np.array_equal(np.isinf(ms), np.isinf(want))
        fin = np.isfinite(want)
        assert np.all(np.abs(ms[fin] - want[fin]) <= 1e-7), (name, k)
        print("gridnear pose %s k=%d: narrowed %.3f, %d near left out" % (name, k, (o["avoid_active_steps"] > 0).mean(), int((~keep).sum())))


def _both(w, precision):
    """_with_grid through test_pose_parity._handle: the fp32 and the fp64 handle of test_f32_solve_pose_matches_f64"""
    s = _handle(w["model"], w["B"], w["links"], w["q0"], w["A"], PRM, precision=precision, box=w["box"])
    c = w["col"]
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    s.set_collision_grid_nearest(True)
    s.set_collision_grid(c["grid"].occ, c["grid"].origin, c["grid"].h)
    s.set_collision_avoidance(**AVOID)
    return s


@pytest.mark.parametrize("name", ["panda7", "talos32"])
def test_f32_solve_pose_matches_f64(name):
    """SolvePose of 1 and of 4 steps on an fp32 handle against the fp64 handle on the same workload, which
    test_solve_pose_matches_lockstep_oracle anchors to the reference.  Avoidance is fp64 from the fp64 q on both, so the two differ by
    the fp32 inner solve and by the inward rounding of the box (one ulp of fp32).  What an fp32 solve owes an fp64 one is the library's
    recorded accuracy contract (include/loik_amd.h at LOIKB_OPT_F32_ACCURATE, pinned by test_fp32_parity.CONTRACT_PINS): |z_f32 - z_f64|
    of a converged solve, 8e-3 at the 99th percentile on the largest of these robots.  A step moves q by dt z, so k steps may differ by
    k dt F32_Z at most; the pose error and avoid_min_seen move with q at most as fast as a point of the robot does, |dq| times its
    reach (the scale of test_clearance.py).  The steps, the status bits and the count of narrowed steps are the same.  A grid normal of
    the wrong sign or a wrong ordinal in the fp32 step kernel moves a narrowed instance by a step of its own, 1e-2 .. 1e-1 here.
    (Solves cut at a fixed iteration count, as test_pose_parity.F32_STEP_REL has them, are no referee here: under a box that binds
    the unconverged fp32 and fp64 iterates of one instance part by 2e-2 in q within two steps, with the grid and without it alike.)"""
    w = GC.pose_workload(name)
    dt, gain = LAW
    scale = _scale(w, w["q0"])
    for k in STEPS:
        res = {}
        for prec in (capi.F32, capi.F64):
            s = _both(w, prec)
            out = s.SolvePose(w["tg"], dt=dt, gain=gain, tol_pose=TOL, max_steps=k)
            res[prec] = (out, s.get("q"))
            s.close()
        (o32, q32), (o64, q64) = res[capi.F32], res[capi.F64]
        ran = o64["steps"] > 0
        dq = np.abs(q32 - q64).max(axis=1)
        fin = ran & np.isfinite(o64["avoid_min_seen"])
        dm = np.abs(o32["avoid_min_seen"][fin] - o64["avoid_min_seen"][fin])
        de = np.abs(o32["err"] - o64["err"]).max(axis=(1, 2))
        bound = k * dt * F32_Z
        print("gridnear pose %s k=%d f32 vs f64: max |dq| %.3e (bound %.3e), max |d err| %.3e, max |d min_seen| %.3e, narrowed %.3f, moved up to %.3e" %
              (name, k, dq.max(), bound, de.max(), dm.max(initial=0.0), (o64["avoid_active_steps"] > 0).mean(), np.abs(q64 - w["q0"]).max()))
        assert ran.any() and (o64["avoid_active_steps"] > 0).mean() >= 0.25
        assert np.array_equal(o32["steps"], o64["steps"]) and np.array_equal(o32["status"] & 9, o64["status"] & 9)
        assert np.array_equal(o32["avoid_active_steps"], o64["avoid_active_steps"])
        assert np.array_equal(np.isinf(o32["avoid_min_seen"]), np.isinf(o64["avoid_min_seen"]))
        assert dq.max() <= bound and np.all(dq[~ran] == 0.0), (name, k, dq.max())
        assert de.max() <= bound * scale and dm.max(initial=0.0) <= bound * scale, (name, k, de.max(), dm.max(initial=0.0))


@pytest.mark.parametrize("name", ["panda7", "talos32"])
def test_f32_step_stays_inside_the_f64_box(name):
    """one step of an fp32 handle from the same q: its z lies inside the fp64 box of the query, which reads the same grid and does not
    round, and its flags are the query's narrowed sides (test_avoid_pose.test_f32_box_is_inside_the_f64_box...)"""
    w = GC.pose_workload(name)
    lb, ub = w["box"]
    ref = _with_grid(w)
    box = ref.avoidance_box(w["q0"], LAW[0], lb, ub, **AVOID)
    nwo = w["col"]["ws"].shape[0] + w["col"]["wb"].shape[0]
    assert (box["partner"][:, :, 0] == nwo).any()
    ref.close()
    s = _with_grid(w, precision=capi.F32)
    out = s.SolvePose(w["tg"], dt=LAW[0], gain=LAW[1], tol_pose=TOL, max_steps=1)
    ran = out["steps"] == 1
    z = s.get("z").astype(np.float64)
    assert ran.any() and np.all(z[ran] >= box["lo"][ran]) and np.all(z[ran] <= box["hi"][ran])
    on_lo, on_hi = (out["avoid_flags"] & 1) != 0, (out["avoid_flags"] & 2) != 0
    assert np.array_equal(on_lo[ran], (box["lo"] > lb)[ran]) and np.array_equal(on_hi[ran], (box["hi"] < ub)[ran])
    assert ((on_lo | on_hi) & ran[:, None]).any()
    s.close()


def test_wall_of_voxels():
    w = GC.wall_workload()
    B = w["B"]
    kw = dict(dt=WALL_DT, gain=WALL_GAIN, tol_pose=TOL)
    scale = _scale(w, w["q0"])
    s = _with_grid(w, avoid=WALL)
    q, rows = w["q0"], [w["q0"]]
    for step in range(WALL_STEPS):
        before = _device_clearance(s, w, q)
        out = s.SolvePose(w["tg"], max_steps=1, q=q if step == 0 else None, **kw)
        ran = out["steps"] == 1
        assert np.array_equal(out["avoid_min_seen"][ran], before[ran]), step      # the same pair, the same bits as clearance()
        assert np.all(np.isposinf(out["avoid_min_seen"][~ran]))
        q = s.get("q")
        rows.append(q)
    exact = exact_path_clearance(w, [np.stack([r[b] for r in rows]) for b in range(B)])
    print("gridnear wall: least exact clearance %.4f (floor %.4f)" % (exact.min(), WALL_FLOOR))
    assert np.all(exact >= WALL_FLOOR)
    one = s.SolvePose(w["tg"], max_steps=WALL_STEPS, q=w["q0"], **kw)
    q_one = s.get("q")
    assert np.all(exact_path_clearance(w, [q_one[b][None] for b in range(B)]) >= WALL_FLOOR)
    assert (one["avoid_active_steps"] > 0).mean() >= 0.5
    e0, e1 = wall_errors(w, w["q0"]), np.abs(one["err"]).max(axis=(1, 2))
    assert np.all(e1 <= WALL_PROGRESS * e0) and np.all(np.abs(q_one - w["q0"]).max(axis=1) > 0.2)
    # SolvePosePath over one waypoint is SolvePose, bit for bit, with the grid as without
    res = []
    for path in (False, True):
        h = _with_grid(w, avoid=WALL)
        o = h.SolvePosePath(w["tg"][:, None], max_steps=WALL_STEPS, **kw) if path else h.SolvePose(w["tg"], max_steps=WALL_STEPS, **kw)
        res.append((o, h.get("q")))
        h.close()
    assert np.array_equal(res[0][1], res[1][1]) and (res[0][0]["avoid_active_steps"] > 0).any()
    for f in ("avoid_min_seen", "avoid_active_steps", "avoid_flags"):
        assert np.array_equal(res[0][0][f], res[1][0][f]), f
    # TrackPose through the wall: q_traj holds every step-start configuration, so avoid_min_seen is the minimum of their clearance()
    T = WALL_STEPS
    qs = np.stack([[P.integrate(w["model"], w["q0"][b], (k / T) * _way(w, b)) for k in range(T + 1)] for b in range(B)])
    smp = P.fk12(w["model"], qs.reshape(-1, w["model"].nq), w["links"]).reshape(B, T + 1, len(w["links"]), 12)
    out = s.TrackPose(smp, dt=WALL_DT, gain=WALL_GAIN, tol_track=1e-3, q=w["q0"])
    traj = out["q_traj"]
    assert np.isfinite(traj).all()
    cl = _device_clearance(s, w, traj).reshape(B, T + 1)
    assert np.all(np.abs(out["avoid_min_seen"] - cl[:, :T].min(axis=1)) <= BOUND * scale)
    assert np.all(exact_path_clearance(w, list(traj)) >= WALL_FLOOR) and (out["avoid_active_steps"] > 0).mean() >= 0.5
    # without the latch of avoidance the same loop runs into the voxels
    # (one step a call, every configuration on the way: the arm goes through the slab and ends behind it)
    s.clear_collision_avoidance()
    rows = [w["q0"]]
    for step in range(WALL_STEPS):
        s.SolvePose(w["tg"], max_steps=1, q=w["q0"] if step == 0 else None, **kw)
        rows.append(s.get("q"))
    free = exact_path_clearance(w, [np.stack([r[b] for r in rows]) for b in range(B)])
    s.close()
    assert (free < WALL_FLOOR).mean() >= 0.5


def test_a_latch_set_and_cleared_is_no_latch_in_a_pose_loop():
    w = GC.pose_workload("panda7")
    a, b = _with_grid(w, avoid=None), _latched(w)
    a.set_collision_grid(None)
    a.set_collision_grid_nearest(False)
    a.set_collision_avoidance(**AVOID)
    ra = a.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=4)
    rb = b.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=4)
    assert set(ra) == set(rb) and all(np.array_equal(ra[f], rb[f]) for f in ra if "timing" not in f)
    for f in ("q", "z", "iter"):
        assert np.array_equal(a.get(f), b.get(f)), f
    # latch on, no grid: the same again
    a.set_collision_grid_nearest(True)
    rc = a.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=4, q=w["q0"])
    rd = b.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=4, q=w["q0"])
    assert all(np.array_equal(rc[f], rd[f]) for f in rc if "timing" not in f) and np.array_equal(a.get("q"), b.get("q"))
    # a grid set while avoidance and the latch are on is read by the next step
    g = w["col"]["grid"]
    a.set_collision_grid(g.occ, g.origin, g.h)
    re = a.SolvePose(w["tg"], dt=0.25, gain=0.5, tol_pose=TOL, max_steps=4, q=w["q0"])
    assert not np.array_equal(re["avoid_min_seen"], rd["avoid_min_seen"])
    a.close(); b.close()
