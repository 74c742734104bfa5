"""GPU: the step mode of k_avoid_box (loik_pose_avoid.hpp) on robots whose DoFs stride past one wavefront -- the 170- and the 330-joint
tree of test_clearance.py -- on both placements routes: the LDS stages and, past the 64 KB rule, the placements k_avoid_placements writes
to HBM.  Until this file the step mode ran on at most 32 joints, and the HBM route in the two queries alone.

The instantiations of k_avoid_box and the tests that hold them to a reference or an exact identity:
  <false, AVD_GRAD, double>   test_avoid_box.test_clearance_gradient_matches_numpy, test_gridnear.test_gradient_and_box_match_numpy
  <true,  AVD_GRAD, double>   the same two on tree330
  <false, AVD_QUERY, double>  test_avoid_box.test_avoidance_box_matches_numpy; here test_205_and_206_spheres_give_the_same_bits (205)
  <true,  AVD_QUERY, double>  the same on tree330; here test_205_and_206_spheres_give_the_same_bits (206)
  <false, AVD_STEP, double>   test_avoid_pose / test_avoid_routes; here test_z_is_inside_the_clamped_query[tree170-ns64/ns205-f64] and
                              test_solve_pose_matches_lockstep_oracle[lds-nolimits] with nb > 64
  <false, AVD_STEP, float>    test_avoid_routes.test_z_is_inside_the_clamped_query_exactly[f32]; here [tree170-ns64/ns205-f32]
  <true,  AVD_STEP, double>   here alone: test_z_is_inside_the_clamped_query[*-hbm-f64], test_solve_pose_matches_lockstep_oracle[hbm-*],
                              test_base_box_comes_back_on_the_hbm_route, test_path_of_one_waypoint_and_track
  <true,  AVD_STEP, float>    here alone: test_z_is_inside_the_clamped_query[*-hbm-f32]

Every input is built without a GPU by tests/avoid_big_cases.py, and tests/test_avoid_big_numpy.py asserts on the reference alone the
conditions that make each case mean something.  The gates are the project's: exact where stated; test_pose_parity._gate (the same
reached / steps, |dq| < 1e-7 -- at B = 5 on every instance) and test_avoid_routes._assert_results against the lock-step oracle."""
import numpy as np
import pytest

from loik_amd import capi

from test_avoid_pose import AVOID, TOL, _latched
import test_avoid_box as TB
import test_avoid_routes as R
import test_clearance as TC
import avoid_big_cases as BC

pytestmark = pytest.mark.gpu


# ---- 1. exact, on every row of the table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", BC.TABLE, ids=BC.row_id)
def test_z_is_inside_the_clamped_query(case, precision):
    """test_avoid_routes._check_containment as it stands, two calls of one step: z in clamp(A(q), lb, ub) of the fp64 query at the
    configuration before the call, the flags the clamp's, the active steps counted, the fp32 bound the fp64 one rounded toward zero and
    at least one entry resting on a bound whose nearest fp32 number lies outside the box.  Then avoid_min_seen of one step is
    clearance(q)["min"] of the same handle, bit for bit"""
    name, ns, hbm, waves, B, _ = case
    w = BC.table_case(case)
    assert BC.launch_shape(w["model"].njoints - 1, ns) == (hbm, waves) and w["B"] == B
    R._check_containment(w, precision, (BC.row_id(case), "f64" if precision == capi.F64 else "f32"), calls=2)
    s = R._loop_handle(w, precision=precision)
    before = s.clearance(w["q0"])["min"]
    out = s.SolvePose(w["tg"], dt=BC.LAW[0], gain=BC.LAW[1], tol_pose=TOL, max_steps=1)
    s.close()
    ran = out["steps"] == 1
    assert ran.any() and np.array_equal(out["avoid_min_seen"][ran], before[ran]), (out["avoid_min_seen"], before)
    assert np.all(np.isposinf(out["avoid_min_seen"][~ran]))


# ---- 2. the centres of k_avoid_placements have the bits of the LDS stages -------------------------------------------------------------------
def test_205_and_206_spheres_give_the_same_bits():
    """the query at the same q with the first 205 spheres (the LDS stages) and the first 206 (the placements from HBM): the world column of
    the first 205 spheres bit for bit, and the self column on the pairs both handles have"""
    w5, w6 = BC.table_case(BC.row("tree170", 205)), BC.table_case(BC.row("tree170", 206))
    assert np.array_equal(w5["q0"], w6["q0"]) and np.array_equal(w5["col"]["spheres"], w6["col"]["spheres"][:205])
    got = []
    for w in (w5, w6):
        c = w["col"]
        s = TC._open(w["model"], w["q0"])
        s.set_collision_spheres(c["links"], c["spheres"])
        s.set_collision_world(w6["col"]["ws"], w6["col"]["wb"])
        s.set_self_collision(True)
        got.append(s.avoidance_box(None, TB.DT, -np.inf, np.inf, **TB.PRM))
        s.close()
    a, b = got
    assert np.isfinite(a["pairs"][:, :, 0]).all() and np.isfinite(a["pairs"][:, :, 1]).any()
    assert np.array_equal(a["pairs"][:, :, 0], b["pairs"][:, :205, 0]) and np.array_equal(a["partner"][:, :, 0], b["partner"][:, :205, 0])
    # sphere 205 is the second of its self pairs: where it is not the partner, the nearest of the pairs both handles have is the answer
    both = b["partner"][:, :205, 1] != 205
    assert both.mean() >= 0.9
    assert np.array_equal(a["pairs"][:, :, 1][both], b["pairs"][:, :205, 1][both]) and np.array_equal(a["partner"][:, :, 1][both], b["partner"][:, :205, 1][both])
    assert np.all(b["pairs"][:, :205, 1][~both] <= a["pairs"][:, :, 1][~both])


# ---- 3. lock-step parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BC.PARITY, ids=lambda c: c[0])
def test_solve_pose_matches_lockstep_oracle(case):
    w = BC.parity_case(case)
    for k in BC.STEPS:
        out, q, o, same = R._solve_pose_parity(w, BC.LAW[0], BC.LAW[1], k, ("avoid_big", case[0], k), case[3] > 0, exact=True)
        assert not o["near"].any() and same.all()
        assert (o["avoid_active_steps"] > 0).mean() >= 0.25 and np.all(out["avoid_active_steps"] <= out["steps"])
        assert np.array_equal(out["avoid_flags"], o["avoid_flags"])


# ---- 4. the base box comes back on the HBM route ------------------------------------------------------------------------------------------------
def test_base_box_comes_back_on_the_hbm_route():
    """the second half of test_avoid_routes.test_per_instance_base_box_comes_back on the 206 spheres of tree170, in fp64"""
    w = BC.back_case()
    assert BC.launch_shape(170, w["ns"])[0]
    s, t = _latched(w), _latched(w, avoid=None)
    out = s.SolvePose(w["tg"], dt=BC.LAW[0], gain=BC.LAW[1], tol_pose=TOL, max_steps=2)
    t.SolvePose(w["tg"], dt=BC.LAW[0], gain=BC.LAW[1], tol_pose=TOL, max_steps=2)
    q = s.get("q")
    assert (out["avoid_active_steps"] > 0).any() and not np.array_equal(q, t.get("q"))
    R._cold_solve_in_the_base_box(s, t, w, q, BC.LAW[0], BC.LAW[1])
    s.close(); t.close()


# ---- 5. the loops beside SolvePose --------------------------------------------------------------------------------------------------------------
def test_path_of_one_waypoint_and_track():
    """SolvePosePath over one waypoint is SolvePose bit for bit; every z_traj[b, k] of TrackPose lies inside the clamped query at
    q_traj[b, k] (test_avoid_routes.test_track_through_the_wall_keeps_every_z_inside_the_clamped_query)"""
    w = BC.loops_case()
    assert BC.launch_shape(330, w["ns"]) == (True, 2)
    kw = dict(dt=BC.LAW[0], gain=BC.LAW[1], tol_pose=TOL, max_steps=2)
    res = []
    for path in (False, True):
        h = _latched(w)
        o = h.SolvePosePath(w["tg"][:, None], **kw) if path else h.SolvePose(w["tg"], **kw)
        res.append((o, h.get("q"), h.get("z")))
        h.close()
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2]) and (res[0][0]["avoid_active_steps"] > 0).any()
    for f in R.RESULTS + ("steps", "status"):
        assert np.array_equal(res[0][0][f], res[1][0][f]), f
    B, T, nv = w["B"], BC.TRACK_T, w["model"].nv
    lb, ub = w["box"]
    s = _latched(w)
    out = s.TrackPose(BC.track_samples(w), dt=BC.LAW[0], gain=BC.LAW[1], tol_track=1e-3, feedforward="difference")
    qt, zt = out["q_traj"], out["z_traj"]
    assert np.isfinite(qt).all() and np.isfinite(zt).all()
    inf = np.inf * np.ones(nv)
    box = s.avoidance_box(qt[:, :T].reshape(B * T, -1), BC.LAW[0], -inf, inf, **AVOID)
    s.close()
    lo = np.minimum(np.maximum(box["lo"], lb), ub).reshape(B, T, nv)
    hi = np.minimum(np.maximum(box["hi"], lb), ub).reshape(B, T, nv)
    assert np.all(zt >= lo) and np.all(zt <= hi), float(np.maximum(lo - zt, zt - hi).max())
    narrowed = (lo > lb) | (hi < ub)
    assert np.array_equal(out["avoid_active_steps"], narrowed.any(axis=2).sum(axis=1))
    assert np.array_equal(out["avoid_flags"], (lo[:, T - 1] > lb).astype(np.int32) | ((hi[:, T - 1] < ub).astype(np.int32) << 1))
    rests = (((zt == lo) & (lo > lb)) | ((zt == hi) & (hi < ub))).any(axis=(0, 1))
    print("avoid_big track: narrowed instance-steps %d | DoFs with a z entry resting on a narrowed side %s" % (int(narrowed.any(axis=2).sum()), np.flatnonzero(rests).tolist()))
    assert narrowed.any(axis=2).any(axis=1).mean() >= 0.25 and rests.any()
