"""GPU: a recorded SolvePosePath through path_clearance (include/loik_amd_motion.h).  Panda-7 follows four waypoints; a box of half
thickness 0.005 stands across the tool sphere's way between the second and the third.  The clearance query finds every recorded
configuration clear; the certified check of the segments between them finds the box."""
import numpy as np
import pytest

import clearance_numpy as CN
import motion_numpy as MN
import pose_numpy as P
import qp_cases as QC
from test_motion_clearance import _compare
from test_pose_ik import _handle

pytestmark = pytest.mark.gpu


def test_a_thin_box_between_two_waypoints():
    model = QC.model_of("panda7")
    B, T, tool = 4, 4, 7
    rng = np.random.default_rng(900)
    q0 = np.tile(model.random_configurations(rng, 1), (B, 1))
    step = np.array([0.25, -0.2, 0.15, 0.25, -0.2, 0.15, 0.1])
    rows = np.clip(q0[0][None] + np.arange(T)[:, None] * step[None], model.q_lo, model.q_hi)
    wp = np.tile(P.fk12(model, rows, [tool])[None], (B, 1, 1, 1))          # [B][T][1][12]: every instance the same path
    s, _ = _handle(model, B, [tool], q0)
    links, spheres = np.array([tool], dtype=np.int32), np.array([[0.0, 0.0, 0.1, 0.01]])
    s.set_collision_spheres(links, spheres)
    path = s.SolvePosePath(wp, tol_pose=1e-6, max_steps=200)
    q_path = path["q_path"]
    assert path["reached"].all() and np.isfinite(q_path).all() and q_path.shape == (B, T, model.nq)
    # the box across segment 1 of the recorded path
    dv = MN.difference(model, q_path[0, :-1], q_path[0, 1:])
    box = MN.thin_box_across(model, q_path[0, 1], dv[1], tool, spheres[0])
    s.set_collision_world(None, box[None])
    at = s.clearance(q_path.reshape(-1, model.nq))
    assert np.all(at["min"] > 1e-3), at["min"]
    got = s.path_clearance(q_path, margin=0.0, tol=1e-3, max_evals=256)
    assert got["status"].shape == (B, T - 1) and got["witness"].shape == (B, T - 1, 3)
    assert np.all(got["status"][:, 1] == MN.BLOCKED) and np.all(got["status"][:, [0, 2]] == MN.FREE), got["status"]
    assert np.all((got["s_free"][:, 1] > 0.0) & (got["s_free"][:, 1] < 1.0)) and np.all(got["witness"][:, 1] == [CN.WORLD_BOX, 0, 0])
    # ... and it is the reference's answer: the difference of consecutive samples, then the advancement
    qa = q_path[:, :-1].reshape(-1, model.nq)
    dvs = MN.difference(model, qa, q_path[:, 1:].reshape(-1, model.nq))
    want = MN.advance(model, qa, dvs, links, spheres, wboxes=box[None], margin=0.0, tol=1e-3, max_evals=256)
    flat = {k: v.reshape((-1,) + v.shape[2:]) for k, v in got.items()}
    ends = MN.centres(model, q_path.reshape(-1, model.nq), links, spheres)
    _compare(flat, want, 1.0 + float(np.max(np.abs(ends))) + 0.01, "panda7 recorded path")
    # the same through motion_clearance with the end points, and a path with a row that is not finite: its two segments alone are INVALID
    via = s.motion_clearance(qa, qb=q_path[:, 1:].reshape(-1, model.nq), margin=0.0, tol=1e-3, max_evals=256)
    assert all(np.array_equal(via[k], flat[k]) for k in flat)
    broken = q_path.copy()
    broken[2, 1, 0] = np.nan
    bad = s.path_clearance(broken, margin=0.0, tol=1e-3, max_evals=256)
    assert np.all(bad["status"][2, :2] == MN.INVALID) and bad["status"][2, 2] == MN.FREE
    keep = np.arange(B) != 2
    assert all(np.array_equal(bad[k][keep], got[k][keep]) for k in got)
    s.close()
