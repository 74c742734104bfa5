"""GPU: a recorded SolvePosePath through path_clearance (include/loik_amd_motion.h).  Panda-7 follows four waypoints; a box of half
thickness 0.005 stands across the tool sphere's way between the second and the third.  The clearance query finds every recorded
configuration clear; the certified check of the segments between them finds the box.

Then paths that differ from instance to instance, on robots with nq != nv: motion_row and the T > 0 form of k_difference are the only
code that turns (b, t) into rows, and equal instances cannot show a confusion between them."""
import ctypes as C

import numpy as np
import pytest

from loik_amd import capi

import clearance_numpy as CN
import motion_numpy as MN
import pose_numpy as P
import qp_cases as QC
from test_motion_clearance import MAX_EVALS, SIZE, TOL, _compare, _open, _same, motion_case
from test_pose_ik import _handle

pytestmark = pytest.mark.gpu

# Paths that differ from instance to instance, on the two robots with nq != nv (multidof13: a free-flyer's quaternion, (cos, sin) blocks;
# composite20: a (cos, sin) sub-joint inside a composite), so that q_path and the differences have different strides.  (B, T): T = 2
# is motion_row(i, T) = 2 i; (13, 6) is 65 segments, one past a workgroup of k_difference
PATH_ROBOTS = ["multidof13", "composite20"]
PATH_SIZES = [(5, 2), (5, 3), (3, 7), (13, 6)]

_PATHS = {}


def path_case(name, B, T):
    """the model, spheres, world, pairs and margin of motion_case(name); B paths of T samples, path b from a random start by steps
    q[b][t + 1] = q[b][t] (+) dv[b][t] with dv = SIZE * uniform(-1, 1) of its own; the segments flattened (qa, qb) and the numpy answer,
    the reference's difference of consecutive samples, then its advancement: computed once"""
    key = (name, B, T)
    if key not in _PATHS:
        c = dict(motion_case(name))
        model = c["model"]
        rng = np.random.default_rng(920 + 100 * PATH_ROBOTS.index(name) + 10 * PATH_SIZES.index((B, T)))
        q_path = np.empty((B, T, model.nq))
        q_path[:, 0] = model.random_configurations(rng, B)
        for t in range(T - 1):
            dv = SIZE[name] * rng.uniform(-1.0, 1.0, size=(B, model.nv))
            for b in range(B):
                q_path[b, t + 1] = MN.interpolate(model, q_path[b, t], dv[b], 1.0)
        qa, qb = q_path[:, :-1].reshape(-1, model.nq), q_path[:, 1:].reshape(-1, model.nq)
        c.update(q_path=q_path, qa=qa, qb=qb, B=B, T=T, kw=dict(margin=c["margin"], tol=TOL, max_evals=MAX_EVALS))
        c["want"] = MN.advance(model, qa, MN.difference(model, qa, qb), c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], **c["kw"])
        cen = MN.centres(model, q_path.reshape(-1, model.nq), c["links"], c["spheres"])
        c["scale"] = 1.0 + float(np.max(np.abs(cen))) + float(np.max(c["spheres"][:, 3]))
        _PATHS[key] = c
    return _PATHS[key]


def _flat(r):
    return {k: v.reshape((-1,) + v.shape[2:]) for k, v in r.items()}


@pytest.mark.parametrize("B,T", PATH_SIZES)
@pytest.mark.parametrize("name", PATH_ROBOTS)
def test_paths_that_differ(name, B, T):
    c = path_case(name, B, T)
    model, q_path, kw = c["model"], c["q_path"], c["kw"]
    n = B * (T - 1)
    s = _open(c)
    got = s.path_clearance(q_path, **kw)
    assert got["status"].shape == (B, T - 1) and got["witness"].shape == (B, T - 1, 3)
    flat = _flat(got)
    # the flattened consecutive rows through motion_clearance with the end points: the device's difference both ways, the same bits
    assert _same(flat, s.motion_clearance(c["qa"], qb=c["qb"], **kw))
    # the reference: difference, then the advancement
    _compare(flat, c["want"], c["scale"], "%s paths %d x %d" % (name, B, T))
    # the instances permuted: the answers go with them
    perm = np.roll(np.arange(B)[::-1], 1)
    assert _same(s.path_clearance(q_path[perm].copy(), **kw), {k: v[perm] for k, v in got.items()})
    # a row that is not finite: the one or two segments that touch it are INVALID, every other keeps its bits
    for b, t in ((0, 0), (B - 1, T - 1), (B // 2, T // 2)):
        broken = q_path.copy()
        broken[b, t, (b + t) % model.nq] = np.nan
        bad = _flat(s.path_clearance(broken, **kw))
        touched = [b * (T - 1) + u for u in (t - 1, t) if 0 <= u < T - 1]
        assert len(touched) == (2 if 0 < t < T - 1 else 1)
        for i in touched:
            assert bad["status"][i] == MN.INVALID and bad["evals"][i] == 0 and tuple(bad["witness"][i]) == (CN.NONE, -1, -1)
            assert np.isnan([bad["s_free"][i], bad["min_sampled"][i], bad["s_at_min"][i]]).all()
        keep = ~np.isin(np.arange(n), touched)
        assert _same({k: v[keep] for k, v in bad.items()}, {k: v[keep] for k, v in flat.items()}), (b, t)
    # a device tensor in, device buffers out
    dq = capi.DeviceArray(q_path)
    assert _same(got, s.path_clearance(dq, **kw))
    val, info = capi.DeviceArray(np.full(3 * n, -1.0)), capi.DeviceArray(np.zeros((5 * n + 1) // 2))
    s.path_clearance(dq, out=(val, info), **kw)
    hip = capi.DeviceArray.hip()
    v, i = np.empty((n, 3)), np.empty((5 * n + 1) // 2)
    assert hip.hipMemcpy(v.ctypes.data_as(C.c_void_p), C.c_void_p(val.data_ptr()), v.nbytes, 2) == 0   # hipMemcpyDeviceToHost
    assert hip.hipMemcpy(i.ctypes.data_as(C.c_void_p), C.c_void_p(info.data_ptr()), i.nbytes, 2) == 0
    assert _same(flat, capi.BatchedLoik._motion_result(v, i.view(np.int32)[:5 * n].reshape(n, 5)))
    for a in (dq, val, info):
        a.free()
    s.close()


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
