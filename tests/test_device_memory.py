"""GPU: what a handle takes from the device it gives back.  The library counts what is live through its two allocators (device and
pinned host memory: allocations and bytes, loikb_debug_device_memory, an undeclared debug export); the counters are the process's own,
so nothing else on the card disturbs them and every comparison here is exact.

  1. a handle that has used every buffer it can own returns all four counters to their values before create, three times over;
  2. a buffer that grows on demand (waypoint and step counts, the clearance's placement records) grows once, and what the calls
     return equals, bit for bit, a fresh handle's answer to the same call;
  3. a collision model that replaces another frees it.

panda7, batch 67 (one instance past a wavefront: the last tile is partial), fp64, and one fp32 handle for the reference table's two
precisions.  Allocation failures are not provoked here: tests/cpp/test_devmem.cpp covers those paths on the CPU."""
import ctypes as C

import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from helpers import FIXTURE, feasible_batch
from test_pose_ik import BOUND, PRM, _links
import clearance_numpy as CN
import pose_numpy as P

pytestmark = pytest.mark.gpu

B = 67
COLD = dict(PRM, warm_start=False)   # (every inner solve starts cold: what a call returns does not depend on the handle's earlier calls)


def _counters():
    out = (C.c_ulonglong * 4)()
    assert capi.lib().loikb_debug_device_memory(out) == 0
    return tuple(int(x) for x in out)


def _pose_handle(model, q0, **kw):
    links = _links(model, 1)
    s = loik_amd.BatchedLoik(model, B, **dict(COLD, num_eq_c=1, **kw))
    s.SolveInit(q0, np.eye(6), np.zeros(6), np.array(links, dtype=np.int32), np.eye(6)[None], np.zeros((B, 1, 6)),
                -BOUND * np.ones(model.nv), BOUND * np.ones(model.nv))
    return s


@pytest.fixture(scope="module")
def w():
    """configurations, targets, waypoints and samples (up to 9 steps), sphere models: computed once, never written to"""
    model = loik_amd.builtin_model("panda7")
    rng = np.random.default_rng(2024)
    links = _links(model, 1)
    lo, hi = np.array(model.q_lo, dtype=float), np.array(model.q_hi, dtype=float)
    q0 = model.random_configurations(rng, B)
    # a trajectory of ten poses per instance: FK along a short random joint-space line from q0
    v = 0.02 * rng.normal(size=(B, model.nv))
    poses = np.stack([P.fk12(model, np.stack([P.integrate(model, q0[b], (t + 1) * v[b]) for b in range(B)]), links) for t in range(10)], axis=1)
    small = CN.make_spheres(model, 2, 600)
    other = CN.make_spheres(model, 3, 601)
    # 290 spheres per link: 2030 centres and the placements of 7 joints and 7 carriers are more than a wavefront's 64 KB of LDS --
    # the clearance kernels' instantiation that takes the placements from device memory (d_place), the motion check's slab (d_mslab)
    dense = CN.make_spheres(model, 290, 602)
    world = np.array([[0.4, 0.1, 0.5, 0.1], [-0.3, 0.2, 0.3, 0.05]])
    box = np.concatenate([np.eye(3).reshape(9), [0.5, -0.4, 0.2], [0.1, 0.2, 0.1]])[None]
    q_many = model.random_configurations(rng, 300)
    return dict(model=model, links=links, lo=lo, hi=hi, q0=q0, poses=poses, small=small, other=other, dense=dense, world=world, box=box,
                q_many=q_many)


def _use_everything(w):
    """one handle of each kind through every buffer it can own, closed at the end"""
    model, q0, poses = w["model"], w["q0"], w["poses"]
    # ---- the solver: both layouts of A, the result getters, the getter scratch, the pass state
    prm = dict(FIXTURE, max_iter=60)
    wl = feasible_batch(model, B, 7, 11)
    wa = feasible_batch(model, B, 7, 11, per_instance_A=True)
    for precision in (capi.F64, capi.F32):
        s = loik_amd.BatchedLoik(model, B, precision=precision, **prm)
        for x in (wl, wa):   # (A shared, then A per instance: ensure_layout's relayout)
            s.SolveInit(x["q"], x["H_ref"], x["v_ref"], x["c_ids"], x["Ais"], x["bis"], x["lb"], x["ub"])
            s.Solve()
        assert s.get_results(("z", "nu"))["z"].shape == (B, model.nv)
        assert s.get_results(("z", "w", "scalars"))["scalars"].shape == (B, s.NSCALARS)
        assert np.isfinite(s.get("UDinv")).all() and np.isfinite(s.get("pis")).all()
        if precision == capi.F64:
            s.SolveInit(wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])
            s.FwdPass1()
            assert np.isfinite(s.get("pis")).all()
        s.close()
    s = loik_amd.BatchedLoik(model, B, logging=True, **prm)
    s.SolveInit(wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])
    s.Solve()
    assert s.solver_info()["rows"].min() >= 1
    s.close()
    # ---- the pose layer
    s = _pose_handle(model, q0)
    s.set_joint_limits(w["lo"], w["hi"])
    s.set_joint_accel_limits(50.0 * np.ones(model.nv))
    s.SolvePose(poses[:, 0], dt=0.5, gain=0.8, tol_pose=1e-6, max_steps=4, q=q0)
    s.set_joint_accel_limits(np.inf * np.ones(model.nv))   # (step control and acceleration limits exclude each other)
    s.set_step_control()
    s.SolvePose(poses[:, 0], dt=0.5, gain=0.8, tol_pose=1e-6, max_steps=4, q=q0)
    s.clear_step_control()
    s.SolvePosePath(poses[:, :3], dt=0.5, gain=0.8, tol_pose=1e-4, max_steps=6, record=True, q=q0)
    s.TrackPose(poses[:, :4], dt=0.5, gain=0.8, record=("q", "z"), q=q0)
    # ---- the collision model: spheres twice with different counts, the world twice, self pairs on, off, on
    s.set_collision_spheres(*w["small"])
    first = _counters()[0]
    s.set_collision_spheres(*w["dense"])
    second = _counters()[0]
    s.set_collision_world(spheres=w["world"])
    s.set_collision_world(spheres=w["world"][:1], boxes=w["box"])
    assert np.isfinite(s.clearance(q0)["min"]).all()                                       # (d_place)
    assert s.path_clearance(np.stack([q0, w["q_many"][:B]], axis=1), max_evals=8)["status"].shape == (B, 1)   # (d_mslab)
    s.set_collision_spheres(*w["small"])   # (back to the small model: two million self pairs of the dense one serve nothing here)
    s.set_self_collision(True)
    with_pairs = _counters()[0]
    s.set_self_collision(False)
    assert _counters()[0] == with_pairs - 1
    s.set_self_collision(True, ignore=[(1, 3)])
    assert _counters()[0] == with_pairs
    assert np.isfinite(s.clearance()["min"]).all()
    # ---- tasks, then the multi-start with the dexterity pick and with the clearance latch (one goal, 67 seeds)
    s.set_pose_tasks(["position"])
    s.SolvePoseMultiStart(poses[:1, 0], B, seed=3, pick="dexterous", q0=q0[:1], tol_pose=1e-4, max_steps=4)
    s.SolvePoseMultiStart(poses[:1, 0], B, seed=3, q0=q0[:1], tol_pose=1e-4, max_steps=4, clearance_margin=0.01)
    s.close()
    return first, second


def test_close_gives_back_everything_a_handle_took(w):
    """every owner of device or pinned memory driven once, then close(): the four counters are what they were before create, exactly;
    and three such cycles in one process leave them level"""
    before = _counters()
    for cycle in range(3):
        first, second = _use_everything(w)
        assert _counters() == before, (cycle, before, _counters())
        # the second sphere model took the place of the first: three buffers each (spheres, their carriers' indices, the carriers)
        assert second == first, (first, second)


def test_replacing_a_collision_model_frees_the_old_one(w):
    """set_spheres twice: as many live device allocations after the second as after the first -- one fewer when the first had self
    pairs and the second has none (all its spheres on one link)"""
    s = _pose_handle(w["model"], w["q0"])
    s.set_collision_spheres(*w["small"])
    first = _counters()
    s.set_collision_spheres(*w["other"])
    second = _counters()
    assert second[0] == first[0] and second[1] > first[1]
    s.set_self_collision(True)
    assert s.num_self_pairs() > 0 and _counters()[0] == second[0] + 1
    s.set_collision_spheres(*w["small"])                     # (self pairs stay on: the list is rebuilt for the new model)
    assert s.num_self_pairs() > 0 and _counters()[0] == second[0] + 1
    s.set_collision_spheres(*CN.make_spheres(w["model"], 4, 603, links=[7]))
    assert s.num_self_pairs() == 0 and _counters()[0] == second[0]
    s.set_collision_spheres(np.zeros(0, dtype=np.int32), np.zeros((0, 4)))
    assert _counters()[0] == second[0] - 3
    s.close()


# ---- 2. growth ---------------------------------------------------------------------------------------------------------------
PATH_FIELDS = ("cursor", "path_status", "wsteps", "q_path")
TRACK_FIELDS = ("q_traj", "z_traj", "errmax", "inner", "ontrack", "worst", "worst_at")


def _path_call(s, w, T):
    s.SolvePosePath(w["poses"][:, :T], dt=0.5, gain=0.8, tol_pose=1e-4, max_steps=2 * T, record=True, q=w["q0"])
    return {f: s.path_get(f) for f in PATH_FIELDS}


def _track_call(s, w, T):
    s.TrackPose(w["poses"][:, :T + 1], dt=0.5, gain=0.8, record=("q", "z"), q=w["q0"])
    return {f: s.track_get(f) for f in TRACK_FIELDS}


def _clearance_call(s, w, n):
    r = s.clearance(w["q_many"][:n])
    return {k: r[k] for k in ("min", "min_world", "min_self", "witness")}


def _clearance_handle(w):
    s = _pose_handle(w["model"], w["q0"])
    s.set_collision_spheres(*w["dense"])
    s.set_collision_world(spheres=w["world"], boxes=w["box"])
    return s


def _same_bits(got, want, what):
    for f in want:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f)
        assert got[f].tobytes() == want[f].tobytes(), (what, f)


@pytest.mark.parametrize("kind", ["path", "track", "clearance"])
def test_growth_keeps_results_right_and_does_not_accumulate(w, kind):
    """sizes small, large, small on one handle: after each call every field of the getter equals, bit for bit, a fresh handle's after
    the same call; the second call replaces buffers by larger ones (as many live allocations, more bytes) and the third allocates
    nothing -- the buffers grown for the second serve it.
    (clearance: the dense sphere model of panda7, 2030 spheres, is the one whose placements do not fit the LDS, so d_place grows with
    n here: 67, 300, 67 configurations.)"""
    call, open_, sizes = {"path": (_path_call, lambda: _pose_handle(w["model"], w["q0"]), (3, 9, 3)),
                          "track": (_track_call, lambda: _pose_handle(w["model"], w["q0"]), (3, 9, 3)),
                          "clearance": (_clearance_call, lambda: _clearance_handle(w), (67, 300, 67))}[kind]
    fresh = {}
    for n in sorted(set(sizes)):
        f = open_()
        fresh[n] = call(f, w, n)
        f.close()
    s = open_()
    live = []
    for n in sizes:
        got = call(s, w, n)
        live.append(_counters()[:2])
        _same_bits(got, fresh[n], "%s, size %d after %s" % (kind, n, sizes[:len(live) - 1]))
    # the second call grew buffers, each in place of its smaller self; the third found them large enough
    assert live[1][0] == live[0][0] and live[1][1] > live[0][1], live
    assert live[2] == live[1], live
    s.close()
