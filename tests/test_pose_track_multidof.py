"""GPU: timed trajectories (include/loik_amd_track.h) on robots with nq != nv -- the four multi-DoF trees of
test_pose_ik._fk_models()[2:6].  k_track_record runs one thread per max(nq, nv) and writes Q[B][T+1][nq] and Z[B][T][nv], and the
feed-forward is transported through the frame of a link that hangs under a free-flyer: a stride taken from the wrong width passes
every test on Talos-32 and Panda-7.  Parity with the lock-step tracking oracle under test_pose_track._track_gate, unchanged, on
links from test_pose_parity._leaf_and_multidof with a per-instance non-symmetric A; the device's own numbers (z_traj reproduces
q_traj through the integrator -- the assertion that fails when a Q or Z stride uses the wrong width); a start ON the path without
feed-forward, where the first step is |z| <= 3e-15 and the integrator's zero-angle branch runs inside the loop; a NaN in a
quaternion coordinate; and SolvePose bit for bit.

The seeds in the case table were chosen on the CPU so that the 99 % gate tests the device and not the case: the oracle run twice,
as given and with q0 scaled by 1 + 1e-13, agrees with itself on every instance (profiles/pose_multidof_parity.md)."""
import numpy as np
import pytest

from loik_amd import capi

from test_pose_ik import PRM, _fk_models
from test_pose_parity import _box, _handle, _leaf_and_multidof, _nonsym_A, _subset
from test_pose_track import (FFS, _check_nan_seed_stops_alone, _check_no_feedforward_is_solve_pose, _check_trajectories_and_feedforward,
                             _download, _track_gate, _track_workload)
from test_pose_path_multidof import TREES, _quaternions_are_unit
import integrate_mp as MP
import pose_limits_numpy as PL
import pose_tasks_numpy as PT
import pose_track_numpy as TR

pytestmark = pytest.mark.gpu

B, T = 128, 5
TOL_TRACK = 1e-4
KINDS = ["position", "orientation"]

PARITY = [
    # (tree, (gain, dt), feed-forward, variant, workload seed); the seed is chosen so that the oracle agrees with itself
    # under a 1e-13 change of q0
    (2, (1.0, 1.0), "difference", "plain", 6201),
    (2, (0.5, 0.25), "none", "plain", 6211),
    (3, (0.5, 0.25), "difference", "plain", 6301),
    (3, (1.0, 1.0), "none", "plain", 6311),
    (4, (1.0, 1.0), "difference", "plain", 6401),
    (4, (0.5, 0.25), "none", "plain", 6411),
    (5, (0.5, 0.25), "difference", "plain", 6501),
    (5, (1.0, 1.0), "none", "plain", 6511),
    (2, (0.5, 0.25), "difference", "limits", 6221),
    (3, (1.0, 1.0), "difference", "limits", 6321),
    (3, (0.5, 0.25), "difference", "tasks", 6331),
    (2, (1.0, 1.0), "difference", "device", 6241),
]


def _case_id(c):
    return "%s-g%g-dt%g-%s-%s" % (TREES[c[0]], c[1][0], c[1][1], c[2], c[3])


def _inputs(case):
    """everything a parity case is made of, for the device run and for the oracle"""
    k, (gain, dt), ff, variant, seed = case
    model = _fk_models()[k]
    links = _leaf_and_multidof(model)
    nc = len(links)
    rng = np.random.default_rng(seed + 1)
    tasks, limits = variant == "tasks", variant == "limits"
    frames = PT.random_frames(rng, nc) if tasks else None
    # (with tasks the constraint matrix is the task's own, A_c = S_c X_c^-1: the handle's A is replaced and the oracle ignores it)
    A = np.tile(np.eye(6), (nc, 1, 1)) if tasks else _nonsym_A(rng, nc, B)
    q0, smp, q_path = _track_workload(model, links, B, T, seed=seed, frames=frames)
    w = dict(model=model, links=links, nc=nc, A=A, q0=q0, smp=smp, frames=frames, okw={}, q_lo=None, q_hi=None, ff=ff, box=_box(model),
             kw=dict(dt=dt, gain=gain, tol_track=TOL_TRACK, feedforward=ff))
    if limits:
        w["q_lo"], w["q_hi"], w["q0"] = PL.binding_limits(model, q_path[:, T], q0, seed + 2)
        w["okw"].update(q_lo=w["q_lo"], q_hi=w["q_hi"])
    if tasks:
        w["okw"].update(kinds=[capi.TASK_KINDS[kind] for kind in KINDS[:nc]], frames=frames)
    return w


def _oracle(w, idx, q0=None):
    """the lock-step oracle on the instances idx; q0: other seeds (scripts/pose_multidof_seed_agreement.py perturbs them)"""
    kw = w["kw"]
    lb, ub = w["box"]
    q0 = w["q0"] if q0 is None else q0
    return TR.lockstep_track_loop(w["model"], PRM, q0[idx], np.eye(6), np.zeros(6), w["links"], w["A"][idx] if w["A"].ndim == 4 else w["A"],
                                  lb, ub, w["smp"][idx], kw["dt"], kw["gain"], TOL_TRACK, ff=FFS[w["ff"]], **w["okw"])


@pytest.mark.parametrize("case", PARITY, ids=_case_id)
def test_track_matches_lockstep_track_oracle_on_multidof_trees(case):
    _, _, ff, variant, _ = case
    w = _inputs(case)
    model, links, q0, smp = w["model"], w["links"], w["q0"], w["smp"]
    s = _handle(model, B, links, q0, w["A"], PRM, box=w["box"])
    if variant == "tasks":
        s.set_pose_tasks(KINDS[:w["nc"]], w["frames"])
    if variant == "limits":
        s.set_joint_limits(w["q_lo"], w["q_hi"])
    if variant == "device":
        out = s.TrackPose(capi.DeviceArray(smp), q=capi.DeviceArray(q0), **w["kw"])
        for key, dtype in (("q_traj", np.float64), ("z_traj", np.float64), ("errmax", np.float64), ("inner", np.int32), ("ontrack", np.int32),
                           ("worst", np.float64), ("worst_at", np.int32)):
            dev = capi.DeviceArray(np.zeros(out[key].size))
            s.track_get(key, out=dev)
            assert np.array_equal(_download(dev, out[key].shape, dtype), out[key], equal_nan=True), key
            dev.free()
    else:
        out = s.TrackPose(smp, **w["kw"])
    q = s.get("q")
    timing = s.track_get("timing")
    s.close()
    idx = _subset(B)
    o = _oracle(w, idx)
    same = _track_gate(out, o, idx, _case_id(case))
    # the shapes: q_traj has nq columns, z_traj nv
    assert out["q_traj"].shape == (B, T + 1, model.nq) and out["z_traj"].shape == (B, T, model.nv) and q.shape == (B, model.nq)
    assert timing["steps"] == T and np.all(out["steps"] == T) and not out["reached"].any()
    assert np.array_equal(out["q_traj"][:, T], q) and np.array_equal(out["q_traj"][:, 0], q0)
    assert _quaternions_are_unit(model, out["q_traj"]) <= 1e-12
    assert np.max(np.abs(out["err"][idx][same] - o["err"][same])) < 1e-7
    assert np.mean(out["ontrack"][idx][same] != o["ontrack"][same]) <= 0.01   # (an errmax within rounding of tol_track may fall on either side)
    assert np.max(np.abs(out["worst"][idx][same] - o["worst"][same])) < 1e-7
    if variant == "limits":
        assert (out["limit_flags"][idx][same] != o["limit_flags"][same]).any(axis=1).mean() <= 0.01
        lim = np.isfinite(w["q_lo"]) | np.isfinite(w["q_hi"])
        ci = PL.limit_q_index(model)[lim]
        assert np.all(w["q_lo"][lim] <= q[:, ci]) and np.all(q[:, ci] <= w["q_hi"][lim])
        assert (o["inner"] & TR.IN_LIMIT).any()
    if ff == "difference" and variant != "limits":   # the case means something: the seeds are off the path and the loop pulls them in
        assert np.median(o["errmax"][:, T]) < 0.5 * np.median(o["errmax"][:, 0])


@pytest.mark.parametrize("k", [2, 3], ids=lambda k: TREES[k])
def test_trajectories_are_consistent_and_feedforward_tracks_better_on_free_flyer_trees(k):
    model = _fk_models()[k]
    res = _check_trajectories_and_feedforward(model, _leaf_and_multidof(model), B)
    # the start is ON the path: without feed-forward the first step is a zero step (the oracle's |z| <= 3e-15 there), so the
    # integrator's zero-angle branch runs inside the loop -- and stops no instance
    none = res["none"]
    print("pose_track_measured %s on the path, no feed-forward: max |z_traj[:, 0]| = %.3e" % (model.name, np.abs(none["z_traj"][:, 0]).max()))
    assert np.abs(none["z_traj"][:, 0]).max() < 1e-9
    for out in res.values():
        assert not (out["status"] & capi.POSE_ST_STOPPED).any() and np.all(out["steps"] == T)
        assert not np.isnan(out["q_traj"]).any() and not np.isnan(out["z_traj"]).any() and not np.isnan(out["errmax"]).any()
        assert out["q_traj"].shape == (B, T + 1, model.nq) and out["z_traj"].shape == (B, T, model.nv)
        assert _quaternions_are_unit(model, out["q_traj"]) <= 1e-12


def test_nan_in_a_quaternion_coordinate_stops_that_instance_alone():
    model = _fk_models()[2]
    quat = [o for o, n in MP.unit_blocks(model) if n == 4][0]
    _check_nan_seed_stops_alone(model, _leaf_and_multidof(model), B, 37, quat + 1)


@pytest.mark.parametrize("form", ["Ainst", "limits"])
def test_no_feedforward_on_constant_samples_is_solve_pose_bit_for_bit_on_a_free_flyer_tree(form):
    model = _fk_models()[3]
    _check_no_feedforward_is_solve_pose(model, _leaf_and_multidof(model), B, form)
