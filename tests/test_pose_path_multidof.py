"""GPU: waypoint paths (include/loik_amd_path.h) on robots with nq != nv -- the four multi-DoF trees of
test_pose_ik._fk_models()[2:6]: a free-flyer root with a spherical and a translation joint; a free-flyer root with ZYX, planar and
(cos, sin) joints; a composite tree; a helical tree.  k_path_record copies q rows into Q[B][T][nq]: a stride or an index taken
from nv instead passes every test on Talos-32 and Panda-7, where the two are equal.  Parity with the lock-step path oracle under
test_pose_path._path_gate, unchanged, on links from test_pose_parity._leaf_and_multidof with a per-instance non-symmetric A; one
waypoint is SolvePose bit for bit; q_path has nq columns and every recorded quaternion is unit.

The seeds in the case table were chosen on the CPU so that the 99 % gate tests the device and not the case: the oracle run twice,
as given and with q0 scaled by 1 + 1e-13, agrees with itself on every instance (profiles/pose_multidof_parity.md)."""
import numpy as np
import pytest

from loik_amd import capi

from test_pose_ik import PRM, _fk_models
from test_pose_parity import _box, _handle, _leaf_and_multidof, _nonsym_A, _subset
from test_pose_path import TOL, _check_one_waypoint_is_solve_pose, _path_gate, _path_workload
import integrate_mp as MP
import pose_limits_numpy as PL
import pose_path_numpy as PP
import pose_tasks_numpy as PT

pytestmark = pytest.mark.gpu

B = 128
TREES = {2: "ff-sph-trans", 3: "ff-zyx-planar-cs", 4: "composite", 5: "helical"}

PARITY = [
    # (tree, T, (gain, dt), variant, max_steps, budget per waypoint, workload seed); max_steps is chosen on the oracle so that the loop
    # ends with the cursors spread over the path (T = 2: a budget of 2 steps per waypoint and gain 0.85, so that about a third of
    # the instances complete, a half stall on the first waypoint and the rest on the second), the seed so that the oracle agrees
    # with itself under a 1e-13 change of q0
    (2, 5, (1.0, 1.0), "plain", 4, 0, 5201),
    (3, 5, (0.5, 0.25), "plain", 4, 0, 5301),
    (4, 5, (1.0, 1.0), "plain", 4, 0, 5401),
    (5, 5, (0.5, 0.25), "plain", 4, 0, 5501),
    (2, 2, (0.85, 0.5), "plain", 4, 2, 5211),
    (3, 2, (0.85, 1.0), "plain", 4, 2, 5311),
    (4, 2, (0.85, 0.5), "plain", 4, 2, 5411),
    (5, 2, (0.85, 1.0), "plain", 4, 2, 5511),
    (2, 5, (1.0, 0.5), "limits", 4, 0, 5221),
    (3, 5, (1.0, 1.0), "limits", 4, 0, 5323),
    (2, 5, (1.0, 1.0), "tasks", 4, 0, 5231),
    (3, 5, (1.0, 1.0), "device", 4, 0, 5341),
]


def _case_id(c):
    return "%s-T%d-g%g-dt%g-%s-k%d-m%d" % (TREES[c[0]], c[1], c[2][0], c[2][1], c[3], c[4], c[5])


def _inputs(case):
    """everything a parity case is made of, for the device run and for the oracle"""
    k, T, (gain, dt), variant, max_steps, budget, seed = case
    model = _fk_models()[k]
    links = _leaf_and_multidof(model)
    nc = len(links)
    rng = np.random.default_rng(seed + 1)
    tasks, limits = variant == "tasks", variant == "limits"
    frames = PT.random_frames(rng, nc) if tasks else None
    # (with tasks the constraint matrix is the task's own, A_c = S_c X_c^-1: the handle's A is replaced and the oracle ignores it)
    A = np.tile(np.eye(6), (nc, 1, 1)) if tasks else _nonsym_A(rng, nc, B)
    q0, wp, q_t = _path_workload(model, links, B, T, seed=seed, frames=frames)
    w = dict(model=model, links=links, nc=nc, T=T, A=A, q0=q0, wp=wp, frames=frames, okw={}, q_lo=None, q_hi=None, box=_box(model),
             kw=dict(dt=dt, gain=gain, tol_pose=TOL, max_steps=max_steps, max_steps_per_waypoint=budget))
    if limits:
        w["q_lo"], w["q_hi"], w["q0"] = PL.binding_limits(model, q_t, q0, seed + 2)
        w["okw"].update(q_lo=w["q_lo"], q_hi=w["q_hi"])
    if tasks:
        w["okw"].update(kinds=[PT.TASK_POSITION] * nc, frames=frames)
    return w


def _oracle(w, idx, q0=None):
    """the lock-step oracle on the instances idx; q0: other seeds (scripts/pose_multidof_seed_agreement.py perturbs them)"""
    kw = w["kw"]
    lb, ub = w["box"]
    q0 = w["q0"] if q0 is None else q0
    return PP.lockstep_path_loop(w["model"], PRM, q0[idx], np.eye(6), np.zeros(6), w["links"], w["A"][idx] if w["A"].ndim == 4 else w["A"],
                                 lb, ub, w["wp"][idx], kw["dt"], kw["gain"], TOL, kw["max_steps"], budget=kw["max_steps_per_waypoint"],
                                 **w["okw"])


def _quaternions_are_unit(model, rows):
    """rows [..., nq] without NaN: the largest | |quat| - 1 | over the quaternion blocks"""
    worst = 0.0
    for o, n in MP.unit_blocks(model):
        if n == 4:
            worst = max(worst, float(np.max(np.abs(np.linalg.norm(rows[..., o:o + 4], axis=-1) - 1.0))))
    return worst


@pytest.mark.parametrize("case", PARITY, ids=_case_id)
def test_path_matches_lockstep_path_oracle_on_multidof_trees(case):
    k, T, _, variant, _, budget, _ = case
    w = _inputs(case)
    model, links, q0, wp = w["model"], w["links"], w["q0"], w["wp"]
    s = _handle(model, B, links, q0, w["A"], PRM, box=w["box"])
    if variant == "tasks":
        s.set_pose_tasks(["position"] * w["nc"], w["frames"])
    if variant == "limits":
        s.set_joint_limits(w["q_lo"], w["q_hi"])
    if variant == "device":
        out = s.SolvePosePath(capi.DeviceArray(wp), q=capi.DeviceArray(q0), **w["kw"])
    else:
        out = s.SolvePosePath(wp, **w["kw"])
    q = s.get("q")
    timing = s.path_get("timing")
    s.close()
    idx = _subset(B)
    o = _oracle(w, idx)
    print("pose_path_measured %s | oracle cursor %s | path_status %s | steps %s | status %s | loop %d (device %d)"
          % (_case_id(case), np.bincount(o["cursor"], minlength=T + 1).tolist(), np.bincount(o["path_status"], minlength=3).tolist(),
             np.bincount(o["steps"]).tolist(), np.bincount(o["status"], minlength=8).tolist(), o["n_solves"], timing["steps"]))
    same = _path_gate(out, q, o, idx, _case_id(case))
    # the shapes: nq columns, not nv
    assert q.shape == (B, model.nq) and out["q_path"].shape == (B, T, model.nq) and out["wsteps"].shape == (B, T)
    rec = ~np.isnan(out["q_path"]).any(axis=2)
    assert np.array_equal(rec, np.arange(T)[None, :] < out["cursor"][:, None])
    assert not np.isnan(out["q_path"][rec]).any() and np.all(np.isnan(out["q_path"][~rec]))
    if rec.any():
        assert _quaternions_are_unit(model, out["q_path"][rec]) <= 1e-12
    assert _quaternions_are_unit(model, q) <= 1e-12
    assert np.array_equal(out["wsteps"].sum(axis=1), out["steps"])
    assert timing["steps"] == out["steps"].max()
    if variant == "limits":
        assert (out["limit_flags"][idx][same] != o["limit_flags"][same]).any(axis=1).mean() <= 0.01
        lim = np.isfinite(w["q_lo"]) | np.isfinite(w["q_hi"])
        ci = PL.limit_q_index(model)[lim]
        assert np.all(w["q_lo"][lim] <= q[:, ci]) and np.all(q[:, ci] <= w["q_hi"][lim])
        assert (o["limit_flags"] != 0).any()
    # the case means something: instances are spread over the path, and rows are recorded
    assert len(set(o["cursor"].tolist())) > 2 and o["steps"].any() and (o["cursor"] > 0).mean() > 0.25
    if budget:
        assert (o["path_status"] == PP.PATH_STALLED).any()


@pytest.mark.parametrize("k,form", [(3, "Ainst"), (3, "limits"), (3, "tasks"), (4, "Ainst")],
                         ids=lambda v: TREES[v] if isinstance(v, int) else v)
def test_one_waypoint_is_solve_pose_bit_for_bit_on_multidof_trees(k, form):
    model = _fk_models()[k]
    _check_one_waypoint_is_solve_pose(model, _leaf_and_multidof(model), B, form)
