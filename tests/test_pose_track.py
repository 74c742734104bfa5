"""GPU: timed trajectories in the pose loop (include/loik_amd_track.h, loikb_track_pose) -- without feed-forward and on constant
samples the call IS SolvePose, bit for bit; parity with the lock-step tracking oracle (tests/pose_track_numpy.py, proven on the CPU
by tests/test_pose_track_oracle.py) in the manner of tests/test_pose_parity.py's gate: on >= 99 % of the oracle's subset every
q_traj row and every errmax within 1e-7 and inner equal, the NaN pattern identical on all; the device's own numbers (z_traj
reproduces q_traj, worst / worst_at / ontrack follow from errmax, the feed-forward tracks better); a NaN seed; and the errors."""
import ctypes as C

import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from test_pose_ik import PRM, _links
from test_pose_parity import F32_STEP_REL, _box, _handle, _nonsym_A, _subset
from test_pose_path import _path_workload
import pose_numpy as P
import pose_limits_numpy as PL
import pose_tasks_numpy as PT
import pose_track_numpy as TR

pytestmark = pytest.mark.gpu

FFS = {"none": TR.FF_NONE, "difference": TR.FF_DIFFERENCE}


def _kinds(nc):
    return ["pose"] if nc == 1 else ["position", "orientation"][:nc]


def _track_workload(model, links, B, T, seed, spread=(1e-4, 0.05), shared=False, frames=None, on_path=False):
    """samples along the smooth joint paths of pose_track_numpy.joint_path_workload (a sample moves the joints by about 1e-2); the
    seeds are the paths' starts moved off them by a velocity of a size log-uniform in `spread` (test_pose_parity._seeds), so that
    feedback and feed-forward both act -- on_path: not moved.  shared: the path of instance 0 for the batch.
    Returns (q0 [B][nq], samples [B][T+1][nc][12] or [T+1][nc][12], q_path [B][T+1][nq])."""
    q_a, smp, q_path = TR.joint_path_workload(model, links, B, T, seed, frames=frames)
    rng = np.random.default_rng(seed + 1)
    if shared:
        smp, q_a, q_path = smp[0], np.repeat(q_a[:1], B, axis=0), np.repeat(q_path[:1], B, axis=0)
    if on_path:
        return q_a, smp, q_path
    size = np.exp(rng.uniform(np.log(spread[0]), np.log(spread[1]), size=B))
    q0 = np.stack([P.integrate(model, q_a[b], size[b] * rng.normal(size=model.nv) / np.sqrt(model.nv)) for b in range(B)])
    return q0, smp, q_path


def _smp_of(smp, idx):
    return smp[idx] if smp.ndim == 4 else np.broadcast_to(smp, (len(idx),) + smp.shape)


def _track_gate(out, o, idx, what):
    """the NaN pattern of q_traj / z_traj / errmax identical on every instance of the subset; on >= 99 % of them every q_traj row and
    errmax within 1e-7 of the oracle's and inner equal -- and on those the same steps and status"""
    for key in ("q_traj", "z_traj", "errmax"):
        assert np.array_equal(np.isnan(out[key][idx]), np.isnan(o[key])), (what, key)
    with np.errstate(invalid="ignore"):
        dq = np.nan_to_num(np.abs(out["q_traj"][idx] - o["q_traj"])).max(axis=(1, 2))
        de = np.nan_to_num(np.abs(out["errmax"][idx] - o["errmax"])).max(axis=1)
    same_inner = (out["inner"][idx] == o["inner"]).all(axis=1)
    same = (dq < 1e-7) & (de < 1e-7) & same_inner
    print("pose_track_measured %s | same %.4f | max dq %.3e (all %.3e) | max derrmax %.3e | inner differs on %d | oracle errmax by sample %s"
          % (what, same.mean(), dq[same].max() if same.any() else np.nan, dq.max(), de.max(), int((~same_inner).sum()),
             np.nanmax(o["errmax"], axis=0)))
    assert same.mean() >= 0.99, (what, same.mean(), dq.max(), de.max())
    assert np.array_equal(out["steps"][idx][same], o["steps"][same]) and np.array_equal(out["status"][idx][same], o["status"][same]), what
    return same


def _download(dev, shape, dtype):
    """the first bytes of a DeviceArray as a host array of `shape` / `dtype`"""
    host = np.empty(shape, dtype=dtype)
    assert host.nbytes <= dev.size * 8
    assert capi.DeviceArray.hip().hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(dev.data_ptr()), host.nbytes, 2) == 0   # device to host
    return host


# ---- 1. no feed-forward, constant samples: SolvePose bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("form", ["Ash", "Ainst", "tasks", "limits", "f32"])
@pytest.mark.parametrize("name,nc,B", [("talos32", 2, 193), ("panda7", 1, 64), ("talos32", 1, 1)])
def test_no_feedforward_on_constant_samples_is_solve_pose_bit_for_bit(name, nc, B, form):
    model = loik_amd.builtin_model(name)
    _check_no_feedforward_is_solve_pose(model, _links(model, nc), B, form)


def _check_no_feedforward_is_solve_pose(model, links, B, form):
    nc = len(links)
    T = 4
    rng = np.random.default_rng(4000 + B)
    frames = PT.random_frames(rng, nc) if form == "tasks" else None
    q0, wp, q_t = _path_workload(model, links, B, 1, seed=4001 + B + nc, frames=frames)
    tg = wp[:, 0]
    smp = np.repeat(wp, T + 1, axis=1)
    A = _nonsym_A(rng, nc, B) if form == "Ainst" else np.tile(np.eye(6), (nc, 1, 1)) if form == "tasks" else _nonsym_A(rng, nc)
    if form == "limits":
        q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, 4002)
    res = []
    for track in (False, True):
        s = _handle(model, B, links, q0, A, PRM, precision=capi.F32 if form == "f32" else capi.F64)
        if form == "tasks":
            s.set_pose_tasks(["position", "pose"][:nc], frames)
        if form == "limits":
            s.set_joint_limits(q_lo, q_hi)
        if track:
            out = s.TrackPose(smp, dt=0.5, gain=0.8, tol_track=0.0, feedforward="none")
        else:
            out = s.SolvePose(tg, dt=0.5, gain=0.8, tol_pose=0.0, max_steps=T)
        res.append((out, s.get("q"), s.get("z")))
        s.close()
    (a, qa, za), (b, qb, zb) = res
    for key in ("steps", "status", "err") + (("limit_flags",) if form == "limits" else ()):
        assert np.array_equal(a[key], b[key]), (form, key)
    assert np.array_equal(qa, qb) and np.array_equal(za, zb)
    assert np.all(a["steps"] == T) and not a["reached"].any()
    assert np.array_equal(b["q_traj"][:, T], qb) and np.array_equal(b["q_traj"][:, 0], q0) and np.array_equal(b["z_traj"][:, T - 1], zb)
    assert np.array_equal(b["errmax"][:, T], np.abs(b["err"]).max(axis=(1, 2))) and not np.isnan(b["errmax"]).any()
    if form == "limits" and B > 1:
        assert (b["inner"] & capi.TRACK_IN_LIMIT).any()
        assert np.array_equal((b["inner"][:, T - 1] & capi.TRACK_IN_LIMIT) != 0, b["limit_flags"].any(axis=1))


# ---- 2. parity with the lock-step tracking oracle -------------------------------------------------------------------------------------
PARITY = [
    # (robot, nc, B, samples shared, A per instance, (gain, dt), feed-forward, variant)
    ("talos32", 1, 193, False, False, (1.0, 1.0), "difference", "plain"),
    ("talos32", 2, 193, True, False, (1.0, 1.0), "none", "plain"),
    ("talos32", 2, 193, False, True, (0.5, 0.25), "difference", "plain"),
    ("panda7", 1, 64, False, True, (0.5, 0.25), "none", "plain"),
    ("panda7", 2, 1, False, False, (1.0, 1.0), "difference", "plain"),
    ("talos32", 1, 1, False, False, (0.5, 0.25), "difference", "plain"),
    ("talos32", 2, 193, False, True, (0.5, 0.25), "difference", "limits"),
    ("panda7", 1, 64, False, False, (1.0, 1.0), "difference", "limits"),
    ("talos32", 2, 193, False, False, (0.5, 0.25), "difference", "tasks"),
    ("panda7", 1, 64, True, False, (1.0, 1.0), "difference", "tasks"),
    ("talos32", 2, 193, False, True, (1.0, 1.0), "difference", "device"),
    ("panda7", 1, 64, True, False, (1.0, 1.0), "none", "device"),
]


@pytest.mark.parametrize("case", PARITY, ids=lambda c: "%s-nc%d-B%d-%s-%s-g%g-dt%g-%s-%s" % (
    c[0], c[1], c[2], "smsh" if c[3] else "sminst", "Ainst" if c[4] else "Ash", c[5][0], c[5][1], c[6], c[7]))
def test_track_matches_lockstep_track_oracle(case):
    name, nc, B, shared, a_inst, (gain, dt), ff, variant = case
    model = loik_amd.builtin_model(name)
    links = _links(model, nc)
    T = 5
    rng = np.random.default_rng(4100 + B + 10 * nc)
    tasks, limits = variant == "tasks", variant == "limits"
    frames = PT.random_frames(rng, nc) if tasks else None
    A = np.tile(np.eye(6), (nc, 1, 1)) if tasks else _nonsym_A(rng, nc, B if a_inst else None)
    q0, smp, q_path = _track_workload(model, links, B, T, seed=4101 + B + nc, shared=shared, frames=frames)
    okw = {}
    if limits:
        q_lo, q_hi, q0 = PL.binding_limits(model, q_path[:, T], q0, 4102)
        okw.update(q_lo=q_lo, q_hi=q_hi)
    if tasks:
        okw.update(kinds=[capi.TASK_KINDS[k] for k in _kinds(nc)], frames=frames)
    s = _handle(model, B, links, q0, A, PRM)
    if tasks:
        s.set_pose_tasks(_kinds(nc), frames)
    if limits:
        s.set_joint_limits(q_lo, q_hi)
    kw = dict(dt=dt, gain=gain, tol_track=1e-4, feedforward=ff)
    if variant == "device":
        out = s.TrackPose(capi.DeviceArray(smp), q=capi.DeviceArray(q0), **kw)
        for key, dtype in (("q_traj", np.float64), ("z_traj", np.float64), ("errmax", np.float64), ("inner", np.int32), ("ontrack", np.int32),
                           ("worst", np.float64), ("worst_at", np.int32)):
            dev = capi.DeviceArray(np.zeros(out[key].size))
            s.track_get(key, out=dev)
            assert np.array_equal(_download(dev, out[key].shape, dtype), out[key], equal_nan=True), key
            dev.free()
    else:
        out = s.TrackPose(smp, **kw)
    q = s.get("q")
    timing = s.track_get("timing")
    s.close()
    idx = _subset(B)
    lb, ub = _box(model)
    o = TR.lockstep_track_loop(model, PRM, q0[idx], np.eye(6), np.zeros(6), links, A[idx] if A.ndim == 4 else A, lb, ub, _smp_of(smp, idx), dt,
                               gain, 1e-4, ff=FFS[ff], **okw)
    same = _track_gate(out, o, idx, case)
    assert timing["steps"] == T and np.all(out["steps"] == T) and not out["reached"].any()
    assert np.array_equal(out["q_traj"][:, T], q) and np.array_equal(out["q_traj"][:, 0], q0)
    assert np.max(np.abs(out["err"][idx][same] - o["err"][same])) < 1e-7
    assert np.mean(out["ontrack"][idx][same] != o["ontrack"][same]) <= 0.01   # (an errmax within rounding of tol_track may fall on either side)
    assert np.max(np.abs(out["worst"][idx][same] - o["worst"][same])) < 1e-7
    if limits:
        assert (out["limit_flags"][idx][same] != o["limit_flags"][same]).any(axis=1).mean() <= 0.01, case
        lim = np.isfinite(q_lo) | np.isfinite(q_hi)
        ci = PL.limit_q_index(model)[lim]
        assert np.all(q_lo[lim] <= q[:, ci]) and np.all(q[:, ci] <= q_hi[lim])
        assert (o["inner"] & TR.IN_LIMIT).any()
    if B > 1 and ff == "difference" and not limits:   # the case means something: the seeds are off the path and the loop pulls them in
        assert np.median(o["errmax"][:, T]) < 0.5 * np.median(o["errmax"][:, 0])


def test_f32_handle_step_and_fp64_error():
    """an fp32 handle with a per-instance A (the re-target reads A from the f32 tiles): one feed-forward step against an fp64 handle
    given the same float32-rounded A (F32_STEP_REL of test_pose_parity: both inner solves run the same 40 iterations), errmax and
    err are fp64, and the fp64 handle is anchored to the oracle"""
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 2)
    B, T = 128, 1
    q0, smp, _ = _track_workload(model, links, B, T, seed=4201, spread=(1e-3, 0.05))
    A = _nonsym_A(np.random.default_rng(4202), 2, B).astype(np.float32).astype(np.float64)
    prm = dict(PRM, max_iter=40, tol_abs=0.0, tol_rel=0.0, tol_primal_inf=0.0, tol_dual_inf=0.0)
    res = {}
    for prec in (capi.F32, capi.F64):
        s = _handle(model, B, links, q0, A, prm, precision=prec)
        out = s.TrackPose(smp, dt=0.5, gain=0.7, tol_track=1e-9)
        res[prec] = (out, s.get("q"))
        s.close()
    (o32, q32), (o64, q64) = res[capi.F32], res[capi.F64]
    assert np.array_equal(o32["steps"], o64["steps"]) and np.all(o64["steps"] == 1)
    assert np.max(np.abs(o32["errmax"][:, 0] - np.abs(P.pose_errors(model, q0, links, smp[:, 0])).max(axis=(1, 2)))) <= 1e-10
    assert np.array_equal(o32["q_traj"][:, 0], q0) and np.array_equal(o32["q_traj"][:, 1], q32)
    assert np.max(np.abs(o32["errmax"][:, 1] - np.abs(P.pose_errors(model, q32, links, smp[:, 1])).max(axis=(1, 2)))) <= 1e-10
    rel = np.abs(q32 - q64).max(axis=1) / np.abs(q64 - q0).max(axis=1)
    print("pose_track_measured f32 vs f64 track step: max relative difference %.3e, median %.3e" % (rel.max(), np.median(rel)))
    assert rel.max() < F32_STEP_REL, rel.max()
    idx = _subset(B)
    lb, ub = _box(model)
    o = TR.lockstep_track_loop(model, prm, q0[idx], np.eye(6), np.zeros(6), links, A[idx], lb, ub, smp[idx], 0.5, 0.7, 1e-9)
    assert np.abs(q64[idx] - o["q"]).max() < 1e-7


# ---- 3. the device's own numbers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nc,B", [("talos32", 2, 193), ("panda7", 1, 64)])
def test_trajectories_are_consistent_and_feedforward_tracks_better(name, nc, B):
    model = loik_amd.builtin_model(name)
    _check_trajectories_and_feedforward(model, _links(model, nc), B)


def _check_trajectories_and_feedforward(model, links, B):
    """returns the two runs, {"none": out, "difference": out}"""
    name, nc = model.name, len(links)
    T, dt, tol = 5, 0.5, 1e-4
    q0, smp, _ = _track_workload(model, links, B, T, seed=4301 + B, on_path=True)
    A = np.tile(np.eye(6), (nc, 1, 1))
    res = {}
    for ff in ("none", "difference"):
        s = _handle(model, B, links, q0, A, PRM)
        res[ff] = s.TrackPose(smp, dt=dt, gain=1.0, tol_track=tol, feedforward=ff)
        s.close()
    for ff, out in res.items():
        # z_traj reproduces q_traj
        worst = 0.0
        for b in range(B):
            for k in range(T):
                worst = max(worst, np.max(np.abs(P.integrate(model, out["q_traj"][b, k], dt * out["z_traj"][b, k]) - out["q_traj"][b, k + 1])))
        print("pose_track_measured %s %s: max |integrate(q_k, dt z_k) - q_{k+1}| = %.3e" % (name, ff, worst))
        assert worst <= 1e-12, (ff, worst)
        # worst, worst_at and ontrack follow from errmax
        w, at = TR.worst_of(out["errmax"])
        assert np.array_equal(out["worst"], w) and np.array_equal(out["worst_at"], at)
        assert np.array_equal(out["ontrack"], (out["errmax"] <= tol).sum(axis=1)) and np.all(out["ontrack"] >= 1)
        assert np.all(out["errmax"][:, 0] < 1e-12)
    print("pose_track_measured %s: worst none %.3e .. %.3e, difference %.3e .. %.3e" % (
        name, res["none"]["worst"].min(), res["none"]["worst"].max(), res["difference"]["worst"].min(), res["difference"]["worst"].max()))
    assert np.all(res["difference"]["worst"] < res["none"]["worst"])
    assert np.all(res["difference"]["ontrack"] >= res["none"]["ontrack"])
    return res


# ---- 4. stops and errors --------------------------------------------------------------------------------------------------------------
def test_nan_seed_stops_alone():
    model = loik_amd.builtin_model("panda7")
    _check_nan_seed_stops_alone(model, _links(model, 2), 64, 37, 2)


def _check_nan_seed_stops_alone(model, links, B, bad, coord):
    """the seed of instance `bad` with a NaN in coordinate `coord`"""
    T = 4
    q0, smp, _ = _track_workload(model, links, B, T, seed=4401)
    A = np.tile(np.eye(6), (len(links), 1, 1))
    res = []
    for with_nan in (False, True):
        qs = q0.copy()
        if with_nan:
            qs[bad, coord] = np.nan
        s = _handle(model, B, links, qs, A, PRM)
        res.append(s.TrackPose(smp, dt=0.5, gain=0.8))
        s.close()
    ref, out = res
    assert out["status"][bad] == capi.POSE_ST_STOPPED and out["steps"][bad] == 0 and out["ontrack"][bad] == 0
    want0 = q0[bad].copy()
    want0[coord] = np.nan
    assert np.array_equal(out["q_traj"][bad, 0], want0, equal_nan=True) and np.all(np.isnan(out["q_traj"][bad, 1:]))
    assert np.all(np.isnan(out["z_traj"][bad])) and np.all(np.isnan(out["errmax"][bad])) and not out["inner"][bad].any()
    assert np.isnan(out["worst"][bad]) and out["worst_at"][bad] == -1
    keep = np.arange(B) != bad
    for key in ("q_traj", "z_traj", "errmax", "inner", "ontrack", "worst", "worst_at", "steps", "status", "err"):
        assert np.array_equal(out[key][keep], ref[key][keep]), key
    assert np.all(ref["steps"] == T) and not np.isnan(ref["q_traj"]).any() and not np.isnan(ref["z_traj"]).any()


def test_argument_errors_leave_the_handle_unchanged():
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 1)
    B, T = 16, 2
    q0, smp, _ = _track_workload(model, links, B, T, seed=4501)
    A = np.eye(6)[None]
    kw = dict(dt=0.5, gain=0.9, tol_pose=1e-4, max_steps=3)
    s = _handle(model, B, links, q0, A, PRM)
    fresh = s.SolvePose(smp[:, T], **kw)
    fresh["q"], fresh["z"] = s.get("q"), s.get("z")
    s.close()
    flat = np.ascontiguousarray(smp.reshape(B, T + 1, 1, 12))
    bad_rot = flat.copy()
    bad_rot[5, T, 0, 0] += 1e-6          # the LAST sample of an instance: the check covers all T + 1
    nan_smp = flat.copy()
    nan_smp[2, 0, 0, 10] = np.nan
    ok = dict(dt=0.5, gain=0.9, tol_track=1e-4, n_steps=T, feedforward=1, record=3, flags=0)

    def raw(s, w, **change):
        return s.L.loikb_track_pose(s.h, None, w.ctypes.data_as(C.c_void_p), 0, C.byref(capi.TrackParams(**dict(ok, **change))))

    cases = {
        "dt = 0": lambda s: raw(s, flat, dt=0.0), "dt < 0": lambda s: raw(s, flat, dt=-0.5), "dt nan": lambda s: raw(s, flat, dt=np.nan),
        "dt inf": lambda s: raw(s, flat, dt=np.inf),
        "gain = 0": lambda s: raw(s, flat, gain=0.0), "gain < 0": lambda s: raw(s, flat, gain=-1.0), "gain nan": lambda s: raw(s, flat, gain=np.nan),
        "gain inf": lambda s: raw(s, flat, gain=np.inf),
        "tol < 0": lambda s: raw(s, flat, tol_track=-1.0), "tol nan": lambda s: raw(s, flat, tol_track=np.nan),
        "T = 0": lambda s: raw(s, flat, n_steps=0), "T < 0": lambda s: raw(s, flat, n_steps=-1),
        "feedforward 2": lambda s: raw(s, flat, feedforward=2), "feedforward -1": lambda s: raw(s, flat, feedforward=-1),
        "record 4": lambda s: raw(s, flat, record=4), "record -1": lambda s: raw(s, flat, record=-1),
        "flags": lambda s: raw(s, flat, flags=1),
        "rotation": lambda s: raw(s, bad_rot), "nan": lambda s: raw(s, nan_smp),
        "null samples": lambda s: s.L.loikb_track_pose(s.h, None, None, 0, C.byref(capi.TrackParams(**ok))),
        "null params": lambda s: s.L.loikb_track_pose(s.h, None, flat.ctypes.data_as(C.c_void_p), 0, None),
    }
    for what, call in cases.items():
        s = _handle(model, B, links, q0, A, PRM)
        assert call(s) == -20, what
        buf = np.empty(B, dtype=np.int32)
        assert s.L.loikb_track_get(s.h, capi.TRACK_F_ONTRACK, buf.ctypes.data_as(C.c_void_p), 0) == -24, what
        got = s.SolvePose(smp[:, T], **kw)
        for key in ("steps", "status", "err"):
            assert np.array_equal(got[key], fresh[key]), (what, key)
        assert np.array_equal(s.get("q"), fresh["q"]) and np.array_equal(s.get("z"), fresh["z"]), what
        s.close()
    # the binding's own checks, and a handle before SolveInit
    s = _handle(model, B, links, q0, A, PRM)
    with pytest.raises(ValueError):
        s.TrackPose(smp[:, :, 0])          # [B][T+1][12]: no constraint axis
    with pytest.raises(ValueError):
        s.TrackPose(smp, feedforward="spline")
    with pytest.raises(loik_amd.LoikError) as e:
        s.TrackPose(bad_rot)
    assert e.value.code == -20 and "sample" in str(e.value)
    s.close()
    s = loik_amd.BatchedLoik(model, B, **dict(PRM))
    with pytest.raises(loik_amd.LoikError) as e:
        s.TrackPose(flat)
    assert e.value.code == -24
    s.close()


def test_track_get_before_the_first_call_and_unrecorded_fields():
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 1)
    B, T = 4, 2
    q0, smp, _ = _track_workload(model, links, B, T, seed=4601)
    s = _handle(model, B, links, q0, np.eye(6)[None], PRM)
    buf = np.empty(B, dtype=np.int32)
    assert s.L.loikb_track_get(s.h, capi.TRACK_F_ONTRACK, buf.ctypes.data_as(C.c_void_p), 0) == -24
    s.SolvePose(smp[:, 0], max_steps=1)
    assert s.L.loikb_track_get(s.h, capi.TRACK_F_ONTRACK, buf.ctypes.data_as(C.c_void_p), 0) == -24
    s.close()
    qbuf, zbuf = np.empty((B, T + 1, model.nq)), np.empty((B, T, model.nv))
    full = None
    for record, q_rc, z_rc in ((("q", "z"), 0, 0), ((), -24, -24), ("q", 0, -24), ("z", -24, 0)):   # (a fresh handle each: warm starts)
        s = _handle(model, B, links, q0, np.eye(6)[None], PRM)
        out = s.TrackPose(smp, record=record)
        full = full or out
        assert (out["q_traj"] is None) == (q_rc != 0) and (out["z_traj"] is None) == (z_rc != 0)
        assert s.L.loikb_track_get(s.h, capi.TRACK_F_Q, qbuf.ctypes.data_as(C.c_void_p), 0) == q_rc, record
        assert s.L.loikb_track_get(s.h, capi.TRACK_F_Z, zbuf.ctypes.data_as(C.c_void_p), 0) == z_rc, record
        assert q_rc or np.array_equal(qbuf, full["q_traj"])
        assert z_rc or np.array_equal(zbuf, full["z_traj"])
        for key in ("errmax", "inner", "ontrack", "worst", "worst_at"):   # what is recorded changes nothing of what is computed
            assert np.array_equal(out[key], full[key]), (record, key)
        assert s.L.loikb_track_get(s.h, 99, qbuf.ctypes.data_as(C.c_void_p), 0) == -20
        s.close()
