"""GPU: the pose loop (loik_pose.hpp, loikb_solve_pose) against the lock-step CPU oracle (pose_numpy.lockstep_pose_loop) outside the
setting of tests/test_pose_ik.py: a non-symmetric A (shared and per instance), gain and dt other than 1, multi-DoF robots, every inner
engine, f32 handles, the status bits, a NaN seed, what the data object holds afterwards and a formulation edited before the pose
solve.  The gate is test_pose_ik's: the same reached / steps on >= 99 % of the instances, |dq| < 1e-7 on those."""
import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from test_engines import ENGINES
from test_pose_ik import BOUND, PRM, _fk_models, _links
import pose_numpy as P

pytestmark = pytest.mark.gpu

ORACLE_MAX = 256   # instances the oracle runs per case (a strided subset of a larger batch)
ENGINE_ENV = ("LOIKB_LEAN", "LOIKB_FLAT", "LOIKB_FLAT_SPLIT", "LOIKB_FLAT_SLICE", "LOIKB_LEAN_WG_PER_CU", "LOIKB_LEAN_KLO",
              "LOIKB_LEAN_DECADES", "LOIKB_LEAN_ADAPT", "LOIKB_FLAT_BUILD", "LOIKB_CHUNKS")


def _nonsym_A(rng, nc, B=None):
    """I + N / (2 |N|_2): condition number <= 3 and far from symmetric (a transposed A asks for another step); [nc][6][6] or
    [B][nc][6][6]"""
    N = rng.normal(size=(nc, 6, 6) if B is None else (B, nc, 6, 6))
    A = np.eye(6) + 0.5 * N / np.linalg.norm(N, ord=2, axis=(-2, -1))[..., None, None]
    assert np.all(np.abs(A - np.swapaxes(A, -1, -2)).max(axis=(-2, -1)) > 0.05)
    return A


def _box(model, bound=BOUND):
    return -bound * np.ones(model.nv), bound * np.ones(model.nv)


def _handle(model, B, links, q0, A, prm, precision=capi.F64, box=None, **kw):
    """SolveInit with b = 0 and A shared ([nc][6][6]) or per instance ([B][nc][6][6])"""
    nc = len(links)
    s = loik_amd.BatchedLoik(model, B, precision=precision, **dict(prm, num_eq_c=nc), **kw)
    lb, ub = box if box is not None else _box(model)
    s.SolveInit(q0, np.eye(6), np.zeros(6), np.array(links, dtype=np.int32), A, np.zeros((B, nc, 6)), lb, ub)
    return s


def _seeds(model, B, links, seed, spread=(1e-4, 0.15)):
    """targets = FK of random configurations; seeds = those moved on the configuration manifold by a random velocity of a size
    log-uniform in `spread` (so that instances reach at different steps)"""
    rng = np.random.default_rng(seed)
    q_t = model.random_configurations(rng, B)
    size = np.exp(rng.uniform(np.log(spread[0]), np.log(spread[1]), size=B))
    q0 = np.stack([P.integrate(model, q_t[b], size[b] * rng.normal(size=model.nv) / np.sqrt(model.nv)) for b in range(B)])
    return q0, P.fk12(model, q_t, links)


def _subset(B):
    return np.arange(0, B, max(1, -(-B // ORACLE_MAX)))


def _oracle(model, prm, q0, links, A, tg, dt, gain, tol, k, idx, box=None):
    """lockstep_pose_loop on the instances idx (A and targets per instance or shared as given)"""
    lb, ub = box if box is not None else _box(model)
    A_i = A[idx] if A.ndim == 4 else A
    tg_i = tg[idx] if tg.ndim == 3 else np.broadcast_to(tg, (len(idx),) + tg.shape)
    return P.lockstep_pose_loop(model, prm, q0[idx], np.eye(6), np.zeros(6), links, A_i, lb, ub, tg_i, dt, gain, tol, k)


def _gate(out, q, o, idx, what):
    same = (out["reached"][idx] == o["reached"]) & (out["steps"][idx] == o["steps"])
    assert same.mean() >= 0.99, (what, same.mean())
    dq = np.abs(q[idx] - o["q"]).max(axis=1)
    assert np.all(dq[same] < 1e-7), (what, dq[same].max())
    return same


def _run_case(model, links, B, A, tg, q0, dt, gain, tol, k, prm=PRM, what="", **kw):
    s = _handle(model, B, links, q0, A, prm, **kw)
    out = s.SolvePose(tg, dt=dt, gain=gain, tol_pose=tol, max_steps=k)
    q = s.get("q")
    s.close()
    idx = _subset(B)
    o = _oracle(model, prm, q0, links, A, tg, dt, gain, tol, k, idx)
    same = _gate(out, q, o, idx, what)
    return out, q, o, idx, same


# ---- 1. the control law: non-symmetric A, gain and dt, nc, ragged and single batches, shared targets ------------------------------
LAW_CASES = [
    # (robot, nc, A per instance, (gain, dt), B, shared target)
    ("talos32", 1, False, (0.5, 0.25), 193, False),
    ("talos32", 2, True, (0.5, 0.25), 193, False),
    ("talos32", 2, False, (1.7, 2.0), 193, True),
    ("talos32", 2, True, (1.7, 2.0), 256, True),
    ("talos32", 2, False, (0.5, 0.25), 1, False),
    ("talos32", 1, False, (1.7, 2.0), 1, True),
    ("panda7", 1, True, (1.7, 2.0), 193, False),
    ("panda7", 2, True, (0.5, 0.25), 64, True),
]


@pytest.mark.parametrize("case", LAW_CASES, ids=lambda c: "%s-nc%d-%s-g%g-dt%g-B%d-%s" % (
    c[0], c[1], "Ainst" if c[2] else "Ash", c[3][0], c[3][1], c[4], "tgsh" if c[5] else "tginst"))
def test_control_law_matches_lockstep_oracle(case):
    name, nc, per_inst, (gain, dt), B, shared_tg = case
    model = loik_amd.builtin_model(name)
    links = _links(model, nc)
    rng = np.random.default_rng(B + 10 * nc + int(per_inst))
    A = _nonsym_A(rng, nc, B if per_inst else None)
    q0, tg = _seeds(model, B, links, seed=B + nc, spread=(1e-5, 0.1) if shared_tg else (1e-4, 0.15))
    if shared_tg:
        tg = tg[0]
        # (the seeds around the first target: the others would start far from it)
        q0 = np.stack([P.integrate(model, q0[0], 0.02 * rng.normal(size=model.nv) * 10.0 ** rng.uniform(-3, 0)) for _ in range(B)])
    for k in (1, 3):
        out, q, o, idx, same = _run_case(model, links, B, A, tg, q0, dt, gain, 1e-4, k, what=(case, k))
        assert np.all(out["steps"] <= k)
        if k == 3 and B > 1:
            assert np.any(out["steps"] > 0)


# ---- 2. multi-DoF robots: constraints on a leaf and on a multi-DoF joint --------------------------------------------------------
MULTI_DOF = {9, 10, 11, 12, 13, 17}   # free-flyer, spherical, translation, ZYX, planar, composite


def _leaf_and_multidof(model):
    children = np.zeros(model.njoints, dtype=int)
    for i in range(1, model.njoints):
        children[int(model.parents[i])] += 1
    jt = [int(t) for t in model.jtype]
    multi = [i for i in range(1, model.njoints) if jt[i] in MULTI_DOF] or [i for i in range(1, model.njoints) if jt[i] >= 19]
    leaves = [i for i in range(1, model.njoints) if children[i] == 0 and i not in multi]
    assert multi and leaves, model.name
    return [leaves[-1], multi[-1]]


@pytest.mark.parametrize("k", range(2, 6))
def test_multidof_robots_match_lockstep_oracle(k):
    model = _fk_models()[k]
    links = _leaf_and_multidof(model)
    B = 128
    rng = np.random.default_rng(300 + k)
    A = _nonsym_A(rng, 2, B)
    q0, tg = _seeds(model, B, links, seed=310 + k, spread=(1e-4, 0.1))
    for steps in (1, 3):
        out, q, o, idx, same = _run_case(model, links, B, A, tg, q0, 0.5, 0.8, 1e-4, steps, what=(model.name, steps))
        if steps == 3:
            assert np.any(out["steps"] > 0) and np.max(np.abs(q - q0)) > 1e-3


# ---- 3. every inner engine sees the device-side b edits between its solves -------------------------------------------------------
_ENGINE_ORACLE = {}
ENGINE_RUNS = list(ENGINES) + ["chunks3"]


def _engine_problem():
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 2)
    B = 384   # (six tiles of 64: LOIKB_CHUNKS=3 gets three chunks of two)
    rng = np.random.default_rng(77)
    A = {"Ash": _nonsym_A(rng, 2), "Ainst": _nonsym_A(rng, 2, B)}
    q0, tg = _seeds(model, B, links, seed=78)
    return model, links, B, A, q0, tg


@pytest.mark.parametrize("akind", ["Ash", "Ainst"])
@pytest.mark.parametrize("engine", ENGINE_RUNS)
def test_every_engine_matches_lockstep_oracle(engine, akind, monkeypatch):
    model, links, B, A, q0, tg = _engine_problem()
    A = A[akind]
    gain, dt, tol, k = 1.0, 0.5, 1e-4, 3
    for v in ENGINE_ENV:
        monkeypatch.delenv(v, raising=False)
    if engine == "chunks3":   # (the keywords of test_gpu_parity.test_concurrent_chunks_change_nothing)
        env, kw = dict(LOIKB_CHUNKS="3"), dict(compact_min_instances=128, max_launch_iters=5, tail_max_instances=900)
    else:
        env, kw = ENGINES[engine]
    for v, x in env.items():
        monkeypatch.setenv(v, x)
    s = _handle(model, B, links, q0, A, PRM, **kw)
    out = s.SolvePose(tg, dt=dt, gain=gain, tol_pose=tol, max_steps=k)
    q = s.get("q")
    if engine == "chunks3":
        assert s.stats()["chunks"] == 3
    s.close()
    idx = _subset(B)
    if akind not in _ENGINE_ORACLE:
        _ENGINE_ORACLE[akind] = _oracle(model, PRM, q0, links, A, tg, dt, gain, tol, k, idx)
    o = _ENGINE_ORACLE[akind]
    _gate(out, q, o, idx, (engine, akind))
    assert np.any(out["steps"] > 1)


# ---- 4. f32 handles: the pose kernels are fp64 whatever the handle's precision ---------------------------------------------------
def test_f32_handle_err_is_fp64():
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 2)
    B = 96
    q0, tg = _seeds(model, B, links, seed=401)
    A = _nonsym_A(np.random.default_rng(402), 2, B)
    s = _handle(model, B, links, q0, A, PRM, precision=capi.F32)
    out = s.SolvePose(tg, max_steps=0)
    s.close()
    want = P.pose_errors(model, q0, links, tg)
    assert np.max(np.abs(out["err"] - want)) <= 1e-10, np.max(np.abs(out["err"] - want))
    assert not out["steps"].any()


# f32 step against fp64 step, relative to the step: both inner solves run the same 40 ADMM iterations (no stopping test), so they
# differ by the f32 solve's rounding alone -- f32's unit roundoff (6e-8) carried through 40 iterations of sweeps over 32 joints and
# amplified by H's conditioning (rho = 1e-5).  Measured on an MI355X: 4.1e-4 at most, 1.8e-5 median over the 128 instances; the
# bound leaves 5x.  An A read from the wrong slot or transposed changes the step by O(1) of itself.
F32_STEP_REL = 2e-3


def test_f32_handle_per_instance_A_step():
    """one step with a per-instance A on an f32 handle (the retarget reads A from the f32 tiles) against an fp64 handle given the
    same, float32-rounded, A (F32_STEP_REL above), and the fp64 handle against the oracle"""
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 2)
    B = 128
    q0, tg = _seeds(model, B, links, seed=411, spread=(1e-3, 0.1))
    A = _nonsym_A(np.random.default_rng(412), 2, B).astype(np.float32).astype(np.float64)
    prm = dict(PRM, max_iter=40, tol_abs=0.0, tol_rel=0.0, tol_primal_inf=0.0, tol_dual_inf=0.0)
    res = {}
    for prec in (capi.F32, capi.F64):
        s = _handle(model, B, links, q0, A, prm, precision=prec)
        out = s.SolvePose(tg, dt=0.5, gain=0.7, tol_pose=1e-9, max_steps=1)
        res[prec] = (out, s.get("q"))
        s.close()
    (o32, q32), (o64, q64) = res[capi.F32], res[capi.F64]
    assert np.array_equal(o32["steps"], o64["steps"]) and o64["steps"].all()
    dq64 = np.abs(q64 - q0).max(axis=1)
    rel = np.abs(q32 - q64).max(axis=1) / dq64
    print("f32 vs f64 step: max relative difference %.3e, median %.3e" % (rel.max(), np.median(rel)))
    assert rel.max() < F32_STEP_REL, rel.max()
    # and the fp64 handle against the oracle, so that the pair is anchored
    idx = _subset(B)
    o = _oracle(model, prm, q0, links, A, tg, 0.5, 0.7, 1e-9, 1, idx)
    assert np.abs(q64[idx] - o["q"]).max() < 1e-7


# ---- 5. status bits and stopping ------------------------------------------------------------------------------------------------
NOT_CONV_MAX_ITER = 30   # (the oracle's inner solves stop short on about a fifth of the instances)


def test_not_converged_bit_matches_oracle():
    """inner solves cut short by max_iter: POSE_NOT_CONVERGED on the instances whose oracle solve did not converge"""
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 2)
    B = 160
    q0, tg = _seeds(model, B, links, seed=501)
    A = _nonsym_A(np.random.default_rng(502), 2)
    prm = dict(PRM, max_iter=NOT_CONV_MAX_ITER)
    out, q, o, idx, same = _run_case(model, links, B, A, tg, q0, 0.5, 1.0, 1e-4, 2, prm=prm, what="not converged")
    nc_dev = (out["status"][idx] & P.POSE_NOT_CONVERGED) != 0
    nc_ora = (o["status"] & P.POSE_NOT_CONVERGED) != 0
    assert 0.1 < nc_ora.mean() < 0.9, nc_ora.mean()
    assert np.mean(nc_dev != nc_ora) <= 0.01, (np.flatnonzero(nc_dev != nc_ora), nc_ora.mean())
    assert np.array_equal(nc_dev[same], nc_ora[same])


INF_TOL = 1e-2   # tol_primal_inf: the oracle certifies about a sixth of the instances infeasible in the 0.05 box


def test_infeasible_bit_matches_oracle():
    """targets outside a tight velocity box: the oracle certifies primal infeasibility (tol_primal_inf) on some instances"""
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 1)
    B = 128
    q0, tg = _seeds(model, B, links, seed=511, spread=(1e-3, 0.6))
    A = np.eye(6)[None]
    box = _box(model, 0.05)
    prm = dict(PRM, tol_primal_inf=INF_TOL)
    s = _handle(model, B, links, q0, A, prm, box=box)
    out = s.SolvePose(tg, dt=1.0, gain=1.0, tol_pose=1e-4, max_steps=2)
    q = s.get("q")
    s.close()
    idx = _subset(B)
    o = _oracle(model, prm, q0, links, A, tg, 1.0, 1.0, 1e-4, 2, idx, box=box)
    same = _gate(out, q, o, idx, "infeasible")
    inf_dev = (out["status"][idx] & P.POSE_INFEASIBLE) != 0
    inf_ora = (o["status"] & P.POSE_INFEASIBLE) != 0
    assert 0.1 < inf_ora.mean() < 0.95, inf_ora.mean()
    assert np.array_equal(inf_dev[same], inf_ora[same]) and np.mean(inf_dev != inf_ora) <= 0.01


@pytest.mark.parametrize("engine", ["flat", "lean", "tail", "solve"])
def test_nan_seed_stops_alone(engine, monkeypatch):
    """one seed with a NaN coordinate: that instance is stopped at once (0 steps, q untouched), every other instance does what it does
    without it"""
    for v in ENGINE_ENV:
        monkeypatch.delenv(v, raising=False)
    env, kw = ENGINES[engine]
    for v, x in env.items():
        monkeypatch.setenv(v, x)
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 2)
    B, bad = 130, 67
    q0, tg = _seeds(model, B, links, seed=521)
    A = _nonsym_A(np.random.default_rng(522), 2)
    res = []
    for with_nan in (False, True):
        qs = q0.copy()
        if with_nan:
            qs[bad, 3] = np.nan
        s = _handle(model, B, links, qs, A, PRM, **kw)
        out = s.SolvePose(tg, dt=0.5, gain=1.0, tol_pose=1e-4, max_steps=3)
        res.append((out, s.get("q")))
        s.close()
    (o0, q_ref), (o1, q1) = res
    assert o1["status"][bad] == P.POSE_STOPPED and o1["steps"][bad] == 0
    other = np.arange(model.nq) != 3
    assert np.isnan(q1[bad, 3]) and np.array_equal(q1[bad, other], q0[bad, other])
    keep = np.arange(B) != bad
    assert np.array_equal(o1["steps"][keep], o0["steps"][keep]) and np.array_equal(o1["status"][keep], o0["status"][keep])
    assert np.all(np.isfinite(q1[keep])) and np.max(np.abs(q1[keep] - q_ref[keep])) <= 1e-12
    assert np.all(np.isfinite(o1["err"][keep])) and np.max(np.abs(o1["err"][keep] - o0["err"][keep])) <= 1e-12
    assert o0["steps"].max() >= 2


# ---- 6. what the data object holds afterwards ----------------------------------------------------------
@pytest.mark.parametrize("ending", ["mixed", "all_at_once", "max_steps"])
def test_data_object_after_pose_solve(ending):
    """z and iter of the handle after the loop are the lock-step oracle's: the idle b = 0 solves at the final q for the instances that
    reached before the last solve, the last step's solve for those still running then or reaching at the final re-target"""
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 1)
    B = 96
    rng = np.random.default_rng(601)
    A = _nonsym_A(rng, 1)
    q0, tg = _seeds(model, B, links, seed=602, spread=(1e-5, 0.02))
    k = 20 if ending != "max_steps" else 2
    if ending == "all_at_once":   # a third already there, the others from one seed: they all reach together and end the loop
        far = int(np.argmax(np.abs(P.pose_errors(model, q0, links, tg)).max(axis=(1, 2))))
        q0[B // 3:], tg[B // 3:] = q0[far], tg[far]
        tg[:B // 3] = P.fk12(model, q0[:B // 3], links)
    prm = dict(PRM, max_iter=500, tol_abs=1e-9)
    s = _handle(model, B, links, q0, A, prm)
    out = s.SolvePose(tg, dt=1.0, gain=1.0, tol_pose=1e-6, max_steps=k)
    q, z, it = s.get("q"), s.get("z"), s.get("iter")
    s.close()
    idx = np.arange(B)   # (the number of solves is the batch's: the oracle runs the whole batch)
    o = _oracle(model, prm, q0, links, A, tg, 1.0, 1.0, 1e-6, k, idx)
    same = _gate(out, q, o, idx, ending)
    if ending == "max_steps":
        assert not o["reached"].all() and o["steps"].max() == k
    if ending == "all_at_once":   # (the loop ends because none is running any more, before max_steps)
        assert o["reached"].all() and o["steps"].max() < k and len(np.unique(o["steps"])) == 2
    last = o["steps"].max()
    assert np.any(o["steps"] < last) and np.any(o["steps"] == last)
    same_it = same & (it == o["iter"])
    assert same_it.mean() >= 0.97, (ending, same_it.mean())
    assert np.max(np.abs(z[same_it] - o["z"][same_it])) < 1e-7, np.max(np.abs(z[same_it] - o["z"][same_it]))
    # the instances that reached at the final re-target keep the z that moved them there: not small
    at_last = same_it & o["reached"] & (o["steps"] == last)
    if ending == "all_at_once":
        assert at_last.any() and np.all(np.abs(z[at_last]).max(axis=1) > 1e-7)


# ---- 7. the formulation edited before the pose solve ----------------------------------------------------------------------------
@pytest.mark.parametrize("per_inst", [False, True], ids=["Ash", "Ainst"])
def test_remove_constraint_then_pose_equals_direct_init(per_inst):
    model = loik_amd.builtin_model("talos32")
    l0, l2 = _links(model, 2)
    lm = model.getJointId("arm_left_4_joint")
    B = 96
    rng = np.random.default_rng(701 + per_inst)
    A3 = _nonsym_A(rng, 3, B if per_inst else None)
    A2 = A3[..., [0, 2], :, :]
    q0, tg = _seeds(model, B, [l0, l2], seed=702)
    lb, ub = _box(model)
    a = loik_amd.BatchedLoik(model, B, **dict(PRM, num_eq_c=3))
    a.SolveInit(q0, np.eye(6), np.zeros(6), np.array([l0, lm, l2], dtype=np.int32), A3, np.zeros((B, 3, 6)), lb, ub)
    assert a.RemoveEqConstraint(lm) and a.active_task_constraint_ids() == [l0, l2]
    b = _handle(model, B, [l0, l2], q0, A2, PRM)
    outs = []
    for s in (a, b):
        o = s.SolvePose(tg, dt=0.5, gain=0.9, tol_pose=1e-4, max_steps=3)
        o["q"] = s.get("q")
        outs.append(o)
        s.close()
    oa, ob = outs
    assert np.array_equal(oa["steps"], ob["steps"]) and np.array_equal(oa["status"], ob["status"])
    assert np.max(np.abs(oa["q"] - ob["q"])) <= 1e-12 and np.max(np.abs(oa["err"] - ob["err"])) <= 1e-12
    idx = _subset(B)
    o = _oracle(model, PRM, q0, [l0, l2], A2, tg, 0.5, 0.9, 1e-4, 3, idx)
    _gate(ob, ob["q"], o, idx, "direct")
