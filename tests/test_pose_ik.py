"""GPU: batched pose IK (include/loik_amd_pose.h) -- world placements, the device log6, the pose loop step by step against the
CPU oracle driven from the host, end to end from many seeds, and the call forms."""
import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from helpers import FIXTURE, composite_tree, fixture_problem, helical_tree, random_tree_multidof
from test_multidof import _np_integrate
import pose_numpy as P

pytestmark = pytest.mark.gpu

PRM = dict(FIXTURE, max_iter=300, tol_abs=1e-6, tol_rel=0.0, warm_start=True)
BOUND = 2.0


def _links(model, n):
    if model.name == "panda7":
        return [7, 4][:n]
    return [model.getJointId("arm_left_7_joint"), model.getJointId("arm_right_7_joint")][:n]


def _handle(model, B, links, q0, precision=capi.F64, **kw):
    prm = dict(PRM, num_eq_c=len(links), **kw)
    s = loik_amd.BatchedLoik(model, B, precision=precision, **prm)
    nc = len(links)
    s.SolveInit(q0, np.eye(6), np.zeros(6), np.array(links, dtype=np.int32), np.tile(np.eye(6), (nc, 1, 1)), np.zeros((B, nc, 6)),
                -BOUND * np.ones(model.nv), BOUND * np.ones(model.nv))
    return s, prm


def _seeds(model, B, links, seed, spread=0.1):
    """targets = FK of random configurations within the limits; seeds = those configurations perturbed"""
    rng = np.random.default_rng(seed)
    q_t = model.random_configurations(rng, B)
    q0 = np.clip(q_t + spread * rng.normal(size=q_t.shape), model.q_lo, model.q_hi)
    return q0, P.fk12(model, q_t, links)


# ---- 1. world placements ---------------------------------------------------------------------------------------------------
def _fk_models():
    return [loik_amd.builtin_model("talos32"), loik_amd.builtin_model("panda7"),
            random_tree_multidof(seed=5, nb=9, root_freeflyer=True, n_spherical=1, n_translation=1),
            random_tree_multidof(seed=23, nb=13, root_freeflyer=True, n_spherical=0, n_translation=1, n_zyx=2, n_planar=1, n_rub=3),
            composite_tree(seed=31, nb=8, which=[2, 5]),
            helical_tree(seed=41, nb=9, n_helical=4)]


@pytest.mark.parametrize("k", range(6))
def test_forward_kinematics_matches_numpy(k):
    model = _fk_models()[k]
    B = 96
    rng = np.random.default_rng(100 + k)
    q = model.random_configurations(rng, B)
    p = fixture_problem(model, bound=BOUND)
    s = loik_amd.BatchedLoik(model, B, **dict(FIXTURE, max_iter=200))
    s.SolveInit(q, p["H_ref"], p["v_ref"], p["c_ids"], p["Ais"], np.tile(p["bis"], (B, 1, 1)), p["lb"], p["ub"])
    links = list(range(model.njoints))
    want = P.fk12(model, q, links)
    got = s.forward_kinematics(links)
    assert np.max(np.abs(got[..., :3, :3].reshape(B, -1, 9) - want[..., :9])) < 1e-12, model.name
    assert np.max(np.abs(got[..., :3, 3] - want[..., 9:])) < 1e-12, model.name
    # after integrate: the resident q, not the liMi of the last FwdPassInit
    s.Solve()
    s.integrate(0.7)
    q1 = s.get("q")
    assert np.max(np.abs(q1 - q)) > 1e-6
    got1 = s.forward_kinematics(links)
    want1 = P.fk12(model, q1, links)
    assert np.max(np.abs(got1[..., :3, :3].reshape(B, -1, 9) - want1[..., :9])) < 1e-12, model.name
    assert np.max(np.abs(got1[..., :3, 3] - want1[..., 9:])) < 1e-12, model.name
    s.close()


# ---- 2. the device log6 -------------------------------------------------------------------------------------------------------
# the branch switches of pose_log3 (series below theta = 1e-4, symmetric-part axis below cos theta = -0.8) and pose_log6 (series of
# beta below theta = 1e-3), both sides of each; pi approached and met (the numpy log6 is pinned to mpmath at these: test_pose_abi)
EDGE_THETAS = [1e-9, 1e-4 * (1 - 1e-3), 1e-4 * (1 + 1e-3), 1e-3 * (1 - 1e-3), 1e-3 * (1 + 1e-3), np.arccos(-0.8) - 1e-6,
               np.arccos(-0.8) + 1e-6, np.pi - 1e-3, np.pi - 1e-6, np.pi - 1e-9, np.pi - 1e-12]
EDGE_AXES = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, -3)]
EDGE_TRANSLATIONS = [1e-9, 1e3]
# |dw| <= EDGE_REL theta + EDGE_ABS, |d nu| <= EDGE_REL |nu| + EDGE_ABS.  The floor covers what the device's and numpy's FK leave in
# oMi^-1 oMdes; measured on an MI355X: |dw| <= 2.4e-16 below theta = 2e-3, |dw| / theta <= 4.5e-16 above.  A wrong theta^2 / 6 term
# in the theta -> 0 series changes w by theta^3 / 6 = 1.7e-13 at theta = 1e-4, which an absolute bound of 1e-10 does not see.
EDGE_REL, EDGE_ABS = 1e-12, 2e-15


@pytest.mark.parametrize("case", ["random", "near_identity", "near_pi", "edges", "pi_exactly"])
def test_err_matches_numpy_log6(case):
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 1)
    B = 256
    rng = np.random.default_rng(7)
    q = model.random_configurations(rng, B)
    R, t = P.fk(model, q, links[0])
    tg = np.empty((B, 1, 12))
    theta = np.empty(B)
    for b in range(B):
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        if case == "random":
            nu = np.r_[rng.normal(size=3), rng.uniform(0, np.pi) * a]
        elif case == "near_identity":
            nu = np.r_[1e-3 * rng.normal(size=3), rng.uniform(0, 1e-7) * a]
        elif case == "near_pi":
            nu = np.r_[rng.normal(size=3), (np.pi - rng.uniform(0, 1e-6)) * a]
        else:
            th = np.pi if case == "pi_exactly" else EDGE_THETAS[b % len(EDGE_THETAS)]
            if b % 3 == 0:
                a = np.asarray(EDGE_AXES[(b // 3) % len(EDGE_AXES)], dtype=float)
                a /= np.linalg.norm(a)
            v = rng.normal(size=3)
            nu = np.r_[EDGE_TRANSLATIONS[(b // 2) % 2] * v / np.linalg.norm(v), th * a]
        theta[b] = np.linalg.norm(nu[3:])
        Rd, pd = P.exp6(nu)
        if case == "pi_exactly":
            Rd = 2.0 * np.outer(a, a) - np.eye(3)
        tg[b, 0] = np.r_[(R[b] @ Rd).ravel(), t[b] + R[b] @ pd]
    s, _ = _handle(model, B, links, q)
    out = s.SolvePose(tg, max_steps=0)
    s.close()
    assert not out["steps"].any()
    want = P.pose_errors(model, q, links, tg)
    got = out["err"]
    if case == "pi_exactly":   # (the sign of the axis is free at pi: compare the placements exp6 gives back)
        for b in range(B):
            (Rg, pg), (Rw, pw) = P.exp6(got[b, 0]), P.exp6(want[b, 0])
            assert np.max(np.abs(Rg - Rw)) < 1e-10 and np.max(np.abs(pg - pw)) < 1e-10, b
            assert abs(np.linalg.norm(got[b, 0, 3:]) - np.pi) < 1e-7
        return
    assert np.max(np.abs(got - want)) < 1e-10, np.max(np.abs(got - want))
    if case == "edges":
        dw = np.abs(got[:, 0, 3:] - want[:, 0, 3:]).max(axis=1)
        dnu = np.abs(got[:, 0] - want[:, 0]).max(axis=1)
        nrm = np.linalg.norm(want[:, 0], axis=1)
        small = theta < 2e-3
        print("log6 edges: max |dw| = %.3e below theta = 2e-3, max |dw| / theta = %.3e above; max |dnu| / |nu| = %.3e"
              % (dw[small].max(), (dw / theta)[~small].max(), (dnu / nrm).max()))
        assert np.all(dw <= EDGE_REL * theta + EDGE_ABS), (theta[np.argmax(dw - EDGE_REL * theta)], dw.max())
        assert np.all(dnu <= EDGE_REL * nrm + EDGE_ABS), (dnu / nrm).max()


# ---- 3. step by step against the CPU oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nc", [("panda7", 1), ("panda7", 2), ("talos32", 1), ("talos32", 2)])
def test_pose_steps_match_oracle_host_loop(name, nc):
    model = loik_amd.builtin_model(name)
    links = _links(model, nc)
    B = 256
    q0, tg = _seeds(model, B, links, seed=11 + nc)
    tol = 1e-4
    for k in (1, 3):
        s, prm = _handle(model, B, links, q0)
        out = s.SolvePose(tg, dt=1.0, gain=1.0, tol_pose=tol, max_steps=k)
        q = s.get("q")
        s.close()
        q_o, steps_o, reached_o = P.host_pose_loop(model, prm, q0, np.eye(6), np.zeros(6), links, np.tile(np.eye(6), (nc, 1, 1)),
                                                   -BOUND * np.ones(model.nv), BOUND * np.ones(model.nv), tg, 1.0, 1.0, tol, k,
                                                   _np_integrate)
        same = (out["reached"] == reached_o) & (out["steps"] == steps_o)
        assert same.mean() >= 0.99, (name, nc, k, same.mean())
        dq = np.abs(q - q_o).max(axis=1)
        assert np.all(dq[same] < 1e-7), (name, nc, k, dq[same].max())
        assert out["reached"].any() or k == 1


# ---- 4. end to end from many seeds -------------------------------------------------------------------------------------------
def test_pose_end_to_end_many_seeds():
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 1)
    B, tol = 4096, 1e-6
    q0, tg = _seeds(model, B, links, seed=5, spread=0.15)
    s, prm = _handle(model, B, links, q0)
    out = s.SolvePose(tg, dt=1.0, gain=1.0, tol_pose=tol, max_steps=20)
    q = s.get("q")
    s.close()
    r = out["reached"]
    assert r.mean() > 0.5
    e = P.pose_errors(model, q[r], links, tg[r])
    assert np.max(np.abs(e)) <= tol
    _, _, reached_o = P.host_pose_loop(model, prm, q0, np.eye(6), np.zeros(6), links, np.eye(6)[None], -BOUND * np.ones(model.nv),
                                       BOUND * np.ones(model.nv), tg, 1.0, 1.0, tol, 20, _np_integrate)
    assert r.mean() >= reached_o.mean() - 0.01, (r.mean(), reached_o.mean())


# ---- 5. reached instances stay put; max_steps = 0 ----------------------------------------------------------------------------
def test_reached_instances_do_not_move_and_zero_steps():
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 1)
    B = 512
    q0, tg = _seeds(model, B, links, seed=3)
    s, _ = _handle(model, B, links, q0)
    z0 = s.SolvePose(tg, tol_pose=1e-5, max_steps=0)
    assert np.array_equal(s.get("q"), q0) and not z0["steps"].any()
    assert np.max(np.abs(z0["err"] - P.pose_errors(model, q0, links, tg))) < 1e-10
    a = s.SolvePose(tg, tol_pose=1e-5, max_steps=3)
    qa = s.get("q")
    ra = a["reached"]
    assert ra.any()
    b = s.SolvePose(tg, tol_pose=1e-5, max_steps=10)   # from the resident q: the reached ones are reached at once
    qb = s.get("q")
    assert np.array_equal(qb[ra], qa[ra])
    assert not b["steps"][ra].any() and b["reached"][ra].all()
    moved = b["steps"] > 0
    assert np.all(np.any(qb[moved] != qa[moved], axis=1))
    s.close()


# ---- 6. call forms -----------------------------------------------------------------------------------------------------------
def test_call_forms_agree():
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 2)
    B = 128
    q0, tg = _seeds(model, B, links, seed=9)
    shared = tg[0]
    kw = dict(tol_pose=1e-6, max_steps=8)
    outs = []
    for form in ("per_instance_host", "shared_host", "per_instance_4x4", "per_instance_device", "shared_device"):
        s, _ = _handle(model, B, links, np.zeros_like(q0))
        if form == "per_instance_host":
            o = s.SolvePose(np.tile(shared, (B, 1, 1)), q=q0, **kw)
        elif form == "shared_host":
            o = s.SolvePose(shared, q=q0, **kw)
        elif form == "per_instance_4x4":
            M = np.zeros((B, 2, 4, 4))
            M[..., :3, :3] = np.tile(shared, (B, 1, 1))[..., :9].reshape(B, 2, 3, 3)
            M[..., :3, 3] = shared[:, 9:]
            M[..., 3, 3] = 1
            o = s.SolvePose(M, q=q0, **kw)
        else:
            t_dev = capi.DeviceArray(np.tile(shared, (B, 1, 1)) if form == "per_instance_device" else shared)
            q_dev = capi.DeviceArray(q0)
            o = s.SolvePose(t_dev, q=q_dev, **kw)
        o["q"] = s.get("q")
        outs.append(o)
        s.close()
    for o in outs[1:]:
        for key in ("reached", "steps", "status", "err", "q"):
            assert np.array_equal(o[key], outs[0][key]), key
    # B = 1
    s, _ = _handle(model, 1, links, q0[:1])
    o = s.SolvePose(shared, **kw)
    assert o["err"].shape == (1, 2, 6) and abs(int(o["steps"][0]) - int(outs[0]["steps"][0])) <= 1
    assert o["reached"][0] == (np.abs(o["err"]).max() <= 1e-6)
    s.close()


def test_f32_handle_reaches_1e_3():
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 1)
    B = 1024
    q0, tg = _seeds(model, B, links, seed=13)
    s, _ = _handle(model, B, links, q0, precision=capi.F32, tol_abs=1e-4)
    out = s.SolvePose(tg, tol_pose=1e-3, max_steps=20)
    q = s.get("q")
    s.close()
    r = out["reached"]
    assert r.mean() > 0.8
    assert np.max(np.abs(P.pose_errors(model, q[r], links, tg[r]))) <= 1e-3


# ---- 7. argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors():
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 1)
    B = 8
    q0, tg = _seeds(model, B, links, seed=1)
    s = loik_amd.BatchedLoik(model, B, **dict(PRM))
    with pytest.raises(loik_amd.LoikError) as e:
        s.SolvePose(tg)
    assert e.value.code == -24
    s.close()
    s, _ = _handle(model, B, links, q0)
    for kw in (dict(dt=0.0), dict(dt=-1.0), dict(gain=0.0), dict(tol_pose=-1e-3), dict(max_steps=-1)):
        with pytest.raises(loik_amd.LoikError) as e:
            s.SolvePose(tg, **kw)
        assert e.value.code == -20, kw
    bad = tg.copy()
    bad[3, 0, 0] += 1e-6
    with pytest.raises(loik_amd.LoikError) as e:
        s.SolvePose(bad)
    assert e.value.code == -20
    refl = tg.copy()
    refl[0, 0, :3] *= -1   # orthonormal, determinant -1
    with pytest.raises(loik_amd.LoikError) as e:
        s.SolvePose(refl)
    assert e.value.code == -20
    assert np.array_equal(s.get("q"), q0)   # (rejected before anything changed)
    for links_bad in ([model.njoints], [-1]):
        with pytest.raises(loik_amd.LoikError) as e:
            s.forward_kinematics(links_bad)
        assert e.value.code == -20
    s.close()
