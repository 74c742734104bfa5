"""CPU: the numpy reference the GPU tests of include/loik_amd_jacobian.h rest on (tests/jacobian_numpy.py), proven against things it does
not share code with: the linear rows of its LOCAL_WORLD_ALIGNED Jacobian against a central difference of the frame origin taken from
pose_tasks_numpy.frame_fk12, the three reference frames against each other through the frame placement, and its SVD-based dexterity
against the eigenvalues of the Gram matrix."""
import numpy as np
import pytest

import jacobian_numpy as JN
import pose_limits_numpy as PL
import pose_tasks_numpy as T
import qp_cases as C
import qp_numpy as QP

ROBOTS = ["panda7", "talos32", "multidof20", "composite20"]


def _case(name, B=3, seed=17):
    model = C.model_of(name)
    rng = np.random.default_rng(seed)
    q = model.random_configurations(rng, B)
    links = sorted({1, model.njoints // 2, model.njoints - 1} | {int(l) for l in rng.integers(1, model.njoints, size=3)})
    return model, rng, q, links, T.random_frames(rng, len(links))


@pytest.mark.parametrize("name", ROBOTS)
def test_world_aligned_linear_rows_match_a_central_difference(name):
    """d(origin of oMf)/dq_k, k a DoF whose coordinate a plain sum advances, h = 1e-6: rounding u reach / h = 1e-10, truncation h^2 =
    1e-12 of a third derivative of the order of the reach -- 1e-8 max(1, reach) leaves two decades"""
    model, rng, q, links, frames = _case(name)
    B, h = q.shape[0], 1e-6
    J = JN.frame_jacobians(model, q, links, frames, JN.LOCAL_WORLD_ALIGNED)
    qidx = PL.limit_q_index(model)
    plain = np.flatnonzero(qidx >= 0)
    assert plain.size >= 7
    reach = float(np.max(np.abs(T.frame_fk12(model, q, links, frames)[..., 9:])))
    worst = 0.0
    for k in plain:
        qp, qm = q.copy(), q.copy()
        qp[:, qidx[k]] += h
        qm[:, qidx[k]] -= h
        fd = (T.frame_fk12(model, qp, links, frames)[..., 9:] - T.frame_fk12(model, qm, links, frames)[..., 9:]) / (2 * h)
        worst = max(worst, float(np.max(np.abs(fd - J[:, :, :3, k]))))
    print("%s: reach %.3f, worst |fd - J| %.3e over %d plain DoFs" % (name, reach, worst, plain.size))
    assert worst <= 1e-8 * max(1.0, reach), (name, worst, reach)


@pytest.mark.parametrize("name", ROBOTS)
def test_reference_frames_are_consistent(name):
    """identity frames give qp_numpy.jacobians itself; LOCAL -> LOCAL_WORLD_ALIGNED is the rotation of oMf, -> WORLD its action; the
    universe and the off-path columns are exact zeros in all three"""
    model, rng, q, links, frames = _case(name)
    assert np.array_equal(JN.frame_jacobians(model, q, links), QP.jacobians(model, q, links))
    Jl = JN.frame_jacobians(model, q, [0] + links, np.vstack([T.IDENTITY12[None], frames]), "local")
    Ja = JN.frame_jacobians(model, q, [0] + links, np.vstack([T.IDENTITY12[None], frames]), "local_world_aligned")
    Jw = JN.frame_jacobians(model, q, [0] + links, np.vstack([T.IDENTITY12[None], frames]), "world")
    assert not Jl[:, 0].any() and not Ja[:, 0].any() and not Jw[:, 0].any()
    assert np.array_equal((Jl != 0).any(axis=2), (Ja != 0).any(axis=2)) and np.array_equal((Jl != 0).any(axis=2), (Jw != 0).any(axis=2))
    for e, l in enumerate(links):
        R, t = T.frame_fk(model, q, l, frames[e])
        for b in range(q.shape[0]):
            assert np.allclose(Ja[b, e + 1, :3], R[b] @ Jl[b, e + 1, :3], rtol=0, atol=1e-14 * max(1, np.abs(Jl).max()))
            assert np.allclose(Ja[b, e + 1, 3:], R[b] @ Jl[b, e + 1, 3:], rtol=0, atol=1e-14)
            assert np.array_equal(Jw[b, e + 1, 3:], Ja[b, e + 1, 3:])
            lever = np.cross(t[b][None, :], Ja[b, e + 1, 3:].T).T
            assert np.allclose(Jw[b, e + 1, :3], Ja[b, e + 1, :3] + lever, rtol=0, atol=1e-13 * max(1, np.abs(Jw).max()))


@pytest.mark.parametrize("name", ROBOTS)
def test_dexterity_matches_the_gram_eigenvalues(name):
    """sigma^2 of the SVD of J^ against eigvalsh(J^ J^T) to a few u sigma_0^2; zeros past popcount(rows); manipulability and the
    inverse condition number from their definitions; a link with fewer ancestors than selected rows has trailing zeros"""
    model, rng, q, links, frames = _case(name)
    J = JN.frame_jacobians(model, q, links, frames)
    for rows, length in [(0x3f, 1.0), (0x07, 1.0), (0x38, 0.25), (0x1f, 0.25)]:
        m = bin(rows).count("1")
        for b in range(q.shape[0]):
            for e in range(len(links)):
                d = JN.dexterity(J[b, e], rows, length)
                Jh = JN.row_weights(rows, length)[:, None] * J[b, e]
                lam = np.sort(np.linalg.eigvalsh(Jh @ Jh.T))[::-1]
                s0sq = d["sigma"][0] ** 2
                assert np.max(np.abs(d["sigma"] ** 2 - np.maximum(lam, 0.0) * (np.arange(6) < m))) <= 64 * QP.U * max(s0sq, 1e-300)
                assert np.all(d["sigma"][m:] == 0.0) and np.all(np.diff(d["sigma"]) <= 0.0)
                assert d["manipulability"] == np.prod(d["sigma"][:m])
                assert d["inv_condition"] == (d["sigma"][m - 1] / d["sigma"][0] if d["sigma"][0] > 0 else 0.0)
    # link 1 of the arm has one ancestor DoF: rank 1
    if name == "panda7":
        d = JN.dexterity(JN.frame_jacobians(model, q, [1])[0, 0])
        assert d["sigma"][0] > 0.5 and np.all(d["sigma"][1:] <= 1e-15) and d["manipulability"] <= 1e-15 and d["inv_condition"] <= 1e-15
    batch = JN.dexterity_batch(model, q, links, frames, [0x07] * len(links), 0.5)
    assert batch["sigma"].shape == (q.shape[0], len(links), 6)
    assert np.array_equal(batch["sigma"][1, 2], JN.dexterity(J[1, 2], 0x07, 0.5)["sigma"])
