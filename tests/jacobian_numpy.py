"""The numpy reference of include/loik_amd_jacobian.h: frame Jacobians in Pinocchio's three reference frames and the dexterity
measures of a masked, scaled task Jacobian.

frame_jacobians rests on qp_numpy.jacobians -- the LOCAL Jacobian of a link's JOINT frame column by column from the definition, which
test_qp_optimum_cpu.py checks three ways -- and on two frame changes, restated from the header, twists [linear; angular]:

    J_local(f)  = X(iMf)^-1 J_local(i)                  X(R, t) = [[R, [t]x R], [0, R]]   (pose_tasks_numpy.x_inv)
    J_lwa(f)    = blockdiag(oRf, oRf) J_local(f)
    J_world(f)  = X(oMf) J_local(f)                     oMf = oMi iMf                     (pose_tasks_numpy.frame_fk)

dexterity takes the singular values from np.linalg.svd of J^ = D S_r J_local itself, NOT from the Gram matrix the device forms: the
two agree in sigma^2 to a few u sigma_0^2, which is the contract of the header.  test_jacobian_numpy.py proves both functions without a
GPU."""
import numpy as np

import pose_numpy as P
import pose_tasks_numpy as T
import qp_numpy as QP

LOCAL, LOCAL_WORLD_ALIGNED, WORLD = 0, 1, 2
REFERENCES = {"local": LOCAL, "local_world_aligned": LOCAL_WORLD_ALIGNED, "world": WORLD}
# the row masks of the task kinds (loikb_pose_set_tasks): pose, position, orientation, and the two with the spin about z free
KIND_ROWS = {0: 0x3f, 1: 0x07, 2: 0x38, 4: 0x1f, 6: 0x18}


def frame_jacobians(model, q, links, frames=None, reference=LOCAL, J_joint=None):
    """J [B][n][6][nv] of the frames iMf = frames[e] [12] (None: the identity) on `links` for configurations q [B][nq]; J_joint:
    qp_numpy.jacobians(model, q, links) when the caller has it already"""
    reference = REFERENCES.get(reference, reference)
    q = np.atleast_2d(np.asarray(q, dtype=float))
    links = [int(l) for l in links]
    n = len(links)
    frames = np.tile(T.IDENTITY12, (n, 1)) if frames is None else np.asarray(frames, dtype=float).reshape(n, 12)
    Ji = QP.jacobians(model, q, links) if J_joint is None else J_joint
    out = np.empty_like(Ji)
    for e, l in enumerate(links):
        Jl = np.einsum("ij,bjk->bik", T.x_inv(frames[e]), Ji[:, e])
        if reference == LOCAL:
            out[:, e] = Jl
            continue
        R, t = T.frame_fk(model, q, l, frames[e])
        for b in range(q.shape[0]):
            X = QP._action(R[b], t[b] if reference == WORLD else np.zeros(3))
            out[b, e] = X @ Jl[b]
    return out


def row_weights(rows, length):
    """the diagonal of D S_r for a 6-bit mask"""
    w = np.array([(int(rows) >> r) & 1 for r in range(6)], dtype=float)
    w[:3] /= float(length)
    return w


def dexterity(J_local, rows=0x3f, length=1.0):
    """of ONE local Jacobian [6][nv]: dict(sigma [6] descending with zeros from popcount(rows) on, manipulability, inv_condition)"""
    m = bin(int(rows) & 0x3f).count("1")
    Jh = row_weights(rows, length)[:, None] * np.asarray(J_local, dtype=float)
    sv = np.linalg.svd(Jh, compute_uv=False)
    sigma = np.zeros(6)
    k = min(m, sv.size)
    sigma[:k] = sv[:k]
    return dict(sigma=sigma, manipulability=float(np.prod(sigma[:m])), inv_condition=float(sigma[m - 1] / sigma[0]) if sigma[0] > 0 else 0.0)


def dexterity_batch(model, q, links, frames=None, rows=None, length=1.0):
    """dict(sigma [B][n][6], manipulability [B][n], inv_condition [B][n]) as BatchedLoik.frame_dexterity returns it"""
    J = frame_jacobians(model, q, links, frames, LOCAL)
    B, n = J.shape[:2]
    rows = [0x3f] * n if rows is None else [int(r) for r in rows]
    out = dict(sigma=np.empty((B, n, 6)), manipulability=np.empty((B, n)), inv_condition=np.empty((B, n)))
    for b in range(B):
        for e in range(n):
            d = dexterity(J[b, e], rows[e], length)
            for k in out:
                out[k][b, e] = d[k]
    return out
