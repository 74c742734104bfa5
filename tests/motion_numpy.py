"""The numpy reference of include/loik_amd_motion.h: difference (the inverse of pose_numpy.integrate), the motion bound Lambda of every
robot sphere over a segment q(s) = qa (+) s dv, and the conservative advancement with its certificate.

Restated from the header on top of pose_numpy (joint motions, integrate, log3 / log6) and clearance_numpy (the three distance formulas,
the pair ordinals).  The advancement runs all segments in lock step so that one batched forward-kinematics pass serves a sample of
every segment that still runs; test_motion_numpy.py proves difference, the bound and the certificate without a GPU."""
import numpy as np

from loik_amd import workloads as W
import clearance_numpy as CN
import pose_numpy as P

FREE, BLOCKED, UNDECIDED, INVALID = 0, 1, 2, 3
NEAR = 1e-9   # a decision of the reference this close to its threshold may fall the other way on the device

_REV = (P.J_RX, P.J_RY, P.J_RZ, P.J_RU, P.J_RUBX, P.J_RUBY, P.J_RUBZ, P.J_RUBU)
_PRI = (P.J_PX, P.J_PY, P.J_PZ, P.J_PU)
_HEL = (P.J_HX, P.J_HY, P.J_HZ, P.J_HU)
_RUB = (P.J_RUBX, P.J_RUBY, P.J_RUBZ, P.J_RUBU)


def chain_of(model):
    """(the model with every composite written out as its sub-joints, the chain joint that carries each of the caller's links)"""
    if getattr(model, "composite", None):
        ch = getattr(model, "_chain_cache", None)
        if ch is None:
            ch = model._chain_cache = W._Chain(model)
        return ch, [int(l) for l in ch.link_of]
    return model, list(range(model.njoints))


def _quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                     a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def difference(model, q0, q1):
    """v [n][nv] with integrate(q0, v) = q1, per joint type as the header lists them; a row that is not finite yields a NaN row"""
    ch, _ = chain_of(model)
    q0, q1 = np.atleast_2d(np.asarray(q0, dtype=float)), np.atleast_2d(np.asarray(q1, dtype=float))
    nv = int(model.nv)
    out = np.full((q0.shape[0], nv), np.nan)
    for r in range(q0.shape[0]):
        a, b = q0[r], q1[r]
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            continue
        v = np.zeros(nv)
        for i in range(1, ch.njoints):
            jt, iq, iv = int(ch.jtype[i]), int(ch.idx_q[i]), int(ch.idx_v[i])
            if jt == P.J_FREEFLYER:
                R0, R1 = W.quat_rot(a[None, iq + 3:iq + 7])[0], W.quat_rot(b[None, iq + 3:iq + 7])[0]
                v[iv:iv + 6] = P.log6(R0.T @ R1, R0.T @ (b[iq:iq + 3] - a[iq:iq + 3]))
            elif jt == P.J_SPHERICAL:
                qa = a[iq:iq + 4]
                qr = _quat_mul(np.array([-qa[0], -qa[1], -qa[2], qa[3]]), b[iq:iq + 4])
                v[iv:iv + 3] = P.log3(W.quat_rot(qr[None])[0])
            elif jt == P.J_PLANAR:
                c0, s0, c1, s1 = a[iq + 2], a[iq + 3], b[iq + 2], b[iq + 3]
                w = np.arctan2(c0 * s1 - s0 * c1, c0 * c1 + s0 * s1)
                ex, ey = b[iq] - a[iq], b[iq + 1] - a[iq + 1]
                px, py = c0 * ex + s0 * ey, c0 * ey - s0 * ex
                al, bq = np.sinc(w / np.pi), np.sin(0.5 * w) * np.sinc(0.5 * w / np.pi)   # integrate's V = [[al, -bq], [bq, al]]
                det = al * al + bq * bq
                v[iv:iv + 3] = (al * px + bq * py) / det, (al * py - bq * px) / det, w
            elif jt in _RUB:
                v[iv] = np.arctan2(a[iq] * b[iq + 1] - a[iq + 1] * b[iq], a[iq] * b[iq] + a[iq + 1] * b[iq + 1])
            elif jt in (P.J_TRANSLATION, P.J_SPHERICAL_ZYX):
                v[iv:iv + 3] = b[iq:iq + 3] - a[iq:iq + 3]
            else:
                v[iv] = b[iq] - a[iq]
        out[r] = v
    return out


def interpolate(model, qa, dv, s):
    """q(s) = qa (+) s dv of one segment"""
    return P.integrate(model, np.asarray(qa, dtype=float), s * np.asarray(dv, dtype=float))


def joint_travel(ch, i, qa, dv):
    """(lin, ang, tau) of joint i of a model without composites over the segment: the table of the header"""
    jt, iq, iv = int(ch.jtype[i]), int(ch.idx_q[i]), int(ch.idx_v[i])
    n = np.linalg.norm
    if jt in _REV:
        return 0.0, abs(dv[iv]), 0.0
    if jt in _PRI:
        return abs(dv[iv]), 0.0, max(abs(qa[iq]), abs(qa[iq] + dv[iv]))
    if jt in _HEL:
        h = float(ch.pitch[i])
        return abs(h * dv[iv]), abs(dv[iv]), abs(h) * max(abs(qa[iq]), abs(qa[iq] + dv[iv]))
    if jt == P.J_TRANSLATION:
        return n(dv[iv:iv + 3]), 0.0, max(n(qa[iq:iq + 3]), n(qa[iq:iq + 3] + dv[iv:iv + 3]))
    if jt == P.J_SPHERICAL:
        return 0.0, n(dv[iv:iv + 3]), 0.0
    if jt == P.J_SPHERICAL_ZYX:
        return 0.0, abs(dv[iv]) + abs(dv[iv + 1]) + abs(dv[iv + 2]), 0.0
    if jt == P.J_FREEFLYER:
        return n(dv[iv:iv + 3]), n(dv[iv + 3:iv + 6]), n(qa[iq:iq + 3]) + n(dv[iv:iv + 3])
    if jt == P.J_PLANAR:
        return n(dv[iv:iv + 2]), abs(dv[iv + 2]), n(qa[iq:iq + 2]) + n(dv[iv:iv + 2])
    raise ValueError("joint type %d" % jt)


def motion_bound(model, qa, dv, links, spheres):
    """Lambda [ns] of one segment: the sum over the joints J on the root path of the sphere's link of lin_J + ang_J rho_J, rho_J = |c| +
    the sum of |p_K| + tau_K over the joints strictly below J"""
    ch, link_of = chain_of(model)
    qa, dv = np.asarray(qa, dtype=float), np.asarray(dv, dtype=float)
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    rec = [(0.0, 0.0, 0.0)] + [joint_travel(ch, i, qa, dv) for i in range(1, ch.njoints)]
    pn = [float(np.linalg.norm(np.asarray(ch.placement[i], dtype=float)[9:12])) for i in range(ch.njoints)]
    out = np.zeros(len(links))
    for s, l in enumerate(links):
        reach, L = float(np.linalg.norm(spheres[s, :3])), 0.0
        j = link_of[int(l)]
        while j > 0:
            lin, ang, tau = rec[j]
            L += lin + ang * reach
            reach += pn[j] + tau
            j = int(ch.parents[j])
        out[s] = L
    return out


def placements(model, q):
    """world placements of every link of the chain model for q [B][nq], root side first as pose_numpy.fk composes them:
    (R [nj][B][3][3], t [nj][B][3])"""
    ch, _ = chain_of(model)
    B = q.shape[0]
    R, t = [np.broadcast_to(np.eye(3), (B, 3, 3))], [np.zeros((B, 3))]
    for i in range(1, ch.njoints):
        Pl = np.asarray(ch.placement[i], dtype=float)
        Rp, tp = Pl[:9].reshape(3, 3), Pl[9:]
        Rj, tj = P.joint_motion(ch, i, q)
        Rl, tl = Rp[None] @ Rj, tp[None] + tj @ Rp.T
        p = int(ch.parents[i])
        t.append(t[p] + np.einsum("bij,bj->bi", R[p], tl))
        R.append(R[p] @ Rl)
    return R, t


def centres(model, q, links, spheres):
    """world centres [B][ns][3] (clearance_numpy.centres with one forward-kinematics pass for all links)"""
    _, link_of = chain_of(model)
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    R, t = placements(model, q)
    out = np.empty((q.shape[0], len(links), 3))
    for s, l in enumerate(links):
        j = link_of[int(l)]
        out[:, s] = t[j] + np.einsum("bij,j->bi", R[j], spheres[s, :3])
    return out


def pair_values(cen, radii, ws, wb, pairs):
    """every pair clearance [B][npairs_total] in ordinal order (clearance_numpy.pair_table, vectorised over the pairs)"""
    B, ns = cen.shape[:2]
    cols = []
    if ws.shape[0]:
        cols.append(CN.sphere_sphere(cen[:, :, None, :], radii[None, :, None], ws[None, None, :, :3], ws[None, None, :, 3]).reshape(B, -1))
    if wb.shape[0]:
        cols.append(np.stack([CN.sphere_box(cen, radii[None, :], wb[o]) for o in range(wb.shape[0])], axis=2).reshape(B, -1))
    if len(pairs):
        pa, pb = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
        cols.append(CN.sphere_sphere(cen[:, pa], radii[None, pa], cen[:, pb], radii[None, pb]))
    return np.concatenate(cols, axis=1) if cols else np.zeros((B, 0))


def pair_names(ns, nws, nwb, pairs):
    """(kind, a, b) [npairs_total][3] of every ordinal"""
    rows = [(CN.WORLD_SPHERE, a, o) for a in range(ns) for o in range(nws)] + [(CN.WORLD_BOX, a, o) for a in range(ns) for o in range(nwb)]
    rows += [(CN.SELF, int(a), int(b)) for a, b in pairs]
    return np.array(rows, dtype=np.int32).reshape(-1, 3)


def advance(model, qa, dv, links, spheres, wspheres=(), wboxes=(), pairs=(), margin=0.0, tol=1e-3, max_evals=256):
    """the conservative advancement of the header for segments qa [n][nq], dv [n][nv].  Returns dict(status [n], evals [n], s_free [n],
    min_sampled [n], s_at_min [n], witness [n][3], near [n] = some decision lay within NEAR of its threshold, Lambda [n][ns], samples =
    per segment the list of (s, min clearance) taken)"""
    qa, dv = np.atleast_2d(np.asarray(qa, dtype=float)), np.atleast_2d(np.asarray(dv, dtype=float))
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    ws, wb = np.asarray(wspheres, dtype=float).reshape(-1, 4), np.asarray(wboxes, dtype=float).reshape(-1, 15)
    pairs = list(pairs)
    n, ns = qa.shape[0], spheres.shape[0]
    names = pair_names(ns, ws.shape[0], wb.shape[0], pairs)
    out = dict(status=np.full(n, UNDECIDED, dtype=np.int32), evals=np.zeros(n, dtype=np.int32), s_free=np.zeros(n), min_sampled=np.full(n, np.inf),
               s_at_min=np.zeros(n), witness=np.tile(np.array([CN.NONE, -1, -1], dtype=np.int32), (n, 1)), near=np.zeros(n, dtype=bool),
               Lambda=np.zeros((n, ns)), samples=[[] for _ in range(n)])
    ok = np.isfinite(qa).all(axis=1) & np.isfinite(dv).all(axis=1)
    for i in np.flatnonzero(~ok):
        out["status"][i] = INVALID
        out["s_free"][i] = out["min_sampled"][i] = out["s_at_min"][i] = np.nan
    lam_pair = np.zeros((n, names.shape[0]))
    for i in np.flatnonzero(ok):
        L = out["Lambda"][i] = motion_bound(model, qa[i], dv[i], links, spheres)
        world = names[:, 0] != CN.SELF
        lam_pair[i, world] = L[names[world, 1]]
        lam_pair[i, ~world] = L[names[~world, 1]] + L[names[~world, 2]]
    s = np.zeros(n)
    run = np.flatnonzero(ok)
    for k in range(max_evals):
        if run.size == 0:
            break
        q = np.stack([interpolate(model, qa[i], dv[i], s[i]) for i in run])
        V = pair_values(centres(model, q, links, spheres), spheres[:, 3], ws, wb, pairs)
        still = []
        for r, i in enumerate(run):
            v = V[r]
            o = int(np.argmin(v)) if v.size else -1          # the first of equal minima: the lowest ordinal
            m = float(v[o]) if o >= 0 else np.inf
            out["evals"][i] = k + 1
            out["samples"][i].append((float(s[i]), m))
            out["s_free"][i] = s[i]
            if k == 0 or m < out["min_sampled"][i]:
                out["min_sampled"][i], out["s_at_min"][i] = m, s[i]
                out["witness"][i] = names[o] if o >= 0 else (CN.NONE, -1, -1)
            out["near"][i] |= abs(m - margin - tol) <= NEAR
            if m < margin + tol:
                out["status"][i] = BLOCKED
                continue
            if s[i] == 1.0:
                out["status"][i] = FREE
                continue
            if k + 1 == max_evals:
                continue
            pos = lam_pair[i] > 0
            delta = float(np.min((v[pos] - margin) / lam_pair[i, pos])) if pos.any() else np.inf
            out["near"][i] |= abs(s[i] + delta - 1.0) <= NEAR
            s[i] = min(s[i] + delta, 1.0)
            still.append(i)
        run = np.array(still, dtype=int)
    return out


def clearance_min(model, q, links, spheres, wspheres=(), wboxes=(), pairs=()):
    """the minimum clearance [B] of configurations q [B][nq] (what clearance_numpy.clearance calls min), for dense sampling"""
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    ws, wb = np.asarray(wspheres, dtype=float).reshape(-1, 4), np.asarray(wboxes, dtype=float).reshape(-1, 15)
    V = pair_values(centres(model, np.atleast_2d(q), links, spheres), spheres[:, 3], ws, wb, list(pairs))
    return V.min(axis=1) if V.shape[1] else np.full(V.shape[0], np.inf)


def interpolate_many(model, qa, dv, ss):
    """q(s) [len(ss)][nq] of one segment: the plain-sum joints for all s at once (the same sum as pose_numpy.integrate), and a model
    with a joint on a manifold one s at a time"""
    ch, _ = chain_of(model)
    qa, dv, ss = np.asarray(qa, dtype=float), np.asarray(dv, dtype=float), np.asarray(ss, dtype=float)
    plain3 = (P.J_TRANSLATION, P.J_SPHERICAL_ZYX)
    if any(int(ch.jtype[i]) in (P.J_FREEFLYER, P.J_SPHERICAL, P.J_PLANAR) + _RUB for i in range(1, ch.njoints)):
        return np.stack([interpolate(model, qa, dv, s) for s in ss])
    out = np.tile(qa, (ss.size, 1))
    for i in range(1, ch.njoints):
        iq, iv, n = int(ch.idx_q[i]), int(ch.idx_v[i]), 3 if int(ch.jtype[i]) in plain3 else 1
        out[:, iq:iq + n] = qa[iq:iq + n] + ss[:, None] * dv[iv:iv + n]
    return out


def thin_box_across(model, qa, dv, link, sphere, s=0.5, half=(0.05, 0.05, 0.005)):
    """a box [15] centred where the centre of `sphere` (x, y, z, r on `link`) is at q(s), its thin axis (z) along the centre's direction of
    travel there: the obstacle a sampled check misses"""
    c = centres(model, interpolate_many(model, qa, dv, [s - 1e-4, s, s + 1e-4]), [link], [sphere])[:, 0]
    z = (c[2] - c[0]) / np.linalg.norm(c[2] - c[0])
    x = np.cross(z, [1.0, 0.0, 0.0] if abs(z[0]) < 0.9 else [0.0, 1.0, 0.0])
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z], axis=1)
    return np.concatenate([R.reshape(9), c[1], np.asarray(half, dtype=float)])
