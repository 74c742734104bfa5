"""The numpy reference of include/loik_amd_blend.h: the rule of the header restated on motion_numpy (difference, the table of joint travels,
the centres and the pair clearances), pose_numpy.integrate and retime_numpy's conventions, plainly: a loop per corner, per piece and per
sample.  The advancement of the curves runs all corners of a try in lock step, as motion_numpy.advance runs its segments, so that one
batched forward-kinematics pass serves a sample of every curve that still runs.  test_blend_numpy.py proves the rule's claims without a
GPU."""
import math

import numpy as np

import clearance_numpy as CN
import grid_numpy as GN
import motion_numpy as MN
import pose_numpy as P
import retime_numpy as RN

TRUNCATED, INVALID, SKIPPED = 1, 2, 4
TAKEN, BLOCKED, UNDECIDED, COUPLED, ZERO_LEG, OFF = range(6)
NEAR = MN.NEAR
_COUPLED_NV = {P.J_FREEFLYER: 6, P.J_SPHERICAL: 3, P.J_PLANAR: 3}
_NO_WITNESS = (CN.NONE, -1, -1)


def norm_of(dv):
    """|dv| in the norm of loikb_path_length: the squares summed in DoF order"""
    acc = 0.0
    for x in dv:
        acc += x * x
    return math.sqrt(acc)


def differences(model, rows):
    """dv [L - 1][nv] of consecutive rows: motion_numpy.difference, with exactly 0 for equal rows and, joint by joint, for a joint whose own
    coordinates are equal in the two rows"""
    ch, _ = MN.chain_of(model)
    dvs = MN.difference(model, rows[:-1], rows[1:])
    dvs[np.all(rows[:-1] == rows[1:], axis=1)] = 0.0
    for i in range(1, ch.njoints):
        jt, iq, iv = int(ch.jtype[i]), int(ch.idx_q[i]), int(ch.idx_v[i])
        mq, mv = {P.J_FREEFLYER: (7, 6), P.J_SPHERICAL: (4, 3), P.J_PLANAR: (4, 3), P.J_TRANSLATION: (3, 3), P.J_SPHERICAL_ZYX: (3, 3)}.get(
            jt, (2, 1) if jt in MN._RUB else (1, 1))
        still = np.all(rows[:-1, iq:iq + mq] == rows[1:, iq:iq + mq], axis=1)
        dvs[still, iv:iv + mv] = 0.0
    return dvs


def coupled(model, dva, dvb):
    """a spherical, free-flyer or planar block (sub-joint by sub-joint inside a composite) moves on both legs"""
    ch, _ = MN.chain_of(model)
    for i in range(1, ch.njoints):
        n = _COUPLED_NV.get(int(ch.jtype[i]))
        if n:
            iv = int(ch.idx_v[i])
            if np.any(dva[iv:iv + n] != 0.0) and np.any(dvb[iv:iv + n] != 0.0):
                return True
    return False


def w_of(P0, P2, u):
    return ((1.0 - u) * (1.0 - u)) * P0 + (u * u) * P2


def curve_point(model, qk, P0, P2, u):
    """q(u) = q_k (+) w(u)"""
    return P.integrate(model, np.asarray(qk, dtype=float), w_of(P0, P2, u))


def curve_bound(model, qk, P0, P2, links, spheres):
    """Lambda [ns] of the curve: lin = 2 max, ang = 2 max, tau = max of the table's values for the segments (q_k, P0) and (q_k, P2); a
    SphericalZYX joint counts as its chain of three revolute joints, ang = the sum over its angles of 2 max(|P0_i|, |P2_i|)"""
    ch, link_of = MN.chain_of(model)
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    rec = [(0.0, 0.0, 0.0)]
    for i in range(1, ch.njoints):
        l0, a0, t0 = MN.joint_travel(ch, i, qk, P0)
        l2, a2, t2 = MN.joint_travel(ch, i, qk, P2)
        ang = 2.0 * max(a0, a2)
        if int(ch.jtype[i]) == P.J_SPHERICAL_ZYX:   # its chain of three revolute joints, each angle on its own
            iv = int(ch.idx_v[i])
            ang = sum(2.0 * max(abs(P0[iv + c]), abs(P2[iv + c])) for c in range(3))
        rec.append((2.0 * max(l0, l2), ang, max(t0, t2)))
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


def advance_curves(model, qk, P0, P2, links, spheres, ws, wb, pairs, margin, tol, max_evals, grid=None):
    """the advancement of loik_amd_motion.h on the curves q_k[i] (+) w_i(u), in lock step.  Returns dict(status (MN.FREE / BLOCKED /
    UNDECIDED), evals, min_sampled, witness [n][3], near [n], samples = per curve the list of (u, min)).  grid: a grid_numpy.Grid; the
    table is then grid_numpy's, a witness of kind 4 names the voxel read at the sample of the minimum, and a centre within
    grid_numpy.FACE of a voxel face at some sample sets near"""
    n, ns = qk.shape[0], spheres.shape[0]
    if grid is None:
        names = MN.pair_names(ns, ws.shape[0], wb.shape[0], pairs)
        table = lambda cen: (MN.pair_values(cen, spheres[:, 3], ws, wb, pairs), None)
    else:
        names = GN.pair_names(ns, ws.shape[0], wb.shape[0], grid, pairs)
        table = lambda cen: GN.pair_values(cen, spheres[:, 3], ws, wb, grid, pairs)
    out = dict(status=np.full(n, MN.UNDECIDED, dtype=np.int32), evals=np.zeros(n, dtype=np.int32), min_sampled=np.full(n, np.inf),
               witness=np.tile(np.array(_NO_WITNESS, dtype=np.int32), (n, 1)), near=np.zeros(n, dtype=bool), samples=[[] for _ in range(n)])
    lam_pair = np.zeros((n, names.shape[0]))
    world = names[:, 0] != CN.SELF
    for i in range(n):
        L = curve_bound(model, qk[i], P0[i], P2[i], links, spheres)
        lam_pair[i, world] = L[names[world, 1]]
        lam_pair[i, ~world] = L[names[~world, 1]] + L[names[~world, 2]]
    u = np.zeros(n)
    run = np.arange(n)
    for k in range(max_evals):
        if run.size == 0:
            break
        q = np.stack([curve_point(model, qk[i], P0[i], P2[i], u[i]) for i in run])
        cen = MN.centres(model, q, links, spheres)
        V, vox = table(cen)
        still = []
        for r, i in enumerate(run):
            v = V[r]
            if grid is not None:
                out["near"][i] |= bool(GN.near_face(cen[r], grid))
            o = int(np.argmin(v)) if v.size else -1
            m = float(v[o]) if o >= 0 else np.inf
            out["evals"][i] = k + 1
            out["samples"][i].append((float(u[i]), m))
            if k == 0 or m < out["min_sampled"][i]:
                out["min_sampled"][i] = m
                out["witness"][i] = GN._name(names, o, None if vox is None else vox[r])
            out["near"][i] |= abs(m - margin - tol) <= NEAR
            if m < margin + tol:
                out["status"][i] = MN.BLOCKED
                continue
            if u[i] == 1.0:
                out["status"][i] = MN.FREE
                continue
            if k + 1 == max_evals:
                continue
            pos = lam_pair[i] > 0
            delta = float(np.min((v[pos] - margin) / lam_pair[i, pos])) if pos.any() else np.inf
            out["near"][i] |= abs(u[i] + delta - 1.0) <= NEAR
            u[i] = min(u[i] + delta, 1.0)
            still.append(i)
        run = np.array(still, dtype=int)
    return out


def rate_limit(P0, P2, v_max, a_max):
    """w_max of a blend"""
    inv = max(math.sqrt(float(np.max(2.0 * np.abs(P0 + P2) / a_max))), float(np.max(2.0 * np.abs(P0) / v_max)), float(np.max(2.0 * np.abs(P2) / v_max)))
    return 1.0 / inv


def passes(A, r_in, r_out, w):
    """the forward and the backward pass over the rates w [L] of the corners (index k, 0 where the corner stops; entries 0 and L - 1 are the
    ends of the path); A [L - 1] of the legs.  Returns the lowered rates"""
    w = np.array(w, dtype=float)
    L = w.size
    vout = 0.0
    for k in range(L - 2):          # leg k ends in corner k + 1
        c = k + 1
        if w[c] > 0.0:
            bound = vout * vout + 2.0 * A[k] * (1.0 - r_out[k] - r_in[c])
            vin = 2.0 * r_in[c] * w[c]
            if vin * vin > bound:
                w[c] = math.sqrt(bound) / (2.0 * r_in[c])
        vout = 2.0 * r_out[c] * w[c]
    vin = 0.0
    for k in range(L - 2, 0, -1):   # leg k starts in corner k
        if w[k] > 0.0:
            bound = vin * vin + 2.0 * A[k] * (1.0 - r_out[k] - r_in[k + 1])
            vo = 2.0 * r_out[k] * w[k]
            if vo * vo > bound:
                w[k] = math.sqrt(bound) / (2.0 * r_out[k])
        vin = 2.0 * r_in[k] * w[k]
    return w


def leg_profile(A, V, sl, v0, v1):
    """(D, v_p) of a straight piece of s-length sl from the rate v0 to the rate v1; D = 0 for a piece that does not move"""
    if not (A > 0.0 and sl > 0.0):
        return 0.0, 0.0
    vp = max(min(V, math.sqrt(0.5 * (2.0 * A * sl + v0 * v0 + v1 * v1))), max(v0, v1))
    t1, t3 = (vp - v0) / A, (vp - v1) / A
    s1, s3 = (vp * vp - v0 * v0) / (2.0 * A), (vp * vp - v1 * v1) / (2.0 * A)
    return t1 + max(sl - s1 - s3, 0.0) / vp + t3, vp


def leg_at(rec, tau):
    """(s, sdot) of a leg record dict(D, v0, v1, vp, A, s0, sl) at tau in [0, D]"""
    D, v0, v1, vp, A, s0, sl = (rec[k] for k in ("D", "v0", "v1", "vp", "A", "s0", "sl"))
    t1, t3 = (vp - v0) / A, (vp - v1) / A
    if tau < t1:
        sig, sd = v0 * tau + 0.5 * A * tau * tau, v0 + A * tau
    elif tau <= D - t3:
        sig, sd = (vp * vp - v0 * v0) / (2.0 * A) + vp * (tau - t1), vp
    else:
        r = max(D - tau, 0.0)
        sig, sd = sl - (v1 * r + 0.5 * A * r * r), v1 + A * r
    return s0 + sig, sd


def piece_at(model, rows, dvs, rec, tau):
    """(q, v) of a piece record at tau in [0, D]"""
    k = rec["k"]
    if rec["blend"]:
        w, ri, ro = rec["w"], rec["r_in"], rec["r_out"]
        u = min(w * tau, 1.0)
        ca, cb = -ri * ((1.0 - u) * (1.0 - u)), ro * (u * u)
        x = ca * dvs[k - 1] + cb * dvs[k]
        return P.integrate(model, rows[k], x), (2.0 * (1.0 - u) * ri * w) * dvs[k - 1] + (2.0 * u * ro * w) * dvs[k]
    s, sd = leg_at(rec, tau)
    return (rows[k].copy() if s == 0.0 else P.integrate(model, rows[k], s * dvs[k])), sd * dvs[k]


def blend(model, q_path, links, spheres, wspheres, wboxes, pairs, v_max, a_max, dt, reach, margin=0.0, tol=1e-3, max_evals=256, max_tries=4,
          n_waypoints=None, S=None, grid=None):
    """the rule for q_path [B][T][nq].  S None: timing only.  grid: a grid_numpy.Grid, whose pairs then join the check of a curve.  Returns dict(n_samples, n_waypoints, taken, flags [B], duration [B], corner
    [B][T-2][5], corner_info [B][T-2][6], piece [B][2T-3][4], near [B][T-2] = a decision of the corner's tries lay within NEAR of its
    threshold, w_max [B][T-2] = the rate limits before the passes, records = per path the list of its piece records, dv = per path its
    differences, and with S q_traj [B][S][nq], v_traj [B][S][nv])"""
    q_path = np.asarray(q_path, dtype=float)
    v_max, a_max = np.asarray(v_max, dtype=float), np.asarray(a_max, dtype=float)
    spheres = np.asarray(spheres, dtype=float).reshape(-1, 4)
    ws, wb = np.asarray(wspheres, dtype=float).reshape(-1, 4), np.asarray(wboxes, dtype=float).reshape(-1, 15)
    pairs = list(pairs)
    B, T, nq = q_path.shape
    nv = model.nv
    n = np.full(B, T, dtype=np.int64) if n_waypoints is None else np.asarray(n_waypoints, dtype=np.int64)
    NC, NP = T - 2, 2 * T - 3
    out = dict(n_samples=np.zeros(B, dtype=np.int32), n_waypoints=np.zeros(B, dtype=np.int32), taken=np.zeros(B, dtype=np.int32),
               flags=np.zeros(B, dtype=np.int32), duration=np.full(B, np.nan), corner=np.full((B, NC, 5), np.nan),
               corner_info=np.tile(np.array((OFF, 0, 0) + _NO_WITNESS, dtype=np.int32), (B, NC, 1)), piece=np.full((B, NP, 4), np.nan),
               near=np.zeros((B, NC), dtype=bool), w_max=np.zeros((B, NC)), records=[[] for _ in range(B)], dv=[None] * B)
    if S is not None:
        out["q_traj"], out["v_traj"] = np.full((B, S, nq), np.nan), np.full((B, S, nv), np.nan)
    # the segments
    good, seg = [], {}
    for b in range(B):
        L = int(n[b])
        if not 2 <= L <= T:
            out["flags"][b] = SKIPPED
            continue
        out["n_waypoints"][b] = L
        rows = q_path[b, :L]
        dvs = differences(model, rows)
        if not (np.isfinite(rows).all() and np.isfinite(dvs).all()):
            out["flags"][b] = INVALID
            continue
        nrm, A, V = np.zeros(L - 1), np.zeros(L - 1), np.zeros(L - 1)
        for k in range(L - 1):
            cv, ca = float(np.max(np.abs(dvs[k]) / v_max)), float(np.max(np.abs(dvs[k]) / a_max))
            if cv > 0.0 and ca > 0.0:
                nrm[k], A[k], V[k] = norm_of(dvs[k]), 1.0 / ca, 1.0 / cv
        good.append(b)
        seg[b] = (rows, dvs, nrm, A, V)
        out["dv"][b] = dvs
        out["corner"][b] = 0.0
    # the corners: every try of all corners that still run, in lock step
    pend = []
    for b in good:
        rows, dvs, nrm, A, V = seg[b]
        for k in range(1, rows.shape[0] - 1):
            info = out["corner_info"][b, k - 1]
            if max_tries == 0:
                continue
            if not (nrm[k - 1] > 0.0 and nrm[k] > 0.0):
                info[0] = ZERO_LEG
            elif coupled(model, dvs[k - 1], dvs[k]):
                info[0] = COUPLED
            else:
                pend.append((b, k, min(reach, min(0.5 * nrm[k - 1], 0.5 * nrm[k]))))
    ctl = {}
    for i in range(max_tries):
        if not pend:
            break
        geo = []
        for b, k, base in pend:
            rows, dvs, nrm, A, V = seg[b]
            l = base * 2.0 ** -i
            ri, ro = l / nrm[k - 1], l / nrm[k]
            geo.append((l, ri, ro, -ri * dvs[k - 1], ro * dvs[k]))
        res = advance_curves(model, np.stack([seg[b][0][k] for b, k, _ in pend]), np.stack([g[3] for g in geo]), np.stack([g[4] for g in geo]),
                             links, spheres, ws, wb, pairs, margin, tol, max_evals, grid)
        still = []
        for j, (b, k, base) in enumerate(pend):
            info, cor = out["corner_info"][b, k - 1], out["corner"][b, k - 1]
            st = int(res["status"][j])
            info[0] = TAKEN if st == MN.FREE else BLOCKED if st == MN.BLOCKED else UNDECIDED
            info[1] = i + 1
            info[2] += res["evals"][j]
            info[3:6] = res["witness"][j]
            cor[4] = res["min_sampled"][j]
            out["near"][b, k - 1] |= res["near"][j]
            if st == MN.FREE:
                l, ri, ro, P0, P2 = geo[j]
                cor[:4] = l, ri, ro, rate_limit(P0, P2, v_max, a_max)
                out["w_max"][b, k - 1] = cor[3]
                ctl[(b, k)] = (P0, P2)
            else:
                still.append((b, k, base))
        pend = still
    out["controls"] = ctl
    # the timing and the samples
    for b in good:
        rows, dvs, nrm, A, V = seg[b]
        L = rows.shape[0]
        cor = out["corner"][b]
        r_in, r_out, w = np.zeros(L), np.zeros(L), np.zeros(L)
        r_in[1:L - 1], r_out[1:L - 1], w[1:L - 1] = cor[:L - 2, 1], cor[:L - 2, 2], cor[:L - 2, 3]
        w = passes(A, r_in, r_out, w)
        cor[:L - 2, 3] = w[1:L - 1]
        out["taken"][b] = int(np.sum(out["corner_info"][b, :L - 2, 0] == TAKEN))
        recs, start = [], 0.0
        piece = np.zeros((NP, 4))
        for p in range(2 * L - 3):
            if p & 1:
                k = (p + 1) // 2
                D = 1.0 / w[k] if w[k] > 0.0 else 0.0
                rec = dict(blend=True, k=k, start=start, D=D, w=w[k], r_in=r_in[k], r_out=r_out[k])
                row = (start, D, w[k], w[k])
            else:
                k = p // 2
                v0, v1 = 2.0 * r_out[k] * w[k], 2.0 * r_in[k + 1] * w[k + 1]
                sl = 1.0 - r_out[k] - r_in[k + 1]
                D, vp = leg_profile(A[k], V[k], sl, v0, v1)
                rec = dict(blend=False, k=k, start=start, D=D, v0=v0, v1=v1, vp=vp, A=A[k], V=V[k], s0=r_out[k], sl=sl)
                row = (start, D, v0, v1)
            if D > 0.0:
                piece[p] = row
            recs.append(rec)
            start += D
        total = start
        count = RN.n_samples_of(total, dt)
        out["piece"][b], out["duration"][b], out["n_samples"][b] = piece, total, int(min(count, RN.INT_MAX))
        out["records"][b] = recs
        if S is None:
            continue
        if count > min(S, RN.INT_MAX):
            out["flags"][b] |= TRUNCATED
        starts = np.array([r["start"] for r in recs])
        for i in range(S):
            t = i * dt
            if t >= total:
                out["q_traj"][b, i], out["v_traj"][b, i] = rows[L - 1], 0.0
                continue
            p = int(np.flatnonzero(starts <= t)[-1])
            out["q_traj"][b, i], out["v_traj"][b, i] = piece_at(model, rows, dvs, recs[p], t - recs[p]["start"])
    return out
