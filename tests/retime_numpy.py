"""The numpy reference of include/loik_amd_retime.h: the retiming rule of the header restated on motion_numpy.difference and
pose_numpy.integrate, plainly, a loop per segment and a loop per sample.

Per segment k < L - 1: dv = difference(q_k, q_{k+1}) (equal rows: 0), cv = max |dv_j| / v_max_j, ca = max |dv_j| / a_max_j, A = 1 / ca;
triangular (ca >= cv cv): D = 2 sqrt(ca), t_acc = sqrt(ca), peak = 1 / sqrt(ca); trapezoid: D = cv + ca / cv, t_acc = ca / cv, peak = 1 / cv.
test_retime_numpy.py proves the rule's claims without a GPU."""
import math

import numpy as np

import motion_numpy as MN
import pose_numpy as P

SNAP = 1
TRUNCATED, INVALID, SKIPPED = 1, 2, 4
INT_MAX = 2 ** 31 - 1
TICK_MAX = 2 ** 31   # the ticks of one segment saturate here: no sample index reaches past it


def segment(dv, v_max, a_max, dt, snap):
    """(duration, t_acc, peak, A, ticks, triangular) of one segment; ticks is 0 without snap.  A segment that does not move is all 0"""
    cv = float(np.max(np.abs(dv) / v_max))
    ca = float(np.max(np.abs(dv) / a_max))
    if not (cv > 0.0 and ca > 0.0):
        return 0.0, 0.0, 0.0, 0.0, 0, False
    A = 1.0 / ca
    tri = ca >= cv * cv
    if tri:
        rt = math.sqrt(ca)
        D, t_acc, peak = 2.0 * rt, rt, 1.0 / rt
    else:
        t_acc = ca / cv
        D, peak = cv + t_acc, 1.0 / cv
    n = 0
    if snap:
        nd = math.ceil(D / dt) if math.isfinite(D / dt) else math.inf
        n = int(min(nd, TICK_MAX))
        D = dt * nd
        peak = 2.0 / (D + math.sqrt(max(D * D - 4.0 * ca, 0.0)))
        t_acc = peak * ca
    return D, t_acc, peak, A, n, tri


def profile(tau, D, t_acc, peak, A):
    """(s, sdot) of a segment's profile at tau in [0, D)"""
    if tau < t_acc:
        return 0.5 * A * tau * tau, A * tau
    if tau <= D - t_acc:
        return peak * (tau - 0.5 * t_acc), peak
    r = max(D - tau, 0.0)
    return 1.0 - 0.5 * A * r * r, A * r


def n_samples_of(D, dt):
    """ceil(D / dt) + 1, not yet saturated"""
    return math.ceil(D / dt) + 1 if math.isfinite(D / dt) else math.inf


def retime(model, q_path, v_max, a_max, dt, n_waypoints=None, S=None, snap=False):
    """the rule for q_path [B][T][nq].  S None: timing only.  Returns dict(n_samples, n_waypoints, moved, flags [B], duration [B],
    seg [B][T-1][4], ticks [B][T] (the tick N_k of waypoint k with snap, else 0), regimes = per path the list of 'tri' / 'trap' / None
    per segment, and with S q_traj [B][S][nq], v_traj [B][S][nv])"""
    q_path = np.asarray(q_path, dtype=float)
    v_max, a_max = np.asarray(v_max, dtype=float), np.asarray(a_max, dtype=float)
    B, T, nq = q_path.shape
    nv = model.nv
    n = np.full(B, T, dtype=np.int64) if n_waypoints is None else np.asarray(n_waypoints, dtype=np.int64)
    out = dict(n_samples=np.zeros(B, dtype=np.int32), n_waypoints=np.zeros(B, dtype=np.int32), moved=np.zeros(B, dtype=np.int32),
               flags=np.zeros(B, dtype=np.int32), duration=np.full(B, np.nan), seg=np.full((B, T - 1, 4), np.nan),
               ticks=np.zeros((B, T), dtype=np.int64), regimes=[[] for _ in range(B)])
    if S is not None:
        out["q_traj"], out["v_traj"] = np.full((B, S, nq), np.nan), np.full((B, S, nv), np.nan)
    for b in range(B):
        L = int(n[b])
        if not 2 <= L <= T:
            out["flags"][b] = SKIPPED
            continue
        out["n_waypoints"][b] = L
        rows = q_path[b, :L]
        dvs = MN.difference(model, rows[:-1], rows[1:])
        dvs[np.all(rows[:-1] == rows[1:], axis=1)] = 0.0
        if not (np.isfinite(rows).all() and np.isfinite(dvs).all()):
            out["flags"][b] = INVALID
            continue
        recs, start, tick = [], 0.0, 0
        seg = np.zeros((T - 1, 4))
        for k in range(L - 1):
            D, t_acc, peak, A, nk, tri = segment(dvs[k], v_max, a_max, dt, snap)
            t0 = dt * tick if snap else start
            recs.append((t0, D, t_acc, peak, A, tick))
            seg[k] = (t0, D, t_acc, peak) if D > 0.0 else 0.0   # (a segment that does not move: a record of zeros)
            out["regimes"][b].append(None if D == 0.0 else "tri" if tri else "trap")
            out["ticks"][b, k] = tick
            start, tick = start + D, tick + nk
        out["ticks"][b, L - 1:] = tick
        total = dt * tick if snap else start
        count = tick + 1 if snap else n_samples_of(total, dt)
        ns = int(min(count, INT_MAX))
        out["seg"][b], out["duration"][b], out["n_samples"][b] = seg, total, ns
        out["moved"][b] = sum(r[1] > 0.0 for r in recs)
        if S is None:
            continue
        if count > min(S, INT_MAX):   # (a count that saturates is truncated whatever S is)
            out["flags"][b] |= TRUNCATED
        for i in range(S):
            t = i * dt
            if (i >= tick) if snap else (t >= total):
                out["q_traj"][b, i], out["v_traj"][b, i] = rows[L - 1], 0.0
                continue
            k = max(k for k in range(L - 1) if ((recs[k][5] <= i) if snap else (recs[k][0] <= t)))
            t0, D, t_acc, peak, A, tk = recs[k]
            tau = (i - tk) * dt if snap else t - t0
            s, sd = profile(tau, D, t_acc, peak, A)
            out["q_traj"][b, i] = rows[k] if s == 0.0 else P.integrate(model, rows[k], s * dvs[k])
            out["v_traj"][b, i] = sd * dvs[k]
    return out
