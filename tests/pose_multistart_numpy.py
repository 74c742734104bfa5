"""The CPU side of the multi-start pose IK tests (include/loik_amd_multistart.h): the sampler restated exactly (uint64 arithmetic,
the product rounded before the sum), the selection rule, and the multi-round loop on top of the lock-step oracle with limits
(pose_limits_numpy.lockstep_pose_loop_limits).  No test in here."""
import numpy as np

import pose_limits_numpy as PL
from pose_numpy import POSE_REACHED, POSE_STOPPED

PICK_NEAREST, PICK_FIRST = 0, 1
GOAL_REACHED, GOAL_BEST_EFFORT, GOAL_FAILED = 1, 2, 4

_U = np.uint64
_GOLDEN = _U(0x9E3779B97F4A7C15)


def mix(x):
    """the finalizer of splitmix64 on uint64 arrays (wrapping)"""
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> _U(30)
        x *= _U(0xBF58476D1CE4E5B9)
        x ^= x >> _U(27)
        x *= _U(0x94D049BB133111EB)
        x ^= x >> _U(31)
    return x


def words(seed, rnd, b, j):
    """word(b, j) of round rnd: b and j broadcast against each other"""
    with np.errstate(over="ignore"):
        key = mix(_U(seed % (1 << 64)) + _GOLDEN * _U(rnd + 1))
    b = np.asarray(b, dtype=np.uint64)
    j = np.asarray(j, dtype=np.uint64)
    return mix(key ^ ((b << _U(32)) | j))


def uniforms(seed, rnd, b, j):
    """u in [0, 1): the top 53 bits of the word, exactly"""
    return (words(seed, rnd, b, j) >> _U(11)).astype(np.float64) * 2.0 ** -53


def sampled_dofs(model, s_lo, s_hi):
    """(DoF indices j, their coordinates in q) of the DoFs with a finite pair"""
    qidx = PL.limit_q_index(model)
    j = np.flatnonzero(np.isfinite(s_lo) & np.isfinite(s_hi))
    assert np.all(qidx[j] >= 0), "a finite range on a DoF that cannot carry one"
    return j, qidx[j]


def sample(model, q0, K, seed, rnd, s_lo, s_hi):
    """the seeds of round rnd for ALL instances: [B][nq] with B = G * K from q0 [G][nq] (seed k = 0 of round 0 is the q0 row)"""
    q0 = np.asarray(q0, dtype=float)
    G, nq = q0.shape
    B = G * K
    s_lo, s_hi = np.asarray(s_lo, dtype=float), np.asarray(s_hi, dtype=float)
    q = np.repeat(q0, K, axis=0)
    j, c = sampled_dofs(model, s_lo, s_hi)
    if j.size:
        u = uniforms(seed, rnd, np.arange(B)[:, None], j[None, :])
        prod = u * (s_hi[j] - s_lo[j])[None, :]          # (numpy rounds the product: it is an array of doubles)
        q[:, c] = np.minimum(s_lo[j][None, :] + prod, s_hi[j][None, :])
        if rnd == 0:
            q[::K] = q0
    return q


def resample(model, q, status, q0, K, seed, rnd, s_lo, s_hi):
    """the re-sampler: rows without REACHED get the seeds of round rnd, the others stay"""
    fresh = sample(model, q0, K, seed, rnd, s_lo, s_hi)
    keep = (np.asarray(status) & POSE_REACHED) != 0
    out = np.array(q, dtype=float)
    out[~keep] = fresh[~keep]
    return out, ~keep


def instance_keys(status, err, q, q0, K, pick, qidx, weights=None):
    """(class [B], cost [B]) of the selection rule"""
    status = np.asarray(status)
    B = status.size
    reached, stopped = (status & POSE_REACHED) != 0, (status & POSE_STOPPED) != 0
    cls = np.where(stopped, 2, np.where(reached, 0, 1))
    cost = np.zeros(B)
    with np.errstate(all="ignore"):
        worst = np.abs(np.asarray(err).reshape(B, -1))
        m = worst.max(axis=1)
        m[np.isnan(worst).any(axis=1)] = np.nan
    cost[cls == 1] = m[cls == 1]
    if pick == PICK_NEAREST:
        dof = np.flatnonzero(qidx >= 0)
        w = np.ones(qidx.size) if weights is None else np.asarray(weights, dtype=float)
        d = np.asarray(q)[:, qidx[dof]] - np.repeat(np.asarray(q0), K, axis=0)[:, qidx[dof]]
        near = (w[dof][None, :] * d * d).sum(axis=1)
        cost[cls == 0] = near[cls == 0]
    return cls, cost


def select_tables(cls, cost, status, K):
    """the selection on (class, cost) tables: lexicographic minimum of (class, cost, b) per goal, NaN after every number, ties to
    the lowest b.  Returns dict(winner, goal_status, cost, nreached, margin): margin [G] = (runner-up cost - best cost) / best
    cost among the winner's class (inf when the winner is alone in its class or best is 0 and the runner-up is not)"""
    cls, cost, status = np.asarray(cls), np.asarray(cost, dtype=float), np.asarray(status)
    G = cls.size // K
    winner = np.zeros(G, dtype=np.int32)
    gstat = np.zeros(G, dtype=np.int32)
    wcost = np.zeros(G)
    nreached = np.zeros(G, dtype=np.int32)
    margin = np.full(G, np.inf)
    for g in range(G):
        keys = []
        for b in range(g * K, (g + 1) * K):
            nan = bool(np.isnan(cost[b]))
            keys.append((int(cls[b]), nan, 0.0 if nan else float(cost[b]), b))
        keys.sort()
        best = keys[0]
        winner[g], gstat[g], wcost[g] = best[3], 1 << best[0], cost[best[3]]
        nreached[g] = int(((status[g * K:(g + 1) * K] & POSE_REACHED) != 0).sum())
        if len(keys) > 1 and keys[1][0] == best[0] and not best[1]:
            second = np.inf if keys[1][1] else keys[1][2]
            margin[g] = (second - best[2]) / best[2] if best[2] > 0 else (np.inf if second > 0 else 0.0)
    return dict(winner=winner, goal_status=gstat, cost=wcost, nreached=nreached, margin=margin)


def select(status, err, q, q0, K, pick, qidx, weights=None):
    cls, cost = instance_keys(status, err, q, q0, K, pick, qidx, weights)
    return select_tables(cls, cost, status, K)


def multistart_loop(model, prm, q0, K, rounds, seed, s_lo, s_hi, links, A, lb, ub, targets, dt, gain, tol, max_steps, q_lo, q_hi):
    """the loop of loikb_solve_pose_multistart on the oracle: q0 [G][nq], targets [G][nc][12].  Every round is a fresh
    lockstep_pose_loop_limits from the round's q (reached rows start reached and do not move).  Returns dict(q, status, err, round
    [B], rounds_run, answered: goals with a reached seed after each round)"""
    G = q0.shape[0]
    B = G * K
    tg = np.repeat(np.asarray(targets, dtype=float), K, axis=0)
    q = sample(model, q0, K, seed, 0, s_lo, s_hi)
    rnd_of = np.zeros(B, dtype=np.int32)
    answered = []
    for r in range(rounds):
        o = PL.lockstep_pose_loop_limits(model, prm, q, np.eye(6), np.zeros(6), links, A, lb, ub, tg, dt, gain, tol, max_steps, q_lo, q_hi)
        q, status = o["q"], o["status"]
        ok = ((status & POSE_REACHED) != 0) & ((status & POSE_STOPPED) == 0)
        answered.append(int(ok.reshape(G, K).any(axis=1).sum()))
        if r == rounds - 1 or answered[-1] == G:
            break
        q, fresh = resample(model, q, status, q0, K, seed, r + 1, s_lo, s_hi)
        rnd_of[fresh] = r + 1
    return dict(q=q, status=status, err=o["err"], round=rnd_of, rounds_run=len(answered), answered=answered, reached=ok)
