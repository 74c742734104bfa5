"""The numpy reference of include/loik_amd_shortcut.h: the shortcut rule of the header restated on motion_numpy.difference and
motion_numpy.advance (the certified check) and on pose_multistart_numpy.words (the draws), and the path length.

Per path: keep = 0 .. len - 1, L = len; for round r = 0 .. rounds - 1 while L >= 3: i = word(r, b, 0) mod (L - 2), j = i + 2 +
word(r, b, 1) mod (L - 2 - i); the segment q[keep[i]] (+) s difference(q[keep[i]], q[keep[j]]) is checked by advance; FREE removes
keep[i + 1 .. j - 1].  test_shortcut_numpy.py proves the rule's claims without a GPU."""
import numpy as np

import grid_numpy as GN
import motion_numpy as MN
import pose_multistart_numpy as MS


def draw(seed, rnd, b, L):
    """(i, j) of round rnd on path b with L >= 3 kept waypoints"""
    w = MS.words(seed, rnd, b, np.arange(2))
    i = int(w[0] % np.uint64(L - 2))
    j = i + 2 + int(w[1] % np.uint64(L - 2 - i))
    return i, j


def path_length(model, q_path, n_waypoints=None):
    """[B]: the sum over k < len - 1 of || difference(q_k, q_{k+1}) ||_2, the squares summed in DoF order and the segments in path order
    (np.cumsum adds one by one); finite rows that are equal entry by entry are exactly 0 apart.  len of 0 or 1: 0; len outside 0 .. T: NaN"""
    q_path = np.asarray(q_path, dtype=float)
    B, T = q_path.shape[:2]
    n = np.full(B, T) if n_waypoints is None else np.asarray(n_waypoints)
    out = np.full(B, np.nan)
    for b in range(B):
        if 0 <= n[b] <= T:
            out[b] = _length(model, q_path[b, :max(int(n[b]), 0)])
    return out


def _length(model, rows):
    if rows.shape[0] < 2:
        return 0.0
    dv = MN.difference(model, rows[:-1], rows[1:])
    seg = np.sqrt(np.cumsum(dv * dv, axis=1)[:, -1])
    seg[np.all(rows[:-1] == rows[1:], axis=1)] = 0.0   # (equal rows are exactly 0 apart, as the header has it; a NaN row equals nothing)
    return float(np.cumsum(seg)[-1])


def shortcut(model, q_path, links, spheres, wspheres=(), wboxes=(), pairs=(), n_waypoints=None, rounds=64, seed=0, margin=0.0, tol=1e-3,
             max_evals=256, grid=None):
    """the rule for q_path [B][T][nq]; grid: a grid_numpy.Grid, whose pairs then join the check (grid_numpy.advance).  Returns dict(keep [B][T] (-1 after the kept indices), n_waypoints, tried, accepted, blocked,
    undecided, invalid [B], length_in, length_out [B], q_path [B][T][nq] (the kept rows, the last one repeated), near [B] = some tried
    segment's advance(...)["near"] was set, segments = per path the list of (row i, row j, status) tried).  A path with a count outside
    2 .. T is skipped: counters 0, keep -1, NaN rows and lengths"""
    q_path = np.asarray(q_path, dtype=float)
    B, T, nq = q_path.shape
    n = np.full(B, T, dtype=np.int64) if n_waypoints is None else np.asarray(n_waypoints, dtype=np.int64)
    out = dict(keep=np.full((B, T), -1, dtype=np.int32), q_path=np.full((B, T, nq), np.nan), near=np.zeros(B, dtype=bool),
               length_in=np.full(B, np.nan), length_out=np.full(B, np.nan), segments=[[] for _ in range(B)])
    names = ("n_waypoints", "tried", "accepted", "blocked", "undecided", "invalid")
    for k in names:
        out[k] = np.zeros(B, dtype=np.int32)
    count = {MN.FREE: "accepted", MN.BLOCKED: "blocked", MN.UNDECIDED: "undecided", MN.INVALID: "invalid"}
    live = [b for b in range(B) if 2 <= n[b] <= T]
    keeps = {b: list(range(int(n[b]))) for b in live}
    for b in live:
        out["length_in"][b] = _length(model, q_path[b, keeps[b]])
    for r in range(rounds):   # the paths of a round side by side: one batched advancement serves them all, segment by segment as alone
        draws = [(b,) + draw(seed, r, b, len(keeps[b])) for b in live if len(keeps[b]) >= 3]
        if not draws:
            break
        qa = np.stack([q_path[b, keeps[b][i]] for b, i, j in draws])
        qb = np.stack([q_path[b, keeps[b][j]] for b, i, j in draws])
        res = GN.advance_of(grid)(model, qa, MN.difference(model, qa, qb), links, spheres, wspheres, wboxes, pairs, margin=margin, tol=tol, max_evals=max_evals)
        for k, (b, i, j) in enumerate(draws):
            st, keep = int(res["status"][k]), keeps[b]
            out["tried"][b] += 1
            out["near"][b] |= bool(res["near"][k])
            out["segments"][b].append((keep[i], keep[j], st))
            out[count[st]][b] += 1
            if st == MN.FREE:
                del keep[i + 1:j]
    for b in live:
        keep = keeps[b]
        L = len(keep)
        out["n_waypoints"][b] = L
        out["keep"][b, :L] = keep
        out["q_path"][b] = q_path[b, keep + [keep[-1]] * (T - L)]
        out["length_out"][b] = _length(model, q_path[b, keep])
    return out
