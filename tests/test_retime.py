"""GPU: time-optimal retiming of include/loik_amd_retime.h against the numpy reference of tests/retime_numpy.py (proven on the CPU by
test_retime_numpy.py, which also fixes the inputs): the eight robots of test_clearance.ROBOTS (tree330 also with its tables in the global
slab), the inequalities of the rule on the device's own outputs, the shapes, the edge cases, the certificate that carries over, the
pointer routes, neutrality towards the solves, determinism and the validation."""
import ctypes as C

import numpy as np
import pytest

import loik_amd
from loik_amd import capi

import motion_numpy as MN
import pose_numpy as P
import retime_numpy as RN
import test_clearance as TC
import test_motion_clearance as TM
import test_retime_numpy as TR
import test_shortcut as TS

pytestmark = pytest.mark.gpu

ERR_ARG = -20
T_PATH, DT, S_ROWS = TR.T_PATH, TR.DT, TR.S_ROWS
FLOATS = ("duration", "seg", "q_traj", "v_traj")
INTS = ("n_samples", "n_waypoints", "moved", "flags")
# max |got - numpy| / (1 + |numpy|) over duration, seg, q_traj and v_traj: 16 times the largest error measured on one MI355X over the
# eight robots of test 1, with and without SNAP (profiles/retime_measured.md), the allowance for another compiler's rounding, as
# LENGTH_BOUND of test_shortcut.py was set
RETIME_MEASURED = 1.517e-13   # (multidof20; multidof13 1.47e-13, composite20 6.5e-15, the robots without a free-flyer or planar joint 7e-17 .. 6e-16)
RETIME_BOUND = 16 * RETIME_MEASURED
# the rng of the paths: 1200 unless a robot's reference has a D / dt within 1e-9 of an integer (then the next one, recorded here)
RNG_OF = {}


def _case(name):
    return TR.retime_case(name, RNG_OF.get(name, TR.RNG))


def _open(c, precision=capi.F64):
    return TC._open(c["model"], c["q"], precision)      # no spheres: none are needed


def _kw(c, **over):
    return dict(dict(v_max=c["v_max"], a_max=c["a_max"], dt=DT), **over)


def _error(got, want):
    """|got - want| / (1 + |want|), the largest of each float output; NaN where the reference has NaN"""
    err = {}
    for k in FLOATS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), k
        ok = ~np.isnan(w)
        err[k] = float(np.max(np.abs(g[ok] - w[ok]) / (1.0 + np.abs(w[ok])), initial=0.0))
    return err


def _check(name, what, got, want):
    for k in INTS:
        assert np.array_equal(got[k], want[k]), (name, what, k, got[k], want[k])
    each = _error(got, want)
    err = max(each.values())
    print("retime_measured %s %s: max |got - numpy| / (1 + |numpy|) %.3e (%s)" % (name, what, err, ", ".join("%s %.1e" % kv for kv in each.items())))
    assert err <= RETIME_BOUND, (name, what, each)
    return err


def _same(a, b, keys=FLOATS + INTS):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _ticks(got):
    """N_k of every waypoint from a SNAP result: exact, seg's t_start is dt N_k and its duration dt n_k"""
    n = np.rint(got["seg"][:, :, 1] / DT).astype(np.int64)
    return np.concatenate([np.zeros((n.shape[0], 1), dtype=np.int64), np.cumsum(n, axis=1)], axis=1)


# ---- 1. against numpy on eight robots ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.ROBOTS))
def test_retime_matches_numpy(name):
    c = _case(name)
    model, paths, B = c["model"], c["paths"], c["B"]
    TR.check_comparable(c["want"][False])      # (what makes the integers comparable; the six small robots are checked on the CPU too)
    s = _open(c)
    for snap in (False, True):
        want = c["want"][snap]
        got = s.retime_paths(paths, max_samples=S_ROWS, snap=snap, **_kw(c))
        _check(name, "snap" if snap else "free", got, want)
        if snap:
            N = want["ticks"]
            assert np.array_equal(_ticks(got), N) and np.array_equal(got["seg"][:, :, 0], DT * N[:, :-1]) and np.array_equal(got["duration"], DT * N[:, -1])
            assert np.array_equal(got["seg"][:, :, 1], DT * np.diff(N, axis=1))
    if name == "tree330":
        # the tables of a wavefront are [T - 1][5 + nv] doubles, in LDS only when they fit 64 KB: 32 rows of which the first 6 are
        # waypoints leave no choice but the slab, and the result is the one of T = 6, bit for bit
        T_big = 32
        assert (T_big - 1) * (5 + model.nv) * 8 > 65536 >= (T_PATH - 1) * (5 + model.nv) * 8
        wide = np.concatenate([paths, np.full((B, T_big - T_PATH, model.nq), np.nan)], axis=1)
        n = np.full(B, T_PATH, dtype=np.int32)
        for snap in (False, True):
            lds = s.retime_paths(paths, max_samples=S_ROWS, snap=snap, **_kw(c))
            slab = s.retime_paths(wide, n_waypoints=n, max_samples=S_ROWS, snap=snap, **_kw(c))
            assert _same(lds, slab, ("duration", "q_traj", "v_traj") + INTS)
            assert np.array_equal(slab["seg"][:, :T_PATH - 1], lds["seg"]) and np.all(slab["seg"][:, T_PATH - 1:] == 0.0)
            _check(name, "slab snap" if snap else "slab free", dict(slab, seg=slab["seg"][:, :T_PATH - 1]), c["want"][snap])
    s.close()


# ---- 2. the inequalities of the rule on the device's own outputs -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["panda7", "multidof13", "multidof20"])
def test_limits_hold_on_the_device_outputs(name):
    c = _case(name)
    model, paths, v_max, a_max, B = c["model"], c["paths"], c["v_max"], c["a_max"], c["B"]
    s = _open(c)
    free = s.retime_paths(paths, max_samples=S_ROWS, **_kw(c))
    snap = s.retime_paths(paths, max_samples=S_ROWS, snap=True, **_kw(c))
    dv = s.difference(paths[:, :-1].reshape(-1, model.nq), paths[:, 1:].reshape(-1, model.nq)).reshape(B, T_PATH - 1, model.nv)
    for r in (free, snap):
        TR.check_limits(r, v_max, a_max, DT)
        t0, D, t_acc, peak = (r["seg"][:, :, k] for k in range(4))
        A = peak / t_acc
        sat_v = np.max(peak[:, :, None] * np.abs(dv) / v_max, axis=2)
        sat_a = np.max(A[:, :, None] * np.abs(dv) / a_max, axis=2)
        assert np.all(sat_v <= 1.0 + 1e-12) and np.all(np.abs(sat_a - 1.0) <= 1e-12)
        if r is free:
            assert np.all((np.abs(sat_v - 1.0) <= 1e-12) | (t_acc * 2.0 == D))     # trapezoid: the velocity limit; triangular: D = 2 t_acc
        for b in range(B):
            ns = int(r["n_samples"][b])
            assert np.array_equal(r["q_traj"][b, 0], paths[b, 0]) and np.array_equal(r["q_traj"][b, ns - 1:], np.tile(paths[b, -1], (S_ROWS - ns + 1, 1)))
            assert np.all(r["v_traj"][b, ns - 1:] == 0.0) and np.any(r["v_traj"][b, ns - 2] != 0.0)
    # SNAP: waypoint k at sample N_k bit for bit, at rest; no peak raised, no segment stretched by a whole sample
    N = _ticks(snap)
    for b in range(B):
        assert snap["n_samples"][b] == N[b, -1] + 1
        for k in range(T_PATH):
            assert np.array_equal(snap["q_traj"][b, N[b, k]], paths[b, k]) and np.all(snap["v_traj"][b, N[b, k]] == 0.0)
    assert np.all(snap["seg"][:, :, 3] <= free["seg"][:, :, 3]) and np.all(snap["seg"][:, :, 1] >= free["seg"][:, :, 1])
    assert np.all(snap["seg"][:, :, 1] - free["seg"][:, :, 1] < DT)
    # every sample lies on its segment: difference(q_k, sample) is s dv_k with one s in [0, 1] for all DoFs
    b = 0
    starts = free["seg"][b, :, 0]
    for i in range(1, int(free["n_samples"][b]) - 1, 7):
        k = int(np.searchsorted(starts, i * DT, side="right")) - 1
        d = s.difference(paths[b, k][None], free["q_traj"][b, i][None])[0]
        j = int(np.argmax(np.abs(dv[b, k])))
        sk = d[j] / dv[b, k, j]
        assert 0.0 <= sk <= 1.0 and np.allclose(d, sk * dv[b, k], rtol=0, atol=1e-9), (name, i, k)
    s.close()


# ---- 3. shapes ---------------------------------------------------------------------------------------------------------------------------
def test_shapes():
    c = _case("talos32")
    model, paths, want = c["model"], c["paths"], c["want"][False]
    s = _open(c)
    full = s.retime_paths(paths, max_samples=S_ROWS, **_kw(c))
    for B in (1, 5, 13):
        got = s.retime_paths(paths[:B], max_samples=S_ROWS, **_kw(c))
        assert _same(got, {k: full[k][:B] for k in FLOATS + INTS})
    # S sized by the call itself: the largest n_samples; then every row of the longest path is used
    auto = s.retime_paths(paths, **_kw(c))
    S = int(full["n_samples"].max())
    assert auto["q_traj"].shape == (c["B"], S, model.nq) and auto["v_traj"].shape == (c["B"], S, model.nv) and np.all(auto["flags"] == 0)
    assert np.array_equal(auto["q_traj"], full["q_traj"][:, :S]) and np.array_equal(auto["v_traj"], full["v_traj"][:, :S])
    # S = 100: TRUNCATED, the first 100 rows those of the full call; S = 1
    for S in (100, 1):
        cut = s.retime_paths(paths, max_samples=S, **_kw(c))
        assert np.all(cut["flags"] == capi.RETIME_TRUNCATED) and np.array_equal(cut["n_samples"], full["n_samples"])
        assert np.array_equal(cut["q_traj"], full["q_traj"][:, :S]) and np.array_equal(cut["v_traj"], full["v_traj"][:, :S])
        assert _same(cut, full, ("duration", "seg", "n_waypoints", "moved"))
    assert np.array_equal(cut["q_traj"][:, 0], paths[:, 0]) and np.all(cut["v_traj"] == 0.0)
    # timing only: the same duration and info apart from the flag (never TRUNCATED)
    timing = s.retime_paths(paths, max_samples=0, **_kw(c))
    assert timing["q_traj"] is None and timing["v_traj"] is None and np.all(timing["flags"] == 0)
    assert _same(timing, cut, ("duration", "seg", "n_samples", "n_waypoints", "moved"))
    s.close()


def test_more_segments_than_one_chunk():
    c = _case("panda7")
    model, T, B, dt = c["model"], 70, 3, 0.1
    paths = TS.make_paths(model, c["q"][:B], TM.SIZE["panda7"], T, np.random.default_rng(1201))
    free = RN.retime(model, paths, c["v_max"], c["a_max"], dt)
    assert np.all(TR.off_integer(free["seg"][:, :, 1] / dt) > 1e-9) and np.all(TR.off_integer(free["duration"] / dt) > 1e-9) and np.all(free["moved"] == T - 1)
    s = _open(c)
    for snap in (False, True):
        S = int(RN.retime(model, paths, c["v_max"], c["a_max"], dt, snap=snap)["n_samples"].max())
        want = RN.retime(model, paths, c["v_max"], c["a_max"], dt, S=S, snap=snap)
        got = s.retime_paths(paths, **_kw(c, dt=dt, snap=snap))
        assert got["q_traj"].shape[1] == S > 64
        _check("panda7", "T = 70 snap" if snap else "T = 70 free", got, want)
    s.close()


# ---- 4. edge cases -----------------------------------------------------------------------------------------------------------------------
def test_edges():
    c = _case("panda7")
    model, paths, B = c["model"], c["paths"], c["B"]
    T, nq = T_PATH, model.nq
    s = _open(c)
    full = s.retime_paths(paths, max_samples=S_ROWS, **_kw(c))
    # n_waypoints of 0, 1, 2, T and T + 1 in one batch
    n = np.array([0, 1, 2, T, T + 1], dtype=np.int32)
    for snap in (False, True):
        got = s.retime_paths(paths[:5], n_waypoints=n, max_samples=S_ROWS, snap=snap, **_kw(c))
        _check("panda7", "counts", got, RN.retime(model, paths[:5], c["v_max"], c["a_max"], DT, n_waypoints=n, S=S_ROWS, snap=snap))
        assert got["flags"].tolist() == [capi.RETIME_SKIPPED] * 2 + [0, 0, capi.RETIME_SKIPPED] and got["n_waypoints"].tolist() == [0, 0, 2, T, 0]
        assert all(np.isnan(got[k][[0, 1, 4]]).all() for k in FLOATS) and np.all(got["seg"][2, 1:] == 0.0)
    got = s.retime_paths(paths[:5], n_waypoints=n, max_samples=S_ROWS, **_kw(c))
    assert _same({k: got[k][3] for k in FLOATS + INTS}, {k: full[k][3] for k in FLOATS + INTS})
    # a NaN waypoint: INVALID, and its neighbours in the batch are untouched; beyond the count it is not read
    bad = paths.copy()
    bad[2, 3, 1] = np.nan
    got = s.retime_paths(bad, max_samples=S_ROWS, **_kw(c))
    others = np.arange(B) != 2
    assert _same({k: got[k][others] for k in FLOATS + INTS}, {k: full[k][others] for k in FLOATS + INTS})
    assert got["flags"][2] == capi.RETIME_INVALID and got["n_samples"][2] == 0 and got["n_waypoints"][2] == T and got["moved"][2] == 0
    assert all(np.isnan(got[k][2]).all() for k in FLOATS)
    cut = s.retime_paths(bad, n_waypoints=np.full(B, 3, dtype=np.int32), max_samples=S_ROWS, **_kw(c))
    assert np.all(cut["flags"] == 0) and np.all(cut["moved"] == 2)
    # repeated waypoints are corners of duration 0: the trajectory of the path without them, bit for bit
    rep = np.ascontiguousarray(np.repeat(paths, 2, axis=1))
    got = s.retime_paths(rep, max_samples=S_ROWS, **_kw(c))
    assert _same(got, full, ("q_traj", "v_traj", "duration", "n_samples", "moved", "flags")) and np.all(got["n_waypoints"] == 2 * T)
    assert np.all(got["seg"][:, 0::2] == 0.0) and np.array_equal(got["seg"][:, 1::2], full["seg"])
    # a padded shortcut result with len == NULL equals the call with its count
    pad = paths.copy()
    pad[:, 3:] = pad[:, 2:3]
    a = s.retime_paths(pad, max_samples=S_ROWS, **_kw(c))
    b = s.retime_paths(pad, n_waypoints=np.full(B, 3, dtype=np.int32), max_samples=S_ROWS, **_kw(c))
    assert _same(a, b, ("q_traj", "v_traj", "duration", "seg", "n_samples", "moved", "flags"))
    assert np.all(a["seg"][:, 2:] == 0.0) and np.all(a["moved"] == 2) and np.all(a["n_waypoints"] == T) and np.all(b["n_waypoints"] == 3)
    # two equal rows: duration 0, one sample
    still = np.ascontiguousarray(np.tile(paths[:, :1], (1, 2, 1)))
    for snap in (False, True):
        got = s.retime_paths(still, max_samples=3, snap=snap, **_kw(c))
        assert np.all(got["duration"] == 0.0) and np.all(got["n_samples"] == 1) and np.all(got["moved"] == 0) and np.all(got["flags"] == 0)
        assert np.array_equal(got["q_traj"], np.tile(paths[:, :1], (1, 3, 1))) and np.all(got["v_traj"] == 0.0) and np.all(got["seg"] == 0.0)
    # B = 0
    none = s.retime_paths(paths[:0], max_samples=4, **_kw(c))
    assert none["q_traj"].shape == (0, 4, nq) and none["duration"].shape == (0,) and none["seg"].shape == (0, T - 1, 4)
    s.close()


def test_q_and_minus_q_of_a_spherical_joint():
    c = _case("multidof20")
    model, paths, B = c["model"], c["paths"], c["B"]
    j = next(i for i in range(1, model.njoints) if int(model.jtype[i]) == 10)     # the spherical joint: (x, y, z, w) at idx_q
    iq = int(model.idx_q[j])
    two = np.ascontiguousarray(paths[:, :2].copy())
    two[:, 1] = two[:, 0]
    two[:, 1, iq:iq + 4] *= -1.0
    s = _open(c)
    for snap in (False, True):
        got = s.retime_paths(two, max_samples=4, snap=snap, **_kw(c))
        # the same rotation: a difference of rounding size, a duration that is 0 or tiny, and both rows as they came
        assert np.all(got["flags"] == 0) and np.all(got["duration"] >= 0.0) and np.all(got["duration"] <= (DT if snap else 1e-6))
        assert np.all(got["n_samples"] <= 2) and np.array_equal(got["q_traj"][:, 0], two[:, 0]) and np.array_equal(got["q_traj"][:, 2:], two[:, 1:].repeat(2, axis=1))
        assert np.all(np.abs(got["v_traj"]) <= c["v_max"])
    # a path through -q: the trajectory of the path through q, up to the sign of the samples on the segment that leaves -q
    thru = paths.copy()
    thru[:, 2, iq:iq + 4] *= -1.0
    a, b = s.retime_paths(paths, max_samples=S_ROWS, **_kw(c)), s.retime_paths(thru, max_samples=S_ROWS, **_kw(c))
    assert np.array_equal(a["n_samples"], b["n_samples"]) and np.allclose(a["duration"], b["duration"], rtol=0, atol=1e-12)
    assert np.allclose(a["v_traj"], b["v_traj"], rtol=0, atol=1e-9)
    qa, qb = a["q_traj"][:, :, iq:iq + 4], b["q_traj"][:, :, iq:iq + 4]
    assert np.all(np.minimum(np.abs(qa - qb).max(axis=2), np.abs(qa + qb).max(axis=2)) <= 1e-9)
    s.close()


# ---- 5. the certificate carries over -----------------------------------------------------------------------------------------------------
def test_a_certified_path_stays_certified():
    c = TS.shortcut_case("panda7")
    model, paths, margin = c["model"], c["paths"], c["margin"]
    v_max, a_max = TR.limits("panda7", model.nv)
    B, T = paths.shape[:2]
    dv = MN.difference(model, paths[:, :-1].reshape(-1, model.nq), paths[:, 1:].reshape(-1, model.nq))
    ref = MN.advance(model, paths[:, :-1].reshape(-1, model.nq), dv, c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], margin=margin, tol=TS.TOL,
                     max_evals=256)
    assert np.all(ref["status"].reshape(B, T - 1) == MN.FREE, axis=1).any()      # on the reference: some path qualifies
    s = TM._open(c)
    chk = s.path_clearance(paths, margin=margin, tol=TS.TOL, max_evals=256)
    free = np.all(chk["status"] == MN.FREE, axis=1)
    assert free.any()
    for snap in (False, True):
        got = s.retime_paths(paths[free], v_max, a_max, DT, snap=snap)
        assert np.all(got["flags"] == 0)
        clear = s.clearance(got["q_traj"].reshape(-1, model.nq))["min"]
        assert np.all(clear >= margin - 1e-9), (clear.min(), margin)
    s.close()


# ---- 6. pointer routes, 8. determinism ---------------------------------------------------------------------------------------------------
def test_determinism_and_pointer_routes():
    c = _case("talos32")
    model, paths, B = c["model"], c["paths"], c["B"]
    T, nq, nv, S = T_PATH, model.nq, model.nv, S_ROWS
    n = np.array([T - b % 3 for b in range(B)], dtype=np.int32)
    s = _open(c)
    for snap in (False, True):
        kw = _kw(c, snap=snap, max_samples=S)
        host = s.retime_paths(paths, n_waypoints=n, **kw)
        assert _same(host, s.retime_paths(paths, n_waypoints=n, **kw))       # the same call twice
        s32 = _open(c, capi.F32)
        assert _same(host, s32.retime_paths(paths, n_waypoints=n, **kw))     # fp64 whatever the handle's precision
        s32.close()
        dq, dn = capi.DeviceArray(paths), TS._device_i32(n)
        assert _same(host, s.retime_paths(dq, n_waypoints=dn, **kw))         # device in, host out
        for a, l in ((paths, n), (dq, dn)):                                  # host in and device in, device out
            bufs = (capi.DeviceArray(np.full(B * S * nq, -1.0)), capi.DeviceArray(np.full(B * S * nv, -1.0)), capi.DeviceArray(np.full(B * (T - 1) * 4, -1.0)),
                    capi.DeviceArray(np.full(B, -1.0)), TS._device_i32(np.zeros(4 * B)))
            s.retime_paths(a, n_waypoints=l, out=bufs, **kw)
            got = capi.BatchedLoik._retime_result(TS._back(bufs[0], (B, S, nq), np.float64), TS._back(bufs[1], (B, S, nv), np.float64),
                                                  TS._back(bufs[2], (B, T - 1, 4), np.float64), TS._back(bufs[3], (B,), np.float64),
                                                  TS._back(bufs[4], (B, 4), np.int32))
            assert _same(host, got)
            # without velocities and records; then timing only
            s.retime_paths(a, n_waypoints=l, out=(bufs[0], None, None, bufs[3], bufs[4]), **kw)
            assert np.array_equal(TS._back(bufs[0], (B, S, nq), np.float64), host["q_traj"])
            s.retime_paths(a, n_waypoints=l, out=(None, None, None, bufs[3], bufs[4]), **kw)
            assert np.array_equal(TS._back(bufs[3], (B,), np.float64), host["duration"])
            assert np.array_equal(TS._back(bufs[4], (B, 4), np.int32)[:, 0], host["n_samples"])
            for d in bufs:
                d.free()
        dq.free(); dn.free()
        # the contents of the other paths do not reach path b
        other = paths[::-1].copy()
        other[5] = paths[5]
        got = s.retime_paths(other, n_waypoints=n, **kw)
        assert _same({k: host[k][5] for k in FLOATS + INTS}, {k: got[k][5] for k in FLOATS + INTS})
    s.close()


# ---- 7. neutrality -----------------------------------------------------------------------------------------------------------------------
def test_the_call_changes_no_solve_and_no_resident_q():
    c = _case("talos32")
    model, paths = c["model"], c["paths"]
    qa = c["q"]
    links = TC._links(model, 1)
    tg = P.fk12(model, np.clip(qa + 0.05, model.q_lo, model.q_hi), links)
    res = []
    for with_calls in (False, True):
        s, _ = TC._handle(model, c["n"], links, qa)

        def calls():
            if with_calls:
                s.retime_paths(paths, **_kw(c))
                s.retime_paths(paths, snap=True, max_samples=7, **_kw(c))
        q0 = s.get("q")
        calls()
        assert np.array_equal(q0, s.get("q"))
        s.Solve()
        out = [s.get("z"), s.get("iter")]
        calls()
        out += [s.get("z"), s.get("iter"), s.get("q")]
        p = s.SolvePose(tg, tol_pose=1e-4, max_steps=6)
        calls()
        out += [s.get("q"), p["status"], p["err"]]
        res.append(out)
        s.close()
    assert all(np.array_equal(a, b) for a, b in zip(*res))


# ---- 9. validation -----------------------------------------------------------------------------------------------------------------------
def test_errors():
    c = _case("panda7")
    model, paths = c["model"], c["paths"]
    B, T, nq = paths.shape
    nv, S = model.nv, 8
    s = _open(c)
    L, h, vp = s.L, s.h, C.c_void_p
    ptr = lambda a: a.ctypes.data_as(vp)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    outs = [np.full((B, S, nq), -7.0), np.full((B, S, nv), -7.0), np.full((B, T - 1, 4), -7.0), np.full(B, -7.0), np.full((B, 4), -7, dtype=np.int32)]
    vm, am = np.ascontiguousarray(c["v_max"]), np.ascontiguousarray(c["a_max"])
    good = capi.RetimeParams(DT, 0)
    untouched = lambda: all(np.all(o == -7) for o in outs)

    def call(prm=good, q_=ptr(paths), B_=B, T_=T, vm_=dp(vm), am_=dp(am), S_=S, traj_=ptr(outs[0]), vel_=ptr(outs[1]), seg_=ptr(outs[2]),
             dur_=ptr(outs[3]), info_=ptr(outs[4]), h_=h):
        return L.loikb_retime_paths(h_, q_, None, B_, T_, 0, vm_, am_, C.byref(prm) if prm is not None else None, S_, traj_, vel_, seg_, dur_, info_, 0)

    def spoiled(a, j, x):
        a = a.copy()
        a[j] = x
        return a
    P_ = capi.RetimeParams
    cases = [(dict(prm=P_(np.nan, 0)), b"dt"), (dict(prm=P_(np.inf, 0)), b"dt"), (dict(prm=P_(0.0, 0)), b"dt"), (dict(prm=P_(-DT, 0)), b"dt"),
             (dict(prm=P_(DT, 2)), b"flags"), (dict(prm=P_(DT, -1)), b"flags"), (dict(prm=None), b"p == NULL"),
             (dict(vm_=None), b"v_max"), (dict(am_=None), b"a_max"), (dict(dur_=None), b"out_duration"), (dict(info_=None), b"out_info"),
             (dict(S_=0), b"S < 1"), (dict(S_=-3), b"S < 1"), (dict(traj_=None), b"out_vel without out_traj")]
    keep = []
    for j, x in ((0, np.nan), (nv - 1, np.inf), (2, 0.0), (3, -1.0)):
        keep += [spoiled(vm, j, x), spoiled(am, j, x)]
        cases += [(dict(vm_=dp(keep[-2])), b"v_max"), (dict(am_=dp(keep[-1])), b"a_max")]
    for kw, text in cases:
        assert call(**kw) == ERR_ARG and text in L.loikb_last_error(), (text, L.loikb_last_error())
        assert call(**dict(kw, B_=0)) == ERR_ARG       # the arguments are checked before anything else
    assert call(h_=None) == ERR_ARG
    assert call(q_=None) == ERR_ARG and b"q_path" in L.loikb_last_error() and call(B_=-1) == ERR_ARG and b"B >= 0" in L.loikb_last_error()
    assert call(T_=1) == ERR_ARG and b"T >= 2" in L.loikb_last_error() and call(T_=1, B_=0) == ERR_ARG
    assert call(B_=1 << 20, T_=1 << 11) == ERR_ARG and b"2^31" in L.loikb_last_error()
    assert call(B_=1 << 20, S_=1 << 11) == ERR_ARG and b"B * S < 2^31" in L.loikb_last_error()
    assert call(traj_=ptr(paths)) == ERR_ARG and b"out_traj == q_path" in L.loikb_last_error()
    assert untouched()
    assert call(B_=0, q_=None) == 0 and untouched()
    # what is allowed: no velocities, no records, timing only (S is then ignored)
    assert call(vel_=None, seg_=None) == 0 and np.all(outs[1] == -7.0) and np.all(outs[2] == -7.0) and np.all(outs[3] > 0.0)
    outs[0][:] = -7.0; outs[3][:] = -7.0
    assert call(traj_=None, vel_=None, S_=-5) == 0 and np.all(outs[0] == -7.0) and np.all(outs[3] > 0.0) and np.all(outs[4][:, 3] == 0)
    assert call(prm=P_(DT, capi.RETIME_SNAP)) == 0 and np.all(outs[4][:, 3] == capi.RETIME_TRUNCATED)
    s.close()
