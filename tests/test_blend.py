"""GPU: the certified blends of include/loik_amd_blend.h against the numpy reference of tests/blend_numpy.py (proven on the CPU by
test_blend_numpy.py, which also fixes the inputs): the eight robots of test_clearance.ROBOTS (tree330 with its records and tables in the
global slab), more corners than one chunk of lanes, the certificate checked independently with clearance(), the reduction to
retime_paths, the durations, the pointer routes, neutrality towards the solves, determinism and the validation."""
import ctypes as C

import numpy as np
import pytest

import loik_amd
from loik_amd import capi

import blend_numpy as BN
import motion_numpy as MN
import pose_numpy as P
import retime_numpy as RN
import test_blend_numpy as TB
import test_clearance as TC
import test_motion_clearance as TM
import test_retime_numpy as TR
import test_shortcut as TS

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -20, -24
T_PATH, DT, S_ROWS = TB.T_PATH, TB.DT, TB.S_ROWS
FLOATS = ("duration", "corner", "piece", "q_traj", "v_traj")
INTS = ("n_samples", "n_waypoints", "taken", "flags", "corner_info")
# max |got - numpy| / (1 + |numpy|) over duration, corner, piece, q_traj and v_traj: 16 times the largest error measured on one MI355X over
# the eight robots of test 6 and the paths of test 7 (profiles/blend_measured.md), the allowance for another compiler's rounding, as
# RETIME_BOUND of test_retime.py and LENGTH_BOUND of test_shortcut.py were set
BLEND_MEASURED = 1.325e-13   # (multidof13, q_traj; multidof20 1.26e-13 -- the two robots with free-flyer, spherical or planar joints, as in RETIME_MEASURED; the six others 1.6e-16 .. 3.2e-15)
BLEND_BOUND = 16 * BLEND_MEASURED


def _case(name):
    return TB.blend_case(name)


def _open(c, precision=capi.F64):
    return TM._open(c, precision)


def _kw(c, **over):
    return dict(dict(v_max=c["v_max"], a_max=c["a_max"], **c["kw"]), **over)


def _error(got, want):
    """|got - want| / (1 + |want|), the largest of each float output; NaN where the reference has NaN"""
    err = {}
    for k in FLOATS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), k
        assert np.array_equal(np.isinf(g), np.isinf(w)) and np.array_equal(g[np.isinf(w)], w[np.isinf(w)]), k
        ok = np.isfinite(w)
        err[k] = float(np.max(np.abs(g[ok] - w[ok]) / (1.0 + np.abs(w[ok])), initial=0.0))
    return err


def _check(name, what, got, want):
    for k in INTS:
        assert np.array_equal(got[k], want[k]), (name, what, k, got[k], want[k])
    each = _error(got, want)
    err = max(each.values())
    print("blend_measured %s %s: max |got - numpy| / (1 + |numpy|) %.3e (%s)" % (name, what, err, ", ".join("%s %.1e" % kv for kv in each.items())))
    assert err <= BLEND_BOUND, (name, what, each)
    return err


def _same(a, b, keys=FLOATS + INTS):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _rows(r, rows, keys=FLOATS + INTS):
    return {k: r[k][rows] for k in keys}


# ---- 6. against numpy on eight robots ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.ROBOTS))
def test_blend_matches_numpy(name):
    c = _case(name)
    model, paths, want = c["model"], c["paths"], c["want"]
    TB.check_comparable(want)      # (what makes the integers comparable; test_blend_numpy.py checks it on the CPU too)
    print("blend_measured %s: %s" % (name, TB.coverage(want)))
    ns, ncar, nb = len(c["links"]), len(set(int(l) for l in c["links"])), model.nv
    need = (4 * ns + ns + 12 * nb + 12 * ncar + 2 * nb + 3 * (T_PATH - 1) + 5 * (T_PATH - 2) + 8 * (2 * T_PATH - 3) + (T_PATH - 1) * nb) * 8
    if name == "tree330":
        assert need > 65536          # the records and the tables of a wavefront do not fit the LDS: the slab instantiation
    else:
        assert need <= 65536 - 8192  # ... and here they do, beside whatever the compiler keeps for itself
    s = _open(c)
    got = s.blend_paths(paths, max_samples=S_ROWS, **_kw(c))
    _check(name, "T = 6", got, want)
    s.close()


# ---- 7. more corners than one chunk of lanes, counts shorter than T ---------------------------------------------------------------------
def test_more_corners_than_one_chunk():
    c = _case("panda7")
    model, T, B, dt = c["model"], 70, 3, 0.1
    paths = TS.make_paths(model, c["q"][:B], TM.SIZE["panda7"], T, np.random.default_rng(1301))
    n = np.array([T, T - 3, 67], dtype=np.int32)
    paths[1, T - 3:] = np.nan
    paths[2, 67:] = np.nan
    kw = dict(c["kw"], dt=dt, max_evals=12, max_tries=2)
    args = (c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], c["v_max"], c["a_max"])
    S = int(BN.blend(model, paths, *args, n_waypoints=n, **kw)["n_samples"].max())
    want = BN.blend(model, paths, *args, n_waypoints=n, S=S, **kw)
    assert not want["near"].any() and np.all(TR.off_integer(want["duration"] / dt) > 1e-9) and np.all(want["flags"] == 0)
    st = TB.statuses(want)
    assert np.sum(st[0] == BN.TAKEN) > 0 and np.sum(st[0] != BN.TAKEN) > 0 and np.all(st[1, T - 5:] == BN.OFF) and np.all(st[2, 65:] == BN.OFF)
    s = _open(c)
    got = s.blend_paths(paths, n_waypoints=n, v_max=c["v_max"], a_max=c["a_max"], **kw)
    assert got["q_traj"].shape[1] == S > 64
    _check("panda7", "T = 70", got, want)
    # without the counts the NaN rows are waypoints: INVALID, and path 0 as before
    bad = s.blend_paths(paths, max_samples=S, v_max=c["v_max"], a_max=c["a_max"], **kw)
    assert bad["flags"].tolist() == [0, capi.BLEND_INVALID, capi.BLEND_INVALID] and _same(_rows(bad, [0]), _rows(got, [0]))
    s.close()


# ---- 8. the certificate, independently --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["panda7", "multidof13"])
def test_every_blend_taken_is_clear(name):
    c = _case(name)
    model, paths, margin = c["model"], c["paths"], c["margin"]
    s = _open(c)
    got = s.blend_paths(paths, max_samples=S_ROWS, **_kw(c))
    uu = np.linspace(0.0, 1.0, 257)
    seen = 0
    for b in range(c["B"]):
        dv = BN.differences(model, paths[b])
        for k in range(1, T_PATH - 1):
            l, ri, ro, w, m = got["corner"][b, k - 1]
            if got["corner_info"][b, k - 1, 0] != capi.BLEND_TAKEN:
                continue
            seen += 1
            assert 0.0 < l <= c["kw"]["reach"] and m >= margin + TB.TOL
            P0, P2 = -ri * dv[k - 1], ro * dv[k]
            q = np.stack([BN.curve_point(model, paths[b, k], P0, P2, u) for u in uu])
            clear = s.clearance(q)["min"]
            assert np.all(clear >= margin), (name, b, k, float(clear.min()), margin)
            # the curve leaves the incoming leg at 1 - r_in and joins the outgoing leg at r_out
            gap = MN.difference(model, np.stack([q[0], q[-1]]), np.stack([P.integrate(model, paths[b, k - 1], (1.0 - ri) * dv[k - 1]), P.integrate(model, paths[b, k], ro * dv[k])]))
            assert np.max(np.abs(gap)) <= 1e-12
    assert seen > 0
    # ... and so is every sample of the trajectory that lies on a blend
    for b in range(c["B"]):
        for p in range(1, 2 * T_PATH - 3, 2):
            t0, D = got["piece"][b, p, :2]
            if D > 0.0:
                i0, i1 = int(np.ceil(t0 / DT)), int(np.floor((t0 + D) / DT))
                if i1 >= i0:
                    assert np.all(s.clearance(got["q_traj"][b, i0:i1 + 1])["min"] >= margin - 1e-9)
    s.close()


# ---- 9. reduction on the device, 10. the durations ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TB.SIX))
def test_no_tries_is_retime_and_blends_are_not_slower(name):
    c = _case(name)
    model, paths = c["model"], c["paths"]
    s = _open(c)
    ref = s.retime_paths(paths, c["v_max"], c["a_max"], DT, max_samples=S_ROWS)
    off = s.blend_paths(paths, max_samples=S_ROWS, **_kw(c, max_tries=0))
    assert np.all(off["corner_info"][:, :, 0] == capi.BLEND_OFF) and np.all(off["corner_info"][:, :, 1:3] == 0) and np.all(off["corner"] == 0.0)
    assert np.array_equal(off["n_samples"], ref["n_samples"]) and np.array_equal(off["flags"], ref["flags"]) and np.all(off["taken"] == 0)
    err = max(float(np.max(np.abs(off[k] - ref[k]) / (1.0 + np.abs(ref[k])))) for k in ("duration", "q_traj", "v_traj"))
    print("blend_measured %s reduction: max |blend - retime| / (1 + |retime|) %.3e" % (name, err))
    assert err <= BLEND_BOUND, (name, err)
    got = s.blend_paths(paths, max_samples=S_ROWS, **_kw(c))
    some = got["taken"] > 0
    assert some.any() and np.all(got["duration"][some] <= ref["duration"][some]), (name, got["duration"], ref["duration"])
    assert np.array_equal(got["duration"][~some], off["duration"][~some])
    print("blend_measured %s duration: blend / retime %s" % (name, np.round(got["duration"] / ref["duration"], 3).tolist()))
    TR.check_limits(got, c["v_max"], c["a_max"], DT)
    s.close()


# ---- 11. pointer routes, determinism, neutrality, validation -------------------------------------------------------------------------------
def _bufs(B, T, S, nq, nv):
    return (capi.DeviceArray(np.full(B * S * nq, -1.0)), capi.DeviceArray(np.full(B * S * nv, -1.0)), capi.DeviceArray(np.full(B, -1.0)),
            TS._device_i32(np.zeros(4 * B)), capi.DeviceArray(np.full(B * (T - 2) * 5, -1.0)), TS._device_i32(np.zeros(B * (T - 2) * 6)),
            capi.DeviceArray(np.full(B * (2 * T - 3) * 4, -1.0)))


def _result(bufs, B, T, S, nq, nv):
    return capi.BatchedLoik._blend_result(TS._back(bufs[0], (B, S, nq), np.float64), TS._back(bufs[1], (B, S, nv), np.float64),
                                          TS._back(bufs[2], (B,), np.float64), TS._back(bufs[3], (B, 4), np.int32),
                                          TS._back(bufs[4], (B, T - 2, 5), np.float64), TS._back(bufs[5], (B, T - 2, 6), np.int32),
                                          TS._back(bufs[6], (B, 2 * T - 3, 4), np.float64))


def test_determinism_and_pointer_routes():
    c = _case("multidof13")
    model, paths, B = c["model"], c["paths"], c["B"]
    T, nq, nv, S = T_PATH, model.nq, model.nv, S_ROWS
    n = np.array([T - b % 3 for b in range(B)], dtype=np.int32)
    s = _open(c)
    kw = _kw(c, max_samples=S)
    host = s.blend_paths(paths, n_waypoints=n, **kw)
    assert (host["taken"] > 0).any()
    assert _same(host, s.blend_paths(paths, n_waypoints=n, **kw))       # the same call twice
    s32 = _open(c, capi.F32)
    assert _same(host, s32.blend_paths(paths, n_waypoints=n, **kw))     # fp64 whatever the handle's precision
    s32.close()
    dq, dn = capi.DeviceArray(paths), TS._device_i32(n)
    assert _same(host, s.blend_paths(dq, n_waypoints=dn, **kw))         # device in, host out
    for a, l in ((paths, n), (dq, dn)):                                 # host in and device in, device out
        bufs = _bufs(B, T, S, nq, nv)
        s.blend_paths(a, n_waypoints=l, out=bufs, **kw)
        assert _same(host, _result(bufs, B, T, S, nq, nv))
        # without velocities and tables; then timing only
        s.blend_paths(a, n_waypoints=l, out=(bufs[0], None, bufs[2], bufs[3], None, None, None), **kw)
        assert np.array_equal(TS._back(bufs[0], (B, S, nq), np.float64), host["q_traj"])
        s.blend_paths(a, n_waypoints=l, out=(None, None, bufs[2], bufs[3], None, None, None), **kw)
        assert np.array_equal(TS._back(bufs[2], (B,), np.float64), host["duration"])
        assert np.array_equal(TS._back(bufs[3], (B, 4), np.int32)[:, 0], host["n_samples"])
        for d in bufs:
            d.free()
    dq.free(); dn.free()
    # an INVALID and a SKIPPED path leave their neighbours untouched; the contents of the other paths do not reach path b
    full = s.blend_paths(paths, **kw)
    bad = paths.copy()
    bad[1, 3, 1] = np.nan
    m = np.array([T, T, T, T + 1, T], dtype=np.int32)
    got = s.blend_paths(bad, n_waypoints=m, **kw)
    assert got["flags"].tolist() == [0, capi.BLEND_INVALID, 0, capi.BLEND_SKIPPED, 0] and got["n_waypoints"].tolist() == [T, T, T, 0, T]
    assert _same(_rows(got, [0, 2, 4]), _rows(full, [0, 2, 4]))
    assert all(np.isnan(got[k][[1, 3]]).all() for k in FLOATS) and np.all(got["n_samples"][[1, 3]] == 0) and np.all(got["taken"][[1, 3]] == 0)
    assert np.all(got["corner_info"][[1, 3], :, 0] == capi.BLEND_OFF) and np.all(got["corner_info"][[1, 3], :, 1:3] == 0)
    other = paths[::-1].copy()
    other[2] = paths[2]
    assert _same(_rows(s.blend_paths(other, **kw), [2]), _rows(full, [2]))
    # a timing-only call, and one sized by the call itself
    timing = s.blend_paths(paths, **_kw(c, max_samples=0))
    assert timing["q_traj"] is None and _same(timing, full, ("duration", "corner", "piece") + INTS)
    auto = s.blend_paths(paths, **_kw(c))
    Smax = int(full["n_samples"].max())
    assert auto["q_traj"].shape == (B, Smax, nq) and np.array_equal(auto["q_traj"], full["q_traj"][:, :Smax]) and np.all(auto["flags"] == 0)
    cut = s.blend_paths(paths, **_kw(c, max_samples=50))
    assert np.all(cut["flags"] == capi.BLEND_TRUNCATED) and np.array_equal(cut["q_traj"], full["q_traj"][:, :50]) and np.array_equal(cut["v_traj"], full["v_traj"][:, :50])
    s.close()


def test_the_call_changes_no_solve_and_no_resident_q():
    c = _case("talos32")
    model, paths = c["model"], c["paths"]
    qa = c["q"]
    links = TC._links(model, 1)
    tg = P.fk12(model, np.clip(qa + 0.05, model.q_lo, model.q_hi), links)
    res = []
    for with_calls in (False, True):
        s, _ = TC._handle(model, c["n"], links, qa)
        s.set_collision_spheres(c["links"], c["spheres"])
        s.set_collision_world(c["ws"], c["wb"])
        s.set_self_collision(True)

        def calls():
            if with_calls:
                s.blend_paths(paths, **_kw(c))
                s.blend_paths(paths, **_kw(c, max_samples=7, max_tries=1))
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


def test_errors():
    c = _case("panda7")
    model, paths = c["model"], c["paths"]
    B, T, nq = paths.shape
    nv, S = model.nv, 8
    s = _open(c)
    L, h, vp = s.L, s.h, C.c_void_p
    ptr = lambda a: a.ctypes.data_as(vp)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    outs = [np.full((B, S, nq), -7.0), np.full((B, S, nv), -7.0), np.full(B, -7.0), np.full((B, 4), -7, dtype=np.int32), np.full((B, T - 2, 5), -7.0),
            np.full((B, T - 2, 6), -7, dtype=np.int32), np.full((B, 2 * T - 3, 4), -7.0)]
    vm, am = np.ascontiguousarray(c["v_max"]), np.ascontiguousarray(c["a_max"])
    k = c["kw"]

    def P_(margin=k["margin"], tol=k["tol"], reach=k["reach"], dt=DT, max_evals=k["max_evals"], max_tries=k["max_tries"], flags=0):
        return capi.BlendParams(margin, tol, reach, dt, max_evals, max_tries, flags)
    good = P_()
    untouched = lambda: all(np.all(o == -7) for o in outs)

    def call(prm=good, q_=ptr(paths), B_=B, T_=T, vm_=dp(vm), am_=dp(am), S_=S, traj_=ptr(outs[0]), vel_=ptr(outs[1]), dur_=ptr(outs[2]),
             info_=ptr(outs[3]), cor_=ptr(outs[4]), cinfo_=ptr(outs[5]), piece_=ptr(outs[6]), h_=h):
        return L.loikb_blend_paths(h_, q_, None, B_, T_, 0, vm_, am_, C.byref(prm) if prm is not None else None, S_, traj_, vel_, dur_, info_, cor_,
                                   cinfo_, piece_, 0)

    def spoiled(a, j, x):
        a = a.copy()
        a[j] = x
        return a
    cases = [(dict(prm=P_(dt=x)), b"dt") for x in (np.nan, np.inf, 0.0, -DT)] + [(dict(prm=P_(reach=x)), b"reach") for x in (np.nan, np.inf, 0.0, -1.0)]
    cases += [(dict(prm=P_(margin=np.nan)), b"margin"), (dict(prm=P_(margin=np.inf)), b"margin"), (dict(prm=P_(tol=np.nan)), b"tol"),
              (dict(prm=P_(tol=1e-10)), b"tol"), (dict(prm=P_(max_evals=0)), b"max_evals"), (dict(prm=P_(max_evals=65537)), b"max_evals"),
              (dict(prm=P_(max_tries=-1)), b"max_tries"), (dict(prm=P_(max_tries=17)), b"max_tries"), (dict(prm=P_(flags=1)), b"flags"),
              (dict(prm=None), b"p == NULL"), (dict(vm_=None), b"v_max"), (dict(am_=None), b"a_max"), (dict(dur_=None), b"out_duration"),
              (dict(info_=None), b"out_info"), (dict(S_=0), b"S < 1"), (dict(S_=-3), b"S < 1"), (dict(traj_=None), b"out_vel without out_traj")]
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
    assert call(B_=1, T_=1 << 30) == ERR_ARG and b"T < 2^30" in L.loikb_last_error() and call(B_=0, T_=1 << 30) == ERR_ARG
    assert call(B_=1 << 20, S_=1 << 11) == ERR_ARG and b"B * S < 2^31" in L.loikb_last_error()
    assert call(traj_=ptr(paths)) == ERR_ARG and b"out_traj == q_path" in L.loikb_last_error()
    assert untouched()
    # the state: a handle without spheres, after the arguments
    bare = TC._open(model, c["q"])
    assert call(h_=bare.h) == ERR_STATE and b"no spheres" in bare.L.loikb_last_error() and call(h_=bare.h, B_=0) == ERR_STATE
    assert call(h_=bare.h, prm=P_(dt=0.0)) == ERR_ARG and untouched()
    bare.close()
    assert call(B_=0, q_=None) == 0 and untouched()
    # what is allowed: no velocities, no tables, timing only (S is then ignored), max_tries = 0
    assert call(vel_=None, cor_=None, cinfo_=None, piece_=None) == 0 and all(np.all(outs[i] == -7) for i in (1, 4, 5, 6)) and np.all(outs[2] > 0.0)
    outs[0][:] = -7.0; outs[2][:] = -7.0
    assert call(traj_=None, vel_=None, S_=-5) == 0 and np.all(outs[0] == -7.0) and np.all(outs[2] > 0.0) and np.all(outs[3][:, 3] == 0)
    assert call(prm=P_(max_tries=0)) == 0 and np.all(outs[5][:, :, 0] == capi.BLEND_OFF) and np.all(outs[3][:, 3] == capi.BLEND_TRUNCATED)
    s.close()
