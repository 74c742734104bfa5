"""GPU: the motion checks of include/loik_amd_motion.h against the numpy reference of tests/motion_numpy.py (proven on the CPU by
test_motion_numpy.py): the eight robots, spheres and world of test_clearance._case (tree330 takes its records from the global slab;
composite20's links are several device joints each), the three outcomes, a sphere on a universal joint alone, the edge cases, the pointer routes, neutrality towards the solves, the validation, and difference on every robot."""
import ctypes as C

import numpy as np
import pytest

import loik_amd
from loik_amd import capi

import clearance_numpy as CN
import motion_numpy as MN
import pose_numpy as P
import qp_cases as QC
import test_clearance as TC

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -20, -24
BOUND = TC.BOUND          # |min_sampled - oracle| <= BOUND * scale, scale = 1 + max |centre| + max r: the bound of test_clearance.py
# |s_free - oracle| and |s_at_min - oracle|: 16 times the largest error measured on one MI355X over the six robots (multidof20, whose
# quaternion joints the reference normalises exactly and the device to first order; the others stay below 5e-15:
# profiles/motion_measured.md), the allowance for another compiler's rounding.  The bound stands as it was set then: composite20 and
# multidof13, added later, measure 3.1e-15 and 8.7e-13 (a free-flyer root again), inside it
S_FREE_MEASURED = 1.292e-13
S_BOUND = 16 * S_FREE_MEASURED
TOL, MAX_EVALS = 1e-3, 12
# dv = SIZE * uniform(-1, 1) per DoF: small enough that some segments end FREE within MAX_EVALS samples, large enough that some hit
# something on the way and some run out of samples
SIZE = {"panda7": 0.3, "talos32": 0.08, "multidof20": 0.1, "helical24": 0.1, "tree170": 0.02, "tree330": 0.01,
        "composite20": 0.03, "multidof13": 0.1}

_CASES = {}


def motion_case(name):
    """the model, spheres, world and pairs of test_clearance._case, its q as the start of one segment each, and the numpy answer: computed
    once.  The margin is the 40 % quantile of the oracle's clearance at the starts: the dense world of that case leaves few configurations
    clear of everything, and a margin below zero is as good a threshold as any"""
    if name not in _CASES:
        c = dict(TC._case(name))
        rng = np.random.default_rng(800 + list(TC.ROBOTS).index(name))
        c["qa"] = c["q"]
        c["dv"] = SIZE[name] * rng.uniform(-1.0, 1.0, size=(c["n"], c["model"].nv))
        c["margin"] = float(np.quantile(c["want"]["min"], 0.4))
        c["want"] = MN.advance(c["model"], c["qa"], c["dv"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], margin=c["margin"], tol=TOL,
                               max_evals=MAX_EVALS)
        ends = np.stack([MN.interpolate(c["model"], c["qa"][i], c["dv"][i], 1.0) for i in range(c["n"])])
        cen = np.concatenate([MN.centres(c["model"], c["qa"], c["links"], c["spheres"]), MN.centres(c["model"], ends, c["links"], c["spheres"])])
        c["scale"] = 1.0 + float(np.max(np.abs(cen))) + float(np.max(c["spheres"][:, 3]))
        _CASES[name] = c
    return _CASES[name]


def _open(c, precision=capi.F64, q=None):
    s = TC._open(c["model"], c["q"] if q is None else q, precision)
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    return s


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def _compare(got, want, scale, what, rows=None):
    """status, evals and witness equal, min_sampled within BOUND * scale, s_free and s_at_min within S_BOUND, on the segments none of whose
    reference decisions lay within 1e-9 of its threshold (at most 2 %).  Returns (largest s error, largest min_sampled error / scale)"""
    rows = np.arange(want["status"].size) if rows is None else np.asarray(rows)
    near = want["near"][rows]
    assert near.sum() <= 0.02 * rows.size, (what, int(near.sum()))
    keep = rows[~near]
    for k in ("status", "evals", "witness"):
        assert np.array_equal(got[k][~near], want[k][keep]), (what, k)
    bad = want["status"][keep] == MN.INVALID
    assert all(np.isnan(got[k][~near][bad]).all() for k in ("s_free", "min_sampled", "s_at_min"))
    g, w = got["min_sampled"][~near][~bad], want["min_sampled"][keep][~bad]
    inf = np.isposinf(w)
    assert np.array_equal(np.isposinf(g), inf)
    e_min = float(np.max(np.abs(g[~inf] - w[~inf]))) if (~inf).any() else 0.0
    e_s = max(float(np.max(np.abs(got[k][~near][~bad] - want[k][keep][~bad]), initial=0.0)) for k in ("s_free", "s_at_min"))
    print("motion_measured %s: max |s - oracle| %.3e, max |min_sampled - oracle| %.3e, scale %.3f, relative %.3e" % (what, e_s, e_min, scale, e_min / scale))
    assert e_min <= BOUND * scale, (what, e_min, scale)
    assert e_s <= S_BOUND, (what, e_s)
    return e_s, e_min / scale


# ---- 1. against numpy on eight robots ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.ROBOTS))
def test_motion_clearance_matches_numpy(name):
    c = motion_case(name)
    want = c["want"]
    count = [int((want["status"] == st).sum()) for st in range(4)]
    print("motion_measured %s outcomes free / blocked / undecided %s, evals median %d largest %d" % (name, count[:3], np.median(want["evals"]), want["evals"].max()))
    if name not in TC.BIG_TREES:
        assert min(count[:3]) > 0, count
    s = _open(c)
    got = s.motion_clearance(c["qa"], dv=c["dv"], margin=c["margin"], tol=TOL, max_evals=MAX_EVALS)
    _compare(got, want, c["scale"], name)
    assert _same(got, s.motion_clearance(c["qa"], dv=c["dv"], margin=c["margin"], tol=TOL, max_evals=MAX_EVALS))
    # fp64 from fp64 inputs whatever the handle's precision
    s32 = _open(c, capi.F32)
    assert _same(got, s32.motion_clearance(c["qa"], dv=c["dv"], margin=c["margin"], tol=TOL, max_evals=MAX_EVALS))
    # the end point given instead of dv: the device's own difference
    qb = np.stack([MN.interpolate(c["model"], c["qa"][i], c["dv"][i], 1.0) for i in range(c["n"])])
    via = s.motion_clearance(c["qa"], qb=qb, margin=c["margin"], tol=TOL, max_evals=MAX_EVALS)
    assert np.mean(via["status"] == got["status"]) >= 0.9
    s.close(); s32.close()


@pytest.mark.parametrize("name", list(TC.ROBOTS))
def test_difference_matches_numpy(name):
    c = motion_case(name)
    model = c["model"]
    rng = np.random.default_rng(820 + list(TC.ROBOTS).index(name))
    q1 = model.random_configurations(rng, c["n"])
    want = MN.difference(model, c["q"], q1)
    s = _open(c)
    got = s.difference(c["q"], q1)
    scale = 1.0 + float(np.max(np.abs(want)))
    err = float(np.max(np.abs(got - want)))
    print("motion_measured difference %s: max |got - oracle| %.3e, scale %.3f" % (name, err, scale))
    assert got.shape == (c["n"], model.nv) and err <= 1e-13 * scale
    # q0 (+) v = q1 on the device's own integrator is test_motion_numpy's claim for the reference; here: a NaN row is NaN alone
    qb = q1.copy()
    qb[c["n"] - 1, 0] = np.inf
    bad = s.difference(c["q"], qb)
    assert np.isnan(bad[-1]).all() and np.array_equal(bad[:-1], got[:-1])
    assert s.difference(c["q"][:0], q1[:0]).shape == (0, model.nv)
    s.close()


def universal_case():
    """composite20 with one sphere on link 1 alone, the universal joint that hangs on the universe, against the world of its _case.  The
    bound of the reference takes the joint as two revolutes with their placements: Lambda = |d0| (|c| + |p_1|) + |d1| |c| with p_1 the
    placement of the second revolute inside the composite, and nothing else of dv counts.  The sphere sits 0.3 from the link's frame
    so that the angular travel dominates Lambda: a bound that took the joint for one revolute, or left |p_1| out, steps differently"""
    if "universal" not in _CASES:
        c = dict(TC._case("composite20"))
        model = c["model"]
        assert [int(st) for st, _, _ in model.composite[1]] == [P.J_RU, P.J_RU] and int(model.parents[1]) == 0
        rng = np.random.default_rng(840)
        c["links"], c["spheres"], c["pairs"] = np.array([1], dtype=np.int32), np.array([[0.2, -0.1, 0.2, 0.05]]), []
        c["qa"] = c["q"]
        c["dv"] = 0.8 * rng.uniform(-1.0, 1.0, size=(c["n"], model.nv))
        at = CN.clearance(model, c["q"], c["links"], c["spheres"], c["ws"], c["wb"])["min"]
        c["margin"] = float(np.quantile(at, 0.4))
        c["want"] = MN.advance(model, c["qa"], c["dv"], c["links"], c["spheres"], c["ws"], c["wb"], margin=c["margin"], tol=TOL, max_evals=MAX_EVALS)
        ends = np.stack([MN.interpolate(model, c["qa"][i], c["dv"][i], 1.0) for i in range(c["n"])])
        cen = np.concatenate([MN.centres(model, c["qa"], c["links"], c["spheres"]), MN.centres(model, ends, c["links"], c["spheres"])])
        c["scale"] = 1.0 + float(np.max(np.abs(cen))) + 0.05
        _CASES["universal"] = c
    return _CASES["universal"]


def test_a_sphere_on_the_universal_joint_alone():
    """Lambda of the device is not exposed: evals, s_free and status show it"""
    c = universal_case()
    model, want = c["model"], c["want"]
    p1 = float(np.linalg.norm(np.asarray(model.composite[1][1][2], dtype=float)[9:12]))
    reach = float(np.linalg.norm(c["spheres"][0, :3]))
    assert p1 > 0.1 and np.allclose(want["Lambda"][:, 0], np.abs(c["dv"][:, 0]) * (reach + p1) + np.abs(c["dv"][:, 1]) * reach, rtol=1e-14, atol=0)
    assert want["evals"].max() > 4
    s = TC._open(model, c["q"])
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    got = s.motion_clearance(c["qa"], dv=c["dv"], margin=c["margin"], tol=TOL, max_evals=MAX_EVALS)
    _compare(got, want, c["scale"], "composite20 with a sphere on the universal joint alone")
    # the rest of dv moves nothing that the sphere sees
    dv = np.zeros_like(c["dv"])
    dv[:, :2] = c["dv"][:, :2]
    assert _same(got, s.motion_clearance(c["qa"], dv=dv, margin=c["margin"], tol=TOL, max_evals=MAX_EVALS))
    s.close()


# ---- 2. the edge cases --------------------------------------------------------------------------------------------------------------------
def test_edges():
    c = motion_case("panda7")
    model, qa, dv, n = c["model"], c["qa"], c["dv"], c["n"]
    kw = dict(margin=c["margin"], tol=TOL, max_evals=MAX_EVALS)
    s = _open(c)
    full = s.motion_clearance(qa, dv=dv, **kw)
    # n in {1, 63, 64, 65}: every row is its own segment
    for m in (1, 63, 64):
        assert _same(s.motion_clearance(qa[:m], dv=dv[:m], **kw), {k: v[:m] for k, v in full.items()})
    assert _same(s.motion_clearance(qa[7:8], dv=dv[7:8], **kw), {k: v[7:8] for k, v in full.items()})
    # n = 0
    empty = s.motion_clearance(qa[:0], dv=dv[:0], **kw)
    assert empty["status"].shape == (0,) and empty["witness"].shape == (0, 3)
    # dv = 0: nothing moves, delta = +inf: BLOCKED at 0 after one sample or FREE after two
    still = s.motion_clearance(qa, dv=np.zeros_like(dv), **kw)
    start = s.clearance(qa)
    blocked = start["min"] < c["margin"] + TOL
    assert np.array_equal(still["status"], np.where(blocked, MN.BLOCKED, MN.FREE)) and np.array_equal(still["evals"], np.where(blocked, 1, 2))
    assert np.array_equal(still["s_free"], np.where(blocked, 0.0, 1.0)) and np.all(still["s_at_min"] == 0.0)
    assert np.max(np.abs(still["min_sampled"] - start["min"])) <= BOUND * c["scale"] and np.array_equal(still["witness"], start["witness"])
    # max_evals = 1: the sample at 0 alone; UNDECIDED unless it blocks
    one = s.motion_clearance(qa, dv=dv, margin=c["margin"], tol=TOL, max_evals=1)
    assert np.array_equal(one["status"], np.where(blocked, MN.BLOCKED, MN.UNDECIDED)) and np.all(one["evals"] == 1) and np.all(one["s_free"] == 0.0)
    assert np.array_equal(one["min_sampled"], still["min_sampled"])
    # a NaN row of qa, an infinite entry of dv: INVALID alone
    qn, dn = qa.copy(), dv.copy()
    qn[2, 3], dn[64, model.nv - 1] = np.nan, np.inf
    bad = s.motion_clearance(qn, dv=dn, **kw)
    for i in (2, 64):
        assert bad["status"][i] == MN.INVALID and bad["evals"][i] == 0 and tuple(bad["witness"][i]) == (CN.NONE, -1, -1)
        assert np.isnan([bad["s_free"][i], bad["min_sampled"][i], bad["s_at_min"][i]]).all()
    keep = ~np.isin(np.arange(n), (2, 64))
    assert _same({k: v[keep] for k, v in bad.items()}, {k: v[keep] for k, v in full.items()})
    # a sphere on link 0 does not move: alone against the world it answers at once, with the others it changes no step of theirs
    s.set_collision_spheres([0], [[0.3, 0.1, 0.2, 0.05]])
    fixed = s.motion_clearance(qa, dv=dv, margin=-10.0, tol=TOL, max_evals=MAX_EVALS)
    assert np.all(fixed["status"] == MN.FREE) and np.all(fixed["evals"] == 2) and np.max(np.abs(fixed["min_sampled"] - s.clearance(qa)["min"])) <= BOUND * c["scale"]
    lk, sp = np.concatenate([[0], c["links"]]).astype(np.int32), np.concatenate([[[0.3, 0.1, 0.2, 0.05]], c["spheres"]])
    s.set_collision_spheres(lk, sp)
    pairs = CN.self_pairs(model.parents, lk)
    want = MN.advance(model, qa, dv, lk, sp, c["ws"], c["wb"], pairs, margin=c["margin"], tol=TOL, max_evals=MAX_EVALS)
    assert np.all(want["Lambda"][:, 0] == 0.0)
    _compare(s.motion_clearance(qa, dv=dv, **kw), want, c["scale"], "panda7 with a sphere on link 0")
    s.close()


def test_pointer_routes_agree():
    c = motion_case("talos32")
    model, qa, dv, n = c["model"], c["qa"], c["dv"], c["n"]
    kw = dict(margin=c["margin"], tol=TOL, max_evals=MAX_EVALS)
    s = _open(c)
    host = s.motion_clearance(qa, dv=dv, **kw)
    dqa, ddv = capi.DeviceArray(qa), capi.DeviceArray(dv)
    assert _same(host, s.motion_clearance(dqa, dv=ddv, **kw))          # device in, host out
    hip = capi.DeviceArray.hip()

    def back(val, info):
        v, i = np.empty((n, 3)), np.empty((5 * n + 1) // 2)
        assert hip.hipMemcpy(v.ctypes.data_as(C.c_void_p), C.c_void_p(val.data_ptr()), v.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        assert hip.hipMemcpy(i.ctypes.data_as(C.c_void_p), C.c_void_p(info.data_ptr()), i.nbytes, 2) == 0
        return capi.BatchedLoik._motion_result(v, i.view(np.int32)[:5 * n].reshape(n, 5))
    for a, d in ((qa, dv), (dqa, ddv)):                                  # host in and device in, device out
        val, info = capi.DeviceArray(np.full(3 * n, -1.0)), capi.DeviceArray(np.zeros((5 * n + 1) // 2))
        s.motion_clearance(a, dv=d, out=(val, info), **kw)
        assert _same(host, back(val, info))
        val.free(); info.free()
    # difference: the four routes; then the end point on the device
    q1 = model.random_configurations(np.random.default_rng(830), n)
    v = s.difference(qa, q1)
    dq1, dvo = capi.DeviceArray(q1), capi.DeviceArray(np.zeros((n, model.nv)))
    assert np.array_equal(v, s.difference(dqa, dq1))
    for a, b in ((qa, q1), (dqa, dq1)):
        s.difference(a, b, out=dvo)
        got = np.empty((n, model.nv))
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), C.c_void_p(dvo.data_ptr()), got.nbytes, 2) == 0
        assert np.array_equal(got, v)
    assert _same(s.motion_clearance(qa, qb=q1, **kw), s.motion_clearance(dqa, qb=dq1, **kw))
    for a in (dqa, ddv, dq1, dvo):
        a.free()
    s.close()


# ---- 3. neutrality --------------------------------------------------------------------------------------------------------------------------
def test_the_calls_change_no_solve_and_no_resident_q():
    c = motion_case("talos32")
    model, qa, dv = c["model"], c["qa"], c["dv"]
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
                s.motion_clearance(qa[::-1].copy(), dv=dv, margin=c["margin"], tol=TOL, max_evals=MAX_EVALS)
                s.difference(qa[::-1].copy(), qa)
                s.path_clearance(np.stack([qa, qa[::-1]], axis=1), margin=c["margin"], tol=TOL, max_evals=4)
        q0 = s.get("q")
        calls()
        assert np.array_equal(q0, s.get("q"))
        s.Solve()
        out = [s.get("z"), s.get("iter")]
        calls()
        out += [s.get("z"), s.get("iter"), s.get("q")]
        p = s.SolvePose(tg, tol_pose=1e-4, max_steps=6)
        calls()
        out += [s.get("q"), p["status"], p["err"], s.clearance()["min"]]
        res.append(out)
        s.close()
    assert all(np.array_equal(a, b) for a, b in zip(*res))


# ---- 4. validation ---------------------------------------------------------------------------------------------------------------------------
def test_errors():
    c = motion_case("panda7")
    model, qa, dv, n = c["model"], c["qa"], c["dv"], c["n"]
    s = TC._open(model, qa)
    # no spheres: LOIKB_ERR_STATE from both checks, n = 0 included; difference needs none
    for fn, a in ((s.motion_clearance, dict(dv=dv)), (s.path_clearance, {})):
        with pytest.raises(capi.LoikError) as e:
            fn(qa if a else np.stack([qa, qa], axis=1), **a)
        assert e.value.code == ERR_STATE and "no spheres" in str(e.value)
    assert s.difference(qa, qa).shape == (n, model.nv)
    s.close()
    s = _open(c)
    L, h, vp = s.L, s.h, C.c_void_p
    val, info = np.empty((n, 3)), np.empty((n, 5), dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(vp)
    good = capi.MotionParams(0.0, 1e-3, 8, 0)

    def call(prm=good, qa_=ptr(qa), dv_=ptr(dv), n_=n, val_=ptr(val), info_=ptr(info)):
        return L.loikb_motion_clearance(h, qa_, dv_, n_, 0, C.byref(prm) if prm is not None else None, val_, info_, 0)

    def path(prm=good, q_=ptr(qa), B_=n // 5, T_=5, val_=ptr(val), info_=ptr(info)):
        return L.loikb_motion_clearance_path(h, q_, B_, T_, 0, C.byref(prm) if prm is not None else None, val_, info_, 0)
    assert call() == 0 and path() == 0
    for bad, text in ((capi.MotionParams(np.nan, 1e-3, 8, 0), b"margin"), (capi.MotionParams(np.inf, 1e-3, 8, 0), b"margin"),
                      (capi.MotionParams(0.0, np.nan, 8, 0), b"tol"), (capi.MotionParams(0.0, np.inf, 8, 0), b"tol"),
                      (capi.MotionParams(0.0, 0.5e-9, 8, 0), b"tol"), (capi.MotionParams(0.0, -1e-3, 8, 0), b"tol"),
                      (capi.MotionParams(0.0, 1e-3, 0, 0), b"max_evals"), (capi.MotionParams(0.0, 1e-3, 65537, 0), b"max_evals"),
                      (capi.MotionParams(0.0, 1e-3, 8, 1), b"flags"), (None, b"p == NULL")):
        assert call(bad) == ERR_ARG and text in L.loikb_last_error(), text
        assert path(bad) == ERR_ARG and text in L.loikb_last_error(), text
        assert call(bad, n_=0) == ERR_ARG       # the arguments are checked before anything else
    assert call(capi.MotionParams(0.0, 1e-9, 65536, 0), n_=1) == 0
    assert call(n_=-1) == ERR_ARG and call(qa_=None) == ERR_ARG and call(dv_=None) == ERR_ARG and call(val_=None) == ERR_ARG and call(info_=None) == ERR_ARG
    assert call(n_=0, qa_=None, dv_=None, val_=None, info_=None) == 0
    assert L.loikb_motion_clearance(None, ptr(qa), ptr(dv), n, 0, C.byref(good), ptr(val), ptr(info), 0) == ERR_ARG
    assert path(T_=1) == ERR_ARG and b"T >= 2" in L.loikb_last_error() and path(T_=0) == ERR_ARG and path(T_=1, B_=0) == ERR_ARG
    assert path(B_=-1) == ERR_ARG and path(q_=None) == ERR_ARG and path(val_=None) == ERR_ARG and path(info_=None) == ERR_ARG
    assert path(B_=0, q_=None, val_=None, info_=None) == 0
    v = np.empty((n, model.nv))
    assert L.loikb_difference(h, ptr(qa), ptr(qa), -1, 0, ptr(v), 0) == ERR_ARG and L.loikb_difference(h, None, ptr(qa), n, 0, ptr(v), 0) == ERR_ARG
    assert L.loikb_difference(h, ptr(qa), None, n, 0, ptr(v), 0) == ERR_ARG and L.loikb_difference(h, ptr(qa), ptr(qa), n, 0, None, 0) == ERR_ARG
    assert L.loikb_difference(None, ptr(qa), ptr(qa), n, 0, ptr(v), 0) == ERR_ARG and L.loikb_difference(h, None, None, 0, 0, None, 0) == 0
    # spheres gone: the state error again
    s.set_collision_spheres([], np.zeros((0, 4)))
    assert call() == ERR_STATE and path() == ERR_STATE and call(n_=0) == ERR_STATE
    s.close()
