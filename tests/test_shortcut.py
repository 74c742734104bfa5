"""GPU: certified shortcutting of include/loik_amd_shortcut.h against the numpy reference of tests/shortcut_numpy.py (proven on the CPU by
test_shortcut_numpy.py): the eight robots, spheres and world of test_clearance._case (tree330 takes its records and dv from the global
slab), agreement with path_clearance and motion_clearance, the wall a sampled check misses, the edge cases, determinism and the pointer
routes, neutrality towards the solves, the validation, and path_length."""
import ctypes as C

import numpy as np
import pytest

import loik_amd
from loik_amd import capi

import motion_numpy as MN
import pose_numpy as P
import qp_cases as QC
import shortcut_numpy as SN
import test_clearance as TC
import test_motion_clearance as TM

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -20, -24
T_PATH, TOL, MAX_EVALS, ROUNDS, SEED = 6, 1e-3, 24, 8, 4242
# |length - numpy| / (1 + length): 16 times the largest error measured on one MI355X over the eight robots of test 1 and the two of
# test 8 (profiles/shortcut_measured.md), the allowance for another compiler's rounding, as S_BOUND of test_motion_clearance.py was set
LENGTH_MEASURED = 1.111e-16   # (multidof13; the others between 6.4e-17 and 1.11e-16)
LENGTH_BOUND = 16 * LENGTH_MEASURED

_CASES = {}


def make_paths(model, q0, size, T, rng):
    """[B][T][nq]: path b starts at q0[b]; each next waypoint is the last (+) size * uniform(-1, 1), the steps drawn waypoint by waypoint"""
    rows = [np.asarray(q0, dtype=float)]
    for _ in range(T - 1):
        step = size * rng.uniform(-1.0, 1.0, size=(rows[0].shape[0], model.nv))
        rows.append(np.stack([P.integrate(model, q, v) for q, v in zip(rows[-1], step)]))
    return np.ascontiguousarray(np.stack(rows, axis=1))


def shortcut_case(name):
    """the model, spheres, world and pairs of test_clearance._case, B = min(16, n) paths of T = 6 waypoints from its q, the margin = the
    10 % quantile of the clearance over all waypoints, and the numpy answer: computed once"""
    if name not in _CASES:
        c = dict(TC._case(name))
        model = c["model"]
        B = min(16, c["n"])
        c["B"], c["paths"] = B, make_paths(model, c["q"][:B], TM.SIZE[name], T_PATH, np.random.default_rng(900))
        at = MN.clearance_min(model, c["paths"].reshape(-1, model.nq), c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"])
        c["margin"] = float(np.quantile(at, 0.1))
        c["kw"] = dict(rounds=ROUNDS, seed=SEED, margin=c["margin"], tol=TOL, max_evals=MAX_EVALS)
        c["want"] = SN.shortcut(model, c["paths"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], **c["kw"])
        _CASES[name] = c
    return _CASES[name]


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def _rows(r, rows):
    return {k: v[rows] for k, v in r.items()}


COUNTERS = ("n_waypoints", "tried", "accepted", "blocked", "undecided", "invalid")


def _check_shape(got, paths, n=None):
    """what holds for every result: the kept rows bit for bit, the padding, the ends, a strictly increasing keep"""
    B, T = paths.shape[:2]
    n = np.full(B, T) if n is None else np.asarray(n)
    for b in range(B):
        L = int(got["n_waypoints"][b])
        if not 2 <= n[b] <= T:
            assert L == 0 and np.all(got["keep"][b] == -1) and np.isnan(got["q_path"][b]).all()
            assert all(got[k][b] == 0 for k in COUNTERS) and np.isnan(got["length_in"][b]) and np.isnan(got["length_out"][b])
            continue
        keep = got["keep"][b]
        assert 2 <= L <= n[b] and keep[0] == 0 and keep[L - 1] == n[b] - 1 and np.all(np.diff(keep[:L]) > 0) and np.all(keep[L:] == -1)
        assert np.array_equal(got["q_path"][b, :L], paths[b, keep[:L]], equal_nan=True)
        assert np.array_equal(got["q_path"][b, L:], np.tile(paths[b, keep[L - 1]], (T - L, 1)), equal_nan=True)
        assert got["tried"][b] == got["accepted"][b] + got["blocked"][b] + got["undecided"][b] + got["invalid"][b]
        assert L == n[b] - int(np.sum(np.diff(keep[:L]) - 1))


def _length_error(got, want):
    err = 0.0
    for k in ("length_in", "length_out"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k]))
        ok = ~np.isnan(want[k])
        err = max(err, float(np.max(np.abs(got[k][ok] - want[k][ok]) / (1.0 + want[k][ok]), initial=0.0)))
    return err


# ---- 1. against numpy on eight robots, 2. agreement with the existing entry points -----------------------------------------------------
# The reference of all eight robots has no path with a decision within 1e-9 of its threshold (checked on the CPU; at most 1 of 16 is
# allowed), so rng 900 and seed 4242 stand for every robot.  panda7, talos32, multidof13 and composite20 accept / block / leave undecided
# 36 / 34 / 14, 39 / 27 / 0, 35 / 42 / 11 and 34 / 22 / 28 segments; some paths stay at 6 waypoints, some collapse to 2.  The two big trees
# walk every root path in Python: their reference takes 9 s and 17 s of numpy, the others 1 to 2 s
@pytest.mark.parametrize("name", list(TC.ROBOTS))
def test_shortcut_matches_numpy_and_the_motion_checks(name):
    c = shortcut_case(name)
    model, paths, want, B = c["model"], c["paths"], c["want"], c["B"]
    tot = {k: int(want[k].sum()) for k in COUNTERS}
    print("shortcut_measured %s: %s, paths with near %d, waypoints left %s" % (name, tot, int(want["near"].sum()), want["n_waypoints"].tolist()))
    if name not in TC.BIG_TREES:
        assert tot["accepted"] > 0 and tot["blocked"] > 0, tot
    assert want["near"].sum() <= 1
    s = TM._open(c)
    got = s.shortcut_paths(paths, **c["kw"])
    _check_shape(got, paths)
    sure = ~want["near"]
    for k in COUNTERS + ("keep",):
        assert np.array_equal(got[k][sure], want[k][sure]), (name, k, got[k], want[k])
    err = _length_error(_rows(got, sure), _rows({k: want[k] for k in got}, sure))
    print("shortcut_measured %s: max |length - numpy| / (1 + length) %.3e" % (name, err))
    assert err <= LENGTH_BOUND, (name, err)
    # the repeated last row adds nothing: the length of the padded result is the length after, bit for bit
    assert np.array_equal(s.path_length(got["q_path"]), got["length_out"])
    # 2. every segment that is not an input segment is FREE under path_clearance, and its row is motion_clearance's, bit for bit
    chk = s.path_clearance(got["q_path"], margin=c["margin"], tol=TOL, max_evals=MAX_EVALS)
    seen = 0
    for b in range(B):
        L, keep = int(got["n_waypoints"][b]), got["keep"][b]
        for k in range(L - 1):
            if keep[k + 1] == keep[k] + 1:
                continue
            seen += 1
            assert chk["status"][b, k] == MN.FREE, (name, b, k)
            one = s.motion_clearance(paths[b, keep[k]][None], qb=paths[b, keep[k + 1]][None], margin=c["margin"], tol=TOL, max_evals=MAX_EVALS)
            assert all(np.array_equal(one[f][0], chk[f][b, k]) for f in one), (name, b, k)
    assert seen > 0 or tot["accepted"] == 0
    s.close()


# ---- 3. the wall a sampled check misses ---------------------------------------------------------------------------------------------------
def test_a_thin_box_across_the_direct_segment_blocks_the_shortcut():
    model = QC.model_of("panda7")
    rng = np.random.default_rng(750)
    A = model.random_configurations(rng, 1)[0]
    dv = np.array([0.9, -0.7, 0.5, 0.8, -0.6, 0.4, 0.3])
    Bq = A + dv
    Cq = A + 0.5 * dv + np.array([0.3, 0.3, -0.3, 0.0, 0.0, 0.0, 0.0])
    links, spheres = np.array([7], dtype=np.int32), np.array([[0.0, 0.0, 0.1, 0.01]])
    box = MN.thin_box_across(model, A, dv, 7, spheres[0])
    paths = np.stack([A, Cq, Bq])[None]
    margin = 0.0
    s = TC._open(model, paths[0])
    s.set_collision_spheres(links, spheres)
    s.set_collision_world(None, box[None])
    assert np.all(s.clearance(np.stack([A, Bq]))["min"] >= margin + TOL)
    got = s.shortcut_paths(paths, rounds=4, seed=1, margin=margin, tol=TOL)
    assert got["n_waypoints"][0] == 3 and got["tried"][0] == got["blocked"][0] == 4 and got["accepted"][0] == 0
    assert got["keep"][0].tolist() == [0, 1, 2] and np.array_equal(got["q_path"], paths)
    s.set_collision_world(None, None)
    got = s.shortcut_paths(paths, rounds=4, seed=1, margin=margin, tol=TOL)
    assert got["n_waypoints"][0] == 2 and got["tried"][0] == got["accepted"][0] == 1 and got["keep"][0].tolist() == [0, 2, -1]
    assert np.array_equal(got["q_path"][0], np.stack([A, Bq, Bq])) and got["length_out"][0] < got["length_in"][0]
    s.close()


# ---- 4. the edge cases -----------------------------------------------------------------------------------------------------------------------
def test_edges():
    c = shortcut_case("panda7")
    model, paths, B, kw = c["model"], c["paths"], c["B"], c["kw"]
    T = paths.shape[1]
    s = TM._open(c)
    full = s.shortcut_paths(paths, **kw)
    # rounds = 0: a copy with lengths
    zero = s.shortcut_paths(paths, **dict(kw, rounds=0))
    assert np.array_equal(zero["q_path"], paths) and np.all(zero["n_waypoints"] == T) and np.all(zero["keep"] == np.arange(T))
    assert all(np.all(zero[k] == 0) for k in COUNTERS[1:]) and np.array_equal(zero["length_in"], zero["length_out"])
    assert np.array_equal(zero["length_in"], full["length_in"]) and np.array_equal(zero["length_in"], s.path_length(paths))
    # T = 2: nothing to draw
    two = s.shortcut_paths(paths[:, :2].copy(), **kw)
    assert np.array_equal(two["q_path"], paths[:, :2]) and np.all(two["n_waypoints"] == 2) and np.all(two["tried"] == 0)
    # n_waypoints of 0, 1, 2, T and T + 1 in one batch: the three outside 2 .. T are skipped, the others are as a run of their own
    n = np.array([0, 1, 2, T, T + 1], dtype=np.int32)
    mixed = s.shortcut_paths(paths[:5], n_waypoints=n, **kw)
    _check_shape(mixed, paths[:5], n)
    assert mixed["n_waypoints"][2] == 2 and mixed["tried"][2] == 0 and mixed["keep"][2].tolist() == [0, 1] + [-1] * (T - 2)
    assert _same(_rows(mixed, [3]), _rows(full, [3]))
    lens = s.path_length(paths[:5], n_waypoints=n)
    assert lens[0] == 0.0 and lens[1] == 0.0 and np.isnan(lens[4]) and lens[3] == full["length_in"][3] and lens[2] == mixed["length_in"][2] > 0.0
    # NaN rows from a cursor on, as SolvePosePath records them, with n_waypoints = cursor: the truncated path's result
    cur = 4
    rec = paths.copy()
    rec[:, cur:] = np.nan
    got = s.shortcut_paths(rec, n_waypoints=np.full(B, cur, dtype=np.int32), **kw)
    _check_shape(got, rec, np.full(B, cur))
    cut = s.shortcut_paths(np.ascontiguousarray(paths[:, :cur]), **kw)
    assert np.array_equal(got["keep"][:, :cur], cut["keep"]) and np.array_equal(got["q_path"][:, :cur], cut["q_path"])
    assert all(np.array_equal(got[k], cut[k]) for k in COUNTERS + ("length_in", "length_out")) and cut["accepted"].sum() > 0
    # ... and cursors that differ from path to path, against the reference
    curs = np.array([2 + b % (T - 1) for b in range(B)], dtype=np.int32)
    for b in range(B):
        rec[b] = paths[b]
        rec[b, curs[b]:] = np.nan
    got = s.shortcut_paths(rec, n_waypoints=curs, **kw)
    _check_shape(got, rec, curs)
    want = SN.shortcut(model, rec, c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], n_waypoints=curs, **kw)
    sure = ~want["near"]
    assert sure.sum() >= B - 1 and all(np.array_equal(got[k][sure], want[k][sure]) for k in COUNTERS + ("keep",))
    # a NaN waypoint inside a path, at an inner end of the path's first draw: the tried segments that touch it are invalid, the other
    # paths bit-identical
    b, row = next((b, r) for b in range(B) for r in c["want"]["segments"][b][0][:2] if 0 < r < T - 1)
    bad = paths.copy()
    bad[b, row, 1] = np.nan
    got = s.shortcut_paths(bad, **kw)
    _check_shape(got, bad)
    others = np.arange(B) != b
    assert _same(_rows(got, others), _rows(full, others))
    want = SN.shortcut(model, bad, c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], **kw)
    touched = sum(row in (i, j) for i, j, _ in want["segments"][b])
    assert touched > 0 and want["invalid"][b] == touched and np.isnan(got["length_in"][b])
    assert want["near"][b] or (all(got[k][b] == want[k][b] for k in COUNTERS) and np.array_equal(got["keep"][b], want["keep"][b]))
    # B = 0
    none = s.shortcut_paths(paths[:0], **kw)
    assert none["q_path"].shape == (0, T, model.nq) and none["keep"].shape == (0, T) and none["tried"].shape == (0,)
    assert s.path_length(paths[:0]).shape == (0,)
    s.close()


# ---- 5. determinism and the routes ----------------------------------------------------------------------------------------------------------
def _device_i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32).ravel()
    return capi.DeviceArray(np.concatenate([a, np.zeros(a.size % 2, dtype=np.int32)]).view(np.float64))


def _back(dev, shape, dtype):
    n = int(np.prod(shape))
    raw = np.empty((n * np.dtype(dtype).itemsize + 7) // 8)
    assert capi.DeviceArray.hip().hipMemcpy(raw.ctypes.data_as(C.c_void_p), C.c_void_p(dev.data_ptr()), raw.nbytes, 2) == 0   # hipMemcpyDeviceToHost
    return raw.view(dtype)[:n].reshape(shape).copy()


def test_determinism_and_pointer_routes():
    c = shortcut_case("talos32")
    model, paths, B, kw = c["model"], c["paths"], c["B"], c["kw"]
    T, nq = paths.shape[1], model.nq
    n = np.array([T - b % 3 for b in range(B)], dtype=np.int32)
    s = TM._open(c)
    host = s.shortcut_paths(paths, n_waypoints=n, **kw)
    assert _same(host, s.shortcut_paths(paths, n_waypoints=n, **kw))       # the same call twice
    s32 = TM._open(c, capi.F32)
    assert _same(host, s32.shortcut_paths(paths, n_waypoints=n, **kw))     # fp64 whatever the handle's precision
    s32.close()
    dq, dn = capi.DeviceArray(paths), _device_i32(n)
    assert _same(host, s.shortcut_paths(dq, n_waypoints=dn, **kw))         # device in, host out
    assert np.array_equal(s.path_length(paths, n_waypoints=n), s.path_length(dq, n_waypoints=dn))
    for a, l in ((paths, n), (dq, dn)):                                    # host in and device in, device out
        bufs = (capi.DeviceArray(np.full(B * T * nq, -1.0)), _device_i32(np.zeros(B * T)), _device_i32(np.zeros(6 * B)), capi.DeviceArray(np.zeros(2 * B)))
        s.shortcut_paths(a, n_waypoints=l, out=bufs, **kw)
        got = capi.BatchedLoik._shortcut_result(_back(bufs[0], (B, T, nq), np.float64), _back(bufs[1], (B, T), np.int32),
                                                _back(bufs[2], (B, 6), np.int32), _back(bufs[3], (B, 2), np.float64))
        assert _same(host, got)
        # without keep and lengths: the keep rows live in the handle's scratch
        s.shortcut_paths(a, n_waypoints=l, out=(bufs[0], None, bufs[2], None), **kw)
        assert np.array_equal(_back(bufs[0], (B, T, nq), np.float64), host["q_path"])
        assert np.array_equal(_back(bufs[2], (B, 6), np.int32)[:, 0], host["n_waypoints"])
        ln = capi.DeviceArray(np.zeros(B))
        s.path_length(a, n_waypoints=l, out=ln)
        assert np.array_equal(_back(ln, (B,), np.float64), host["length_in"])
        for d in bufs + (ln,):
            d.free()
    dq.free(); dn.free()
    # the contents of the other paths do not reach path b
    other = paths[::-1].copy()
    other[5] = paths[5]
    assert _same(_rows(host, [5]), _rows(s.shortcut_paths(other, n_waypoints=n, **kw), [5]))
    # another seed draws other segments
    reseeded = s.shortcut_paths(paths, n_waypoints=n, **dict(kw, seed=SEED + 1))
    assert not np.array_equal(reseeded["keep"], host["keep"])
    s.close()


# ---- 6. neutrality ---------------------------------------------------------------------------------------------------------------------------
def test_the_calls_change_no_solve_and_no_resident_q():
    c = shortcut_case("talos32")
    model, paths, kw = c["model"], c["paths"], c["kw"]
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
                s.shortcut_paths(paths, **kw)
                s.path_length(paths)
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


# ---- 7. validation ---------------------------------------------------------------------------------------------------------------------------
def test_errors():
    c = shortcut_case("panda7")
    model, paths = c["model"], c["paths"]
    B, T, nq = paths.shape
    s = TC._open(model, c["q"])
    with pytest.raises(capi.LoikError) as e:      # no spheres: the state error, B = 0 included; path_length needs none
        s.shortcut_paths(paths)
    assert e.value.code == ERR_STATE and "no spheres" in str(e.value)
    with pytest.raises(capi.LoikError) as e:
        s.shortcut_paths(paths[:0])
    assert e.value.code == ERR_STATE
    assert s.path_length(paths).shape == (B,)
    s.close()
    s = TM._open(c)
    L, h, vp = s.L, s.h, C.c_void_p
    ptr = lambda a: a.ctypes.data_as(vp)
    outs = [np.full((B, T, nq), -7.0), np.full((B, T), -7, dtype=np.int32), np.full((B, 6), -7, dtype=np.int32), np.full((B, 2), -7.0)]
    good = capi.ShortcutParams(0.0, 1e-3, 8, 4, 1, 0)
    untouched = lambda: all(np.all(o == -7) for o in outs)

    def call(prm=good, q_=ptr(paths), len_=None, B_=B, T_=T, path_=ptr(outs[0]), keep_=ptr(outs[1]), info_=ptr(outs[2]), val_=ptr(outs[3]), h_=h):
        return L.loikb_shortcut_paths(h_, q_, len_, B_, T_, 0, C.byref(prm) if prm is not None else None, path_, keep_, info_, val_, 0)
    P_ = capi.ShortcutParams
    for bad, text in ((P_(np.nan, 1e-3, 8, 4, 1, 0), b"margin"), (P_(np.inf, 1e-3, 8, 4, 1, 0), b"margin"), (P_(0.0, np.nan, 8, 4, 1, 0), b"tol"),
                      (P_(0.0, 0.5e-9, 8, 4, 1, 0), b"tol"), (P_(0.0, 1e-3, 0, 4, 1, 0), b"max_evals"), (P_(0.0, 1e-3, 65537, 4, 1, 0), b"max_evals"),
                      (P_(0.0, 1e-3, 8, -1, 1, 0), b"rounds"), (P_(0.0, 1e-3, 8, 1048577, 1, 0), b"rounds"), (P_(0.0, 1e-3, 8, 4, 1, 1), b"flags"),
                      (None, b"p == NULL")):
        assert call(bad) == ERR_ARG and text in L.loikb_last_error(), text
        assert call(bad, B_=0) == ERR_ARG       # the arguments are checked before anything else
    assert call(h_=None) == ERR_ARG
    assert call(path_=None) == ERR_ARG and b"out_path" in L.loikb_last_error() and call(info_=None) == ERR_ARG and b"out_info" in L.loikb_last_error()
    assert call(q_=None) == ERR_ARG and b"q_path" in L.loikb_last_error() and call(B_=-1) == ERR_ARG and b"B >= 0" in L.loikb_last_error()
    assert call(T_=1) == ERR_ARG and b"T >= 2" in L.loikb_last_error() and call(T_=1, B_=0) == ERR_ARG
    assert call(B_=1 << 20, T_=1 << 11) == ERR_ARG and b"2^31" in L.loikb_last_error()
    assert call(path_=ptr(paths)) == ERR_ARG and b"out_path == q_path" in L.loikb_last_error()
    assert untouched()
    assert call(B_=0, q_=None) == 0 and untouched()
    assert call(P_(0.0, 1e-9, 65536, 1048576, 2 ** 64 - 1, 0), B_=0) == 0 and untouched() and call(keep_=None, val_=None) == 0
    ln = np.full(B, -7.0)

    def length(q_=ptr(paths), B_=B, T_=T, out_=ptr(ln), h_=h):
        return L.loikb_path_length(h_, q_, None, B_, T_, 0, out_, 0)
    assert length(h_=None) == ERR_ARG and length(q_=None) == ERR_ARG and b"q_path" in L.loikb_last_error()
    assert length(B_=-1) == ERR_ARG and length(T_=1) == ERR_ARG and b"T >= 2" in L.loikb_last_error()
    assert length(B_=1 << 20, T_=1 << 11) == ERR_ARG and length(out_=None) == ERR_ARG and b"out_length" in L.loikb_last_error()
    assert np.all(ln == -7.0) and length(B_=0, q_=None) == 0 and np.all(ln == -7.0) and length() == 0 and np.all(ln >= 0.0)
    # spheres gone: the state error again
    outs[0][:] = -7.0; outs[1][:] = -7; outs[2][:] = -7; outs[3][:] = -7.0
    s.set_collision_spheres([], np.zeros((0, 4)))
    assert call() == ERR_STATE and call(B_=0) == ERR_STATE and untouched()
    s.close()


# ---- 8. path_length ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["panda7", "multidof13"])
def test_path_length_matches_numpy(name):
    c = shortcut_case(name)
    model, paths, B = c["model"], c["paths"], c["B"]
    T = paths.shape[1]
    s = TC._open(model, c["q"])      # no spheres: none are needed
    n = np.array([b % (T + 1) for b in range(B)], dtype=np.int32)
    for cnt in (None, n):
        got, want = s.path_length(paths, n_waypoints=cnt), SN.path_length(model, paths, cnt)
        err = float(np.max(np.abs(got - want) / (1.0 + want)))
        print("shortcut_measured path_length %s: max |length - numpy| / (1 + length) %.3e, longest %.3f" % (name, err, want.max()))
        assert got.shape == (B,) and err <= LENGTH_BOUND, (name, err)
    assert np.all(want[n < 2] == 0.0) and np.all(got[n < 2] == 0.0) and np.all(want[n >= 2] > 0.0)
    # identical waypoints: exactly 0
    still = np.ascontiguousarray(np.tile(paths[:, :1], (1, T, 1)))
    assert np.all(s.path_length(still) == 0.0)
    s.close()
