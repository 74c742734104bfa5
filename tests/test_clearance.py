"""GPU: the clearance query of include/loik_amd_collision.h against the numpy reference of tests/clearance_numpy.py (proven on the CPU by
test_clearance_numpy.py): eight robots (a chain, a tree, nq != nv, helical / prismatic joints, a 170-joint tree that launches fewer
configurations per workgroup, a 330-joint tree whose liM records do not fit one wavefront's LDS and takes the placements from HBM, a
tree with composite joints whose links are several device joints each, a second multi-DoF tree), the sizes at which the kernel
changes its path, the caller's parents and ignore pairs on composite links, the witness, ties, the sphere / box branches, the q
routes, a NaN row, neutrality towards the solves and the validation."""
import ctypes as C

import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from helpers import random_rotation, random_tree
from test_pose_ik import PRM, _fk_models, _handle, _links
import clearance_numpy as CN
import pose_numpy as P
import qp_cases as QC

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -20, -24
# |min - oracle| <= BOUND * scale, scale = 1 + max |centre| + max r: the bound of the FK-derived quantities of test_frame_jacobians.py
BOUND = 1e-13
# name -> (configurations, spheres per link).  tree170: 170 * 96 * 2 + 170 * 32 bytes = 38 KB a wavefront, one configuration per
# workgroup instead of four; tree330: 74 KB > 64 KB, the HBM-placement instantiation.  The reference walks every root path in Python,
# so the two big trees take fewer configurations
ROBOTS = {"panda7": (65, 3), "talos32": (65, 2), "multidof20": (65, 2), "helical24": (65, 2), "tree170": (9, 1), "tree330": (3, 1),
          "composite20": (65, 2), "multidof13": (65, 2)}
BIG_TREES = {"tree170": (52, 170), "tree330": (53, 330)}

_CASES = {}


def _model(name):
    if name == "multidof13":   # free-flyer root, translation, two ZYX, planar, three (cos, sin) revolutes
        return _fk_models()[3]
    return random_tree(*BIG_TREES[name]) if name in BIG_TREES else QC.model_of(name)


def _world(rng, nws, nwb):
    ws = np.concatenate([rng.uniform(-1.0, 1.0, size=(nws, 3)), rng.uniform(0.05, 0.3, size=(nws, 1))], axis=1)
    wb = np.array([np.concatenate([random_rotation(rng).reshape(9), rng.uniform(-1.0, 1.0, size=3), rng.uniform(0.05, 0.4, size=3)]) for _ in range(nwb)]).reshape(nwb, 15)
    return ws, wb


def _case(name):
    """model, q, spheres on every link, a world of 33 spheres and 32 boxes, the self pairs and the numpy answer: computed once"""
    if name not in _CASES:
        n, k = ROBOTS[name]
        model = _model(name)
        rng = np.random.default_rng(400 + list(ROBOTS).index(name))
        q = model.random_configurations(rng, n)
        links, spheres = CN.make_spheres(model, k, 410)
        ws, wb = _world(rng, 33, 32)
        pairs = CN.self_pairs(model.parents, links)
        _CASES[name] = dict(model=model, n=n, q=q, links=links, spheres=spheres, ws=ws, wb=wb, pairs=pairs,
                            want=CN.clearance(model, q, links, spheres, ws, wb, pairs))
    return _CASES[name]


def _open(model, q, precision=capi.F64):
    s, _ = _handle(model, q.shape[0], [model.njoints - 1], q, precision=precision)
    return s


def _scale(want, spheres):
    return 1.0 + float(np.max(np.abs(want["centres"]))) + float(np.max(np.asarray(spheres)[:, 3]))


def _compare(got, want, spheres, what):
    """the three minima within BOUND * scale, their signs where the oracle is clear of zero, the device's witness pair at the oracle's
    minimum, min == min(min_world, min_self) exactly.  Returns the largest error over scale"""
    scale = _scale(want, spheres)
    worst = 0.0
    for key in ("min", "min_world", "min_self"):
        g, w = got[key], want[key]
        assert g.shape == w.shape
        inf = np.isposinf(w)
        assert np.array_equal(np.isposinf(g), inf), (what, key)
        err = float(np.max(np.abs(g[~inf] - w[~inf]))) if (~inf).any() else 0.0
        worst = max(worst, err / scale)
        print("clearance_measured %s %s: max |got - oracle| %.3e, scale %.3f, relative %.3e" % (what, key, err, scale, err / scale))
        assert err <= BOUND * scale, (what, key, err, scale)
        clear = ~inf & (np.abs(w) > BOUND * scale)
        assert np.array_equal(np.sign(g[clear]), np.sign(w[clear])), (what, key)
    assert np.array_equal(got["min"], np.minimum(got["min_world"], got["min_self"]))
    for i in range(want["min"].size):
        wit = got["witness"][i]
        if np.isposinf(want["min"][i]):
            assert tuple(wit) == (CN.NONE, -1, -1)
            continue
        assert abs(CN.witness_value(want["table"], i, wit) - want["min"][i]) <= BOUND * scale, (what, i, wit)
    return worst


# ---- 1. against numpy on eight robots ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ROBOTS))
def test_clearance_matches_numpy(name):
    c = _case(name)
    s = _open(c["model"], c["q"])
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    assert s.num_self_pairs() == len(c["pairs"]) > 64
    got = s.clearance()
    again = s.clearance()
    worst = _compare(got, c["want"], c["spheres"], name)
    # two launches give the same bits
    assert all(np.array_equal(got[k], again[k]) for k in got)
    # fp64 from the fp64 q whatever the handle's precision
    s32 = _open(c["model"], c["q"], capi.F32)
    s32.set_collision_spheres(c["links"], c["spheres"])
    s32.set_collision_world(c["ws"], c["wb"])
    s32.set_self_collision(True)
    got32 = s32.clearance(c["q"])
    assert all(np.array_equal(got[k], got32[k]) for k in got)
    s.close(); s32.close()
    print("clearance_measured %s worst relative %.3e" % (name, worst))


# ---- 2. the sizes at which the kernel can go wrong ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 63, 64, 65, 130])
def test_sizes(ns):
    """panda7, the spheres dealt round-robin to the links 0..7 (the universe included); world objects in {0, 1, 64, 65} split between
    spheres and boxes, self pairs off and (with 0 and 65 objects) on; configurations 65 (the resident q: a last workgroup with three idle wavefronts), 3 and 1
    (an explicit q, n != B)"""
    model = QC.model_of("panda7")
    rng = np.random.default_rng(500 + ns)
    q = model.random_configurations(rng, 65)
    links = np.arange(ns, dtype=np.int32) % model.njoints
    _, spheres = CN.make_spheres(model, 1, 510 + ns, links=links)
    pairs_on = CN.self_pairs(model.parents, links)
    s = _open(model, q)
    s.set_collision_spheres(links, spheres)
    for nw in (0, 1, 64, 65):
        for split in ((nw, 0), (0, nw), (nw // 2, nw - nw // 2)) if nw else ((0, 0),):
            ws, wb = _world(rng, *split)
            s.set_collision_world(ws, wb)
            for self_on in (False, True) if nw in (0, 65) else (False,):
                s.set_self_collision(self_on)
                pairs = pairs_on if self_on else []
                assert s.num_self_pairs() == len(pairs)
                want = CN.clearance(model, q, links, spheres, ws, wb, pairs)
                what = "panda7 ns=%d world=%d+%d self=%d" % (ns, split[0], split[1], len(pairs))
                got = s.clearance()
                _compare(got, want, spheres, what)
                if nw == 0 and not pairs:   # an empty world with self pairs off
                    assert np.all(np.isposinf(got["min"])) and np.all(got["witness"] == [CN.NONE, -1, -1])
                for n in (3, 1):
                    sub = s.clearance(q[:n])
                    assert all(np.array_equal(sub[k], got[k][:n]) for k in got), (what, n)
    s.close()


def test_one_self_pair_and_more_than_64():
    model = QC.model_of("panda7")
    q = model.random_configurations(np.random.default_rng(520), 65)
    s = _open(model, q)
    for links, k in (([1, 5], 1), (list(range(1, 8)), 3)):
        lk, spheres = CN.make_spheres(model, k, 521, links=links)
        pairs = CN.self_pairs(model.parents, lk)
        assert len(pairs) == (1 if k == 1 else 135)
        s.set_collision_spheres(lk, spheres)
        s.set_self_collision(True)
        assert s.num_self_pairs() == len(pairs)
        got = s.clearance()
        _compare(got, CN.clearance(model, q, lk, spheres, pairs=pairs), spheres, "panda7 self pairs %d" % len(pairs))
        assert np.all(got["witness"][:, 0] == CN.SELF) and np.all(np.isposinf(got["min_world"]))
    # the list is rebuilt when the spheres are set, honours the ignore pairs in either order, and goes with enable = 0 or ns = 0
    s.set_self_collision(True, ignore=[(5, 1), (2, 7)])
    ig = CN.self_pairs(model.parents, lk, ignore=[(1, 5), (7, 2)])
    assert s.num_self_pairs() == len(ig) == 135 - 18
    _compare(s.clearance(), CN.clearance(model, q, lk, spheres, pairs=ig), spheres, "panda7 ignore")
    lk2, sp2 = CN.make_spheres(model, 2, 522, links=[1, 3, 5, 2])
    s.set_collision_spheres(lk2, sp2)
    assert s.num_self_pairs() == len(CN.self_pairs(model.parents, lk2, ignore=[(1, 5), (7, 2)])) == 12
    s.set_self_collision(False)
    assert s.num_self_pairs() == 0
    s.set_self_collision(True)
    s.set_collision_spheres([], np.zeros((0, 4)))
    assert s.num_self_pairs() == 0
    s.close()


# ---- 2b. a caller's link that is several device joints ---------------------------------------------------------------------------------
def _family(model, c):
    """(the parent, c, the first child) of link c in the caller's tree"""
    return int(model.parents[c]), c, min(i for i in range(1, model.njoints) if int(model.parents[i]) == c)


def test_composite_links_keep_the_callers_parents():
    """composite20: link 1 is two device joints, link 5 three, link 9 four.  The self-pair list goes by the caller's tree: the parent of
    a composite link is the link that carries the parent of its first device joint, its child hangs on its last one.  Spheres on a
    composite link, its parent and its child: only parent against child is a pair.  Then every link: no witness names a pair that
    the caller's parents exclude"""
    model = _model("composite20")
    assert {c: len(v) for c, v in model.composite.items()} == {1: 2, 5: 3, 9: 4}
    q = model.random_configurations(np.random.default_rng(560), 65)
    s = _open(model, q)
    for c in sorted(model.composite):
        fam = _family(model, c)
        lk, spheres = CN.make_spheres(model, 2, 561 + c, links=fam)
        spheres[:, 3] += 0.1     # (large enough that neighbours overlap: a parent / child pair wrongly listed would be the minimum)
        pairs = CN.self_pairs(model.parents, lk)
        assert pairs == [(a, b) for a in (0, 1) for b in (4, 5)]
        s.set_collision_spheres(lk, spheres)
        s.set_self_collision(True)
        assert s.num_self_pairs() == len(pairs) == 4
        got = s.clearance()
        _compare(got, CN.clearance(model, q, lk, spheres, pairs=pairs), spheres, "composite20 link %d, its parent and its child" % c)
        assert np.all(got["witness"][:, 0] == CN.SELF) and {(int(a), int(b)) for _, a, b in got["witness"]} <= set(pairs)
    k = _case("composite20")
    s.set_collision_spheres(k["links"], k["spheres"])
    s.set_self_collision(True)
    linked = {(int(k["links"][a]), int(k["links"][b])) for a, b in k["pairs"]}
    for c in sorted(model.composite):
        par, _, kid = _family(model, c)
        assert not linked & {(par, c), (c, par), (c, kid), (kid, c)} and ((par, kid) in linked or par == 0)
    got = s.clearance()
    _compare(got, CN.clearance(model, q, k["links"], k["spheres"], pairs=k["pairs"]), k["spheres"], "composite20 self pairs alone")
    assert np.all(got["witness"][:, 0] == CN.SELF) and {(int(a), int(b)) for _, a, b in got["witness"]} <= set(k["pairs"])
    s.close()


def test_an_ignore_pair_that_names_a_composite_link():
    k = _case("composite20")
    model, q, links, spheres = k["model"], k["q"], k["links"], k["spheres"]
    s = _open(model, q)
    s.set_collision_spheres(links, spheres)
    # composite against single, composite against composite, either order; (9, 10) is parent and child whatever the list says
    s.set_self_collision(True, ignore=[(5, 12), (1, 9), (17, 9), (9, 10)])
    pairs = CN.self_pairs(model.parents, links, ignore=[(12, 5), (9, 1), (9, 17), (10, 9)])
    assert s.num_self_pairs() == len(pairs) == len(k["pairs"]) - 3 * 4
    got = s.clearance()
    _compare(got, CN.clearance(model, q, links, spheres, pairs=pairs), spheres, "composite20 ignore, self pairs alone")
    assert {(int(a), int(b)) for _, a, b in got["witness"]} <= set(pairs)
    s.set_collision_world(k["ws"], k["wb"])
    _compare(s.clearance(), CN.clearance(model, q, links, spheres, k["ws"], k["wb"], pairs), spheres, "composite20 ignore")
    s.close()


# ---- 3. determinism and ties -----------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_index():
    """the same sphere twice and the same box twice in the world: whichever wins, the witness names the first copy"""
    c = _case("talos32")
    s = _open(c["model"], c["q"])
    s.set_collision_spheres(c["links"], c["spheres"])
    for ws, wb, kind in ((c["ws"][[2, 2]], np.zeros((0, 15)), CN.WORLD_SPHERE), (np.zeros((0, 4)), c["wb"][[1, 1]], CN.WORLD_BOX),
                         (c["ws"][[2, 2]], c["wb"][[1, 1]], None)):
        s.set_collision_world(ws, wb)
        got = s.clearance()
        assert np.all(got["witness"][:, 2] == 0) and (kind is None or np.all(got["witness"][:, 0] == kind))
        again = s.clearance()
        assert all(np.array_equal(got[k], again[k]) for k in got)
        _compare(got, CN.clearance(c["model"], c["q"], c["links"], c["spheres"], ws, wb), c["spheres"], "talos32 ties")
    # two copies of a robot sphere against one obstacle: the lower a
    lk = np.concatenate([c["links"][:1], c["links"][:1]])
    sp = np.concatenate([c["spheres"][:1], c["spheres"][:1]])
    s.set_collision_spheres(lk, sp)
    s.set_collision_world(c["ws"][:1], None)
    assert np.all(s.clearance()["witness"] == [CN.WORLD_SPHERE, 0, 0])
    s.close()


# ---- 4. the sphere / box branches -------------------------------------------------------------------------------------------------------
def test_sphere_box_regions_by_hand():
    """one sphere of the robot fixed in the world (link 0) at c = (0.5, 0.25, 1), r = 0.125, and four boxes, every number a binary
    fraction.  With e = R^T (c - t), d = |e| - h:
      face    t = (0.5, 0.25, 0), h = (1, 1, 0.5):  d = (-1, -1, 0.5)                             0.5 - 0.125    =  0.375
      edge    t = (0, 0.25, 0), R = Rz(90 deg), e = (0, -0.5, 1), h = (1, 0.125, 0.5): d = (-1, 0.375, 0.5)   0.625 - 0.125  =  0.5
      corner  t = (0, -0.5, 0), h = (0.25, 0.25, 0.5):  d = (0.25, 0.5, 0.5)                      0.75 - 0.125   =  0.625
      inside  t = (0.25, 0.25, 1), h = (0.5, 1, 1):  d = (-0.25, -1, -1)                          -0.25 - 0.125  = -0.375"""
    model = QC.model_of("panda7")
    q = model.random_configurations(np.random.default_rng(530), 3)
    s = _open(model, q)
    s.set_collision_spheres([0], [[0.5, 0.25, 1.0, 0.125]])
    I, Rz = [1, 0, 0, 0, 1, 0, 0, 0, 1], [0, -1, 0, 1, 0, 0, 0, 0, 1]
    boxes = np.array([I + [0.5, 0.25, 0.0, 1.0, 1.0, 0.5], Rz + [0.0, 0.25, 0.0, 1.0, 0.125, 0.5], I + [0.0, -0.5, 0.0, 0.25, 0.25, 0.5],
                      I + [0.25, 0.25, 1.0, 0.5, 1.0, 1.0]], dtype=float)
    values = [0.375, 0.5, 0.625, -0.375]
    for k, v in enumerate(values):
        assert float(CN.sphere_box([0.5, 0.25, 1.0], 0.125, boxes[k])) == v
        s.set_collision_world(None, boxes[k:k + 1])
        got = s.clearance()
        assert np.all(got["min"] == v) and np.all(got["min_world"] == v) and np.all(got["witness"] == [CN.WORLD_BOX, 0, 0]), (k, got["min"])
    s.set_collision_world(None, boxes)
    got = s.clearance()
    assert np.all(got["min"] == -0.375) and np.all(got["witness"] == [CN.WORLD_BOX, 0, 3])
    # ... and moving with the arm: the same four boxes carried to the tool sphere's centre of each configuration
    s.set_collision_spheres([7], [[0.0, 0.0, 0.0, 0.125]])
    cen = CN.centres(model, q, [7], [[0.0, 0.0, 0.0, 0.125]])[:, 0]
    for i in range(3):
        moved = boxes.copy()
        moved[:, 9:12] += cen[i] - np.array([0.5, 0.25, 1.0])
        s.set_collision_world(None, moved)
        got = s.clearance(q[i:i + 1])
        assert abs(got["min"][0] + 0.375) <= BOUND * (1.125 + np.abs(cen[i]).max()) and tuple(got["witness"][0]) == (CN.WORLD_BOX, 0, 3)
        for k, v in enumerate(values):
            s.set_collision_world(None, moved[k:k + 1])
            assert abs(s.clearance(q[i:i + 1])["min"][0] - v) <= BOUND * (1.125 + np.abs(cen[i]).max()), (i, k)
    s.close()


# ---- 5. the q routes ----------------------------------------------------------------------------------------------------------------------
def test_q_routes_agree():
    c = _case("talos32")
    model, q, n = c["model"], c["q"], c["n"]
    s = _open(model, q)
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    res = s.clearance()
    host = s.clearance(q)
    dq = capi.DeviceArray(q)
    dev = s.clearance(dq)
    assert all(np.array_equal(res[k], host[k]) and np.array_equal(res[k], dev[k]) for k in res)
    # device outputs get what the host path gets; the witness may be left out
    hip = capi.DeviceArray.hip()
    dm, dw = capi.DeviceArray(np.full(3 * n, np.nan)), capi.DeviceArray(np.zeros((3 * n + 1) // 2))
    for wit in (dw, None):
        s.clearance(dq, out=(dm, wit))
        back = np.empty((n, 3))
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(dm.data_ptr()), back.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        assert np.array_equal(back, np.stack([res["min"], res["min_world"], res["min_self"]], axis=1))
    wb = np.empty((3 * n + 1) // 2)
    assert hip.hipMemcpy(wb.ctypes.data_as(C.c_void_p), C.c_void_p(dw.data_ptr()), wb.nbytes, 2) == 0
    assert np.array_equal(wb.view(np.int32)[:3 * n].reshape(n, 3), res["witness"])
    dm.free(); dw.free(); dq.free()
    # n != B with an explicit q, more rows than the batch included
    twice = s.clearance(np.concatenate([q[5:], q]))
    assert all(np.array_equal(twice[k], np.concatenate([res[k][5:], res[k]])) for k in res)
    assert s.clearance(np.zeros((0, model.nq)))["min"].shape == (0,)
    s.close()


def test_a_recorded_path_in_one_call():
    model = QC.model_of("panda7")
    B, T = 16, 3
    links = _links(model, 1)
    rng = np.random.default_rng(540)
    q0 = model.random_configurations(rng, B)
    wp = np.stack([P.fk12(model, np.clip(q0 + 0.05 * t * rng.normal(size=q0.shape), model.q_lo, model.q_hi), links) for t in range(T)], axis=1)
    s, _ = _handle(model, B, links, q0)
    lk, spheres = CN.make_spheres(model, 2, 541)
    s.set_collision_spheres(lk, spheres)
    s.set_collision_world(*_world(rng, 5, 5))
    s.set_self_collision(True)
    path = s.SolvePosePath(wp, tol_pose=1e-4, max_steps=8)
    rows = path["q_path"].reshape(-1, model.nq)
    assert np.isfinite(rows).all(axis=1).sum() >= B   # (the first waypoint is where each instance starts)
    got = s.clearance(rows)
    assert got["min"].shape == (B * T,)
    for i in range(B * T):
        one = s.clearance(rows[i:i + 1])
        assert all(np.array_equal(one[k][0], got[k][i], equal_nan=True) for k in got), i
    s.close()


# ---- 6. a row that is not finite ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["multidof20", "tree330"])
def test_a_nan_row_is_nan_and_alone(name):
    c = _case(name)
    q = c["q"].copy()
    s = _open(c["model"], q)
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    clean = s.clearance(q)
    for bad, value in ((1, np.nan), (0, np.inf)):
        qb = q.copy()
        qb[bad, c["model"].nq - 1] = value
        got = s.clearance(qb)
        for k in ("min", "min_world", "min_self"):
            assert np.isnan(got[k][bad])
        assert tuple(got["witness"][bad]) == (CN.NONE, -1, -1)
        keep = np.arange(q.shape[0]) != bad
        assert all(np.array_equal(got[k][keep], clean[k][keep]) for k in clean)
    s.close()


# ---- 7. neutrality ---------------------------------------------------------------------------------------------------------------------------
def test_the_model_and_the_query_change_no_solve():
    from test_multistart import SEED, TOL, _goal_rows, _mk, _robot
    model, links, lo, hi, _ = _robot("talos32")
    B, K = 64, 16
    q0g = _goal_rows("talos32", model, lo, hi, None, B // K, 61)
    tg = P.fk12(model, _goal_rows("talos32", model, lo, hi, None, B // K, 62), links)
    q_init = np.repeat(q0g, K, axis=0)
    lk, spheres = CN.make_spheres(model, 2, 551)
    rng = np.random.default_rng(552)
    res = []
    for with_model in (False, True):
        s = _mk(model, B, links, q_init, lo, hi)
        if with_model:
            s.set_collision_spheres(lk, spheres)
            s.set_collision_world(*_world(rng, 8, 8))
            s.set_self_collision(True)
            s.clearance()
        s.Solve()
        out = [s.get("z"), s.get("iter")]
        if with_model:
            s.clearance()
        p = s.SolvePose(np.repeat(tg, K, axis=0), tol_pose=TOL, max_steps=6)
        out += [s.get("q"), p["status"], p["err"]]
        if with_model:
            s.clearance()
        m = s.SolvePoseMultiStart(tg, K, rounds=2, seed=SEED, q0=q0g, tol_pose=TOL, max_steps=6)
        out += [m[k] for k in ("winner", "goal_status", "q", "err", "cost", "nreached", "round")]
        assert "clearance" not in m
        res.append(out)
        s.close()
    assert all(np.array_equal(a, b) for a, b in zip(*res))


# ---- 8. validation ---------------------------------------------------------------------------------------------------------------------------
def _raises(code, text, fn, *a, **kw):
    with pytest.raises(capi.LoikError) as e:
        fn(*a, **kw)
    assert e.value.code == code and text in str(e.value), (e.value.code, str(e.value))


def test_errors_leave_the_model_as_it_was():
    c = _case("panda7")
    model, q = c["model"], c["q"]
    nj, B = model.njoints, q.shape[0]
    # before anything is resident or set
    s = loik_amd.BatchedLoik(model, B, **dict(PRM, num_eq_c=1))
    _raises(ERR_STATE, "no spheres", s.clearance, q)
    _raises(ERR_STATE, "no spheres", s.set_multistart_clearance, 0.0)
    _raises(ERR_STATE, "no spheres", s.set_self_collision, True)
    s.set_collision_spheres([1], [[0, 0, 0, 0.1]])
    _raises(ERR_STATE, "resident", s.clearance)
    assert np.all(np.isposinf(s.clearance(q)["min"]))
    s.close()
    s = _open(model, q)
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True, ignore=[(1, 4)])
    s.set_multistart_clearance(0.02)
    before, npairs = s.clearance(), s.num_self_pairs()
    L, h = s.L, s.h
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    good_l, good_s = np.array([1, 2], dtype=np.int32), np.array([[0, 0, 0, 0.1], [0, 0, 0, 0.1]], dtype=float)

    def spheres(links, sph):
        s.set_collision_spheres(np.array(links, dtype=np.int32), np.array(sph, dtype=float))

    def bad_sphere(k, v):
        x = good_s.copy(); x[1, k] = v
        return x
    _raises(ERR_ARG, "sphere 1: link id", spheres, [1, nj], good_s)
    _raises(ERR_ARG, "sphere 1: link id", spheres, [1, -1], good_s)
    _raises(ERR_ARG, "sphere 1: a number is not finite", spheres, good_l, bad_sphere(0, np.nan))
    _raises(ERR_ARG, "sphere 1: a number is not finite", spheres, good_l, bad_sphere(3, np.inf))
    _raises(ERR_ARG, "sphere 1: negative radius", spheres, good_l, bad_sphere(3, -1e-3))
    _raises(ERR_ARG, "LOIKB_CLR_MAX_SPHERES", spheres, np.ones(capi.CLR_MAX_SPHERES + 1), np.tile(good_s[:1], (capi.CLR_MAX_SPHERES + 1, 1)))
    assert L.loikb_collision_set_spheres(h, None, good_s.ctypes.data_as(dp), 2) == ERR_ARG
    assert L.loikb_collision_set_spheres(h, good_l.ctypes.data_as(ip), None, 2) == ERR_ARG
    assert L.loikb_collision_set_spheres(h, good_l.ctypes.data_as(ip), good_s.ctypes.data_as(dp), -1) == ERR_ARG
    ws, wb = c["ws"][:2].copy(), c["wb"][:2].copy()

    def world(ws_, wb_):
        s.set_collision_world(ws_, wb_)

    def edit(a, i, k, v):
        x = a.copy(); x[i, k] = v
        return x
    _raises(ERR_ARG, "sphere 1: a number is not finite", world, edit(ws, 1, 1, np.nan), wb)
    _raises(ERR_ARG, "sphere 0: negative radius", world, edit(ws, 0, 3, -0.5), wb)
    _raises(ERR_ARG, "box 1: a number is not finite", world, ws, edit(wb, 1, 10, np.inf))
    _raises(ERR_ARG, "box 1: a half extent is not > 0", world, ws, edit(wb, 1, 13, 0.0))
    _raises(ERR_ARG, "box 0: a half extent is not > 0", world, ws, edit(wb, 0, 12, -0.1))
    _raises(ERR_ARG, "box 1: the rotation", world, ws, edit(wb, 1, 0, wb[1, 0] + 1e-6))
    mirrored = wb.copy(); mirrored[0, 0:3] *= -1.0   # orthonormal, determinant -1
    _raises(ERR_ARG, "box 0: the rotation", world, ws, mirrored)
    assert L.loikb_collision_set_world(h, None, 1, None, 0) == ERR_ARG and L.loikb_collision_set_world(h, None, 0, None, 1) == ERR_ARG
    assert L.loikb_collision_set_world(h, ws.ctypes.data_as(dp), -1, None, 0) == ERR_ARG and L.loikb_collision_set_world(h, None, 0, wb.ctypes.data_as(dp), -2) == ERR_ARG
    _raises(ERR_ARG, "ignore pair 1: link id", s.set_self_collision, True, [(1, 2), (3, nj)])
    _raises(ERR_ARG, "ignore pair 0: link id", s.set_self_collision, False, [(-1, 2)])
    assert L.loikb_collision_set_self_pairs(h, 1, None, 1) == ERR_ARG and L.loikb_collision_set_self_pairs(h, 1, None, -1) == ERR_ARG
    _raises(ERR_ARG, "finite margin", s.set_multistart_clearance, np.nan)
    _raises(ERR_ARG, "finite margin", s.set_multistart_clearance, np.inf)
    prm = capi.ClearanceParams(0.0, 1)
    assert L.loikb_clearance_set_multistart(h, C.byref(prm)) == ERR_ARG
    mins, wit = np.empty((B, 3)), np.empty((B, 3), dtype=np.int32)
    vp = C.c_void_p
    assert L.loikb_clearance(h, None, B - 1, 0, mins.ctypes.data_as(vp), wit.ctypes.data_as(vp), 0) == ERR_ARG and b"n == the batch" in L.loikb_last_error()
    assert L.loikb_clearance(h, q.ctypes.data_as(vp), -1, 0, mins.ctypes.data_as(vp), None, 0) == ERR_ARG
    assert L.loikb_clearance(h, q.ctypes.data_as(vp), B, 0, None, wit.ctypes.data_as(vp), 0) == ERR_ARG
    assert L.loikb_clearance(None, q.ctypes.data_as(vp), B, 0, mins.ctypes.data_as(vp), None, 0) == ERR_ARG
    assert L.loikb_clearance_get_multistart_result(h, capi.CLR_MS_F_CLEARANCE, mins.ctypes.data_as(vp), 0) == ERR_STATE
    # ... and after all of it the model, the pair list and the latch are what they were
    after = s.clearance()
    assert all(np.array_equal(before[k], after[k]) for k in before) and s.num_self_pairs() == npairs
    assert s.multistart_clearance() == dict(margin=0.02)
    # spheres gone: the query, the latch and a latched multi-start say so
    s.set_collision_spheres([], np.zeros((0, 4)))
    _raises(ERR_STATE, "no spheres", s.clearance)
    _raises(ERR_STATE, "no spheres", s.set_multistart_clearance, 0.0)
    _raises(ERR_STATE, "no spheres", s.set_self_collision, True)
    s.set_joint_limits(model.q_lo, model.q_hi)
    _raises(ERR_STATE, "no spheres", s.SolvePoseMultiStart, P.fk12(model, q[:1], [model.njoints - 1])[0], B)
    s.clear_multistart_clearance()
    assert s.multistart_clearance() is None
    s.close()
