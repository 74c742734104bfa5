"""GPU: the two queries of include/loik_amd_avoid.h -- loikb_avoid_box and loikb_clearance_gradient -- against the numpy reference of
tests/avoid_numpy.py (proven on the CPU by test_avoid_numpy.py), on the eight robots, worlds and configurations of test_clearance._case:
a chain, trees, nq != nv, helical / prismatic joints, the 170-DoF tree whose DoFs stride past one wavefront, the 330-joint tree that
takes the placements of every joint from HBM, composite joints; then the sizes at which the kernel changes its path, the q and output
routes, a NaN row and the validation.

The rows on which a reference decision lies within 1e-9 of its threshold (avoid_numpy's `near`) are left out of the box and gradient
comparisons, at most 2 % of them; test_avoid_numpy.py asserts that share for these very inputs without a GPU."""
import ctypes as C

import numpy as np
import pytest

from loik_amd import capi

import avoid_numpy as AN
import clearance_numpy as CN
import qp_cases as QC
import test_clearance as TC

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -20, -24
BOUND = TC.BOUND
PRM = dict(d_safe=0.02, d_influence=0.15, kappa=0.5)
DT = 0.25
# The finite entries of lo / hi with an unbounded base box are A_lo / A_hi themselves, -r / (m g): the relative error is that of g, a sum
# of products that may cancel.  |got - want| <= BOX_BOUND * |want|, BOX_BOUND = 16 times the largest relative error measured on one
# MI355X over the eight robots (profiles/avoidance_measured.md), the allowance for another compiler's rounding; GRAD_BOUND likewise for
# |grad - want| / scale, scale = 1 + max |centre| + max r as in test_clearance.py
BOX_MEASURED = 7.298e-12
GRAD_MEASURED = 8.592e-15
BOX_BOUND, GRAD_BOUND = 16 * BOX_MEASURED, 16 * GRAD_MEASURED
NEAR_SHARE = 0.02
_REFS = {}


def _setup(name):
    """test_clearance._case, cut to the first LOIKB_AVOID_MAX_SPHERES spheres where it has more (tree330: 329)"""
    c = dict(TC._case(name))
    if len(c["links"]) > capi.AVOID_MAX_SPHERES:
        c["links"], c["spheres"] = c["links"][:capi.AVOID_MAX_SPHERES], c["spheres"][:capi.AVOID_MAX_SPHERES]
        c["pairs"] = CN.self_pairs(c["model"].parents, c["links"])
    return c


def _ref(name):
    """the numpy answers of one robot, computed once: the box over an unbounded base, and the gradient"""
    if name not in _REFS:
        c = _setup(name)
        args = (c["model"], c["q"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"])
        box = AN.avoidance_box(*args, DT, -np.inf, np.inf, **PRM)
        _REFS[name] = dict(c=c, box=box, grad=AN.clearance_gradient(*args))
    return _REFS[name]


def _open_case(c, precision=capi.F64, q=None):
    s = TC._open(c["model"], c["q"] if q is None else q, precision)
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    return s


def _scale(cen, spheres):
    return 1.0 + float(np.max(np.abs(cen))) + float(np.max(np.asarray(spheres)[:, 3]))


def _rel(got, want, what):
    """the infinities equal exactly; the largest |got - want| / |want| over the finite entries (an exact zero must be one)"""
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), what
    g, w = got[~inf], want[~inf]
    zero = w == 0.0
    assert np.all(g[zero] == 0.0), what
    return float(np.max(np.abs(g[~zero] - w[~zero]) / np.abs(w[~zero]), initial=0.0))


def _compare_box(got, ref, keep, scale, what):
    """partners equal and lo / hi within BOX_BOUND on the rows `keep`; the per-sphere clearances within BOUND * scale on every row.  Returns the
    largest relative error of lo / hi"""
    want = ref["box"]
    inf = np.isposinf(want["pairs"])
    assert np.array_equal(np.isposinf(got["pairs"]), inf), what
    e = float(np.max(np.abs(got["pairs"][~inf] - want["pairs"][~inf]), initial=0.0))
    assert e <= BOUND * scale, (what, e, scale)
    assert np.array_equal(got["partner"][keep], want["partner"][keep]), what
    assert np.all(got["lo"] <= 0.0) and np.all(got["hi"] >= 0.0), what
    worst = max(_rel(got["lo"][keep], want["lo"][keep], what), _rel(got["hi"][keep], want["hi"][keep], what))
    print("avoidance_measured %s box: max relative error %.3e over %d rows (%d near left out), clearances %.3e / scale %.3f" %
          (what, worst, int(keep.sum()), int((~keep).sum()), e, scale))
    assert worst <= BOX_BOUND, (what, worst)
    return worst


# ---- 1. against numpy on eight robots ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.ROBOTS))
def test_avoidance_box_matches_numpy(name):
    ref = _ref(name)
    c = ref["c"]
    s = _open_case(c)
    keep = ~ref["box"]["near"]
    assert (~keep).mean() <= NEAR_SHARE
    scale = _scale(ref["box"]["centres"], c["spheres"])
    got = s.avoidance_box(None, DT, -np.inf, np.inf, **PRM)
    _compare_box(got, ref, keep, scale, name)
    assert any(len(r) > 0 for r in ref["box"]["cons"]) and np.isinf(ref["box"]["lo"]).any() and np.isfinite(ref["box"]["lo"]).any()
    # the clamp into a finite base box, per DoF: where the reference sits on a bound the device does exactly, elsewhere as above
    lb = -np.linspace(0.5, 1.0, c["model"].nv)
    got1 = s.avoidance_box(c["q"], DT, lb, 1.0, **PRM)
    lo1, hi1 = np.maximum(ref["box"]["lo"], lb), np.minimum(ref["box"]["hi"], 1.0)
    for g, w, edge in ((got1["lo"], lo1, np.broadcast_to(lb, lo1.shape)), (got1["hi"], hi1, np.ones_like(hi1))):
        on = (w == edge) & keep[:, None]
        assert np.array_equal(g[on], w[on]), name
        off = ~(w == edge) & keep[:, None]
        assert np.all(np.abs(g[off] - w[off]) <= BOX_BOUND * np.abs(w[off])), name
    assert np.array_equal(got1["pairs"], got["pairs"]) and np.array_equal(got1["partner"], got["partner"])
    # fp64 from the fp64 q whatever the handle's precision: the query does not round
    s32 = _open_case(c, capi.F32)
    got32 = s32.avoidance_box(c["q"], DT, -np.inf, np.inf, **PRM)
    assert all(np.array_equal(got[k], got32[k]) for k in got)
    s.close(); s32.close()


@pytest.mark.parametrize("name", list(TC.ROBOTS))
def test_clearance_gradient_matches_numpy(name):
    ref = _ref(name)
    c, want = ref["c"], ref["grad"]
    s = _open_case(c)
    got, plain = s.clearance_gradient(), s.clearance()
    for k in ("min", "min_world", "min_self", "witness"):   # the same bits as loikb_clearance
        assert np.array_equal(got[k], plain[k]), (name, k)
    TC._compare(got, want, c["spheres"], name + " gradient")
    keep = ~want["near"]
    assert (~keep).mean() <= NEAR_SHARE
    assert np.array_equal(got["witness"][keep], want["witness"][keep])
    scale = _scale(want["centres"], c["spheres"])
    e = float(np.max(np.abs(got["grad"][keep] - want["grad"][keep]))) / scale
    print("avoidance_measured %s gradient: max |grad - numpy| / scale %.3e, scale %.3f" % (name, e, scale))
    assert e <= GRAD_BOUND, (name, e)
    assert np.array_equal(got["grad"][keep] == 0.0, want["grad"][keep] == 0.0)   # the columns off the pair's path are exactly 0
    assert np.any(want["grad"][keep] != 0.0)
    again = s.clearance_gradient(c["q"][:3])
    assert all(np.array_equal(again[k], got[k][:3]) for k in got)
    s.close()


# ---- 2. the sizes at which the kernel can go wrong ---------------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, capi.AVOID_MAX_SPHERES]
SIZE_WORLDS = (((1, 0), False), ((0, 1), False), ((33, 32), True), ((0, 0), True))   # ((world spheres, boxes), self pairs on)
_INPUTS, _INPUT_REFS = {}, {}


def size_inputs(ns):
    """the inputs of test_sizes[ns], computed once: panda7, the spheres dealt round-robin to the links 0..7 (every eighth sphere is on the
    universe), one world per entry of SIZE_WORLDS; 65 configurations, 9 at the largest size (both leave a last workgroup with idle
    wavefronts; the reference is O(n ns^2))"""
    if ns not in _INPUTS:
        model = QC.model_of("panda7")
        rng = np.random.default_rng(600 + ns)
        q = model.random_configurations(rng, 65 if ns <= 65 else 9)
        links = np.arange(ns, dtype=np.int32) % model.njoints
        _, spheres = CN.make_spheres(model, 1, 601 + ns, links=links)
        pairs_on = CN.self_pairs(model.parents, links)
        out = []
        for split, self_on in SIZE_WORLDS:
            if split == (0, 0) and not pairs_on:
                continue
            ws, wb = TC._world(rng, *split)
            pairs = pairs_on if self_on else []
            out.append(dict(what="panda7 ns=%d world=%d+%d self=%d" % (ns, split[0], split[1], len(pairs)), model=model, q=q, links=links, spheres=spheres,
                            ws=ws, wb=wb, pairs=pairs, split=split, self_on=self_on))
        _INPUTS[ns] = out
    return _INPUTS[ns]


def one_pair_input():
    """the input of test_one_self_pair: panda7, a sphere on link 1 and one on link 5, no world"""
    if "one pair" not in _INPUTS:
        model = QC.model_of("panda7")
        q = model.random_configurations(np.random.default_rng(620), 65)
        lk, spheres = CN.make_spheres(model, 1, 621, links=[1, 5])
        spheres[:, 3] = 0.3   # (so that the pair is under d_influence in some configurations)
        _INPUTS["one pair"] = dict(what="panda7 one self pair", model=model, q=q, links=lk, spheres=spheres, ws=np.zeros((0, 4)), wb=np.zeros((0, 15)),
                                   pairs=CN.self_pairs(model.parents, lk))
    return _INPUTS["one pair"]


def input_ref(inp):
    """the numpy answers of one of those inputs, computed once: dict(box, grad) as _ref"""
    if inp["what"] not in _INPUT_REFS:
        args = (inp["model"], inp["q"], inp["links"], inp["spheres"], inp["ws"], inp["wb"], inp["pairs"])
        _INPUT_REFS[inp["what"]] = dict(box=AN.avoidance_box(*args, DT, -np.inf, np.inf, **PRM), grad=AN.clearance_gradient(*args))
    return _INPUT_REFS[inp["what"]]


def _check_against_numpy(s, inp):
    """the box and the gradient of the handle's resident q against input_ref(inp), on the rows that are not near: at most NEAR_SHARE of
    them for either (with 9 rows: none), which test_avoid_numpy.py asserts for these inputs without a GPU"""
    what, q, spheres = inp["what"], inp["q"], inp["spheres"]
    ref = input_ref(inp)
    want, wg = ref["box"], ref["grad"]
    keep, kg = ~want["near"], ~wg["near"]
    assert (~keep).mean() <= NEAR_SHARE and (~kg).mean() <= NEAR_SHARE, (what, int((~keep).sum()), int((~kg).sum()))
    got = s.avoidance_box(None, DT, -np.inf, np.inf, **PRM)
    _compare_box(got, ref, keep, _scale(want["centres"], spheres), what)
    gg, plain = s.clearance_gradient(), s.clearance()
    assert all(np.array_equal(gg[k], plain[k]) for k in plain), what
    assert np.array_equal(gg["witness"][kg], wg["witness"][kg]), what
    assert np.all(np.abs(gg["grad"][kg] - wg["grad"][kg]) <= GRAD_BOUND * _scale(wg["centres"], spheres)), what
    for n in (3, 1):   # an explicit q, n != B: a last workgroup with idle wavefronts
        sub = s.avoidance_box(q[:n], DT, -np.inf, np.inf, **PRM)
        assert all(np.array_equal(sub[k], got[k][:n]) for k in got), (what, n)
    return got, want


@pytest.mark.parametrize("ns", SIZES)
def test_sizes(ns):
    """size_inputs(ns): one world object (a sphere, then a box) and 65, self pairs off and on; a sphere on link 0 constrains nothing against
    the world; the resident configurations, then 3 and 1 of them"""
    inputs = size_inputs(ns)
    model, q, links, spheres = (inputs[0][k] for k in ("model", "q", "links", "spheres"))
    s = TC._open(model, q)
    s.set_collision_spheres(links, spheres)
    for inp in inputs:
        s.set_collision_world(inp["ws"], inp["wb"])
        s.set_self_collision(inp["self_on"])
        got, want = _check_against_numpy(s, inp)
        if not inp["self_on"]:
            assert np.all(np.isposinf(got["pairs"][:, :, 1])) and np.all(got["partner"][:, :, 1] == -1)
        if inp["split"] == (0, 0):
            assert np.all(np.isposinf(got["pairs"][:, :, 0])) and np.all(got["partner"][:, :, 0] == -1)
        # a sphere on link 0 moves with no DoF: against the world it narrows nothing
        on0 = [a for a in range(ns) if links[a] == 0]
        for i in range(3):
            for cst in want["cons"][i]:
                if cst["a"] in on0 and cst["kind"] == 0:
                    assert cst["m"] == 0 and not np.any(cst["g"])
    s.close()


def test_one_self_pair():
    inp = one_pair_input()
    assert len(inp["pairs"]) == 1
    s = TC._open(inp["model"], inp["q"])
    s.set_collision_spheres(inp["links"], inp["spheres"])
    s.set_self_collision(True)
    got, want = _check_against_numpy(s, inp)
    assert any(len(r) for r in want["cons"])
    assert np.all(got["partner"][:, 0, 1] == 1) and np.all(got["partner"][:, 1, 1] == -1)
    # DoF 0 is on both root paths: exactly 0, it is never narrowed
    assert np.all(np.isinf(got["lo"][:, 0])) and np.all(np.isinf(got["hi"][:, 0]))
    s.close()


# ---- 3. routes, a NaN row, validation --------------------------------------------------------------------------------------------------
def _back(dev, shape, dtype=np.float64):
    """the contents of a capi.DeviceArray (doubles underneath) as `dtype` [shape]"""
    raw = np.empty(dev.size)
    assert capi.DeviceArray.hip().hipMemcpy(raw.ctypes.data_as(C.c_void_p), C.c_void_p(dev.data_ptr()), raw.nbytes, 2) == 0   # hipMemcpyDeviceToHost
    return raw.view(dtype)[:int(np.prod(shape))].reshape(shape)


def _ints(count):
    return capi.DeviceArray(np.zeros((count + 1) // 2))


def test_device_and_host_routes_agree():
    ref = _ref("multidof13")
    c = ref["c"]
    s = _open_case(c)
    n, nv, ns = c["n"], c["model"].nv, len(c["links"])
    res = s.avoidance_box(None, DT, -np.inf, np.inf, **PRM)
    host = s.avoidance_box(c["q"], DT, -np.inf, np.inf, **PRM)
    rg, hg = s.clearance_gradient(), s.clearance_gradient(c["q"])
    dq = capi.DeviceArray(c["q"])
    dev, dg = s.avoidance_box(dq, DT, -np.inf, np.inf, **PRM), s.clearance_gradient(dq)
    assert all(np.array_equal(res[k], host[k]) and np.array_equal(res[k], dev[k]) for k in res)
    assert all(np.array_equal(rg[k], hg[k]) and np.array_equal(rg[k], dg[k]) for k in rg)
    outs = (capi.DeviceArray(np.zeros((n, nv))), capi.DeviceArray(np.zeros((n, nv))), capi.DeviceArray(np.zeros((n, ns, 2))), _ints(2 * n * ns))
    s.avoidance_box(dq, DT, -np.inf, np.inf, out=outs, **PRM)
    assert np.array_equal(_back(outs[0], (n, nv)), res["lo"]) and np.array_equal(_back(outs[1], (n, nv)), res["hi"])
    assert np.array_equal(_back(outs[2], (n, ns, 2)), res["pairs"]) and np.array_equal(_back(outs[3], (n, ns, 2), np.int32), res["partner"])
    gouts = (capi.DeviceArray(np.zeros((n, 3))), _ints(3 * n), capi.DeviceArray(np.zeros((n, nv))))
    s.clearance_gradient(dq, out=gouts)
    assert np.array_equal(_back(gouts[0], (n, 3)), np.stack([rg["min"], rg["min_world"], rg["min_self"]], axis=1))
    assert np.array_equal(_back(gouts[1], (n, 3), np.int32), rg["witness"]) and np.array_equal(_back(gouts[2], (n, nv)), rg["grad"])
    for a in outs + gouts + (dq,):
        a.free()
    s.close()


def test_a_nan_row_is_alone():
    ref = _ref("panda7")
    c = ref["c"]
    q = np.array(c["q"])
    q[7, 2] = np.nan
    q[20, 0] = np.inf
    s = _open_case(c, q=q)
    lb = -np.ones(c["model"].nv)
    got, clean = s.avoidance_box(None, DT, lb, 1.0, **PRM), s.avoidance_box(c["q"], DT, lb, 1.0, **PRM)
    gg, gclean = s.clearance_gradient(), s.clearance_gradient(c["q"])
    ok = np.ones(c["n"], dtype=bool)
    ok[[7, 20]] = False
    for k in got:
        assert np.array_equal(got[k][ok], clean[k][ok]), k
    for k in gg:
        assert np.array_equal(gg[k][ok], gclean[k][ok]), k
    for i in (7, 20):   # the base interval, NaN clearances, no partner; a NaN gradient row with loikb_clearance's NaN answer
        assert np.array_equal(got["lo"][i], lb) and np.all(got["hi"][i] == 1.0)
        assert np.all(np.isnan(got["pairs"][i])) and np.all(got["partner"][i] == -1)
        assert np.all(np.isnan(gg["grad"][i])) and np.isnan(gg["min"][i]) and tuple(gg["witness"][i]) == (CN.NONE, -1, -1)
    s.close()


def _err(fn, code):
    with pytest.raises(capi.LoikError) as e:
        fn()
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def test_errors_leave_the_latch_and_the_model_as_they_were():
    ref = _ref("panda7")
    c = ref["c"]
    s = TC._open(c["model"], c["q"])
    # state: no spheres yet
    _err(lambda: s.set_collision_avoidance(**PRM), ERR_STATE)
    _err(lambda: s.clearance_gradient(), ERR_STATE)
    _err(lambda: s.avoidance_box(None, DT, -1.0, 1.0, **PRM), ERR_STATE)
    assert s.collision_avoidance() is None
    s.set_collision_spheres(c["links"], c["spheres"])
    s.set_collision_world(c["ws"], c["wb"])
    s.set_self_collision(True)
    before = s.avoidance_box(None, DT, -1.0, 1.0, **PRM)
    # arguments
    for bad in (dict(PRM, d_safe=np.nan), dict(PRM, d_influence=np.inf), dict(PRM, d_influence=PRM["d_safe"]), dict(PRM, kappa=0.0),
                dict(PRM, kappa=1.5), dict(PRM, kappa=np.nan)):
        _err(lambda: s.set_collision_avoidance(**bad), ERR_ARG)
        _err(lambda: s.avoidance_box(None, DT, -1.0, 1.0, **bad), ERR_ARG)
        assert s.collision_avoidance() is None
    for dt in (0.0, -1.0, np.inf, np.nan):
        _err(lambda: s.avoidance_box(None, dt, -1.0, 1.0, **PRM), ERR_ARG)
    _err(lambda: s.avoidance_box(None, DT, 1.0, -1.0, **PRM), ERR_ARG)
    _err(lambda: s.avoidance_box(None, DT, np.nan, 1.0, **PRM), ERR_ARG)
    prm = capi.AvoidParams(PRM["d_safe"], PRM["d_influence"], PRM["kappa"], 1)
    assert s.L.loikb_avoid_set(s.h, prm) == ERR_ARG
    assert s.L.loikb_clearance_gradient(s.h, None, 3, 0, None, None, None, 0) == ERR_ARG    # q = NULL needs n == B (arguments before state)
    assert s.L.loikb_clearance_gradient(s.h, None, -1, 0, None, None, None, 0) == ERR_ARG
    assert s.L.loikb_clearance_gradient(s.h, None, 0, 0, None, None, None, 0) == ERR_ARG    # (n != B)
    assert s.L.loikb_avoid_get_result(s.h, 7, before["lo"].ctypes.data, 0) == ERR_ARG
    assert s.L.loikb_avoid_get_result(s.h, capi.AVOID_F_MIN_SEEN, before["lo"].ctypes.data, 0) == ERR_STATE
    # the latch, and the sphere model under it
    s.set_collision_avoidance(**PRM)
    assert s.collision_avoidance() == PRM
    _err(lambda: s.set_collision_avoidance(**dict(PRM, kappa=2.0)), ERR_ARG)
    assert s.collision_avoidance() == PRM
    many = np.zeros(capi.AVOID_MAX_SPHERES + 1, dtype=np.int32)
    msg = _err(lambda: s.set_collision_spheres(many, np.tile([0.0, 0.0, 0.0, 0.01], (many.size, 1))), ERR_STATE)
    assert str(capi.AVOID_MAX_SPHERES) in msg
    _err(lambda: s.set_collision_spheres([], np.zeros((0, 4))), ERR_STATE)
    assert s.collision_avoidance() == PRM
    after = s.avoidance_box(None, DT, -1.0, 1.0, **PRM)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    s.clear_collision_avoidance()
    assert s.collision_avoidance() is None
    # without the latch the collision model takes more spheres than the avoidance kernel; the setter then names the limit
    s.set_collision_spheres(many, np.tile([0.0, 0.0, 0.0, 0.01], (many.size, 1)))
    msg = _err(lambda: s.set_collision_avoidance(**PRM), ERR_STATE)
    assert str(capi.AVOID_MAX_SPHERES) in msg
    _err(lambda: s.clearance_gradient(), ERR_STATE)
    assert np.isfinite(s.clearance()["min"]).all()
    s.close()
