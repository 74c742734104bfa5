"""The inputs of tests/test_grid_routes.py (GPU) and of the CPU tests that tie their references to the geometry (test_grid_numpy.py): four
robots in the light world of test_grid_clearance.case -- three world spheres, two boxes, the self pairs and a sparse grid of 25 x 21 x 17
voxels of 6 cm -- as segments, paths to shorten, planning queries and paths to blend, each with the numpy answer with the grid
(grid_numpy.advance and the references that call it) and the same call without it.  Every answer is computed once."""
import numpy as np

import blend_numpy as BN
import clearance_numpy as CN
import grid_numpy as GN
import motion_numpy as MN
import plan_numpy as PN
import pose_limits_numpy as PL
import pose_numpy as P
import qp_cases as QC
import shortcut_numpy as SN
import test_blend_numpy as TB
import test_clearance as TC
import test_grid_clearance as TG
import test_motion_clearance as TM
import test_plan_numpy as TP
import test_retime_numpy as TR
import test_shortcut as TS

SMALL = ("panda7", "talos32", "multidof13")      # the LDS builds
SLAB = "tree330"                                 # the slab builds
ROBOTS = SMALL + (SLAB,)
# panda7 with one small sphere on each link: no two of them overlap, so that the margin is above zero and a FREE segment lies outside the
# occupied cubes altogether (CPU only: test_grid_numpy.py)
CLEAR = "panda7-clear"
_ALL = ROBOTS + (CLEAR,)
SIZES = (1, 63, 64, 65, 130)
SIZES_RNG = 1640   # (1440 + 64 draws a world sphere over a sphere of the universe: a pair that never moves decides every segment)
TOL, MAX_EVALS = 1e-3, 24
# the share of occupied voxels: less leaves too few voxel witnesses among the corners of a blend and the segments of a shortcut (panda7,
# multidof13), and talos32 and tree330, whose self pairs lie far below zero, next to no segment that a voxel
# decides
FRAC = {"panda7": 0.01, "talos32": 0.15, "multidof13": 0.01, "tree330": 0.2, "sizes": 0.02, CLEAR: 0.002}
# the samples of a segment: talos32 decides every segment within 18, so that 12 leave some UNDECIDED (test_motion_clearance's number)
EVALS_MOTION = {"talos32": 12}
# the quantile of the clearance at the inputs that is the margin: of the segments' starts, of the waypoints to shorten and of the ends to
# plan between (test_shortcut's and test_plan_numpy's 10 %), of the waypoints to blend (test_blend_numpy's 20 %)
Q_MOTION, Q_PATHS, Q_BLEND = 0.15, 0.1, TB.QUANTILE
T_PATH, T_PLAN, ROUNDS, SEED = TS.T_PATH, TP.T_PLAN, TS.ROUNDS, TS.SEED
# per robot: paths to shorten, queries (test_plan.ROBOTS' goals and parameters for the slab robot), paths to blend
BATCH = {"panda7": (16, 16, 5), "talos32": (16, 16, 5), "multidof13": (16, 16, 5), "tree330": (2, 2, 2), CLEAR: (8, 8, 5)}
PLAN_OVER = {"tree330": (0.03, dict(max_iters=4, step=0.05, margin=-1.0))}

_CASES = {}


def _margin(c, q, quantile):
    """the quantile of the reference clearance at q; the clear world: 5 mm, whatever the inputs"""
    return 0.005 if c["name"] == CLEAR else float(np.quantile(clearance_at(c, q), quantile))


def _memo(fn):
    def wrapped(*key):
        k = (fn.__name__,) + key
        if k not in _CASES:
            _CASES[k] = fn(*key)
        return _CASES[k]
    wrapped.__doc__ = fn.__doc__
    return wrapped


@_memo
def world(name):
    """the model, q, spheres and self pairs of test_clearance._case, the world and a grid as test_grid_clearance.case has them"""
    c = {k: v for k, v in TC._case(_robot(name)).items() if k != "want"}
    c["name"] = name
    if name == CLEAR:
        model = c["model"]
        c["links"], c["spheres"] = CN.make_spheres(model, 1, 1520, links=np.arange(1, model.njoints, dtype=np.int32))
        c["spheres"][:, 3] *= 0.4
        c["pairs"] = CN.self_pairs(model.parents, c["links"])
        c["q"] = c["q"][:33]
    c["ws"], c["wb"] = TC._world(np.random.default_rng(900), 3, 2)
    c["grid"] = TG._grid(1401 + _ALL.index(name), frac=FRAC[name])
    return c


def _robot(name):
    return name.split("-")[0]


def world_args(c, grid=True):
    """(links, spheres, ws, wb, grid, pairs) as grid_numpy takes them"""
    return c["links"], c["spheres"], c["ws"], c["wb"], c["grid"] if grid else None, c["pairs"]


def clearance_at(c, q):
    """[n]: the reference clearance of configurations q in the whole world of c"""
    return GN.clearance(c["model"], q, *world_args(c))["min"]


def exact_clearance_at(c, q, depth=True):
    """[n]: the least exact clearance of configurations q against the spheres, the boxes and the self pairs (motion_numpy.clearance_min) and
    against the union of the occupied cubes: the geometry itself, not the pair of the header.  depth: the signed distance to the cubes,
    below zero by the depth inside them (grid_numpy.exact_clearance); without it the distance, zero inside them, which is what the
    header promises a bound of (`where v <= 0 it is not a penetration depth`)"""
    if "cubes" not in c:
        c["cubes"] = GN.cubes(c["grid"])
    spheres = np.asarray(c["spheres"], dtype=float)
    if depth:
        cubes = GN.exact_clearance(c["model"], q, c["links"], spheres, c["grid"], c["cubes"])
    else:
        d = GN.exact_distance(MN.centres(c["model"], np.atleast_2d(q), c["links"], spheres), c["grid"], c["cubes"])
        cubes = (np.maximum(d, 0.0) - spheres[None, :, 3]).min(axis=1)
    return np.minimum(MN.clearance_min(c["model"], q, c["links"], spheres, c["ws"], c["wb"], c["pairs"]), cubes)


def _segments(c, size, seed, quantile, max_evals=MAX_EVALS):
    model, qa = c["model"], c["q"]
    c["qa"] = qa
    c["dv"] = size * np.random.default_rng(seed).uniform(-1.0, 1.0, size=(qa.shape[0], model.nv))
    c["margin"] = _margin(c, qa, quantile) - 2.0 * TOL   # (less 2 tol: a pair that never moves does not block every segment)
    c["kw"] = dict(margin=c["margin"], tol=TOL, max_evals=max_evals)
    a = world_args(c)
    c["want"] = GN.advance(model, qa, c["dv"], *a, **c["kw"])
    if c["name"] != SLAB:
        c["plain"] = MN.advance(model, qa, c["dv"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], **c["kw"])
    # the route by end points: the device takes its own difference, the reference motion_numpy's
    c["qb"] = np.ascontiguousarray(np.stack([MN.interpolate(model, qa[i], c["dv"][i], 1.0) for i in range(qa.shape[0])]))
    c["want_path"] = GN.advance(model, qa, MN.difference(model, qa, c["qb"]), *a, **c["kw"])
    cen = np.concatenate([MN.centres(model, qa, c["links"], c["spheres"]), MN.centres(model, c["qb"], c["links"], c["spheres"])])
    c["scale"] = 1.0 + float(np.max(np.abs(cen))) + float(np.max(c["spheres"][:, 3]))
    return c


@_memo
def motion_case(name):
    """one segment from every q of the world: dv = test_motion_clearance.SIZE * uniform(-1, 1), the margin = the 15 % quantile of the
    clearance at the starts, tol 1e-3, 24 samples"""
    return _segments(dict(world(name)), TM.SIZE[_robot(name)], 1420 + _ALL.index(name), Q_MOTION, EVALS_MOTION.get(name, MAX_EVALS))


@_memo
def sizes_case(ns):
    """test_grid_clearance.test_sizes' set-up: panda7, ns spheres dealt round-robin to the links 0 .. 7 (the universe included), one world
    sphere, one box, a grid, the self pairs; 17 segments"""
    model = QC.model_of("panda7")
    rng = np.random.default_rng(SIZES_RNG + ns)
    links = np.arange(ns, dtype=np.int32) % model.njoints
    _, spheres = CN.make_spheres(model, 1, 1450 + ns, links=links)
    ws, wb = TC._world(rng, 1, 1)
    c = dict(name="panda7 ns=%d" % ns, model=model, n=17, q=model.random_configurations(rng, 17), links=links, spheres=spheres, ws=ws, wb=wb,
             pairs=CN.self_pairs(model.parents, links), grid=TG._grid(1460 + ns, frac=FRAC["sizes"]))
    return _segments(c, TM.SIZE["panda7"], 1470 + ns, Q_MOTION)


@_memo
def shortcut_case(name):
    """paths of six waypoints from the first q of the world as test_shortcut.shortcut_case draws them; eight rounds (four on the slab robot)"""
    c = dict(world(name))
    model = c["model"]
    B = BATCH[name][0]
    c["B"], c["paths"] = B, TS.make_paths(model, c["q"][:B], TM.SIZE[_robot(name)], T_PATH, np.random.default_rng(1480 + _ALL.index(name)))
    c["margin"] = _margin(c, c["paths"].reshape(-1, model.nq), Q_PATHS)
    c["kw"] = dict(rounds=4 if name == SLAB else ROUNDS, seed=SEED, margin=c["margin"], tol=TOL, max_evals=MAX_EVALS)
    a = (model, c["paths"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"])
    c["want"] = SN.shortcut(*a, grid=c["grid"], **c["kw"])
    # every segment the rule tried, (path, row i, row j) in path order, and its advancement on its own, with the grid and without it
    c["tried"] = [(b, i, j) for b in range(B) for i, j, _ in c["want"]["segments"][b]]
    qa, qb = np.stack([c["paths"][b, i] for b, i, j in c["tried"]]), np.stack([c["paths"][b, j] for b, i, j in c["tried"]])
    mkw = dict(margin=c["margin"], tol=TOL, max_evals=MAX_EVALS)
    c["tried_want"] = GN.advance(model, qa, MN.difference(model, qa, qb), *world_args(c), **mkw)
    assert c["tried_want"]["status"].tolist() == [st for b in range(B) for _, _, st in c["want"]["segments"][b]]
    if name != SLAB:
        c["plain"] = SN.shortcut(*a, **c["kw"])
        c["tried_plain"] = MN.advance(model, qa, MN.difference(model, qa, qb), c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], **mkw)
    return c


@_memo
def plan_case(name):
    """queries q[b] -> q[b + B] as test_plan_numpy.plan_case makes them (on the slab robot: test_plan's goals near the starts and its
    parameters), the ranges = the box of the ends widened by 0.5"""
    c = dict(world(name))
    model, q = c["model"], c["q"]
    B = BATCH[name][1]
    near, over = PLAN_OVER.get(name, (None, {}))
    c["B"], c["start"] = B, np.ascontiguousarray(q[:B])
    if near is None:
        c["goal"] = np.ascontiguousarray(q[B:2 * B])
    else:
        v = near * np.random.default_rng(1310).uniform(-1.0, 1.0, size=(B, model.nv))
        c["goal"] = np.ascontiguousarray(np.stack([P.integrate(model, a, d) for a, d in zip(c["start"], v)]))
    ends = np.concatenate([c["start"], c["goal"]])
    c["margin"] = _margin(c, ends, Q_PATHS)
    qi = PL.limit_q_index(model)
    ok = qi >= 0
    c["lo"], c["hi"] = np.full(model.nv, -np.inf), np.full(model.nv, np.inf)
    c["lo"][ok], c["hi"][ok] = ends[:, qi[ok]].min(axis=0) - 0.5, ends[:, qi[ok]].max(axis=0) + 0.5
    c["kw"] = dict(dict(step=0.5, max_iters=16, max_nodes=64, seed=SEED, margin=c["margin"], tol=TOL, max_evals=MAX_EVALS), **over)
    a = (model, c["start"], c["goal"], c["links"], c["spheres"], c["lo"], c["hi"], T_PLAN, c["ws"], c["wb"], c["pairs"])
    c["want"] = PN.plan(*a, grid=c["grid"], **c["kw"])
    if name != SLAB:
        c["plain"] = PN.plan(*a, **c["kw"])
    return c


@_memo
def blend_case(name):
    """paths of six waypoints as test_blend_numpy.make_paths shapes them, its limits, reach and parameters, the answer at S = 256"""
    c = dict(world(name))
    model = c["model"]
    B = BATCH[name][2]
    c["B"], c["paths"] = B, TB.make_paths(model, c["q"][:B], TM.SIZE[_robot(name)], T_PATH, np.random.default_rng(1500 + _ALL.index(name)))
    c["v_max"], c["a_max"] = TR.limits(_robot(name), model.nv)
    c["margin"] = _margin(c, c["paths"].reshape(-1, model.nq), Q_BLEND)
    c["kw"] = dict(dt=TB.DT, reach=TB.reach_of(_robot(name), model.nv), margin=c["margin"], tol=TOL, max_evals=MAX_EVALS, max_tries=TB.MAX_TRIES)
    a = (model, c["paths"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], c["v_max"], c["a_max"])
    c["want"] = BN.blend(*a, S=TB.S_ROWS, grid=c["grid"], **c["kw"])
    if name != SLAB:
        c["plain"] = BN.blend(*a, S=TB.S_ROWS, **c["kw"])
    return c


def kind4_share(witness):
    """the share of witnesses [..., 3] that name a voxel, among those that name a pair at all"""
    kind = np.asarray(witness)[..., 0].reshape(-1)
    named = kind != CN.NONE
    return float(np.sum(kind == GN.WORLD_GRID)) / max(int(named.sum()), 1)
