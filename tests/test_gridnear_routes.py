"""GPU: the grid branch of k_avoid_box's step mode (the wavefront-uniform m.g.F branch, ordinal nws + nwb, gridnear_cube in avd_entry) on
the routes of tests/test_avoid_routes.py: its workloads with a voxel grid beside their spheres and boxes, built as
gridnear_cases.pose_workload builds it (a cube within d_safe + 2 h of a sphere of some seed is taken out), latched in the order of
test_gridnear_pose._with_grid.  The referee is the lock-step oracle of avoid_numpy with the grid in its collision model
(avoid_numpy.constraints_of: gridnear_numpy.constraints), through the very helpers of test_avoid_routes.py.

  a. the route matrix: the tiles route after k_pose_limit_box / k_pose_dyn_box, the per-instance box and A, panda7 and the multi-DoF robot
  b. ragged batches B = 1, 5, 13 on the shared and the per-instance box, exact on every instance
  c. exact containment in fp64 and fp32 on the shared and the per-instance box, and on every engine
  d. the HBM route with a grid: the 330-joint tree of test_avoid_big.py with the box and voxel of gridnear_cases.avoid_case("tree330")'s
     grid, moved to where that workload's spheres are (hbm_case)
  e. SolvePosePath with a budget, f. TrackPose with feedforward="difference", g. step control (the three STEP_CASES), h. the three-round
     multi-start against the host-driven sequence bit for bit and against the oracle: the bodies of test_avoid_routes.py's tests

Every input is built without a GPU; tests/test_gridnear_routes_numpy.py asserts on the reference alone what makes each case a test."""
import numpy as np
import pytest

from loik_amd import capi

from test_engines import ENGINES
from test_pose_parity import ENGINE_ENV
from test_avoid_pose import AVOID, LAWS, TOL
import clearance_numpy as CN
import grid_numpy as GN
import gridnear_cases as GC
import gridnear_numpy as NN
import test_avoid_routes as R
import avoid_big_cases as BC

pytestmark = pytest.mark.gpu

_WORK = {}
LAW = LAWS[0]
GRID_FRAC = 0.02


# ---- the inputs (no GPU) ---------------------------------------------------------------------------------------------------------------------
def with_grid(w, grid, what, q=None):
    """the workload w with `grid` in its collision model, less the cubes within d_safe + 2 h of a sphere of some seed (q, by default the
    workload's q0): the bound v (at most sqrt(3) h under the distance) is above d_safe at every seed"""
    key = (what, id(w))
    if key not in _WORK:
        col = w["col"]
        cen = CN.centres(w["model"], w["q0"] if q is None else q, col["links"], col["spheres"])
        occ = np.array(grid.occ, dtype=np.uint8)
        for (uz, uy, ux), cube in zip(np.argwhere(grid.occ), GN.cubes(grid)):
            if np.min(CN.sphere_box(cen, col["spheres"][None, :, 3], cube)) < AVOID["d_safe"] + 2.0 * grid.h:
                occ[uz, uy, ux] = 0
        _WORK[key] = dict(w, col=dict(col, grid=NN.Grid(occ, grid.origin, grid.h)))
    return _WORK[key]


def _grid_of(seed):
    import test_grid_clearance as TG
    return TG._grid(seed, frac=GRID_FRAC)


# a. (test_avoid_routes.ROUTES row, the grid's seed): limits variants 1 and 2, the per-instance box and A, both robots
ROUTES = [(R.ROUTES[0], 3400), (R.ROUTES[3], 3410), (R.ROUTES[4], 3420), (R.ROUTES[7], 3430)]
ROUTE_STEPS = (1, 4)


def route_case(c):
    return with_grid(R.route_case(c[0]), _grid_of(c[1]), "route")


# b. (test_avoid_routes.RAGGED row, the grid's seed)
RAGGED_GRIDS = (3501, 3510, 3520, 3530, 3540, 3553)   # the first from 35x0 on for which test_gridnear_routes_numpy.test_ragged_inputs holds
RAGGED = list(zip(R.RAGGED, RAGGED_GRIDS))


def ragged_case(c):
    return with_grid(R.ragged_case(c[0]), _grid_of(c[1]), "ragged")


# c.
CONTAIN_GRID = 3600


def contain_case(box_inst):
    return with_grid(R.contain_case(box_inst), _grid_of(CONTAIN_GRID), "contain")


# d.
HBM_GRID, HBM_FRAC = 3700, 0.05


def hbm_case():
    """the tree330 / 100 row of test_avoid_big.py.  Its spheres sit on the links at the leaf end, metres from the base and elsewhere at
    every seed, so the grid of gridnear_cases.avoid_case("tree330") around the base is out of every sphere's reach: its box and voxel are
    kept, moved to the middle of the first seed's spheres, at a density that leaves cubes under d_influence after the thinning"""
    if "hbm grid" not in _WORK:
        w = BC.table_case(BC.row("tree330", 100))
        g = GC.avoid_case("tree330")["grid"]
        cen = CN.centres(w["model"], w["q0"][:1], w["col"]["links"], w["col"]["spheres"])[0]
        mid = 0.5 * (cen.min(axis=0) + cen.max(axis=0))
        occ = GN.random_occupancy(tuple(int(n) for n in g.n), HBM_FRAC, HBM_GRID)
        _WORK["hbm grid"] = GN.Grid(occ, mid - 0.5 * g.h * g.n.astype(float), g.h)
    return with_grid(BC.table_case(BC.row("tree330", 100)), _WORK["hbm grid"], "hbm")


# e. - h. the loops beside SolvePose: the workloads of test_avoid_routes.py, each with a grid (the seed beside it: the first from the
# round number on for which the conditions of test_gridnear_routes_numpy.py hold)
PATHS = list(zip(R.PATHS, (3800, 3810, 3820, 3830)))
TRACKS = list(zip(R.TRACKS, (3901, 3910, 3920, 3930)))
STEPS = list(zip(R.STEP_CASES, (4000, 4010, 4020)))
MS_GRID = 4103


def path_case(c):
    return with_grid(R.path_workload(*c[0]), _grid_of(c[1]), "path")


def track_case(c):
    return with_grid(R.track_workload(*c[0]), _grid_of(c[1]), "track")


def step_case(c):
    return with_grid(R.step_workload(c[0][0], c[0][1]), _grid_of(c[1]), "step")


def multistart_case():
    """test_avoid_routes.multistart_workload with a grid thinned around the seeds that round 0 draws"""
    import pose_multistart_numpy as M
    w = R.multistart_workload()
    q = M.sample(w["model"], w["q0g"], w["K"], R.MS_DRAW, 0, w["lo"], w["hi"])
    return with_grid(w, _grid_of(MS_GRID), "ms", q=q)


def grid_share(w, q=None):
    """the share of the instances with a grid pair among the entries under d_influence at the seed (the oracle's constraint list of the
    first step, kind grid)"""
    c = w["col"]
    cons = NN.constraints(w["model"], w["q0"] if q is None else q, c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], AVOID["d_influence"], c["grid"], d_safe=AVOID["d_safe"],
                          clamped=True)[0]
    nwo = c["ws"].shape[0] + c["wb"].shape[0]
    return float(np.mean([any(k["kind"] == 0 and k["partner"] == nwo for k in row) for row in cons]))


# ---- a. the route matrix -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ROUTES, ids=lambda c: R.route_id(c[0]))
def test_route_matrix_with_a_grid_matches_lockstep_oracle(case):
    w = route_case(case)
    for k in ROUTE_STEPS:
        out, q, o, same = R._solve_pose_parity(w, LAW[0], LAW[1], k, ("grid", R.route_id(case[0]), k), True)
        assert (o["avoid_active_steps"] > 0).mean() >= 0.25 and np.all(out["avoid_active_steps"] <= out["steps"])


# ---- b. ragged batches ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RAGGED, ids=lambda c: "B%d-%s" % (c[0][0], "boxinst" if c[0][1] else "boxsh"))
def test_ragged_batches_with_a_grid(case):
    w = ragged_case(case)
    out, q, o, same = R._solve_pose_parity(w, R.RAGGED_LAW[0], R.RAGGED_LAW[1], R.RAGGED_STEPS, ("grid ragged",) + case[0][:2], False, exact=True)
    assert not o["near"].any() and same.all()
    assert np.array_equal(out["avoid_flags"], o["avoid_flags"])


# ---- c. exact containment ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box_inst", [False, True], ids=["boxsh", "boxinst"])
@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
def test_z_is_inside_the_clamped_query_with_a_grid(precision, box_inst):
    R._check_containment(contain_case(box_inst), precision, ("grid", "f64" if precision == capi.F64 else "f32", "boxinst" if box_inst else "boxsh"))


@pytest.mark.parametrize("engine", list(ENGINES))
def test_every_engine_honours_the_box_narrowed_by_the_grid(engine, monkeypatch):
    for v in ENGINE_ENV:
        monkeypatch.delenv(v, raising=False)
    env, kw = ENGINES[engine]
    for v, x in env.items():
        monkeypatch.setenv(v, x)
    R._check_containment(contain_case(False), capi.F64, ("grid engine", engine), calls=2, **kw)


# ---- d. the HBM route ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [capi.F64, capi.F32], ids=["f64", "f32"])
def test_hbm_route_with_a_grid(precision):
    """k_avoid_box<true, AVD_STEP, *> with the grid branch: containment, and avoid_min_seen of one step is clearance()["min"] bit for bit"""
    w = hbm_case()
    assert BC.launch_shape(330, w["ns"]) == (True, 2)
    R._check_containment(w, precision, ("grid tree330-ns100-hbm", "f64" if precision == capi.F64 else "f32"), calls=2)
    s = R._loop_handle(w, precision=precision)
    before = s.clearance(w["q0"])
    out = s.SolvePose(w["tg"], dt=BC.LAW[0], gain=BC.LAW[1], tol_pose=TOL, max_steps=1)
    s.close()
    ran = out["steps"] == 1
    assert ran.any() and np.array_equal(out["avoid_min_seen"][ran], before["min"][ran])


# ---- e. - h. the loops beside SolvePose ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PATHS, ids=lambda c: "%s-%s" % (c[0][0], "limits" if c[0][1] else "nolimits"))
def test_path_with_a_budget_and_a_grid_matches_the_path_oracle(case):
    R._check_path(path_case(case), case[0])


@pytest.mark.parametrize("case", TRACKS, ids=lambda c: "%s-%s" % (c[0][0], "limits" if c[0][1] else "nolimits"))
def test_track_with_feedforward_and_a_grid_matches_the_track_oracle(case):
    R._check_track(track_case(case), case[0])


@pytest.mark.parametrize("case", STEPS, ids=lambda c: R.step_id(c[0]))
def test_step_control_with_a_grid_matches_the_step_oracle(case):
    R._check_step(step_case(case), case[0])


def test_multistart_three_rounds_with_a_grid():
    """bit for bit against the host-driven sequence, and its rounds against the oracle"""
    R._check_multistart(multistart_case())
