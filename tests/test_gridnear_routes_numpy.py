"""CPU: the conditions that make every input of tests/test_gridnear_routes.py a test, on the reference alone -- in every parity case a
grid pair is among the entries under d_influence in at least a quarter of the instances (without it the case repeats
test_avoid_routes.py), the share of near instances is at most gridnear_cases.NEAR_SHARE and zero where the test is exact -- and the
oracle's `grid` route proven neutral: without a grid in the collision model, or with grid = None, lockstep_pose_loop_avoid and the
`narrow` hook are what they were, bit for bit."""
import time

import numpy as np
import pytest

import avoid_numpy as AN
import gridnear_cases as GC
import test_avoid_pose as TP
import test_avoid_routes as R
import test_avoid_routes_numpy as RN
import test_gridnear_routes as GR

GRID_SHARE = 0.25


def test_without_a_grid_the_oracle_is_what_it_was():
    """constraints_of is constraints() when the collision model names no grid: the oracle of test_avoid_pose's first parity case, whose
    results test_avoid_numpy.py pins, against the same run with grid = None in the model; and the hook likewise"""
    w = TP._workload("panda7", 0)
    want = TP._oracle(w, 0.25, 0.5, 4)
    lb, ub = w["box"]
    col = dict(w["col"], grid=None)
    got = AN.lockstep_pose_loop_avoid(w["model"], TP.PRM, w["q0"], np.eye(6), np.zeros(6), w["links"], w["A"], lb, ub, w["tg"], 0.25, 0.5, TP.TOL, 4,
                                      w["q_lo"], w["q_hi"], col, TP.AVOID)
    for k in ("q", "steps", "status", "err", "z", "iter", "limit_flags", "avoid_min_seen", "avoid_active_steps", "avoid_flags", "near"):
        assert np.array_equal(got[k], want[k]), k
    a, b = AN.narrower(w["model"], w["col"], TP.AVOID, 0.25, w["B"]), AN.narrower(w["model"], col, TP.AVOID, 0.25, w["B"])
    inf = np.inf * np.ones(w["model"].nv)
    for i in range(4):
        x, y = a(i, w["q0"][i], -inf, inf), b(i, w["q0"][i], -inf, inf)
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
    args = (w["model"], w["q0"][:4], w["col"]["links"], w["col"]["spheres"], w["col"]["ws"], w["col"]["wb"], w["col"]["pairs"], 0.15)
    plain, through = AN.constraints(*args, d_safe=0.02), AN.constraints_of(w["model"], w["q0"][:4], w["col"], TP.AVOID)
    assert np.array_equal(plain[1], through[1]) and all(np.array_equal(p["g"], t["g"]) for rp, rt in zip(plain[0], through[0]) for p, t in zip(rp, rt))


def grid_conditions(w, o, exact=False):
    miss = []
    if o["near"].mean() > (0.0 if exact else GC.NEAR_SHARE):
        miss.append(("near", o["near"].tolist()))
    if GR.grid_share(w) < GRID_SHARE:
        miss.append(("grid share", GR.grid_share(w)))
    if (o["avoid_active_steps"] > 0).mean() < 0.25:
        miss.append(("narrowed", float((o["avoid_active_steps"] > 0).mean())))
    return miss


@pytest.mark.parametrize("case", GR.ROUTES, ids=lambda c: R.route_id(c[0]))
def test_route_matrix_inputs(case):
    """test_avoid_routes_numpy.route_conditions on the one law, the grid's share, and limits that bind at either step count"""
    w = GR.route_case(case)
    t0 = time.time()
    assert RN.route_conditions(w, laws=[GR.LAW], steps=GR.ROUTE_STEPS) == []
    print("gridnear_routes %s: oracle of 1 and 4 steps %.1f s, grid share %.2f" % (R.route_id(case[0]), time.time() - t0, GR.grid_share(w)))
    for k in GR.ROUTE_STEPS:
        o = TP._oracle(w, *GR.LAW, k)
        assert grid_conditions(w, o) == [], k
        assert (o["limit_flags"] != 0).any(), k


def loop_conditions(w, o, miss, q=None):
    """the conditions of the no-grid input (`miss`, of test_avoid_routes_numpy) and the grid's share"""
    miss = list(miss)
    if o["near"].mean() > GC.NEAR_SHARE:
        miss.append(("near", float(o["near"].mean())))
    if GR.grid_share(w, q) < GRID_SHARE:
        miss.append(("grid share", GR.grid_share(w, q)))
    return miss


@pytest.mark.parametrize("case", GR.PATHS, ids=lambda c: "%s-%s" % (c[0][0], "limits" if c[0][1] else "nolimits"))
def test_path_inputs(case):
    w = GR.path_case(case)
    assert loop_conditions(w, R.path_oracle(w), RN.path_conditions(w)) == []


@pytest.mark.parametrize("case", GR.TRACKS, ids=lambda c: "%s-%s" % (c[0][0], "limits" if c[0][1] else "nolimits"))
def test_track_inputs(case):
    w = GR.track_case(case)
    o = R.track_oracle(w)
    assert loop_conditions(w, o, RN.track_conditions(w, o)) == []


@pytest.mark.parametrize("case", GR.STEPS, ids=lambda c: R.step_id(c[0]))
def test_step_control_inputs(case):
    w = GR.step_case(case)
    assert loop_conditions(w, R.step_oracle(w, case[0][2]), RN.step_conditions(w, case[0][2])) == []


def test_multistart_input():
    import pose_multistart_numpy as M
    w = GR.multistart_case()
    q = M.sample(w["model"], w["q0g"], w["K"], R.MS_DRAW, 0, w["lo"], w["hi"])
    assert loop_conditions(w, R.multistart_oracle(w)["last"], RN.multistart_conditions(w), q) == []


@pytest.mark.parametrize("case", GR.RAGGED, ids=lambda c: "B%d-%s" % (c[0][0], "boxinst" if c[0][1] else "boxsh"))
def test_ragged_inputs(case):
    w = GR.ragged_case(case)
    t0 = time.time()
    o = TP._oracle(w, *R.RAGGED_LAW, R.RAGGED_STEPS)
    print("gridnear_routes ragged B%d %s: oracle %.1f s, grid share %.2f" % (case[0][0], "boxinst" if case[0][1] else "boxsh", time.time() - t0, GR.grid_share(w)))
    assert grid_conditions(w, o, exact=True) == []
    assert R.decision_margin(w, o) >= 1e-3 and o["steps"].max() >= 2


@pytest.mark.parametrize("box_inst", [False, True])
def test_containment_inputs(box_inst):
    w = GR.contain_case(box_inst)
    assert grid_conditions(w, TP._oracle(w, *R.CONTAIN_LAW, R.CONTAIN_CALLS)) == []


def test_hbm_input():
    w = GR.hbm_case()
    assert grid_conditions(w, TP._oracle(w, *R.CONTAIN_LAW, 1), exact=True) == []
