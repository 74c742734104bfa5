"""CPU: the conditions that make every input of tests/test_avoid_big.py a test, on the reference alone, and the launch shape of every
row of its table from the formula of loik_pose_avoid.hpp.  Each `*_conditions` function returns the list of the conditions an input
misses (empty: none).

At B <= 5 a share means nothing, so no instance may be near (avoid_numpy's sense), at least half the seeds start above d_safe (at or
under it r = 0, every bound is 0 and the step says little), a quarter of the instances are narrowed, and an entry of z rests on a
narrowed, non-zero bound of a DoF past the first wavefront (index >= 64, and one >= 128 on the 330-joint tree)."""
import time

import numpy as np
import pytest

import pose_accel_numpy as PA
import pose_limits_numpy as PL
import test_avoid_pose as TP
import test_avoid_routes as R
import avoid_big_cases as BC

MARGIN = 1e-2


def test_launch_shapes_of_the_table():
    for name, ns, hbm, waves, B, _ in BC.TABLE:
        nb = BC.model_of(name).njoints - 1
        assert nb == BC.model_of(name).nv == {"tree170": 170, "tree330": 330}[name]
        assert BC.launch_shape(nb, ns) == (hbm, waves), (name, ns, BC.launch_shape(nb, ns))
        print("avoid_big launch shape %s ns=%d: %s placements, %d B of LDS a wavefront, %d wavefront(s) a workgroup, %d workgroup(s) at B = %d"
              % (name, ns, "HBM" if hbm else "LDS", BC.wave_doubles(nb, ns, hbm) * 8, waves, -(-B // waves), B))
    # 205 is the last count whose LDS stages fit on tree170, 206 the first that does not; the ancestor rows take 6 and 11 words
    assert BC.wave_doubles(170, 205, False) * 8 <= BC.LDS_BYTES < BC.wave_doubles(170, 206, False) * 8
    assert (170 + 31) >> 5 == 6 and (330 + 31) >> 5 == 11
    assert BC.deepest_leaf(BC.model_of("tree170"))[1] == 66 and BC.deepest_leaf(BC.model_of("tree330"))[1] == 154
    # the ragged last workgroup: B = 3 at two wavefronts
    assert BC.row("tree330", 100)[3:5] == (2, 3)


def past(name):
    """the DoF indices an entry of z must rest past"""
    return [64, 128] if name == "tree330" else [64]


def common_conditions(w, o, law):
    miss = []
    if o["near"].any():
        miss.append(("near", o["near"].tolist()))
    start = BC.start_clearance(w)
    if (start > TP.AVOID["d_safe"]).mean() < 0.5:
        miss.append(("start", start.tolist()))
    if (o["avoid_active_steps"] > 0).mean() < 0.25:
        miss.append(("narrowed", float((o["avoid_active_steps"] > 0).mean())))
    dofs = BC.resting_dofs(w, law)
    for t in past(w["name"]):
        if not (dofs >= t).any():
            miss.append(("resting past", t, dofs.tolist()))
    return miss


def table_conditions(w):
    t0 = time.time()
    o = TP._oracle(w, *R.CONTAIN_LAW, 1)   # (the first of the two calls; the second is held to the device's own query at its own q)
    miss = common_conditions(w, o, R.CONTAIN_LAW)
    if R.resting_on_narrowed(w, R.CONTAIN_LAW) < 8:   # (rounding to nearest rounds about half of them outward: enough that one is)
        miss.append(("resting on a narrowed side", R.resting_on_narrowed(w, R.CONTAIN_LAW)))
    print("avoid_big table %s ns=%d: narrowed %.2f, resting %d, on DoFs up to %s, start clearance %s, oracle %.1f s"
          % (w["name"], w["ns"], (o["avoid_active_steps"] > 0).mean(), R.resting_on_narrowed(w, R.CONTAIN_LAW),
             BC.resting_dofs(w, R.CONTAIN_LAW).max(initial=-1), np.round(BC.start_clearance(w), 3).tolist(), time.time() - t0))
    return miss


@pytest.mark.parametrize("case", BC.TABLE, ids=BC.row_id)
def test_table_inputs(case):
    assert table_conditions(BC.table_case(case)) == []


def decided_by_the_step_box(w, o):
    """how many entries of the oracle's z of the first step rest on a side the position / acceleration limits narrowed and avoidance
    left alone"""
    qidx = PL.limit_q_index(w["model"])
    lb, ub = (np.broadcast_to(x, (w["B"], w["model"].nv)) for x in w["box"])
    count = 0
    for b in np.flatnonzero(o["steps"] == 1):
        lo, hi = PA.dyn_box(w["q0"][b], np.zeros(w["model"].nv), np.asarray(w["a_max"], dtype=float), w["q_lo"], w["q_hi"], lb[b], ub[b], BC.LAW[0], qidx)[:2]
        af = o["avoid_flags"][b]
        count += int(((np.abs(o["z"][b] - lo) < 1e-9) & (lo > lb[b]) & ((af & 1) == 0)).sum() + ((np.abs(o["z"][b] - hi) < 1e-9) & (hi < ub[b]) & ((af & 2) == 0)).sum())
    return count


def parity_conditions(w, limits):
    miss = []
    for k in BC.STEPS:
        o = TP._oracle(w, *BC.LAW, k)
        miss += [(k,) + m for m in common_conditions(w, o, BC.LAW)]
        margin = R.decision_margin(w, o)
        if margin < MARGIN:
            miss.append((k, "margin", margin))
    if limits:
        o = TP._oracle(w, *BC.LAW, 1)
        if decided_by_the_step_box(w, o) == 0 or not (o["limit_flags"] != 0).any():
            miss.append("no entry decided by the step box")
        if R.resting_on_narrowed(w, BC.LAW) == 0:
            miss.append("no entry decided by avoidance")
    return miss


@pytest.mark.parametrize("case", BC.PARITY, ids=lambda c: c[0])
def test_parity_inputs(case):
    w = BC.parity_case(case)
    t0 = time.time()
    miss = parity_conditions(w, case[3] > 0)
    o = TP._oracle(w, *BC.LAW, 2)
    print("avoid_big parity %s: narrowed %.2f reached %s steps %s, oracle of 1 and 2 steps %.1f s"
          % (case[0], (o["avoid_active_steps"] > 0).mean(), o["reached"].tolist(), o["steps"].tolist(), time.time() - t0))
    assert miss == []


def test_base_box_and_loops_inputs():
    """the two workloads that are held to exact identities only: both are narrowed on the reference"""
    for w in (BC.back_case(), BC.loops_case()):
        o = TP._oracle(w, *BC.LAW, 2)
        assert not o["near"].any() and (o["avoid_active_steps"] > 0).mean() >= 0.25 and o["steps"].max() == 2
        assert (BC.start_clearance(w) > TP.AVOID["d_safe"]).mean() >= 0.5
