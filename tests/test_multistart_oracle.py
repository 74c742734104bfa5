"""CPU: the numpy side of the multi-start tests (tests/pose_multistart_numpy.py) -- the restated sampler and the selection rule --
checked on their own, so that the GPU tests compare the device against something that is known to be right."""
import numpy as np

import loik_amd

import pose_limits_numpy as PL
import pose_multistart_numpy as M
from pose_numpy import POSE_NOT_CONVERGED, POSE_REACHED, POSE_STOPPED


def _panda():
    model = loik_amd.builtin_model("panda7")
    return model, np.array(model.q_lo, dtype=float), np.array(model.q_hi, dtype=float)


def test_mix_is_splitmix64():
    """the published first outputs of splitmix64 from state 0: mix(k * golden) for k = 1, 2, 3"""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    with np.errstate(over="ignore"):
        got = M.mix(np.uint64(0x9E3779B97F4A7C15) * np.arange(1, 4, dtype=np.uint64))
    assert [int(x) for x in got] == want


def test_sampler_is_deterministic_and_differs_between_rounds_and_seeds():
    model, lo, hi = _panda()
    q0 = 0.5 * (lo + hi)[None, :] * np.ones((3, 1))
    a = M.sample(model, q0, 7, 11, 0, lo, hi)
    assert np.array_equal(a, M.sample(model, q0, 7, 11, 0, lo, hi))
    assert a.shape == (21, model.nq)
    b, c = M.sample(model, q0, 7, 11, 1, lo, hi), M.sample(model, q0, 7, 12, 0, lo, hi)
    free = np.ones(21, dtype=bool)
    free[::7] = False   # (seed 0 of round 0 is q0)
    assert np.array_equal(a[~free], q0) and np.array_equal(c[~free], q0) and not np.array_equal(b[~free], q0)
    assert np.all(a[free] != b[free]) and np.all(a[free] != c[free])
    assert len(np.unique(a[free])) == a[free].size


def test_sampler_stays_in_range_and_a_point_range_is_exact():
    model, lo, hi = _panda()
    q0 = np.zeros((2, model.nq))
    for rnd in (0, 1, 5):
        q = M.sample(model, q0, 500, 3, rnd, lo, hi)
        rows = np.ones(1000, dtype=bool)
        if rnd == 0:
            rows[::500] = False
        assert np.all(q[rows] >= lo) and np.all(q[rows] <= hi)
    pin = 0.1 + 0.7 * np.arange(model.nv)
    q = M.sample(model, q0, 500, 3, 2, pin, pin)
    assert np.array_equal(q, np.broadcast_to(pin, q.shape))
    # a DoF without a finite pair keeps q0
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[2], hi2[4] = -np.inf, np.inf
    q = M.sample(model, q0 + 0.25, 500, 3, 2, lo2, hi2)
    assert np.all(q[:, [2, 4]] == 0.25) and np.all(q[:, [0, 1, 3, 5, 6]] != 0.25)


def test_uniforms_are_uniform_and_words_do_not_collide():
    u = M.uniforms(2024, 0, np.arange(1000)[:, None], np.arange(100)[None, :]).ravel()
    assert u.size == 10 ** 5 and np.all(u >= 0.0) and np.all(u < 1.0)
    assert abs(u.mean() - 0.5) < 0.01
    w = M.words(2024, 0, np.arange(100)[:, None], np.arange(100)[None, :]).ravel()
    assert len(set(int(x) for x in w[:10 ** 4])) == 10 ** 4


def test_product_is_rounded_before_the_sum():
    """a case where a fused multiply-add gives another double: the restated sampler must give the two-rounding result"""
    from fractions import Fraction
    u, lo, hi = 0.1, 1.0, 1.0 + 3 * 2.0 ** -3
    two = lo + u * (hi - lo)
    exact = Fraction(lo) + Fraction(u) * Fraction(hi - lo)
    # the helper's arithmetic is numpy's elementwise product then sum: two roundings
    model, plo, phi = _panda()
    j = 0
    s_lo, s_hi = np.full(model.nv, -np.inf), np.full(model.nv, np.inf)
    s_lo[j], s_hi[j] = lo, hi
    q = M.sample(model, np.zeros((1, model.nq)), 2, 5, 1, s_lo, s_hi)
    uu = M.uniforms(5, 1, np.arange(2), j)
    assert np.array_equal(q[:, j], np.minimum(lo + np.array([x * (hi - lo) for x in uu]), hi))
    assert abs(Fraction(two) - exact) < Fraction(2.0 ** -50)


# ---- the selection rule on hand-built tables ------------------------------------------------------------------------------------
R, N, S = POSE_REACHED, POSE_NOT_CONVERGED, POSE_STOPPED


def test_selection_covers_every_class():
    #        goal 0: reached wins       goal 1: best effort          goal 2: all stopped      goal 3: reached beats a cheaper class 1
    status = [0, R, R | N, S,           0, N, S, 0,                  S, S, S, S,              0, 0, R, 0]
    cls = np.where(np.array(status) & S, 2, np.where(np.array(status) & R, 0, 1))
    cost = [9.0, 3.0, 2.0, 0.0,         0.5, 0.25, 0.0, 0.75,        0.0, 0.0, 0.0, 0.0,      1e-9, 1e-9, 50.0, 1e-9]
    o = M.select_tables(cls, cost, status, 4)
    assert o["winner"].tolist() == [2, 5, 8, 14]
    assert o["goal_status"].tolist() == [M.GOAL_REACHED, M.GOAL_BEST_EFFORT, M.GOAL_FAILED, M.GOAL_REACHED]
    assert o["nreached"].tolist() == [2, 0, 0, 1]
    assert o["cost"].tolist() == [2.0, 0.25, 0.0, 50.0]
    assert np.isclose(o["margin"][0], 0.5) and np.isclose(o["margin"][1], 1.0) and np.isinf(o["margin"][3])


def test_selection_orders_nan_last_and_breaks_ties_by_index():
    status = [R, R, R,   0, 0, 0,   R, R, R,    0, 0, 0]
    cls = [0, 0, 0,      1, 1, 1,   0, 0, 0,    1, 1, 1]
    nan = np.nan
    cost = [nan, 4.0, 4.0,   nan, nan, 7.0,   1.0, 1.0, 1.0,   nan, nan, nan]
    o = M.select_tables(cls, cost, status, 3)
    assert o["winner"].tolist() == [1, 5, 6, 9]
    assert o["margin"][0] == 0.0 and o["margin"][2] == 0.0
    assert np.isnan(o["cost"][3]) and o["goal_status"][3] == M.GOAL_BEST_EFFORT
    # a NaN class-0 cost still beats every class-1 instance
    o = M.select_tables([0, 1], [nan, 0.0], [R, 0], 2)
    assert o["winner"].tolist() == [0] and o["goal_status"].tolist() == [M.GOAL_REACHED]


def test_instance_keys_and_pick_first():
    model, lo, hi = _panda()
    qidx = PL.limit_q_index(model)
    q0 = np.zeros((2, model.nq))
    q = np.zeros((6, model.nq))
    q[0, 0], q[1, 1], q[2, 2] = 0.3, 0.2, 0.1          # goal 0: all reached, instance 2 nearest
    q[3, 0], q[4, 0] = 0.1, 0.2                         # goal 1: 3 not reached, 4 reached, 5 stopped
    status = np.array([R, R, R, 0, R, S])
    err = np.zeros((6, 1, 6))
    err[3, 0, 4] = -0.6
    err[5, 0, 0] = np.nan
    cls, cost = M.instance_keys(status, err, q, q0, 3, M.PICK_NEAREST, qidx)
    assert cls.tolist() == [0, 0, 0, 1, 0, 2]
    assert np.allclose(cost, [0.09, 0.04, 0.01, 0.6, 0.04, 0.0], rtol=1e-15)
    assert M.select(status, err, q, q0, 3, M.PICK_NEAREST, qidx)["winner"].tolist() == [2, 4]
    w = np.ones(model.nv)
    w[2] = 100.0   # the metric decides: instance 2's DoF is now the dearest
    assert M.select(status, err, q, q0, 3, M.PICK_NEAREST, qidx, w)["winner"].tolist() == [1, 4]
    first = M.select(status, err, q, q0, 3, M.PICK_FIRST, qidx)
    assert first["winner"].tolist() == [0, 4] and first["cost"].tolist() == [0.0, 0.0]


def test_resample_leaves_reached_rows():
    model, lo, hi = _panda()
    q0 = np.zeros((2, model.nq))
    q = M.sample(model, q0, 3, 1, 0, lo, hi)
    status = np.array([R, 0, S, 0, R | N, N])
    q2, fresh = M.resample(model, q, status, q0, 3, 1, 1, lo, hi)
    assert fresh.tolist() == [False, True, True, True, False, True]
    assert np.array_equal(q2[~fresh], q[~fresh])
    assert np.array_equal(q2[fresh], M.sample(model, q0, 3, 1, 1, lo, hi)[fresh])
