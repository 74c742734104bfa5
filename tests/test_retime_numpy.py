"""CPU: the numpy reference of the retiming rule (tests/retime_numpy.py) keeps what include/loik_amd_retime.h promises: both regimes occur,
some DoF saturates on every moved segment, the limits hold at every sample and between every two, SNAP puts the waypoints on samples and
never raises a peak, and the padding of a shortcut result changes nothing.  It also fixes the inputs of the GPU test (test_retime.py) and
checks what makes their integer outputs comparable."""
import numpy as np
import pytest

import motion_numpy as MN
import retime_numpy as RN
import test_clearance as TC
import test_motion_clearance as TM
import test_shortcut as TS

T_PATH, DT, S_ROWS, RNG = 6, 0.02, 256, 1200
SIX = ("panda7", "talos32", "multidof13", "composite20", "multidof20", "helical24")
REGIMES = {"panda7": (68, 12), "talos32": (71, 9), "multidof13": (70, 10), "composite20": (70, 10), "multidof20": (66, 14), "helical24": (67, 13)}

_CASES = {}


def limits(name, nv):
    j = np.arange(nv)
    return TM.SIZE[name] * (2.0 + 0.25 * (j % 5)), TM.SIZE[name] * (4.0 + 1.5 * (j % 3))


def retime_case(name, rng=RNG):
    """the model of test_clearance._case, B = min(16, n) paths of T = 6 waypoints from its q, the limits of the issue, and the numpy answer
    with and without SNAP at S = 256: computed once"""
    if name not in _CASES:
        c = dict(TC._case(name))
        model = c["model"]
        B = min(16, c["n"])
        c["B"], c["paths"] = B, TS.make_paths(model, c["q"][:B], TM.SIZE[name], T_PATH, np.random.default_rng(rng))
        c["v_max"], c["a_max"] = limits(name, model.nv)
        c["want"] = {snap: RN.retime(model, c["paths"], c["v_max"], c["a_max"], DT, S=S_ROWS, snap=snap) for snap in (False, True)}
        _CASES[name] = c
    return _CASES[name]


def off_integer(x):
    """the distance of every x to the nearest integer"""
    return np.abs(x - np.round(x))


def check_comparable(want):
    """no segment and no path has D / dt within 1e-9 of an integer: ceil is the same in every arithmetic within the bound"""
    D = want["seg"][:, :, 1]
    assert np.all(off_integer(D[D > 0.0] / DT) > 1e-9) and np.all(off_integer(want["duration"] / DT) > 1e-9)


def check_limits(r, v_max, a_max, dt):
    """|v| <= v_max (1 + 1e-12) at every sample, |v_{i+1} - v_i| <= a_max dt (1 + 1e-9) at every consecutive pair, stops included"""
    v = r["v_traj"]
    assert np.all(np.abs(v) <= v_max * (1.0 + 1e-12))
    assert np.all(np.abs(np.diff(v, axis=1)) <= a_max * dt * (1.0 + 1e-9))
    assert np.all(v[:, 0] == 0.0) and np.all(v[:, -1] == 0.0)


@pytest.mark.parametrize("name", SIX)
def test_regimes_saturation_and_limits(name):
    c = retime_case(name)
    model, paths, v_max, a_max = c["model"], c["paths"], c["v_max"], c["a_max"]
    for snap in (False, True):
        want = c["want"][snap]
        reg = sum(want["regimes"], [])
        assert (reg.count("tri"), reg.count("trap")) == REGIMES[name]
        assert np.all(want["flags"] == 0) and np.all(want["moved"] == T_PATH - 1) and np.all(want["n_samples"] <= S_ROWS)
        check_limits(want, v_max, a_max, DT)
    want = c["want"][False]
    check_comparable(want)
    assert 3.9 <= want["duration"].min() and want["duration"].max() <= 4.94 and 199 <= want["n_samples"].min() and want["n_samples"].max() <= 248
    # some DoF saturates on every moved segment: the velocity limit at the peak, or the acceleration limit
    for b in range(c["B"]):
        dv = MN.difference(model, paths[b, :-1], paths[b, 1:])
        for k in range(T_PATH - 1):
            t0, D, t_acc, peak = want["seg"][b, k]
            A = peak / t_acc
            sat_v, sat_a = np.max(peak * np.abs(dv[k]) / v_max), np.max(A * np.abs(dv[k]) / a_max)
            assert sat_v <= 1.0 + 1e-12 and sat_a <= 1.0 + 1e-12
            assert abs(sat_a - 1.0) <= 1e-12 and (want["regimes"][b][k] == "tri" or abs(sat_v - 1.0) <= 1e-12)
    # the trajectory ends on the last waypoint and every sample before n_samples - 1 is in motion or at a corner
    for b in range(c["B"]):
        ns = int(want["n_samples"][b])
        assert np.array_equal(want["q_traj"][b, ns - 1:], np.tile(paths[b, -1], (S_ROWS - ns + 1, 1)))
        assert np.array_equal(want["q_traj"][b, 0], paths[b, 0])


@pytest.mark.parametrize("name", ("panda7", "multidof13"))
def test_snap_puts_waypoints_on_samples_and_never_raises_a_peak(name):
    c = retime_case(name)
    free, snap = c["want"][False], c["want"][True]
    T = T_PATH
    for b in range(c["B"]):
        N = snap["ticks"][b]
        assert N[0] == 0 and np.all(np.diff(N) >= 1) and snap["n_samples"][b] == N[T - 1] + 1
        for k in range(T):
            assert np.array_equal(snap["q_traj"][b, N[k]], c["paths"][b, k]) and np.all(snap["v_traj"][b, N[k]] == 0.0)
        assert np.array_equal(snap["seg"][b, :, 0], DT * N[:T - 1]) and snap["duration"][b] == DT * N[T - 1]
    assert np.all(snap["seg"][:, :, 3] <= free["seg"][:, :, 3]) and np.all(snap["seg"][:, :, 1] >= free["seg"][:, :, 1])
    assert np.all(snap["seg"][:, :, 1] - free["seg"][:, :, 1] < DT)
    n = np.round(snap["seg"][:, :, 1] / DT)
    assert np.array_equal(n, np.diff(snap["ticks"], axis=1)) and np.all(off_integer(snap["seg"][:, :, 1] / DT) < 1e-9)


def test_padded_shortcut_result_equals_its_waypoints():
    c = TS.shortcut_case("panda7")
    model, short = c["model"], c["want"]
    v_max, a_max = limits("panda7", model.nv)
    L = short["n_waypoints"]
    assert (L < T_PATH).any()
    padded = RN.retime(model, short["q_path"], v_max, a_max, DT, S=S_ROWS)
    counted = RN.retime(model, short["q_path"], v_max, a_max, DT, n_waypoints=L, S=S_ROWS)
    for k in ("q_traj", "v_traj", "duration", "seg", "n_samples", "flags"):
        assert np.array_equal(padded[k], counted[k]), k
    assert np.array_equal(padded["moved"], L - 1) and np.all(padded["n_waypoints"] == T_PATH)
    # ... and repeated waypoints inside a path are corners of duration 0
    rep = np.repeat(c["paths"][:2], 2, axis=1)
    twice, once = RN.retime(model, rep, v_max, a_max, DT, S=S_ROWS), RN.retime(model, c["paths"][:2], v_max, a_max, DT, S=S_ROWS)
    assert all(np.array_equal(twice[k], once[k]) for k in ("q_traj", "v_traj", "duration", "n_samples", "moved"))
    assert np.all(twice["seg"][:, 0::2] == 0.0) and np.array_equal(twice["seg"][:, 1::2], once["seg"])


def test_edges_of_the_rule():
    c = retime_case("panda7")
    model, paths, v_max, a_max = c["model"], c["paths"], c["v_max"], c["a_max"]
    n = np.array([0, 1, 2, T_PATH, T_PATH + 1])
    r = RN.retime(model, paths[:5], v_max, a_max, DT, n_waypoints=n, S=S_ROWS)
    assert r["flags"].tolist() == [RN.SKIPPED, RN.SKIPPED, 0, 0, RN.SKIPPED] and r["n_waypoints"].tolist() == [0, 0, 2, T_PATH, 0]
    assert np.isnan(r["duration"][[0, 1, 4]]).all() and np.isnan(r["q_traj"][[0, 1, 4]]).all() and r["moved"][2] == 1
    assert np.all(r["seg"][2, 1:] == 0.0) and np.array_equal(r["q_traj"][3], c["want"][False]["q_traj"][3])
    bad = paths[:3].copy()
    bad[1, 2, 0] = np.nan
    r = RN.retime(model, bad, v_max, a_max, DT, S=S_ROWS)
    assert r["flags"].tolist() == [0, RN.INVALID, 0] and r["n_samples"][1] == 0 and np.isnan(r["q_traj"][1]).all() and np.isnan(r["duration"][1])
    still = np.tile(paths[:1, :1], (1, 2, 1))
    r = RN.retime(model, still, v_max, a_max, DT, S=3)
    assert r["duration"][0] == 0.0 and r["n_samples"][0] == 1 and r["moved"][0] == 0 and np.array_equal(r["q_traj"][0], np.tile(paths[0, 0], (3, 1)))
    r = RN.retime(model, paths[:2], v_max, a_max, DT, S=100)
    assert np.all(r["flags"] == RN.TRUNCATED) and np.array_equal(r["q_traj"], c["want"][False]["q_traj"][:2, :100])
    r = RN.retime(model, paths[:2], v_max, a_max, DT)
    assert np.all(r["flags"] == 0) and np.array_equal(r["duration"], c["want"][False]["duration"][:2]) and "q_traj" not in r
