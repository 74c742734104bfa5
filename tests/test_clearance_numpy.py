"""CPU: the numpy reference of include/loik_amd_collision.h (tests/clearance_numpy.py) from first principles -- the sphere / box distance
against a brute-force minimum over the box surface, hand-computable scenes, the self-pair list on a tree written out by hand, and the
selection rule of the collision-aware multi-start on a hand-made table."""
import numpy as np

import loik_amd

from helpers import random_rotation
import clearance_numpy as CN


def _surface(h, pitch):
    """points on the surface of the axis-aligned box [-h, h]: a grid of at most `pitch` on each of the six faces"""
    pts = []
    for ax in range(3):
        u, v = [a for a in range(3) if a != ax]
        gu = np.linspace(-h[u], h[u], int(np.ceil(2 * h[u] / pitch)) + 1)
        gv = np.linspace(-h[v], h[v], int(np.ceil(2 * h[v] / pitch)) + 1)
        U, V = np.meshgrid(gu, gv, indexing="ij")
        for sgn in (-1.0, 1.0):
            p = np.zeros(U.shape + (3,))
            p[..., ax], p[..., u], p[..., v] = sgn * h[ax], U, V
            pts.append(p.reshape(-1, 3))
    return np.concatenate(pts)


def test_sphere_box_outside_matches_the_brute_force_minimum_over_the_surface():
    """centres in the face, edge and corner regions of an oriented box: the distance to the nearest of a dense sampling of the surface
    is at least the formula's (the surface is the closest set) and at most it plus the sampling pitch"""
    rng = np.random.default_rng(3)
    h = np.array([0.3, 0.2, 0.45])
    R, t = random_rotation(rng), np.array([0.4, -0.2, 0.7])
    box = np.concatenate([R.reshape(9), t, h])
    pitch = 0.01
    surf = _surface(h, pitch) @ R.T + t
    local = {"face": [0.1, -0.05, 0.9], "face-x": [-0.8, 0.1, 0.2], "edge": [0.6, 0.5, 0.1], "edge-yz": [0.0, -0.6, -0.8],
             "corner": [0.7, 0.4, 0.9], "corner-neg": [-0.5, -0.45, -0.6]}
    for name, p in local.items():
        p = np.array(p)
        outside = int((np.abs(p) > h).sum())
        assert outside == {"f": 1, "e": 2, "c": 3}[name[0]], name
        c = R @ p + t
        r = 0.07
        brute = np.sqrt(((surf - c) ** 2).sum(axis=1)).min() - r
        got = float(CN.sphere_box(c, r, box))
        assert got > -r and got <= brute + 1e-12 and brute <= got + pitch, (name, got, brute)


def test_sphere_box_inside_is_minus_the_distance_to_the_nearest_face():
    rng = np.random.default_rng(4)
    h = np.array([0.3, 0.2, 0.45])
    R, t = random_rotation(rng), np.array([-0.1, 0.3, 0.2])
    box = np.concatenate([R.reshape(9), t, h])
    for p in ([0.0, 0.0, 0.0], [0.25, 0.0, 0.1], [-0.1, -0.19, 0.4], [0.29, 0.19, 0.44]):
        p = np.array(p)
        r = 0.03
        got = float(CN.sphere_box(R @ p + t, r, box))
        want = -float((h - np.abs(p)).min()) - r
        assert got < 0.0 and abs(got - want) <= 1e-14, (p, got, want)   # (the rotation there and back rounds)
    # the sign is exact: on an axis-aligned box nothing rounds, a centre on the surface is at 0, one ulp-sized steps either side are not
    flat = CN.box15(np.eye(4), h)
    assert float(CN.sphere_box([0.3, 0.1, 0.1], 0.0, flat)) == 0.0
    assert float(CN.sphere_box([np.nextafter(0.3, 1.0), 0.1, 0.1], 0.0, flat)) > 0.0
    assert float(CN.sphere_box([np.nextafter(0.3, 0.0), 0.1, 0.1], 0.0, flat)) < 0.0


def test_hand_computable_scenes():
    # two touching spheres
    assert CN.sphere_sphere(np.array([0.0, 0.0, 0.0]), 0.25, np.array([0.75, 0.0, 0.0]), 0.5) == 0.0
    # a sphere centred in a cube of half extent h: -h - r
    cube = CN.box15(np.eye(4), [0.5, 0.5, 0.5])
    assert float(CN.sphere_box(np.zeros(3), 0.125, cube)) == -0.5 - 0.125
    # through the model: one sphere on the universe, one world sphere that touches it, an empty world
    model = loik_amd.builtin_model("panda7")
    q = np.zeros((2, model.nq))
    out = CN.clearance(model, q, [0], [[1.0, 0.0, 0.0, 0.25]], wspheres=[[1.0, 0.75, 0.0, 0.5]])
    assert np.array_equal(out["min"], [0.0, 0.0]) and np.array_equal(out["witness"], [[CN.WORLD_SPHERE, 0, 0]] * 2)
    assert np.all(np.isposinf(out["min_self"]))
    out = CN.clearance(model, q, [0], [[1.0, 0.0, 0.0, 0.25]])
    assert np.all(np.isposinf(out["min"])) and np.array_equal(out["witness"], [[CN.NONE, -1, -1]] * 2)
    # a NaN row: NaN minima, no witness, the other row as before
    q[1, 2] = np.nan
    out = CN.clearance(model, q, [3], [[0.0, 0.0, 0.0, 0.1]], wspheres=[[0.0, 0.0, 0.0, 0.1]])
    assert np.isfinite(out["min"][0]) and np.isnan(out["min"][1]) and np.array_equal(out["witness"][1], [CN.NONE, -1, -1])


def test_the_ordered_minimum_takes_the_lowest_ordinal_of_a_tie_and_a_nan_last():
    assert CN.ordered_min([3.0, 1.0, 1.0, 2.0]) == 1
    assert CN.ordered_min([np.nan, 5.0, np.nan]) == 1
    assert CN.ordered_min([np.nan, np.nan]) == 0
    assert CN.ordered_min([]) == -1


def test_pair_list_on_a_five_link_tree():
    """0 (universe) - 1 - 2 - 3, and 4 a second child of 1.  Spheres: two on link 1, one each on 2, 3, 4, one on the universe"""
    parents = [0, 0, 1, 2, 1]
    links = [1, 1, 2, 3, 4, 0]
    #         a: 0  1  2  3  4  5
    got = CN.self_pairs(parents, links)
    # same link (0,1); parent-child 1-2: (0,2), (1,2); 2-3: (2,3); 1-4: (0,4), (1,4); universe-1: (0,5), (1,5)
    want = [(0, 3), (1, 3), (2, 4), (2, 5), (3, 4), (3, 5), (4, 5)]
    assert got == want and got == sorted(got)
    # ignoring the link pair (3, 1) in the other order removes both of its sphere pairs, nothing else
    assert CN.self_pairs(parents, links, ignore=[(3, 1)]) == [(2, 4), (2, 5), (3, 4), (3, 5), (4, 5)]
    assert CN.self_pairs(parents, links, ignore=[(1, 3), (4, 0), (2, 4)]) == [(2, 5), (3, 4), (3, 5)]


def test_selection_rule_of_the_latched_multistart():
    """K = 6 seeds per goal, hand-made: statuses REACHED = 1, NOT_CONVERGED = 2, STOPPED = 8"""
    R, N, S = 1, 2, 8
    margin = 0.01
    #            goal 0: clear and colliding reached seeds, a running one, a stopped one
    status = [N, R, R, R, S | R, R,
              #  goal 1: only colliding reached seeds (one NaN), running ones
              N, R, R, R, N, N,
              #  goal 2: nothing reached; goal 3: stopped only
              N, N, N, N, N, N,
              S, S, S, S, S, S]
    clr = [0.5, -0.2, 0.3, 0.02, 0.9, 0.02,
           0.5, -0.2, np.nan, -0.05, 0.5, 0.5,
           0.5, 0.5, 0.5, 0.5, 0.5, 0.5,
           0.5, 0.5, 0.5, 0.5, 0.5, 0.5]
    base_cls = [1, 0, 0, 0, 2, 0, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2]
    base_cost = [0.3, 9.0, 4.0, 2.0, 0.0, 2.0, 0.1, 1.0, 1.0, 1.0, 0.2, 0.3, 0.5, 0.4, 0.4, 0.6, np.nan, 0.7, 0, 0, 0, 0, 0, 0]
    cls, cost = CN.ms_keys(base_cls, base_cost, status, clr, margin)
    assert list(cls[:6]) == [1, 0.5, 0, 0, 2, 0] and cost[1] == 0.2          # -clr orders class 0c; a stopped seed stays class 2
    out = CN.ms_select(cls, cost, 6)
    # goal 0: class 0 beats the cheaper-looking 0c; of the two class-0 seeds with cost 2.0 the lower b
    assert out["winner"][0] == 3 and out["goal_status"][0] == 1 and out["nclear"][0] == 3
    # goal 1: 0c beats the running seeds; the least penetration (-0.05) first, the NaN last
    assert out["winner"][1] == 9 and out["goal_status"][1] == CN.MS_GOAL_IN_COLLISION and out["nclear"][1] == 0 and out["cost"][1] == 0.05
    # goals 2, 3 as without the latch: the smallest error (ties to the lowest b, the NaN last); all stopped
    assert out["winner"][2] == 13 and out["goal_status"][2] == 2
    assert out["winner"][3] == 18 and out["goal_status"][3] == 4
    # only NaN clearances in class 0c: the lowest b of them
    cls2, cost2 = CN.ms_keys([0, 0, 1], [1.0, 1.0, 0.5], [R, R, N], [np.nan, np.nan, 0.5], margin)
    assert CN.ms_select(cls2, cost2, 3)["winner"][0] == 0 and CN.ms_select(cls2, cost2, 3)["goal_status"][0] == 8
    # the class order 0 < 0c < 1 < 2 on one goal of four
    o = CN.ms_select(*CN.ms_keys([2, 1, 0, 0], [0, 0.1, 5.0, 7.0], [S, N, R, R], [1, 1, -1.0, 1.0], 0.0), 4)
    assert o["winner"][0] == 3 and o["goal_status"][0] == 1
    # the re-sampler's status word: REACHED cleared on class 0c alone
    ls = CN.ms_loop_status(status[:6], clr[:6], margin)
    assert list(ls) == [N, 0, R, R, S | R, R]
