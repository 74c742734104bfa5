"""CPU: the numpy reference of include/loik_amd_avoid.h (tests/avoid_numpy.py) proven before it referees the device: the gradient row of
every pair kind against a central finite difference of clearance_numpy through the oracle's integrate, the inscribed box against its
half-spaces, the loop oracle against the limits oracle it extends, and the share of `near` rows in the inputs of the GPU tests."""
import numpy as np
import pytest

import avoid_numpy as AN
import clearance_numpy as CN
import pose_limits_numpy as PL
import pose_numpy as P
import test_avoid_box as TB
import test_clearance as TC

H = 1e-6   # the step of the central difference: truncation ~ H^2 |d3|, rounding ~ 1e-16 / H
FD_TOL = 2e-8


def _pair_value(model, q, links, spheres, ws, wb, a, kind, partner):
    """the clearance of one pair for configurations q [n][nq], by clearance_numpy's centres and distance formulas"""
    sel = [a, partner] if kind else [a]
    cen = CN.centres(model, q, [links[k] for k in sel], spheres[sel])
    if kind:
        return CN.sphere_sphere(cen[:, 0], spheres[a, 3], cen[:, 1], spheres[partner, 3])
    if partner < ws.shape[0]:
        return CN.sphere_sphere(cen[:, 0], spheres[a, 3], ws[partner, :3], ws[partner, 3])
    return CN.sphere_box(cen[:, 0], spheres[a, 3], wb[partner - ws.shape[0]])


def _fd_gradient(model, q, links, spheres, ws, wb, a, kind, partner):
    """d(pair clearance)/dz by central differences through pose_numpy.integrate"""
    rows = []
    for j in range(model.nv):
        v = np.zeros(model.nv)
        v[j] = H
        rows += [P.integrate(model, q, v), P.integrate(model, q, -v)]
    t = _pair_value(model, np.stack(rows), links, spheres, ws, wb, a, kind, partner)
    return (t[0::2] - t[1::2]) / (2.0 * H)


def _ordinal(a, kind, partner, ns, nws, nwb, pairs):
    """the column of a pair in clearance_numpy.pair_table: world spheres a major, then world boxes a major, then the self pairs"""
    if kind:
        return ns * (nws + nwb) + pairs.index((a, partner))
    return a * nws + partner if partner < nws else ns * nws + a * nwb + (partner - nws)


def _box_region(c, box15):
    """how many of d = |R^T (c - t)| - h are positive: 0 inside, 1 a face, 2 an edge, 3 a corner"""
    R, t, h = box15[:9].reshape(3, 3), box15[9:12], box15[12:15]
    return int((np.abs(R.T @ (c - t)) - h > 0.0).sum())


@pytest.mark.parametrize("name", ["multidof13", "multidof20"])
def test_gradient_matches_finite_differences(name):
    """every pair of a small model -- world spheres, world boxes in all four regions, self pairs -- at three configurations, every joint type
    of the two multi-DoF models among the DoFs; the pairs whose own decision is near (a centre on a sphere's centre, the argmax inside a
    box) are left out, as are the box pairs whose centre is within 1e-4 of a face plane (the finite difference straddles the kink)"""
    model = TC._model(name)
    rng = np.random.default_rng(700)
    q = model.random_configurations(rng, 3)
    links, spheres = CN.make_spheres(model, 1, 701)
    ws, wb = TC._world(rng, 3, 6)
    wb[:3, 12:15] *= 4.0   # (boxes large enough to hold a centre)
    pairs = CN.self_pairs(model.parents, links)
    nws, nwb, ns = ws.shape[0], wb.shape[0], len(links)
    pairs = [(int(a), int(b)) for a, b in pairs]
    seen, worst = set(), 0.0
    for i in range(q.shape[0]):
        cen = CN.centres(model, q[i:i + 1], links, spheres)[0]
        todo = [(a, 0, o) for a in range(ns) for o in range(nws + nwb)] + [(a, 1, b) for a, b in pairs]
        table = CN.pair_table(cen[None], spheres[:, 3], ws, wb, pairs)[0][0]
        for a, kind, partner in todo[::3]:
            assert _pair_value(model, q[i:i + 1], links, spheres, ws, wb, a, kind, partner)[0] == table[_ordinal(a, kind, partner, ns, nws, nwb, pairs)]
            nrm, g, m, near = AN.pair_gradient(model, q[i], links, spheres, ws, wb, None, a, kind, partner, cen)
            if near:
                continue
            region = "self" if kind else "sphere"
            if kind == 0 and partner >= nws:
                box = wb[partner - nws]
                d = np.abs(box[:9].reshape(3, 3).T @ (cen[a] - box[9:12])) - box[12:15]
                if np.min(np.abs(d)) < 1e-4:
                    continue
                region = "box%d" % _box_region(cen[a], box)
            fd = _fd_gradient(model, q[i], links, spheres, ws, wb, a, kind, partner)
            err = float(np.max(np.abs(g - fd)))
            worst = max(worst, err)
            assert err <= FD_TOL, (name, i, a, kind, partner, region, err)
            assert abs(np.linalg.norm(nrm) - 1.0) < 1e-12
            on = AN.pair_dofs(model, links[a], links[partner] if kind else None)
            assert m == int(on.sum()) and not np.any(g[~on]) and np.all(np.abs(fd[~on]) <= FD_TOL)
            seen.add(region)
    print("avoid_numpy %s: max |g - finite difference| %.3e over the regions %s" % (name, worst, sorted(seen)))
    assert seen >= {"sphere", "self", "box0", "box1", "box2", "box3"}, seen
    jt = {int(t) for t in model.jtype[1:]}
    assert len(jt) >= 4   # (the multi-DoF models mix free-flyer / spherical / translation / ZYX / planar / (cos, sin) joints with 1-DoF ones)


def test_inside_box_normal_goes_to_the_lowest_index_on_a_tie():
    box = CN.box15(np.eye(4), [1.0, 1.0, 2.0])
    n, gap = AN.normal_box([0.5, -0.5, 0.0], box)
    assert np.array_equal(n, [1.0, 0.0, 0.0]) and gap == 0.0
    n, gap = AN.normal_box([0.2, -0.5, 0.0], box)
    assert np.array_equal(n, [0.0, -1.0, 0.0]) and abs(gap - 0.3) < 1e-15
    n, gap = AN.normal_box([3.0, -5.0, 0.0], box)
    assert np.allclose(n, np.array([2.0, -4.0, 0.0]) / np.sqrt(20.0)) and gap == np.inf
    assert np.array_equal(AN.normal_sphere([1.0, 2.0, 3.0], [1.0, 2.0, 3.0])[0], np.zeros(3))


@pytest.mark.parametrize("name", ["panda7", "multidof13"])
def test_every_z_of_the_box_keeps_every_half_space(name):
    """1000 random z of the narrowed box per configuration satisfy g_k . z >= -r_k for every active k, up to rounding: the base box holds 0"""
    ref = TB._ref(name)
    c, box = ref["c"], ref["box"]
    rng = np.random.default_rng(710)
    nv = c["model"].nv
    lb, ub = -rng.uniform(0.5, 2.0, size=nv), rng.uniform(0.5, 2.0, size=nv)
    checked = 0
    for i in range(0, c["n"], 4):
        cons = box["cons"][i]
        lo, hi, A_lo, A_hi, r = AN.narrow(cons, lb, ub, TB.PRM["d_safe"], TB.PRM["kappa"], TB.DT)
        assert np.all(A_lo <= 0.0) and np.all(A_hi >= 0.0) and np.all(lb <= lo) and np.all(lo <= 0.0) and np.all(0.0 <= hi) and np.all(hi <= ub)
        z = rng.uniform(lo, hi, size=(1000, nv))
        z[:500] = np.where(rng.uniform(size=(500, nv)) < 0.5, lo, hi)   # (half of them vertices: where a linear form is least)
        for k, cst in enumerate(cons):
            gz = z @ cst["g"]
            assert np.all(gz >= -r[k] - 1e-12 * (1.0 + r[k])), (name, i, k, float(gz.min()), r[k])
            if cst["d"] <= TB.PRM["d_safe"]:
                assert r[k] == 0.0
            checked += 1
    assert checked > 100


def test_loop_oracle_without_influence_is_the_limits_oracle():
    """with d_influence below every clearance no constraint is ever active: np.array_equal to lockstep_pose_loop_limits"""
    import test_avoid_pose as TP
    w = TP._workload("panda7", 0)
    idx = np.arange(4)
    A, (lb, ub) = w["A"], w["box"]
    args = (w["model"], TP.PRM, w["q0"][idx], np.eye(6), np.zeros(6), w["links"], A, lb, ub, w["tg"][idx], 0.25, 0.5, TP.TOL, 3, w["q_lo"], w["q_hi"])
    want = PL.lockstep_pose_loop_limits(*args)
    got = AN.lockstep_pose_loop_avoid(*args, w["col"], dict(d_safe=-1e9, d_influence=-1e8, kappa=0.5))
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert not got["avoid_active_steps"].any() and not got["avoid_flags"].any() and not got["near"].any()
    ran = got["steps"] > 0
    assert ran.any() and np.all(np.isfinite(got["avoid_min_seen"][ran])) and np.all(np.isposinf(got["avoid_min_seen"][~ran]))


def test_the_wall_is_hit_without_the_latch_and_kept_away_from_with_it():
    """the two conditions that make the wall of test_avoid_pose.py a test, on the oracle's recorded paths: without the latch at least
    half of them reach clearance < 0, with it every one stays >= d_safe / 2; and no instance's run touches a near configuration"""
    import test_avoid_pose as TP
    cfree, cheld = TP.wall_oracle_paths()
    print("avoid_numpy wall: without the latch %.3f of the paths collide (least %.4f); with it the least clearance is %.4f" %
          ((cfree < 0.0).mean(), cfree.min(), cheld.min()))
    assert (cfree < 0.0).mean() >= 0.5
    assert np.all(cheld >= TP.WALL["d_safe"] / 2)
    held = TP._oracle(TP._wall_case(), TP.WALL_DT, TP.WALL_GAIN, TP.WALL_STEPS, TP.WALL)
    assert (held["avoid_active_steps"] > 0).mean() >= 0.5 and held["near"].mean() <= 0.02
    # no freeze: with the latch every instance still moves and closes a quarter of its pose error before the wall holds it
    w = TP._wall_case()
    e0, e1 = TP.wall_errors(w, w["q0"]), np.abs(held["err"]).max(axis=(1, 2))
    print("avoid_numpy wall: pose error left with the latch, over the initial one: median %.3f, largest %.3f" % (np.median(e1 / e0), (e1 / e0).max()))
    assert np.all(e1 <= TP.WALL_PROGRESS * e0) and np.all(np.abs(held["q"] - w["q0"]).max(axis=1) > 0.2)


def test_near_share_of_the_gpu_inputs():
    """the inputs of test_avoid_box.py: at most 2 % of the rows are near, for the box and for the gradient -- on each of the eight robots, at
    each size of test_sizes (with 9 rows that means none) and on the one-self-pair case"""
    refs = [(name, TB._ref(name)) for name in TC.ROBOTS]
    refs += [(inp["what"], TB.input_ref(inp)) for ns in TB.SIZES for inp in TB.size_inputs(ns)]
    refs.append((TB.one_pair_input()["what"], TB.input_ref(TB.one_pair_input())))
    for name, ref in refs:
        for what, near in (("box", ref["box"]["near"]), ("gradient", ref["grad"]["near"])):
            print("avoid_numpy %s %s: %d of %d rows near, %d active constraints" % (name, what, int(near.sum()), near.size, sum(len(r) for r in ref["box"]["cons"])))
            assert near.mean() <= TB.NEAR_SHARE, (name, what, near.mean())


def test_near_share_of_the_parity_workloads():
    """the inputs of test_avoid_pose.test_solve_pose_matches_lockstep_oracle: on every workload, law and step count at most 2 % of the
    instances touch a near configuration in the oracle's run, and the conditions that make a case mean something hold"""
    import test_avoid_pose as TP
    for case in TP.PARITY_CASES:
        w = TP._workload(*case)
        for dt, gain in TP.LAWS:
            for k in TP.PARITY_STEPS:
                o = TP._oracle(w, dt, gain, k)
                narrowed = (o["avoid_active_steps"] > 0).mean()
                print("avoid_numpy parity %s dt %g gain %g k %d: near %.3f narrowed %.3f reached %.3f" % (case, dt, gain, k, o["near"].mean(), narrowed, o["reached"].mean()))
                assert o["near"].mean() <= 0.02, (case, dt, gain, k)
                assert narrowed >= 0.25, (case, dt, gain, k)
