"""CPU: the claims of the planning reference (tests/plan_numpy.py, the rule of include/loik_amd_plan.h) on its own: the wall a direct
segment cannot pass is planned around, every segment of every found path is FREE under motion_numpy.advance and clear of the margin
under dense sampling, the ends are the inputs bit for bit, the outcome is a function of the seed, every status occurs, and max_iters = 0
is the direct check alone."""
import numpy as np

import motion_numpy as MN
import plan_numpy as PN
import qp_cases as QC
import shortcut_numpy as SN
import test_clearance as TC

TOL, MAX_EVALS, T_PLAN = 1e-3, 24, 32
_CASES = {}


def wall_case():
    """test_shortcut's thin-box case: panda7, one sphere on link 7, a thin box across the segment A -> A + dv, ranges of +- 1 around the
    two ends"""
    model = QC.model_of("panda7")
    A = model.random_configurations(np.random.default_rng(750), 1)[0]
    dv = np.array([0.9, -0.7, 0.5, 0.8, -0.6, 0.4, 0.3])
    links, spheres = np.array([7], dtype=np.int32), np.array([[0.0, 0.0, 0.1, 0.01]])
    box = MN.thin_box_across(model, A, dv, 7, spheres[0])
    return dict(model=model, A=A, Bq=A + dv, links=links, spheres=spheres, box=box, lo=np.minimum(A, A + dv) - 1.0, hi=np.maximum(A, A + dv) + 1.0)


def plan_case(name, B=16, rng=None, near=None, **over):
    """the model, spheres, world and pairs of test_clearance._case, B queries q[b] -> q[b + B] (q[b + 1] where q is short), the margin = the 10 % quantile of the
    clearance over the ends (unless `over` gives one), ranges = the box of the ends widened by 0.5, and the numpy answer: computed once"""
    key = (name, B, rng, near, tuple(sorted(over.items())))
    if key not in _CASES:
        c = dict(TC._case(name))
        model = c["model"]
        q = c["q"] if rng is None else model.random_configurations(np.random.default_rng(rng), 2 * B)
        first = B if 2 * B <= q.shape[0] else 1      # (tree330 has three configurations: its two queries share one)
        c["B"], c["start"], c["goal"] = B, np.ascontiguousarray(q[:B]), np.ascontiguousarray(q[first:first + B])
        if near is not None:      # goals a short way from the starts: start (+) near * uniform(-1, 1) per DoF
            import pose_numpy as P
            v = near * np.random.default_rng(1310).uniform(-1.0, 1.0, size=(B, model.nv))
            c["goal"] = np.ascontiguousarray(np.stack([P.integrate(model, a, d) for a, d in zip(c["start"], v)]))
        ends = np.concatenate([c["start"], c["goal"]])
        c["margin"] = float(np.quantile(MN.clearance_min(model, ends, c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"]), 0.1))
        import pose_limits_numpy as PL
        qi = PL.limit_q_index(model)
        lo, hi = np.full(model.nv, -np.inf), np.full(model.nv, np.inf)
        ok = qi >= 0
        lo[ok], hi[ok] = ends[:, qi[ok]].min(axis=0) - 0.5, ends[:, qi[ok]].max(axis=0) + 0.5
        c["lo"], c["hi"] = lo, hi
        c["kw"] = dict(dict(step=0.5, max_iters=16, max_nodes=64, seed=4242, margin=c["margin"], tol=TOL, max_evals=MAX_EVALS), **over)
        c["want"] = PN.plan(model, c["start"], c["goal"], c["links"], c["spheres"], lo, hi, T_PLAN, c["ws"], c["wb"], c["pairs"], **c["kw"])
        _CASES[key] = c
    return _CASES[key]


def check_found_paths(model, want, start, goal, links, spheres, ws, wb, pairs, margin, tol, max_evals, dense=33):
    """what a FOUND path claims, on the reference alone; returns the number of found paths"""
    found = np.flatnonzero(want["status"] == PN.FOUND)
    for b in found:
        L, path = int(want["n_waypoints"][b]), want["q_path"][b]
        assert L >= 2 and np.array_equal(path[0], start[b]) and np.array_equal(path[L - 1], goal[b])
        assert np.array_equal(path[L:], np.tile(path[L - 1], (path.shape[0] - L, 1)))
        dv = MN.difference(model, path[:L - 1], path[1:L])
        res = MN.advance(model, path[:L - 1], dv, links, spheres, ws, wb, pairs, margin=margin, tol=tol, max_evals=max_evals)
        assert np.all(res["status"] == MN.FREE), (b, res["status"])
        for k in range(L - 1):
            q = MN.interpolate_many(model, path[k], dv[k], np.linspace(0.0, 1.0, dense))
            assert MN.clearance_min(model, q, links, spheres, ws, wb, pairs).min() >= margin, (b, k)
        assert want["length"][b] == SN._length(model, path[:L]) and want["length"][b] > 0.0
    rest = want["status"] != PN.FOUND
    assert np.isnan(want["q_path"][rest]).all() and np.isnan(want["length"][rest]).all()
    assert np.all(want["n_waypoints"][rest & (want["status"] != PN.TOO_LONG)] == 0)
    return found.size


def test_the_wall_is_planned_around():
    w = wall_case()
    model, A, Bq = w["model"], w["A"], w["Bq"]
    direct = MN.advance(model, A[None], MN.difference(model, A, Bq), w["links"], w["spheres"], (), w["box"][None], margin=0.0, tol=TOL)
    assert direct["status"][0] == MN.BLOCKED and direct["s_free"][0] > 0.0
    for seed in range(4):
        for step in (0.5, 1.0):
            got = PN.plan(model, A, Bq, w["links"], w["spheres"], w["lo"], w["hi"], 16, wboxes=w["box"][None], step=step, max_iters=16, max_nodes=16,
                          seed=seed, tol=TOL)
            assert got["status"][0] == PN.FOUND and got["n_waypoints"][0] >= 3 and got["iterations"][0] >= 1, (seed, step, got["status"])
            assert got["edges"][0][0][2] == MN.BLOCKED
            assert check_found_paths(model, got, A[None], Bq[None], w["links"], w["spheres"], (), w["box"][None], (), 0.0, TOL, 256) == 1
    # without the wall: the 2-waypoint path in 0 iterations
    got = PN.plan(model, A, Bq, w["links"], w["spheres"], w["lo"], w["hi"], 16, step=0.5, max_iters=16, max_nodes=16, tol=TOL)
    assert got["status"][0] == PN.FOUND and got["n_waypoints"][0] == 2 and got["iterations"][0] == 0 and got["edges_checked"][0] == 1
    assert np.array_equal(got["q_path"][0, 0], A) and np.all(got["q_path"][0, 1:] == Bq)


def test_found_paths_are_free_and_every_status_occurs():
    seen = set()
    for name in ("panda7", "talos32"):
        c = plan_case(name)
        want = c["want"]
        print("plan_numpy %s: status %s, L %s, iterations %s, near %d" % (name, want["status"].tolist(), want["n_waypoints"].tolist(),
                                                                          want["iterations"].tolist(), int(want["near"].sum())))
        n = check_found_paths(c["model"], want, c["start"], c["goal"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], c["margin"], TOL, MAX_EVALS)
        assert n > 0
        seen |= set(want["status"].tolist())
        direct = (want["status"] == PN.FOUND) & (want["iterations"] == 0)
        assert np.all(want["n_waypoints"][direct] == 2) and np.all(want["n_waypoints"][(want["status"] == PN.FOUND) & ~direct] >= 3)
        assert np.all(want["edges_checked"] >= want["edges_free"]) and np.all(want["nodes"] <= c["kw"]["max_nodes"])
    assert {PN.FOUND, PN.EXHAUSTED_ITERS, PN.START_BLOCKED, PN.GOAL_BLOCKED} <= seen, seen
    # the three statuses the budgets and the inputs make: two nodes per tree, two rows per path, a NaN start
    c = plan_case("panda7")
    model, want = c["model"], c["want"]
    tree = np.flatnonzero((want["status"] == PN.FOUND) & (want["n_waypoints"] >= 3))
    assert tree.size
    b = int(tree[0])
    args = (model, c["start"][b:b + 1], c["goal"][b:b + 1], c["links"], c["spheres"], c["lo"], c["hi"])
    world = (c["ws"], c["wb"], c["pairs"])

    def alone(T=T_PLAN, **over):
        # (the words of a query depend on its index b: NaN rows, INVALID at once, keep it at row b)
        pad = lambda a: np.concatenate([np.full((b, a.shape[1]), np.nan), a])
        r = PN.plan(model, pad(args[1]), pad(args[2]), *args[3:], T, *world, **dict(c["kw"], **over))
        return {k: v[b] for k, v in r.items()}
    same = alone()
    assert same["status"] == PN.FOUND and np.array_equal(same["q_path"], want["q_path"][b]) and same["length"] == want["length"][b]
    short = alone(T=2)
    assert short["status"] == PN.TOO_LONG and short["n_waypoints"] == want["n_waypoints"][b] and np.isnan(short["q_path"]).all() and np.isnan(short["length"])
    few = alone(max_nodes=2)
    assert few["status"] == PN.EXHAUSTED_NODES and few["nodes"].max() == 2 and few["n_waypoints"] == 0
    bad = args[1].copy()
    bad[0, 1] = np.nan
    inv = PN.plan(model, bad, args[2], *args[3:], T_PLAN, *world, **c["kw"])
    assert inv["status"][0] == PN.INVALID and np.all(inv["nodes"][0] == 0) and inv["edges_checked"][0] == 0


def test_the_outcome_is_a_function_of_the_seed_and_zero_iterations_is_the_direct_check():
    c = plan_case("panda7")
    model, want = c["model"], c["want"]
    args = (model, c["start"], c["goal"], c["links"], c["spheres"], c["lo"], c["hi"], T_PLAN, c["ws"], c["wb"], c["pairs"])
    again = PN.plan(*args, **c["kw"])
    assert all(np.array_equal(again[k], want[k], equal_nan=True) for k in want if k != "edges")
    other = PN.plan(*args, **dict(c["kw"], seed=c["kw"]["seed"] + 1))
    tree = want["iterations"] > 0
    assert tree.any() and not np.array_equal(other["q_path"][tree], want["q_path"][tree], equal_nan=True)
    # the queries a direct check settles do not depend on the seed
    assert all(np.array_equal(other[k][~tree], want[k][~tree], equal_nan=True) for k in want if k != "edges")
    # max_iters = 0 on talos32, whose batch has direct paths
    c = plan_case("talos32")
    model, want = c["model"], c["want"]
    args = (model, c["start"], c["goal"], c["links"], c["spheres"], c["lo"], c["hi"], T_PLAN, c["ws"], c["wb"], c["pairs"])
    zero = PN.plan(*args, **dict(c["kw"], max_iters=0))
    direct = (want["status"] == PN.FOUND) & (want["iterations"] == 0)
    assert direct.any() and np.array_equal(zero["status"] == PN.FOUND, direct) and np.all(zero["iterations"] == 0)
    settled = np.isin(want["status"], (PN.START_BLOCKED, PN.GOAL_BLOCKED, PN.INVALID))
    assert np.array_equal(zero["status"][settled], want["status"][settled]) and np.all(zero["status"][~settled & ~direct] == PN.EXHAUSTED_ITERS)
    assert np.all(zero["edges_checked"] <= 2) and np.all(zero["nodes"] == 1)
    assert np.array_equal(zero["q_path"][direct], want["q_path"][direct])
