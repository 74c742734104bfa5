"""CPU: the oracles against the CERTIFIED optimum of the IK QP (tests/qp_numpy.py) -- the pin of the converged answer that does not
pass through another restatement of the solver.

What is compared, for every case of tests/qp_cases.py (model families x formulations, the tight settings there): z and nu against x*,
vis[i] against J_i x*, and the stationarity residual P z + c + sum_c J_c^T A_c^T y_c + w built from the SOLVER's duals and the
independent Jacobians.

The duals' convention, from the reference's formulation (the ADMM's updates y_c += mu_eq (A_c v_c - b_c), w += mu (nu - z)): `yis[c]` is
the multiplier of A_c J_c nu = b_c and `w` that of nu = z, both entering the Lagrangian with a PLUS sign and unscaled, so that at the
optimum P z + c + sum_c J_c^T A_c^T yis_c + w = 0 with w_k >= 0 where z_k sits on its upper bound, <= 0 on the lower one, 0 inside.

Tolerances are measured on the oracle, never on a kernel: tests/golden/qp_optimum_measured.json (tests/golden/make_qp_optimum_measured.py
writes it) holds, per case, the oracle's largest distance; the oracle must stay within 2x of it (another libm or compiler), with an
absolute floor of 1e-12.  A compared instance that does not converge fails the test."""
import numpy as np
import pytest

from loik_amd import capi, workloads
import pose_numpy as P
import qp_cases as C
import qp_numpy as Q

MEASURED = C.measured()
JACOBIAN_MODELS = ["panda7", "talos32", "talos44", "tree20", "tree35", "deep60", "bushy42", "helical24", "multidof20", "composite20",
                   "talos32_bfs", "tree31", "multidof9"]


@pytest.mark.parametrize("name", JACOBIAN_MODELS)
def test_jacobian_three_ways(name):
    """J from its definition (qp_numpy.jacobians), against (a) a central finite difference of pose_numpy.fk through log6 -- the twist of
    oMi(q)^-1 oMi(q (+) h v) is h J_i v + O(h^2), the difference of the two sides O(h^3): h = 1e-4 leaves 1e-8 |v|^3-ish on a twist
    quotient of O(1), rounding 1e-16 / h = 1e-12 -- and (b) workloads.link_velocity, the recursion the workloads are built with (the same
    algebra in another order: rounding only).  For a composite joint the three are less than independent: all of them write the joint
    out as its sub-joints through workloads._Chain (indices and placements), so a mistake THERE passes here; what pins the expansion is
    tests/test_composite.py (the universal joint by hand, composites against their written-out chain models)."""
    model = C.model_of(name)
    rng = np.random.default_rng(31)
    B, h = 3, 1e-4
    q = model.random_configurations(rng, B)
    links = sorted({1, model.njoints // 2, model.njoints - 1} | {int(l) for l in rng.integers(1, model.njoints, size=3)})
    J = Q.jacobians(model, q, links)
    V = rng.normal(size=(B, model.nv))
    worst_fd = 0.0
    for n, l in enumerate(links):
        want = workloads.link_velocity(model, q, V, l)
        got = np.einsum("bij,bj->bi", J[:, n], V)
        assert np.max(np.abs(got - want)) < 1e-12 * max(1.0, np.abs(want).max()), (name, l, np.max(np.abs(got - want)))
        for b in range(B):
            R0, t0 = P.fk(model, q[b:b + 1], l)
            tw = []
            for sgn in (1.0, -1.0):
                R1, t1 = P.fk(model, P.integrate(model, q[b], sgn * h * V[b])[None], l)
                tw.append(P.log6(R0[0].T @ R1[0], R0[0].T @ (t1[0] - t0[0])))
            fd = (tw[0] - tw[1]) / (2 * h)
            worst_fd = max(worst_fd, np.max(np.abs(fd - got[b])) / max(1.0, np.abs(got[b]).max()))
    assert worst_fd < 1e-6, (name, worst_fd)
    # zero off the root path: a DoF of a joint that is no ancestor of the link moves nothing
    ch, link_of = Q._chain(model)
    for n, l in enumerate(links):
        on_path, j = set(), int(link_of[l])
        while j > 0:
            on_path.update(range(int(ch.idx_v[j]), int(ch.idx_v[j]) + Q._nv(ch, j)))
            j = int(ch.parents[j])
        off = [k for k in range(model.nv) if k not in on_path]
        assert not J[:, n][:, :, off].any()
        assert np.all(np.abs(J[:, n][:, :, sorted(on_path)]).max(axis=1) > 0)


def test_active_set_solver_on_a_problem_with_a_known_answer():
    """min 1/2 |x - a|^2 s.t. sum x = 1, 0 <= x <= 0.6: the projection of a onto the capped simplex, x = clip(a - t, 0, 0.6) with t from the
    sum.  By hand for a = (2, 0.5, -1, 0): t = 0.1, x = (0.6, 0.4, 0, 0) -- x1 on its upper bound, x3 and x4 on the lower one"""
    a = np.array([2.0, 0.5, -1.0, 0.0])
    s = Q.solve_qp(np.eye(4), -a, np.ones((1, 4)), np.array([1.0]), np.zeros(4), 0.6 * np.ones(4))
    assert s["cert"]["certified"], s["cert"]
    assert np.allclose(s["x"], [0.6, 0.4, 0.0, 0.0], rtol=0, atol=1e-15)
    assert list(s["side"]) == [1, 0, -1, -1] and s["w"][0] > 0 and s["w"][2] < 0 and s["w"][3] < 0
    # a rank-deficient equality block (a zero row and a repeated one) and an infeasible one
    E = np.array([[1.0, 1, 1, 1], [0, 0, 0, 0], [2, 2, 2, 2]])
    s2 = Q.solve_qp(np.eye(4), -a, E, np.array([1.0, 0.0, 2.0]), np.zeros(4), 0.6 * np.ones(4))
    assert s2["cert"]["certified"] and s2["cert"]["rank_E"] == 1 and np.allclose(s2["x"], s["x"], rtol=0, atol=1e-15)
    s3 = Q.solve_qp(np.eye(4), -a, np.ones((1, 4)), np.array([3.0]), np.zeros(4), 0.6 * np.ones(4))
    assert not s3["cert"]["certified"]
    # a certificate refuses a perturbed point and a multiplier of the wrong sign
    bad = Q.certify(np.eye(4), -a, np.ones((1, 4)), np.array([1.0]), np.zeros(4), 0.6 * np.ones(4), s["x"] + 1e-9, s["y"], s["w"], s["side"])
    assert not bad["certified"]
    bad = Q.certify(np.eye(4), -a, np.ones((1, 4)), np.array([1.0]), np.zeros(4), 0.6 * np.ones(4), s["x"], s["y"], -s["w"], s["side"])
    assert not bad["signs_ok"] and not bad["certified"]


def test_the_schedules_the_flat_engines_need():
    """the deep 60-joint tree and the bushy one are trees capi.flat_schedule accepts: the robots the flat engines exist for"""
    for name in ("deep60", "bushy42", "tree20", "tree35"):
        assert capi.flat_schedule(C.model_of(name).parents) is not None, name


def _compare(name, B, solver, key):
    wl = C.problem(name, B)
    idx = C.sample(B)
    opt = C.reference(wl, idx)
    C.check_conditions(name, wl, opt)
    got = C.oracle_solve(wl, idx, solver)
    assert got["converged"].all() and not got["infeasible"].any(), (name, got["iter"], got["converged"])
    f = C.figures(opt, got)
    rec = MEASURED[key]
    bad = []
    for m in C.FIGURES:
        worst = C.worst(f[m])
        assert (worst is None) == (rec[m] is None), (key, m)
        if worst is None:   # (y, w: no instance of the case has unique multipliers -- rank-3 task matrices)
            continue
        print("%s %s: oracle %.3e (recorded %.3e)" % (key, m, worst, rec[m]))
        if worst > max(2.0 * rec[m], C.FLOOR):
            bad.append((m, worst, rec[m]))
    assert not bad, (key, bad)
    assert rec["instances"] == idx.size and rec["certified"] == int(opt["certified"].sum()), (key, rec, int(opt["certified"].sum()))
    # the duals themselves where the reference's are unique: strict complementarity and a task block of full row rank
    for k in np.flatnonzero(opt["certified"]):
        c = opt["certs"][k]
        if c["rank_E"] == 6 * len(wl["c_ids"]) and c["min_active_multiplier"] > 1e-3 and c["min_free_gap"] > 1e-3:
            assert np.array_equal(np.sign(got["w"][k]) * (np.abs(got["w"][k]) > 1e-6), np.sign(opt["w"][k])), (key, k)
    return f


@pytest.mark.parametrize("name", list(C.CASES))
def test_c_oracle_converges_to_the_certified_optimum(name):
    _compare(name, C.CPU_BATCH, "ref", C.key(name, C.CPU_BATCH))


@pytest.mark.parametrize("name", list(C.DENSE_CASES))
def test_dense_oracle_converges_to_the_certified_optimum(name):
    """oracle/dense.py (the plain solver with the explicit QP) at the sizes it is practical at, and the C oracle on the same problems"""
    _compare(name, 3, "dense", C.key(name, 3) + ":dense")
    _compare(name, 3, "ref", C.key(name, 3))


def test_the_record_says_where_it_comes_from():
    p = MEASURED["_provenance"]["settings"]
    assert p["tol_abs"] == C.TIGHT["tol_abs"] and p["tol_rel"] == 0.0 and p["max_iter"] == C.TIGHT["max_iter"]
    expected = ({C.key(n, C.CPU_BATCH) for n in C.CASES} | {C.key(n, 3) for n in C.DENSE_CASES}
                                               | {C.key(n, 3) + ":dense" for n in C.DENSE_CASES} | {C.key(n, B) for n, B in C.GPU_KEYS})
    for n, B in C.GPU_KEYS:   # (the batches of the GPU file: all of a batch up to 64 or the sample of 64, at least 95 % certified)
        rec = MEASURED[C.key(n, B)]
        assert rec["instances"] == min(B, 64) and rec["certified"] >= 0.95 * rec["instances"], (n, B, rec)
    expected |= {"fp32:" + f for f in C.FP32_FAMILIES}
    assert set(MEASURED) - {"_provenance"} == expected
    for n in list(C.CASES) + list(C.DENSE_CASES):
        assert MEASURED[C.key(n, C.CPU_BATCH if n in C.CASES else 3)]["not_converged"] == []


@pytest.mark.parametrize("name,B", [("talos32_c3", 63), ("panda7", 63), ("composite20", 63)])
def test_the_gpu_batches_record_is_the_oracles(name, B):
    """what the GPU file takes from the record is re-derived here for the batches of 63: the instances the C oracle stalls on over the WHOLE
    batch (an index added by hand would excuse an engine there), and the oracle's distances on the compared instances, within 2x"""
    wl = C.problem(name, B)
    rec = MEASURED[C.key(name, B)]
    stalled = C.stalled_instances(wl)
    assert stalled.tolist() == rec["not_converged"], (name, stalled, rec["not_converged"])
    idx = C.sample(B)
    live = ~np.isin(idx, stalled)
    opt = C.reference(wl, idx)
    C.check_conditions(name, wl, opt)
    got = C.oracle_solve(wl, idx[live])
    assert got["converged"].all() and not got["infeasible"].any()
    sub = dict(opt, idx=idx[live], x=opt["x"][live], y=opt["y"][live], w=opt["w"][live], vis=opt["vis"][live], certified=opt["certified"][live],
               certs=[c for c, l in zip(opt["certs"], live) if l],
               qp={k: (v[live] if isinstance(v, np.ndarray) else v) for k, v in opt["qp"].items()})
    f = C.figures(sub, got)
    for m in C.FIGURES:
        worst = C.worst(f[m])
        assert (worst is None) == (rec[m] is None), (name, m)
        assert worst is None or worst <= max(2.0 * rec[m], C.FLOOR), (name, m, worst, rec[m])
