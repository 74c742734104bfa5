"""CPU-only first-principles pins of the oracle (no upstream golden vectors exist):
the converged answer must (i) satisfy the kinematics v_i = J_i(q) nu with an independently computed Jacobian,
(ii) satisfy the task and box constraints, (iii) coincide with the solution of the reduced dense QP
   min_nu sum_i 1/2 |J_i nu - v_ref|^2_Href  s.t.  A J_c nu = b,  lb <= nu <= ub
obtained from scipy's SLSQP -- an algorithm that shares nothing with LoIK's ADMM / tree recursion.

Narrow on purpose (three 1-DoF robots, one constraint, H_ref = I, SLSQP good to 2e-4): tests/test_qp_optimum_cpu.py pins the oracles'
converged primal and dual answer to the certified QP optimum (tests/qp_numpy.py) on the joint types and formulations of
tests/qp_cases.py, six orders tighter, and tests/test_qp_optimum_gpu.py does the same for every engine.  Neither file pins iteration counts, the stopping and infeasibility logic, the tail solve or bit-parity with upstream."""
import numpy as np
import pytest
from scipy.optimize import minimize

from loik_amd import workloads
from oracle import ref
from helpers import FIXTURE, feasible_batch, problem_args, random_tree


def jacobian(model, q, link):
    J = np.zeros((6, model.nv))
    for k in range(model.nv):
        e = np.zeros((1, model.nv))
        e[0, k] = 1.0
        J[:, k] = workloads.link_velocity(model, q[None], e, link)[0]
    return J


@pytest.mark.parametrize("which", ["panda7", "panda9", "tree"])
def test_converged_solution_is_the_qp_optimum(which, request):
    model = random_tree(4, 9) if which == "tree" else request.getfixturevalue(which)
    link = model.njoints - 1 if which != "panda9" else model.getJointId("panda_joint7")
    wl = feasible_batch(model, 3, link, 17, bound=0.5, nu_scale=0.5)
    for b in range(3):
        s = ref.RefSolver(model, **dict(FIXTURE, max_iter=3000, tol_abs=1e-9, tol_rel=0.0, tol_primal_inf=1e-12))
        s.Solve(*problem_args(wl, b))
        assert s.get_convergence_status(), s.get_iter()
        q, nu, z = wl["q"][b], s.nu, s.z
        Js = [jacobian(model, q, i) for i in range(1, model.njoints)]
        # (i) kinematics
        for i in range(1, model.njoints):
            assert np.max(np.abs(Js[i - 1] @ nu - s.vis[i])) < 1e-12
        # (ii) feasibility
        A, bb = wl["Ais"][0], wl["bis"][b, 0]
        assert np.max(np.abs(A @ s.vis[link] - bb)) < 1e-8
        assert np.all(z >= wl["lb"] - 1e-12) and np.all(z <= wl["ub"] + 1e-12) and np.max(np.abs(nu - z)) < 1e-8
        # (iii) optimality against an unrelated QP method
        Hq = sum(J.T @ J for J in Js)
        Jc = A @ Js[link - 1]
        res = minimize(lambda x: 0.5 * x @ Hq @ x, np.zeros(model.nv), jac=lambda x: Hq @ x, method="SLSQP",
                       bounds=list(zip(wl["lb"], wl["ub"])),
                       constraints=[dict(type="eq", fun=lambda x: Jc @ x - bb, jac=lambda x: Jc)],
                       options=dict(ftol=1e-15, maxiter=500))
        assert res.success
        assert abs(0.5 * z @ Hq @ z - res.fun) < 1e-7 * max(1.0, abs(res.fun))
        assert np.max(np.abs(z - res.x)) < 2e-4


def test_infeasible_target_is_flagged(talos):
    """the reference fixture's head target is not reachable by a 4-joint chain: OSQP-style certificate + tail solve
    (loik-loid-optimized.hxx:572-606, loik-loid-optimized.hpp:271-319)"""
    from helpers import fixture_problem
    p = fixture_problem(talos, bound=4.0)
    s = ref.RefSolver(talos, **dict(FIXTURE, max_iter=200))
    s.Solve(*problem_args(p))
    assert s.get_primal_infeasibility_status() and not s.get_convergence_status()
    assert s.get_iter() < 200
