"""Every compiled kernel of the flat engine, by name, against the oracle: one case per instantiation of k_flat2 (18), k_flat1 (14 at
each of NA = 10 and NA = 16) and k_flat (2 that run, 2 that the plan never launches: that is asserted instead), from the recipes of tests/flat_census.py -- tests/test_flat_census.py proves on the CPU
that the recipes cover the instantiation lists of loik_amd/csrc/loik_flat_inst.hpp exactly.  NA is more than a loop bound in these
kernels (the packed ancestor words, the LDS layout, the one-slot / two-slot choice of k_flat1), and the NA = 16 builds used to be reached
by two random trees in their plain variant only.  A second test puts the default launch on every carrier tree the recipes did not
already run plain: the classification's boundaries (depth 11 against 12, depth 17, 17 / 32 / 33 / 64 joints, a full wavefront, subtrees of
exactly a power of two, stars) on the device.  Figures of the MI355X runs: profiles/flat_instantiations_measured.md."""
import time

import numpy as np
import pytest

import loik_amd
import flat_census as C
from helpers import assert_close, assert_end_to_end, assert_solver_info_matches, fetch_end_to_end
from oracle import ref
from test_engines import FIELDS, SCALARS

pytestmark = pytest.mark.gpu


def _handle(wl, B, prm, logging):
    return loik_amd.BatchedLoik(wl["model"], B, logging=logging, **prm)


def _assert_plan(s, kernel, nanc, mur):
    plan = s.plan()
    if kernel is None:   # (flat_census.UNREACHABLE_RECIPES: the plan refuses the flat engine, and says why)
        assert C.plan_kernel(plan)[0] is None and C.NO_FLAT_ENGINE in plan, plan
        return
    assert C.plan_kernel(plan) == (kernel, nanc), plan
    if mur == 1:
        assert "OSQP" in plan, plan
    if mur == 2:
        assert "in-wave" in plan, plan


def _compare(what, wl, B, kernel, nanc, sliced=False, logging=False, mur=0, tol=1e-9):
    """the comparisons of one launch: the plan names the kernel; k iterations field by field; end to end; the SolverInfo lists"""
    t0 = time.time()
    model, osqp = wl["model"], mur == 1
    worst = {}
    for k in C.K_ITERATIONS:
        prm = C.k_params(wl, osqp, k)
        s = _handle(wl, B, prm, logging)
        C.solve(s, wl)
        _assert_plan(s, kernel, nanc, mur)
        st = s.stats()
        if kernel is not None:
            assert st["flat_launches"] >= 1 and st["tail_instances"] == B and st["lean_escaped"] == 0, (s.plan(), st)
        assert np.all(s.get("iter") == k)
        got = {n: s.get(n) for n in FIELDS + SCALARS}
        got["His"] = s.His_full()
        s.close()
        pairs = []
        for b in range(0, B, C.SAMPLE_EVERY):
            r = ref.RefSolver(model, **prm)
            C.solve(r, wl, b)
            for n in FIELDS:
                want = r.field(n)
                pairs.append(("%s b%d k%d" % (n, b, k), got[n][b], want[1:] if n in ("vis", "fis", "g") else want))
            pairs.append(("His b%d k%d" % (b, k), got["His"][b], r.His[1:]))
            for n in SCALARS:
                pairs.append(("%s b%d k%d" % (n, b, k), got[n][b], r.scalar(n)))
        worst[k] = max(C.distance(a, w) for _, a, w in pairs)
        print("CENSUS-K %s k=%d largest abs-or-rel distance to the oracle %.3e (bound %.0e)" % (what, k, worst[k], tol))
        for name, a, w in pairs:
            assert_close(a, w, tol, "%s %s" % (what, name))
    prm = C.params(wl, osqp, **C.END_TO_END)
    out = C.oracle_end_to_end(wl, osqp)
    s = _handle(wl, B, prm, logging)
    C.solve(s, wl)
    _assert_plan(s, kernel, nanc, mur)
    st = s.stats()
    got = fetch_end_to_end(s, residuals=osqp)
    same = got["iter"] == out["iters"]
    dz = np.abs(got["z"] - out["z"]).max(axis=1)
    print("CENSUS-E %s | %s | B %d | k2 %.2e | k7 %.2e | same %.4f | dz %.2e | dz_off %.2e | requeues %d | built %d" % (
        what, model.name, B, worst[2], worst[7], same.mean(), dz[same].max(), dz[~same].max() if (~same).any() else 0.0,
        st["lean_requeues"], st["flat_built"]))
    if kernel is not None:
        assert st["flat_launches"] >= 1 and st["tail_instances"] == B and st["lean_escaped"] == 0, (s.plan(), st)
    else:
        assert st["flat_launches"] == 0, (s.plan(), st)
    assert (st["lean_requeues"] > 0) == sliced, st
    assert (st["flat_built"] > 0) == (mur != 0), st
    if osqp:   # (the arguments of tests/test_engines.py::test_whole_body_osqp_rule_on_the_flat_engine, for the reason written there)
        assert_end_to_end(got, out, prm, same_frac=0.99, ztol=5e-9, off_ztol=1e-5, res_tol=(1e-8, 1e-6), what=what)
    else:
        assert_end_to_end(got, out, prm, same_frac=0.99, ztol=1e-9, off_ztol=1e-5, what=what)
    if logging:
        info, it, tail = s.solver_info(), s.get("iter"), s.get("tail_solve_iter")
        assert info["truncated_instances"] == 0
        for b in (0, B // 2, B - 1):
            r = ref.RefSolver(model, **prm)
            C.solve(r, wl, b)
            assert_solver_info_matches(info, it, tail, b, r, 1e-9)
    s.close()
    print("CENSUS-T %s wall %.2f s" % (what, time.time() - t0))


def _set_environment(monkeypatch, env):
    for k in C.ENV_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("rc", C.RECIPES, ids=[C.inst_id(C.predicted(rc)) for rc in C.RECIPES])
def test_every_compiled_instantiation_against_the_oracle(rc, monkeypatch):
    """One launch per compiled kernel.  That the launch IS that kernel is read off what the host says: the plan names k_flat2 / k_flat1 /
    k_flat and the ancestors per joint (<= 10: the NA = 10 build, else NA = 16); lean_requeues > 0 exactly in the SLICED builds;
    flat_built > 0 and the plan's rule for MUR = 1 / 2.  loikb_stats cannot tell HM or LOG apart: those two template arguments follow from
    the inputs alone (href_mode of the weight given, the handle's logging flag) through flat_variant, which tests/test_flat_variant.py
    pins input by input -- and a LOG build that did not log, or an HM build that read the wrong weight, fails the comparison itself.
    Tolerances: 1e-9 for decade steps, 1e-8 under OSQP's rule (mu follows the residual ratio: the roundings of two summation orders reach
    mu itself), the figures of tests/test_engines.py for exactly these comparisons.  They hold where the comparison is well posed: the
    batches' seeds are chosen on the CPU so that the oracle converges everywhere and its own fields at the compared instances move by
    less than a tenth of the bound under a rounding of its inputs (tests/test_flat_census.py::test_comparisons_are_well_posed)."""
    inst = C.predicted(rc)
    _set_environment(monkeypatch, C.environment(rc))
    mur = C.mur_of(inst)
    _compare(C.inst_id(inst), C.workload(rc), C.batch_of(rc), inst[0], C.schedule_of(rc.carrier)["nanc"], sliced=C.is_sliced(inst),
             logging=rc.logging, mur=mur, tol=1e-8 if mur == 1 else 1e-9)


@pytest.mark.parametrize("rc", C.UNREACHABLE_RECIPES, ids=[C.inst_id(C.predicted(rc)) + " is not launched" for rc in C.UNREACHABLE_RECIPES])
def test_builds_that_no_launch_reaches(rc, monkeypatch):
    """k_flat<double, 16, LOG> is what flat_kind() makes of a 17..32-joint tree deeper than 11, and the plan never gives it one: its
    row buffers alone leave five wavefronts per CU where the plan asks six (flat_census.UNREACHABLE_RECIPES).  The launch that would
    run the build says so and runs elsewhere; what runs is compared with the oracle like every other case.  If this fails because the
    plan now names k_flat, the two builds have become reachable: move their recipes into flat_census.RECIPES."""
    inst = C.predicted(rc)
    assert inst[:2] == ("k_flat", C.FLAT_MAXA)
    _set_environment(monkeypatch, C.environment(rc))
    _compare(C.inst_id(inst) + " (not launched)", C.workload(rc), C.batch_of(rc), None, None, logging=rc.logging)


_RUN_PLAIN = {rc.carrier for rc in C.RECIPES + C.UNREACHABLE_RECIPES if rc[1:] == (0, False, False, 0, ())}
EDGE_SHAPES = [c for c in C.CARRIER_TABLE if c not in _RUN_PLAIN]


@pytest.mark.parametrize("carrier", EDGE_SHAPES)
def test_edge_shapes_on_the_default_launch(carrier, monkeypatch):
    """the default environment, H_ref = I, on the carriers no recipe ran in the plain variant: with those, every row of
    flat_census.CARRIER_TABLE has run the kernel the table names, unsliced and without a builder, against the oracle --
    comb(32,11) and comb(32,12) differ by one level: the first runs k_flat2, the second would run k_flat<double, 16> and, like the two
    depth-17 trees in 32 lanes, is refused by the plan (test_builds_that_no_launch_reaches)"""
    assert len(EDGE_SHAPES) + len(_RUN_PLAIN & set(C.CARRIER_TABLE)) == len(C.CARRIER_TABLE)
    _set_environment(monkeypatch, {})
    kernel, nanc = C.launched_kernel(carrier), C.CARRIER_TABLE[carrier][3]
    wl = C.plain_workload(carrier)
    assert np.array_equal(wl["H_ref"], np.eye(6))
    _compare("default launch, " + carrier, wl, 130, kernel, nanc)
