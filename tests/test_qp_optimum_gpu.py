"""GPU: every engine against the CERTIFIED optimum of the IK QP (tests/qp_numpy.py), through the C ABI, fp64 handles, the tight settings
of tests/qp_cases.py.  The oracle is not in the loop: an engine and the oracle that shared a misreading of a convention would agree
with each other and both miss x*.

Each entry of tests/test_engines.py's ENGINES table, the pass-by-pass route and the plain default plan are forced in turn on a subset of
the cases that lands on that engine's own ground (Talos-32, 20 joints: k_flat2; Talos-44, 60 joints: k_flat1; a small arm and a bushy
tree: k_tail, the pass route; multi-DoF, composite and helical robots wherever they are taken), in batches of 1, 63 and 130 / 300.  x* is
computed once per (case, batch) -- every instance of a batch up to 64, else the fixed seeded sample qp_cases.sample -- and shared.

Assertions, on what loikb_get and loikb_get_results return (equal bit for bit): z, nu against x*, vis[i] against J_i x*, the stationarity
residual from the engine's own yis and w, and yis, w themselves where the multipliers are unique; bounds 10 x the ORACLE's recorded distance for that (case, batch)
(tests/golden/qp_optimum_measured.json; floor 1e-12) -- the engines legitimately stop an iteration apart from the oracle on near-ties, and
one iteration moves z by about the residual.  No instance is flagged infeasible; every instance converged, except that one the record
names as stalled on the oracle (qp_cases: the penalty rule's flip-flop) may stay unconverged; none is dropped from the comparison.  A plain
solve leaves no pose state: no limit flags, no tasks, q as given.

LOIKB_QP_TABLE=<file> appends one line per (engine, case): instances compared, share certified, the oracle's distance, the engine's."""
import os

import numpy as np
import pytest

import loik_amd
from loik_amd import capi
import qp_cases as C
from test_engines import ENGINES

pytestmark = pytest.mark.gpu
MEASURED = C.measured()
ENV_KEYS = ("LOIKB_LEAN", "LOIKB_FLAT", "LOIKB_FLAT_SPLIT", "LOIKB_FLAT_SLICE", "LOIKB_LEAN_WG_PER_CU", "LOIKB_LEAN_KLO", "LOIKB_LEAN_DECADES",
            "LOIKB_LEAN_ADAPT", "LOIKB_FLAT_BUILD")
ROUTES = dict(ENGINES, default=(dict(), dict()), pass_route=(dict(), dict(flags=capi.OPT_NO_H_CACHE)), pass_logged=(dict(), dict(logging=True)))
HEADLINE = [("talos32_c3", 300)]
GROUND = {
    "default": list(C.GPU_KEYS),
    "flat": HEADLINE + [("tree20", 63), ("tree31", 130), ("talos44_wholebody", 300), ("deep60", 130), ("multidof20", 130), ("composite20", 63),
                        ("helical24", 130)],
    "flat_one_lane": HEADLINE + [("tree20", 63)],
    "flat_sliced": HEADLINE + [("talos44_wholebody", 300)],
    "lean": HEADLINE + [("tree20", 63), ("multidof20", 130), ("composite20", 63)],
    "tail": [("talos32_c3", 63), ("panda7", 63), ("bushy42", 130), ("multidof20", 130), ("composite20", 63)],
    "solve": HEADLINE + [("panda7", 63), ("helical24", 130), ("multidof20", 130), ("composite20", 63)],
    "pass_route": [("bushy42", 130)],      # (a tree too bushy for k_solve whose options rule the on-chip engines out)
    "pass_logged": [("panda7", 63)],       # (a small arm: logging handles run pass by pass)
}
PARAMS = [(e, n, B) for e in ROUTES for n, B in GROUND.get(e, HEADLINE)]
_REF = {}


def _reference(name, B):
    if (name, B) not in _REF:
        wl = C.problem(name, B)
        idx = C.sample(B)
        opt = C.reference(wl, idx)
        C.check_conditions(name, wl, opt)
        _REF[(name, B)] = (wl, idx, opt)
    return _REF[(name, B)]


def _check_route(engine, name, s, st, B):
    plan = s.plan()
    if engine in ("flat", "flat_sliced") and name in ("talos32_c3", "talos44_wholebody"):
        assert st["flat_launches"] >= 1 and st["tail_instances"] == B, (plan, st)
        assert ("k_flat2" if name == "talos32_c3" else "k_flat1") in plan, plan
        assert (st["lean_requeues"] > 0) == (engine == "flat_sliced"), st
    if engine == "flat_one_lane" and name == "talos32_c3":
        assert st["flat_launches"] >= 1 and st["flat_split_launches"] == 0, (plan, st)
    if engine == "lean":
        assert st["flat_launches"] == 0, (plan, st)
        if name == "talos32_c3":
            assert st["lean_launches"] >= 1 and st["tail_instances"] == B, (plan, st)
    if engine == "tail" and name in ("talos32_c3", "panda7"):   # (a tree too bushy for k_solve goes whole to an on-chip engine)
        assert st["lean_launches"] == 0 and st["flat_launches"] == 0 and st["tail_instances"] > 0, (plan, st)
    if engine == "solve":
        assert st["tail_instances"] == 0 and st["flat_launches"] == 0 and st["lean_launches"] == 0, (plan, st)
    if engine in ("pass_route", "pass_logged"):
        assert "k_pass_solve" in plan and st["tail_instances"] == 0, (plan, st)
    if engine == "flat" and name == "tree20":   # (17..32 joints, depth-first: two lanes per joint)
        assert "k_flat2" in plan and st["flat_launches"] >= 1 and st["tail_instances"] == B, (plan, st)
    if engine == "flat" and name == "tree31":   # (the planner gives this 31-joint tree to k_lean, not to k_flat2: whole batch on chip)
        assert st["lean_launches"] >= 1 and st["tail_instances"] == B, (plan, st)
    if engine == "flat" and name == "deep60":
        assert "k_flat1" in plan and st["flat_launches"] >= 1, (plan, st)
    # the forced mixtures of test_engines.ENGINES, as test_every_engine_matches_the_oracle proves them
    if engine == "hybrid":
        assert st["lean_launches"] == 0 and st["tail_instances"] > 0, (plan, st)
    if engine in ("hybrid_lean", "hybrid_flat"):
        assert st["lean_launches"] >= 1 and 0 < st["tail_instances"] < B and (st["flat_launches"] >= 1) == (engine == "hybrid_flat"), (plan, st)
    if engine in ("flat_builds", "flat_builds_sliced"):
        assert st["flat_split_launches"] >= 1 and st["flat_built"] > 0 and st["lean_escaped"] == 0 and st["tail_instances"] == B, (plan, st)
    if engine in ("lean_escapes", "flat_escapes"):
        assert st["lean_launches"] >= 1 and st["lean_escaped"] > 0 and (st["flat_launches"] >= 1) == (engine == "flat_escapes"), (plan, st)


@pytest.mark.parametrize("engine,name,B", PARAMS)
def test_engine_converges_to_the_certified_optimum(engine, name, B, monkeypatch):
    wl, idx, opt = _reference(name, B)
    rec = MEASURED[C.key(name, B)]
    env, kw = ROUTES[engine]
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = loik_amd.BatchedLoik(wl["model"], B, **wl["prm"], **kw)
    if wl["refs"] is None:
        s.Solve(*C.solve_args(wl))
    else:
        s.SolveInit(*C.solve_args(wl)); s.UpdateReferences(*wl["refs"]); s.Solve()
    st = s.stats()
    _check_route(engine, name, s, st, B)
    conv = np.asarray(s.get("converged")).astype(bool)
    assert not np.asarray(s.get("primal_infeasible")).any(), (engine, name)
    # every instance converged, but for instances the record names as stalled on the oracle (none is left out: a stalled instance the
    # engine does converge on is compared with x* like any other.  The flip-flop of mu is chaotic -- which of the marginal instances
    # leave it within max_iter differs between two summation orders -- so the engine's set is a subset of the record's, not its equal)
    lost = sorted(set(np.flatnonzero(~conv).tolist()) - set(rec["not_converged"]))
    assert not lost, (engine, name, lost, rec["not_converged"], s.get("iter")[lost])
    got = {k: np.asarray(s.get(k)) for k in ("z", "nu", "w", "yis", "vis")}
    res = s.get_results()
    for k in got:
        assert np.array_equal(res[k], got[k]), k
    got = {k: v[idx] for k, v in got.items()}
    got["vis"] = np.concatenate([np.zeros((idx.size, 1, 6)), got["vis"]], axis=1)   # (row 0: the universe)
    f = C.figures(opt, got)
    live = conv[idx] & opt["certified"]
    assert live.sum() >= 0.9 * idx.size
    bad, row = [], []
    for m in C.FIGURES:
        worst = C.worst(f[m][live])
        assert (worst is None) == (rec[m] is None), (engine, name, m)
        if worst is None:   # (y, w of a case whose multipliers are not unique: covered by the stationarity residual)
            continue
        row.append("%s %.2e / %.2e" % (m, rec[m], worst))
        if worst > max(10.0 * rec[m], C.FLOOR):
            bad.append((m, worst, rec[m]))
    line = "%-18s %-22s compared %3d certified %5.1f %%  oracle / engine: %s" % (engine, C.key(name, B), int(live.sum()),
                                                                                100.0 * opt["certified"].mean(), "  ".join(row))
    print(line)
    if os.environ.get("LOIKB_QP_TABLE"):
        with open(os.environ["LOIKB_QP_TABLE"], "a") as fh:
            fh.write(line + "\n")
    assert not bad, (engine, name, B, bad)
    # a plain solve leaves the pose layer alone
    assert s.pose_tasks() == [] and np.array_equal(np.asarray(s.get("q")), wl["q"])
    with pytest.raises(loik_amd.LoikError):
        s.pose_limit_flags()
    s.close()


# ---- single precision -------------------------------------------------------------------------------------------------------------------
# A float handle cannot reach 1e-10.  What the project pins for a CONVERGED fp32 solve is test_fp32_parity.CONTRACT_PINS: p99 of
# |z_f32 - z_f64|_inf over the instances that converge in both, tol_abs = 1e-3, on three families.  Here: every entry of
# test_fp32_parity.ENGINES32 that runs on one of those families, F32 handles, the contract's own problems (inputs exact in fp32), and
#     p99 |z_f32 - x*|_inf  <=  the pin's p99  +  the fp64 oracle's largest distance to x* at the same settings on the same instances
# (tests/golden/qp_optimum_measured.json "fp32:<family>", measured on the CPU) -- the triangle inequality, no new fp32 number.  The
# ENGINES32 entries on robots without such a pin (tree21, tree80, panda7, the bushy tree) have no recorded contract to bound them by.
from test_fp32_parity import CONTRACT_PINS, ENGINES32   # noqa: E402

FAMILY32 = {"talos32": "talos32", "talos44": "talos44_wholebody"}
PARAMS32 = [(e, FAMILY32[v[2]]) for e, v in ENGINES32.items() if v[2] in FAMILY32] + [("default-multidof", "multidof")]
_REF32 = {}


@pytest.mark.parametrize("engine,family", PARAMS32)
def test_fp32_engine_stays_within_its_contract_of_the_certified_optimum(engine, family, monkeypatch):
    if family not in _REF32:
        _REF32[family] = C.fp32_reference(family)
    model, wl, prm, idx, opt, _, conv64 = _REF32[family]
    rec = MEASURED["fp32:" + family]
    assert opt["certified"].mean() >= 0.95
    env, kw, _, ran = ENGINES32.get(engine, (dict(), dict(), None, None))
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B = wl["q"].shape[0]
    s = loik_amd.BatchedLoik(model, B, precision=capi.F32, **prm, **kw)
    s.Solve(*C.solve_args(wl))
    st = s.stats()
    assert st["flat_launches"] == 0, (s.plan(), st)   # (the flat engines are fp64 only)
    if ran is not None:
        assert ran(st, B), (engine, s.plan(), st)
    z = np.asarray(s.get("z"))[idx]
    both = np.asarray(s.get("converged")).astype(bool)[idx] & conv64 & opt["certified"]
    assert both.mean() > 0.5, (engine, both.mean())
    dz = np.abs(z - opt["x"]).max(axis=1)[both]
    p99 = float(np.quantile(dz, 0.99))
    bound = CONTRACT_PINS[family][0] + rec["z_max"]
    line = "%-22s fp32 %-18s compared %3d certified %5.1f %%  oracle z %.2e  pin %.1e  engine p99 %.2e max %.2e (bound %.2e)" % (
        engine, family, int(both.sum()), 100.0 * opt["certified"].mean(), rec["z_max"], CONTRACT_PINS[family][0], p99, float(dz.max()), bound)
    print(line)
    if os.environ.get("LOIKB_QP_TABLE"):
        with open(os.environ["LOIKB_QP_TABLE"], "a") as fh:
            fh.write(line + "\n")
    assert p99 <= bound, (engine, family, p99, bound)
    s.close()
