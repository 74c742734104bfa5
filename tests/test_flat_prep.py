"""The prepared records of fresh instances (loik_amd/csrc/loik_flat_prep.hpp): k_fslots writes down the world placements, S^w, the
constraint blocks at the world origin and the record's scalars of every listed instance, and k_flat2 takes a fresh instance from that
block instead of setting it up from the tile records a second time.  Every case runs twice, LOIKB_FLAT_PREP=0 (the old load) and =1:
the bytes of get_results() must be equal, and the answer is compared with the oracle through helpers.assert_end_to_end with the
tolerances of tests/test_flat_instantiations.py.  Shapes: the smallest at which the block's layout or k_fslots' lane groups can go
wrong (see each test)."""
import numpy as np
import pytest

import flat_census as C
import helpers
import loik_amd
from helpers import assert_end_to_end, fetch_end_to_end
from loik_amd import workloads
from oracle import ref

pytestmark = pytest.mark.gpu

TOL = dict(same_frac=0.99, ztol=1e-9, off_ztol=1e-5)
SWITCHES = C.ENV_NAMES + ("LOIKB_FLAT_PREP", "LOIKB_FLAT_ZERO_STATE", "LOIKB_TRACE")


def _args(wl):
    return (wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])


def _both(monkeypatch, capfd, model, B, prm, run, env=(), kernel="k_flat2", check=None):
    """`run(handle)` under LOIKB_FLAT_PREP=0 and =1 on fresh handles: equal bytes in every field of get_results(); returns what
    fetch_end_to_end reads from the second.  The launches' trace lines (LOIKB_TRACE=1) say which load the launch used."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(env).items():
        monkeypatch.setenv(k, v)
    res, got = {}, None
    for prep in ("0", "1"):
        monkeypatch.setenv("LOIKB_FLAT_PREP", prep)
        monkeypatch.setenv("LOIKB_TRACE", "1")
        s = loik_amd.BatchedLoik(model, B, **prm)
        capfd.readouterr()
        run(s)
        lines = [l for l in capfd.readouterr().err.splitlines() if "flat engine:" in l]
        st = s.stats()
        assert kernel in s.plan(), s.plan()
        assert st["flat_launches"] >= 1 and st["tail_instances"] == B, st
        # (a solve's first launch takes the records; no launch does without the switch, or on k_flat1)
        taken = sum("prepared records" in l for l in lines)
        assert len(lines) >= 1 and (taken >= 1 if prep == "1" and kernel == "k_flat2" else taken == 0), (prep, lines)
        if check is not None:
            check(st)
        res[prep] = s.get_results()
        got = fetch_end_to_end(s)
        s.close()
    assert set(res["0"]) == set(res["1"])
    for k in res["0"]:
        a, b = np.asarray(res["0"][k]), np.asarray(res["1"][k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, "LOIKB_FLAT_PREP=0 and =1 differ")
    return got


def _cold(monkeypatch, capfd, wl, model, prm, what, **kw):
    B = wl["q"].shape[0]
    got = _both(monkeypatch, capfd, model, B, prm, lambda s: C.solve(s, wl) if "refs" in wl else s.Solve(*_args(wl)), **kw)
    out = ref.solve_batch(model, *_args(wl), nthreads=8, want_nu=True, refs=wl.get("refs"), **prm)
    assert_end_to_end(got, out, prm, what=what, **TOL)


def _leaves(model, n):
    parents = set(int(p) for p in model.parents[1:])
    return [i for i in range(1, model.njoints) if i not in parents][:n]


@pytest.mark.parametrize("carrier", [C.S17, C.C32])
def test_edge_trees(carrier, monkeypatch, capfd):
    """star(17): no ancestors, no pointer-jumping round (njmp = 0), fifteen idle lanes per half; comb(32,11): the deepest tree k_flat2
    takes, no idle lane"""
    wl = C.plain_workload(carrier)
    prm = C.params(wl, False, **C.END_TO_END)
    got = _both(monkeypatch, capfd, wl["model"], 130, prm, lambda s: C.solve(s, wl))
    assert_end_to_end(got, C.oracle_end_to_end(wl, False), prm, what=carrier, **TOL)


@pytest.mark.parametrize("B", [1, 2, 3, 65, 2049])
def test_batches(B, monkeypatch, capfd):
    """k_fslots holds two instances per wavefront: an odd batch leaves its last wavefront's second lane group without an instance; 2049
    is the first batch beyond the short sequence (ring fill, order pass)"""
    wl = workloads.talos_c3(B, seed=70 + B % 7)
    prm = dict(wl["params"], max_iter=400)
    _cold(monkeypatch, capfd, wl, wl["model"], prm, "talos32 B=%d" % B)


@pytest.mark.parametrize("nc,per_instance_A", [(1, False), (1, True), (3, False), (3, True)])
def test_constraint_blocks(nc, per_instance_A, monkeypatch, capfd):
    """one and three task constraints on talos32 (three blocks fill most of the rows k_fslots builds them in), A shared by the batch
    (from the uniform inputs) and per instance (from the records)"""
    model = loik_amd.builtin_model("talos32")
    wl = helpers.multi_task_batch(model, 65, _leaves(model, nc), 81 + nc, nu_scale=0.3, per_instance_A=per_instance_A)
    prm = C.params(dict(num_eq_c=nc), False, **C.END_TO_END)
    _cold(monkeypatch, capfd, wl, model, prm, "talos32 nc=%d per-instance A=%s" % (nc, per_instance_A))


@pytest.mark.parametrize("hm", [0, 1, 2, 3])
def test_reference_weights(hm, monkeypatch, capfd):
    """H_ref = h I, diagonal, general and per link, each with a target (H_ref v_ref != 0: the reference term's subtree sums run in the
    new load too); per link: two constraint blocks in different subtrees"""
    wl = C._workload(C.C32, 130, hm, False, C.seed_of(C.C32, 130, hm, False))
    prm = C.params(wl, False, **C.END_TO_END)
    got = _both(monkeypatch, capfd, wl["model"], 130, prm, lambda s: C.solve(s, wl))
    assert_end_to_end(got, C.oracle_end_to_end(wl, False), prm, what="hm %d" % hm, **TOL)


@pytest.mark.parametrize("per_instance", [False, True])
def test_bounds(per_instance, monkeypatch, capfd):
    """the box shared by the batch (uniform inputs) and per instance (rows of the block)"""
    model = loik_amd.builtin_model("talos32")
    wl = helpers.feasible_batch(model, 65, _leaves(model, 1)[0], 91, nu_scale=0.3, per_instance_bounds=per_instance)
    prm = C.params(dict(num_eq_c=1), False, **C.END_TO_END)
    _cold(monkeypatch, capfd, wl, model, prm, "bounds per instance=%s" % per_instance)


def test_helical_and_prismatic_joints(monkeypatch, capfd):
    """S^w of a helical joint carries the pitch term, of a prismatic joint only its linear half: comb(32,11) with three of its revolute
    joints turned helical (helpers.helical_tree's recipe on a tree k_flat2 takes)"""
    m = C.model_of(C.C32)
    rng = np.random.default_rng(97)
    jt, pitch = m.jtype.copy(), np.zeros(m.njoints)
    rev = [i for i in range(1, m.njoints) if int(jt[i]) in (1, 2, 3, 7)]
    for i in rng.choice(rev, size=3, replace=False):
        jt[i] = 22 if int(jt[i]) == 7 else 19 + (int(jt[i]) - 1)
        pitch[i] = float(rng.choice([-1.0, 1.0]) * rng.uniform(0.05, 0.3))
    model = loik_amd.Model(m.parents, jt, m.axis, m.placement, q_lo=m.q_lo, q_hi=m.q_hi, pitch=pitch, name="comb_32_11_helical")
    assert any(int(t) in (4, 5, 6, 8) for t in jt[1:]) and np.count_nonzero(pitch) == 3
    wl = helpers.feasible_batch(model, 65, C.deepest_joint(model), 92, nu_scale=0.3)
    prm = C.params(dict(num_eq_c=1), False, **C.END_TO_END)
    _cold(monkeypatch, capfd, wl, model, prm, "comb(32,11) with helical joints")


def test_warm_started_tailored_sequence(monkeypatch, capfd):
    """Solve(q, c_id, Ai, bi) three times on a warm-started handle, q and A changing between the calls: the geometry comes from the
    block, the state from the tiles, and the first iteration uses the A^T y of the matrix the instance arrives with"""
    B = 65
    wl = workloads.talos_c3(B, seed=93)
    model, link = wl["model"], int(wl["c_ids"][0])
    prm = dict(wl["params"], max_iter=400)
    rng = np.random.default_rng(94)
    # (steps small enough that the oracle still converges on 64 of the 65 instances)
    steps = [(wl["q"] + 0.005 * (k + 1) * rng.normal(size=wl["q"].shape), np.asarray(wl["Ais"]) + 0.01 * (k + 1) * rng.normal(size=(1, 6, 6)),
              (1.0 - 0.2 * (k + 1)) * wl["bis"][:, 0]) for k in range(3)]

    def run(s):
        s.set_warm_start(True)
        s.Solve(*_args(wl))
        for q, A, b in steps:
            s.Solve(q, link, A, b)

    got = _both(monkeypatch, capfd, model, B, prm, run)
    out = dict(iters=np.zeros(B, int), converged=np.zeros(B, bool), primal_infeasible=np.zeros(B, bool), z=np.zeros_like(got["z"]),
               nu=np.zeros_like(got["nu"]), primal_residual=np.zeros(B), dual_residual=np.zeros(B))
    for i in range(B):
        r = ref.RefSolver(model, **prm)
        r.set_warm_start(True)
        r.Solve(wl["q"][i], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"][i], wl["lb"], wl["ub"])
        for q, A, b in steps:
            r.Solve(q[i], link, A, b[i])
        out["iters"][i], out["converged"][i], out["primal_infeasible"][i] = r.get_iter(), r.get_convergence_status(), r.get_primal_infeasibility_status()
        out["z"][i], out["nu"][i] = r.field("z"), r.field("nu")
        out["primal_residual"][i], out["dual_residual"][i] = r.scalar("primal_residual"), r.scalar("dual_residual")
    assert_end_to_end(got, out, prm, what="warm-started tailored sequence", **TOL)


def test_time_sliced_launch_with_a_narrow_window(monkeypatch, capfd):
    """32 768 instances in arrival order: a time-sliced launch; k_fslots builds two decades of the table only.  Fresh loads from the
    block, unparks and in-wave builds of decade slots all occur in the one launch."""
    B = 32768
    wl = workloads.talos_c3(B, seed=95)
    prm = dict(wl["params"])

    def check(st):
        assert st["flat_split_launches"] == 1 and st["lean_requeues"] > 0 and st["flat_built"] > 0 and st["lean_escaped"] == 0, st

    got = _both(monkeypatch, capfd, wl["model"], B, prm, lambda s: s.Solve(*_args(wl)), env=dict(LOIKB_FLAT_BUILD="1", LOIKB_FLAT_WINDOW="0,2"), check=check)
    idx = np.arange(0, B, 64)
    sub = (wl["q"][idx], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"][idx], wl["lb"], wl["ub"])
    out = ref.solve_batch(wl["model"], *sub, nthreads=8, want_nu=True, **prm)
    assert_end_to_end({k: v[idx] for k, v in got.items()}, out, prm, what="time-sliced, window of two", **TOL)


def test_whole_body_stays_on_its_own_load(monkeypatch, capfd):
    """talos44 runs k_flat1, which keeps the load from the tile records: the switch changes nothing there"""
    B = 65
    wl = workloads.talos_wholebody(B, seed=96)
    prm = dict(wl["params"], max_iter=400)
    got = _both(monkeypatch, capfd, wl["model"], B, prm, lambda s: s.Solve(*_args(wl)), kernel="k_flat1")
    out = ref.solve_batch(wl["model"], *_args(wl), nthreads=8, want_nu=True, **prm)
    assert_end_to_end(got, out, prm, what="talos44", **TOL)
