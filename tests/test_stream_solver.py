"""The solver core on a caller's stream behind pending work (include/loik_amd.h at loikb_set_stream: the contract).

Every case is one sequence of calls run twice (stream_harness.run_both): on a fresh handle on the null stream with host arrays, and on
a fresh handle moved to a non-blocking stream with loikb_set_stream, a gate in front of EVERY call (asserted closed when the call is
entered), the per-instance inputs in device arrays that hold the neighbouring instance's data until a copy queued behind the gate, and
every getter into a poisoned device array read back through the null stream right after the call.  The two records are compared byte
for byte: the rest of the suite pins the null-stream run to numpy and the oracle, so nothing here needs a tolerance.

Where it is cheap a third run uses a handle created with LOIKB_OPT_OWN_STREAM, host arrays and no gate (the stream is private): byte
for byte against the null-stream run as it is -- the one route that option changes, the flat engine's time slicing, starts at 32 768
instances, far above every batch here."""
import numpy as np
import pytest

import loik_amd
import stream_harness as H
from helpers import FIXTURE, feasible_batch, multi_task_batch
from loik_amd import capi, workloads
from test_engines import ENGINES
from test_flat_sequence import _blocks
from test_formulation_editing import per_link_references

pytestmark = pytest.mark.gpu

ENGINE_ENV = ("LOIKB_LEAN", "LOIKB_FLAT", "LOIKB_FLAT_SPLIT", "LOIKB_FLAT_SLICE", "LOIKB_LEAN_WG_PER_CU", "LOIKB_LEAN_KLO", "LOIKB_LEAN_DECADES",
              "LOIKB_LEAN_ADAPT", "LOIKB_FLAT_BUILD", "LOIKB_CHUNKS", "LOIKB_TRACE", "LOIKB_FLAT_SEQ", "LOIKB_FLAT_SMALL_BATCH")
VECTORS = ["z", "nu", "w", "Stf_plus_w", "r", "Dinv", "vis", "fis", "g", "pis", "UDinv", "His", "liMi", "yis", "Aty", "q", "primal_residual_vec",
           "dual_residual_vec"]
REBUILT = ["UDinv", "His", "pis", "Aty", "g"]
PRM = dict(FIXTURE, max_iter=300, tol_abs=1e-6, tol_rel=0.0)
_WL = {}


def _talos_batch(B, seed):
    if (B, seed) not in _WL:
        talos = loik_amd.builtin_model("talos32")
        _WL[B, seed] = (talos, feasible_batch(talos, B, talos.getJointId("arm_left_7_joint"), seed, nu_scale=0.5))
    return _WL[B, seed]


def _clean(monkeypatch, env=()):
    for k in ENGINE_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(env).items():
        monkeypatch.setenv(k, v)


def _init_args(run, wl):
    return (run.inp(wl["q"]), wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], run.inp(wl["bis"]), wl["lb"], wl["ub"])


def _snap(run, s, tag, names):
    for n in names:
        run.get("%s:%s" % (tag, n), lambda out, n=n: s.get(n, out=out))
    run.put(tag + ":instance_iterations", int(s.stats()["instance_iterations"]))


def _results(run, s, tag):
    """loikb_get_results takes host arrays only: behind a gate, its values recorded as they are"""
    res = run.do(s.get_results, s.RESULT_FIELDS)
    for k in s.RESULT_FIELDS:
        run.put("%s:results:%s" % (tag, k), res[k])


def _core(wl, wl2, names):
    """SolveInit + Solve, solve_full on another batch, integrate, the tailored Solve on the resident q and on a given q"""
    def sequence(run, s):
        run.do(s.SolveInit, *_init_args(run, wl))
        run.do(s.Solve)
        _snap(run, s, "solve", names)
        _results(run, s, "solve")
        run.do(s.Solve, *_init_args(run, wl2))
        _snap(run, s, "full", names)
        run.do(s.integrate, 0.05)
        run.get("integrate:q", lambda out: s.get("q", out=out))
        link = int(wl["c_ids"][0])
        run.do(s.Solve, None, link, wl["Ais"][0], run.inp(wl["bis"][:, 0]))
        _snap(run, s, "tailored", names)
        run.do(s.Solve, run.inp(wl["q"]), link, wl["Ais"][0], run.inp(wl2["bis"][:, 0]))
        _snap(run, s, "tailored q", names)
        _results(run, s, "tailored q")
    return sequence


def _own_stream_too(make_own, sequence, ref, what):
    s = make_own()
    run = H.Run()
    try:
        sequence(run, s)
    finally:
        s.close()
    H.assert_same_records(run.rec, ref, what + ", LOIKB_OPT_OWN_STREAM")


def test_positive_control_a_misordered_read_is_seen():
    """no library code: behind a closed gate on stream A the copy of X over Y has not happened -- a read through stream B, which does
    not wait for A, gives Y; after A is drained it gives X.  If the first read gave X, the gate would not gate and no other test
    here would mean anything."""
    rng = np.random.default_rng(5)
    X, Y = rng.normal(size=(200, 32)), rng.normal(size=(200, 32))
    a, b, dev, pin = H.Lane(), H.Lane(), None, None
    try:
        dev, pin = H.DevBuf(Y), H.Pinned(X)
        ev = a.gate()
        a.copy_in(dev, pin)
        assert a.closed(ev)
        first = b.read_through(dev)
        a.synchronize()
        assert not a.closed(ev)
        second = b.read_through(dev)
        assert first.tobytes() == Y.tobytes(), "the gate does not hold back what is queued behind it"
        assert second.tobytes() == X.tobytes()
    finally:
        a.synchronize(); b.synchronize()
        for x in (dev, pin):
            if x is not None:
                x.free()
        a.close(); b.close()


def test_positive_control_of_the_read_back():
    """no library code: the plain hipMemcpy that every test reads its device outputs with, right after the call, neither waits for
    device work queued on a non-blocking stream nor runs behind it.  A device-to-device copy of X over Y -- what a getter with
    LOIKB_OUT_DEVICE ends with -- behind a closed gate: the read gives Y and returns while the gate is closed; after the stream is
    drained it gives X.  (A HOST-to-device copy behind the gate is another matter on this runtime: the transfer engines serve the
    streams in turn, so a plain read queues up behind it -- profiles/stream_measured.md.  That is why stream_harness.Run.get_n also asks
    hipStreamQuery, before it reads, whether the call left anything queued.)"""
    rng = np.random.default_rng(6)
    X, Y = rng.normal(size=(200, 32)), rng.normal(size=(200, 32))
    a, dev, src = H.Lane(), None, None
    try:
        dev, src = H.DevBuf(Y), H.DevBuf(X)
        ev = a.gate()
        a.copy_dev(dev, src)
        assert a.closed(ev)
        first = dev.read()
        still_closed = a.closed(ev)
        a.synchronize()
        second = dev.read()
        assert first.tobytes() == Y.tobytes(), "the plain read waited for the stream: it cannot tell a complete output from a pending one"
        assert still_closed, "the plain read outlasted the gate"
        assert second.tobytes() == X.tobytes()
    finally:
        a.synchronize()
        for x in (dev, src):
            if x is not None:
                x.free()
        a.close()


def test_every_field_host_and_device_out(monkeypatch):
    """get() of every field after a Solve() and again in the middle of pass-level calls (the pass state's own getters, its int
    route among them); the getters rebuilt from the problem also into a host array behind the gate"""
    _clean(monkeypatch)
    model, wl = _talos_batch(200, 91)
    everything = VECTORS + list(capi._SCALAR_FIELDS) + list(capi.INT_FIELDS)

    def sequence(run, s):
        run.do(s.SolveInit, *_init_args(run, wl))
        run.do(s.Solve)
        _snap(run, s, "solve", everything)
        for n in REBUILT:
            run.put("host:" + n, run.do(s.get, n))
        _results(run, s, "solve")
        run.do(s.SolveInit, *_init_args(run, wl))
        for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0, 1, 2, 3, 4, 5, 6, 7, 8):
            run.do(s._pass, k)
        _snap(run, s, "passes", everything)
        _results(run, s, "passes")
        for n in REBUILT:
            run.put("passes host:" + n, run.do(s.get, n))

    make = lambda **kw: loik_amd.BatchedLoik(model, 200, **PRM, **kw)
    ref, gates = H.run_both(make, sequence, what="every field")
    assert gates >= 2 * len(everything)
    _own_stream_too(lambda: make(flags=capi.OPT_OWN_STREAM), sequence, ref, "every field")


@pytest.mark.parametrize("engine", list(ENGINES))
def test_every_engine(engine, monkeypatch):
    env, kw = ENGINES[engine]
    _clean(monkeypatch, env)
    model, wl = _talos_batch(200, 91)
    _, wl2 = _talos_batch(200, 92)
    sequence = _core(wl, wl2, ["z", "nu", "vis", "fis", "yis", "g", "His", "iter", "status", "mu", "primal_residual", "mu_updates"])
    make = lambda **k2: loik_amd.BatchedLoik(model, 200, **PRM, **kw, **k2)
    ref, _ = H.run_both(make, sequence, what=engine)
    assert (ref["solve:iter"] > 1).all()
    _own_stream_too(lambda: make(flags=capi.OPT_OWN_STREAM), sequence, ref, engine)


def test_fp32_handle(monkeypatch):
    _clean(monkeypatch)
    model, wl = _talos_batch(200, 91)
    _, wl2 = _talos_batch(200, 92)
    sequence = _core(wl, wl2, ["z", "nu", "vis", "fis", "yis", "His", "UDinv", "iter", "status", "mu"])
    prm = dict(FIXTURE, max_iter=200, tol_abs=1e-3, tol_rel=0.0)
    H.run_both(lambda: loik_amd.BatchedLoik(model, 200, precision=capi.F32, **prm), sequence, what="fp32")


def test_formulation_edits_and_warm_start(monkeypatch):
    """UpdateReferences, UpdateEqConstraint (both overloads), Add / RemoveEqConstraint, UpdateIneqConstraints with a per-instance
    box on the device, then set_warm_start(True) and a second solve -- each edit behind a gate, a solve and a snapshot after each"""
    _clean(monkeypatch)
    talos = loik_amd.builtin_model("talos32")
    a, b_ = talos.getJointId("arm_left_7_joint"), talos.getJointId("arm_right_7_joint")
    B = 200
    wl = multi_task_batch(talos, B, [a, b_], 31)
    rng = np.random.default_rng(32)
    lb, ub = -0.5 * (1 + 0.2 * rng.random((B, talos.nv))), 0.5 * (1 + 0.2 * rng.random((B, talos.nv)))
    Hl, vl = per_link_references(talos, 7, "full")
    names = ["z", "nu", "yis", "Aty", "g", "iter", "status"]

    def sequence(run, s):
        run.do(s.SolveInit, run.inp(wl["q"]), wl["H_ref"], wl["v_ref"], wl["c_ids"][:1], wl["Ais"][:1], run.inp(wl["bis"][:, :1]), wl["lb"], wl["ub"])
        run.do(s.Solve)
        _snap(run, s, "init {a}", names)
        run.do(s.AddEqConstraint, b_, wl["Ais"][1], run.inp(wl["bis"][:, 1]))
        run.do(s.Solve, None, -1, None, None)
        _snap(run, s, "add b", names)
        run.do(s.UpdateEqConstraint, a, run.inp(0.5 * wl["bis"][:, 0]))
        run.do(s.Solve)
        _snap(run, s, "update a (bi)", names)
        run.do(s.UpdateEqConstraint, a, wl["Ais"][0], run.inp(wl["bis"][:, 0]))
        run.do(s.Solve)
        _snap(run, s, "update a (Ai, bi)", names)
        run.put("removed", run.do(s.RemoveEqConstraint, a))
        run.do(s.Solve, None, -1, None, None)
        _snap(run, s, "remove a", names)
        run.do(s.UpdateIneqConstraints, run.inp(lb), run.inp(ub))
        run.do(s.Solve)
        _snap(run, s, "per-instance box", names)
        run.do(s.UpdateReferences, Hl, vl)
        run.do(s.Solve)
        _snap(run, s, "per-link references", names)
        s.set_warm_start(True)
        run.do(s.Solve, None, b_, wl["Ais"][1], run.inp(wl["bis"][:, 1]))
        _snap(run, s, "warm", names)

    make = lambda **kw: loik_amd.BatchedLoik(talos, B, **dict(PRM, num_eq_c=1, eq_c_capacity=2), **kw)
    ref, _ = H.run_both(make, sequence, what="edits")
    assert ref["removed"]
    _own_stream_too(lambda: make(flags=capi.OPT_OWN_STREAM), sequence, ref, "edits")


def test_logged_solve_and_solver_info(monkeypatch):
    """logging = True: on the flat engine's LOG build, and (LOIKB_FLAT=0) on the pass-by-pass implementation"""
    model, wl = _talos_batch(200, 91)
    prm = dict(FIXTURE, max_iter=40, tol_abs=1e-6, tol_rel=0.0)

    def sequence(run, s):
        run.do(s.SolveInit, *_init_args(run, wl))
        run.do(s.Solve)
        info = run.do(s.solver_info)
        for k, v in info.items():
            run.put("info:" + k, v)
        _snap(run, s, "logged", ["z", "nu", "iter", "status", "mu", "His"])
        run.do(s.Solve, *_init_args(run, wl))
        for k, v in run.do(s.solver_info).items():
            run.put("info full:" + k, v)

    for env in (dict(), dict(LOIKB_FLAT="0")):
        _clean(monkeypatch, env)
        ref, _ = H.run_both(lambda: loik_amd.BatchedLoik(model, 200, logging=True, **prm), sequence, what="logged %s" % env)
        assert ref["info:rows"].max() > 1


def test_three_chunks(monkeypatch):
    """LOIKB_CHUNKS=3: the chunk streams fork from the handle's stream -- here a gated non-blocking one -- and join before the call
    returns"""
    _clean(monkeypatch, dict(LOIKB_CHUNKS="3"))
    model, wl = _talos_batch(384, 93)
    _, wl2 = _talos_batch(384, 94)
    kw = dict(compact_min_instances=128, max_launch_iters=5, tail_max_instances=900)   # (test_pose_parity's chunks3 row)
    sequence0 = _core(wl, wl2, ["z", "nu", "yis", "iter", "status", "mu"])

    def sequence(run, s):
        sequence0(run, s)
        run.put("chunks", s.stats()["chunks"])

    ref, _ = H.run_both(lambda: loik_amd.BatchedLoik(model, 384, **PRM, **kw), sequence, what="three chunks")
    assert ref["chunks"] == 3


@pytest.mark.parametrize("inputs", ["device", "host"])
def test_long_flat_sequence(inputs, monkeypatch, capfd):
    """B = 2113 (test_flat_sequence.py): solve twice on one batch, then the stale-state pair.  The trace says that the gated run's
    plain Solve()s went without the reset pass.  inputs = host: q and b of 2113 instances are too large for the pinned block, so
    both go through the one device staging buffer, one after the other in stream order"""
    _clean(monkeypatch, dict(LOIKB_TRACE="1"))
    B = 2113
    X, Y = workloads.talos_c3(B, seed=11), workloads.talos_c3(B, seed=12)
    prm = dict(X["params"], max_iter=60)

    def sequence(run, s):
        run.do(s.SolveInit, *_init_args(run, X)); run.do(s.Solve)
        _snap(run, s, "X", ["z", "iter", "status"]); _results(run, s, "X")
        run.do(s.Solve)
        run.put("ordered", s.stats()["flat_ordered"])
        _snap(run, s, "X again", ["z", "iter", "status"]); _results(run, s, "X again")
        run.do(s.SolveInit, *_init_args(run, Y)); run.do(s.Solve)
        _snap(run, s, "Y", ["z", "iter", "status"]); _results(run, s, "Y")
        run.do(s.Solve)
        _snap(run, s, "Y again", ["z", "iter", "status"])
        run.put("prepared records", run.do(_blocks, s, B, 1))   # (loikb_debug_flat_prep: a drain, then a plain hipMemcpy)
        if run.gated:
            lines = [l for l in capfd.readouterr().err.splitlines() if "flat engine:" in l]
            assert sum("no reset pass" in l for l in lines) == 4, lines   # (every plain Solve() of the gated run)
        else:
            capfd.readouterr()

    ref, _ = H.run_both(lambda: loik_amd.BatchedLoik(X["model"], B, **prm), sequence, what="B = 2113", host_inputs=inputs == "host")
    assert ref["ordered"] == 1


def test_set_stream_between_any_two_calls(monkeypatch):
    """contract point 3: the handle alternates between two non-blocking streams, moved before every call with a gate queued on
    the stream it leaves"""
    _clean(monkeypatch)
    model, wl = _talos_batch(200, 91)
    _, wl2 = _talos_batch(200, 92)
    link = int(wl["c_ids"][0])

    def sequence(run, s):
        state = [0]

        def hop():
            if run.gated:
                run.lanes[state[0]].gate()
                state[0] ^= 1
                s.set_stream(run.lanes[state[0]].ptr)
                run.on(run.lanes[state[0]])
        hop(); run.do(s.SolveInit, *_init_args(run, wl))
        hop(); run.do(s.Solve)
        hop()
        if run.gated:
            run.lane.gate()   # (a second gate: integrate's kernel, which the call does not wait for, is still behind it when the next call's own gate opens)
        run.do(s.integrate, 0.05)
        hop(); run.do(s.Solve, None, link, wl["Ais"][0], run.inp(wl2["bis"][:, 0]))
        for n in ["z", "nu", "q", "yis", "His", "iter", "status"]:
            hop(); run.get(n, lambda out, n=n: s.get(n, out=out))
        hop(); _results(run, s, "end")

    H.run_both(lambda: loik_amd.BatchedLoik(model, 200, **PRM), sequence, lanes=2, what="alternating streams")


def test_integrate_then_set_stream(monkeypatch):
    """loikb_integrate returns with its kernel queued (the one solver-core call that is not complete on return); loikb_set_stream
    drains the stream it leaves, so a getter on the new stream sees the integrated q"""
    _clean(monkeypatch)
    model, wl = _talos_batch(200, 91)

    def sequence(run, s):
        run.do(s.SolveInit, *_init_args(run, wl))
        run.do(s.Solve)
        run.do(s.integrate, 0.25)
        if run.gated:
            s.set_stream(run.lanes[1].ptr)
            run.gated = False   # (no gate on B: the read is ordered by set_stream alone)
            run.put("q", s.get("q"))
            run.gated = True
        else:
            run.put("q", s.get("q"))

    ref, _ = H.run_both(lambda: loik_amd.BatchedLoik(model, 200, **PRM), sequence, lanes=2, what="integrate, set_stream")
    assert np.abs(ref["q"] - wl["q"]).max() > 1e-3


def test_two_handles_do_not_disturb_each_other(monkeypatch):
    """contract point 4: stream A is gated for a long time; a whole solve on a handle on stream B returns while A's gate is still closed,
    then the gated call on A's handle; both equal their null-stream runs"""
    _clean(monkeypatch)
    model, wla = _talos_batch(200, 91)
    _, wlb = _talos_batch(200, 92)
    make = lambda: loik_amd.BatchedLoik(model, 200, **PRM)

    def seq_for(wl):
        def sequence(run, s):
            run.do(s.Solve, *_init_args(run, wl))
            _snap(run, s, "end", ["z", "nu", "iter", "status"])
        return sequence
    refs = []
    for wl in (wla, wlb):
        s, r = make(), H.Run()
        try:
            seq_for(wl)(r, s)
        finally:
            s.close()
        refs.append(r.rec)
    A, Bl = H.Lane(), H.Lane()
    sa = sb = None
    ra, rb = H.Run(A, like=refs[0]), H.Run()
    try:
        sa, sb = make(), make()
        sa.set_stream(A.ptr); sb.set_stream(Bl.ptr)
        for _ in range(9):
            A.gate()
        ev = A.gate()
        seq_for(wlb)(rb, sb)
        assert A.closed(ev), "the calls on stream B waited for stream A's gate (or outlasted it)"
        seq_for(wla)(ra, sa)
        H.assert_same_records(rb.rec, refs[1], "handle on B")
        H.assert_same_records(ra.rec, refs[0], "handle on A")
    finally:
        A.synchronize(); Bl.synchronize()
        for s in (sa, sb):
            if s is not None:
                s.close()
        ra.close(); rb.close()
        A.close(); Bl.close()
