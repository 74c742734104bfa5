"""The flat engine's long launch sequence (batches above the short sequence's 2048 instances; loik_host.hip: virtual_reset_route,
launch_flat).  By default a plain Solve() that takes every instance from a record k_fslots prepares launches no k_reset -- k_fslots
writes what the reset would have written into the record as constants (MODE_VIRTUAL_RESET) --, one kernel sets up list, ring and
counters (k_queue_init), and one pass over the scalar records behind the engine delivers the unfinished list, the counts, the order's
bins and the end decades (k_finish_order).  LOIKB_FLAT_SEQ=0 is the sequence as it was: k_reset, k_list_iota, a memset, k_ring_fill,
..., k_list_unfinished, a memset, k_order_count.

Every case runs on two fresh handles, switch on and off, and compares byte for byte: get_results(RESULT_FIELDS) (the 30 logged
scalars among them: the engine stores those only for an instance that iterated), the iteration counts, the converged and infeasible
flags and stats()["instance_iterations"], after every solve of the case.  The launches' trace lines (LOIKB_TRACE=1) say whether a
launch went without the reset pass: the cases that must, do, and the routes that must keep the real reset never do.

Shapes: 2113 = 33 tiles + 1 instance (the last tile is partial, the list is longer than 2048), or 300 instances on handles created
under LOIKB_FLAT_SMALL_BATCH=0."""
import ctypes

import numpy as np
import pytest

import flat_census as C
import helpers
import loik_amd
from loik_amd import capi, workloads

pytestmark = pytest.mark.gpu

B = 2113
SWITCHES = C.ENV_NAMES + ("LOIKB_FLAT_PREP", "LOIKB_FLAT_ZERO_STATE", "LOIKB_FLAT_SEQ", "LOIKB_TRACE")
_WL = {}


def _talos(seed, batch=B):
    if (seed, batch) not in _WL:
        _WL[seed, batch] = workloads.talos_c3(batch, seed=seed)
    return _WL[seed, batch]


def _args(wl):
    return (wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])


def _snap(s):
    d = {k: np.asarray(v).tobytes() for k, v in s.get_results(s.RESULT_FIELDS).items()}
    for k in ("iter", "converged", "primal_infeasible"):
        d[k] = np.asarray(s.get(k)).tobytes()
    d["instance_iterations"] = int(s.stats()["instance_iterations"])
    return d


def _both(monkeypatch, capfd, make, run, virtual, env=()):
    """`run(handle)` -> a list of snapshots, on a fresh handle under LOIKB_FLAT_SEQ=1 and =0: equal snapshots; `virtual` launches of
    the first (a count, or a list that says it launch by launch) went without the reset pass, none of the second.  Returns what run
    returned besides (its second value), per switch."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(env).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("LOIKB_TRACE", "1")
    snaps, extra = {}, {}
    for seq in ("1", "0"):
        monkeypatch.setenv("LOIKB_FLAT_SEQ", seq)
        s = make()
        capfd.readouterr()
        snaps[seq], extra[seq] = run(s)
        lines = [l for l in capfd.readouterr().err.splitlines() if "flat engine:" in l]
        s.close()
        went = ["no reset pass" in l for l in lines]
        if isinstance(virtual, list):   # (launch by launch)
            assert went == (virtual if seq == "1" else [False] * len(virtual)), (seq, went)
        else:
            assert sum(went) == (virtual if seq == "1" else 0), (seq, went)
    assert len(snaps["1"]) == len(snaps["0"]) > 0
    for k, (a, b) in enumerate(zip(snaps["1"], snaps["0"])):
        assert set(a) == set(b)
        for f in a:
            assert a[f] == b[f], "solve %d of the case: %s differs between LOIKB_FLAT_SEQ=1 and =0" % (k, f)
    return extra


def _talos_handle(**kw):
    wl = _talos(11)
    prm = dict(wl["params"])
    prm.update(kw)
    return lambda: loik_amd.BatchedLoik(wl["model"], B, **prm)


def test_stale_state(monkeypatch, capfd):
    """batch X stopped at max_iter = 60 leaves converged, flagged and cut-off instances in the tiles -- duals, iteration counts, status
    bits, logged scalars, mu in other decades --, then SolveInit(Y) and Solve(): nothing of X may reach Y's solve through the records"""
    X, Y = _talos(11), _talos(12)

    def run(s):
        out = []
        s.SolveInit(*_args(X)); s.Solve()
        conv, inf = s.get("converged").astype(bool), s.get("primal_infeasible").astype(bool)
        assert conv.any() and inf.any() and (~conv & ~inf).any(), (conv.sum(), inf.sum())
        out.append(_snap(s))
        s.SolveInit(*_args(Y)); s.Solve()
        out.append(_snap(s))
        return out, None

    _both(monkeypatch, capfd, _talos_handle(max_iter=60), run, virtual=2)


def test_solve_twice_on_one_batch(monkeypatch, capfd):
    """the second Solve() takes the order the first left (k_queue_init fills list and ring from it) and keeps nu (ResetRecursion)"""
    X = _talos(11)

    def run(s):
        out = []
        s.SolveInit(*_args(X)); s.Solve()
        out.append(_snap(s))
        s.Solve()
        assert s.stats()["flat_ordered"] == 1
        out.append(_snap(s))
        return out, None

    _both(monkeypatch, capfd, _talos_handle(), run, virtual=2)


def test_three_solves_with_getters_between(monkeypatch, capfd):
    """the getters that rebuild members (UDinv, His, pis) write the records' tag and status between the solves"""
    X = _talos(13)

    def run(s):
        out = []
        s.SolveInit(*_args(X))
        for _ in range(3):
            s.Solve()
            out.append(_snap(s))
            for name in ("UDinv", "His", "pis", "Aty", "g"):
                s.get(name)
        return out, None

    _both(monkeypatch, capfd, _talos_handle(max_iter=200), run, virtual=3)


def test_tailored_solve_after_a_plain_one(monkeypatch, capfd):
    """Solve(q, c, A, b) has its own reset flavour and keeps the real pass; the plain Solve() after it goes without again"""
    X = _talos(11)
    link = int(X["c_ids"][0])
    rng = np.random.default_rng(5)
    q2 = X["q"] + 0.01 * rng.normal(size=X["q"].shape)
    A2 = np.asarray(X["Ais"]) + 0.01 * rng.normal(size=(1, 6, 6))
    b2 = 0.8 * X["bis"][:, 0]

    def run(s):
        out = []
        s.SolveInit(*_args(X)); s.Solve()
        out.append(_snap(s))
        s.Solve(q2, link, A2, b2)
        out.append(_snap(s))
        s.Solve()
        out.append(_snap(s))
        return out, None

    _both(monkeypatch, capfd, _talos_handle(max_iter=200), run, virtual=2)


@pytest.mark.parametrize("route", ["logging", "osqp", "talos44", "fp32", "max_launch_iters", "max_iter_1"])
def test_routes_that_keep_the_real_reset(route, monkeypatch, capfd):
    """SolverInfo lists, OSQP's rule (no prepared records), a 44-joint robot (k_flat1), an fp32 handle, a caller-fixed launch length
    (the streaming engine) and max_iter = 1 (no instance iterates, so the engine's store leaves the logged scalars alone): stale
    state, SolveInit, Solve() as in test_stale_state, and no launch without the reset pass"""
    if route == "talos44":
        X, Y = workloads.talos_wholebody(B, seed=21), workloads.talos_wholebody(B, seed=22)
    else:
        X, Y = _talos(11), _talos(12)
    kw = dict(logging=dict(logging=True), osqp=dict(mu_update_strat=1), talos44={}, fp32=dict(precision=capi.F32),
              max_launch_iters=dict(max_launch_iters=8), max_iter_1={})[route]
    prm = dict(X["params"], max_iter=60)
    prm.update(kw)

    def run(s):
        s.SolveInit(*_args(X)); s.Solve()
        s.SolveInit(*_args(Y))
        if route == "max_iter_1":
            s.set_max_iter(1)
        s.Solve()
        return [_snap(s)], None

    # (max_iter_1: the case's first solve, under max_iter = 60, is an ordinary one and goes without; the second must not)
    _both(monkeypatch, capfd, lambda: loik_amd.BatchedLoik(X["model"], B, **prm), run, virtual=[True, False] if route == "max_iter_1" else 0)


def _leaves(model, n):
    parents = set(int(p) for p in model.parents[1:])
    return [i for i in range(1, model.njoints) if i not in parents][:n]


def _blocks(s, n, nc):
    """the first n prepared records of the handle's last flat launch, the entries k_fslots writes (the scalar row has 17 of 32)"""
    L = capi.lib()
    L.loikb_debug_flat_prep.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.loikb_debug_flat_prep.restype = ctypes.c_int
    stride = 12 * 32 + 4 * 32 + 3 * 64 + 32 + nc * 164   # (flat_prep_stride: PR_C + nc * C2D)
    out = np.empty((n, stride), dtype=np.float64)
    got = ctypes.c_int(0)
    assert L.loikb_debug_flat_prep(s.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n, ctypes.byref(got)) == 0
    assert got.value == stride
    pr_sc = 12 * 32 + 4 * 32 + 3 * 64
    keep = np.ones(stride, bool)
    keep[pr_sc + 17:pr_sc + 32] = False
    return np.ascontiguousarray(out[:, keep])


@pytest.mark.parametrize("nc", [1, 3])
def test_prepared_blocks(nc, monkeypatch, capfd):
    """the records k_fslots writes under the virtual reset are, byte for byte, the ones it writes after the real one -- over stale
    state, with A per instance (the constraint blocks take A, b from the tiles and y, A^T y as zeros).  One constraint: 2113
    instances; three: 300 instances beyond a short sequence of 0"""
    model = loik_amd.builtin_model("talos32")
    n = B if nc == 1 else 300
    X = helpers.multi_task_batch(model, n, _leaves(model, nc), 31 + nc, nu_scale=0.3, per_instance_A=True)
    Y = helpers.multi_task_batch(model, n, _leaves(model, nc), 41 + nc, nu_scale=0.3, per_instance_A=True)
    prm = C.params(dict(num_eq_c=nc), False, max_iter=60, tol_abs=1e-6, tol_rel=0.0)

    def run(s):
        s.SolveInit(*_args(X)); s.Solve()
        s.SolveInit(*_args(Y)); s.Solve()
        return [_snap(s)], _blocks(s, n, nc)

    blocks = _both(monkeypatch, capfd, lambda: loik_amd.BatchedLoik(model, n, **prm), run, virtual=2,
                   env=dict(LOIKB_FLAT_SMALL_BATCH="0") if nc == 3 else ())
    assert blocks["1"].shape == blocks["0"].shape and blocks["1"].tobytes() == blocks["0"].tobytes()
    # (the scalar row as the reset leaves it: mu = mu0, decade, iteration, status, tail iterations, flips = 0)
    pr_sc = 12 * 32 + 4 * 32 + 3 * 64
    assert np.all(blocks["1"][:, pr_sc + 11] == prm["mu"]) and not blocks["1"][:, pr_sc + 12:pr_sc + 17].any()
