"""GPU: frame Jacobians, dexterity measures and the dexterous multi-start pick (include/loik_amd_jacobian.h) against the numpy
reference of tests/jacobian_numpy.py (proven on the CPU by test_jacobian_numpy.py), their exact and structural properties, their use
in a solve, the robustness against a NaN row, the selection rule and the validation."""
import ctypes as C

import numpy as np
import pytest

import loik_amd
from loik_amd import capi

from helpers import random_tree
from test_pose_ik import BOUND, PRM, _fk_models, _handle, _links
from test_multistart import ERR_ARG, ERR_STATE, SEED, TOL, _goal_rows, _mk, _pose_fields, _robot
import jacobian_numpy as JN
import pose_limits_numpy as PL
import pose_multistart_numpy as M
import pose_numpy as P
import pose_tasks_numpy as T
import qp_cases as QC
import qp_numpy as QP

pytestmark = pytest.mark.gpu

# batches: not multiples of 64, one across a 256-thread block.  The numpy reference walks (link, ancestor, instance) in Python, so the
# wide batch goes to the two small trees
ROBOTS = [("panda7", 257), ("talos32", 257), ("deep60", 67), ("helical24", 67), ("multidof20", 67), ("composite20", 67), ("fk3", 67),
          ("tree90", 35), ("tree170", 9), ("tree330", 3)]
# generated trees past a wavefront's 64 lanes (name -> seed, joints): k_frame_jacobians strides over the DoFs from nv = 65 on (tree90:
# a second trip), shares a workgroup between two (instance, frame) pairs instead of four from nv = 158 on (tree170) and gives it to one
# from nv = 316 on (tree330).  Root paths of 40, 66 and 154 joints; smaller batches, the reference being a Python loop over them
BIG_TREES = {"tree90": (51, 90), "tree170": (52, 170), "tree330": (53, 330)}
IDS = [r[0] for r in ROBOTS]
REFERENCES = ["local", "local_world_aligned", "world"]
MASKS = [0x3f, 0x07, 0x38, 0x1f]
J_BOUND = 1e-11     # (the 154-joint path of tree330 is 2.4 times the 64 reasoned with here: well inside the two decades of margin) |J - J_ref| <= J_BOUND max(1, max |J_ref|): at most 64 compositions of about 30 flops at u = 1.1e-16
DEX_BOUND = 1e-11   # |sigma^2 - sigma_ref^2| <= DEX_BOUND max(1, sigma_0^2): J_BOUND through 64 rank-1 updates and a backward-stable Jacobi

_CASES = {}


def _case(name):
    """model, batch, q, all links (the universe included), one tool frame per link, and the numpy joint-frame Jacobian: computed once"""
    if name not in _CASES:
        B = dict(ROBOTS)[name]
        model = _fk_models()[3] if name == "fk3" else random_tree(*BIG_TREES[name]) if name in BIG_TREES else QC.model_of(name)
        rng = np.random.default_rng(200 + IDS.index(name))
        q = model.random_configurations(rng, B)
        links = list(range(model.njoints))
        _CASES[name] = dict(model=model, B=B, q=q, links=links, frames=T.random_frames(rng, len(links)), J_joint=QP.jacobians(model, q, links))
    return _CASES[name]


def _open(c, precision=capi.F64):
    s, _ = _handle(c["model"], c["B"], [c["model"].njoints - 1], c["q"], precision=precision)
    return s


# ---- 1. the Jacobian against numpy: all links at once, with and without tool frames, in the three reference frames ----------------
@pytest.mark.parametrize("name", IDS)
def test_frame_jacobians_match_numpy(name):
    c = _case(name)
    model, q, links = c["model"], c["q"], c["links"]
    off = ~(c["J_joint"] != 0.0).any(axis=2)   # [B][n][nv]: the DoF is not on the link's root path (the universe: every DoF)
    assert off[:, 0].all() and not off[:, -1].all()
    s = _open(c)
    worst = 0.0
    for frames in (None, c["frames"]):
        for ref in REFERENCES:
            got = s.frame_jacobians(links, frames, reference=ref)
            want = JN.frame_jacobians(model, q, links, frames, ref, J_joint=c["J_joint"])
            assert got.shape == want.shape == (c["B"], len(links), 6, model.nv)
            err, scale = float(np.max(np.abs(got - want))), max(1.0, float(np.max(np.abs(want))))
            worst = max(worst, err / scale)
            print("jacobian_measured %s frames=%s %s: max |J - J_ref| %.3e, max |J_ref| %.3f" % (name, frames is not None, ref, err, scale))
            assert err <= J_BOUND * scale, (name, ref, err)
            # off-path columns and the universe's matrix are exact zeros
            assert not got[:, 0].any()
            assert not np.any(got[np.broadcast_to(off[:, :, None, :], got.shape)] != 0.0)
            # ... and on-path columns are not (every DoF moves the frame of its own link)
            assert np.array_equal((got != 0.0).any(axis=2), ~off)
    s.close()
    print("jacobian_measured %s worst relative %.3e" % (name, worst))


# ---- 2. exact and structural properties -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["panda7", "multidof20", "deep60", "tree170"])
def test_exact_properties(name):
    c = _case(name)
    model, links, B = c["model"], c["links"], c["B"]
    n = len(links)
    s, s32 = _open(c), _open(c, capi.F32)
    ident = np.tile(T.IDENTITY12, (n, 1))
    hip = capi.DeviceArray.hip()
    for ref in REFERENCES:
        J = s.frame_jacobians(links, c["frames"], reference=ref)
        # frames=None is the identity frame, bit for bit
        assert np.array_equal(s.frame_jacobians(links, None, reference=ref), s.frame_jacobians(links, ident, reference=ref))
        # a device buffer gets what the host path gets
        d = capi.DeviceArray(np.full(J.shape, np.nan))
        assert s.frame_jacobians(links, c["frames"], reference=ref, out=d) is d
        back = np.empty_like(J)
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(d.data_ptr()), back.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        d.free()
        assert np.array_equal(back, J)
        # fp64 from the resident fp64 q whatever the handle's precision
        assert np.array_equal(s32.frame_jacobians(links, c["frames"], reference=ref), J)
    dex = s.frame_dexterity(links, c["frames"], [MASKS[e % 4] for e in range(n)], length=0.25)
    dex32 = s32.frame_dexterity(links, c["frames"], [MASKS[e % 4] for e in range(n)], length=0.25)
    assert all(np.array_equal(dex[k], dex32[k]) for k in dex)
    # the three frames through frame_placements of the same handle: J_lwa = blockdiag(R, R) J_local, J_world = J_lwa + [t]x of its angular rows
    Jl, Ja, Jw = (s.frame_jacobians(links, c["frames"], reference=r) for r in REFERENCES)
    Mf = s.frame_placements(links, c["frames"])
    R, t = Mf[..., :3, :3], Mf[..., :3, 3]
    scale = max(1.0, float(np.max(np.abs(Jw))))
    assert np.max(np.abs(Ja[:, :, :3] - R @ Jl[:, :, :3])) <= 1e-13 * scale and np.max(np.abs(Ja[:, :, 3:] - R @ Jl[:, :, 3:])) <= 1e-13
    assert np.array_equal(Jw[:, :, 3:], Ja[:, :, 3:])
    lever = np.cross(t[:, :, None, :], np.swapaxes(Ja[:, :, 3:], 2, 3)).swapaxes(2, 3)
    assert np.max(np.abs(Jw[:, :, :3] - (Ja[:, :, :3] + lever))) <= 1e-13 * scale
    s.close(); s32.close()


# ---- 3. use in a solve: J_local z is the solver's own link velocity -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["panda7", "talos32"])
def test_jacobian_times_z_is_the_solvers_vis(name):
    """A = I on one link, b = J nu0 of a small nu0 (so the constraint can be met inside the box and the solve converges): on the
    converged instances J_local z is the vis the solver reports for the link, to the solve's tolerance"""
    model = loik_amd.builtin_model(name)
    link = _links(model, 1)[0]
    B = 67
    rng = np.random.default_rng(31)
    q = model.random_configurations(rng, B)
    b = np.einsum("bij,bj->bi", QP.jacobians(model, q, [link])[:, 0], 0.1 * rng.normal(size=(B, model.nv)))
    s = loik_amd.BatchedLoik(model, B, **dict(PRM, num_eq_c=1))
    s.SolveInit(q, np.eye(6), np.zeros(6), np.array([link], dtype=np.int32), np.eye(6)[None], b[:, None, :],
                -BOUND * np.ones(model.nv), BOUND * np.ones(model.nv))
    s.Solve()
    z, vis, conv = s.get("z"), s.get("vis"), s.get("converged") != 0
    J = s.frame_jacobians([link])[:, 0]
    s.close()
    assert conv.sum() >= B // 2 and np.max(np.abs(z)) > 1e-2, conv.mean()   # (a six-row task near a singular posture can run out of iterations)
    diff = np.abs(np.einsum("bij,bj->bi", J, z) - vis[:, link - 1])[conv]
    print("jacobian_measured %s: %d of %d converged, max |J z - vis| %.3e (tol_abs %.1e)" % (name, conv.sum(), B, diff.max(), PRM["tol_abs"]))
    assert diff.max() <= PRM["tol_abs"]


# ---- 4. dexterity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["panda7", "talos32", "deep60", "helical24", "multidof20", "composite20", "fk3", "tree90"])
def test_dexterity_matches_numpy(name):
    c = _case(name)
    model, q, links, B = c["model"], c["q"], c["links"], c["B"]
    n = len(links)
    Jl = JN.frame_jacobians(model, q, links, c["frames"], "local", J_joint=c["J_joint"])
    s = _open(c)
    worst = 0.0
    for length, shift in [(1.0, 0), (0.25, 1), (1.0, 2), (0.25, 3)]:
        rows = [MASKS[(e + shift) % 4] for e in range(n)]
        got = s.frame_dexterity(links, c["frames"], rows, length=length)
        sg = got["sigma"]
        assert sg.shape == (B, n, 6) and got["manipulability"].shape == got["inv_condition"].shape == (B, n)
        assert np.all(np.isfinite(sg)) and np.all(sg >= 0.0) and np.all(np.diff(sg, axis=2) <= 0.0)
        for e in range(n):
            m = bin(rows[e]).count("1")
            assert not sg[:, e, m:].any()
            w = JN.row_weights(rows[e], length)
            for b in range(B):
                sv = np.linalg.svd(w[:, None] * Jl[b, e], compute_uv=False)
                want = np.zeros(6)
                want[:min(m, sv.size)] = sv[:m]
                err = float(np.max(np.abs(sg[b, e] ** 2 - want ** 2))) / max(1.0, want[0] ** 2)
                worst = max(worst, err)
            # manipulability and the inverse condition number are those of the returned sigma
            mp = np.prod(sg[:, e, :m], axis=1)
            assert np.all(np.abs(got["manipulability"][:, e] - mp) <= 1e-14 * mp)
            ic = np.where(sg[:, e, 0] > 0, sg[:, e, m - 1] / np.where(sg[:, e, 0] > 0, sg[:, e, 0], 1.0), 0.0)
            assert np.all(np.abs(got["inv_condition"][:, e] - ic) <= 1e-14 * ic)
    print("dexterity_measured %s: max |sigma^2 - sigma_ref^2| / max(1, sigma_0^2) %.3e" % (name, worst))
    assert worst <= DEX_BOUND, (name, worst)
    if name == "panda7":
        # link 3 has three ancestor DoFs: of the six singular values of the full mask the last three are zero within the bound
        sg = s.frame_dexterity([3], c["frames"][3:4], [0x3f])["sigma"][:, 0]
        assert np.all(np.isfinite(sg)) and np.all(sg >= 0.0) and np.all(sg[:, 0] > 0.1)
        assert np.all(sg[:, 3:] ** 2 <= DEX_BOUND * np.maximum(1.0, sg[:, :1] ** 2))
        dflt = s.frame_dexterity([3, 7])
        assert all(np.array_equal(dflt[k], s.frame_dexterity([3, 7], np.tile(T.IDENTITY12, (2, 1)), [0x3f, 0x3f], length=1.0)[k]) for k in dflt)
    s.close()


def test_dexterity_of_the_handles_tasks():
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 2)
    B = 67
    rng = np.random.default_rng(77)
    q = model.random_configurations(rng, B)
    frames = T.random_frames(rng, 2)
    s, _ = _handle(model, B, links, q)
    none = s.frame_dexterity(length=0.5)
    want = s.frame_dexterity(links, None, [0x3f, 0x3f], length=0.5)
    assert all(np.array_equal(none[k], want[k]) for k in none)
    s.set_pose_tasks(["position", "pose_axis"], frames)
    tasks = s.frame_dexterity(length=0.5)
    want = s.frame_dexterity(links, frames, [0x07, 0x1f], length=0.5)
    assert all(np.array_equal(tasks[k], want[k]) for k in tasks)
    assert not tasks["sigma"][:, 0, 3:].any() and not tasks["sigma"][:, 1, 5:].any() and np.all(tasks["sigma"][:, 1, 4] > 0)
    assert not np.array_equal(tasks["sigma"], none["sigma"])
    s.close()


# ---- 5. a NaN row --------------------------------------------------------------------------------------------------------------------
def test_a_nan_row_ends_as_non_finite_outputs_and_touches_no_other_row():
    model = loik_amd.builtin_model("talos32")
    links = _links(model, 2)
    B, bad = 67, 41
    rng = np.random.default_rng(5)
    q = model.random_configurations(rng, B)
    frames = T.random_frames(rng, model.njoints)
    all_links = list(range(model.njoints))
    rows = [MASKS[e % 4] for e in all_links]
    s, _ = _handle(model, B, links, q)
    tg = P.fk12(model, q, links)
    J0 = s.frame_jacobians(all_links, frames, reference="world")
    D0 = s.frame_dexterity(all_links, frames, rows, length=0.5)
    qn = q.copy()
    qn[bad] = np.nan
    out = s.SolvePose(tg, max_steps=0, q=qn)
    assert out["status"][bad] & capi.POSE_ST_STOPPED and np.isnan(s.get("q")[bad]).all()
    J1 = s.frame_jacobians(all_links, frames, reference="world")
    D1 = s.frame_dexterity(all_links, frames, rows, length=0.5)
    s.close()
    keep = np.arange(B) != bad
    assert not np.isfinite(J1[bad]).all() and np.array_equal(J1[keep], J0[keep])
    assert not J1[bad, 0].any()   # (the universe has no column to be NaN in)
    for k in D0:
        assert np.isnan(D1[k][bad]).all() and np.array_equal(D1[k][keep], D0[k][keep]), k


# ---- 6. the dexterous multi-start pick -----------------------------------------------------------------------------------------------
def _ms_setup(G=8, K=16):
    model, links, lo, hi, valid = _robot("panda7")
    rng = np.random.default_rng(70 + G)
    q0g = _goal_rows("panda7", model, lo, hi, valid, G, seed=71)
    tg = P.fk12(model, rng.uniform(lo, hi, size=(G, model.nq)), links)
    return model, links, lo, hi, q0g, tg, np.repeat(q0g, K, axis=0)


def test_dexterous_pick_is_the_numpy_selection_on_the_devices_own_dexterity():
    G, K, LEN = 8, 16, 0.5
    model, links, lo, hi, q0g, tg, q_init = _ms_setup(G, K)
    kw = dict(seed=SEED, q0=q0g, tol_pose=TOL, max_steps=12)
    a, b = _mk(model, G * K, links, q_init, lo, hi), _mk(model, G * K, links, q_init, lo, hi)
    assert a.multistart_pick_dexterous() is None
    a.set_multistart_pick_dexterous(LEN)
    assert a.multistart_pick_dexterous() == dict(length=LEN)
    out = a.SolvePoseMultiStart(tg, K, pick="first", **kw)
    status, _, err = _pose_fields(a)
    q = a.get("q")
    sig_min = a.frame_dexterity(length=LEN)["sigma"][:, :, 5].min(axis=1)   # (one pose task: m = 6)
    cls, cost = M.instance_keys(status, err, q, q0g, K, M.PICK_FIRST, PL.limit_q_index(model))
    cost[cls == 0] = -sig_min[cls == 0]
    o = M.select_tables(cls, cost, status, K)
    print("multistart_measured dexterous | nreached %s | winners %s | sigma_min of the winners %s" % (o["nreached"].tolist(), o["winner"].tolist(),
                                                                                                      np.round(sig_min[o["winner"]], 4).tolist()))
    assert np.sum(o["nreached"] >= 2) >= 2, o["nreached"]   # (a choice to make)
    assert np.array_equal(out["winner"], o["winner"]) and np.array_equal(out["goal_status"], o["goal_status"])
    assert np.array_equal(out["cost"], o["cost"]) and np.array_equal(out["nreached"], o["nreached"])
    assert np.array_equal(out["q"], q[o["winner"]]) and np.array_equal(out["err"], err[o["winner"]])
    # every winner is at least as far from singular as the first reached seed of its goal, and some are farther
    reached = (status & capi.POSE_ST_REACHED) != 0
    first = np.array([g * K + int(np.argmax(reached[g * K:(g + 1) * K])) for g in range(G)])
    answered = o["goal_status"] == M.GOAL_REACHED
    assert np.all(sig_min[out["winner"]][answered] >= sig_min[first][answered])
    assert np.any(sig_min[out["winner"]][answered] > sig_min[first][answered])
    # pick="dexterous" on a handle without a latch is the latched call (b is as fresh as a was: a handle's warm-started solves depend on
    # what it ran before, so only handles with the same history are compared bit for bit), and it leaves no latch behind
    keys = ("winner", "goal_status", "q", "err", "cost", "nreached", "round")
    two = b.SolvePoseMultiStart(tg, K, pick="dexterous", length=LEN, **kw)
    assert b.multistart_pick_dexterous() is None
    assert all(np.array_equal(two[k], out[k]) for k in keys)
    # ... and on a handle with one, that latch is back in force afterwards
    a.set_multistart_pick_dexterous(2.0)
    x, y = a.SolvePoseMultiStart(tg, K, pick="dexterous", length=LEN, **kw), b.SolvePoseMultiStart(tg, K, pick="dexterous", length=LEN, **kw)
    assert a.multistart_pick_dexterous() == dict(length=2.0) and b.multistart_pick_dexterous() is None
    assert all(np.array_equal(x[k], y[k]) for k in keys)
    # cleared: what a handle that never set it computes, bit for bit (c: never latched, and the same two multi-starts behind it --
    # the pick ranks seeds, it does not touch a solve)
    c = _mk(model, G * K, links, q_init, lo, hi)
    for _ in range(2):
        c.SolvePoseMultiStart(tg, K, pick="first", **kw)
    assert c.multistart_pick_dexterous() is None
    a.clear_multistart_pick_dexterous()
    assert a.multistart_pick_dexterous() is None
    for pick in ("first", "nearest"):
        x, y = a.SolvePoseMultiStart(tg, K, pick=pick, **kw), c.SolvePoseMultiStart(tg, K, pick=pick, **kw)
        assert all(np.array_equal(x[k], y[k]) for k in keys), pick
        assert np.array_equal(a.get("q"), c.get("q"))
        if pick == "first":
            assert not x["cost"][x["goal_status"] == M.GOAL_REACHED].any()
    with pytest.raises(capi.LoikError):   # pick = 2 is still refused by the library: the latch is the only way in
        b.SolvePoseMultiStart(tg, K, pick=2, **kw)
    a.close(); b.close(); c.close()


# ---- 7. validation ---------------------------------------------------------------------------------------------------------------------
def test_validation_refuses_and_changes_nothing():
    model = loik_amd.builtin_model("panda7")
    links = _links(model, 1)
    B = 5
    q = model.random_configurations(np.random.default_rng(3), B)
    s, _ = _handle(model, B, links, q)
    L, h = s.L, s.h
    nv, nj = model.nv, model.njoints
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    ok_links = np.array([7, 3], dtype=np.int32)
    lp = ok_links.ctypes.data_as(ip)
    outJ, outD = np.full((B, 2, 6, nv), 7.0), np.full((B, 2, 8), 7.0)
    oj, od = outJ.ctypes.data_as(C.c_void_p), outD.ctypes.data_as(C.c_void_p)
    prm = capi.DexterityParams(1.0, 0)
    q_before, plan_before = s.get("q"), s.plan()

    def refused(rc, want):
        assert rc == want, (rc, want)
        assert np.array_equal(s.get("q"), q_before) and s.plan() == plan_before
        assert np.all(outJ == 7.0) and np.all(outD == 7.0)

    def frames_with(bad):
        f = np.tile(T.IDENTITY12, (2, 1))
        f[1] = bad
        return f

    skewed, nan_t = T.IDENTITY12.copy(), T.IDENTITY12.copy()
    skewed[1] = 1e-6
    nan_t[10] = np.nan
    mirror = np.r_[np.diag([1.0, 1.0, -1.0]).ravel(), np.zeros(3)]
    # loikb_frame_jacobians
    refused(L.loikb_frame_jacobians(None, lp, None, 2, 0, oj, 0), ERR_ARG)
    refused(L.loikb_frame_jacobians(h, lp, None, 2, 0, None, 0), ERR_ARG)
    refused(L.loikb_frame_jacobians(h, lp, None, -1, 0, oj, 0), ERR_ARG)
    refused(L.loikb_frame_jacobians(h, None, None, 2, 0, oj, 0), ERR_ARG)
    for bad_link in (-1, nj):
        bl = np.array([7, bad_link], dtype=np.int32)
        refused(L.loikb_frame_jacobians(h, bl.ctypes.data_as(ip), None, 2, 0, oj, 0), ERR_ARG)
        refused(L.loikb_frame_dexterity(h, bl.ctypes.data_as(ip), None, None, 2, C.byref(prm), od, 0), ERR_ARG)
    for bad_frame in (skewed, nan_t, mirror):
        f = frames_with(bad_frame)
        refused(L.loikb_frame_jacobians(h, lp, f.ctypes.data_as(dp), 2, 0, oj, 0), ERR_ARG)
        refused(L.loikb_frame_dexterity(h, lp, f.ctypes.data_as(dp), None, 2, C.byref(prm), od, 0), ERR_ARG)
    for ref in (-1, 3):
        refused(L.loikb_frame_jacobians(h, lp, None, 2, ref, oj, 0), ERR_ARG)
    # loikb_frame_dexterity
    refused(L.loikb_frame_dexterity(None, lp, None, None, 2, C.byref(prm), od, 0), ERR_ARG)
    refused(L.loikb_frame_dexterity(h, lp, None, None, 2, C.byref(prm), None, 0), ERR_ARG)
    refused(L.loikb_frame_dexterity(h, lp, None, None, -1, C.byref(prm), od, 0), ERR_ARG)
    refused(L.loikb_frame_dexterity(h, lp, None, None, 2, None, od, 0), ERR_ARG)
    for bad_rows in (0, 0x40, -1):
        r = np.array([0x3f, bad_rows], dtype=np.int32)
        refused(L.loikb_frame_dexterity(h, lp, None, r.ctypes.data_as(ip), 2, C.byref(prm), od, 0), ERR_ARG)
    for bad_prm in (capi.DexterityParams(0.0, 0), capi.DexterityParams(-1.0, 0), capi.DexterityParams(np.nan, 0), capi.DexterityParams(np.inf, 0),
                    capi.DexterityParams(1.0, 1)):
        refused(L.loikb_frame_dexterity(h, lp, None, None, 2, C.byref(bad_prm), od, 0), ERR_ARG)
        # ... and the latch takes none of them and keeps what it holds
        s.set_multistart_pick_dexterous(0.75)
        refused(L.loikb_dexterity_set_multistart_pick(h, C.byref(bad_prm)), ERR_ARG)
        assert s.multistart_pick_dexterous() == dict(length=0.75)
        s.clear_multistart_pick_dexterous()
        refused(L.loikb_dexterity_set_multistart_pick(h, C.byref(bad_prm)), ERR_ARG)
        assert s.multistart_pick_dexterous() is None
    refused(L.loikb_frame_dexterity(h, None, None, None, 2, C.byref(prm), od, 0), ERR_ARG)   # links == NULL: n must be nc_active = 1
    refused(L.loikb_dexterity_set_multistart_pick(None, C.byref(prm)), ERR_ARG)
    assert L.loikb_dexterity_get_multistart_pick(None, None) == 0 and L.loikb_dexterity_get_multistart_pick(h, None) == 0
    # n == 0 is fine and writes nothing
    refused(L.loikb_frame_jacobians(h, lp, None, 0, 0, oj, 0), 0)
    refused(L.loikb_frame_dexterity(h, lp, None, None, 0, C.byref(prm), od, 0), 0)
    # what is accepted afterwards is what a fresh handle gives: the refusals left nothing behind
    t, _ = _handle(model, B, links, q)
    assert np.array_equal(s.frame_jacobians(ok_links), t.frame_jacobians(ok_links))
    s.close(); t.close()
    # no configurations resident yet, and links == NULL before SolveInit
    u = loik_amd.BatchedLoik(model, B, **dict(PRM, num_eq_c=1))
    assert u.L.loikb_frame_jacobians(u.h, lp, None, 2, 0, oj, 0) == ERR_STATE
    assert u.L.loikb_frame_dexterity(u.h, lp, None, None, 2, C.byref(prm), od, 0) == ERR_STATE
    assert u.L.loikb_frame_dexterity(u.h, None, None, None, 1, C.byref(prm), od, 0) == ERR_STATE
    assert np.all(outJ == 7.0) and np.all(outD == 7.0)
    u.close()
