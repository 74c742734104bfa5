"""The collision-aware multi-start of include/loik_amd_collision.h: panda7, G = 4 goals, K = 16 seeds, B = 64.

The scene is built from the unlatched run: a world sphere of radius 0.03 at the centre of the elbow sphere (link 4, mid-chain, where
the reached seeds of a goal do not coincide as they do at the tool) of the unlatched winner of goal 0, which then collides by
construction.  The GPU tests ASSERT their precondition on the device's own q with the numpy reference: goal 0 keeps at least one reached
seed with clr >= margin and its unlatched winner is class 0c.  The target seed TSEED was chosen so that this holds, and it was checked
on the CPU first with tests/pose_multistart_numpy.py (the oracle's loop): there goal 0 has 7 reached seeds of which 5 stay clear, and goal
1 has 9, all of them inside the second scene's sphere.  test_the_scene_on_the_oracle below repeats that check without a GPU."""
import numpy as np
import pytest

from loik_amd import capi

from test_pose_ik import BOUND as VBOUND, PRM
import clearance_numpy as CN
import pose_limits_numpy as PL
import pose_multistart_numpy as M
import pose_numpy as P

G, K, B = 4, 16, 64
STEPS, TOL, SEED, TSEED = 12, 1e-4, 7, 102
MARGIN = 0.01
ELBOW = 3            # the sphere on link 4 (one sphere per link, links 1..7)
BOUND = 1e-13        # of test_clearance.py


def _workload():
    import loik_amd
    from test_pose_ik import _links
    model = loik_amd.builtin_model("panda7")
    lo, hi = np.array(model.q_lo, dtype=float), np.array(model.q_hi, dtype=float)
    links = _links(model, 1)
    tg = P.fk12(model, np.random.default_rng(TSEED).uniform(lo, hi, size=(G, model.nq)), links)
    q0g = np.tile(0.5 * (lo + hi), (G, 1))
    lk, sph = CN.make_spheres(model, 1, 600)
    return dict(model=model, lo=lo, hi=hi, links=links, tg=tg, q0g=q0g, lk=lk, sph=sph)


def _scene_elbow(w, q, winner0):
    """the world of the first scene: one sphere at the elbow sphere's centre of instance winner0"""
    c = CN.centres(w["model"], q[winner0:winner0 + 1], w["lk"], w["sph"])[0, ELBOW]
    return np.array([[c[0], c[1], c[2], 0.03]])


def _scene_engulf(w):
    """the world of the second scene: a sphere of radius 0.2 about the tool target of goal 1 -- every seed that reaches goal 1 is in it"""
    return np.array([[*w["tg"][1, 0, 9:12], 0.2]])


def _reached(status):
    status = np.asarray(status)
    return ((status & M.POSE_REACHED) != 0) & ((status & M.POSE_STOPPED) == 0)


def test_the_scene_on_the_oracle():
    """CPU: the precondition of the GPU tests on the oracle's loop"""
    from test_pose_ik import BOUND as box
    w = _workload()
    model = w["model"]
    o = M.multistart_loop(model, PRM, w["q0g"], K, 1, SEED, w["lo"], w["hi"], w["links"], np.tile(np.eye(6), (1, 1, 1)),
                          -box * np.ones(model.nv), box * np.ones(model.nv), w["tg"], 1.0, 1.0, TOL, STEPS, w["lo"], w["hi"])
    q, status = o["q"], o["status"]
    sel = M.select(status, o["err"], q, w["q0g"], K, M.PICK_FIRST, PL.limit_q_index(model))
    ok = _reached(status)
    clr = CN.clearance(model, q, w["lk"], w["sph"], _scene_elbow(w, q, sel["winner"][0]))["min"]
    assert sel["goal_status"][0] == 1 and clr[sel["winner"][0]] < MARGIN
    assert int((ok[:K] & (clr[:K] >= MARGIN)).sum()) >= 3
    clr2 = CN.clearance(model, q, w["lk"], w["sph"], _scene_engulf(w))["min"]
    assert ok[K:2 * K].sum() >= 3 and np.all(clr2[K:2 * K][ok[K:2 * K]] < MARGIN)
    assert all((ok[g * K:(g + 1) * K] & (clr2[g * K:(g + 1) * K] >= MARGIN)).any() for g in (0, 2, 3))


def _open(w):
    from test_multistart import _mk
    s = _mk(w["model"], B, w["links"], np.repeat(w["q0g"], K, axis=0), w["lo"], w["hi"])
    s.set_collision_spheres(w["lk"], w["sph"])
    return s


def _run(s, w, **kw):
    return s.SolvePoseMultiStart(w["tg"], K, seed=SEED, q0=w["q0g"], tol_pose=TOL, max_steps=STEPS, **kw)


def _device_state(s):
    from test_multistart import _pose_fields
    status, _, err = _pose_fields(s)
    return status, err, s.get("q")


def _numpy_selection(w, status, err, q, world, pick=M.PICK_FIRST, cost_in=None):
    """the latched selection on the device's statuses, q and errors and the ORACLE's clearances"""
    model = w["model"]
    ref = CN.clearance(model, q, w["lk"], w["sph"], world)
    cls, cost = M.instance_keys(status, err, q, w["q0g"], K, pick, PL.limit_q_index(model))
    if cost_in is not None:
        cost = np.where(np.asarray(cls) == 0, cost_in, cost)
    cls, cost = CN.ms_keys(cls, cost, status, ref["min"], MARGIN)
    return CN.ms_select(cls, cost, K), cls, ref


def _check_against_numpy(w, s, out, world, what, **kw):
    status, err, q = _device_state(s)
    o, cls, ref = _numpy_selection(w, status, err, q, world, **kw)
    scale = 1.0 + float(np.abs(ref["centres"]).max()) + float(w["sph"][:, 3].max())
    inst = s.multistart_clearance_get("instance")
    print("clearance_ms_measured %s: goal_status %s nclear %s, max |clr - oracle| %.3e" % (what, o["goal_status"].tolist(), o["nclear"].tolist(),
                                                                                            np.abs(inst - ref["min"]).max()))
    assert np.max(np.abs(inst - ref["min"])) <= BOUND * scale
    assert np.array_equal(out["winner"], o["winner"]) and np.array_equal(out["goal_status"], o["goal_status"]), what
    assert np.array_equal(out["nclear"], o["nclear"]) and np.array_equal(out["nreached"], (status.reshape(G, K) & M.POSE_REACHED != 0).sum(axis=1)), what
    assert np.array_equal(out["clearance"], inst[out["winner"]])
    assert np.array_equal(out["q"], q[out["winner"]]) and np.array_equal(out["err"], err[out["winner"]])
    for g in range(G):
        b = int(out["winner"][g])
        assert abs(CN.witness_value(ref["table"], b, out["witness"][g]) - ref["min"][b]) <= BOUND * scale, (what, g)
    return o, cls, ref, (status, err, q)


@pytest.mark.gpu
def test_one_round_picks_a_clear_seed():
    w = _workload()
    s = _open(w)
    plain = _run(s, w, pick="first")
    assert "clearance" not in plain and plain["goal_status"][0] == capi.MS_GOAL_REACHED
    status, err, q = _device_state(s)
    world = _scene_elbow(w, q, int(plain["winner"][0]))
    s.set_collision_world(world)
    # the precondition, on the device's own q with the numpy reference
    ref = CN.clearance(w["model"], q, w["lk"], w["sph"], world)
    ok = _reached(status)
    assert ref["min"][plain["winner"][0]] < MARGIN and int((ok[:K] & (ref["min"][:K] >= MARGIN)).sum()) >= 1
    out = _run(s, w, pick="first", clearance_margin=MARGIN)
    assert s.multistart_clearance() is None                      # (set for the call alone)
    s.set_multistart_clearance(MARGIN)
    out = _run(s, w, pick="first")
    assert out["rounds_run"] == 1
    o, cls, ref, _ = _check_against_numpy(w, s, out, world, "elbow scene, first")
    # goal 0: another winner than without the latch, and a clear one
    b = int(out["winner"][0])
    assert b != plain["winner"][0] and out["goal_status"][0] == capi.MS_GOAL_REACHED and out["clearance"][0] >= MARGIN and cls[b] == 0
    assert cls[plain["winner"][0]] == 0.5
    # the nearest-seed cost within class 0
    out = _run(s, w, pick="nearest")
    _check_against_numpy(w, s, out, world, "elbow scene, nearest", pick=M.PICK_NEAREST)
    s.close()


@pytest.mark.gpu
def test_a_goal_with_only_colliding_answers():
    w = _workload()
    s = _open(w)
    world = _scene_engulf(w)
    s.set_collision_world(world)
    s.set_multistart_clearance(MARGIN)
    out = _run(s, w, pick="first")
    o, cls, ref, (status, err, q) = _check_against_numpy(w, s, out, world, "engulfed goal 1")
    ok = _reached(status)
    assert ok[K:2 * K].sum() >= 2 and np.all(ref["min"][K:2 * K][ok[K:2 * K]] < MARGIN)        # the precondition
    assert out["goal_status"][1] == capi.MS_GOAL_IN_COLLISION == 8 and out["nclear"][1] == 0 and out["nreached"][1] == ok[K:2 * K].sum()
    # ... with the least-penetrating reached seed
    cand = K + np.flatnonzero(ok[K:2 * K])
    assert out["winner"][1] == cand[np.argmax(ref["min"][cand])] and out["cost"][1] == -out["clearance"][1] > 0
    assert all(out["goal_status"][g] == capi.MS_GOAL_REACHED for g in (0, 2, 3))
    # the public pose status is not edited: the colliding seeds still read REACHED
    assert np.all(s.multistart_get("round") == 0)
    s.close()


@pytest.mark.gpu
def test_a_second_round_draws_the_colliding_seeds_anew():
    w = _workload()
    world = _scene_engulf(w)
    a, b = _open(w), _open(w)
    for s in (a, b):
        s.set_collision_world(world)
        s.set_multistart_clearance(MARGIN)
    _run(a, w, pick="first", rounds=1)
    status0, _, q0 = _device_state(a)
    clr0 = a.multistart_clearance_get("instance")
    ok0 = _reached(status0)
    class0, class0c = ok0 & (clr0 >= MARGIN), ok0 & ~(clr0 >= MARGIN)
    assert class0.sum() >= 3 and class0c.sum() >= 2
    out = _run(b, w, pick="first", rounds=2)
    assert out["rounds_run"] == 2                                 # goal 1 had only colliding answers: the restart ran
    status1, _, q1 = _device_state(b)
    assert np.all(out["round"][class0c] == 1) and np.all(out["round"][~ok0] == 1)
    assert np.all(out["round"][class0] == 0) and np.array_equal(q1[class0], q0[class0])
    assert np.all(np.any(q1[class0c] != q0[class0c], axis=1))
    # the new seeds are those of the numpy re-sampler given the loop-private status word
    fresh, moved = M.resample(w["model"], q0, CN.ms_loop_status(status0, clr0, MARGIN), w["q0g"], K, SEED, 1, w["lo"], w["hi"])
    assert np.array_equal(moved, ~class0)
    a.close(); b.close()


@pytest.mark.gpu
def test_with_both_latches_class_0_costs_the_dexterity():
    w = _workload()
    s = _open(w)
    plain = _run(s, w, pick="first")
    _, _, q = _device_state(s)
    world = _scene_elbow(w, q, int(plain["winner"][0]))
    s.set_collision_world(world)
    s.set_multistart_clearance(MARGIN)
    out = _run(s, w, pick="dexterous", length=0.5)
    dex = s.frame_dexterity(length=0.5)                            # (of the resident q the solve left)
    cost_in = -dex["sigma"][:, :, 5].min(axis=1)
    o, cls, ref, _ = _check_against_numpy(w, s, out, world, "both latches", cost_in=cost_in)
    won = out["goal_status"] == capi.MS_GOAL_REACHED
    assert won[0] and np.array_equal(out["cost"][won], cost_in[out["winner"][won]])
    assert cls[out["winner"][0]] == 0 and out["winner"][0] != plain["winner"][0]
    s.close()


@pytest.mark.gpu
def test_a_cleared_latch_is_a_handle_that_never_had_it():
    w = _workload()
    a, b = _open(w), _open(w)
    a.set_collision_world(_scene_engulf(w))
    a.set_multistart_clearance(MARGIN)
    # the same solve behind both handles (the handles warm-start): one round, in which the latch ranks seeds and touches no solve
    la, lb = _run(a, w, rounds=1), _run(b, w, rounds=1)
    assert "clearance" in la and "clearance" not in lb and np.array_equal(a.get("q"), b.get("q"))
    assert la["goal_status"][1] == capi.MS_GOAL_IN_COLLISION and lb["goal_status"][1] == capi.MS_GOAL_REACHED
    a.clear_multistart_clearance()
    assert a.multistart_clearance() is None
    ra, rb = _run(a, w, rounds=2), _run(b, w, rounds=2)
    assert "clearance" not in ra and np.array_equal(a.get("q"), b.get("q"))
    assert all(np.array_equal(ra[k], rb[k]) for k in ("winner", "goal_status", "q", "err", "cost", "nreached", "round"))
    with pytest.raises(capi.LoikError) as e:
        a.multistart_clearance_get("clearance")
    assert e.value.code == -24
    a.close(); b.close()
