"""CPU: the numpy reference of include/loik_amd_motion.h (tests/motion_numpy.py) from first principles, before it referees the device --
difference inverts integrate, the motion bound dominates the true path length of every sphere centre for every joint type of the
header's table, the advancement's FREE / BLOCKED certificates hold under dense sampling, a thin box between clear samples is found, and
the segments the GPU tests use keep the reference's own decisions clear of their thresholds."""
import numpy as np
import pytest

from test_pose_ik import _fk_models
import clearance_numpy as CN
import motion_numpy as MN
import pose_numpy as P
import qp_cases as QC

ROBOTS = ["panda7", "talos32", "multidof13", "helical24", "composite20", "multidof20"]


def _model(name):
    return _fk_models()[3] if name == "multidof13" else QC.model_of(name)


def _segments(model, n, seed, size):
    """qa [n][nq] random, dv [n][nv] of norm `size` * sqrt(nv) at most per DoF scale (rotations stay under pi for size <= 1)"""
    rng = np.random.default_rng(seed)
    qa = model.random_configurations(rng, n)
    dv = size * rng.uniform(-1.0, 1.0, size=(n, model.nv))
    return qa, dv


# ---- 1. difference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROBOTS)
def test_difference_inverts_integrate(name):
    model = _model(name)
    rng = np.random.default_rng(700 + ROBOTS.index(name))
    n = 12
    q0, q1 = model.random_configurations(rng, n), model.random_configurations(rng, n)
    v = MN.difference(model, q0, q1)
    links = list(range(model.njoints))
    back = np.stack([P.integrate(model, q0[i], v[i]) for i in range(n)])
    assert np.max(np.abs(P.fk12(model, back, links) - P.fk12(model, q1, links))) <= 1e-12
    # ... and integrate inverts difference for rotations under pi
    qa, dv = _segments(model, n, 710 + ROBOTS.index(name), 1.0)
    qb = np.stack([P.integrate(model, qa[i], dv[i]) for i in range(n)])
    assert np.max(np.abs(MN.difference(model, qa, qb) - dv)) <= 1e-12
    # a row that is not finite is NaN alone
    q0[3, model.nq - 1] = np.nan
    vb = MN.difference(model, q0, q1)
    keep = np.arange(n) != 3
    assert np.isnan(vb[3]).all() and np.array_equal(vb[keep], v[keep])


# ---- 2. the bound dominates -------------------------------------------------------------------------------------------------------------
def test_every_joint_type_of_the_table_occurs():
    seen, universal = set(), False
    for name in ROBOTS:
        model = _model(name)
        ch, _ = MN.chain_of(model)
        seen |= {int(t) for t in ch.jtype[1:]}
        for i in range(1, model.njoints):
            if int(model.jtype[i]) == P.J_COMPOSITE:
                universal |= [int(st) for st, _, _ in model.composite[i]] == [P.J_RU, P.J_RU]
    for group in (MN._REV[:4], MN._RUB, MN._PRI, MN._HEL, (P.J_TRANSLATION,), (P.J_SPHERICAL,), (P.J_SPHERICAL_ZYX,), (P.J_FREEFLYER,), (P.J_PLANAR,)):
        assert seen & set(group), group
    assert universal


@pytest.mark.parametrize("name", ROBOTS)
def test_the_bound_dominates_the_path_length(name):
    model = _model(name)
    links, spheres = CN.make_spheres(model, 2, 720)
    links, spheres = np.concatenate([[0], links]), np.concatenate([[[0.1, 0.2, 0.3, 0.05]], spheres])   # a sphere on link 0
    qa, dv = _segments(model, 32, 721 + ROBOTS.index(name), 0.8)
    ss = np.linspace(0.0, 1.0, 2049)
    worst = 0.0
    for i in range(32):
        lam = MN.motion_bound(model, qa[i], dv[i], links, spheres)
        cen = MN.centres(model, MN.interpolate_many(model, qa[i], dv[i], ss), links, spheres)
        length = np.linalg.norm(np.diff(cen, axis=0), axis=2).sum(axis=0)
        assert lam[0] == 0.0 and length[0] == 0.0
        assert np.all(length <= lam * (1 + 1e-12)), (name, i, float(np.max(length - lam)))
        worst = max(worst, float(np.max(length[1:] / lam[1:])))
        # s Lambda bounds the length over [s0, s0 + s] too: the second half
        half = np.linalg.norm(np.diff(cen[1024:], axis=0), axis=2).sum(axis=0)
        assert np.all(half <= 0.5 * lam * (1 + 1e-12))
    print("motion bound %s: largest length / Lambda %.3f" % (name, worst))
    assert worst > 0.05   # (the bound is not vacuous)


# ---- 3. the certificate ------------------------------------------------------------------------------------------------------------------
def _small_world(seed):
    rng = np.random.default_rng(seed)
    ws = np.concatenate([rng.uniform(-1.0, 1.0, size=(5, 3)), rng.uniform(0.05, 0.2, size=(5, 1))], axis=1)
    from helpers import random_rotation
    wb = np.array([np.concatenate([random_rotation(rng).reshape(9), rng.uniform(-1.0, 1.0, size=3), rng.uniform(0.05, 0.3, size=3)]) for _ in range(4)])
    return ws, wb


@pytest.mark.parametrize("name", ROBOTS)
def test_free_and_blocked_are_certificates(name):
    model = _model(name)
    links, spheres = CN.make_spheres(model, 2, 730)
    ws, wb = _small_world(731)
    pairs = CN.self_pairs(model.parents, links)
    n, tol = 16, 1e-3
    qa, dv = _segments(model, n, 732 + ROBOTS.index(name), 0.25)
    # the margin: the lower quartile of the clearance at the start, so that most segments start clear whatever the robot's spheres do
    margin = float(np.quantile(MN.clearance_min(model, qa, links, spheres, ws, wb, pairs), 0.25))
    got = MN.advance(model, qa, dv, links, spheres, ws, wb, pairs, margin=margin, tol=tol, max_evals=256)
    ss = np.linspace(0.0, 1.0, 1025)
    count = {MN.FREE: 0, MN.BLOCKED: 0, MN.UNDECIDED: 0}
    for i in range(n):
        st, sf = int(got["status"][i]), float(got["s_free"][i])
        count[st] += 1
        dense = MN.clearance_min(model, MN.interpolate_many(model, qa[i], dv[i], ss), links, spheres, ws, wb, pairs)
        if st == MN.FREE:
            assert sf == 1.0 and np.all(dense >= margin), (name, i, float(dense.min()), margin)
        elif st == MN.BLOCKED:
            at = float(MN.clearance_min(model, MN.interpolate(model, qa[i], dv[i], sf)[None], links, spheres, ws, wb, pairs)[0])
            assert at < margin + tol and np.all(dense[ss < sf] >= margin), (name, i, at)
        # the samples taken say what the result says
        s_k, m_k = np.array(got["samples"][i]).T
        assert got["evals"][i] == s_k.size and got["min_sampled"][i] == m_k.min() and got["s_at_min"][i] == s_k[np.argmin(m_k)]
        assert np.all(np.diff(s_k) > 0) and s_k[0] == 0.0 and s_k[-1] == sf
    print("motion certificate %s: %s, median evals %d, largest %d" % (name, count, np.median(got["evals"]), got["evals"].max()))
    assert count[MN.FREE] > 0 and count[MN.BLOCKED] > 0   # (a segment that grazes a contact for long may stay UNDECIDED: it claims nothing)
    # max_evals ends the loop: UNDECIDED at the last sample taken
    few = MN.advance(model, qa, dv, links, spheres, ws, wb, pairs, margin=margin, tol=tol, max_evals=2)
    und = few["status"] == MN.UNDECIDED
    assert und.any() and np.all(few["evals"][und] == 2) and np.all(few["s_free"][und] < 1.0)
    for i in np.flatnonzero(und):
        assert few["s_free"][i] == got["samples"][i][1][0]


def test_vectorised_pairs_are_the_clearance_querys():
    model = _model("multidof20")
    links, spheres = CN.make_spheres(model, 2, 740)
    ws, wb = _small_world(741)
    pairs = CN.self_pairs(model.parents, links)
    q = model.random_configurations(np.random.default_rng(742), 5)
    want = CN.clearance(model, q, links, spheres, ws, wb, pairs)
    V = MN.pair_values(MN.centres(model, q, links, spheres), spheres[:, 3], ws, wb, pairs)
    names = MN.pair_names(len(links), 5, 4, pairs)
    assert np.array_equal(V, want["table"][0]) and np.array_equal(names[:, 0], want["table"][1])
    assert np.array_equal(names[np.argmin(V, axis=1)], want["witness"]) and np.array_equal(V.min(axis=1), want["min"])


# ---- 4. the thin box ---------------------------------------------------------------------------------------------------------------------
def thin_box_case():
    """panda7, one small sphere on the tool, a segment, and a box of half thickness 0.005 across the sphere's path at s = 0.5"""
    model = QC.model_of("panda7")
    rng = np.random.default_rng(750)
    qa = model.random_configurations(rng, 1)[0]
    dv = np.array([0.9, -0.7, 0.5, 0.8, -0.6, 0.4, 0.3])
    links, spheres = np.array([7], dtype=np.int32), np.array([[0.0, 0.0, 0.1, 0.01]])
    box = MN.thin_box_across(model, qa, dv, 7, spheres[0])
    return model, qa, dv, links, spheres, box


def test_a_thin_box_between_clear_samples_blocks():
    model, qa, dv, links, spheres, box = thin_box_case()
    uniform = np.linspace(0.0, 1.0, 10)   # both endpoints and 8 samples between them
    clear = MN.clearance_min(model, MN.interpolate_many(model, qa, dv, uniform), links, spheres, wboxes=[box])
    assert np.all(clear > 0.0), clear
    got = MN.advance(model, qa[None], dv[None], links, spheres, wboxes=[box], margin=0.0, tol=1e-3)
    assert got["status"][0] == MN.BLOCKED and 4.0 / 9.0 < got["s_free"][0] < 5.0 / 9.0
    assert tuple(got["witness"][0]) == (CN.WORLD_BOX, 0, 0) and got["min_sampled"][0] < 1e-3


# ---- 5. the segments of the GPU tests -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["panda7", "talos32", "multidof20", "helical24", "composite20", "multidof13"])
def test_gpu_cases_stay_clear_of_their_thresholds(name):
    """tests/test_motion_clearance.py leaves a segment out of the comparison when a decision of the reference lies within 1e-9 of its
    threshold, at most 2 % of a robot's: with its seeds the reference alone stays within that, and all three outcomes occur"""
    from test_motion_clearance import motion_case
    c = motion_case(name)
    want = c["want"]
    assert want["near"].sum() <= 0.02 * c["n"], (name, int(want["near"].sum()))
    for st in (MN.FREE, MN.BLOCKED, MN.UNDECIDED):
        assert (want["status"] == st).any(), (name, st)


def test_gpu_path_cases_stay_clear_of_their_thresholds():
    """... and so do the paths of tests/test_motion_path.py, whose segments are compared under the same cap; over each robot's paths
    all three outcomes occur"""
    from test_motion_path import PATH_ROBOTS, PATH_SIZES, path_case
    for name in PATH_ROBOTS:
        seen = set()
        for B, T in PATH_SIZES:
            want = path_case(name, B, T)["want"]
            assert want["status"].shape == (B * (T - 1),)
            assert want["near"].sum() <= 0.02 * want["near"].size, (name, B, T, int(want["near"].sum()))
            seen |= {int(st) for st in want["status"]}
        assert seen == {MN.FREE, MN.BLOCKED, MN.UNDECIDED}, (name, seen)


def test_gpu_composite_cases_stay_clear_of_their_thresholds():
    """... and the segments of test_motion_clearance.test_a_sphere_on_the_universal_joint_alone"""
    from test_motion_clearance import universal_case
    c = universal_case()
    want = c["want"]
    assert want["near"].sum() <= 0.02 * c["n"], int(want["near"].sum())
    for st in (MN.FREE, MN.BLOCKED, MN.UNDECIDED):
        assert (want["status"] == st).any(), st
