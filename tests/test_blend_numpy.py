"""CPU: the numpy reference of the blend rule (tests/blend_numpy.py) keeps what include/loik_amd_blend.h promises: the bound of a curve
dominates the length of every sphere centre's path, every piece is feasible after the two passes, position and velocity are continuous
where pieces join, the limits hold on the samples, a blend stays within its half-length of the corner, and max_tries = 0 is
retime_numpy.  It also fixes the inputs of the GPU test (test_blend.py) and checks that they cover every status and stay clear of
every threshold."""
import numpy as np
import pytest

import blend_numpy as BN
import clearance_numpy as CN
import motion_numpy as MN
import pose_numpy as P
import retime_numpy as RN
import test_clearance as TC
import test_motion_clearance as TM
import test_retime_numpy as TR

T_PATH, DT, S_ROWS, RNG = 6, 0.02, 256, 1300
TOL, MAX_EVALS, MAX_TRIES = 1e-3, 24, 3
SIX = ("panda7", "talos32", "multidof13", "composite20", "multidof20", "helical24")
# the rng of a robot's paths and world: RNG unless its reference has a decision within 1e-9 of a threshold (then the next one, recorded here)
RNG_OF = {}
# the quantile of the waypoints' clearance that is the margin: low enough that most corners are clear, high enough that some are not
QUANTILE = 0.2

_CASES = {}


def coupled_blocks(model):
    """(iq, nq) of every spherical, free-flyer or planar (sub-)joint"""
    ch, _ = MN.chain_of(model)
    nq_of = {P.J_FREEFLYER: 7, P.J_SPHERICAL: 4, P.J_PLANAR: 4}
    return [(int(ch.idx_q[i]), nq_of[int(ch.jtype[i])]) for i in range(1, ch.njoints) if int(ch.jtype[i]) in nq_of]


def make_paths(model, q0, size, T, rng):
    """[B][T][nq] as test_shortcut.make_paths draws them, then shaped so that every kind of corner occurs: leg 2 of every path but 1 and 2 is short (it
    vanishes between the blends of corners 2 and 3), waypoint 3 of path 1 repeats waypoint 2, and the spherical, free-flyer and planar
    joints of every path but path 2 keep their coordinates on the odd legs, bit for bit (they move on one leg only at every corner)"""
    B = q0.shape[0]
    steps = size * rng.uniform(-1.0, 1.0, size=(B, T - 1, model.nv))
    steps[[b for b in range(B) if b not in (1, 2)], 2] *= 0.3
    blocks = coupled_blocks(model)
    paths = np.empty((B, T, model.nq))
    for b in range(B):
        paths[b, 0] = q0[b]
        for k in range(T - 1):
            nxt = P.integrate(model, paths[b, k], steps[b, k])
            if b == 1 and k == 2:
                nxt = paths[b, k].copy()
            if b != 2 and k % 2 == 1:
                for iq, n in blocks:
                    nxt[iq:iq + n] = paths[b, k, iq:iq + n]
            paths[b, k + 1] = nxt
    return np.ascontiguousarray(paths)


def reach_of(name, nv):
    return 0.2 * TM.SIZE[name] * np.sqrt(nv)


def blend_case(name, rng=None):
    """the model and spheres of test_clearance._case, a world of three spheres and two boxes, B = 5 paths of T = 6 waypoints (3 for the two
    big trees), the limits of test_retime_numpy, the margin = a quantile of the clearance over all waypoints, and the numpy answer at
    S = 256: computed once"""
    if name not in _CASES:
        rng = RNG_OF.get(name, RNG) if rng is None else rng
        c = dict(TC._case(name))
        model = c["model"]
        B = 3 if name in TC.BIG_TREES else 5
        g = np.random.default_rng(rng)
        c["B"], c["paths"] = B, make_paths(model, c["q"][:B], TM.SIZE[name], T_PATH, g)
        c["ws"], c["wb"] = TC._world(g, 3, 2)
        c["v_max"], c["a_max"] = TR.limits(name, model.nv)
        at = MN.clearance_min(model, c["paths"].reshape(-1, model.nq), c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"])
        c["margin"] = float(np.quantile(at, QUANTILE))
        c["kw"] = dict(dt=DT, reach=reach_of(name, model.nv), margin=c["margin"], tol=TOL, max_evals=MAX_EVALS, max_tries=MAX_TRIES)
        c["want"] = BN.blend(model, c["paths"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], c["v_max"], c["a_max"], S=S_ROWS, **c["kw"])
        _CASES[name] = c
    return _CASES[name]


def check_comparable(want):
    """no decision of the reference within 1e-9 of its threshold: every sampled minimum against margin + tol, every step against u = 1, and
    D / dt against an integer (test_retime.py's rule)"""
    assert not want["near"].any(), np.argwhere(want["near"])
    ok = want["flags"] & (BN.INVALID | BN.SKIPPED) == 0
    assert np.all(TR.off_integer(want["duration"][ok] / DT) > 1e-9)


def statuses(want):
    return want["corner_info"][:, :, 0]


# ---- 1. the bound -----------------------------------------------------------------------------------------------------------------------
def _corners(model, n, seed, size):
    """n random blendable corners: q_k, P0, P2 with the coupled blocks of one of the two set to zero"""
    rng = np.random.default_rng(seed)
    qk = model.random_configurations(rng, n)
    P0, P2 = size * rng.uniform(-1.0, 1.0, size=(n, model.nv)), size * rng.uniform(-1.0, 1.0, size=(n, model.nv))
    ch, _ = MN.chain_of(model)
    for i in range(1, ch.njoints):
        m = BN._COUPLED_NV.get(int(ch.jtype[i]))
        if m:
            iv = int(ch.idx_v[i])
            for r in range(n):
                (P0 if r % 2 else P2)[r, iv:iv + m] = 0.0
    return qk, P0, P2


@pytest.mark.parametrize("name", list(TC.ROBOTS))
def test_the_bound_dominates_the_path_length(name):
    model = TC._model(name)
    big = name in TC.BIG_TREES
    links, spheres = CN.make_spheres(model, 1 if big else 2, 1310)
    links, spheres = np.concatenate([[0], links]), np.concatenate([[[0.1, 0.2, 0.3, 0.05]], spheres])   # a sphere on link 0
    n, dense = (3, 513) if big else (16, 2049)
    qk, P0, P2 = _corners(model, n, 1311 + list(TC.ROBOTS).index(name), 0.6 if not big else 0.1)
    if name == "multidof13":
        assert len(coupled_blocks(model)) >= 2 and BN.coupled(model, P0[0] + P2[0], P0[1] + P2[1])   # (its free-flyer and planar joints move, on one leg each)
    uu = np.linspace(0.0, 1.0, dense)
    half = (dense - 1) // 2
    worst = 0.0
    for i in range(n):
        assert not BN.coupled(model, P0[i], P2[i])
        lam = BN.curve_bound(model, qk[i], P0[i], P2[i], links, spheres)
        cen = MN.centres(model, np.stack([BN.curve_point(model, qk[i], P0[i], P2[i], u) for u in uu]), links, spheres)
        step = np.linalg.norm(np.diff(cen, axis=0), axis=2)
        length = step.sum(axis=0)
        assert lam[0] == 0.0 and length[0] == 0.0
        assert np.all(length <= lam * (1 + 1e-12)), (name, i, float(np.max(length - lam)))
        # du Lambda bounds the length over [u, u + du] too: each half, and every sixteenth
        assert np.all(step[half:].sum(axis=0) <= 0.5 * lam * (1 + 1e-12)) and np.all(step[:half].sum(axis=0) <= 0.5 * lam * (1 + 1e-12))
        sixteenth = step.reshape(16, -1, step.shape[1]).sum(axis=1)
        assert np.all(sixteenth <= lam / 16.0 * (1 + 1e-12))
        worst = max(worst, float(np.max(length[1:] / lam[1:])))
    print("blend bound %s: largest length / Lambda %.3f" % (name, worst))
    assert worst > 0.05   # (the bound is not vacuous)


# ---- 2. the rule on the reference's own output ------------------------------------------------------------------------------------------
def check_rule(c, r, paths=None):
    """every piece feasible, position and velocity continuous where pieces join, |w| <= l <= reach on every corner taken"""
    model, v_max, a_max, reach = c["model"], c["v_max"], c["a_max"], c["kw"]["reach"]
    paths = c["paths"] if paths is None else paths
    for b in range(paths.shape[0]):
        if r["flags"][b] & (BN.INVALID | BN.SKIPPED):
            continue
        recs, dvs = r["records"][b], r["dv"][b]
        rows = paths[b, :int(r["n_waypoints"][b])]
        for rec in recs:
            if rec["blend"] or not rec["D"] > 0.0:
                continue
            # feasible: the rates are reachable from one another over the piece, and none is above the leg's limit
            assert abs(rec["v0"] ** 2 - rec["v1"] ** 2) <= 2.0 * rec["A"] * rec["sl"] * (1 + 1e-12) + 1e-15, (b, rec)
            assert max(rec["v0"], rec["v1"]) <= rec["vp"] <= rec["V"] * (1 + 1e-12), (b, rec)
        moving = [rec for rec in recs if rec["D"] > 0.0]
        for a, z in zip(moving[:-1], moving[1:]):
            qa, va = BN.piece_at(model, rows, dvs, a, a["D"])
            qz, vz = BN.piece_at(model, rows, dvs, z, 0.0)
            gap = MN.difference(model, qa, qz)[0]
            assert np.max(np.abs(gap)) <= 1e-12 and np.max(np.abs(va - vz) / v_max) <= 1e-9, (b, a, z, np.max(np.abs(gap)), np.max(np.abs(va - vz) / v_max))
        q0, v0 = BN.piece_at(model, rows, dvs, moving[0], 0.0) if moving else (rows[0], np.zeros(model.nv))
        assert np.array_equal(q0, rows[0]) and np.all(v0 == 0.0)
        if moving:
            q1, v1 = BN.piece_at(model, rows, dvs, moving[-1], moving[-1]["D"])
            assert np.max(np.abs(MN.difference(model, q1, rows[-1])[0])) <= 1e-12 and np.max(np.abs(v1) / v_max) <= 1e-9
        for k in range(1, rows.shape[0] - 1):
            l, ri, ro, w, _ = r["corner"][b, k - 1]
            if r["corner_info"][b, k - 1, 0] != BN.TAKEN:
                assert l == 0.0 and ri == 0.0 and ro == 0.0 and w == 0.0
                continue
            assert 0.0 < l <= reach and 0.0 < w <= r["w_max"][b, k - 1] and ri <= 0.5 and ro <= 0.5
            P0, P2 = r["controls"][(b, k)]
            for u in np.linspace(0.0, 1.0, 33):
                assert BN.norm_of(BN.w_of(P0, P2, u)) <= l * (1 + 1e-12)
            # the rate limit: the blend's velocity and its constant acceleration are within the limits, and one of them is met
            acc = np.max(2.0 * np.abs(P0 + P2) * r["w_max"][b, k - 1] ** 2 / a_max)
            vel = max(np.max(2.0 * np.abs(P0) * r["w_max"][b, k - 1] / v_max), np.max(2.0 * np.abs(P2) * r["w_max"][b, k - 1] / v_max))
            assert max(acc, vel) <= 1 + 1e-12 and abs(max(acc, vel) - 1.0) <= 1e-12


@pytest.mark.parametrize("name", SIX)
def test_the_rule_on_the_references_output(name):
    c = blend_case(name)
    want = c["want"]
    check_rule(c, want)
    assert np.all(want["flags"] == 0) and np.all(want["n_samples"] <= S_ROWS)
    TR.check_limits(want, c["v_max"], c["a_max"], DT)
    for b in range(c["B"]):
        ns = int(want["n_samples"][b])
        assert np.array_equal(want["q_traj"][b, 0], c["paths"][b, 0])
        assert np.array_equal(want["q_traj"][b, ns - 1:], np.tile(c["paths"][b, -1], (S_ROWS - ns + 1, 1)))


# ---- 3. reduction -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("panda7", "multidof13"))
def test_no_tries_is_retime(name):
    c = blend_case(name)
    model = c["model"]
    got = BN.blend(model, c["paths"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], c["v_max"], c["a_max"], S=S_ROWS, **dict(c["kw"], max_tries=0))
    ref = RN.retime(model, c["paths"], c["v_max"], c["a_max"], DT, S=S_ROWS)
    assert np.all(statuses(got) == BN.OFF) and np.all(got["taken"] == 0)
    assert np.array_equal(got["n_samples"], ref["n_samples"]) and np.array_equal(got["flags"], ref["flags"])
    for k in ("duration", "q_traj", "v_traj"):
        assert np.max(np.abs(got[k] - ref[k]) / (1.0 + np.abs(ref[k]))) <= 1e-12, k
    assert np.max(np.abs(got["piece"][:, 0::2, :2] - ref["seg"][:, :, :2])) <= 1e-12 and np.all(got["piece"][:, 1::2] == 0.0)


# ---- 4. coverage of the inputs -----------------------------------------------------------------------------------------------------------
def coverage(want):
    """what the cases of the GPU test must show between them, from one reference answer"""
    st, tries = want["corner_info"][:, :, 0], want["corner_info"][:, :, 1]
    cor = want["corner"]
    touching = (st[:, :-1] == BN.TAKEN) & (st[:, 1:] == BN.TAKEN) & (cor[:, :-1, 2] + cor[:, 1:, 1] == 1.0)
    return dict(first=int(np.sum((st == BN.TAKEN) & (tries == 1))), later=int(np.sum((st == BN.TAKEN) & (tries > 1))),
                blocked=int(np.sum((st == BN.BLOCKED) & (tries == MAX_TRIES))), undecided=int(np.sum(st == BN.UNDECIDED)),
                coupled=int(np.sum(st == BN.COUPLED)), zero_leg=int(np.sum(st == BN.ZERO_LEG)), touching=int(np.sum(touching)))


@pytest.mark.parametrize("name", list(TC.ROBOTS))
def test_inputs_stay_clear_of_their_thresholds(name):
    check_comparable(blend_case(name)["want"])


def test_inputs_cover_every_kind_of_corner():
    total = {}
    for name in SIX:
        cov = coverage(blend_case(name)["want"])
        print("blend coverage %s: %s" % (name, cov))
        for k, v in cov.items():
            total[k] = total.get(k, 0) + v
    for k in ("first", "later", "blocked", "coupled", "zero_leg", "touching"):
        assert total[k] > 0, (k, total)


def test_duration_is_not_longer_than_retime():
    for name in SIX:
        c = blend_case(name)
        want = c["want"]
        ref = RN.retime(c["model"], c["paths"], c["v_max"], c["a_max"], DT)
        some = want["taken"] > 0
        assert some.any() and np.all(want["duration"][some] <= ref["duration"][some]), (name, want["duration"], ref["duration"])


def test_edges_of_the_rule():
    c = blend_case("panda7")
    model, paths = c["model"], c["paths"]
    args = (c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], c["v_max"], c["a_max"])
    n = np.array([0, 1, 2, T_PATH, T_PATH + 1])
    r = BN.blend(model, paths[:5], *args, n_waypoints=n, S=S_ROWS, **c["kw"])
    assert r["flags"].tolist() == [BN.SKIPPED, BN.SKIPPED, 0, 0, BN.SKIPPED] and r["n_waypoints"].tolist() == [0, 0, 2, T_PATH, 0]
    assert np.isnan(r["duration"][[0, 1, 4]]).all() and np.isnan(r["q_traj"][[0, 1, 4]]).all() and np.isnan(r["corner"][[0, 1, 4]]).all()
    assert np.all(statuses(r)[[0, 1, 2, 4]] == BN.OFF) and np.all(r["piece"][2, 1:] == 0.0) and np.all(r["corner"][2] == 0.0)
    assert np.array_equal(r["q_traj"][3], c["want"]["q_traj"][3])
    bad = paths[:3].copy()
    bad[1, 2, 0] = np.nan
    r = BN.blend(model, bad, *args, S=S_ROWS, **c["kw"])
    assert r["flags"].tolist() == [0, BN.INVALID, 0] and r["n_samples"][1] == 0 and np.isnan(r["q_traj"][1]).all() and np.isnan(r["duration"][1])
    r = BN.blend(model, paths[:2], *args, S=50, **c["kw"])
    assert np.all(r["flags"] == BN.TRUNCATED) and np.array_equal(r["q_traj"], c["want"]["q_traj"][:2, :50])
    r = BN.blend(model, paths[:2], *args, **c["kw"])
    assert np.all(r["flags"] == 0) and np.array_equal(r["duration"], c["want"]["duration"][:2]) and "q_traj" not in r
