"""GPU: the voxel world (include/loik_amd_grid.h) through every kernel of the motion layer, against numpy: k_motion_clearance (the dv route
and the path route), k_shortcut_paths, k_plan_paths and k_blend_paths, each in its LDS build (panda7, talos32, multidof13) and its slab
build (tree330), in a world that has spheres, boxes, self pairs and a grid at once, so that the grid pairs sit between the boxes and the
self pairs in the ordinal order and compete with them for the minimum and for the step.  The references are grid_numpy.advance and
shortcut_numpy, plan_numpy and blend_numpy with grid=, tied to the geometry on the CPU by test_grid_numpy.py; the inputs are
grid_cases.py's, and what makes them worth running (the three outcomes, the share of voxel witnesses, the difference to the same call
without the grid, the rows too close to a threshold to compare) is asserted on the reference before the device is asked.

Then the grid pair behind a call (k_shortcut_paths<false>) against the pair in line, bit for bit; and the edges at the smallest shapes: an
empty and a full grid, a segment outside the grid's box and one through it, a grid one voxel thick, centres that cross a voxel face
exactly, a grid replaced and cleared between calls, and a row that is not finite."""
import numpy as np
import pytest

import loik_amd
from loik_amd import capi

import blend_numpy as BN
import clearance_numpy as CN
import grid_cases as GC
import grid_numpy as GN
import motion_numpy as MN
import plan_numpy as PN
import pose_numpy as P
import shortcut_numpy as SN
import test_blend as TBL
import test_blend_numpy as TB
import test_clearance as TC
import test_grid_clearance as TG
import test_motion_clearance as TM
import test_plan as TPL
import test_plan_numpy as TP
import test_shortcut as TS

pytestmark = pytest.mark.gpu

BOUND, S_BOUND = TM.BOUND, TM.S_BOUND
FREE, BLOCKED, UNDECIDED, INVALID = MN.FREE, MN.BLOCKED, MN.UNDECIDED, MN.INVALID


def _open(c, grid=True, q=None):
    s = TM._open(c, q=q)
    if grid is not None and grid is not False:
        TG._set(s, c["grid"] if grid is True else grid)
    return s


def _lds_bytes(c, T=None, extra_nb=0):
    """the bytes of LDS a wavefront of the motion layer needs for this robot (motion_aux_doubles and its kin in loik_amd/csrc): above 64 KB
    the kernels take the slab build"""
    ns, nb, ncar = len(c["links"]), c["model"].nv, len(set(int(l) for l in c["links"]))
    n = 4 * ns + ns + 12 * nb + 12 * ncar + extra_nb * nb
    if T is not None:      # the tables of a blend, as test_blend has them
        n += 2 * nb + 3 * (T - 1) + 5 * (T - 2) + 8 * (2 * T - 3) + (T - 1) * nb
    return 8 * n


def _check_build(name, c, **kw):
    need = _lds_bytes(c, **kw)
    if name == GC.SLAB:
        assert need > 65536, need            # the slab build
    else:
        assert need <= 65536 - 8192, need    # the LDS build


def _differs(want, plain, keys=("status", "evals")):
    return int(np.any(np.stack([want[k] != plain[k] for k in keys]), axis=0).sum())


def _inputs_are_worth_running(what, want, plain, small):
    """the conditions on a batch of segments: the three outcomes, voxel witnesses, the grid matters and so do the other pairs"""
    n = want["status"].size
    count = [int((want["status"] == st).sum()) for st in range(4)]
    share, differ = GC.kind4_share(want["witness"]), -1 if plain is None else _differs(want, plain)
    print("grid_measured %s: free / blocked / undecided %s, voxel witnesses %.0f %%, %d of %d segments differ from the call without the grid, near %d" % (
        what, count[:3], 100.0 * share, differ, n, int(want["near"].sum())))
    if small:
        assert min(count[:3]) > 0, (what, count)
        assert share >= 0.1, (what, share)
        assert differ >= 0.05 * n, (what, differ)
        assert share < 1.0 and differ < n, what      # (... and so do the other pairs)


def _flat(r):
    """a result of path_clearance [B][T - 1] as the rows of motion_clearance"""
    return {k: v.reshape((-1,) + v.shape[2:]) for k, v in r.items()}


def _compare(got, want, scale, what):
    e_s, e_min = TM._compare(got, want, scale, what)
    print("grid_measured %s: max |s - numpy| %.3e (bound %.3e), max |min_sampled - numpy| / scale %.3e (bound %.1e)" % (what, e_s, S_BOUND, e_min, BOUND))


# ---- 1. k_motion_clearance: the dv route and the path route -------------------------------------------------------------------------------
def _motion(c, what, small):
    want = c["want"]
    _inputs_are_worth_running(what, want, c.get("plain"), small)
    qa, dv, qb, kw = c["qa"], c["dv"], c["qb"], c["kw"]
    s = _open(c)
    got = s.motion_clearance(qa, dv=dv, **kw)
    _compare(got, want, c["scale"], what + " dv route")
    assert TM._same(got, s.motion_clearance(qa, dv=dv, **kw))            # two launches, the same bits
    # T > 0: the segments between the rows of a path, the device's own difference
    paths = np.ascontiguousarray(np.stack([qa, qb], axis=1))
    via = _flat(s.path_clearance(paths, **kw))
    _compare(via, c["want_path"], c["scale"], what + " path route")
    assert TM._same(via, _flat(s.path_clearance(paths, **kw)))
    assert TM._same(via, s.motion_clearance(qa, qb=qb, **kw))             # the end points given to the dv route: the same rows
    s.close()


@pytest.mark.parametrize("name", GC.ROBOTS)
def test_motion_clearance_with_a_grid_matches_numpy(name):
    c = GC.motion_case(name)
    _check_build(name, c)
    _motion(c, name, name in GC.SMALL)


@pytest.mark.parametrize("ns", GC.SIZES)
def test_motion_clearance_sizes(ns):
    """the sphere counts at which the world-pair loops change their shape: one sphere slot, 64 slots with idle lanes (63), exactly 64, more
    than 64 (65, 130: a lane takes several spheres, and (lane >> lp) == 0 gates the grid pair to one lane per sphere)"""
    c = GC.sizes_case(ns)
    want = c["want"]
    if ns > 1:      # (one sphere on the universe never moves; beyond it the grid decides some segments and names some minima)
        assert 0.0 < GC.kind4_share(want["witness"]) < 1.0 and _differs(want, c["plain"]) > 0
    _motion(c, "panda7 ns=%d" % ns, False)


# ---- 2. k_shortcut_paths, and the pair behind a call against the pair in line ---------------------------------------------------------------
@pytest.mark.parametrize("name", GC.ROBOTS)
def test_shortcut_with_a_grid_matches_numpy_and_the_inline_pair(name):
    c = GC.shortcut_case(name)
    model, paths, want, B, kw = c["model"], c["paths"], c["want"], c["B"], c["kw"]
    mkw = dict(margin=kw["margin"], tol=kw["tol"], max_evals=kw["max_evals"])
    _check_build(name, c, extra_nb=1)
    tot = {k: int(want[k].sum()) for k in TS.COUNTERS}
    print("grid_measured shortcut %s: %s, paths with near %d, waypoints left %s" % (name, tot, int(want["near"].sum()), want["n_waypoints"].tolist()))
    assert want["near"].sum() <= B // 16
    if name in GC.SMALL:
        assert tot["accepted"] > 0 and tot["blocked"] > 0, tot
        _inputs_are_worth_running("shortcut %s, the segments tried" % name, c["tried_want"], c["tried_plain"], True)
    s = _open(c)
    got = s.shortcut_paths(paths, **kw)
    TS._check_shape(got, paths)
    assert TS._same(got, s.shortcut_paths(paths, **kw))                   # two launches, the same bits
    sure = ~want["near"]
    for k in TS.COUNTERS + ("keep",):
        assert np.array_equal(got[k][sure], want[k][sure]), (name, k, got[k], want[k])
    err = TS._length_error(TS._rows(got, sure), TS._rows({k: want[k] for k in got}, sure))
    print("grid_measured shortcut %s: max |length - numpy| / (1 + length) %.3e (bound %.3e)" % (name, err, TS.LENGTH_BOUND))
    assert err <= TS.LENGTH_BOUND, (name, err)
    # every segment the kernel tried (the reference's list: keep and the counters are its own on the sure paths), checked by
    # k_motion_clearance, which has the grid pair in line: its rows are the reference's, and the kernel's counters follow from them
    tried = [t for t in c["tried"] if sure[t[0]]]
    rows = np.array([k for k, t in enumerate(c["tried"]) if sure[t[0]]], dtype=int)
    qa = np.ascontiguousarray(np.stack([paths[b, i] for b, i, j in tried]))
    qb = np.ascontiguousarray(np.stack([paths[b, j] for b, i, j in tried]))
    seg = s.motion_clearance(qa, qb=qb, **mkw)
    cen = MN.centres(model, paths.reshape(-1, model.nq), c["links"], c["spheres"])
    scale = 1.0 + float(np.max(np.abs(cen))) + float(np.max(c["spheres"][:, 3]))
    e = TM._compare(seg, c["tried_want"], scale, "shortcut %s, the segments tried" % name, rows=rows)
    print("grid_measured shortcut %s, the %d segments tried: max |s - numpy| %.3e, max |min_sampled - numpy| / scale %.3e" % ((name, rows.size) + e))
    path_of = np.array([b for b, i, j in tried])
    for b in np.flatnonzero(sure):
        st = seg["status"][path_of == b]
        assert got["accepted"][b] == np.sum(st == FREE) and got["blocked"][b] == np.sum(st == BLOCKED), (name, b)
        assert got["undecided"][b] == st.size - np.sum(st == FREE) - np.sum(st == BLOCKED) - got["invalid"][b] and got["invalid"][b] == 0, (name, b)
    # every spliced segment of the output was tried and accepted as exactly that segment: its row under path_clearance equals the row
    # of motion_clearance, bit for bit
    chk = s.path_clearance(got["q_path"], **mkw)
    index = {t: k for k, t in enumerate(tried)}      # (the last try of a segment, should one be drawn twice: the same ends, the same row)
    seen = 0
    for b in np.flatnonzero(sure):
        L, keep = int(got["n_waypoints"][b]), got["keep"][b]
        for k in range(L - 1):
            if keep[k + 1] == keep[k] + 1:
                continue
            seen += 1
            r = index[(int(b), int(keep[k]), int(keep[k + 1]))]
            assert chk["status"][b, k] == FREE and all(np.array_equal(seg[f][r], chk[f][b, k]) for f in seg), (name, b, k)
    assert seen > 0 or tot["accepted"] == 0
    s.close()


# ---- 3. k_plan_paths ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GC.ROBOTS)
def test_plan_with_a_grid_matches_numpy(name):
    c = GC.plan_case(name)
    model, want, B = c["model"], c["want"], c["B"]
    _check_build(name, c, extra_nb=1)
    print("grid_measured plan %s: status %s, L %s, iterations %s, queries with near %d" % (
        name, want["status"].tolist(), want["n_waypoints"].tolist(), want["iterations"].tolist(), int(want["near"].sum())))
    assert want["near"].sum() <= B // 16
    if name in GC.SMALL:
        differ = int(np.any(np.stack([np.asarray(want[k] != c["plain"][k]).reshape(B, -1).any(axis=1) for k in TPL.FIELDS]), axis=0).sum())
        found = want["status"] == PN.FOUND
        print("grid_measured plan %s: %d of %d queries differ from the call without the grid" % (name, differ, B))
        assert 0.05 * B <= differ < B and (found & (want["iterations"] > 0)).any() and (~found).any()
    s = _open(c)
    got = TPL._plan(s, c, T=GC.T_PLAN)
    assert TPL._same(got, TPL._plan(s, c, T=GC.T_PLAN))                   # two launches, the same bits
    TPL._check_self(s, got, c["start"], c["goal"], c["kw"]["margin"], GC.TOL, c["kw"]["max_evals"])
    sure = ~want["near"]
    for k in TPL.FIELDS:
        assert np.array_equal(got[k][sure], want[k][sure]), (name, k, got[k], want[k])
    found = sure & (want["status"] == PN.FOUND)
    err = 0.0
    for k in ("q_path", "length"):
        err = max(err, float(np.max(np.abs(got[k][found] - want[k][found]) / (1.0 + np.abs(want[k][found])), initial=0.0)))
    print("grid_measured plan %s: max |got - numpy| / (1 + |numpy|) over rows and lengths %.3e (bound %.3e)" % (name, err, TPL.PLAN_BOUND))
    assert err <= TPL.PLAN_BOUND, (name, err)
    s.close()


# ---- 4. k_blend_paths --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GC.ROBOTS)
def test_blend_with_a_grid_matches_numpy(name):
    c = GC.blend_case(name)
    model, paths, want = c["model"], c["paths"], c["want"]
    TB.check_comparable(want)
    _check_build(name, c, T=GC.T_PATH)
    info = want["corner_info"]
    tried = info[:, :, 1] > 0
    share, differ = GC.kind4_share(info[:, :, 3:][tried]), int(np.any(info != c["plain"]["corner_info"], axis=2).sum()) if "plain" in c else -1
    print("grid_measured blend %s: %s, voxel witnesses %.0f %% of the %d corners tried, %d corners differ from the call without the grid" % (
        name, TB.coverage(want), 100.0 * share, int(tried.sum()), differ))
    if name in GC.SMALL:
        st = TB.statuses(want)
        assert (st == BN.TAKEN).any() and (st == BN.BLOCKED).any()
        assert 0.1 <= share < 1.0 and 0.05 * tried.sum() <= differ < tried.sum(), (name, share, differ)
    s = _open(c)
    kw = dict(v_max=c["v_max"], a_max=c["a_max"], max_samples=TB.S_ROWS, **c["kw"])
    got = s.blend_paths(paths, **kw)
    err = TBL._check(name, "with a grid", got, want)
    print("grid_measured blend %s: max |got - numpy| / (1 + |numpy|) %.3e (bound %.3e)" % (name, err, TBL.BLEND_BOUND))
    assert TBL._same(got, s.blend_paths(paths, **kw))                    # two launches, the same bits
    s.close()


# ---- 5. the edges ------------------------------------------------------------------------------------------------------------------------------
def _wall():
    """test_plan_numpy.wall_case: panda7, one sphere of radius 0.01 on link 7, the segment A -> Bq; c0, cm, c1 the sphere's centre at its
    start, its middle and its end"""
    w = dict(TP.wall_case())
    w["dv"] = w["Bq"] - w["A"]
    q = MN.interpolate_many(w["model"], w["A"], w["dv"], [0.0, 0.5, 1.0])
    w["c0"], w["cm"], w["c1"] = MN.centres(w["model"], q, w["links"], w["spheres"])[:, 0]
    w["scale"] = 1.0 + float(np.abs([w["c0"], w["cm"], w["c1"]]).max()) + 0.01
    return w


def _corner_voxel(n):
    occ = np.zeros(n[::-1], dtype=np.uint8)
    occ[0, 0, 0] = 1
    return occ


def _wall_check(w, grid, what, ws=(), margin=0.0, max_evals=64):
    """the wall segment against `grid` (and the world spheres ws) on the device and in numpy; every row is compared, none is near"""
    model, A, dv = w["model"], w["A"], w["dv"]
    want = GN.advance(model, A[None], dv[None], w["links"], w["spheres"], ws, (), grid, margin=margin, tol=GC.TOL, max_evals=max_evals)
    assert not want["near"].any(), what
    s = TC._open(model, np.stack([A, w["Bq"]]))
    s.set_collision_spheres(w["links"], w["spheres"])
    if len(ws):
        s.set_collision_world(np.asarray(ws), None)
    TG._set(s, grid)
    got = s.motion_clearance(A[None], dv=dv[None], margin=margin, tol=GC.TOL, max_evals=max_evals)
    s.close()
    print("grid_measured edge %s: status %d evals %d s_free %.6f min_sampled %.6f witness %s" % (
        what, got["status"][0], got["evals"][0], got["s_free"][0], got["min_sampled"][0], got["witness"][0].tolist()))
    _compare(got, want, w["scale"], "edge " + what)
    # where the centre was at the samples: inside the grid's box or outside it
    cen = np.stack([MN.centres(model, MN.interpolate(model, A, dv, sv)[None], w["links"], w["spheres"])[0, 0] for sv, _ in want["samples"][0]])
    inside = np.all((cen >= grid.origin) & (cen <= grid.hi), axis=1)
    return got, want, inside


def test_an_empty_grid_and_a_full_one():
    w = _wall()
    empty = GN.Grid(np.zeros((3, 3, 3), dtype=np.uint8), w["cm"] - 0.15, 0.1)
    # nothing else in the world: +inf at both samples, FREE in two, and the grid pair is the witness (the lowest ordinal among equals)
    got, want, _ = _wall_check(w, empty, "an empty grid")
    vox = int(GN.sphere_grid(w["c0"], 0.01, empty)[1])
    assert got["status"][0] == FREE and got["evals"][0] == 2 and np.isposinf(got["min_sampled"][0]) and got["s_free"][0] == 1.0
    assert tuple(got["witness"][0]) == (capi.CLR_WORLD_GRID, 0, vox)
    # a world sphere beside it: a finite value beats +inf, the witness is the sphere pair
    got, want, _ = _wall_check(w, empty, "an empty grid and a world sphere", ws=np.array([[3.0, 3.0, 3.0, 0.1]]))
    assert tuple(got["witness"][0]) == (capi.CLR_WORLD_SPHERE, 0, 0) and np.isfinite(got["min_sampled"][0])
    # every voxel occupied, the robot inside: BLOCKED at the first sample, the value the distance to the voxel's centre below zero
    full = GN.Grid(np.ones((8, 8, 8), dtype=np.uint8), (-2.0, -2.0, -2.0), 0.5)
    got, want, inside = _wall_check(w, full, "a full grid")
    i = np.floor((w["c0"] - full.origin) / full.h)
    e2 = float(((w["c0"] - (full.origin + (i + 0.5) * full.h)) ** 2).sum())
    assert inside.all() and got["status"][0] == BLOCKED and got["evals"][0] == 1 and got["s_free"][0] == 0.0
    assert want["min_sampled"][0] == -np.sqrt(e2) - 0.01 and abs(got["min_sampled"][0] - want["min_sampled"][0]) <= BOUND * w["scale"]
    assert tuple(got["witness"][0]) == (capi.CLR_WORLD_GRID, 0, int((i[2] * 8 + i[1]) * 8 + i[0]))


def test_segments_outside_through_and_along_a_thin_grid():
    w = _wall()
    N, H = 21, 0.01
    # wholly outside the grid's box: dout > 0 at every sample
    far = GN.Grid(GN.random_occupancy((4, 3, 2), 0.3, 1601), w["c0"] + np.array([0.4, 0.5, 0.3]), 0.1)
    assert far.occ.any()
    got, want, inside = _wall_check(w, far, "a segment outside the box")
    assert not inside.any() and want["evals"][0] > 2 and tuple(want["witness"][0][:2]) == (GN.WORLD_GRID, 0)
    # in and out again: a box of 21 cm about the middle of the segment, one occupied voxel in its corner
    box = GN.Grid(_corner_voxel((N, N, N)), w["cm"] - 0.5 * N * H, H)
    got, want, inside = _wall_check(w, box, "a segment through the box")
    assert not inside[0] and inside.any() and (got["status"][0] != FREE or not inside[-1]), inside
    # the same box one voxel thick along each axis in turn
    for ax in range(3):
        n = [N, N, N]
        n[ax] = 1
        thin = GN.Grid(_corner_voxel(tuple(n)), w["cm"] - 0.5 * np.array(n) * H, H)
        got, want, inside = _wall_check(w, thin, "a grid with one voxel along axis %d" % ax)
        assert want["evals"][0] > 2


def _slider():
    """a prismatic joint along x on the universe, its placement the identity, and two revolutes behind it that carry nothing: a sphere on
    link 1 has the centre (offset + (q, 0, 0)), exactly, where the numbers are binary fractions"""
    placement = np.array([np.concatenate([np.eye(3).ravel(), np.zeros(3)]), np.concatenate([np.eye(3).ravel(), np.zeros(3)]),
                          np.concatenate([np.eye(3).ravel(), [0.0, 0.0, 0.25]]), np.concatenate([np.eye(3).ravel(), [0.0, 0.25, 0.0]])])
    axis = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]])
    return loik_amd.Model([0, 0, 1, 2], [0, P.J_PX, P.J_RZ, P.J_RY], axis, placement, q_lo=-np.ones(3), q_hi=np.ones(3), name="slider3")


def test_exact_centres_cross_a_voxel_face():
    """the grid of test_exact_centres_on_faces_boundary_and_outside (every face a binary fraction).  A sphere on the slider starts exactly
    on the face x = 1 of its row of voxels and ends exactly on the face x = 2, one edge further; a sphere on the universe sits on a face
    and stays.  The one occupied voxel lies at x = 3 of the moving sphere's row, so that the clearance falls along the segment and the
    minimum is the last sample's: there floor() puts the centre into voxel x = 2, whose value is G = 1: (h / 2) 1 - h / 2 - r = -r; the
    voxel at x = 1 on the other side of the face would give (h / 2) 3 - h / 2 - r = h - r"""
    model = _slider()
    occ = np.zeros((4, 4, 4), dtype=np.uint8)
    occ[2, 1, 3] = 1
    grid = GN.Grid(occ, (-0.25, 0.5, -1.0), 0.25)
    o, h, r = grid.origin, grid.h, 0.03125
    start, fixed = o + h * np.array([1.0, 1.5, 2.5]), o + h * np.array([1.0, 3.0, 0.5])
    links = np.array([1, 0], dtype=np.int32)
    spheres = np.array([[start[0], start[1], start[2], r], [fixed[0], fixed[1], fixed[2], r]])
    qa, dv = np.zeros((1, 3)), np.array([[h, 0.0, 0.0]])
    kw = dict(margin=-1.0, tol=GC.TOL, max_evals=8)
    want = GN.advance(model, qa, dv, links, spheres, grid=grid, **kw)
    cen = MN.centres(model, np.concatenate([qa, qa + dv]), links, spheres)
    assert np.array_equal(cen[0, 0], start) and np.array_equal(cen[1, 0], start + [h, 0.0, 0.0]) and np.array_equal(cen[:, 1], [fixed, fixed])
    assert want["near"][0] and GN.near_face(cen[0], grid) and GN.near_face(cen[1], grid)      # the face-proximity flag is set: and the row is compared all the same
    vox = (2 * 4 + 1) * 4 + 2
    assert want["status"][0] == FREE and want["evals"][0] == 2 and tuple(want["witness"][0]) == (GN.WORLD_GRID, 0, vox)
    assert want["min_sampled"][0] == -r and want["s_at_min"][0] == 1.0
    s = TC._open(model, np.zeros((1, 3)))
    s.set_collision_spheres(links, spheres)
    TG._set(s, grid)
    got = s.motion_clearance(qa, dv=dv, **kw)
    print("grid_measured edge exact centres: status %d evals %d min_sampled %.17g witness %s" % (got["status"][0], got["evals"][0], got["min_sampled"][0], got["witness"][0].tolist()))
    assert got["status"][0] == FREE and got["evals"][0] == 2 and tuple(got["witness"][0]) == (capi.CLR_WORLD_GRID, 0, vox)
    assert got["min_sampled"][0] == -r and got["s_at_min"][0] == 1.0 and got["s_free"][0] == 1.0
    # the other way: from the face x = 2 back to the face x = 1.  The minimum is the first sample's, in voxel x = 2 again
    back = s.motion_clearance(qa + dv, dv=-dv, **kw)
    want = GN.advance(model, qa + dv, -dv, links, spheres, grid=grid, **kw)
    assert want["near"][0] and tuple(want["witness"][0]) == (GN.WORLD_GRID, 0, vox) and want["s_at_min"][0] == 0.0
    assert all(np.array_equal(back[k], want[k]) for k in ("status", "evals", "witness", "min_sampled", "s_at_min", "s_free"))
    s.close()


def _four(s, c):
    """the four entry points on a few rows of panda7's cases, every output"""
    m, sc, pc, bc = (f("panda7") for f in (GC.motion_case, GC.shortcut_case, GC.plan_case, GC.blend_case))
    out = {"motion " + k: v for k, v in s.motion_clearance(m["qa"][:9], dv=m["dv"][:9], **m["kw"]).items()}
    out.update({"path " + k: v for k, v in s.path_clearance(sc["paths"][:3], margin=sc["margin"], tol=GC.TOL, max_evals=GC.MAX_EVALS).items()})
    out.update({"shortcut " + k: v for k, v in s.shortcut_paths(sc["paths"][:5], **sc["kw"]).items()})
    out.update({"plan " + k: v for k, v in TPL._plan(s, pc, start=pc["start"][:5], goal=pc["goal"][:5], T=GC.T_PLAN, max_iters=6).items()})
    out.update({"blend " + k: v for k, v in s.blend_paths(bc["paths"][:3], v_max=bc["v_max"], a_max=bc["a_max"], max_samples=64, **bc["kw"]).items()})
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f")]


def test_a_grid_replaced_and_cleared_answers_as_a_fresh_handle():
    """one handle whose grid is replaced by one of other dimensions, origin and edge, then by the first again, then cleared; after each
    change the four entry points answer as a handle that never had another world, bit for bit"""
    c = GC.world("panda7")
    first = c["grid"]
    second = GN.Grid(GN.random_occupancy((9, 30, 14), 0.02, 1611), (-0.4, -0.9, -0.1), 0.07)
    used = _open(c, grid=None)
    answers = []
    for grid in (first, second, first, None):
        if grid is None:
            used.set_collision_grid(None)
        else:
            TG._set(used, grid)
        fresh = _open(c, grid=grid)
        a, b = _four(used, c), _four(fresh, c)
        fresh.close()
        assert _same(a, b) == [], (None if grid is None else grid.occ.shape, _same(a, b))
        answers.append(a)
    used.close()
    # ... and the three worlds do differ from one another
    for k in ("motion min_sampled", "path min_sampled", "plan evals"):
        assert len({answers[i][k].tobytes() for i in (0, 1, 3)}) == 3, k
    assert _same(answers[0], answers[2]) == []


def test_rows_that_are_not_finite_with_a_grid_set():
    m, sc, pc, bc = (f("panda7") for f in (GC.motion_case, GC.shortcut_case, GC.plan_case, GC.blend_case))
    model = m["model"]
    s = _open(m)
    # a segment
    full = s.motion_clearance(m["qa"], dv=m["dv"], **m["kw"])
    qn, dn = m["qa"].copy(), m["dv"].copy()
    qn[2, 3], dn[64, model.nv - 1] = np.nan, np.inf
    bad = s.motion_clearance(qn, dv=dn, **m["kw"])
    for i in (2, 64):
        assert bad["status"][i] == INVALID and bad["evals"][i] == 0 and tuple(bad["witness"][i]) == (CN.NONE, -1, -1)
        assert np.isnan([bad["s_free"][i], bad["min_sampled"][i], bad["s_at_min"][i]]).all()
    keep = ~np.isin(np.arange(m["qa"].shape[0]), (2, 64))
    assert TM._same({k: v[keep] for k, v in bad.items()}, {k: v[keep] for k, v in full.items()})
    # a waypoint of a path: the segments that touch it under path_clearance, the path under shortcut_paths and blend_paths
    paths = sc["paths"].copy()
    mkw = dict(margin=sc["margin"], tol=GC.TOL, max_evals=GC.MAX_EVALS)
    ok = s.path_clearance(paths, **mkw)
    cut = s.shortcut_paths(paths, **sc["kw"])
    paths[1, 2, 0] = np.nan
    chk = s.path_clearance(paths, **mkw)
    assert chk["status"][1].tolist()[1:3] == [INVALID, INVALID] and np.isnan(chk["min_sampled"][1, 1:3]).all() and np.all(chk["witness"][1, 1:3] == (CN.NONE, -1, -1))
    touched = np.zeros(chk["status"].shape, dtype=bool)
    touched[1, 1:3] = True
    assert all(np.array_equal(chk[k][~touched], ok[k][~touched]) for k in ok)
    got = s.shortcut_paths(paths, **sc["kw"])
    others = np.arange(sc["B"]) != 1
    assert TS._same(TS._rows(got, others), TS._rows(cut, others)) and np.isnan(got["length_in"][1])
    ref = SN.shortcut(model, paths[:2], sc["links"], sc["spheres"], sc["ws"], sc["wb"], sc["pairs"], grid=sc["grid"], **sc["kw"])
    assert ref["near"][1] or got["invalid"][1] == ref["invalid"][1] == sum(2 in (i, j) for i, j, _ in ref["segments"][1])
    bp = bc["paths"].copy()
    bkw = dict(v_max=bc["v_max"], a_max=bc["a_max"], max_samples=64, **bc["kw"])
    whole = s.blend_paths(bp, **bkw)
    bp[1, 3, 1] = np.nan
    part = s.blend_paths(bp, **bkw)
    others = np.arange(bc["B"]) != 1
    assert part["flags"][1] == capi.BLEND_INVALID and all(np.isnan(part[k][1]).all() for k in TBL.FLOATS) and part["taken"][1] == 0
    assert TBL._same(TBL._rows(part, others), TBL._rows(whole, others))
    # a start and a goal
    start, goal = pc["start"].copy(), pc["goal"].copy()
    plan = TPL._plan(s, pc, T=GC.T_PLAN)
    start[3, 1], goal[7, 0] = np.nan, np.inf
    inv = TPL._plan(s, pc, start=start, goal=goal, T=GC.T_PLAN)
    others = ~np.isin(np.arange(pc["B"]), (3, 7))
    assert TPL._same(TPL._rows(inv, others), TPL._rows(plan, others))
    for b in (3, 7):
        assert inv["status"][b] == capi.PLAN_INVALID and all(np.all(inv[k][b] == 0) for k in TPL.FIELDS[1:]) and np.isnan(inv["q_path"][b]).all()
    s.close()

