"""GPU: the motion layer against a voxel world (include/loik_amd_grid.h): a one-voxel-thick wall between two free configurations, the
advancement against tests/grid_numpy.py, what FREE certifies against the exact distance to the union of the cubes, planning around the
wall, shortcuts, blends past an occupied voxel, and the collision-aware multi-start.  The robot, the sphere and the segment are
test_plan_numpy.wall_case's: panda7, one sphere of radius 0.01 on link 7."""
import numpy as np
import pytest

from loik_amd import capi

import blend_numpy as BN
import grid_numpy as GN
import motion_numpy as MN
import test_clearance as TC
import test_plan_numpy as TP

pytestmark = pytest.mark.gpu

BOUND = TC.BOUND
TOL, H, N = 1e-3, 0.01, 21
_W = {}


def _centres(w, q):
    return MN.centres(w["model"], np.atleast_2d(q), w["links"], w["spheres"])[:, 0]


def wall():
    """wall_case with a grid of 21^3 voxels of 1 cm about the sphere's centre at the middle of the segment A -> Bq: the wall is the slab
    of voxels across the axis the centre travels along there, one voxel thick, with a slot six voxels wide at one side"""
    if not _W:
        w = dict(TP.wall_case())
        A, dv = w["A"], w["Bq"] - w["A"]
        c = _centres(w, MN.interpolate_many(w["model"], A, dv, [0.4, 0.5, 0.6]))
        ax = int(np.argmax(np.abs(c[2] - c[0])))
        occ = np.zeros((N, N, N), dtype=np.uint8)
        sl = [slice(None)] * 3                      # [z][y][x]
        sl[2 - ax] = slice(N // 2, N // 2 + 1)
        occ[tuple(sl)] = 1
        sl[2 - (ax + 1) % 3] = slice(0, 6)
        occ[tuple(sl)] = 0
        w["dv"] = dv
        w["grid"] = GN.Grid(occ, c[1] - 0.5 * N * H, H)
        w["cubes"] = GN.cubes(w["grid"])
        _W.update(w)
    return _W


def _open(w, grid=True, q=None):
    s = TC._open(w["model"], np.stack([w["A"], w["Bq"]]) if q is None else q)
    s.set_collision_spheres(w["links"], w["spheres"])
    if grid:
        g = w["grid"] if grid is True else grid
        s.set_collision_grid(g.occ, g.origin, g.h)
    return s


def _exact(w, q, grid=None, cubes=None):
    return GN.exact_clearance(w["model"], q, w["links"], w["spheres"], w["grid"] if grid is None else grid, w["cubes"] if grid is None else cubes)


def _voxel_grid(p):
    """one occupied voxel, the middle one of 21^3, centred at p"""
    occ = np.zeros((N, N, N), dtype=np.uint8)
    occ[N // 2, N // 2, N // 2] = 1
    return GN.Grid(occ, np.asarray(p) - 0.5 * N * H, H)


# ---- 1. the wall blocks, as numpy says ------------------------------------------------------------------------------------------------------
def test_a_wall_between_two_free_configurations_blocks():
    w = wall()
    model, A, Bq, dv = w["model"], w["A"], w["Bq"], w["dv"]
    s = _open(w)
    ends = s.clearance(np.stack([A, Bq]))
    assert np.all(ends["min"] > 0.1) and np.all(ends["witness"][:, 0] == capi.CLR_WORLD_GRID)
    # the whole segment, its first third (free) and the piece through the wall
    qa = np.stack([A, A, MN.interpolate(model, A, dv, 0.4)])
    dvs = np.stack([dv, 0.3 * dv, 0.2 * dv])
    got = s.motion_clearance(qa, dv=dvs, margin=0.0, tol=TOL, max_evals=256)
    want = GN.advance(model, qa, dvs, w["links"], w["spheres"], grid=w["grid"], margin=0.0, tol=TOL, max_evals=256)
    print("grid_measured wall: status %s evals %s s_free %s min_sampled %s" % (got["status"].tolist(), got["evals"].tolist(), got["s_free"].tolist(), got["min_sampled"].tolist()))
    assert not want["near"].any()
    assert got["status"].tolist() == [MN.BLOCKED, MN.FREE, MN.BLOCKED] == want["status"].tolist()
    assert np.array_equal(got["evals"], want["evals"]) and np.array_equal(got["witness"], want["witness"])
    scale = 1.0 + float(np.abs(_centres(w, np.stack([A, Bq]))).max())
    for k in ("min_sampled", "s_free", "s_at_min"):
        assert np.all(np.abs(got[k] - want[k]) <= BOUND * scale), (k, got[k], want[k])
    assert np.all(got["witness"][:, 0] == capi.CLR_WORLD_GRID)
    # what FREE certifies: 2049 samples of the free segment are clear of the union of the cubes
    q = MN.interpolate_many(model, qa[1], dvs[1], np.linspace(0.0, 1.0, 2049))
    exact = _exact(w, q)
    print("grid_measured wall: exact clearance over the free segment %.4f .. %.4f, device min_sampled %.4f" % (exact.min(), exact.max(), got["min_sampled"][1]))
    assert exact.min() >= 0.0      # (>= margin: what FREE promises; min_sampled itself bounds the sampled points only)
    # without the grid the segment is free
    s.set_collision_grid(None)
    assert s.motion_clearance(A[None], dv=dv[None], margin=0.0, tol=TOL)["status"][0] == MN.FREE
    s.close()


# ---- 2. planning around it, shortcuts ---------------------------------------------------------------------------------------------------------
def test_plan_goes_around_the_wall_and_shortcuts_stay_certified():
    w = wall()
    model, A, Bq = w["model"], w["A"], w["Bq"]
    s = _open(w)
    T = 32
    kw = dict(step=0.5, max_iters=64, max_nodes=64, seed=1, margin=0.0, tol=TOL)
    got = s.plan_paths(A[None], Bq[None], w["lo"], w["hi"], T, **kw)
    print("grid_measured plan: status %d L %d iterations %d edges %d free %d evals %d" % tuple(
        int(got[k][0]) for k in ("status", "n_waypoints", "iterations", "edges_checked", "edges_free", "evals")))
    assert got["status"][0] == capi.PLAN_FOUND and got["n_waypoints"][0] > 2
    L = int(got["n_waypoints"][0])
    path = got["q_path"]
    assert np.array_equal(path[0, 0], A) and np.array_equal(path[0, L - 1], Bq)
    # loikb_motion_clearance_path repeats the planner's checks.  The planner reports one total of evals per query and no status or evals
    # per edge, so a comparison edge by edge with the planner is not possible (test_plan._check_self has the same limit): what is
    # checked is that every segment is FREE, that the check gives the same bits twice, and that the evals of the path's L - 1 edges
    # fit in the planner's total, which counts them and the rejected edges
    chk = s.path_clearance(path, margin=0.0, tol=TOL)
    again = s.path_clearance(path, margin=0.0, tol=TOL)
    assert np.all(chk["status"] == MN.FREE) and all(np.array_equal(chk[k], again[k]) for k in chk)
    assert 0 < int(chk["evals"].reshape(-1)[:L - 1].sum()) <= int(got["evals"][0])
    # ... and each is free of the cubes where it is sampled densely
    for k in range(L - 1):
        dv = MN.difference(model, path[0, k][None], path[0, k + 1][None])[0]
        assert _exact(w, MN.interpolate_many(model, path[0, k], dv, np.linspace(0.0, 1.0, 129))).min() >= 0.0, k
    # shortcutting never outputs a segment that motion_clearance does not certify
    cut = s.shortcut_paths(path, n_waypoints=got["n_waypoints"].astype(np.int32), rounds=32, seed=3, margin=0.0, tol=TOL)
    Lc = int(cut["n_waypoints"][0])
    assert 3 <= Lc <= L and cut["invalid"][0] == 0
    seg = s.motion_clearance(cut["q_path"][0, :Lc - 1], qb=np.ascontiguousarray(cut["q_path"][0, 1:Lc]), margin=0.0, tol=TOL)
    assert np.all(seg["status"] == MN.FREE), seg["status"]
    # the same query without the grid is the direct segment
    s.set_collision_grid(None)
    direct = s.plan_paths(A[None], Bq[None], w["lo"], w["hi"], T, **kw)
    assert direct["status"][0] == capi.PLAN_FOUND and direct["n_waypoints"][0] == 2
    s.close()


# ---- 3. blends --------------------------------------------------------------------------------------------------------------------------------
def test_a_voxel_inside_a_corner_stops_the_blend():
    w = wall()
    model, A = w["model"], w["A"]
    dva = 0.5 * w["dv"]
    dvb = dva * np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0])
    M = A + dva
    path = np.stack([A, M, M + dvb])[None]
    reach = 0.3
    l = min(reach, 0.5 * BN.norm_of(dva), 0.5 * BN.norm_of(dvb))
    P0, P2 = -(l / BN.norm_of(dva)) * dva, (l / BN.norm_of(dvb)) * dvb
    mid, corner = _centres(w, BN.curve_point(model, M, P0, P2, 0.5))[0], _centres(w, M)[0]
    kw = dict(v_max=np.full(model.nv, 1.0), a_max=np.full(model.nv, 2.0), dt=0.01, reach=reach, margin=0.0, tol=TOL, max_tries=1)
    s = _open(w, grid=False, q=path[0, :2])
    free = s.blend_paths(path, **kw)
    assert free["corner_info"][0, 0, 0] == capi.BLEND_TAKEN and tuple(free["corner_info"][0, 0, 3:]) == (capi.CLR_NONE, -1, -1)
    # a voxel where the sphere passes at the middle of the curve: the legs stay free, the blend does not
    inside = _voxel_grid(mid)
    s.set_collision_grid(inside.occ, inside.origin, inside.h)
    assert np.all(s.path_clearance(path, margin=0.0, tol=TOL)["status"].reshape(-1)[:2] == MN.FREE)
    got = s.blend_paths(path, **kw)
    print("grid_measured blend: voxel inside the corner: status %d, min_sampled %.4f, witness %s" % (
        got["corner_info"][0, 0, 0], got["corner"][0, 0, 4], got["corner_info"][0, 0, 3:].tolist()))
    assert got["corner_info"][0, 0, 0] == capi.BLEND_BLOCKED and got["taken"][0] == 0
    assert got["corner_info"][0, 0, 3] == capi.CLR_WORLD_GRID and got["corner_info"][0, 0, 4] == 0 and 0 <= got["corner_info"][0, 0, 5] < N ** 3
    assert got["duration"][0] >= free["duration"][0]
    # a voxel beyond the corner, on its outer side: the blend is taken, and every sample of the trajectory is clear of the cube
    outside = _voxel_grid(corner + 1.5 * (corner - mid))
    s.set_collision_grid(outside.occ, outside.origin, outside.h)
    got = s.blend_paths(path, **kw)
    assert got["corner_info"][0, 0, 0] == capi.BLEND_TAKEN and got["corner_info"][0, 0, 3] == capi.CLR_WORLD_GRID
    n = int(got["n_samples"][0])
    exact = _exact(w, got["q_traj"][0, :n], outside, GN.cubes(outside))
    print("grid_measured blend: voxel outside the corner: min_sampled %.4f, exact clearance over %d samples %.4f .. %.4f" % (
        got["corner"][0, 0, 4], n, exact.min(), exact.max()))
    assert exact.min() >= 0.0      # (>= margin: what TAKEN promises)
    s.close()


# ---- 4. the collision-aware multi-start ---------------------------------------------------------------------------------------------------------
def test_the_multistart_rejects_a_seed_inside_a_voxel():
    import test_clearance_multistart as TCM
    w = TCM._workload()
    s = TCM._open(w)
    plain = TCM._run(s, w, pick="first")
    assert plain["goal_status"][0] == capi.MS_GOAL_REACHED
    status, err, q = TCM._device_state(s)
    b0 = int(plain["winner"][0])
    elbow = MN.centres(w["model"], q[b0:b0 + 1], w["lk"], w["sph"])[0, TCM.ELBOW]
    grid = _voxel_grid(elbow)                 # the elbow sphere's centre of the unlatched winner lies in the occupied voxel
    s.set_collision_grid(grid.occ, grid.origin, grid.h)
    clr = s.clearance(q)
    assert clr["min"][b0] < 0.0 and tuple(clr["witness"][b0][:2]) == (capi.CLR_WORLD_GRID, TCM.ELBOW)
    s.set_multistart_clearance(TCM.MARGIN)
    out = TCM._run(s, w, pick="first")
    inst = s.multistart_clearance_get("instance")
    print("grid_measured multistart: goal 0 winner %d -> %d, goal_status %s, clearance %s" % (b0, int(out["winner"][0]), out["goal_status"].tolist(), out["clearance"].tolist()))
    assert inst[b0] < TCM.MARGIN
    assert out["winner"][0] != b0 or out["goal_status"][0] == capi.MS_GOAL_IN_COLLISION
    if out["goal_status"][0] == capi.MS_GOAL_REACHED:
        assert out["clearance"][0] >= TCM.MARGIN
    s.close()
