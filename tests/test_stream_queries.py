"""The query entry points on a caller's stream behind pending work (include/loik_amd.h at loikb_set_stream: the contract): kinematics,
Jacobians and dexterity, clearance, its gradient and the avoidance box, difference, the certified motion checks, shortcutting, path
length, retiming, blending and planning, and the voxel world set from a device array.

One sequence of calls per robot, run twice by stream_harness.run_both: on the null stream with host arrays, and on a non-blocking
stream with a gate in front of every call, every per-row input (q, dv, the paths, n_waypoints, the occupancy) in a device array that
holds the neighbouring row's data until a copy queued behind the gate, every output in a poisoned device array read back right after
the call.  Byte for byte; both runs hand the same out= layout to the bindings, so what a call leaves unwritten compares as well.
The robots: panda7 (the LDS builds) and tree330 (the slab builds), as grid_cases.world has them; the paths, limits and reaches are
drawn by the builders of test_shortcut, test_blend_numpy and test_retime_numpy; the margins are quantiles of the handle's own
clearance at the inputs, taken on the null-stream run."""
import ctypes as C

import numpy as np
import pytest

import grid_cases as GC
import pose_limits_numpy as PL
import pose_numpy as P
import stream_harness as H
import test_avoid_box as TA
import test_blend_numpy as TB
import test_clearance as TC
import test_motion_clearance as TM
import test_plan_numpy as TP
import test_retime_numpy as TR
import test_shortcut as TS
from loik_amd import capi

pytestmark = pytest.mark.gpu

_ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
F, I = np.float64, np.int32
TOL, EVALS, S_ROWS = 1e-3, 24, 64


def _p(o):
    """the (void*, out_flags) of an output of Run.get_n: a host array or a device array"""
    if isinstance(o, np.ndarray):
        return o.ctypes.data_as(C.c_void_p), 0
    return C.c_void_p(o.data_ptr()), capi.OUT_DEVICE


def _sequence(name):
    c = GC.world(name)
    robot = name
    model, q, grid = c["model"], np.ascontiguousarray(c["q"]), c["grid"]
    n, nq, nv, ns = q.shape[0], model.nq, model.nv, len(c["links"])
    B = min(GC.BATCH[name][0], n)
    rng = np.random.default_rng(77)
    links = np.array([model.njoints - 1, 1, model.njoints - 1], dtype=I)
    frames = np.ascontiguousarray(np.stack([np.r_[np.eye(3).reshape(9), 0.1, -0.2, 0.3]] * 3))
    rows = np.array([0x07, 0x38, 0x3f], dtype=I)
    dv = TM.SIZE[robot] * rng.uniform(-1.0, 1.0, size=(n, nv))
    paths = TS.make_paths(model, q[:B], TM.SIZE[robot], TS.T_PATH, np.random.default_rng(78))
    bpaths = TB.make_paths(model, q[:B], TM.SIZE[robot], TS.T_PATH, np.random.default_rng(79))
    T = paths.shape[1]
    nw = (T - np.arange(B) % 3).astype(I)
    v_max, a_max = TR.limits(robot, nv)
    near = 0.03 * rng.uniform(-1.0, 1.0, size=(B, nv))
    memo = dict(goal=np.ascontiguousarray(np.stack([P.integrate(model, a, d) for a, d in zip(q[:B], near)])))
    L = capi.lib()

    def raw(fn):
        def call(outs):
            p, f = _p(outs[0])
            rc = fn(p, f)
            assert rc == 0, L.loikb_last_error()
        return call

    def sequence(run, s):
        occ = np.ascontiguousarray(np.asarray(grid.occ) != 0, dtype=np.uint8)
        run.do(s.set_collision_spheres, c["links"], c["spheres"])
        run.do(s.set_collision_world, c["ws"], c["wb"])
        run.do(s.set_self_collision, True)
        # ---- the resident q: kinematics, Jacobians, dexterity
        run.get_n(["fk"], raw(lambda p, f: L.loikb_forward_kinematics(s.h, links.ctypes.data_as(_ip), 3, p, f)), [((n, 3, 12), F)])
        run.get_n(["frames"], raw(lambda p, f: L.loikb_frame_placements(s.h, links.ctypes.data_as(_ip), frames.ctypes.data_as(_dp), 3, p, f)), [((n, 3, 12), F)])
        prm = capi.DexterityParams(0.25, 0)
        run.get_n(["dexterity"], raw(lambda p, f: L.loikb_frame_dexterity(s.h, links.ctypes.data_as(_ip), frames.ctypes.data_as(_dp), rows.ctypes.data_as(_ip), 3,
                                                                          C.byref(prm), p, f)), [((n, 3, capi.DEX_N), F)])
        run.get_n(["jacobians"], lambda o: s.frame_jacobians(links, frames, "local_world_aligned", out=o[0]), [((n, 3, 6, nv), F)])
        # ---- clearance of the resident q and of a q on the device, the gradient, the box
        run.get_n(["clr resident", "clr resident wit"], lambda o: s.clearance(None, out=tuple(o)), [((n, 3), F), ((n, 3), I)])
        # (every run.inp before the call it is for: Run.do stages what is pending behind the gate it queues)
        d = run.inp(q)
        run.get_n(["clr", "clr wit"], lambda o: s.clearance(d, out=tuple(o)), [((n, 3), F), ((n, 3), I)])
        if ns <= capi.AVOID_MAX_SPHERES:   # (tree330's 330 spheres are more than the gradient and the box take: panda7 alone runs them)
            d = run.inp(q)
            run.get_n(["grad min", "grad wit", "grad"], lambda o: s.clearance_gradient(d, out=tuple(o)), [((n, 3), F), ((n, 3), I), ((n, nv), F)])
            d = run.inp(q)
            run.get_n(["box lo", "box hi", "box pairs", "box partner"],
                      lambda o: s.avoidance_box(d, TA.DT, -np.inf, np.inf, out=tuple(o), **TA.PRM),
                      [((n, nv), F), ((n, nv), F), ((n, ns, 2), F), ((n, ns, 2), I)])
        # ---- the voxel world from an occupancy on the device (after the gradient and the box: a grid's bound has no gradient, and the
        #      two refuse a handle that has one); everything below reads it
        run.do(s.set_collision_grid, run.inp(occ, np.uint8), grid.origin, grid.h)
        g = run.do(s.collision_grid)
        run.put("grid G", g["G"])
        run.put("grid dims", g["dims"])
        nx, ny, nz = (int(x) for x in grid.occ.shape[::-1])

        def field(outs):   # (loikb_collision_get_world_grid has a copy and a synchronisation of its own; 1 = a grid is set)
            p, f = _p(outs[0])
            assert L.loikb_collision_get_world_grid(s.h, None, None, None, p, f) == 1, L.loikb_last_error()
        run.get_n(["grid G raw"], field, [((nz, ny, nx), np.uint32)])
        d = run.inp(q)
        run.get_n(["clr grid", "clr grid wit"], lambda o: s.clearance(d, out=tuple(o)), [((n, 3), F), ((n, 3), I)])
        # ---- motions
        qb = np.roll(q, 1, axis=0)
        d, e = run.inp(q), run.inp(qb)
        run.get_n(["difference"], lambda o: s.difference(d, e, out=o[0]), [((n, nv), F)])
        if not run.gated:
            at = s.clearance(np.concatenate([q, paths.reshape(-1, nq), bpaths.reshape(-1, nq)]))["min"]
            memo["motion"] = float(np.quantile(at[:n], GC.Q_MOTION)) - 2.0 * TOL
            memo["paths"] = float(np.quantile(at[n:n + B * T], GC.Q_PATHS))
            memo["blend"] = float(np.quantile(at[n + B * T:], GC.Q_BLEND))
        mkw = dict(margin=memo["motion"], tol=TOL, max_evals=EVALS)
        d, e = run.inp(q), run.inp(dv)
        run.get_n(["motion val", "motion info"], lambda o: s.motion_clearance(d, dv=e, out=tuple(o), **mkw), [((n, 3), F), ((n, 5), I)])
        d, e = run.inp(q), run.inp(qb)
        run.get_n(["motion qb val", "motion qb info"], lambda o: s.motion_clearance(d, qb=e, out=tuple(o), **mkw), [((n, 3), F), ((n, 5), I)])
        pkw = dict(margin=memo["paths"], tol=TOL, max_evals=EVALS)
        d = run.inp(paths)
        run.get_n(["path clr val", "path clr info"], lambda o: s.path_clearance(d, out=tuple(o), **pkw), [((B * (T - 1), 3), F), ((B * (T - 1), 5), I)])
        # ---- paths: n_waypoints on the device beside the path
        d, e = run.inp(paths), run.inp(nw, I)
        run.get_n(["shortcut path", "shortcut keep", "shortcut info", "shortcut val"],
                  lambda o: s.shortcut_paths(d, e, rounds=4, seed=TS.SEED, out=tuple(o), **pkw),
                  [((B, T, nq), F), ((B, T), I), ((B, 6), I), ((B, 2), F)])
        d, e = run.inp(paths), run.inp(nw, I)
        run.get_n(["length"], lambda o: s.path_length(d, e, out=o[0]), [((B,), F)])
        d, e = run.inp(paths), run.inp(nw, I)
        run.get_n(["retime traj", "retime vel", "retime seg", "retime dur", "retime info"],
                  lambda o: s.retime_paths(d, v_max, a_max, TB.DT, n_waypoints=e, max_samples=S_ROWS, out=tuple(o)),
                  [((B, S_ROWS, nq), F), ((B, S_ROWS, nv), F), ((B, T - 1, 4), F), ((B,), F), ((B, 4), I)])
        d, e = run.inp(bpaths), run.inp(nw, I)
        run.get_n(["blend traj", "blend vel", "blend dur", "blend info", "blend corner", "blend cinfo", "blend piece"],
                  lambda o: s.blend_paths(d, v_max, a_max, TB.DT, TB.reach_of(robot, nv), n_waypoints=e, max_samples=S_ROWS,
                                          margin=memo["blend"], tol=TOL, max_evals=EVALS, max_tries=TB.MAX_TRIES, out=tuple(o)),
                  [((B, S_ROWS, nq), F), ((B, S_ROWS, nv), F), ((B,), F), ((B, 4), I), ((B, T - 2, 5), F), ((B, T - 2, 6), I), ((B, 2 * T - 3, 4), F)])
        # ---- planning between configurations a short way apart (test_plan's slab parameters on both robots: a few iterations)
        ends, qi = np.concatenate([q[:B], memo["goal"]]), PL.limit_q_index(model)
        lo, hi = np.full(nv, -np.inf), np.full(nv, np.inf)
        lo[qi >= 0], hi[qi >= 0] = ends[:, qi[qi >= 0]].min(axis=0) - 0.5, ends[:, qi[qi >= 0]].max(axis=0) + 0.5
        d, e = run.inp(q[:B]), run.inp(memo["goal"])
        run.get_n(["plan path", "plan info", "plan length"],
                  lambda o: s.plan_paths(d, e, lo, hi, TP.T_PLAN, step=0.05, max_iters=4, max_nodes=64, seed=TS.SEED,
                                         margin=-1.0, tol=TOL, max_evals=EVALS, out=tuple(o)),
                  [((B, TP.T_PLAN, nq), F), ((B, 8), I), ((B,), F)])
    return c, sequence


@pytest.mark.parametrize("name", ["panda7", GC.SLAB])
def test_queries_behind_a_gate(name):
    c, sequence = _sequence(name)
    ref, gates = H.run_both(lambda: TC._open(c["model"], c["q"]), sequence, what=name)
    assert gates >= 20
    # the inputs are worth running: the grid was built, segments end in more than one way, shortcuts were tried, samples were written
    assert (ref["grid G"] != ref["grid G"].flat[0]).any() and ref["grid G raw"].tobytes() == ref["grid G"].tobytes()
    assert len(set(ref["motion info"][:, 0].tolist())) > 1 or name == GC.SLAB, ref["motion info"][:, 0]
    assert ref["shortcut info"][:, 1].sum() > 0
    assert (ref["retime info"][:, 0] > 1).all() and np.isfinite(ref["retime dur"]).all()
    assert np.isfinite(ref["length"]).all() and np.isfinite(ref["jacobians"]).all() and np.isfinite(ref["dexterity"]).all()
