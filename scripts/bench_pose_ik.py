"""Global IK from many seeds (include/loik_amd_pose.h): B seeds around T targets, each target the placement of a random configuration
within the model's limits, every seed that configuration perturbed.  Prints one JSON line per run:
  device : loikb_solve_pose -- the whole loop on the device
  host   : the same loop through the existing entry points, the pattern of scripts/bench_outer_loop.py: FK and log6 on the host
           (numpy, vectorised), the tailored Solve with the host's q and b every step, z read back, q integrated on the host
Reported: poses reached per second, mean / p99 steps of the reached, ms per step split into the inner solve and the rest
(re-target, b, integrate, read-backs).

  python scripts/bench_pose_ik.py [--workload talos32|panda7|all] [--batch 65536] [--targets 1024] [--steps 30] [--tol 1e-4]
                                  [--no-host] [--step-control]
--step-control: the device loop with the default step control of include/loik_amd_step.h (the host loop has none: use --no-host)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import loik_amd
from loik_amd import workloads as W

WORKLOADS = {"talos32": "arm_left_7_joint", "panda7": "panda_joint7"}


def fk(model, q, link):
    """world placement of `link` for configurations q [B][nq] of a model of 1-DoF joints: (R [B,3,3], t [B,3])"""
    path, i = [], int(link)
    while i > 0:
        path.append(i)
        i = int(model.parents[i])
    B = q.shape[0]
    R, t = np.broadcast_to(np.eye(3), (B, 3, 3)).copy(), np.zeros((B, 3))
    for i in reversed(path):
        P = model.placement[i]
        Rp, tp = P[:9].reshape(3, 3), P[9:]
        jt = int(model.jtype[i])
        if jt in (W.J_RX, W.J_RY, W.J_RZ, W.J_RU):
            Rl, tl = Rp[None] @ W._rot(jt, model.axis[i], q[:, int(model.idx_q[i])]), np.broadcast_to(tp, (B, 3))
        else:
            a = np.asarray(model.axis[i], dtype=float) if jt == W.J_PU else np.eye(3)[jt - W.J_PX]
            Rl, tl = np.broadcast_to(Rp, (B, 3, 3)), tp[None] + q[:, int(model.idx_q[i]), None] * (Rp @ a)[None]
        t = t + np.einsum("bij,bj->bi", R, tl)
        R = R @ Rl
    return R, t


def log6(R, p):
    """batched pinocchio::log6, the branches of loik_pose.hpp: [B,6]"""
    vee = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
    s = 0.5 * np.linalg.norm(vee, axis=1)
    c = 0.5 * (np.trace(R, axis1=1, axis2=2) - 1.0)
    th = np.arctan2(s, c)
    t2 = th * th
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(th < 1e-4, 0.5 * (1 + t2 / 6 + 7 * t2 * t2 / 360), 0.5 * th / s)
    w = f[:, None] * vee
    near = np.flatnonzero(c < -0.8)
    for b in near:   # (theta -> pi: the axis from the symmetric part; rare for these workloads)
        k = int(np.argmax(np.diag(R[b])))
        omc = 1.0 - c[b]
        a = np.empty(3)
        a[k] = np.sqrt(max(0.0, (R[b, k, k] - c[b]) / omc))
        for j in range(3):
            if j != k:
                a[j] = 0.5 * (R[b, k, j] + R[b, j, k]) / (omc * a[k])
        w[b] = (-th[b] if a @ vee[b] < 0 else th[b]) * a
    t2 = np.sum(w * w, axis=1)
    th = np.sqrt(t2)
    with np.errstate(divide="ignore", invalid="ignore"):
        beta = np.where(th < 1e-3, 1.0 / 12 + t2 / 720 + t2 * t2 / 30240, (1 - 0.5 * th / np.tan(0.5 * th)) / t2)
    wp = np.cross(w, p)
    return np.concatenate([p - 0.5 * wp + beta[:, None] * np.cross(w, wp), w], axis=1)


def make(model, link, B, T, seed, spread):
    rng = np.random.default_rng(seed)
    q_t = model.random_configurations(rng, T)
    R, t = fk(model, q_t, link)
    tgt = np.concatenate([R.reshape(T, 9), t], axis=1)
    which = np.arange(B) % T
    q0 = np.clip(q_t[which] + spread * rng.normal(size=(B, model.nq)), model.q_lo, model.q_hi)
    return q0, tgt[which][:, None, :]


def summary(kind, name, B, T, reached, steps, total_s, n_steps, solve_ms, other_ms, args):
    st = steps[reached]
    return dict(config="pose IK %s B=%d around %d targets, tol_pose %g, max_steps %d" % (name, B, T, args.tol, args.steps), loop=kind,
                reached_fraction=float(reached.mean()), poses_reached_per_s=float(reached.sum() / total_s), wall_s=round(total_s, 4),
                steps_run=int(n_steps), mean_steps=float(st.mean()) if st.size else None,
                p99_steps=float(np.percentile(st, 99)) if st.size else None,
                ms_per_step_solve=round(solve_ms / max(n_steps, 1), 3), ms_per_step_other=round(other_ms / max(n_steps, 1), 3))


def run_device(model, link, q0, tgt, prm, args):
    B = q0.shape[0]
    s = loik_amd.BatchedLoik(model, B, **prm)
    s.SolveInit(q0, np.eye(6), np.zeros(6), np.array([link], dtype=np.int32), np.eye(6)[None], np.zeros((B, 1, 6)),
                -args.bound * np.ones(model.nv), args.bound * np.ones(model.nv))
    if args.step_control:
        s.set_step_control()
    s.synchronize()
    t0 = time.perf_counter()
    out = s.SolvePose(tgt, dt=1.0, gain=1.0, tol_pose=args.tol, max_steps=args.steps, q=q0)
    total = time.perf_counter() - t0
    tm = s.pose_timing()
    s.close()
    return out["reached"], out["steps"], total, tm["steps"], tm["solve_ms"], tm["total_ms"] - tm["solve_ms"]


def run_host(model, link, q0, tgt, prm, args):
    B = q0.shape[0]
    s = loik_amd.BatchedLoik(model, B, **prm)
    A = np.eye(6)
    s.SolveInit(q0, np.eye(6), np.zeros(6), np.array([link], dtype=np.int32), A[None], np.zeros((B, 1, 6)),
                -args.bound * np.ones(model.nv), args.bound * np.ones(model.nv))
    s.synchronize()
    q = q0.copy()
    reached, steps = np.zeros(B, dtype=bool), np.zeros(B, dtype=np.int32)
    Rd, td = tgt[:, 0, :9].reshape(B, 3, 3), tgt[:, 0, 9:]
    solve_s = n_steps = 0
    t0 = time.perf_counter()
    for step in range(args.steps + 1):
        R, t = fk(model, q, link)
        e = log6(np.einsum("bji,bjk->bik", R, Rd), np.einsum("bji,bj->bi", R, td - t))
        reached |= np.abs(e).max(axis=1) <= args.tol
        run = ~reached
        if step == args.steps or not run.any():
            break
        b = np.where(run[:, None], e, 0.0)[:, None, :]   # (gain / dt = 1, A = I)
        t1 = time.perf_counter()
        s.Solve(q, link, A, b)
        solve_s += time.perf_counter() - t1
        z = s.get("z")
        q[run] += z[run]
        steps[run] += 1
        n_steps += 1
    total = time.perf_counter() - t0
    s.close()
    return reached, steps, total, n_steps, solve_s * 1e3, (total - solve_s) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["all"] + list(WORKLOADS))
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--targets", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--spread", type=float, default=0.2)
    ap.add_argument("--bound", type=float, default=2.0)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--step-control", action="store_true")
    args = ap.parse_args()
    names = list(WORKLOADS) if args.workload == "all" else [args.workload]
    for name in names:
        model = loik_amd.builtin_model(name)
        link = model.getJointId(WORKLOADS[name])
        q0, tgt = make(model, link, args.batch, args.targets, 0x9053 + len(name), args.spread)
        prm = dict(W.FIXTURE_PARAMS, max_iter=300, tol_abs=1e-5, tol_rel=0.0, warm_start=True)
        run_device(model, link, q0[:min(args.batch, 4096)], tgt[:min(args.batch, 4096)], prm, args)   # (warm-up: code objects, allocations)
        r = run_device(model, link, q0, tgt, prm, args)
        print(json.dumps(summary("device (loikb_solve_pose%s)" % (", step control" if args.step_control else ""), name, args.batch, args.targets, *r, args)), flush=True)
        if not args.no_host and not args.step_control:
            r = run_host(model, link, q0, tgt, prm, args)
            print(json.dumps(summary("host (FK, log6, integrate in numpy; tailored Solve with q and b)", name, args.batch, args.targets,
                                     *r, args)), flush=True)


if __name__ == "__main__":
    main()
