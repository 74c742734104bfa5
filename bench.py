#!/usr/bin/env python
"""bench.py -- headline benchmark of the MI355X-native batched LoIK solver.

  python bench.py --gpus N --steps K --warmup W [--scaling weak|strong] [--dump-outputs DIR]

`--gpus N` runs N GPUs BY ITSELF: the batch shards into independent contiguous ranges with no exchange step
(SURVEY.md 8(e)), so one process drives N devices with one host thread + one solver handle + one stream per device
(`loikb_options.device`); wall clock around all of them, sum of the solves, max of the time.  Under
`python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N` (WORLD_SIZE > 1 in the environment) every
rank drives ONE device instead and a gloo process group carries only the timing barrier, the max-over-ranks time and
the sums of the counters -- still no collective on the data path.

Metric (BASELINE.json): IK solves/s to 1e-6 residual, Talos humanoid, batch = 65536, fp64, adaptive mu.
A "step" is one cold `Solve()` (the reference's hot loop, /root/reference/include/loik/loik-loid-optimized.hpp:368-455)
over synthetic problem instances whose inputs were placed in HBM by `SolveInit()` before the timed region -- the same
split the reference's own timing test uses (`SolveInit` once, then time `Solve()`, tests/loik-loid.cpp:987-1032).
A "solve" is an instance that stops with primal AND dual residual below 1e-6 (`get_convergence_status()`); instances
that trip the reference's infeasibility certificate or hit max_iter are executed and timed but not counted.
  --scaling weak   (default) every GPU solves its own 65536 instances: `value` grows with N at fixed ms_per_step
  --scaling strong the 65536 instances of the 1-GPU run are split over the N GPUs (BASELINE.json's wording "batch=65536 at
                   1/2/4/8 GPUs"); with N > 1 the weak line also carries a `strong_scaling` object measured in the same run

Prints ONE JSON line (rank 0).  `roofline` prices the DOMINANT kernel (the one that ran most ADMM instance-iterations of
the timed steps) against the roof that bounds it:
  * `k_flat` / `k_lean` / `k_tail` keep an instance's whole ADMM state in registers/LDS (one load and one store of the instance
    per solve): they are bound by fp64 vector issue, not by HBM -> bound "fp64_valu", achieved = algorithmic flops per launch
    (935 nb per instance-iteration) / average launch duration (HIP events recorded by the library on the
    launch stream), peak 78.6 TFLOP/s (fp64 vector, half the guide's 157.3 TFLOP/s fp32 vector rate).  Beside it: the HBM
    bytes the PMC counters saw (`traffic`, `hbm_measured_frac`) and the VALU issue fraction, from the committed rocprofv3
    summary `profiles/pmc_latest.json` when it describes this workload.  A launch has two regimes, reported separately: `bulk`
    (until the work queue runs dry: every lane group busy -- the library times it, `loikb_stats.queue_dry_ms`) and `tail` (the
    rest: the launch waits for the instances that run all 999 iterations, a serial chain per instance -- its length is the
    iteration time of a lone instance, measured on a 64-instance batch).
  * `k_solve` streams every instance through HBM each iteration: bound "hbm", achieved = algorithmic bytes
    (8 B x (203 nb + 108 nc) per instance-iteration) per launch / average launch duration, peak 8000 GB/s.
`cpu_baseline` times the CPU oracle (a line-faithful C port of the reference solver, NOT upstream libloik) on a bounded
sample of the same workload on the cores this process may actually use (affinity mask and cgroup quota), rebuilt with
-march=native on the box.
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0       # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md
FP32_VALU_PEAK_TF = 157.3   # same guide: peak FP32 (vector)
FP64_VALU_PEAK_TF = 78.6    # fp64 vector FMA issues at half the fp32 vector rate (4 cycles per wave64 instruction)
FP64_VALU_MEASURED_TF = 55.5  # independent v_fma_f64 streams on all 256 CUs, two wavefronts per SIMD x 8 chains (scripts/ubench/fp64_rate.hip, profiles/r05_a_fp64_rate.txt)
FLOPS_PER_JOINT_ITERATION = 935  # ~935 flop per joint and ADMM iteration
HEADLINE_BATCH = 65536


def effective_cpus():
    """cores this process may really use: the affinity mask, capped by the cgroup CPU quota (cpu.max / cfs_quota)"""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:  # cgroup v2: "<quota> <period>" or "max <period>"
            q, p = f.read().split()[:2]
            if q != "max":
                quota = float(q) / float(p)
    except Exception:
        try:  # cgroup v1
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / p
        except Exception:
            pass
    note = "affinity mask: %d" % n
    if quota is not None:
        note += ", cgroup quota: %.1f cpus" % quota
        n = max(1, min(n, int(quota + 0.5)))
    return n, note


def cpu_baseline(wl, budget_s=15.0):
    """oracle (kind "port") on the box's host cores, bounded sample of the same workload"""
    from oracle import ref
    cores, cores_note = effective_cpus()
    m, prm = wl["model"], wl["params"]
    B = wl["q"].shape[0]

    def run(n, threads):
        t = time.perf_counter()
        out = ref.solve_batch(m, wl["q"][:n], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"][:n], wl["lb"],
                              wl["ub"], nthreads=threads, native=True, **prm)
        return time.perf_counter() - t, out

    # one thread on the real workload (heavy-tailed iteration counts included): instance-iterations/s per core
    n1 = min(B, 256)
    t1, o1 = run(n1, 1)
    t1, o1 = run(n1, 1)
    rate1 = float(o1["iters"].sum()) / t1
    # all usable cores, sample sized for ~budget_s of wall time
    n0 = min(B, 64 * cores)
    t0, _ = run(n0, cores)  # pilot (also starts the thread pool)
    t0, _ = run(n0, cores)
    n = int(min(B, max(n0, n0 * budget_s / max(t0, 1e-4))))
    n = max(16 * cores, (n // (16 * cores)) * 16 * cores)
    n = min(n, B)
    dt, out = run(n, cores)
    rate = float(out["iters"].sum()) / dt
    # one thread, one iteration at a time: microseconds per ADMM iteration, as the reference's own timing test measures
    # it (SolveInit once, then Solve() with max_iter = 2; /root/reference/tests/loik-loid.cpp:987-1032)
    one_us = None
    try:
        t2 = time.perf_counter()
        o2 = ref.solve_batch(m, wl["q"][:64], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"][:64], wl["lb"],
                             wl["ub"], nthreads=1, native=True, **dict(prm, max_iter=201, tol_abs=0.0, tol_primal_inf=0.0))
        one_us = (time.perf_counter() - t2) / max(int(o2["iters"].sum()), 1) * 1e6
    except Exception:
        pass
    # ONE problem per call, the reference's own use: wall-clock of one cold solve of instance 0 of a 1-instance batch (the GPU's figure for
    # the same call: single_call_variant.b1_solve_wall_ms; with the results on the host, as the CPU solver has them: b1_solve_plus_results_wall_ms)
    one_call_ms = one_call_iters = None
    try:
        from loik_amd import workloads as _w
        w1 = _w.talos_c3(1, seed=3)
        best = 1e9
        for _ in range(20):
            t3 = time.perf_counter()
            o3 = ref.solve_batch(w1["model"], w1["q"], w1["H_ref"], w1["v_ref"], w1["c_ids"], w1["Ais"], w1["bis"], w1["lb"], w1["ub"], nthreads=1,
                                 native=True, **w1["params"])
            best = min(best, time.perf_counter() - t3)
        one_call_ms, one_call_iters = best * 1e3, int(o3["iters"][0])
    except Exception:
        pass
    eff = rate / (cores * rate1)
    return dict(single_problem_solve_ms=one_call_ms, single_problem_iterations=one_call_iters,
                value=float(out["converged"].sum() / dt), unit="solves/s", cores=cores, kind="port",
                cores_note=cores_note + ", os.cpu_count(): %s" % os.cpu_count(),
                single_thread_us_per_iteration=one_us,
                single_thread_instance_iterations_per_s=rate1,
                instance_iterations_per_s=rate,
                parallel_efficiency=eff,
                consistent=bool(0.5 <= eff <= 2.0),
                consistency_def="threads x single-thread rate vs measured rate must agree within 2x "
                                "(parallel_efficiency = measured / (cores x single-thread rate))",
                sample="first %d instances of the same workload, %d OpenMP threads (dynamic schedule, 16 instances per "
                       "block), %.1f s, %.0f ADMM instance-iterations/s; oracle/loik_ref.c = line-faithful C port of the "
                       "reference solver (not upstream libloik), built with -O3 -march=native on this box"
                       % (n, cores, dt, rate))


class Shard:
    """one device: its slice of the workload, its solver handle(s), the per-step statistics of its timed steps.

    fresh = 0: ONE handle solves the shard's batch again and again (the reference's timing test; from the second solve on the
    engine orders the instances by the iteration counts the batch had the solve before -- exact knowledge).
    fresh = n: every step solves a batch NO handle has solved before (what a caller with new problems gets): n handles, each with
    the history a caller's handle would have (one earlier solve of another batch: the decades of mu its instances visit) and
    its own fresh batch resident in HBM (SolveInit, untimed -- the metric times Solve()); step k is handle k's
    first Solve() of that batch.  `fresh_wl(k)` makes batch k (same generator, other seed)."""

    def __init__(self, idx, device, wl, flags, max_launch_iters, factory=None, fresh=0, fresh_wl=None):
        if factory is None:
            import loik_amd
            factory = loik_amd.BatchedLoik
        if callable(wl):
            wl = wl()  # (generated here: build_shards constructs every shard on the host thread of its own)
        self.idx, self.device, self.wl = idx, device, wl
        self.B = wl["q"].shape[0]
        args = lambda w: (w["q"], w["H_ref"], w["v_ref"], w["c_ids"], w["Ais"], w["bis"], w["lb"], w["ub"])
        make = lambda: factory(wl["model"], self.B, device=device, flags=flags, max_launch_iters=max_launch_iters, **wl["params"])
        self.pool = []
        if fresh > 0:
            for k in range(fresh):
                h = make()
                h.SolveInit(*args(wl))
                h.Solve()                      # the handle's history
                t = time.perf_counter()
                h.SolveInit(*args(fresh_wl(k)))
                self.t_init = time.perf_counter() - t
                self.pool.append(h)
            self.solver = self.pool[0]
        else:
            self.solver = make()
            t = time.perf_counter()
            self.solver.SolveInit(*args(wl))
            self.t_init = time.perf_counter() - t  # includes the PCIe upload of the host-side synthetic inputs
        self.nstep = 0
        self.timed = []   # handles of the timed steps (fresh: one each)
        self.acc = {}
        self.last = None
        self.err = None

    def handles(self):
        return self.pool if self.pool else [self.solver]

    def step(self, timed):
        s = self.pool[self.nstep] if self.pool else self.solver
        self.nstep += 1
        s.Solve()
        if timed:
            st = s.stats()
            self.last = st
            self.timed.append(s)
            for k in ("kernel_ms", "tail_ms", "tail_instances", "tail_instance_iterations", "tail_launches", "total_ms",
                      "solve_busy_ms", "tail_busy_ms", "instance_iterations", "launches", "hslots_ms", "lean_launches",
                      "flat_launches", "queue_dry_ms", "flat_split_launches", "flat_ordered"):
                self.acc[k] = self.acc.get(k, 0) + st.get(k, 0)

    def close(self):
        for h in self.handles():
            h.close()

    def chain_summary(self, steps):
        """per timed step of THIS shard: the on-chip launch split into its bulk (until a wavefront first finds the work queue empty) and the
        chain of the long runners behind it (SIMDs mostly idle: what bounds small shards, i.e. the strong-scaling curve), and the slot
        kernel -- so that a multi-GPU run separates chain from bulk per device"""
        a = self.acc
        n = max(steps, 1)
        launch = (a.get("tail_ms", 0.0) - a.get("hslots_ms", 0.0)) / n
        bulk = a.get("queue_dry_ms", 0.0) / n
        return {"gpu": self.idx, "batch": self.B, "launch_ms": launch, "bulk_ms": bulk if bulk > 0 else None,
                "lone_chain_ms": (launch - bulk) if bulk > 0 else None, "slots_ms": a.get("hslots_ms", 0.0) / n,
                "instance_iterations": a.get("instance_iterations", 0) / n}

    def results(self):
        """per timed step (the mean over the steps' batches when every step had its own)"""
        prm = self.wl["params"]
        rows = []
        for s in (self.timed if self.pool else [self.solver]):
            conv = s.get("converged").astype(bool)
            it = s.get("iter")
            infeas = s.get("primal_infeasible").astype(bool)
            rows.append((int(conv.sum()), int(it.sum()), int(infeas.sum()), int(((it >= prm["max_iter"] - 1) & ~conv).sum())))
        m = np.mean(np.array(rows, dtype=float), axis=0)
        return dict(solved=float(m[0]), iters=float(m[1]), batch=self.B, infeasible=float(m[2]), unfinished=float(m[3]))


class ShardC4(Shard):
    """BASELINE.json config 4, one GPU's share: `batch` Talos instances, T successive targets per instance through the TAILORED
    warm-started entry Solve(q, c_id, Ai, bi) (loik-loid-optimized.hpp:596-695) -- the sampling-planner workload.  A step = one
    tailored solve of the whole share on target k mod T (its own configuration q_t and its own feasible wrist twist b_t, both
    resident in HBM before the timed region: loik_amd.capi.DeviceArray, LOIKB_IN_DEVICE); FwdPassInit of q_t, UpdateEqConstraint and
    the warm start are part of the step, as they are of the reference's call.  The converged flags and iteration counts are read back
    after every step (1 MB per step, inside the timed region: the planner needs them)."""

    def __init__(self, idx, device, wl, flags, max_launch_iters, factory=None, fresh=0, fresh_wl=None):
        import loik_amd
        from loik_amd import capi
        if factory is None:
            factory = loik_amd.BatchedLoik
        if callable(wl):
            wl = wl()
        self.idx, self.device, self.wl = idx, device, wl
        self.B = wl["q"].shape[0]
        self.pool = []
        self.solver = factory(wl["model"], self.B, device=device, flags=flags, max_launch_iters=max_launch_iters, **wl["params"])
        t = time.perf_counter()
        self.solver.SolveInit(wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])
        self.t_init = time.perf_counter() - t
        self.link = int(wl["c_ids"][0])
        dev = (lambda a: capi.DeviceArray(a, device)) if factory is loik_amd.BatchedLoik else (lambda a: a)
        self.targets = [(dev(q), dev(b[:, 0])) for q, b in wl["steps"]]
        self.nstep, self.timed, self.acc, self.last, self.err = 0, [], {}, None, None
        self.rows = []

    def step(self, timed):
        q, b = self.targets[self.nstep % len(self.targets)]
        self.nstep += 1
        s = self.solver
        s.Solve(q, self.link, self.wl["Ais"][0], b)
        conv, it = s.get("converged").astype(bool), s.get("iter")
        if timed:
            st = s.stats()
            self.last = st
            inf = s.get("primal_infeasible").astype(bool)
            self.rows.append((int(conv.sum()), int(it.sum()), int(inf.sum()), int(((it >= self.wl["params"]["max_iter"] - 1) & ~conv).sum())))
            for k in ("kernel_ms", "tail_ms", "tail_instances", "tail_instance_iterations", "tail_launches", "total_ms",
                      "solve_busy_ms", "tail_busy_ms", "instance_iterations", "launches", "hslots_ms", "lean_launches",
                      "flat_launches", "queue_dry_ms", "flat_split_launches", "flat_ordered"):
                self.acc[k] = self.acc.get(k, 0) + st.get(k, 0)

    def results(self):
        m = np.mean(np.array(self.rows, dtype=float), axis=0)
        return dict(solved=float(m[0]), iters=float(m[1]), batch=self.B, infeasible=float(m[2]), unfinished=float(m[3]))


def build_shards(specs):
    """Shard(*spec) for every spec, each on a host thread of its own: the synthetic workload of a shard is generated, uploaded
    and SolveInit'ed concurrently with the others' (eight shards one after the other cost eight times the set-up of one)"""
    out, errs = [None] * len(specs), [None] * len(specs)

    def work(i):
        try:
            cls = specs[i][0] if isinstance(specs[i][0], type) else Shard
            out[i] = cls(*(specs[i][1:] if isinstance(specs[i][0], type) else specs[i]))
        except Exception as e:
            errs[i] = e

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(specs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for e in errs:
        if e is not None:
            for sh in out:
                if sh is not None:
                    sh.close()
            raise e
    return out


def run_shards(shards, steps, warmup, barrier=None):
    """every shard on its own host thread: W untimed steps, barrier, K timed steps, barrier.  Returns the wall time from
    the moment all shards are through the first barrier until the last one finished its K steps."""
    n = len(shards)
    sync = threading.Barrier(n + 1)
    t_done = [0.0] * n

    def work(i):
        sh = shards[i]
        try:
            for _ in range(warmup):
                sh.step(False)
            sh.solver.synchronize()
        except Exception as e:  # keep the barriers balanced
            sh.err = e
        sync.wait()   # all warmed up
        sync.wait()   # t0 taken
        try:
            if sh.err is None:
                for _ in range(steps):
                    sh.step(True)
                sh.solver.synchronize()  # hipDeviceSynchronize on the shard's device (Solve() already drained its stream)
        except Exception as e:
            sh.err = e
        t_done[i] = time.perf_counter()
        sync.wait()

    th = [threading.Thread(target=work, args=(i,)) for i in range(n)]
    for t in th:
        t.start()
    sync.wait()
    if barrier is not None:
        barrier()
    t0 = time.perf_counter()
    sync.wait()
    sync.wait()
    for t in th:
        t.join()
    for sh in shards:
        if sh.err is not None:
            raise sh.err
    elapsed = max(t_done) - t0
    if barrier is not None:
        barrier()
    return elapsed


DUMP_MAX_BYTES = 64 * 10**6   # --dump-outputs: at most 64 MB in all; above that a fixed sample of the instances
DUMP_SAMPLE_SEED = 0xD0D0


def dump_outputs(out_dir, shards, dist=None):
    """--dump-outputs DIR: what a caller of the timed path receives after the last timed step -- the result members of the handle
    that ran it (get_results: z, nu, w, vis, fis, yis and the [B][33] scalar block), every shard of the job in device order, instance
    axis first -- as DIR/<name>.npy in float64, and DIR/instance.npy: each row's index in the job's whole batch.  When all of it would
    exceed DUMP_MAX_BYTES, the rows are a fixed, seeded sample of the instances, the same rows for every member.  The inputs are seeded:
    the same arguments give the same files on any build, so that two builds can be compared output for output.  Runs on every rank
    (the rows travel to rank 0 through the gloo group, after the timed region); returns a summary on rank 0, None elsewhere."""
    sizes = [sh.B for sh in shards]
    offset = 0
    if dist is not None:
        every = [None] * dist.get_world_size()
        dist.all_gather_object(every, sizes)
        offset = sum(sum(s) for s in every[:dist.get_rank()])
        total = sum(sum(s) for s in every)
    else:
        total = sum(sizes)
    rows = parts = None
    for sh in shards:
        h = sh.timed[-1] if sh.timed else sh.solver
        res = h.get_results(h.RESULT_FIELDS)
        if rows is None:
            row_bytes = 8 + sum(a.nbytes // max(a.shape[0], 1) for a in res.values())   # (8: instance.npy)
            k = min(total, (DUMP_MAX_BYTES - 256 * (len(res) + 1)) // row_bytes)     # (256: room for each file's .npy header)
            rows = np.arange(total) if k == total else np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(total, k, replace=False))
            parts = {name: [] for name in res}
            parts["instance"] = []
        mine = rows[(rows >= offset) & (rows < offset + sh.B)]
        for name, a in res.items():
            parts[name].append(np.asarray(a, dtype=np.float64)[mine - offset])
        parts["instance"].append(mine.astype(np.float64))
        offset += sh.B
    parts = {name: np.concatenate(p) for name, p in parts.items()}
    if dist is not None:
        got = [None] * dist.get_world_size() if dist.get_rank() == 0 else None
        dist.gather_object(parts, got, dst=0)
        if dist.get_rank() != 0:
            return None
        parts = {name: np.concatenate([g[name] for g in got]) for name in parts}
    os.makedirs(out_dir, exist_ok=True)
    for name, a in parts.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {"dir": out_dir, "files": sorted(name + ".npy" for name in parts), "instances": int(rows.size), "of": int(total),
            "bytes": int(sum(a.nbytes for a in parts.values())), "dtype": "float64",
            "what": "result members of the last timed step (get_results), rows = instance.npy of the whole batch" +
                    (" (a sample seeded with %d)" % DUMP_SAMPLE_SEED if rows.size < total else "")}


def csrc_sha16():
    """identity of the kernels a measurement belongs to: sha256 over loik_amd/csrc/* and include/*.h (first 16 hex digits).  The GPU
    box has no .git; the sources travel, so this is computable wherever the numbers are taken"""
    import hashlib
    h = hashlib.sha256()
    for d in (os.path.join(ROOT, "loik_amd", "csrc"), os.path.join(ROOT, "include")):
        for f in sorted(os.listdir(d)):
            fp = os.path.join(d, f)
            if os.path.isfile(fp):
                h.update(f.encode()); h.update(open(fp, "rb").read())
    return h.hexdigest()[:16]


def load_pmc(B):
    """committed rocprofv3 PMC summary of this workload (scripts/profile_round.sh writes it); None when absent"""
    for name in ("pmc_latest.json", "traffic_latest.json"):
        p = os.path.join(ROOT, "profiles", name)
        if os.path.exists(p):
            try:
                d = json.load(open(p))
                if d.get("batch", HEADLINE_BATCH) == B:
                    d["_file"] = "profiles/" + name
                    return d
            except Exception:
                pass
    return None


def kernel_roofline(acc, last, steps, nb, nc, B):
    """roofline object of the dominant kernel of the timed steps of ONE device (rank 0 / shard 0)"""
    bytes_iter = last["bytes_per_instance_iteration"]
    flops_iter = float(FLOPS_PER_JOINT_ITERATION * nb)
    inst_iters = acc["instance_iterations"]
    tail_iters = acc["tail_instance_iterations"]
    solve_iters = inst_iters - tail_iters
    solve_launches = acc["launches"] - acc["tail_launches"]
    solve_ms = acc["kernel_ms"] - acc["tail_ms"]
    lean = acc["lean_launches"] > 0
    flat = acc.get("flat_launches", 0) > 0
    pmc = load_pmc(B)
    pk = (pmc or {}).get("kernels", {})

    def pmc_bytes(key):
        if key in pk and "fetch_bytes_per_dispatch" in pk[key]:
            return pk[key]["fetch_bytes_per_dispatch"] + pk[key]["write_bytes_per_dispatch"]
        if key in pk:  # (summaries of rounds 1-3: one dispatch per step)
            return pk[key]["fetch_bytes_per_step"] + pk[key]["write_bytes_per_step"]
        return None

    if tail_iters >= solve_iters:
        # ---- on-chip engine: fp64 vector issue is the roof
        name = ("k_flat2" if acc.get("flat_split_launches", 0) > 0 else "k_flat") if flat else "k_lean" if lean else "k_tail"
        slots_name = "k_fslots" if flat else "k_hslots"
        launches = max(acc["tail_launches"], 1)
        # the library times k_hslots (decade-slot precomputation) + the lean launch together; k_lean alone = the rest
        own_ms = acc["tail_ms"] - (acc["hslots_ms"] if lean else 0.0)
        avg_ms = own_ms / launches
        units = tail_iters / launches
        ach = units * flops_iter / (avg_ms * 1e-3) / 1e12 if avg_ms > 0 else 0.0
        traffic = pmc_bytes(name)
        r = {"bound": "fp64_valu", "kernel": name, "achieved": ach, "peak": FP64_VALU_PEAK_TF, "unit": "TFLOP/s",
             "frac": ach / FP64_VALU_PEAK_TF,
             # what a kernel of nothing but independent v_fma_f64 reaches on all 256 CUs of this part (scripts/ubench/fp64_rate.hip, two
             # wavefronts per SIMD x 8 chains: profiles/r05_a_fp64_rate.txt; one CU alone: 65.8): the clock under full fp64 load
             "peak_measured_dense_fma": FP64_VALU_MEASURED_TF, "frac_of_measured_peak": ach / FP64_VALU_MEASURED_TF,
             "traffic": traffic,
             "flops_per_unit": flops_iter,
             "unit_def": "one ADMM iteration of one instance: 935 flop x nb (nb = %d), SURVEY.md 8(d)" % nb,
             "units_per_launch": units, "avg_launch_ms": avg_ms, "launches_per_step": launches / steps,
             "instance_iterations_per_s": units / (avg_ms * 1e-3) if avg_ms > 0 else None,
             "share_of_instance_iterations": tail_iters / max(inst_iters, 1),
             "why_not_hbm": "the state of an instance stays in registers/LDS for its whole solve: HBM sees one load and "
                            "one store per instance plus the decade slots (%s writes, %s fetches on a "
                            "change of mu) -- `traffic` is what the PMC counters measured, a few %% of the streaming "
                            "model's %.0f B per unit" % (slots_name, name, bytes_iter)}
        if flat and acc.get("queue_dry_ms", 0.0) > 0:
            # the two regimes of the launch: bulk = until a lane group first finds the work queue empty, tail = the rest
            bulk_ms = acc["queue_dry_ms"] / launches
            r["bulk"] = {"ms": bulk_ms, "share_of_launch": bulk_ms / avg_ms,
                         "note": "every lane group busy; the instance-iterations of the launch are not split between the regimes "
                                 "(an instance's count is known when it stops), so no flop rate is stated for either alone: "
                                 "see `bulk_rate` for the saturated rate on a 4x batch"}
            r["tail"] = {"ms": avg_ms - bulk_ms, "share_of_launch": 1.0 - bulk_ms / avg_ms,
                         "note": "the launch waits for the instances that run to max_iter: a serial chain of <= 999 iterations "
                                 "from whenever they were fetched -- see `lone_instance_us_per_iteration`"}
        if traffic is not None and avg_ms > 0:
            gbs = traffic / (avg_ms * 1e-3) / 1e9
            r["hbm_measured_GBps"] = gbs
            r["hbm_measured_frac"] = gbs / HBM_PEAK_GBS
            r["hbm_algorithmic_bytes_per_launch"] = units * bytes_iter
        if pmc and name in pk and "valu_insts_per_step" in pk[name]:
            # VALU issue: wave64 fp64 instructions take 4 cycles on a SIMD; 4 SIMDs x CUs, at the shader clock
            insts = pk[name].get("valu_insts_per_dispatch", pk[name]["valu_insts_per_step"] / max(pk[name].get("dispatches_per_step", 1.0), 1.0))
            ncu, clk = pmc.get("compute_units", 256), pmc.get("shader_clock_ghz", 2.4)
            r["valu_issue_frac"] = insts * 4.0 / (4 * ncu * avg_ms * 1e-3 * clk * 1e9)
            if "valu_active_quadcycles_per_dispatch" in pk[name]:
                # SQ_ACTIVE_INST_VALU counts 4-cycle units in which a SIMD's VALU executes an instruction, summed over the SIMDs:
                # the share of the launch in which the vector ALUs were at work (the tools' VALUBusy)
                r["valu_busy_frac_at_nominal_clock"] = pk[name]["valu_active_quadcycles_per_dispatch"] * 4.0 / (4 * ncu * avg_ms * 1e-3 * clk * 1e9)
                r["valu_busy_frac"] = pk[name].get("valu_busy_frac_of_actual_cycles", r["valu_busy_frac_at_nominal_clock"])
                if "shader_cycles_per_dispatch" in pk[name]:
                    r["shader_clock_ghz_measured"] = pk[name]["shader_cycles_per_dispatch"] / (avg_ms * 1e-3) / 1e9
                r["lds_pipe_busy_frac"] = pk[name].get("lds_pipe_busy_frac_of_actual_cycles")
                r["valu_busy_note"] = ("SQ_ACTIVE_INST_VALU x 4 over the SIMD-cycles the dispatch actually took (GRBM_GUI_ACTIVE / 8 XCDs): with every "
                                       "SIMD on fp64 work the chip runs at ~2.06 GHz, not the data sheet's 2.4 (`.._at_nominal_clock` is round 4's "
                                       "figure).  Two wavefronts per SIMD at 256 registers; the vector ALUs AND the CU's LDS pipe are each busy in "
                                       "more than half of the cycles, a wavefront issues in order: a third wavefront per SIMD (168 registers, "
                                       "12.7 KB of LDS: built and measured in round 5, profiles/r05_a_pmc_wpe2_vs_wpe3.txt) adds no throughput")
            r["valu_insts_per_instance_iteration"] = pk[name].get("valu_insts_per_instance_iteration")
            r["lds_bank_conflict_frac"] = pk[name].get("lds_bank_conflict_frac")
        if pmc:
            r["pmc_source"] = pmc["_file"]
            r["pmc_csrc_sha16"] = pmc.get("csrc_sha16")
            r["pmc_stale"] = pmc.get("csrc_sha16") != csrc_sha16()   # counters taken on other kernel sources than the ones timed here
        if lean:
            hs = {"kernel": slots_name, "avg_launch_ms": acc["hslots_ms"] / steps, "traffic": pmc_bytes(slots_name),
                  "role": ("the joints' columns of W (the explicit inverse of the unit-triangular factor of the tree elimination) and "
                           "Dinv for the decades of mu, precomputed once per Solve() before k_flat") if flat else
                          "H_i / Dinv_i of the decades of mu, precomputed once per Solve() before k_lean (HBM write-bound)"}
            if hs["traffic"] is not None and hs["avg_launch_ms"] > 0:
                hs["hbm_measured_GBps"] = hs["traffic"] / (hs["avg_launch_ms"] * 1e-3) / 1e9
            r["other_kernel"] = hs
        elif solve_iters > 0:
            r["other_kernel"] = {"kernel": "k_solve", "share_of_instance_iterations": solve_iters / max(inst_iters, 1),
                                 "sum_of_launch_ms_per_step": solve_ms / steps}
        return r
    # ---- streaming engine: HBM is the roof
    launches = max(solve_launches, 1)
    avg_ms = solve_ms / launches
    units = solve_iters / launches
    ach = units * bytes_iter / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
    traffic = pmc_bytes("k_solve")
    r = {"bound": "hbm", "kernel": "k_solve", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
         "frac": ach / HBM_PEAK_GBS, "traffic": None if traffic is None else traffic / (launches / steps),
         "bytes_per_unit": bytes_iter,
         "unit_def": "one ADMM iteration of one instance: 8 B x (203 nb + 108 nc), nb = %d, nc = %d (three-sweep streaming "
                     "model of SURVEY.md 8(d))" % (nb, nc),
         "units_per_launch": units, "avg_launch_ms": avg_ms, "launches_per_step": launches / steps,
         "share_of_instance_iterations": solve_iters / max(inst_iters, 1)}
    if tail_iters > 0:
        r["other_kernel"] = {"kernel": "k_flat" if flat else "k_lean" if lean else "k_tail",
                             "share_of_instance_iterations": tail_iters / max(inst_iters, 1),
                             "sum_of_launch_ms_per_step": acc["tail_ms"] / steps}
    return r


def whole_body_variant(args, device):
    """Reported beside the headline (not `value`): the 44-DoF Talos tree of the reference's fixture file with FOUR simultaneous
    6-D tasks (both wrists, both feet) -- every limb of the robot works, unlike C3's 9-joint support chain -- same batch,
    tolerances and engine selection (loik_amd.workloads.talos_wholebody).  Like the headline: `value` is a handle's first solve of a
    batch it has not seen; `repeat_same_batch` the reference's timing loop (ordered from the second solve on)."""
    import loik_amd
    from loik_amd import workloads
    wl = workloads.talos_wholebody(args.batch)
    m, prm = wl["model"], wl["params"]
    a = lambda w: (w["q"], w["H_ref"], w["v_ref"], w["c_ids"], w["Ais"], w["bis"], w["lb"], w["ub"])
    s = loik_amd.BatchedLoik(m, args.batch, device=device, flags=args.flags, **prm)
    s.SolveInit(*a(wl))
    s.Solve()
    s.synchronize()
    steps = max(2, min(args.steps, 3))
    t0 = time.perf_counter()
    for _ in range(steps):
        s.Solve()
    s.synchronize()
    dt_rep = (time.perf_counter() - t0) / steps
    conv_rep = s.get("converged").astype(bool)
    it_rep = s.get("iter")
    ms, solved, iters = [], 0, 0
    for i in range(steps):
        w2 = workloads.talos_wholebody(args.batch, seed=0xB0D1 + i)
        s.SolveInit(*a(w2))
        s.synchronize()
        t0 = time.perf_counter()
        s.Solve()
        s.synchronize()
        ms.append(time.perf_counter() - t0)
        solved += int(s.get("converged").astype(bool).sum()); iters += int(s.get("iter").sum())
    dt = sum(ms) / len(ms)
    st = s.stats()
    conv = s.get("converged").astype(bool)
    it = s.get("iter")
    flops = FLOPS_PER_JOINT_ITERATION * m.nv
    out = {"workload": wl["name"], "robot": "talos44 (topology of talos_full_v2.urdf, 44 x 1-DoF, depth 11, four joints on each wrist link)",
           "num_eq_c": len(wl["c_ids"]), "batch": args.batch, "ms_per_step": dt * 1e3, "value": float(solved / sum(ms)),
           "unit": "solves/s", "schedule": "a fresh batch before every timed solve (arrival order, time-sliced)", "solved_fraction": float(conv.mean()),
           "flagged_infeasible_fraction": float(s.get("primal_infeasible").astype(bool).mean()),
           "mean_admm_iterations": float(it.mean()), "instance_iterations_per_s": float(iters / sum(ms)),
           "engine": (next((k for k in ("k_flat2", "k_flat1", "k_flat") if k in s.plan()), "k_flat") if st["flat_launches"] > 0 else "k_lean")
                     if st["lean_launches"] > 0 and st["tail_instances"] == args.batch
                     else "k_solve+k_tail",
           "lean_escaped": st["lean_escaped"],
           "achieved_TFLOPs": float(iters * flops / sum(ms) / 1e12),
           "frac_of_fp64_valu_peak": float(iters * flops / sum(ms) / 1e12 / FP64_VALU_PEAK_TF),
           "repeat_same_batch": {"ms_per_step": dt_rep * 1e3, "value": float(conv_rep.sum() / dt_rep), "unit": "solves/s",
                                 "frac_of_fp64_valu_peak": float(it_rep.sum() * flops / dt_rep / 1e12 / FP64_VALU_PEAK_TF)}}
    s.close()
    return out


def single_call_variant(args, device, wl0):
    """Reported beside the headline: the reference's OWN use -- one problem per Solve() call (tests/loik-loid.cpp:987-1032 times exactly
    that) -- and small batches: wall-clock of a cold Solve() on a handle whose problem is resident (SolveInit untimed), best of 30.
    Round 6: batches below 64 instances run on k_flat2 (2.2 us per iteration of a lone instance; k_tail, round 5's engine for them,
    10-12 us), and up to 2048 instances a Solve() is the short launch sequence (loik_host.hip, small_flat)."""
    import loik_amd
    from loik_amd import workloads
    out = {"what": "wall-clock of Solve() (reset + solve + the host's wait), problem resident, best of 30 calls; Talos-32, the headline's parameters", "rows": []}
    for B in (1, 8, 64, 1024):
        wl = workloads.talos_c3(B, seed=3)
        s = loik_amd.BatchedLoik(wl["model"], B, device=device, flags=args.flags, **wl["params"])
        s.SolveInit(wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])
        ts, tr, tf = [], [], []
        full_args = (wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])
        for _ in range(30):
            t = time.perf_counter(); s.Solve(); t1 = time.perf_counter(); s.get_results(s.RESULT_FIELDS); t2 = time.perf_counter()
            ts.append(t1 - t); tr.append(t2 - t1)
            t = time.perf_counter(); s.Solve(*full_args); tf.append(time.perf_counter() - t)   # (SolveInit + Solve from host arrays: hpp:475-580)
        it = s.get("iter")
        st = s.stats()
        out["rows"].append({"batch": B, "solve_wall_ms": min(ts) * 1e3, "solve_wall_ms_median": float(np.median(ts)) * 1e3, "max_iterations": int(it.max()),
                            "mean_iterations": float(it.mean()), "on_chip_ms": st["kernel_ms"], "engine": "k_flat2" if st["flat_split_launches"] else "k_tail",
                            "results_wall_ms": min(tr) * 1e3, "solve_plus_results_wall_ms": (min(ts) + min(tr)) * 1e3,
                            "full_solve_wall_ms": min(tf) * 1e3, "full_solve_plus_results_wall_ms": (min(tf) + min(tr)) * 1e3})
        s.close()
    out["results_note"] = ("results_wall_ms: z, nu, w, vis, fis, yis of the reference's data object AND the scalar block (iteration count, flags, residuals) to host arrays in one call (loikb_get_results; what the C++ "
                           "mirror include/loik_amd/loik.hpp fetches after every solve) -- a drop-in caller's time per problem is solve + results")
    out["b1_solve_wall_ms"] = out["rows"][0]["solve_wall_ms"]
    out["b1_solve_plus_results_wall_ms"] = out["rows"][0]["solve_plus_results_wall_ms"]
    out["b1_full_solve_plus_results_wall_ms"] = out["rows"][0]["full_solve_plus_results_wall_ms"]
    out["full_solve_note"] = ("full_solve_wall_ms: Solve(q, H_ref, v_ref, ids, Ais, bis, lb, ub) from host arrays = SolveInit + Solve in one call, what a caller with a "
                              "new problem per call uses (loik-loid-optimized.hpp:475-580); with the results on the host it is the figure to hold against the CPU "
                              "solver's time per problem (cpu_baseline.single_problem_solve_ms)")
    out["b1_iterations"] = out["rows"][0]["max_iterations"]
    return out


def schedule_variant(args, device):
    """What the order of the work queue is worth.  `value` is a handle's FIRST solve of a batch it has not seen: arrival order.  This
    variant reports the other ends: `repeat_same_batch` -- the reference's timing test (SolveInit once, then Solve() again and again,
    tests/loik-loid.cpp:987-1032): from its second solve on the engine takes the instances longest first, by the iteration counts the
    batch had the solve before, i.e. exact knowledge -- with the dominant kernel's rate in that regime; `same_batch_arrival_order`
    (LOIKB_FLAT_ORDER=0 on that batch); and `another_batch_every_solve` on ONE handle (SolveInit + Solve per batch, Solve() timed)
    with and without LOIKB_OPT_ORDER_FROM_PREVIOUS (the previous batch's counts predict nothing here: what that flag costs a caller
    whose problems do NOT resemble each other)."""
    import loik_amd
    from loik_amd import workloads
    out = {}
    wl = workloads.talos_c3(args.batch)
    nb = wl["model"].nv

    def timed_repeat(env_order):
        old = os.environ.get("LOIKB_FLAT_ORDER")
        try:
            if env_order is not None:
                os.environ["LOIKB_FLAT_ORDER"] = env_order
            s = loik_amd.BatchedLoik(wl["model"], args.batch, device=device, flags=args.flags, **wl["params"])
        finally:
            if old is None:
                os.environ.pop("LOIKB_FLAT_ORDER", None)
            else:
                os.environ["LOIKB_FLAT_ORDER"] = old
        s.SolveInit(wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])
        s.Solve(); s.Solve(); s.synchronize()
        n = max(3, min(args.steps, 5))
        own, ordered, iters = 0.0, 0, 0
        t0 = time.perf_counter()
        for _ in range(n):
            s.Solve()
            st = s.stats()
            own += st["tail_ms"] - st["hslots_ms"]; ordered += st["flat_ordered"]; iters += st["instance_iterations"]
        s.synchronize()
        dt = (time.perf_counter() - t0) / n
        conv = s.get("converged").astype(bool)
        tf = iters * FLOPS_PER_JOINT_ITERATION * nb / (own * 1e-3) / 1e12 if own > 0 else None
        r = {"ms_per_step": dt * 1e3, "value": float(conv.sum() / dt), "unit": "solves/s", "solves": n, "of_which_ordered": ordered,
             "queue_dry_ms": st["queue_dry_ms"], "kernel_avg_launch_ms": own / n,
             "kernel_instance_iterations_per_s": iters / (own * 1e-3) if own > 0 else None,
             "kernel_achieved_TFLOPs": tf, "kernel_frac_of_fp64_valu_peak": None if tf is None else tf / FP64_VALU_PEAK_TF}
        s.close()
        return r

    out["repeat_same_batch"] = timed_repeat(None)
    out["same_batch_arrival_order"] = timed_repeat("0")
    # (round 5: the batches are generated BEFORE the loop -- a caller has its problems; round 4 generated each one on the host between the
    #  solves, the GPU sat idle for ~0.3 s and the same kernels then ran 6-7 % longer: profiles/r05_a_one_handle_idle_gap.txt.  The
    #  variant `.._after_idle_gap` keeps that measurement: 100 ms of idleness before every timed Solve().)
    batches = [workloads.talos_c3(args.batch, seed=0x5EED + i) for i in range(7)]
    for key, fl, gap in (("another_batch_every_solve", 0, 0.0), ("another_batch_every_solve_after_idle_gap", 0, 0.1),
                         ("another_batch_every_solve_order_from_previous", loik_amd.capi.OPT_ORDER_FROM_PREVIOUS, 0.0)):
        s = loik_amd.BatchedLoik(wl["model"], args.batch, device=device, flags=args.flags | fl, **wl["params"])
        ms, solved, ordered, init_ms = [], [], 0, []
        for i, w2 in enumerate(batches):
            t0 = time.perf_counter()
            s.SolveInit(w2["q"], w2["H_ref"], w2["v_ref"], w2["c_ids"], w2["Ais"], w2["bis"], w2["lb"], w2["ub"])
            s.synchronize()
            init_ms.append((time.perf_counter() - t0) * 1e3)
            if gap:
                time.sleep(gap)
            t0 = time.perf_counter()
            s.Solve()
            s.synchronize()
            if i >= 2:
                ms.append((time.perf_counter() - t0) * 1e3)
                solved.append(int(s.get("converged").astype(bool).sum()))
                ordered += s.stats()["flat_ordered"]
        out[key] = {"ms_per_step": sum(ms) / len(ms), "value": float(sum(solved) / (sum(ms) * 1e-3)), "unit": "solves/s",
                    "solves": len(ms), "of_which_ordered": ordered, "solve_init_ms": sum(init_ms[2:]) / len(init_ms[2:]),
                    "idle_gap_before_solve_s": gap}
        s.close()
    return out


def fp32_tradeoff_variant(args, device):
    """BASELINE config 5's table: Panda-7, B = 65536, tol 1e-3 / 1e-4 x {fp64, fp32 fast, fp32 accurate
    (LOIKB_OPT_F32_ACCURATE)}: solves/s and the distance of the fp32 answers from the fp64 DEVICE answers (the fp64 oracle is
    the judge in tests/test_gpu_parity.py::test_c5_fp32_accuracy_contract; no oracle here)"""
    import numpy as np
    import loik_amd
    from loik_amd import capi, workloads
    rows = []
    for tol in (1e-3, 1e-4):
        wl = workloads.panda_c5(args.batch, tol=tol)
        m, prm = wl["model"], wl["params"]
        z64 = c64 = None
        # fp32_fast: the streaming engines in fp32 (k_solve + k_tail: what a small robot's batches up to 32 768 instances run on; forced
        # here with LOIKB_LEAN=0 -- since round 3 a plain fp32 handle of this size runs k_lean, i.e. the row fp32_accurate)
        for name, prec, flags in (("fp64", capi.F64, 0), ("fp32_fast", capi.F32, 0), ("fp32_accurate", capi.F32, capi.OPT_F32_ACCURATE)):
            old_env = os.environ.get("LOIKB_LEAN")
            if name == "fp32_fast":
                os.environ["LOIKB_LEAN"] = "0"
            try:
                s = loik_amd.BatchedLoik(m, args.batch, device=device, precision=prec, flags=args.flags | flags, **prm)
            finally:
                if old_env is None:
                    os.environ.pop("LOIKB_LEAN", None)
                else:
                    os.environ["LOIKB_LEAN"] = old_env
            s.SolveInit(wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])
            s.Solve()
            s.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                s.Solve()
            s.synchronize()
            dt = (time.perf_counter() - t0) / 3
            z, conv = s.get("z"), s.get("converged").astype(bool)
            st = s.stats()
            row = {"tol_abs": tol, "variant": name, "ms_per_step": dt * 1e3, "value": float(conv.sum() / dt), "unit": "solves/s",
                   "engine": "k_lean" if st["lean_launches"] > 0 else "k_solve+k_tail", "solved_fraction": float(conv.mean()),
                   "mean_admm_iterations": float(s.get("iter").mean())}
            if z64 is None:
                z64, c64 = z, conv
            else:
                dz = np.abs(z - z64).max(axis=1)[conv & c64]
                row["dz_inf_vs_fp64"] = {"median": float(np.median(dz)), "p99": float(np.quantile(dz, 0.99)), "max": float(dz.max())}
            rows.append(row)
            s.close()
    return {"workload": "panda7 C5, B=%d" % args.batch, "rows": rows}


def regimes_variant(args, device, nb):
    """The two regimes of the dominant kernel, each measured where it is alone (goes into `roofline`): the SATURATED rate on a
    batch four times the headline's (the work queue never runs dry for ~3/4 of the launch: the bulk regime) and the iteration
    time of a LONE instance (a 64-instance batch: one launch, its duration / its longest instance's iteration count -- the
    serial chain that the headline launch's tail consists of)."""
    import loik_amd
    from loik_amd import workloads
    out = {}
    for B, key in ((4 * args.batch, "bulk_rate"), (64, "lone")):
        wl = workloads.talos_c3(B)
        s = loik_amd.BatchedLoik(wl["model"], B, device=device, flags=args.flags, **wl["params"])
        s.SolveInit(wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])
        s.Solve(); s.Solve()
        st = s.stats()
        own_ms = st["tail_ms"] - st["hslots_ms"]
        it = s.get("iter")
        if key == "bulk_rate":
            rate = float(st["instance_iterations"] / (own_ms * 1e-3))
            tf = rate * FLOPS_PER_JOINT_ITERATION * nb / 1e12
            out["bulk_rate"] = {"batch": B, "launch_ms": own_ms, "instance_iterations_per_s": rate, "achieved": tf, "unit": "TFLOP/s",
                                "frac": tf / FP64_VALU_PEAK_TF, "queue_dry_share_of_launch": st["queue_dry_ms"] / own_ms if own_ms > 0 else None}
        else:
            out["lone_instance_us_per_iteration"] = float(own_ms * 1e3 / max(int(it.max()), 1))
            out["lone_instance_note"] = "64 instances, one launch of %.2f ms, longest instance %d iterations" % (own_ms, int(it.max()))
        s.close()
    return out


def two_in_flight_variant(args, device):
    """Reported beside the headline (not `value`): TWO headline batches in flight on the one GPU -- two solver handles, two
    host threads, two streams, different instances -- the way a caller that streams batches would drive it.  The lean launch of
    one batch ends ragged (a few long-running instances keep their workgroups while most of the machine is idle); the other
    batch's launch fills that space.  Per-batch latency is NOT better than the headline's; the sum of solves per second is."""
    from loik_amd import workloads
    import loik_amd
    shards = [Shard(g, device, workloads.talos_c3(args.batch, seed=0x101C + 3 + g), args.flags | loik_amd.capi.OPT_OWN_STREAM,
                    args.max_launch_iters) for g in range(2)]
    steps = max(2, min(args.steps, 3))
    try:
        elapsed = run_shards(shards, steps, 1)
        res = [sh.results() for sh in shards]
    finally:
        for sh in shards:
            sh.close()
    solved = sum(r["solved"] for r in res)
    return {"batches_in_flight": 2, "batch_each": args.batch, "steps_each": steps, "ms_per_pair_of_batches": elapsed / steps * 1e3,
            "value": solved * steps / elapsed, "unit": "solves/s",
            "note": "two independent handles on one device; latency per batch is that of a pair"}


def main(argv=None, solver_factory=None, device_count=None):
    """solver_factory / device_count: test hooks (tests/test_bench_multi_device.py drives the N-device host logic with a
    stand-in solver on a machine without GPUs); the product path leaves them None"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=None, help="instances per GPU (weak) / in total (strong); default 65536 (c3), 131072 per GPU (c4)")
    ap.add_argument("--config", choices=["c3", "c4"], default="c3",
                    help="c3: BASELINE.json's headline (cold Solve() of fresh batches).  c4: BASELINE.json config 4, the sampling-planner workload: "
                         "2^20 instances over 8 GPUs = 131072 per GPU, T = 4 successive targets per instance through the tailored warm-started "
                         "Solve(q, c_id, Ai, bi); a step = one tailored solve of every GPU's share")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-variants", action="store_true", help="skip the whole-body variant reported beside the headline at N = 1")
    ap.add_argument("--no-strong-leg", action="store_true", help="skip the extra strong-scaling measurement at N > 1")
    ap.add_argument("--repeat-batch", action="store_true",
                    help="the timed solves repeat ONE batch on one handle (the reference's timing test, tests/loik-loid.cpp:987-1032): from its "
                         "second solve on the engine takes the batch longest first, by the iteration counts it had the solve before.  Default: "
                         "every timed solve is a handle's FIRST solve of a batch no handle has seen (resident in HBM before the timed region)")
    ap.add_argument("--arrival-order", action="store_true",
                    help="with --repeat-batch: LOIKB_FLAT_ORDER=0, every solve in arrival order")
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--max-launch-iters", type=int, default=0)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the results of the last one to DIR/<name>.npy (float64, at most 64 MB: a fixed, "
                         "seeded sample of the instances when the batch's results are larger)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.batch is None:
        args.batch = HEADLINE_BATCH if args.config == "c3" else 131072
    if args.config == "c4":
        args.no_variants = True          # (the variants belong to the headline configuration)
        args.no_strong_leg = True        # (C4 is defined per GPU share: weak by construction)
        args.scaling = "weak"
    if args.arrival_order:
        os.environ["LOIKB_FLAT_ORDER"] = "0"   # (read once per handle, at loikb_create)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    if world > 1:
        import torch  # noqa: F401
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # the data path has no collective; the process group only carries the timing barrier / max-reduce
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        if args.gpus != world:
            raise SystemExit("--gpus %d disagrees with WORLD_SIZE %d" % (args.gpus, world))

    import loik_amd
    from loik_amd import sharding, workloads

    ndev = loik_amd.device_count() if device_count is None else device_count
    if ndev < 1:
        raise SystemExit("bench.py needs a HIP device (there is no CPU fallback)")
    n_total = args.gpus                      # GPUs of the whole job
    local = [rank] if world > 1 else list(range(n_total))   # global shard indices this process drives
    share_ok = os.environ.get("LOIKB_ALLOW_SHARED_GPU") == "1"

    def device_of(g):
        d = local_rank if world > 1 else g
        if d >= ndev:
            # fewer visible GPUs than shards (only for smoke-testing the multi-device path on a 1-GPU box)
            if not share_ok:
                raise SystemExit("shard %d has no GPU of its own (%d visible); set LOIKB_ALLOW_SHARED_GPU=1 to share" % (g, ndev))
            d = d % ndev
        return d

    def barrier():
        if dist is not None:
            dist.barrier()

    nfresh = 0 if args.repeat_batch else args.steps + args.warmup

    def measure(scaling):
        """build the shards of this process for `scaling`, run W + K steps, aggregate over the job"""
        if args.config == "c4":
            make = lambda g: (lambda: workloads.talos_c4(args.batch, T=4, seed=0x101C + 4 + 17 * g))
            shards = build_shards([(ShardC4, g, device_of(g), make(g), args.flags, args.max_launch_iters, solver_factory) for g in local])
            elapsed = run_shards(shards, args.steps, args.warmup, barrier if dist is not None else None)
            res = [sh.results() for sh in shards]
            cnt = {k: sum(r[k] for r in res) for k in ("solved", "iters", "batch")}
            elapsed, tot = sharding.aggregate(dist, elapsed, cnt)
            return shards, res, elapsed, tot
        if scaling == "weak":
            make = lambda g: (lambda: workloads.talos_c3(args.batch, seed=0x101C + 3 + g))
            fresh = lambda g: (lambda k: workloads.talos_c3(args.batch, seed=0xF5E5 + 1000 * g + k))
        else:
            full = workloads.talos_c3(args.batch, seed=0x101C + 3)  # the 1-GPU workload, split contiguously
            make = lambda g: (lambda: sharding.shard_workload(full, g, n_total))
            fresh = lambda g: (lambda k: sharding.shard_workload(workloads.talos_c3(args.batch, seed=0xF5E5 + k), g, n_total))
        shards = build_shards([(g, device_of(g), make(g), args.flags, args.max_launch_iters, solver_factory, nfresh, fresh(g))
                               for g in local])
        elapsed = run_shards(shards, args.steps, args.warmup, barrier if dist is not None else None)
        res = [sh.results() for sh in shards]
        cnt = {k: sum(r[k] for r in res) for k in ("solved", "iters", "batch")}
        elapsed, tot = sharding.aggregate(dist, elapsed, cnt)
        return shards, res, elapsed, tot

    def gather_chains(shs):
        """every shard's chain_summary on rank 0 (objects through the gloo group: bookkeeping after the timed region, not data path)"""
        mine = [sh.chain_summary(args.steps) for sh in shs if hasattr(sh, "chain_summary")]
        if dist is None:
            return mine
        buf = [None] * world
        dist.all_gather_object(buf, mine)
        return sorted((c for part in buf for c in part), key=lambda c: c["gpu"])

    shards, res, elapsed, tot = measure(args.scaling)
    dumped = dump_outputs(args.dump_outputs, shards, dist) if args.dump_outputs else None
    chains = gather_chains(shards)
    plan0 = shards[0].solver.plan() if hasattr(shards[0].solver, "plan") else None   # which kernels ran, and why
    strong = None
    if args.scaling == "weak" and n_total > 1 and not args.no_strong_leg:
        sh0_keep = (shards[0].acc, shards[0].last, shards[0].wl, shards[0].t_init, res[0])
        for sh in shards[1:]:
            sh.close()
        shards[0].close()
        s_shards, s_res, s_elapsed, s_tot = measure("strong")
        s_chains = gather_chains(s_shards)
        strong = {"per_shard": s_chains,
                  "metric": "IK solves/sec to 1e-6 residual, Talos humanoid, batch=%d in total" % args.batch,
                  "scaling": "strong", "n_gpus": n_total, "batch_total": int(s_tot["batch"]),
                  "batch_per_gpu": int(s_tot["batch"]) // n_total,
                  "value": s_tot["solved"] * args.steps / s_elapsed, "unit": "solves/s",
                  "ms_per_step": s_elapsed / args.steps * 1e3,
                  "instance_iterations_per_s": s_tot["iters"] * args.steps / s_elapsed,
                  "note": "the 65536 instances of the 1-GPU run split contiguously over the GPUs (BASELINE.json: "
                          "'batch=65536 at 1/2/4/8 GPUs'); the ~1000-iteration instances are a serial chain of fixed "
                          "length per batch, so this curve flattens where the weak one does not"}
        for sh in s_shards:
            sh.close()
        acc0, last0, wl0, t_init0, res0 = sh0_keep
    else:
        acc0, last0, wl0, t_init0, res0 = shards[0].acc, shards[0].last, shards[0].wl, shards[0].t_init, res[0]

    if rank == 0:
        model, prm = wl0["model"], wl0["params"]
        nb, nc = model.nv, int(len(wl0["c_ids"]))
        B0 = res0["batch"]
        total_solved, total_iters, total_B = tot["solved"], tot["iters"], tot["batch"]
        per_gpu = args.batch if args.scaling == "weak" else args.batch // n_total
        n_ord = (acc0.get("flat_ordered", 0), args.steps)
        if args.config == "c4":
            schedule_note = ("C4: T = 4 targets per instance, cycled; every step is the tailored warm-started Solve(q_t, c_id, Ai, b_t) of the "
                             "whole share (FwdPassInit of q_t + UpdateEqConstraint + solve), q_t / b_t resident in HBM; arrival order, "
                             "long runners time-sliced inside the launch (the engine's default for 32 768..262 144 instances; "
                             "%d of %d launches ordered)" % n_ord)
        elif nfresh:
            schedule_note = ("every timed solve is a handle's FIRST solve of a batch it has not seen (another seed of the same generator, "
                             "resident in HBM before the timed region; the handle solved one other batch before, as a caller's would have): "
                             "instances in arrival order, long runners time-sliced inside the launch (slices of 288 then 96 iterations: the engine's "
                             "default for launches of 32 768..262 144 instances without an order; same results bit for bit), "
                             "%d of %d launches ordered -- schedule_variant.repeat_same_batch is the "
                             "reference's timing test, one batch again and again, which the engine takes longest first from the second "
                             "solve on" % n_ord)
        else:
            schedule_note = ("--repeat-batch: the timed solves repeat one batch (the reference's timing test); the flat engine took %d of %d "
                             "of them longest first, by the iteration counts of the handle's previous solve" % n_ord)
        line = {
            "csrc_sha16": csrc_sha16(),
            "metric": ("IK solves/sec to 1e-6 residual, Talos humanoid, batch=%d %s" % (
                args.batch, "per GPU" if args.scaling == "weak" else "in total")) if args.config == "c3" else
                      "IK solves/sec to 1e-6 residual, Talos humanoid, %d instances per GPU, tailored warm-started solves (BASELINE config 4)" % args.batch,
            "value": total_solved * args.steps / elapsed,
            "unit": "solves/s",
            "n_gpus": n_total,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": wl0["name"] if args.scaling == "weak" else "talos32_leftwrist_B%d_total_split_%d" % (args.batch, n_total),
                "robot": "talos32 (fixed base, 32 x 1-DoF, Talos topology)",
                "batch_per_gpu": per_gpu,
                "batch_total": int(total_B),
                "task": "6-D velocity task on arm_left_7_joint, A=I, b=J(q) nu*, nu*~U(-0.5,0.5)^32, box +-0.5",
                "stop": "tol_abs=1e-6, tol_rel=0, max_iter=1000, reference fixture rho/mu/scale, adaptive mu (DEFAULT)",
                "parallelism": "%d independent shard(s), no collective; %s" % (
                    n_total, "one process per GPU (torchrun), gloo for the timing barrier only" if world > 1 else
                    "one process, one host thread + handle + stream per GPU"),
                "devices_visible": ndev,
                "shared_gpu_smoke_test": bool(n_total > ndev),
                "solved_fraction": total_solved / total_B,
                "flagged_infeasible_fraction_gpu0": res0["infeasible"] / B0,
                "hit_max_iter_fraction_gpu0": res0["unfinished"] / B0,
                "mean_admm_iterations": total_iters / total_B,
                "instance_iterations_per_s": total_iters * args.steps / elapsed,
                "solve_init_s_gpu0_incl_pcie": t_init0,
                "engines_gpu0": plan0,
                "bench_config": args.config,
                "schedule": schedule_note,
                "spuriously_infeasible_note": "the instances are feasible by construction; `flagged_infeasible_fraction_gpu0` of them trip the "
                                              "reference's primal-infeasibility certificate at tol_primal_inf = 1e-2 (the CPU oracle agrees "
                                              "instance by instance) and are executed and timed but not counted as solves",
                "robot_tables": "synthetic Talos-topology tables (no URDF offline); parity with upstream binaries is unpinned (DESIGN.md 2)",
            },
            "roofline": kernel_roofline(acc0, last0, args.steps, nb, nc, B0),
            # per device: the launch's bulk and the chain of its long runners (lone_chain_ms), so that a run on N GPUs shows which of the
            # two bounds a shard (the chain does not shrink with the shard: DESIGN.md 6)
            "per_shard": chains,
        }
        if dumped is not None:
            line["dump_outputs"] = dumped
        if strong is not None:
            # both legs as objects of their own, so that whichever a reader of the line wants is labelled: the top-level
            # value / ms_per_step are the weak leg's
            line["weak_scaling"] = {"metric": line["metric"], "scaling": "weak", "n_gpus": n_total, "batch_total": int(total_B),
                                    "batch_per_gpu": per_gpu, "value": line["value"], "unit": "solves/s",
                                    "ms_per_step": line["ms_per_step"],
                                    "instance_iterations_per_s": total_iters * args.steps / elapsed}
            line["strong_scaling"] = strong
            # BASELINE.json words the metric as "batch=65536 at 1/2/4/8 GPUs": that is the STRONG leg.  Both values at the top level,
            # each under a name that says which it is; `value` stays the weak leg (the contract's "scaling": "weak")
            line["value_strong"] = strong["value"]
            line["ms_per_step_strong"] = strong["ms_per_step"]
            line["value_weak"] = line["value"]
        if n_total == 1 and not args.no_variants and solver_factory is None:
            try:
                for sh in shards:
                    sh.close()
                line["whole_body_variant"] = whole_body_variant(args, device_of(0))
                # (top-level scalars, so that they survive a reader that keeps the line's first level only: VERDICT r05 #4)
                line["whole_body_ms_per_step"] = line["whole_body_variant"]["ms_per_step"]
                line["whole_body_frac_of_fp64_valu_peak"] = line["whole_body_variant"]["frac_of_fp64_valu_peak"]
            except Exception as e:  # the headline must survive a failing variant
                line["whole_body_variant"] = {"failed": repr(e)}
            try:
                line["single_call_variant"] = single_call_variant(args, device_of(0), wl0)
                line["b1_solve_wall_ms"] = line["single_call_variant"]["b1_solve_wall_ms"]
                line["b1_solve_plus_results_wall_ms"] = line["single_call_variant"]["b1_solve_plus_results_wall_ms"]
                line["b1_full_solve_plus_results_wall_ms"] = line["single_call_variant"]["b1_full_solve_plus_results_wall_ms"]
            except Exception as e:
                line["single_call_variant"] = {"failed": repr(e)}
            try:
                line["schedule_variant"] = schedule_variant(args, device_of(0))
            except Exception as e:
                line["schedule_variant"] = {"failed": repr(e)}
            try:   # (top-level scalars: what a caller with ONE handle and new problems gets -- VERDICT r04 #6)
                oh = line["schedule_variant"]["another_batch_every_solve"]
                line["value_one_handle"] = oh["value"]
                line["ms_per_step_one_handle"] = oh["ms_per_step"]
                line["ms_per_step_one_handle_after_idle_gap"] = line["schedule_variant"]["another_batch_every_solve_after_idle_gap"]["ms_per_step"]
            except Exception:
                pass
            try:
                rp = line["schedule_variant"]["repeat_same_batch"]
                line["roofline"]["repeat_same_batch"] = {"avg_launch_ms": rp["kernel_avg_launch_ms"], "achieved": rp["kernel_achieved_TFLOPs"],
                                                         "frac": rp["kernel_frac_of_fp64_valu_peak"],
                                                         "note": "the same kernel when a handle solves one batch again and again (longest first)"}
            except Exception:
                pass
            try:
                line["roofline"].update(regimes_variant(args, device_of(0), nb))
            except Exception as e:
                line["roofline"]["regimes_failed"] = repr(e)
            try:
                line["fp32_tradeoff_variant"] = fp32_tradeoff_variant(args, device_of(0))
            except Exception as e:
                line["fp32_tradeoff_variant"] = {"failed": repr(e)}
            try:
                line["two_batches_in_flight_variant"] = two_in_flight_variant(args, device_of(0))
            except Exception as e:
                line["two_batches_in_flight_variant"] = {"failed": repr(e)}
        if n_total == 1 and not args.no_cpu_baseline:
            try:
                line["cpu_baseline"] = cpu_baseline(wl0)
            except Exception as e:  # the GPU number must survive a broken host toolchain
                line["cpu_baseline"] = {"value": None, "unit": "solves/s", "cores": effective_cpus()[0], "kind": "port",
                                        "sample": "failed: %r" % (e,)}
        print(json.dumps(line), flush=True)
        ret = line
    else:
        ret = None
    if strong is None:
        for sh in shards:
            sh.close()  # (idempotent)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return ret


if __name__ == "__main__":
    main()
