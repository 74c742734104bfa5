// loik_host_pose.hpp -- the pose layer of the host driver: batched pose IK (include/loik_amd_pose.h), joint position limits
// (loik_amd_limits.h) and acceleration limits (loik_amd_accel.h), step control (loik_amd_step.h), tool frames and tasks (loik_amd_tasks.h), frame
// Jacobians and dexterity (loik_amd_jacobian.h), collision clearance (loik_amd_collision.h), voxel worlds (loik_amd_grid.h, loik_amd_gridnear.h), collision avoidance (loik_amd_avoid.h), multi-start (loik_amd_multistart.h), waypoint paths
// (loik_amd_path.h) and timed trajectories (loik_amd_track.h).  Included at the end of loik_host.hip, whose translation unit it
// belongs to: it is no header of its own.  The motion layer (loik_amd_motion.h, _shortcut.h, _retime.h, _blend.h, _plan.h) follows it in
// loik_host_motion.hpp.
//
// What the solves share is here once: pose_check_targets (the check before anything of the handle changes), pose_begin,
// pose_loop (the step loop around the caller's re-target) with pose_step, get_copy_out / get_timing_out for the getters of resident
// results, and for the queries QueryOut (where their outputs land, and their failure path) with the launch-shape rules lds_waves,
// regrow_drained and clr_model.

// ---- batched pose IK (include/loik_amd_pose.h, kernels in loik_pose.hpp) ---------------------------------------------------
static int pose_alloc(loikb_solver_impl* S)
{
  loikb_solver_impl::PoseState& P = S->pose;
  if (P.d_tgt) return LOIKB_OK;
  const size_t B = (size_t)S->B, nc = (size_t)std::max(S->nc, 1);
  int rc;
  if ((rc = alloc_dev(S, (void**)&P.d_tgt, sizeof(double) * B * nc * 12)) || (rc = alloc_dev(S, (void**)&P.d_b, sizeof(double) * B * nc * 6)) ||
      (rc = alloc_dev(S, (void**)&P.d_err, sizeof(double) * B * nc * 6)) || (rc = alloc_dev(S, (void**)&P.d_A, sizeof(double) * nc * 36)) ||
      (rc = alloc_dev(S, (void**)&P.d_status, sizeof(int) * B)) || (rc = alloc_dev(S, (void**)&P.d_steps, sizeof(int) * B)) ||
      (rc = alloc_dev(S, (void**)&P.d_clink, sizeof(int) * nc)) || (rc = alloc_dev(S, (void**)&P.d_count, sizeof(unsigned int) * 2))) {
    P.d_tgt = nullptr;   // (what was allocated stays in `allocs` and goes with the handle; the next call allocates afresh)
    return rc;
  }
  return LOIKB_OK;
}

// ---- joint position limits (include/loik_amd_limits.h) --------------------------------------------------------------------
// buffers of a pose solve with limits; the [nb][B] copy of the base box only for a handle whose box is per instance
static int pose_limits_alloc(loikb_solver_impl* S, bool need_box)
{
  loikb_solver_impl::PoseState& P = S->pose;
  const size_t n = (size_t)S->B * S->nb;
  int rc;
  if (!P.d_lflags && (rc = alloc_dev(S, (void**)&P.d_lflags, sizeof(int) * n))) return rc;
  if (!P.d_inrange && (rc = alloc_dev(S, (void**)&P.d_inrange, n))) return rc;
  if (need_box && !P.d_box && (rc = alloc_dev(S, (void**)&P.d_box, sizeof(double2) * n))) return rc;
  return LOIKB_OK;
}

// ... and of one with acceleration limits (include/loik_amd_accel.h): the velocity state
static int pose_accel_alloc(loikb_solver_impl* S)
{
  loikb_solver_impl::PoseState& P = S->pose;
  if (P.d_zp) return LOIKB_OK;
  return alloc_dev(S, (void**)&P.d_zp, sizeof(double) * (size_t)S->B * S->nb);
}

// ... and of one with step control (include/loik_amd_step.h): the trial rows and the per-instance counters
static int pose_step_alloc(loikb_solver_impl* S)
{
  loikb_solver_impl::PoseState& P = S->pose;
  if (P.d_frun) return LOIKB_OK;
  const size_t B = (size_t)S->B;
  int rc;
  if ((rc = alloc_dev(S, (void**)&P.d_trial, sizeof(double) * B * S->nq)) || (rc = alloc_dev(S, (void**)&P.d_alpha, sizeof(double) * B)) ||
      (rc = alloc_dev(S, (void**)&P.d_backtracks, sizeof(int) * B)) || (rc = alloc_dev(S, (void**)&P.d_failed, sizeof(int) * B)) ||
      (rc = alloc_dev(S, (void**)&P.d_frun, sizeof(int) * B))) {
    P.d_frun = nullptr;   // (as pose_alloc: what was allocated goes with the handle; the next call allocates afresh)
    return rc;
  }
  return LOIKB_OK;
}

static dim3 grid_dof(const loikb_solver_impl* S) { return dim3((unsigned)((S->B + 255) / 256), (unsigned)S->nb); }

// JP_LBUB of the home tiles <-> PoseState::d_box
static int pose_box_copy(loikb_solver_impl* S, int restore)
{
  with_real(S, [&](auto t) {
    hipLaunchKernelGGL(k_box_copy<decltype(t)>, grid_dof(S), dim3(256), 0, S->stream, S->home.tiles, S->L, S->B, S->pose.d_box, restore);
  });
  HIPCHK(hipGetLastError());
  return LOIKB_OK;
}

// The handle while a pose solve with limits (position, acceleration or both) or with collision avoidance runs: per-instance-box mode (every engine, the compaction's move_bounds and the
// pass-level path read S->bnd_shared when a solve is launched: make_params in run_chunk, compact, pass_params), the base box
// kept in the uniform buffer (shared) or in d_box (per instance).  Leaving the scope puts the base box back in force in the
// mode it had, on every return path.
struct PoseBoxScope {
  loikb_solver_impl* S;
  bool active = false, was_shared = false;
  int enter()
  {
    was_shared = S->bnd_shared;
    int rc;
    if ((rc = pose_limits_alloc(S, !was_shared))) return rc;
    if (!was_shared && (rc = pose_box_copy(S, 0))) return rc;
    S->bnd_shared = false;
    active = true;
    return LOIKB_OK;
  }
  int leave()
  {
    if (!active) return LOIKB_OK;
    active = false;
    S->bnd_shared = was_shared;
    S->pass_active = false;
    ++S->inputs_epoch;
    return was_shared ? LOIKB_OK : pose_box_copy(S, 1);
  }
  ~PoseBoxScope() { if (active) { (void)leave(); (void)hipStreamSynchronize(S->stream); } }
};

// (collision avoidance, loik_amd_avoid.h: defined beside the collision block below)
static int avoid_begin(loikb_solver_impl* S);
static int avoid_step(loikb_solver_impl* S, double dt, const PoseBoxScope& box, const int* d_status, bool from_tiles);

// what every pose loop does between pose_begin and its first step: with either kind of limit or the avoidance latch on the handle,
// into the scope, the limit flags start at 0 and the avoidance results are reset
static int pose_box_begin(loikb_solver_impl* S, PoseBoxScope& box)
{
  loikb_solver_impl::PoseState& P = S->pose;
  if (!P.have_limits && !P.have_accel && !P.avoid.have) { P.avoid.valid = false; return LOIKB_OK; }
  int rc;
  if ((rc = box.enter())) return rc;
  HIPCHK(hipMemsetAsync(P.d_lflags, 0, sizeof(int) * (size_t)S->B * S->nb, S->stream));
  if (P.avoid.have) return avoid_begin(S);   // (the results of the last latched loop stand until this one has reset them)
  P.avoid.valid = false;
  return LOIKB_OK;
}

static double ms_since(std::chrono::steady_clock::time_point t0)
{
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// `n` placements [12] of the caller (`dev`: on the device) into `staging`, and the check every pose solve makes before anything
// of the handle changes: `message` and LOIKB_ERR_ARG if one of them is not finite or its rotation not orthonormal with
// determinant 1.  `d_count`: two counters of the caller's state.
static int pose_check_targets(loikb_solver_impl* S, double* staging, const double* src, size_t n, bool dev, unsigned int* d_count,
                              const char* message)
{
  HIPCHK(hipMemcpyAsync(staging, src, sizeof(double) * 12 * n, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, S->stream));
  HIPCHK(hipMemsetAsync(d_count, 0, 2 * sizeof(unsigned int), S->stream));
  hipLaunchKernelGGL(k_pose_check_targets, grid1(n), dim3(256), 0, S->stream, (const double*)staging, (int)n, 1e-9, d_count + 1);
  HIPCHK(hipGetLastError());
  unsigned int counts[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(counts, d_count, sizeof(counts), hipMemcpyDeviceToHost, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));
  if (counts[1]) { g_last_error = message; return LOIKB_ERR_ARG; }
  return LOIKB_OK;
}

// The tail of a getter: `bytes` from the device buffer `src` to `out` (host, or device with LOIKB_OUT_DEVICE), complete on return
static int get_copy_out(loikb_solver_impl* S, const void* src, size_t bytes, void* out, int out_flags)
{
  HIPCHK(hipMemcpyAsync(out, src, bytes, (out_flags & LOIKB_OUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));
  return LOIKB_OK;
}

// ... and of a TIMING field, which lives on the host
static int get_timing_out(const double* timing, size_t nbytes, void* out, bool to_dev)
{
  if (!to_dev) { memcpy(out, timing, nbytes); return LOIKB_OK; }
  HIPCHK(hipMemcpy(out, timing, nbytes, hipMemcpyHostToDevice));
  return LOIKB_OK;
}

// The outputs of a query call.  add() declares them in the order the scratch holds them (unpadded: every caller's doubles come
// before its ints) and names where the kernel writes each: the caller's array itself with LOIKB_OUT_DEVICE, else a slice of
// S->d_getscr[0], which reserve() grows once, for all of them, before it hands any slice out.  A NULL array is an output the caller
// does not want: a NULL device pointer on both routes, and no scratch.  finish() queues the copies to the caller's host arrays and
// drains the stream.  The scope is the failure path of the call as well: it opens before the call queues anything that reads the
// caller's memory, and every return that is not a finish() that went through drains the stream.
class QueryOut {
 public:
  QueryOut(loikb_solver_impl* S, int out_flags) : S_(S), to_dev_(out_flags & LOIKB_OUT_DEVICE) {}
  QueryOut(const QueryOut&) = delete;
  QueryOut& operator=(const QueryOut&) = delete;
  ~QueryOut() { if (!done_) (void)hipStreamSynchronize(S_->stream); }

  template <class T> void add(T* user, size_t bytes, T** dev)
  {
    *dev = user;
    if (user && !to_dev_) o_[n_++] = Item{user, bytes, dev, [](void* slot, void* p) { *static_cast<T**>(slot) = static_cast<T*>(p); }};
  }
  int reserve()
  {
    if (n_ == 0) return LOIKB_OK;
    size_t total = 0;
    for (int i = 0; i < n_; ++i) total += o_[i].bytes;
    if (int rc = regrow(S_->d_getscr[0], total)) return rc;
    char* p = S_->d_getscr[0].as<char>();
    for (int i = 0; i < n_; p += o_[i++].bytes) o_[i].set(o_[i].slot, p);
    return LOIKB_OK;
  }
  int finish()
  {
    const char* p = S_->d_getscr[0].as<char>();
    for (int i = 0; i < n_; p += o_[i++].bytes) HIPCHK(hipMemcpyAsync(o_[i].user, p, o_[i].bytes, hipMemcpyDeviceToHost, S_->stream));
    HIPCHK(hipStreamSynchronize(S_->stream));
    done_ = true;
    return LOIKB_OK;
  }

 private:
  struct Item { void* user; size_t bytes; void* slot; void (*set)(void* slot, void* p); };
  loikb_solver_impl* S_;
  bool to_dev_, done_ = false;
  Item o_[7];
  int n_ = 0;
};

// the largest power-of-two number of wavefronts, at most `max`, whose `per` bytes each fit the 64 KB of LDS of a workgroup (1 where not
// even one does: the caller's case)
static int lds_waves(int max, size_t per)
{
  int waves = max;
  while (waves > 1 && waves * per > 65536) waves >>= 1;
  return waves;
}

// `buf` grown to `need` bytes (OwnedBuf::regrow: never shrunk, the contents not kept).  What is queued may still use the buffer that
// goes: the stream is drained first
template <class Buf> static int regrow_drained(loikb_solver_impl* S, Buf& buf, size_t need)
{
  if (need <= buf.bytes()) return LOIKB_OK;
  HIPCHK(hipStreamSynchronize(S->stream));
  return regrow(buf, need);
}

// iMf [12] = (R row-major, p): finite, R orthonormal with determinant 1 within 1e-9 per entry (k_pose_check_targets' rule)
static bool frame_ok(const double* F)
{
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(F[k])) return false;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double g = F[a] * F[b] + F[3 + a] * F[3 + b] + F[6 + a] * F[6 + b] - (a == b ? 1.0 : 0.0);
      if (!(std::fabs(g) <= 1e-9)) return false;
    }
  const double det = F[0] * (F[4] * F[8] - F[5] * F[7]) - F[1] * (F[3] * F[8] - F[5] * F[6]) + F[2] * (F[3] * F[7] - F[4] * F[6]);
  return std::fabs(det - 1.0) <= 1e-9;
}

// what the getters of placements, Jacobians and dexterity ask of (links, frames) given by the caller; `fn` goes into loikb_last_error()
static int jac_check_entries(const loikb_solver_impl* S, const char* fn, const int* links, const double* frames, int n)
{
  for (int e = 0; e < n; ++e) {
    if (links[e] < 0 || links[e] >= S->ext_nj) { g_last_error = std::string(fn) + ": link id out of range"; return LOIKB_ERR_ARG; }
    if (frames && !frame_ok(frames + 12 * e)) {
      g_last_error = std::string(fn) + ": a frame needs a finite translation and a rotation that is orthonormal with determinant 1 (tolerance 1e-9)";
      return LOIKB_ERR_ARG;
    }
  }
  return LOIKB_OK;
}

// ... and the device joints of those links
static std::vector<int> device_links(const loikb_solver_impl* S, const int* links, int n)
{
  std::vector<int> dl(n);
  for (int e = 0; e < n; ++e) dl[e] = S->link_of[links[e]];
  return dl;
}

// scratch 1 of those getters: the frames [n][12], then the device joints [n], then (d_rows != NULL) room for the row masks [n], which
// `rows` fills when given; queued
static int jac_stage_entries(loikb_solver_impl* S, const int* dl, const double* fr, const int* rows, int n, double** d_fr, int** d_dl, int** d_rows)
{
  const size_t fbytes = sizeof(double) * (size_t)n * 12, ibytes = sizeof(int) * (size_t)n;
  int rc;
  if ((rc = regrow(S->d_getscr[1], fbytes + (d_rows ? 2 : 1) * ibytes))) return rc;
  *d_fr = S->d_getscr[1].as<double>();
  *d_dl = (int*)(S->d_getscr[1].as<char>() + fbytes);
  if (d_rows) *d_rows = *d_dl + n;
  HIPCHK(hipMemcpyAsync(*d_fr, fr, fbytes, hipMemcpyHostToDevice, S->stream));
  HIPCHK(hipMemcpyAsync(*d_dl, dl, ibytes, hipMemcpyHostToDevice, S->stream));
  if (rows) HIPCHK(hipMemcpyAsync(*d_rows, rows, ibytes, hipMemcpyHostToDevice, S->stream));
  return LOIKB_OK;
}

// what loikb_solve_pose asks of its parameters and of the handle before it looks at the targets (loikb_solve_pose_multistart asks
// the same before it changes anything)
static int pose_preconditions(const loikb_solver_impl* S, const loikb_pose_params* p, bool need_resident_q)
{
  if (!(p->dt > 0.0) || !(p->gain > 0.0) || !(p->tol_pose >= 0.0) || p->max_steps < 0 || std::isinf(p->dt) || std::isinf(p->gain)) {
    g_last_error = "solve_pose: need dt > 0, gain > 0, tol_pose >= 0, max_steps >= 0";
    return LOIKB_ERR_ARG;
  }
  if (!S->have_problem) { g_last_error = "solve_pose before SolveInit()"; return LOIKB_ERR_STATE; }
  if (S->nc_active < 1) { g_last_error = "solve_pose: no active task constraint"; return LOIKB_ERR_STATE; }
  if (need_resident_q && !S->have_q) { g_last_error = "solve_pose: no configurations resident on the device yet"; return LOIKB_ERR_STATE; }
  return LOIKB_OK;
}

// The head of a pose loop once its targets are accepted (loikb_solve_pose, loikb_solve_pose_path): q replaces the resident
// configurations, the constraint links and the shared A go to the device, status and steps start at 0.
static int pose_begin(loikb_solver_impl* S, const double* q, bool dev)
{
  loikb_solver_impl::PoseState& P = S->pose;
  const int B = S->B, nc = S->nc_active;
  int rc;
  if (q) {   // (the copy path of k_advance_q: the resident configurations are replaced; FwdPassInit runs in the first solve)
    const void* dq = nullptr;
    if ((rc = to_device(S, q, sizeof(double) * (size_t)B * S->nq, dev, &dq))) return rc;
    with_real(S, [&](auto t) {
      hipLaunchKernelGGL(k_advance_q<decltype(t)>, grid1(B), dim3(256), 0, S->stream, S->d_q, (const double*)dq, 0, S->nq, S->d_jd, S->d_idx_q, S->L, B, S->home.tiles, 0.0);
    });
    HIPCHK(hipGetLastError());
    S->have_q = true;
  }
  std::vector<int> cl(nc);
  for (int c = 0; c < nc; ++c) cl[c] = S->link_of[S->active_ids[c]];
  HIPCHK(hipMemcpyAsync(P.d_clink, cl.data(), sizeof(int) * nc, hipMemcpyHostToDevice, S->stream));
  if (S->a_shared) HIPCHK(hipMemcpyAsync(P.d_A, S->A_host.data(), sizeof(double) * 36 * nc, hipMemcpyHostToDevice, S->stream));
  HIPCHK(hipMemsetAsync(P.d_status, 0, sizeof(int) * B, S->stream));
  HIPCHK(hipMemsetAsync(P.d_steps, 0, sizeof(int) * B, S->stream));
  if (P.have_accel) {   // the velocity state of the first step: the latched start velocity, else rest
    if ((rc = pose_accel_alloc(S))) return rc;
    hipLaunchKernelGGL(k_accel_load_v0, grid_dof(S), dim3(256), 0, S->stream, P.have_v0 ? (const double*)P.d_v0 : nullptr, B, S->nb, P.d_zp);
    HIPCHK(hipGetLastError());
  }
  if (P.have_step) {   // the counters of loik_amd_step.h and the run of failed searches start at 0
    if ((rc = pose_step_alloc(S))) return rc;
    HIPCHK(hipMemsetAsync(P.d_alpha, 0, sizeof(double) * B, S->stream));
    HIPCHK(hipMemsetAsync(P.d_backtracks, 0, sizeof(int) * B, S->stream));
    HIPCHK(hipMemsetAsync(P.d_failed, 0, sizeof(int) * B, S->stream));
    HIPCHK(hipMemsetAsync(P.d_frun, 0, sizeof(int) * B, S->stream));
  }
  HIPCHK(hipStreamSynchronize(S->stream));   // (q, cl are the caller's / locals)
  P.nc = nc;
  P.step_valid = P.have_step;
  P.flags_valid = P.have_limits || P.have_accel;
  P.vel_valid = P.have_accel;
  P.vel_status = nullptr;
  P.have_v0 = false;   // (used or not: the latch is for the next pose loop alone)
  return LOIKB_OK;
}

// One step of a pose loop after its re-target left b_c in P.d_b: the step's box (limits), the b edits, the tailored Solve, the
// integrate, the clamp and (acceleration limits) the keep of the applied z.  `d_status`: the word whose POSE_REACHED / POSE_STOPPED bits say which instances run (P.d_status for
// loikb_solve_pose, the loop-private word for loikb_solve_pose_path).  `sc`: the loop runs with step control (loik_amd_step.h) and
// this is what its re-target ran with; the integrate and the clamp are then k_pose_step_control's.
struct PoseStepTargets {
  const double* tgt;   // [B][nc][12], or the first nc rows with `shared`
  int shared;
  const PoseTask* tasks;   // nullptr: the joint frames
};

static int pose_step(loikb_solver* S, const loikb_pose_params* p, const PoseBoxScope& box, int* d_status, double* solve_ms,
                     const PoseStepTargets* sc = nullptr)
{
  loikb_solver_impl::PoseState& P = S->pose;
  const int B = S->B, nc = S->nc_active;
  int rc = LOIKB_OK;
  if (box.active && P.have_accel) {   // the step's box by the rule of loik_amd_accel.h, from the resident q and the last velocity
    with_real(S, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(k_pose_dyn_box<T>, grid_dof(S), dim3(256), 0, S->stream, (const double*)S->d_q, S->nq,
                         P.have_limits ? (const PoseLimit*)P.d_lim : nullptr, (const double*)P.d_amax, (const double*)P.d_zp, B, p->dt,
                         (const int*)d_status, box.was_shared ? (const T*)S->d_uni + S->nc * 57 : nullptr, (const double2*)P.d_box,
                         S->home.tiles, S->L, P.d_lflags, P.d_inrange);
    });
    HIPCHK(hipGetLastError());
  } else if (box.active && P.have_limits) {   // the step's velocity box from the resident q (the base box for the instances that no longer run)
    with_real(S, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(k_pose_limit_box<T>, grid_dof(S), dim3(256), 0, S->stream, (const double*)S->d_q, S->nq, (const PoseLimit*)P.d_lim, B,
                         p->dt, (const int*)d_status, box.was_shared ? (const T*)S->d_uni + S->nc * 57 : nullptr, (const double2*)P.d_box,
                         S->home.tiles, S->L, P.d_lflags, P.d_inrange);
    });
    HIPCHK(hipGetLastError());
  }
  // collision avoidance (loik_amd_avoid.h): the interval the kernels above left, or the base box, narrowed from the resident q
  if (box.active && P.avoid.have && (rc = avoid_step(S, p->dt, box, d_status, P.have_limits || P.have_accel))) return rc;
  // UpdateEqConstraint(c, NULL, b_c, LOIKB_IN_DEVICE) for every active constraint, queued behind each other (the solve below
  // synchronises), then the tailored Solve on the resident q without a constraint rewrite
  S->defer_sync = true;
  for (int c = 0; c < nc && rc == LOIKB_OK; ++c) rc = update_eq_single(S, S->active_ids[c], nullptr, P.d_b + (size_t)c * B * 6, LOIKB_IN_DEVICE);
  S->defer_sync = false;
  if (rc) { (void)hipStreamSynchronize(S->stream); return rc; }
  S->pass_active = false;
  const auto t_solve = std::chrono::steady_clock::now();
  if ((rc = loikb_solve_tailored(S, nullptr, -1, nullptr, nullptr, 0))) return rc;
  *solve_ms += ms_since(t_solve);
  if (sc) {
    const StepCtl ctl{P.step.shrink, P.step.sufficient, P.step.max_backtracks, P.step.patience};
    const bool clamp = box.active && P.have_limits;
    with_real(S, [&](auto t) {
      hipLaunchKernelGGL(k_pose_step_control<decltype(t)>, grid1(B), dim3(256), 0, S->stream, S->d_q, S->nq, S->d_jd, S->d_idx_q, S->L, B,
                         (const char*)S->home.tiles, p->dt, (const int*)P.d_clink, nc, sc->tasks, sc->tgt, sc->shared, (const double*)P.d_err,
                         clamp ? (const PoseLimit*)P.d_lim : nullptr, clamp ? (const unsigned char*)P.d_inrange : nullptr, ctl, P.d_trial,
                         d_status, P.d_steps, P.d_alpha, P.d_backtracks, P.d_failed, P.d_frun);
    });
    HIPCHK(hipGetLastError());
    ++S->inputs_epoch;
    return LOIKB_OK;
  }
  with_real(S, [&](auto t) {
    hipLaunchKernelGGL(k_pose_integrate<decltype(t)>, grid1(B), dim3(256), 0, S->stream, S->d_q, S->nq, S->d_jd, S->d_idx_q, S->L, B,
                       (const char*)S->home.tiles, p->dt, d_status);
  });
  HIPCHK(hipGetLastError());
  if (box.active && P.have_limits) {
    hipLaunchKernelGGL(k_pose_limit_clamp, grid_dof(S), dim3(256), 0, S->stream, S->d_q, S->nq, (const PoseLimit*)P.d_lim, B,
                       (const unsigned char*)P.d_inrange);
    HIPCHK(hipGetLastError());
  }
  if (box.active && P.have_accel) {   // zp of the next step (the integrate read the same z; it changes neither the tiles nor who runs)
    with_real(S, [&](auto t) {
      hipLaunchKernelGGL(k_accel_keep_z<decltype(t)>, grid_dof(S), dim3(256), 0, S->stream, (const char*)S->home.tiles, S->L, B,
                         (const int*)d_status, P.d_zp);
    });
    HIPCHK(hipGetLastError());
    P.vel_status = d_status;
  }
  ++S->inputs_epoch;
  return LOIKB_OK;
}

static int pose_no_after_step() { return LOIKB_OK; }

// The step loop of a pose solve after pose_begin, and its end.  retarget(go) queues the caller's re-target of the resident q
// (go = 0: the last one, which only judges), which leaves b_c in P.d_b and the count of running instances in P.d_count[0];
// the loop reads that count back, stops at 0 and otherwise runs pose_step on `d_status`, then after_step() (what the caller
// queues behind a step: loikb_track_pose its record).  Then the base box is back in force, the stream is drained and P.timing
// holds {steps, total since t_call, inner solves, the rest} in ms.  `sc`: pose_step's.
template <class Retarget, class AfterStep = int (&)()>
static int pose_loop(loikb_solver* S, const loikb_pose_params* p, PoseBoxScope& box, int* d_status,
                     std::chrono::steady_clock::time_point t_call, Retarget&& retarget, AfterStep&& after_step = pose_no_after_step,
                     const PoseStepTargets* sc = nullptr)
{
  loikb_solver_impl::PoseState& P = S->pose;
  double solve_ms = 0.0;
  int steps_run = 0, rc;
  for (int step = 0;; ++step) {
    const int go = step < p->max_steps;
    HIPCHK(hipMemsetAsync(P.d_count, 0, sizeof(unsigned int), S->stream));
    if ((rc = retarget(go))) return rc;
    if (!go) break;
    unsigned int running = 0;
    HIPCHK(hipMemcpyAsync(&running, P.d_count, sizeof(running), hipMemcpyDeviceToHost, S->stream));
    HIPCHK(hipStreamSynchronize(S->stream));
    if (running == 0) break;
    if ((rc = pose_step(S, p, box, d_status, &solve_ms, sc)) || (rc = after_step())) return rc;
    ++steps_run;
  }
  if ((rc = box.leave())) return rc;
  HIPCHK(hipStreamSynchronize(S->stream));
  const double total = ms_since(t_call);
  P.timing[0] = steps_run; P.timing[1] = total; P.timing[2] = solve_ms; P.timing[3] = total - solve_ms;
  return LOIKB_OK;
}

extern "C" {

int loikb_pose_version(void) { return LOIKB_POSE_VERSION; }

int loikb_forward_kinematics(loikb_solver* S, const int* links, int n, double* out, int out_flags)
{
  if (!S || n < 0 || (n > 0 && (!links || !out))) return LOIKB_ERR_ARG;
  int rc;
  if ((rc = jac_check_entries(S, "forward_kinematics", links, nullptr, n))) return rc;
  if (!S->have_q) { g_last_error = "forward_kinematics: no configurations resident on the device yet"; return LOIKB_ERR_STATE; }
  if (n == 0) return LOIKB_OK;
  HIPCHK(hipSetDevice(S->device));
  const std::vector<int> dl = device_links(S, links, n);
  QueryOut o(S, out_flags);
  double* dst;
  o.add(out, sizeof(double) * (size_t)S->B * n * 12, &dst);
  if ((rc = regrow(S->d_getscr[1], sizeof(int) * (size_t)n)) || (rc = o.reserve())) return rc;
  HIPCHK(hipMemcpyAsync(S->d_getscr[1], dl.data(), sizeof(int) * n, hipMemcpyHostToDevice, S->stream));
  hipLaunchKernelGGL(k_link_placements, grid1((size_t)S->B * n), dim3(256), 0, S->stream, (const double*)S->d_q, S->nq, S->d_jd,
                     S->d_idx_q, S->d_getscr[1].as<const int>(), n, S->B, dst);
  HIPCHK(hipGetLastError());
  return o.finish();   // (dl is a local)
}

int loikb_solve_pose(loikb_solver* S, const double* q, const double* targets, int in_flags, const loikb_pose_params* p)
{
  if (!S || !targets || !p) return LOIKB_ERR_ARG;
  if (int pre = pose_preconditions(S, p, !q)) return pre;
  if (S->pose.have_step && S->pose.have_accel) {
    g_last_error = "solve_pose: the handle has both step control (loikb_pose_set_step_control) and joint acceleration limits (loikb_set_joint_accel_limits); a scaled step is not the velocity the braking box was built for -- clear one of them first";
    return LOIKB_ERR_STATE;
  }
  const auto t_call = std::chrono::steady_clock::now();
  HIPCHK(hipSetDevice(S->device));
  int rc;
  if ((rc = pose_alloc(S))) return rc;
  loikb_solver_impl::PoseState& P = S->pose;
  const int B = S->B, nc = S->nc_active;
  const bool dev = in_flags & LOIKB_IN_DEVICE, tgt_shared = in_flags & LOIKB_POSE_TARGET_SHARED;
  // the targets, checked before anything of the handle changes
  if ((rc = pose_check_targets(S, P.d_tgt, targets, (size_t)(tgt_shared ? 1 : B) * nc, dev, P.d_count,
                               "solve_pose: a target rotation is not orthonormal with determinant 1 (tolerance 1e-9)")))
    return rc;
  ++S->inputs_epoch;
  if ((rc = pose_begin(S, q, dev))) return rc;
  PoseBoxScope box{S};
  if ((rc = pose_box_begin(S, box))) return rc;
  const double k = p->gain / p->dt;
  const PoseStepTargets sc{(const double*)P.d_tgt, (int)tgt_shared, P.have_tasks ? (const PoseTask*)P.d_tasks : nullptr};
  return pose_loop(S, p, box, P.d_status, t_call, [&](int go) -> int {
    if (P.have_tasks)   // (loik_amd_tasks.h: the task-frame error by kind, b = k S e; needs neither the tiles nor A)
      hipLaunchKernelGGL(k_pose_retarget_tasks, grid1(B), dim3(256), 0, S->stream, (const double*)S->d_q, S->nq, S->d_jd, S->d_idx_q,
                         (const int*)P.d_clink, nc, (const PoseTask*)P.d_tasks, (const double*)P.d_tgt, (int)tgt_shared, B, k,
                         p->tol_pose, go, P.d_b, P.d_err, P.d_status, P.d_steps, P.d_count);
    else
      with_real(S, [&](auto t) {
        hipLaunchKernelGGL(k_pose_retarget<decltype(t)>, grid1(B), dim3(256), 0, S->stream, (const double*)S->d_q, S->nq, S->d_jd, S->d_idx_q,
                           (const int*)P.d_clink, nc, (const double*)P.d_tgt, (int)tgt_shared, S->a_shared ? (const double*)P.d_A : nullptr,
                           (const char*)S->home.tiles, S->L, B, k, p->tol_pose, go, P.d_b, P.d_err, P.d_status, P.d_steps, P.d_count);
      });
    HIPCHK(hipGetLastError());
    return LOIKB_OK;
  }, pose_no_after_step, P.have_step ? &sc : nullptr);
}

int loikb_pose_get(loikb_solver* S, int field, void* out, int out_flags)
{
  if (!S || !out) return LOIKB_ERR_ARG;
  if (S->pose.nc == 0) { g_last_error = "pose_get before solve_pose"; return LOIKB_ERR_STATE; }
  HIPCHK(hipSetDevice(S->device));
  const void* src = nullptr;
  size_t bytes = 0;
  switch (field) {
  case LOIKB_POSE_F_STEPS: src = S->pose.d_steps; bytes = sizeof(int) * (size_t)S->B; break;
  case LOIKB_POSE_F_STATUS: src = S->pose.d_status; bytes = sizeof(int) * (size_t)S->B; break;
  case LOIKB_POSE_F_ERR: src = S->pose.d_err; bytes = sizeof(double) * (size_t)S->B * S->pose.nc * 6; break;
  case LOIKB_POSE_F_TIMING: return get_timing_out(S->pose.timing, sizeof(S->pose.timing), out, out_flags & LOIKB_OUT_DEVICE);
  default: g_last_error = "pose_get: unknown field"; return LOIKB_ERR_ARG;
  }
  return get_copy_out(S, src, bytes, out, out_flags);
}

// ---- include/loik_amd_limits.h ----------------------------------------------------------------------------------------------
int loikb_limits_version(void) { return LOIKB_LIMITS_VERSION; }

// The rule of a per-DoF pair (lo, hi) [nv] in idx_v order, shared by loikb_set_joint_limits and loikb_multistart_set_ranges
// (loik_amd_multistart.h): both pointers given, n == nv, no NaN, lo <= hi, and a finite entry only on a DoF whose coordinate a
// plain sum advances (S->lim_q).  `fn`, `lo_name`, `hi_name` go into loikb_last_error().
static int check_dof_pairs(const loikb_solver_impl* S, const char* fn, const char* lo_name, const char* hi_name, const double* lo, const double* hi, int n)
{
  const std::string f(fn), ln(lo_name), hn(hi_name);
  if (!lo || !hi) { g_last_error = f + ": " + ln + " and " + hn + " must both be given, or both be NULL (clear)"; return LOIKB_ERR_ARG; }
  if (n != S->nv) { g_last_error = f + ": need one (" + ln + ", " + hn + ") pair per DoF, n == model.nv"; return LOIKB_ERR_ARG; }
  for (int j = 0; j < n; ++j) {
    char what[96];
    snprintf(what, sizeof(what), "%s: DoF %d (joint %d)", fn, j, S->dof_ext[j]);
    if (std::isnan(lo[j]) || std::isnan(hi[j])) { g_last_error = std::string(what) + ": a limit is NaN"; return LOIKB_ERR_ARG; }
    if (lo[j] > hi[j]) { g_last_error = std::string(what) + ": " + ln + " > " + hn; return LOIKB_ERR_ARG; }
    const bool finite = std::isfinite(lo[j]) || std::isfinite(hi[j]);
    if (finite && S->lim_q[j] < 0) {
      const int jt = S->dof_jt[j];
      const char* kind = jt == LOIKB_J_FREEFLYER ? "free-flyer" : jt == LOIKB_J_SPHERICAL ? "spherical" : jt == LOIKB_J_PLANAR ? "planar" : "unbounded (cos, sin) revolute";
      g_last_error = std::string(what) + " belongs to a " + kind + " joint: its configuration is not a scalar that a plain sum advances, it cannot carry a position limit";
      return LOIKB_ERR_ARG;
    }
  }
  return LOIKB_OK;
}

int loikb_set_joint_limits(loikb_solver* S, const double* q_lo, const double* q_hi, int n)
{
  if (!S) return LOIKB_ERR_ARG;
  loikb_solver_impl::PoseState& P = S->pose;
  if (!q_lo && !q_hi) { P.have_limits = false; return LOIKB_OK; }
  int rc;
  if ((rc = check_dof_pairs(S, "set_joint_limits", "q_lo", "q_hi", q_lo, q_hi, n))) return rc;
  std::vector<PoseLimit> lim(S->nb);
  bool any = false;
  for (int j = 0; j < n; ++j) {
    const bool finite = std::isfinite(q_lo[j]) || std::isfinite(q_hi[j]);
    lim[j].qi = finite ? S->lim_q[j] : -1;
    lim[j].pad = 0;
    lim[j].lo = q_lo[j];
    lim[j].hi = q_hi[j];
    any = any || finite;
  }
  if (!any) { P.have_limits = false; return LOIKB_OK; }   // (no finite limit anywhere: the handle runs what it runs without limits)
  HIPCHK(hipSetDevice(S->device));
  if (!P.d_lim && (rc = alloc_dev(S, (void**)&P.d_lim, sizeof(PoseLimit) * S->nb))) return rc;
  P.lim.swap(lim);
  HIPCHK(hipMemcpyAsync(P.d_lim, P.lim.data(), sizeof(PoseLimit) * S->nb, hipMemcpyHostToDevice, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));
  P.have_limits = true;
  return LOIKB_OK;
}

int loikb_pose_get_limit_flags(loikb_solver* S, int* out, int out_flags)
{
  if (!S || !out) return LOIKB_ERR_ARG;
  if (S->pose.nc == 0 || !S->pose.flags_valid) { g_last_error = "pose_get_limit_flags: the last solve_pose ran without joint position or acceleration limits (or there was none)"; return LOIKB_ERR_STATE; }
  HIPCHK(hipSetDevice(S->device));
  return get_copy_out(S, S->pose.d_lflags, sizeof(int) * (size_t)S->B * S->nb, out, out_flags);
}

// ---- include/loik_amd_accel.h (kernels in loik_pose_accel.hpp) ---------------------------------------------------------------
int loikb_accel_version(void) { return LOIKB_ACCEL_VERSION; }

int loikb_set_joint_accel_limits(loikb_solver* S, const double* a_max, int n)
{
  if (!S) return LOIKB_ERR_ARG;
  loikb_solver_impl::PoseState& P = S->pose;
  if (!a_max) { P.have_accel = false; return LOIKB_OK; }
  if (n != S->nv) { g_last_error = "set_joint_accel_limits: need one limit per DoF, n == model.nv"; return LOIKB_ERR_ARG; }
  bool any = false;
  for (int j = 0; j < n; ++j) {
    if (std::isnan(a_max[j]) || !(a_max[j] > 0.0)) {
      char what[128];
      snprintf(what, sizeof(what), "set_joint_accel_limits: DoF %d (joint %d): a limit is NaN or not > 0 (+inf = no limit)", j, S->dof_ext[j]);
      g_last_error = what;
      return LOIKB_ERR_ARG;
    }
    any = any || std::isfinite(a_max[j]);
  }
  if (!any) { P.have_accel = false; return LOIKB_OK; }   // (no finite limit anywhere: the handle runs what it runs without)
  HIPCHK(hipSetDevice(S->device));
  int rc;
  if (!P.d_amax && (rc = alloc_dev(S, (void**)&P.d_amax, sizeof(double) * S->nb))) return rc;
  P.a_max.assign(a_max, a_max + n);
  HIPCHK(hipMemcpyAsync(P.d_amax, P.a_max.data(), sizeof(double) * S->nb, hipMemcpyHostToDevice, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));
  P.have_accel = true;
  return LOIKB_OK;
}

int loikb_accel_set_start_velocity(loikb_solver* S, const double* v0, int in_flags)
{
  if (!S) return LOIKB_ERR_ARG;
  loikb_solver_impl::PoseState& P = S->pose;
  if (!v0) { P.have_v0 = false; return LOIKB_OK; }
  HIPCHK(hipSetDevice(S->device));
  const size_t bytes = sizeof(double) * (size_t)S->B * S->nb;
  int rc;
  if (!P.d_v0 && (rc = alloc_dev(S, (void**)&P.d_v0, bytes))) return rc;
  HIPCHK(hipMemcpyAsync(P.d_v0, v0, bytes, (in_flags & LOIKB_IN_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));   // (v0 is the caller's)
  P.have_v0 = true;
  return LOIKB_OK;
}

int loikb_accel_get_velocity(loikb_solver* S, double* out, int out_flags)
{
  if (!S || !out) return LOIKB_ERR_ARG;
  loikb_solver_impl::PoseState& P = S->pose;
  if (P.nc == 0 || !P.vel_valid) { g_last_error = "accel_get_velocity: the last pose loop ran without joint acceleration limits (or there was none)"; return LOIKB_ERR_STATE; }
  HIPCHK(hipSetDevice(S->device));
  const size_t n = (size_t)S->B * S->nb;
  const bool to_dev = out_flags & LOIKB_OUT_DEVICE;
  int rc;
  if (!to_dev && !P.d_vout && (rc = alloc_dev(S, (void**)&P.d_vout, sizeof(double) * n))) return rc;
  double* dst = to_dev ? out : P.d_vout;
  hipLaunchKernelGGL(k_accel_get_v, grid1(n), dim3(256), 0, S->stream, (const double*)P.d_zp, P.vel_status, S->B, S->nb, dst);
  HIPCHK(hipGetLastError());
  if (!to_dev) HIPCHK(hipMemcpyAsync(out, dst, sizeof(double) * n, hipMemcpyDeviceToHost, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));
  return LOIKB_OK;
}

// ---- include/loik_amd_step.h (kernel in loik_pose_step.hpp) -------------------------------------------------------------------
int loikb_step_version(void) { return LOIKB_STEP_VERSION; }

int loikb_pose_set_step_control(loikb_solver* S, const loikb_step_params* p)
{
  if (!S) return LOIKB_ERR_ARG;
  loikb_solver_impl::PoseState& P = S->pose;
  if (!p) { P.have_step = false; return LOIKB_OK; }
  // (written so that a NaN fails its comparison)
  if (!(p->shrink > 0.0 && p->shrink < 1.0) || !(p->sufficient >= 0.0 && p->sufficient < 1.0) || p->max_backtracks < 0 || p->max_backtracks > 30 ||
      p->patience < 0 || p->flags != 0) {
    g_last_error = "pose_set_step_control: need shrink in (0, 1), sufficient in [0, 1), max_backtracks in 0..30, patience >= 0, flags 0";
    return LOIKB_ERR_ARG;
  }
  P.step = *p;
  P.have_step = true;
  return LOIKB_OK;
}

int loikb_pose_get_step_control(const loikb_solver* S, loikb_step_params* out)
{
  if (!S || !S->pose.have_step) return 0;
  if (out) *out = S->pose.step;
  return 1;
}

int loikb_step_get(loikb_solver* S, int field, void* out, int out_flags)
{
  if (!S || !out) return LOIKB_ERR_ARG;
  const loikb_solver_impl::PoseState& P = S->pose;
  if (P.nc == 0 || !P.step_valid) { g_last_error = "step_get: the last solve_pose ran without step control (or there was none)"; return LOIKB_ERR_STATE; }
  HIPCHK(hipSetDevice(S->device));
  const void* src = nullptr;
  size_t bytes = 0;
  switch (field) {
  case LOIKB_STEP_F_ALPHA: src = P.d_alpha; bytes = sizeof(double) * (size_t)S->B; break;
  case LOIKB_STEP_F_BACKTRACKS: src = P.d_backtracks; bytes = sizeof(int) * (size_t)S->B; break;
  case LOIKB_STEP_F_FAILED: src = P.d_failed; bytes = sizeof(int) * (size_t)S->B; break;
  default: g_last_error = "step_get: unknown field"; return LOIKB_ERR_ARG;
  }
  return get_copy_out(S, src, bytes, out, out_flags);
}

// ---- include/loik_amd_tasks.h -----------------------------------------------------------------------------------------------
int loikb_tasks_version(void) { return LOIKB_TASKS_VERSION; }
// (include/loik_amd_axis.h: its two kinds are cases of loikb_pose_set_tasks below and of the retarget rule of loik_pose.hpp)
int loikb_axis_version(void) { return LOIKB_AXIS_VERSION; }

// S_c of a task kind as six row bits: the base kind's rows, less the rotation about the frame's z with LOIKB_TASK_FREE_Z (loik_amd_axis.h)
static int task_rows(int kind)
{
  const int base = kind & ~LOIKB_TASK_FREE_Z;
  int rows = base == LOIKB_TASK_POSITION ? 0x07 : (base == LOIKB_TASK_ORIENTATION ? 0x38 : 0x3f);
  if (kind & LOIKB_TASK_FREE_Z) rows &= ~0x20;
  return rows;
}

int loikb_pose_set_tasks(loikb_solver* S, int nc, const int* kinds, const double* frames)
{
  if (!S) return LOIKB_ERR_ARG;
  if (!S->have_problem) { g_last_error = "pose_set_tasks before SolveInit()"; return LOIKB_ERR_STATE; }
  if (!S->a_shared) { g_last_error = "pose_set_tasks: the handle's A is per instance; a task matrix is one per constraint for the whole batch (SolveInit with a shared A)"; return LOIKB_ERR_STATE; }
  if (nc != S->nc_active) { g_last_error = "pose_set_tasks: need one task per active constraint, nc == loikb_num_eq_c()"; return LOIKB_ERR_ARG; }
  if (!kinds) { g_last_error = "pose_set_tasks: kinds is NULL"; return LOIKB_ERR_ARG; }
  static const double ident[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  std::vector<PoseTask> tasks(nc);
  for (int c = 0; c < nc; ++c) {
    char what[64];
    snprintf(what, sizeof(what), "pose_set_tasks: task %d", c);
    const bool known = kinds[c] == LOIKB_TASK_POSE || kinds[c] == LOIKB_TASK_POSITION || kinds[c] == LOIKB_TASK_ORIENTATION ||
                       kinds[c] == LOIKB_TASK_POSE_AXIS || kinds[c] == LOIKB_TASK_AXIS;
    if (!known) { g_last_error = std::string(what) + ": unknown kind (LOIKB_TASK_POSE / POSITION / ORIENTATION / POSE_AXIS / AXIS)"; return LOIKB_ERR_ARG; }
    const double* F = frames ? frames + 12 * c : ident;
    if (!frame_ok(F)) { g_last_error = std::string(what) + ": the frame needs a finite translation and a rotation that is orthonormal with determinant 1 (tolerance 1e-9)"; return LOIKB_ERR_ARG; }
    tasks[c].kind = kinds[c];
    tasks[c].pad = 0;
    memcpy(tasks[c].Rf, F, 9 * sizeof(double));
    memcpy(tasks[c].pf, F + 9, 3 * sizeof(double));
  }
  HIPCHK(hipSetDevice(S->device));
  loikb_solver_impl::PoseState& P = S->pose;
  int rc;
  if (!P.d_tasks && (rc = alloc_dev(S, (void**)&P.d_tasks, sizeof(PoseTask) * std::max(S->nc, 1)))) return rc;
  // A_c = S_c X_c^-1, X^-1 = [[Rf^T, -Rf^T [pf]x], [0, Rf^T]], b_c = 0: UpdateEqConstraint(c, A_c, 0) for every active constraint
  const double zero[6] = {0, 0, 0, 0, 0, 0};
  for (int c = 0; c < nc; ++c) {
    const double *Rf = tasks[c].Rf, *pf = tasks[c].pf;
    const double px[9] = {0, -pf[2], pf[1], pf[2], 0, -pf[0], -pf[1], pf[0], 0};
    double A[36] = {0};
    for (int r = 0; r < 3; ++r)
      for (int m = 0; m < 3; ++m) {
        const double rt = Rf[3 * m + r];   // Rf^T
        A[6 * r + m] = rt;
        A[6 * (3 + r) + 3 + m] = rt;
        A[6 * r + 3 + m] = -(Rf[r] * px[m] + Rf[3 + r] * px[3 + m] + Rf[6 + r] * px[6 + m]);
      }
    const int rows = task_rows(tasks[c].kind);
    for (int r = 0; r < 6; ++r)
      if (!((rows >> r) & 1))
        for (int m = 0; m < 6; ++m) A[6 * r + m] = 0.0;   // the masked-out rows
    if ((rc = update_eq_single(S, S->active_ids[c], A, zero, LOIKB_A_SHARED | LOIKB_B_SHARED))) return rc;
  }
  S->pass_active = false;
  if ((rc = reset_home(S, RS_HCACHE))) return rc;
  P.tasks.swap(tasks);
  HIPCHK(hipMemcpyAsync(P.d_tasks, P.tasks.data(), sizeof(PoseTask) * nc, hipMemcpyHostToDevice, S->stream));
  HIPCHK(hipStreamSynchronize(S->stream));
  P.have_tasks = true;   // (last: update_eq_single drops the specification it is given an A under)
  return LOIKB_OK;
}

int loikb_pose_clear_tasks(loikb_solver* S)
{
  if (!S) return LOIKB_ERR_ARG;
  S->pose.have_tasks = false;
  return LOIKB_OK;
}

int loikb_pose_get_tasks(const loikb_solver* S, int* kinds, double* frames, int cap)
{
  if (!S || !S->pose.have_tasks) return 0;
  const int n = (int)S->pose.tasks.size();
  for (int c = 0; c < std::min(n, cap); ++c) {
    const PoseTask& t = S->pose.tasks[c];
    if (kinds) kinds[c] = t.kind;
    if (frames) { memcpy(frames + 12 * c, t.Rf, 9 * sizeof(double)); memcpy(frames + 12 * c + 9, t.pf, 3 * sizeof(double)); }
  }
  return n;
}

int loikb_frame_placements(loikb_solver* S, const int* links, const double* frames, int n, double* out, int out_flags)
{
  if (!frames) return loikb_forward_kinematics(S, links, n, out, out_flags);
  if (!S || n < 0 || (n > 0 && (!links || !out))) return LOIKB_ERR_ARG;
  int rc;
  if ((rc = jac_check_entries(S, "frame_placements", links, frames, n))) return rc;
  if (!S->have_q) { g_last_error = "frame_placements: no configurations resident on the device yet"; return LOIKB_ERR_STATE; }
  if (n == 0) return LOIKB_OK;
  HIPCHK(hipSetDevice(S->device));
  const std::vector<int> dl = device_links(S, links, n);
  QueryOut o(S, out_flags);
  double *dst, *d_fr;
  int* d_dl;
  o.add(out, sizeof(double) * (size_t)S->B * n * 12, &dst);
  if ((rc = jac_stage_entries(S, dl.data(), frames, nullptr, n, &d_fr, &d_dl, nullptr)) || (rc = o.reserve())) return rc;
  hipLaunchKernelGGL(k_frame_placements, grid1((size_t)S->B * n), dim3(256), 0, S->stream, (const double*)S->d_q, S->nq, S->d_jd,
                     S->d_idx_q, (const int*)d_dl, (const double*)d_fr, n, S->B, dst);
  HIPCHK(hipGetLastError());
  return o.finish();   // (dl and the caller's frames have been read)
}

// ---- include/loik_amd_jacobian.h (kernels in loik_pose_jacobian.hpp) -----------------------------------------------------------
int loikb_jacobian_version(void) { return LOIKB_JACOBIAN_VERSION; }

static const double IDENT12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};

static bool dex_params_ok(const loikb_dexterity_params* p) { return p && std::isfinite(p->length) && p->length > 0.0 && p->flags == 0; }

// the frames given, or the joint frames
static std::vector<double> frames_or_identity(const double* frames, int n)
{
  std::vector<double> fr((size_t)n * 12);
  for (int e = 0; e < n; ++e) memcpy(&fr[(size_t)12 * e], frames ? frames + 12 * e : IDENT12, sizeof(IDENT12));
  return fr;
}

// "the handle's tasks" (links == NULL of loikb_frame_dexterity): the frames and row masks of the active constraints
static void dex_task_entries(const loikb_solver_impl* S, std::vector<double>& fr, std::vector<int>& rows)
{
  const int nc = S->nc_active;
  fr.resize((size_t)nc * 12);
  rows.resize(nc);
  for (int c = 0; c < nc; ++c) {
    const bool tk = S->pose.have_tasks && c < (int)S->pose.tasks.size();
    if (tk) { memcpy(&fr[12 * c], S->pose.tasks[c].Rf, 9 * sizeof(double)); memcpy(&fr[12 * c + 9], S->pose.tasks[c].pf, 3 * sizeof(double)); }
    else memcpy(&fr[12 * c], IDENT12, sizeof(IDENT12));
    rows[c] = tk ? task_rows(S->pose.tasks[c].kind) : 0x3f;
  }
}

int loikb_frame_jacobians(loikb_solver* S, const int* links, const double* frames, int n, int reference_frame, double* out, int out_flags)
{
  if (!S || !out || n < 0 || (n > 0 && !links)) return LOIKB_ERR_ARG;
  if (reference_frame < LOIKB_JAC_LOCAL || reference_frame > LOIKB_JAC_WORLD) { g_last_error = "frame_jacobians: reference_frame must be LOIKB_JAC_LOCAL, _LOCAL_WORLD_ALIGNED or _WORLD"; return LOIKB_ERR_ARG; }
  int rc;
  if ((rc = jac_check_entries(S, "frame_jacobians", links, frames, n))) return rc;
  if (!S->have_q) { g_last_error = "frame_jacobians: no configurations resident on the device yet"; return LOIKB_ERR_STATE; }
  if (n == 0) return LOIKB_OK;
  // the wavefronts of a workgroup: as many of JAC_WAVES as 64 KB of LDS hold root paths for
  const size_t per = jac_wave_doubles(S->nb) * sizeof(double);
  const int waves = lds_waves(JAC_WAVES, per);
  const size_t lds = waves * per;
  if (lds > 65536) { g_last_error = "frame_jacobians: the model has more DoFs than one wavefront's root path fits in 64 KB of LDS for (630)"; return LOIKB_ERR_ARG; }
  HIPCHK(hipSetDevice(S->device));
  const std::vector<int> dl = device_links(S, links, n);
  const std::vector<double> fr = frames_or_identity(frames, n);
  const size_t pairs = (size_t)S->B * n;
  QueryOut o(S, out_flags);
  double *dst, *d_fr;
  int *d_dl, *d_rows;   // (the room for row masks: what this getter has always asked of scratch 1)
  o.add(out, sizeof(double) * pairs * 6 * S->nb, &dst);
  if ((rc = jac_stage_entries(S, dl.data(), fr.data(), nullptr, n, &d_fr, &d_dl, &d_rows)) || (rc = o.reserve())) return rc;
  hipLaunchKernelGGL(k_frame_jacobians, dim3((unsigned)((pairs + waves - 1) / waves)), dim3(64 * waves), lds, S->stream, (const double*)S->d_q, S->nq,
                     S->d_jd, S->d_idx_q, (const int*)d_dl, (const double*)d_fr, n, S->B, S->nb, reference_frame, dst);
  HIPCHK(hipGetLastError());
  return o.finish();   // (dl and fr are locals)
}

int loikb_frame_dexterity(loikb_solver* S, const int* links, const double* frames, const int* rows, int n, const loikb_dexterity_params* p,
                          double* out, int out_flags)
{
  if (!S || !out || n < 0) return LOIKB_ERR_ARG;
  if (!dex_params_ok(p)) { g_last_error = "frame_dexterity: need params with a finite length > 0 and flags 0"; return LOIKB_ERR_ARG; }
  int rc;
  if (!links) {
    if (!S->have_problem) { g_last_error = "frame_dexterity: links == NULL (the handle's tasks) before SolveInit()"; return LOIKB_ERR_STATE; }
    if (n != S->nc_active) { g_last_error = "frame_dexterity: links == NULL (the handle's tasks) needs n == loikb_num_eq_c()"; return LOIKB_ERR_ARG; }
  } else {
    if ((rc = jac_check_entries(S, "frame_dexterity", links, frames, n))) return rc;
    for (int e = 0; rows && e < n; ++e)
      if (rows[e] < 1 || rows[e] > 0x3f) { g_last_error = "frame_dexterity: a row mask must select at least one of the six rows (1..0x3f)"; return LOIKB_ERR_ARG; }
  }
  if (!S->have_q) { g_last_error = "frame_dexterity: no configurations resident on the device yet"; return LOIKB_ERR_STATE; }
  if (n == 0) return LOIKB_OK;
  HIPCHK(hipSetDevice(S->device));
  std::vector<int> dl, rw(n, 0x3f);
  std::vector<double> fr;
  if (!links) {
    dl = device_links(S, S->active_ids.data(), n);
    dex_task_entries(S, fr, rw);
  } else {
    dl = device_links(S, links, n);
    fr = frames_or_identity(frames, n);
    if (rows) rw.assign(rows, rows + n);
  }
  const size_t pairs = (size_t)S->B * n;
  QueryOut o(S, out_flags);
  double *dst, *d_fr;
  int *d_dl, *d_rows;
  o.add(out, sizeof(double) * pairs * DEX_N, &dst);
  if ((rc = jac_stage_entries(S, dl.data(), fr.data(), rw.data(), n, &d_fr, &d_dl, &d_rows)) || (rc = o.reserve())) return rc;
  hipLaunchKernelGGL(k_frame_dexterity, grid1(pairs), dim3(256), 0, S->stream, (const double*)S->d_q, S->nq, S->d_jd, S->d_idx_q, (const int*)d_dl,
                     (const double*)d_fr, (const int*)d_rows, n, S->B, p->length, dst);
  HIPCHK(hipGetLastError());
  return o.finish();   // (dl, fr and rw are locals)
}

int loikb_dexterity_set_multistart_pick(loikb_solver* S, const loikb_dexterity_params* p)
{
  if (!S) return LOIKB_ERR_ARG;
  loikb_solver_impl::PoseState& P = S->pose;
  if (!p) { P.have_dex = false; return LOIKB_OK; }
  if (!dex_params_ok(p)) { g_last_error = "dexterity_set_multistart_pick: need a finite length > 0 and flags 0"; return LOIKB_ERR_ARG; }
  P.dex = *p;
  P.have_dex = true;
  return LOIKB_OK;
}

int loikb_dexterity_get_multistart_pick(const loikb_solver* S, loikb_dexterity_params* out)
{
  if (!S || !S->pose.have_dex) return 0;
  if (out) *out = S->pose.dex;
  return 1;
}

// The cost of class 0 of a dexterous multi-start selection into M.d_dexcost: k_frame_dexterity in the links == NULL mode over all B
// resident rows (the device joints of the active constraints are P.d_clink, which the pose loop just left), then the reduction
// to - min_c sigma_{m_c - 1}.  Queued; the staging is the handle's.
static int ms_dex_cost(loikb_solver_impl* S)
{
  loikb_solver_impl::MultiStartState& M = S->ms;
  const loikb_solver_impl::PoseState& P = S->pose;
  const size_t B = (size_t)S->B, ncap = (size_t)std::max(S->nc, 1);
  const int nc = S->nc_active;
  int rc;
  if (!M.d_dexcost) {
    if ((rc = alloc_dev(S, (void**)&M.d_dex, sizeof(double) * B * ncap * DEX_N)) || (rc = alloc_dev(S, (void**)&M.d_dexfr, sizeof(double) * ncap * 12)) ||
        (rc = alloc_dev(S, (void**)&M.d_dexrows, sizeof(int) * ncap)) || (rc = alloc_dev(S, (void**)&M.d_dexcost, sizeof(double) * B))) {
      M.d_dexcost = nullptr;   // (as pose_alloc: what was allocated goes with the handle; the next call allocates afresh)
      return rc;
    }
  }
  dex_task_entries(S, M.dex_fr, M.dex_rows);
  HIPCHK(hipMemcpyAsync(M.d_dexfr, M.dex_fr.data(), sizeof(double) * 12 * nc, hipMemcpyHostToDevice, S->stream));
  HIPCHK(hipMemcpyAsync(M.d_dexrows, M.dex_rows.data(), sizeof(int) * nc, hipMemcpyHostToDevice, S->stream));
  hipLaunchKernelGGL(k_frame_dexterity, grid1(B * nc), dim3(256), 0, S->stream, (const double*)S->d_q, S->nq, S->d_jd, S->d_idx_q, (const int*)P.d_clink,
                     (const double*)M.d_dexfr, (const int*)M.d_dexrows, nc, S->B, P.dex.length, M.d_dex);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_dex_cost, grid1(B), dim3(256), 0, S->stream, (const double*)M.d_dex, (const int*)M.d_dexrows, nc, S->B, M.d_dexcost);
  HIPCHK(hipGetLastError());
  return LOIKB_OK;
}

// ---- include/loik_amd_collision.h (kernels in loik_pose_collision.hpp) ---------------------------------------------------------
int loikb_collision_version(void) { return LOIKB_COLLISION_VERSION; }

using Collision = loikb_solver_impl::PoseState::Collision;

// the parent of every link in the caller's tree, from the device tree: the link whose last chain joint is the parent of the first
static std::vector<int> col_ext_parents(const loikb_solver_impl* S)
{
  std::vector<int> ext_of(S->nj, 0), par(S->ext_nj, -1);
  for (int i = 1; i < S->ext_nj; ++i) ext_of[S->link_of[i]] = i;
  for (int i = 1; i < S->ext_nj; ++i) par[i] = ext_of[S->parents[S->first_of[i]]];
  return par;
}

// the self-pair list of `links` [ns] under `ignore` [ni][2]: (a < b) lexicographic, the links differ, neither is the other's parent,
// the link pair is not ignored
static std::vector<unsigned short> col_build_pairs(const loikb_solver_impl* S, const std::vector<int>& links, const std::vector<int>& ignore)
{
  const std::vector<int> par = col_ext_parents(S);
  const int ns = (int)links.size(), nl = S->ext_nj;
  std::vector<char> skip((size_t)nl * nl, 0);
  for (size_t k = 0; k + 1 < ignore.size(); k += 2) {
    skip[(size_t)ignore[k] * nl + ignore[k + 1]] = 1;
    skip[(size_t)ignore[k + 1] * nl + ignore[k]] = 1;
  }
  std::vector<unsigned short> pairs;
  for (int a = 0; a < ns; ++a)
    for (int b = a + 1; b < ns; ++b) {
      const int la = links[a], lb = links[b];
      if (la == lb || par[la] == lb || par[lb] == la || skip[(size_t)la * nl + lb]) continue;
      pairs.push_back((unsigned short)a);
      pairs.push_back((unsigned short)b);
    }
  return pairs;
}

// the ordinal of a pair is 32 bits with one value kept for "none"
// (a grid is one more world object: a pair per sphere)
static bool col_ordinals_fit(size_t ns, size_t nws, size_t nwb, bool grid, size_t npairs) { return ns * (nws + nwb + (grid ? 1 : 0)) + npairs < (size_t)0x7fffffff; }

int loikb_collision_set_spheres(loikb_solver* S, const int* links, const double* spheres, int ns)
{
  if (!S) return LOIKB_ERR_ARG;
  if (ns < 0 || (ns > 0 && (!links || !spheres))) { g_last_error = "collision_set_spheres: need ns >= 0 and both arrays when ns > 0"; return LOIKB_ERR_ARG; }
  if (ns > LOIKB_CLR_MAX_SPHERES) { g_last_error = "collision_set_spheres: more than LOIKB_CLR_MAX_SPHERES spheres"; return LOIKB_ERR_ARG; }
  for (int i = 0; i < ns; ++i) {
    const std::string what = "collision_set_spheres: sphere " + std::to_string(i);
    if (links[i] < 0 || links[i] >= S->ext_nj) { g_last_error = what + ": link id out of range"; return LOIKB_ERR_ARG; }
    for (int k = 0; k < 4; ++k)
      if (!std::isfinite(spheres[4 * i + k])) { g_last_error = what + ": a number is not finite"; return LOIKB_ERR_ARG; }
    if (spheres[4 * i + 3] < 0.0) { g_last_error = what + ": negative radius"; return LOIKB_ERR_ARG; }
  }
  Collision& C = S->pose.col;
  if (S->pose.avoid.have && (ns == 0 || ns > LOIKB_AVOID_MAX_SPHERES)) {
    g_last_error = "collision_set_spheres: collision avoidance is set on the handle (loikb_avoid_set), which needs 1 .. LOIKB_AVOID_MAX_SPHERES = " +
                   std::to_string(LOIKB_AVOID_MAX_SPHERES) + " spheres -- clear it first";
    return LOIKB_ERR_STATE;
  }
  HIPCHK(hipSetDevice(S->device));
  std::vector<int> lk(links, links + ns), car, scar(ns), slot(S->nj, -1);
  for (int i = 0; i < ns; ++i) {
    const int dj = S->link_of[lk[i]];
    if (slot[dj] < 0) { slot[dj] = (int)car.size(); car.push_back(dj); }
    scar[i] = slot[dj];
  }
  std::vector<unsigned short> pairs;
  if (ns > 0 && C.self_on) pairs = col_build_pairs(S, lk, C.ignore);
  if (!col_ordinals_fit(ns, C.nws, C.nwb, C.have_grid, pairs.size() / 2)) { g_last_error = "collision_set_spheres: more than 2^31 pairs"; return LOIKB_ERR_ARG; }
  DevBuf<double> d_sph;
  DevBuf<int> d_scar, d_car;
  DevBuf<unsigned short> d_pairs;
  int rc;
  if ((rc = col_upload(S, spheres, sizeof(double) * 4 * ns, d_sph)) || (rc = col_upload(S, scar.data(), sizeof(int) * ns, d_scar)) ||
      (rc = col_upload(S, car.data(), sizeof(int) * car.size(), d_car)) || (rc = col_upload(S, pairs.data(), sizeof(unsigned short) * pairs.size(), d_pairs)))
    return rc;
  HIPCHK(hipStreamSynchronize(S->stream));   // (nothing queued reads the buffers that go: the locals take them)
  C.d_sph.swap(d_sph); C.d_scar.swap(d_scar); C.d_car.swap(d_car); C.d_pairs.swap(d_pairs);
  C.links.swap(lk); C.car.swap(car); C.scar.swap(scar); C.pairs.swap(pairs);
  C.ns = ns;
  if (ns == 0) { C.self_on = false; C.ignore.clear(); }
  return LOIKB_OK;
}

int loikb_collision_set_world(loikb_solver* S, const double* wspheres, int nws, const double* wboxes, int nwb)
{
  if (!S) return LOIKB_ERR_ARG;
  if (nws < 0 || nwb < 0 || (nws > 0 && !wspheres) || (nwb > 0 && !wboxes)) { g_last_error = "collision_set_world: need counts >= 0 and an array for a positive count"; return LOIKB_ERR_ARG; }
  for (int i = 0; i < nws; ++i) {
    const std::string what = "collision_set_world: sphere " + std::to_string(i);
    for (int k = 0; k < 4; ++k)
      if (!std::isfinite(wspheres[4 * i + k])) { g_last_error = what + ": a number is not finite"; return LOIKB_ERR_ARG; }
    if (wspheres[4 * i + 3] < 0.0) { g_last_error = what + ": negative radius"; return LOIKB_ERR_ARG; }
  }
  for (int i = 0; i < nwb; ++i) {
    const std::string what = "collision_set_world: box " + std::to_string(i);
    const double* W = wboxes + 15 * i;
    for (int k = 0; k < 15; ++k)
      if (!std::isfinite(W[k])) { g_last_error = what + ": a number is not finite"; return LOIKB_ERR_ARG; }
    if (!frame_ok(W)) { g_last_error = what + ": the rotation is not orthonormal with determinant 1 (tolerance 1e-9)"; return LOIKB_ERR_ARG; }
    for (int k = 12; k < 15; ++k)
      if (!(W[k] > 0.0)) { g_last_error = what + ": a half extent is not > 0"; return LOIKB_ERR_ARG; }
  }
  Collision& C = S->pose.col;
  if (!col_ordinals_fit(C.ns, nws, nwb, C.have_grid, C.pairs.size() / 2)) { g_last_error = "collision_set_world: more than 2^31 pairs"; return LOIKB_ERR_ARG; }
  HIPCHK(hipSetDevice(S->device));
  DevBuf<double> d_wsph, d_wbox;
  int rc;
  if ((rc = col_upload(S, wspheres, sizeof(double) * 4 * nws, d_wsph)) || (rc = col_upload(S, wboxes, sizeof(double) * 15 * nwb, d_wbox))) return rc;
  HIPCHK(hipStreamSynchronize(S->stream));
  C.d_wsph.swap(d_wsph); C.d_wbox.swap(d_wbox);
  C.nws = nws; C.nwb = nwb;
  return LOIKB_OK;
}

int loikb_collision_set_self_pairs(loikb_solver* S, int enable, const int* ignore_links, int ni)
{
  if (!S) return LOIKB_ERR_ARG;
  if (ni < 0 || (ni > 0 && !ignore_links)) { g_last_error = "collision_set_self_pairs: need ni >= 0 and ignore_links when ni > 0"; return LOIKB_ERR_ARG; }
  for (int i = 0; i < 2 * ni; ++i)
    if (ignore_links[i] < 0 || ignore_links[i] >= S->ext_nj) {
      g_last_error = "collision_set_self_pairs: ignore pair " + std::to_string(i / 2) + ": link id out of range";
      return LOIKB_ERR_ARG;
    }
  Collision& C = S->pose.col;
  if (enable && C.ns == 0) { g_last_error = "collision_set_self_pairs: enable = 1 with no spheres set (loikb_collision_set_spheres)"; return LOIKB_ERR_STATE; }
  HIPCHK(hipSetDevice(S->device));
  std::vector<int> ignore;
  std::vector<unsigned short> pairs;
  if (enable) {
    ignore.assign(ignore_links, ignore_links + 2 * (size_t)ni);
    pairs = col_build_pairs(S, C.links, ignore);
  }
  if (!col_ordinals_fit(C.ns, C.nws, C.nwb, C.have_grid, pairs.size() / 2)) { g_last_error = "collision_set_self_pairs: more than 2^31 pairs"; return LOIKB_ERR_ARG; }
  DevBuf<unsigned short> d_pairs;
  int rc;
  if ((rc = col_upload(S, pairs.data(), sizeof(unsigned short) * pairs.size(), d_pairs))) return rc;
  HIPCHK(hipStreamSynchronize(S->stream));
  C.d_pairs.swap(d_pairs);
  C.pairs.swap(pairs);
  C.ignore.swap(ignore);
  C.self_on = enable != 0;
  return LOIKB_OK;
}

int loikb_collision_num_self_pairs(const loikb_solver* S) { return S ? (int)(S->pose.col.pairs.size() / 2) : 0; }

// ---- include/loik_amd_grid.h (kernels in loik_pose_grid.hpp) ---------------------------------------------------------------------
int loikb_grid_version(void) { return LOIKB_GRID_VERSION; }

static_assert(GRID_MAX_DIM == LOIKB_GRID_MAX_DIM && GRID_MAX_VOXELS == LOIKB_GRID_MAX_VOXELS && GRID_EMPTY == LOIKB_GRID_EMPTY &&
              CLR_WORLD_GRID == LOIKB_CLR_WORLD_GRID, "the kernels' constants and the header's");
static_assert((size_t)GRID_MAX_DIM / 2 * 64 * sizeof(unsigned int) <= 65536 && (size_t)GRID_MAX_DIM * 32 * sizeof(unsigned int) <= 65536,
              "a tile of k_grid_pass fits 64 KB at either width");

// the high corner of the grid's box along one axis: the product rounded, then the sum (loik_amd_grid.h)
static double grid_hi(double origin, int n, double h)
{
  const volatile double e = (double)n * h;   // (volatile: the two operations stay two, whatever the compiler may contract)
  return origin + e;
}

// The nearest-voxel transform of the finished field G [nz][ny][nx] into F (loik_amd_gridnear.h; kernels in loik_pose_gridnear.hpp).
// Queued; the keys go through C.d_nearkey, which only a build uses
static int gridnear_build(loikb_solver_impl* S, const unsigned int* G, int nx, int ny, int nz, unsigned int* F)
{
  Collision& C = S->pose.col;
  const size_t nvox = (size_t)nx * ny * nz;
  if (int rc = regrow_drained(S, C.d_nearkey, sizeof(unsigned long long) * nvox)) return rc;
  unsigned long long* K = C.d_nearkey;
  const long long nlines = (long long)ny * nz;
  const int per = grid_x_lines(nx);
  hipLaunchKernelGGL(k_gridnear_x, dim3((unsigned)((nlines + per - 1) / per)), dim3(GRID_THREADS), 0, S->stream, G, K,
                     (ny > 1 || nz > 1) ? (unsigned int*)nullptr : F, nx, nlines);
  HIPCHK(hipGetLastError());
  if (ny > 1) {   // (an axis of one voxel: the pass is the identity)
    const int W = gridnear_tile_width(ny);
    hipLaunchKernelGGL(k_gridnear_pass, dim3((unsigned)((nx + W - 1) / W), (unsigned)nz), dim3(GRID_THREADS), sizeof(unsigned long long) * (size_t)ny * W,
                       S->stream, K, nz > 1 ? (unsigned int*)nullptr : F, ny, nx, (size_t)nx, (size_t)nx * ny, W);
    HIPCHK(hipGetLastError());
  }
  if (nz > 1) {
    const int W = gridnear_tile_width(nz);
    hipLaunchKernelGGL(k_gridnear_pass, dim3((unsigned)((nx + W - 1) / W), (unsigned)ny), dim3(GRID_THREADS), sizeof(unsigned long long) * (size_t)nz * W,
                       S->stream, K, F, nz, nx, (size_t)nx * ny, (size_t)nx, W);
    HIPCHK(hipGetLastError());
  }
  return LOIKB_OK;
}

// What loikb_collision_set_world_grid asks of a grid and of the handle before anything changes (loik_amd_grid.h); `fn` goes into
// loikb_last_error().  *nvox: the voxels of the grid
static int grid_check(const loikb_solver_impl* S, const char* fn, const int* dims, const double* origin, double h, size_t* nvox)
{
  const Collision& C = S->pose.col;
  const std::string f(fn);
  size_t n = 1;
  for (int k = 0; k < 3; ++k) {
    if (dims[k] < 1 || dims[k] > LOIKB_GRID_MAX_DIM) {
      g_last_error = f + ": a dimension outside 1 .. LOIKB_GRID_MAX_DIM = " + std::to_string(LOIKB_GRID_MAX_DIM);
      return LOIKB_ERR_ARG;
    }
    n *= (size_t)dims[k];
  }
  if (n > GRID_MAX_VOXELS) { g_last_error = f + ": more than LOIKB_GRID_MAX_VOXELS = 2^26 voxels"; return LOIKB_ERR_ARG; }
  if (!std::isfinite(h) || !(h > 0.0) || !std::isfinite(1.0 / h)) {
    g_last_error = f + ": need a finite voxel edge h > 0 with a finite inverse";
    return LOIKB_ERR_ARG;
  }
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(origin[k]) || !std::isfinite(grid_hi(origin[k], dims[k], h))) {
      g_last_error = f + ": the origin or a corner of the grid's box is not finite";
      return LOIKB_ERR_ARG;
    }
  if (!col_ordinals_fit(C.ns, C.nws, C.nwb, true, C.pairs.size() / 2)) { g_last_error = f + ": more than 2^31 pairs"; return LOIKB_ERR_ARG; }
  if (S->pose.avoid.have && !C.near_on) {
    g_last_error = f + ": collision avoidance is set on the handle (loikb_avoid_set), and avoidance cannot read a voxel grid -- clear it first."
                       "  With the nearest-voxel transform latched (loikb_collision_grid_set_nearest) avoidance reads the grid.";
    return LOIKB_ERR_STATE;
  }
  *nvox = n;
  return LOIKB_OK;
}

// The tail of every call that sets a grid: the field G of the device occupancy d_occ [nz][ny][nx] (and with the latch F) into the spare
// buffers, which change places with the resident ones after the stream has drained; a failure leaves the handle as it was.  Complete on
// return: whatever was queued before, the reads of a caller's memory included, has run
static int grid_build_swap(loikb_solver_impl* S, const unsigned char* d_occ, const int* dims, const double* origin, double h)
{
  Collision& C = S->pose.col;
  const int nx = dims[0], ny = dims[1], nz = dims[2];
  const size_t nvox = (size_t)nx * ny * nz;
  BUFCHK(C.d_grid_next.regrow(sizeof(unsigned int) * nvox));   // (nothing queued reads it: it is not the grid that is set)
  unsigned int* G = C.d_grid_next;
  const long long nlines = (long long)ny * nz;
  const int per = grid_x_lines(nx);
  hipLaunchKernelGGL(k_grid_x, dim3((unsigned)((nlines + per - 1) / per)), dim3(GRID_THREADS), 0, S->stream, d_occ, G, nx, nlines);
  HIPCHK(hipGetLastError());
  if (ny > 1) {   // (an axis of one voxel: the pass is the identity)
    const int W = grid_tile_width(ny);
    hipLaunchKernelGGL(k_grid_pass, dim3((unsigned)((nx + W - 1) / W), (unsigned)nz), dim3(GRID_THREADS), sizeof(unsigned int) * (size_t)ny * W, S->stream,
                       G, ny, nx, (size_t)nx, (size_t)nx * ny, W);
    HIPCHK(hipGetLastError());
  }
  if (nz > 1) {
    const int W = grid_tile_width(nz);
    hipLaunchKernelGGL(k_grid_pass, dim3((unsigned)((nx + W - 1) / W), (unsigned)ny), dim3(GRID_THREADS), sizeof(unsigned int) * (size_t)nz * W, S->stream,
                       G, nz, nx, (size_t)nx * ny, (size_t)nx, W);
    HIPCHK(hipGetLastError());
  }
  if (C.near_on) {   // F beside G, both in the spare buffers: they change places below, after both builds went through
    BUFCHK(C.d_near_next.regrow(sizeof(unsigned int) * nvox));
    if (int rc = gridnear_build(S, G, nx, ny, nz, C.d_near_next)) return rc;
  }
  HIPCHK(hipStreamSynchronize(S->stream));   // (the caller's memory has been read; nothing queued reads the grid that goes)
  if (C.near_on) C.d_near.swap(C.d_near_next);
  C.d_grid.swap(C.d_grid_next);
  for (int k = 0; k < 3; ++k) { C.gn[k] = dims[k]; C.go[k] = origin[k]; }
  C.gh = h;
  C.have_grid = true;
  return LOIKB_OK;
}

int loikb_collision_set_world_grid(loikb_solver* S, const unsigned char* occ, const int* dims, const double* origin, double h, int in_flags)
{
  if (!S) return LOIKB_ERR_ARG;
  Collision& C = S->pose.col;
  if (!occ) {   // clear: the buffers stay for the next grid
    HIPCHK(hipSetDevice(S->device));
    HIPCHK(hipStreamSynchronize(S->stream));
    C.have_grid = false;
    return LOIKB_OK;
  }
  if (!dims || !origin) { g_last_error = "collision_set_world_grid: need dims and origin with an occupancy"; return LOIKB_ERR_ARG; }
  if (in_flags & ~LOIKB_IN_DEVICE) { g_last_error = "collision_set_world_grid: in_flags other than LOIKB_IN_DEVICE"; return LOIKB_ERR_ARG; }
  size_t nvox = 0;
  if (int rc = grid_check(S, "collision_set_world_grid", dims, origin, h, &nvox)) return rc;
  HIPCHK(hipSetDevice(S->device));
  const unsigned char* d_occ = occ;
  if (!(in_flags & LOIKB_IN_DEVICE)) {
    BUFCHK(C.d_occ.regrow(nvox));
    HIPCHK(hipMemcpyAsync(C.d_occ, occ, nvox, hipMemcpyHostToDevice, S->stream));
    d_occ = C.d_occ;
  }
  return grid_build_swap(S, d_occ, dims, origin, h);
}

int loikb_collision_get_world_grid(loikb_solver* S, int* dims, double* origin, double* h, unsigned int* G, int out_flags)
{
  if (!S) return 0;
  if (out_flags & ~LOIKB_OUT_DEVICE) { g_last_error = "collision_get_world_grid: out_flags other than LOIKB_OUT_DEVICE"; return LOIKB_ERR_ARG; }
  if (!S->pose.col.have_grid) return 0;
  const Collision& C = S->pose.col;
  for (int k = 0; k < 3; ++k) {
    if (dims) dims[k] = C.gn[k];
    if (origin) origin[k] = C.go[k];
  }
  if (h) *h = C.gh;
  if (G) {
    HIPCHK(hipSetDevice(S->device));
    const size_t bytes = sizeof(unsigned int) * (size_t)C.gn[0] * C.gn[1] * C.gn[2];
    HIPCHK(hipMemcpyAsync(G, (const unsigned int*)C.d_grid, bytes, (out_flags & LOIKB_OUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, S->stream));
    HIPCHK(hipStreamSynchronize(S->stream));
  }
  return 1;
}

// the handle's collision model as every kernel that reads it takes it
static ClrModel clr_model(const loikb_solver_impl* S)
{
  const Collision& C = S->pose.col;
  int lp = 0;
  while (lp < 6 && (1 << lp) < C.ns) ++lp;
  ClrModel m{C.d_sph, C.d_scar, C.d_car, C.d_wsph, C.d_wbox, C.d_pairs, C.ns, (int)C.car.size(), C.nws, C.nwb, (int)(C.pairs.size() / 2), lp,
             ClrGrid{nullptr, {0, 0, 0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0, 0.0, nullptr}};
  if (C.have_grid) {
    m.g.G = C.d_grid;
    if (C.near_on) m.g.F = C.d_near;
    for (int k = 0; k < 3; ++k) { m.g.n[k] = C.gn[k]; m.g.o[k] = C.go[k]; m.g.hi[k] = grid_hi(C.go[k], C.gn[k], C.gh); }
    m.g.h = C.gh;
    m.g.inv_h = 1.0 / C.gh;
  }
  return m;
}

// ---- include/loik_amd_gridnear.h (kernels in loik_pose_gridnear.hpp) ------------------------------------------------------------
int loikb_gridnear_version(void) { return LOIKB_GRIDNEAR_VERSION; }

static_assert(GRID_NO_VOXEL == LOIKB_GRID_NO_VOXEL, "the kernels' constant and the header's");
static_assert((size_t)GRID_MAX_DIM / 2 * 32 * sizeof(unsigned long long) <= 65536 && (size_t)GRID_MAX_DIM * 16 * sizeof(unsigned long long) <= 65536,
              "a tile of k_gridnear_pass fits 64 KB at either width");

int loikb_collision_grid_set_nearest(loikb_solver* S, int on)
{
  if (!S) return LOIKB_ERR_ARG;
  if (on != 0 && on != 1) { g_last_error = "collision_grid_set_nearest: on must be 0 or 1"; return LOIKB_ERR_ARG; }
  Collision& C = S->pose.col;
  HIPCHK(hipSetDevice(S->device));
  if (!on) {
    if (C.have_grid && S->pose.avoid.have) {
      g_last_error = "collision_grid_set_nearest: a voxel grid is set and collision avoidance is set on the handle (loikb_avoid_set), which reads the grid through the "
                     "transform -- clear the avoidance or the grid first";
      return LOIKB_ERR_STATE;
    }
    HIPCHK(hipStreamSynchronize(S->stream));   // (nothing queued reads F)
    C.near_on = false;
    // "as if never latched": the transform, its spare and the keys go back to the device.  While the latch is on they stay, the keys
    // included, so that a set at sensor rate allocates nothing
    C.d_near.release(); C.d_near_next.release(); C.d_nearkey.release();
    return LOIKB_OK;
  }
  if (C.have_grid) {
    BUFCHK(C.d_near_next.regrow(sizeof(unsigned int) * (size_t)C.gn[0] * C.gn[1] * C.gn[2]));
    if (int rc = gridnear_build(S, C.d_grid, C.gn[0], C.gn[1], C.gn[2], C.d_near_next)) return rc;
    HIPCHK(hipStreamSynchronize(S->stream));
    C.d_near.swap(C.d_near_next);
  }
  C.near_on = true;
  return LOIKB_OK;
}

int loikb_collision_grid_get_nearest(loikb_solver* S, unsigned int* F, int out_flags)
{
  if (!S) return 0;
  if (out_flags & ~LOIKB_OUT_DEVICE) { g_last_error = "collision_grid_get_nearest: out_flags other than LOIKB_OUT_DEVICE"; return LOIKB_ERR_ARG; }
  const Collision& C = S->pose.col;
  if (!C.have_grid || !C.near_on) return 0;
  if (F) {
    HIPCHK(hipSetDevice(S->device));
    if (int rc = get_copy_out(S, (const unsigned int*)C.d_near, sizeof(unsigned int) * (size_t)C.gn[0] * C.gn[1] * C.gn[2], F, out_flags)) return rc;
  }
  return 1;
}

int loikb_grid_nearest_query(loikb_solver* S, const double* spheres, int n, int in_flags, double* out_val, int* out_vox, double* out_normal, int out_flags)
{
  if (!S) return LOIKB_ERR_ARG;
  if (n < 0 || (n > 0 && (!spheres || !out_val || !out_vox || !out_normal))) { g_last_error = "grid_nearest_query: need n >= 0 and every array when n > 0"; return LOIKB_ERR_ARG; }
  if (in_flags & ~LOIKB_IN_DEVICE) { g_last_error = "grid_nearest_query: in_flags other than LOIKB_IN_DEVICE"; return LOIKB_ERR_ARG; }
  const Collision& C = S->pose.col;
  if (!C.have_grid) { g_last_error = "grid_nearest_query: no voxel grid set (loikb_collision_set_world_grid)"; return LOIKB_ERR_STATE; }
  if (!C.near_on) { g_last_error = "grid_nearest_query: the nearest-voxel transform is not latched (loikb_collision_grid_set_nearest)"; return LOIKB_ERR_STATE; }
  if (n == 0) return LOIKB_OK;
  HIPCHK(hipSetDevice(S->device));
  QueryOut o(S, out_flags);
  double *d_val, *d_nrm;
  int* d_vox;
  o.add(out_val, sizeof(double) * 2 * (size_t)n, &d_val);
  o.add(out_normal, sizeof(double) * 3 * (size_t)n, &d_nrm);
  o.add(out_vox, sizeof(int) * 2 * (size_t)n, &d_vox);
  int rc;
  const void* ds = nullptr;
  if ((rc = to_device(S, spheres, sizeof(double) * 4 * (size_t)n, in_flags & LOIKB_IN_DEVICE, &ds)) || (rc = o.reserve())) return rc;
  hipLaunchKernelGGL(k_grid_nearest_query, grid1((size_t)n), dim3(256), 0, S->stream, (const double*)ds, n, clr_model(S).g, d_val, d_vox, d_nrm);
  HIPCHK(hipGetLastError());
  return o.finish();   // (the caller's spheres have been read)
}

// ---- include/loik_amd_depth.h (kernels in loik_pose_depth.hpp) --------------------------------------------------------------------
int loikb_depth_version(void) { return LOIKB_DEPTH_VERSION; }

static_assert(DEPTH_F32 == LOIKB_DEPTH_F32 && DEPTH_U16 == LOIKB_DEPTH_U16, "the kernels' constants and the header's");

// what is integrated: the pixels of a camera (points == nullptr) or n world points
struct DepthSource {
  const loikb_depth_camera* cam;
  const void* data;   // the image or the points, as the caller gave them
  int type;
  long long n;        // pixels or points
  size_t bytes;
};

// Steps 1 to 5 of loik_amd_depth.h behind both entry points.  The occupancy is written into C.d_occ, which no call keeps anything in
static int depth_integrate(loikb_solver_impl* S, const char* fn, const DepthSource& src, const int* dims, const double* origin, double h,
                           const loikb_depth_params* prm, const double* q_filter, int n_filter, int in_flags, long long* stats)
{
  const std::string f(fn);
  Collision& C = S->pose.col;
  if (!dims || !origin || !prm) { g_last_error = f + ": need dims, origin and params"; return LOIKB_ERR_ARG; }
  if (in_flags & ~(LOIKB_IN_DEVICE | LOIKB_DEPTH_Q_DEVICE)) { g_last_error = f + ": in_flags other than LOIKB_IN_DEVICE | LOIKB_DEPTH_Q_DEVICE"; return LOIKB_ERR_ARG; }
  if (prm->mode != LOIKB_DEPTH_REPLACE && prm->mode != LOIKB_DEPTH_FUSE) { g_last_error = f + ": mode is neither LOIKB_DEPTH_REPLACE nor LOIKB_DEPTH_FUSE"; return LOIKB_ERR_ARG; }
  if (prm->carve != 0 && prm->carve != 1) { g_last_error = f + ": carve must be 0 or 1"; return LOIKB_ERR_ARG; }
  if (prm->carve && prm->mode != LOIKB_DEPTH_FUSE) { g_last_error = f + ": carve needs LOIKB_DEPTH_FUSE"; return LOIKB_ERR_ARG; }
  if (prm->carve && !src.cam) { g_last_error = f + ": points have no camera to carve from: carve must be 0"; return LOIKB_ERR_ARG; }
  if (!(std::isfinite(prm->band) && prm->band >= 0.0) || !(std::isfinite(prm->filter_pad) && prm->filter_pad >= 0.0)) {
    g_last_error = f + ": band and filter_pad must be finite and >= 0";
    return LOIKB_ERR_ARG;
  }
  if (prm->flags != 0) { g_last_error = f + ": params flags other than 0"; return LOIKB_ERR_ARG; }
  if (n_filter < 0 || n_filter > LOIKB_DEPTH_MAX_FILTER) {
    g_last_error = f + ": n_filter outside 0 .. LOIKB_DEPTH_MAX_FILTER = " + std::to_string(LOIKB_DEPTH_MAX_FILTER);
    return LOIKB_ERR_ARG;
  }
  size_t nvox = 0;
  if (int rc = grid_check(S, fn, dims, origin, h, &nvox)) return rc;
  const bool fuse = prm->mode == LOIKB_DEPTH_FUSE && C.have_grid;
  if (fuse && !(C.gn[0] == dims[0] && C.gn[1] == dims[1] && C.gn[2] == dims[2] && C.go[0] == origin[0] && C.go[1] == origin[1] && C.go[2] == origin[2] && C.gh == h)) {
    g_last_error = f + ": LOIKB_DEPTH_FUSE onto a grid of other dims, origin or h than the one that is set";
    return LOIKB_ERR_STATE;
  }
  if (n_filter > 0) {
    if (C.ns == 0) { g_last_error = f + ": a self-filter needs collision spheres (loikb_collision_set_spheres)"; return LOIKB_ERR_STATE; }
    if (!q_filter && n_filter > S->B) { g_last_error = f + ": q_filter == NULL (the resident q) needs n_filter <= the batch"; return LOIKB_ERR_STATE; }
    if (!q_filter && !S->have_q) { g_last_error = f + ": no configurations resident on the device yet"; return LOIKB_ERR_STATE; }
  }
  HIPCHK(hipSetDevice(S->device));

  DepthCam cam{};
  DepthGrid g{};
  for (int k = 0; k < 3; ++k) { g.n[k] = dims[k]; g.o[k] = origin[k]; }
  g.h = h;
  g.inv_h = 1.0 / h;
  const void* d_src = src.data;
  if (src.n > 0 && !(in_flags & LOIKB_IN_DEVICE)) {
    if (int rc = regrow_drained(S, C.d_dsrc, src.bytes)) return rc;
    HIPCHK(hipMemcpyAsync(C.d_dsrc, src.data, src.bytes, hipMemcpyHostToDevice, S->stream));
    d_src = C.d_dsrc;
  }
  if (src.cam) {
    const loikb_depth_camera& c = *src.cam;
    cam.img = d_src; cam.type = src.type; cam.width = c.width; cam.height = c.height;
    cam.fx = c.fx; cam.fy = c.fy; cam.cx = c.cx; cam.cy = c.cy;
    for (int k = 0; k < 9; ++k) cam.R[k] = c.T_world_cam[k];
    for (int k = 0; k < 3; ++k) cam.p[k] = c.T_world_cam[9 + k];
    cam.scale = c.depth_scale; cam.z_min = c.z_min; cam.z_max = c.z_max;
  }
  int rc;
  if ((rc = regrow_drained(S, C.d_occ, nvox)) || (rc = regrow_drained(S, C.d_dstats, 4 * sizeof(unsigned long long)))) return rc;
  unsigned char* occ = C.d_occ;
  unsigned long long* d_stats = C.d_dstats;
  HIPCHK(hipMemsetAsync(d_stats, 0, 4 * sizeof(unsigned long long), S->stream));
  // 1, 2: the prior, less what the frame sees through
  if (fuse) {
    hipLaunchKernelGGL(k_depth_prior_carve, dim3(depth_blocks(nvox, DEPTH_RUN)), dim3(DEPTH_THREADS), 0, S->stream, (const unsigned int*)C.d_grid, occ, nvox,
                       g, cam, prm->carve, prm->band, d_stats);
    HIPCHK(hipGetLastError());
  } else {
    HIPCHK(hipMemsetAsync(occ, 0, nvox, S->stream));
  }
  // 3: the points
  if (src.n > 0) {
    hipLaunchKernelGGL(k_depth_scatter, grid1((size_t)src.n), dim3(DEPTH_THREADS), 0, S->stream, cam, src.cam ? (const double*)nullptr : (const double*)d_src,
                       src.n, g, occ, d_stats);
    HIPCHK(hipGetLastError());
  }
  // 4: the self-filter
  if (n_filter > 0) {
    const double* dq = S->d_q;
    if (q_filter) {
      dq = q_filter;
      if (!(in_flags & LOIKB_DEPTH_Q_DEVICE)) {
        const size_t qb = sizeof(double) * (size_t)n_filter * S->nq;
        if ((rc = regrow_drained(S, C.d_dq, qb))) return rc;
        HIPCHK(hipMemcpyAsync(C.d_dq, q_filter, qb, hipMemcpyHostToDevice, S->stream));
        dq = C.d_dq;
      }
    }
    const int ncar = (int)C.car.size();
    const size_t rows = (size_t)n_filter * C.ns;
    if ((rc = regrow_drained(S, C.d_place, sizeof(double) * (size_t)n_filter * ncar * 12)) || (rc = regrow_drained(S, C.d_dcen, sizeof(double) * 4 * rows))) return rc;
    hipLaunchKernelGGL(k_link_placements, grid1((size_t)n_filter * ncar), dim3(256), 0, S->stream, dq, S->nq, S->d_jd, S->d_idx_q, (const int*)C.d_car,
                       ncar, n_filter, C.d_place);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_depth_centres, grid1(rows), dim3(256), 0, S->stream, (const double*)C.d_place, clr_model(S), n_filter, prm->filter_pad, (double*)C.d_dcen);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_depth_filter, dim3((unsigned)((rows + DEPTH_THREADS / 64 - 1) / (DEPTH_THREADS / 64))), dim3(DEPTH_THREADS), 0, S->stream,
                       (const double*)C.d_dcen, (int)rows, g, occ);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_depth_count, dim3(depth_blocks(nvox, 16)), dim3(DEPTH_THREADS), 0, S->stream, (const unsigned char*)occ, nvox, d_stats);
  HIPCHK(hipGetLastError());
  unsigned long long st[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(st, d_stats, sizeof(st), hipMemcpyDeviceToHost, S->stream));
  // 5: the build, which drains the stream: st is complete, and the caller's image, points and q have been read
  if ((rc = grid_build_swap(S, occ, dims, origin, h))) { (void)hipStreamSynchronize(S->stream); return rc; }
  if (stats) {   // (k_depth_scatter keeps its two counters in one word)
    stats[0] = (long long)(st[0] & 0xffffffffull); stats[1] = (long long)(st[0] >> 32);
    stats[2] = (long long)st[2]; stats[3] = (long long)st[3];
  }
  return LOIKB_OK;
}

int loikb_collision_grid_integrate_depth(loikb_solver* S, const void* depth, int depth_type, const loikb_depth_camera* cam, const int* dims, const double* origin,
                                         double h, const loikb_depth_params* prm, const double* q_filter, int n_filter, int in_flags, long long* stats)
{
  const char* fn = "collision_grid_integrate_depth";
  const std::string f(fn);
  if (!S) return LOIKB_ERR_ARG;
  if (!depth || !cam) { g_last_error = f + ": need an image and a camera"; return LOIKB_ERR_ARG; }
  if (depth_type != LOIKB_DEPTH_F32 && depth_type != LOIKB_DEPTH_U16) { g_last_error = f + ": depth_type is neither LOIKB_DEPTH_F32 nor LOIKB_DEPTH_U16"; return LOIKB_ERR_ARG; }
  if (cam->width < 1 || cam->width > LOIKB_DEPTH_MAX_IMAGE || cam->height < 1 || cam->height > LOIKB_DEPTH_MAX_IMAGE) {
    g_last_error = f + ": width or height outside 1 .. LOIKB_DEPTH_MAX_IMAGE = " + std::to_string(LOIKB_DEPTH_MAX_IMAGE);
    return LOIKB_ERR_ARG;
  }
  if (!std::isfinite(cam->fx) || !std::isfinite(cam->fy) || !std::isfinite(cam->cx) || !std::isfinite(cam->cy) || !(cam->fx > 0.0) || !(cam->fy > 0.0)) {
    g_last_error = f + ": the intrinsics must be finite with fx, fy > 0";
    return LOIKB_ERR_ARG;
  }
  if (!frame_ok(cam->T_world_cam)) { g_last_error = f + ": T_world_cam is not finite or its rotation not orthonormal with determinant 1 (tolerance 1e-9)"; return LOIKB_ERR_ARG; }
  if (!(std::isfinite(cam->depth_scale) && cam->depth_scale > 0.0)) { g_last_error = f + ": depth_scale must be finite and > 0"; return LOIKB_ERR_ARG; }
  if (!(cam->z_min > 0.0 && cam->z_min <= cam->z_max && std::isfinite(cam->z_max))) { g_last_error = f + ": need 0 < z_min <= z_max < inf"; return LOIKB_ERR_ARG; }
  const long long n = (long long)cam->width * cam->height;
  const DepthSource src{cam, depth, depth_type, n, (size_t)n * (depth_type == LOIKB_DEPTH_F32 ? sizeof(float) : sizeof(unsigned short))};
  return depth_integrate(S, fn, src, dims, origin, h, prm, q_filter, n_filter, in_flags, stats);
}

int loikb_collision_grid_integrate_points(loikb_solver* S, const double* points, int n, const int* dims, const double* origin, double h,
                                          const loikb_depth_params* prm, const double* q_filter, int n_filter, int in_flags, long long* stats)
{
  const char* fn = "collision_grid_integrate_points";
  if (!S) return LOIKB_ERR_ARG;
  if (n < 0 || (n > 0 && !points)) { g_last_error = std::string(fn) + ": need n >= 0 and points when n > 0"; return LOIKB_ERR_ARG; }
  const DepthSource src{nullptr, points, 0, (long long)n, sizeof(double) * 3 * (size_t)n};
  return depth_integrate(S, fn, src, dims, origin, h, prm, q_filter, n_filter, in_flags, stats);
}

int loikb_collision_grid_get_occupancy(loikb_solver* S, unsigned char* occ, int out_flags)
{
  if (!S) return 0;
  if (out_flags & ~LOIKB_OUT_DEVICE) { g_last_error = "collision_grid_get_occupancy: out_flags other than LOIKB_OUT_DEVICE"; return LOIKB_ERR_ARG; }
  Collision& C = S->pose.col;
  if (!C.have_grid) return 0;
  if (occ) {
    HIPCHK(hipSetDevice(S->device));
    const size_t nvox = (size_t)C.gn[0] * C.gn[1] * C.gn[2];
    if (int rc = regrow_drained(S, C.d_occ, nvox)) return rc;   // (through the handle's buffer: the caller's need not be aligned)
    hipLaunchKernelGGL(k_depth_occupancy, grid1((nvox + DEPTH_RUN - 1) / DEPTH_RUN), dim3(DEPTH_THREADS), 0, S->stream, (const unsigned int*)C.d_grid,
                       (unsigned char*)C.d_occ, nvox);
    HIPCHK(hipGetLastError());
    if (int rc = get_copy_out(S, (const unsigned char*)C.d_occ, nvox, occ, out_flags)) return rc;
  }
  return 1;
}

// One clearance launch over n rows of the device array dq [n][nq] into d_min [n][3] and d_wit [n][3] (or nullptr).  Queued.
// As many of CLR_WAVES configurations per workgroup as 64 KB of LDS hold; a model of which one does not fit takes the carriers'
// placements from k_link_placements through C.d_place
static int col_launch(loikb_solver_impl* S, const double* dq, int n, double* d_min, int* d_wit)
{
  Collision& C = S->pose.col;
  const int ncar = (int)C.car.size();
  const bool hbm = clr_wave_doubles(S->nb, ncar, C.ns, false) * sizeof(double) > 65536;
  const size_t per = clr_wave_doubles(S->nb, ncar, C.ns, hbm) * sizeof(double);
  const int waves = lds_waves(CLR_WAVES, per);
  const ClrModel m = clr_model(S);
  const dim3 grid((unsigned)(((size_t)n + waves - 1) / waves)), block(64 * waves);
  if (hbm) {
    if (int rc = regrow_drained(S, C.d_place, sizeof(double) * (size_t)n * ncar * 12)) return rc;
    hipLaunchKernelGGL(k_link_placements, grid1((size_t)n * ncar), dim3(256), 0, S->stream, dq, S->nq, S->d_jd, S->d_idx_q, (const int*)C.d_car,
                       ncar, n, C.d_place);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_clearance<true>, grid, block, waves * per, S->stream, dq, S->nq, S->d_jd, S->d_idx_q, S->nb, n, m,
                       (const double*)C.d_place, d_min, d_wit);
  } else {
    hipLaunchKernelGGL(k_clearance<false>, grid, block, waves * per, S->stream, dq, S->nq, S->d_jd, S->d_idx_q, S->nb, n, m,
                       (const double*)nullptr, d_min, d_wit);
  }
  HIPCHK(hipGetLastError());
  return LOIKB_OK;
}

int loikb_clearance(loikb_solver* S, const double* q, int n, int in_flags, double* out_min, int* out_witness, int out_flags)
{
  if (!S) return LOIKB_ERR_ARG;
  if (n < 0 || (n > 0 && !out_min)) { g_last_error = "clearance: need n >= 0 and out_min when n > 0"; return LOIKB_ERR_ARG; }
  if (!q && n != S->B) { g_last_error = "clearance: q == NULL (the resident q) needs n == the batch"; return LOIKB_ERR_ARG; }
  if (S->pose.col.ns == 0) { g_last_error = "clearance: no spheres set (loikb_collision_set_spheres)"; return LOIKB_ERR_STATE; }
  if (!q && !S->have_q) { g_last_error = "clearance: no configurations resident on the device yet"; return LOIKB_ERR_STATE; }
  if (n == 0) return LOIKB_OK;
  HIPCHK(hipSetDevice(S->device));
  QueryOut o(S, out_flags);
  double* d_min;
  int* d_wit;
  o.add(out_min, sizeof(double) * 3 * (size_t)n, &d_min);
  o.add(out_witness, sizeof(int) * 3 * (size_t)n, &d_wit);
  int rc;
  const void* dq = S->d_q;
  if ((q && (rc = to_device(S, q, sizeof(double) * (size_t)n * S->nq, in_flags & LOIKB_IN_DEVICE, &dq))) || (rc = o.reserve()) ||
      (rc = col_launch(S, (const double*)dq, n, d_min, d_wit)))
    return rc;
  return o.finish();   // (the caller's q has been read)
}

int loikb_clearance_set_multistart(loikb_solver* S, const loikb_clearance_params* p)
{
  if (!S) return LOIKB_ERR_ARG;
  Collision& C = S->pose.col;
  if (!p) { C.have_ms = false; return LOIKB_OK; }
  if (!std::isfinite(p->margin) || p->flags != 0) { g_last_error = "clearance_set_multistart: need a finite margin and flags 0"; return LOIKB_ERR_ARG; }
  if (C.ns == 0) { g_last_error = "clearance_set_multistart: no spheres set (loikb_collision_set_spheres)"; return LOIKB_ERR_STATE; }
  C.ms = *p;
  C.have_ms = true;
  return LOIKB_OK;
}

int loikb_clearance_get_multistart(const loikb_solver* S, loikb_clearance_params* out)
{
  if (!S || !S->pose.col.have_ms) return 0;
  if (out) *out = S->pose.col.ms;
  return 1;
}

// ---- include/loik_amd_avoid.h (kernels in loik_pose_avoid.hpp) -----------------------------------------------------------------
int loikb_avoid_version(void) { return LOIKB_AVOID_VERSION; }

static_assert(AVD_MAX_SPHERES == LOIKB_AVOID_MAX_SPHERES, "the kernel's table and the header's limit");
static_assert(AVD_MAX_SPHERES < (int)AVD_NO_SPHERE, "a list entry holds a sphere index in 16 bits, 0xffff for none");

// the state every avoidance call asks for: 1 .. LOIKB_AVOID_MAX_SPHERES spheres, and a model whose table fits one wavefront's LDS
static int avoid_check_model(const loikb_solver_impl* S, const char* fn)
{
  const Collision& C = S->pose.col;
  const std::string f(fn);
  if (C.ns == 0) { g_last_error = f + ": no spheres set (loikb_collision_set_spheres)"; return LOIKB_ERR_STATE; }
  if (C.have_grid && !C.near_on) {
    g_last_error = f + ": a voxel grid is set (loikb_collision_set_world_grid), and its clearance bound has no gradient for avoidance to follow -- clear the grid first."
                       "  With the nearest-voxel transform latched (loikb_collision_grid_set_nearest) avoidance reads the grid.";
    return LOIKB_ERR_STATE;
  }
  if (C.ns > LOIKB_AVOID_MAX_SPHERES) {
    g_last_error = f + ": " + std::to_string(C.ns) + " spheres set, more than LOIKB_AVOID_MAX_SPHERES = " + std::to_string(LOIKB_AVOID_MAX_SPHERES);
    return LOIKB_ERR_STATE;
  }
  if (avd_wave_doubles(S->nb, C.ns, true) * sizeof(double) > 65536) {
    g_last_error = f + ": the ancestor table of a model with this many DoFs does not fit one wavefront's 64 KB of LDS";
    return LOIKB_ERR_STATE;
  }
  return LOIKB_OK;
}

static bool avoid_params_ok(const loikb_avoid_params* p)
{
  return p && std::isfinite(p->d_safe) && std::isfinite(p->d_influence) && p->d_influence > p->d_safe && p->kappa > 0.0 && p->kappa <= 1.0 && p->flags == 0;
}

// One k_avoid_box launch in `mode` over n rows of the device array dq [n][nq].  Queued.  The launch rule of col_launch
static int avoid_launch(loikb_solver_impl* S, int mode, const double* dq, int n, const AvoidPrm& prm, const AvoidIO& io)
{
  Collision& C = S->pose.col;
  loikb_solver_impl::PoseState::Avoid& A = S->pose.avoid;
  const bool hbm = avd_wave_doubles(S->nb, C.ns, false) * sizeof(double) > 65536;
  const size_t per = avd_wave_doubles(S->nb, C.ns, hbm) * sizeof(double);
  const int waves = lds_waves(CLR_WAVES, per);
  const ClrModel m = clr_model(S);
  const dim3 grid((unsigned)(((size_t)n + waves - 1) / waves)), block(64 * waves);
  const size_t lds = waves * per;
  const double* place = nullptr;
  if (hbm) {
    if (int rc = regrow_drained(S, A.d_place, sizeof(double) * (size_t)n * S->nb * 12)) return rc;
    // (the rounding of the LDS stages: the centres have the bits of k_avoid_box<false> and of k_clearance<false>)
    hipLaunchKernelGGL(k_avoid_placements, grid1((size_t)n * S->nb), dim3(256), 0, S->stream, dq, S->nq, S->d_jd, S->d_idx_q, S->nb, n, (double*)A.d_place);
    HIPCHK(hipGetLastError());
    place = A.d_place;
  }
#define LOIKB_AVD_LAUNCH(H, M, T) \
  hipLaunchKernelGGL((k_avoid_box<H, M, T>), grid, block, lds, S->stream, dq, S->nq, S->d_jd, S->d_idx_q, S->nb, n, m, place, prm, io)
  if (mode == AVD_GRAD) { if (hbm) LOIKB_AVD_LAUNCH(true, AVD_GRAD, double); else LOIKB_AVD_LAUNCH(false, AVD_GRAD, double); }
  else if (mode == AVD_QUERY) { if (hbm) LOIKB_AVD_LAUNCH(true, AVD_QUERY, double); else LOIKB_AVD_LAUNCH(false, AVD_QUERY, double); }
  else if (S->f32) { if (hbm) LOIKB_AVD_LAUNCH(true, AVD_STEP, float); else LOIKB_AVD_LAUNCH(false, AVD_STEP, float); }
  else { if (hbm) LOIKB_AVD_LAUNCH(true, AVD_STEP, double); else LOIKB_AVD_LAUNCH(false, AVD_STEP, double); }
#undef LOIKB_AVD_LAUNCH
  HIPCHK(hipGetLastError());
  return LOIKB_OK;
}

// a pose loop that runs with the latch starts: its result buffers (pose_box_begin)
static int avoid_begin(loikb_solver_impl* S)
{
  loikb_solver_impl::PoseState::Avoid& A = S->pose.avoid;
  int rc;
  if ((rc = avoid_check_model(S, "a pose loop with collision avoidance (loikb_avoid_set)"))) return rc;
  const size_t B = (size_t)S->B;
  if ((rc = regrow(A.d_minseen, sizeof(double) * B)) || (rc = regrow(A.d_asteps, sizeof(int) * B)) || (rc = regrow(A.d_aflags, sizeof(int) * B * S->nb)))
    return rc;
  hipLaunchKernelGGL(k_avoid_reset, grid1(B * S->nb), dim3(256), 0, S->stream, S->B, S->nb, (double*)A.d_minseen, (int*)A.d_asteps, (int*)A.d_aflags);
  HIPCHK(hipGetLastError());
  A.valid = true;
  return LOIKB_OK;
}

// the step's box narrowed from the resident q (pose_step)
static int avoid_step(loikb_solver_impl* S, double dt, const PoseBoxScope& box, const int* d_status, bool from_tiles)
{
  loikb_solver_impl::PoseState& P = S->pose;
  loikb_solver_impl::PoseState::Avoid& A = P.avoid;
  AvoidIO io{};
  io.status = d_status;
  io.base_sh = box.was_shared ? (const void*)((const char*)S->d_uni + (size_t)S->nc * 57 * S->esz) : nullptr;
  io.base_pi = (const double2*)P.d_box;
  io.from_tiles = from_tiles ? 1 : 0;
  io.tiles = S->home.tiles;
  io.L = S->L;
  io.min_seen = A.d_minseen; io.asteps = A.d_asteps; io.aflags = A.d_aflags;
  const AvoidPrm prm{A.prm.d_safe, A.prm.d_influence, A.prm.kappa, dt};
  return avoid_launch(S, AVD_STEP, (const double*)S->d_q, S->B, prm, io);
}

// what loikb_clearance asks of (q, n), for the two queries of this header
static int avoid_check_rows(const loikb_solver_impl* S, const char* fn, const double* q, int n, bool outputs)
{
  const std::string f(fn);
  if (n < 0 || (n > 0 && !outputs)) { g_last_error = f + ": need n >= 0 and every output array when n > 0"; return LOIKB_ERR_ARG; }
  if (!q && n != S->B) { g_last_error = f + ": q == NULL (the resident q) needs n == the batch"; return LOIKB_ERR_ARG; }
  return LOIKB_OK;
}

int loikb_clearance_gradient(loikb_solver* S, const double* q, int n, int in_flags, double* out_min, int* out_witness, double* out_grad, int out_flags)
{
  if (!S) return LOIKB_ERR_ARG;
  int rc;
  if ((rc = avoid_check_rows(S, "clearance_gradient", q, n, out_min && out_witness && out_grad))) return rc;
  if ((rc = avoid_check_model(S, "clearance_gradient"))) return rc;
  if (!q && !S->have_q) { g_last_error = "clearance_gradient: no configurations resident on the device yet"; return LOIKB_ERR_STATE; }
  if (n == 0) return LOIKB_OK;
  HIPCHK(hipSetDevice(S->device));
  QueryOut o(S, out_flags);
  AvoidIO io{};
  o.add(out_min, sizeof(double) * 3 * (size_t)n, &io.out_min);
  o.add(out_grad, sizeof(double) * (size_t)n * S->nb, &io.out_grad);
  o.add(out_witness, sizeof(int) * 3 * (size_t)n, &io.out_wit);
  const void* dq = S->d_q;
  if ((q && (rc = to_device(S, q, sizeof(double) * (size_t)n * S->nq, in_flags & LOIKB_IN_DEVICE, &dq))) || (rc = o.reserve())) return rc;
  const AvoidPrm prm{0.0, 0.0, 1.0, 1.0};
  if ((rc = avoid_launch(S, AVD_GRAD, (const double*)dq, n, prm, io))) return rc;
  return o.finish();   // (the caller's q has been read)
}

int loikb_avoid_set(loikb_solver* S, const loikb_avoid_params* p)
{
  if (!S) return LOIKB_ERR_ARG;
  loikb_solver_impl::PoseState::Avoid& A = S->pose.avoid;
  if (!p) { A.have = false; return LOIKB_OK; }
  if (!avoid_params_ok(p)) { g_last_error = "avoid_set: need a finite d_safe, a finite d_influence > d_safe, 0 < kappa <= 1 and flags 0"; return LOIKB_ERR_ARG; }
  if (int rc = avoid_check_model(S, "avoid_set")) return rc;
  A.prm = *p;
  A.have = true;
  return LOIKB_OK;
}

int loikb_avoid_get(const loikb_solver* S, loikb_avoid_params* out)
{
  if (!S || !S->pose.avoid.have) return 0;
  if (out) *out = S->pose.avoid.prm;
  return 1;
}

int loikb_avoid_box(loikb_solver* S, const double* q, int n, int in_flags, double dt, const double* lb, const double* ub, const loikb_avoid_params* p,
                    double* out_lo, double* out_hi, double* out_pairs, int* out_partner, int out_flags)
{
  if (!S) return LOIKB_ERR_ARG;
  int rc;
  if ((rc = avoid_check_rows(S, "avoid_box", q, n, out_lo && out_hi && out_pairs && out_partner))) return rc;
  if (!avoid_params_ok(p)) { g_last_error = "avoid_box: need params with a finite d_safe, a finite d_influence > d_safe, 0 < kappa <= 1 and flags 0"; return LOIKB_ERR_ARG; }
  if (!(dt > 0.0) || std::isinf(dt)) { g_last_error = "avoid_box: need a finite dt > 0"; return LOIKB_ERR_ARG; }
  if (!lb || !ub) { g_last_error = "avoid_box: need lb and ub [nv]"; return LOIKB_ERR_ARG; }
  for (int j = 0; j < S->nb; ++j)
    if (std::isnan(lb[j]) || std::isnan(ub[j]) || lb[j] > ub[j]) { g_last_error = "avoid_box: DoF " + std::to_string(j) + ": a bound is NaN, or lb > ub"; return LOIKB_ERR_ARG; }
  if ((rc = avoid_check_model(S, "avoid_box"))) return rc;
  if (!q && !S->have_q) { g_last_error = "avoid_box: no configurations resident on the device yet"; return LOIKB_ERR_STATE; }
  if (n == 0) return LOIKB_OK;
  HIPCHK(hipSetDevice(S->device));
  loikb_solver_impl::PoseState::Avoid& A = S->pose.avoid;
  const int ns = S->pose.col.ns, nb = S->nb;
  const size_t bbytes = sizeof(double) * (size_t)n * nb;
  QueryOut o(S, out_flags);
  AvoidIO io{};
  o.add(out_lo, bbytes, &io.out_lo);
  o.add(out_hi, bbytes, &io.out_hi);
  o.add(out_pairs, sizeof(double) * 2 * (size_t)n * ns, &io.out_pairs);
  o.add(out_partner, sizeof(int) * 2 * (size_t)n * ns, &io.out_partner);
  const void* dq = S->d_q;
  if ((q && (rc = to_device(S, q, sizeof(double) * (size_t)n * S->nq, in_flags & LOIKB_IN_DEVICE, &dq))) || (rc = regrow(A.d_base, sizeof(double) * 2 * nb)) ||
      (rc = o.reserve()))
    return rc;
  HIPCHK(hipMemcpyAsync(A.d_base, lb, sizeof(double) * nb, hipMemcpyHostToDevice, S->stream));
  HIPCHK(hipMemcpyAsync((double*)A.d_base + nb, ub, sizeof(double) * nb, hipMemcpyHostToDevice, S->stream));
  io.lb = A.d_base; io.ub = (const double*)A.d_base + nb;
  const AvoidPrm prm{p->d_safe, p->d_influence, p->kappa, dt};
  if ((rc = avoid_launch(S, AVD_QUERY, (const double*)dq, n, prm, io))) return rc;
  return o.finish();   // (the caller's q, lb and ub have been read)
}

int loikb_avoid_get_result(loikb_solver* S, int field, void* out, int out_flags)
{
  if (!S || !out) return LOIKB_ERR_ARG;
  loikb_solver_impl::PoseState::Avoid& A = S->pose.avoid;
  if (field < LOIKB_AVOID_F_MIN_SEEN || field > LOIKB_AVOID_F_FLAGS) { g_last_error = "avoid_get_result: unknown field"; return LOIKB_ERR_ARG; }
  if (S->pose.nc == 0 || !A.valid) { g_last_error = "avoid_get_result: the last pose loop ran without collision avoidance (loikb_avoid_set), or there was none"; return LOIKB_ERR_STATE; }
  HIPCHK(hipSetDevice(S->device));
  const size_t B = (size_t)S->B;
  switch (field) {
  case LOIKB_AVOID_F_MIN_SEEN: return get_copy_out(S, A.d_minseen, sizeof(double) * B, out, out_flags);
  case LOIKB_AVOID_F_ACTIVE_STEPS: return get_copy_out(S, A.d_asteps, sizeof(int) * B, out, out_flags);
  default: return get_copy_out(S, A.d_aflags, sizeof(int) * B * S->nb, out, out_flags);
  }
}

// the buffers of the collision-aware selection, on first use
static int ms_clr_alloc(loikb_solver_impl* S)
{
  loikb_solver_impl::MultiStartState& M = S->ms;
  if (M.d_nclear) return LOIKB_OK;
  const size_t B = (size_t)S->B;
  int rc;
  if ((rc = alloc_dev(S, (void**)&M.d_clr, sizeof(double) * B * 3)) || (rc = alloc_dev(S, (void**)&M.d_clrwit, sizeof(int) * B * 3)) ||
      (rc = alloc_dev(S, (void**)&M.d_lstatus, sizeof(int) * B)) || (rc = alloc_dev(S, (void**)&M.d_iclr, sizeof(double) * B)) ||
      (rc = alloc_dev(S, (void**)&M.d_wclr, sizeof(double) * B)) || (rc = alloc_dev(S, (void**)&M.d_wwit, sizeof(int) * B * 3)) ||
      (rc = alloc_dev(S, (void**)&M.d_nclear, sizeof(int) * B))) {
    M.d_nclear = nullptr;   // (as pose_alloc: what was allocated goes with the handle; the next call allocates afresh)
    return rc;
  }
  return LOIKB_OK;
}

int loikb_clearance_get_multistart_result(loikb_solver* S, int field, void* out, int out_flags)
{
  if (!S || !out) return LOIKB_ERR_ARG;
  const loikb_solver_impl::MultiStartState& M = S->ms;
  if (M.G == 0 || !M.clr_valid) { g_last_error = "clearance_get_multistart_result: the last solve_pose_multistart did not run with loikb_clearance_set_multistart"; return LOIKB_ERR_STATE; }
  HIPCHK(hipSetDevice(S->device));
  const void* src = nullptr;
  size_t bytes = 0;
  const size_t G = (size_t)M.G;
  switch (field) {
  case LOIKB_CLR_MS_F_CLEARANCE: src = M.d_wclr; bytes = sizeof(double) * G; break;
  case LOIKB_CLR_MS_F_WITNESS: src = M.d_wwit; bytes = sizeof(int) * G * 3; break;
  case LOIKB_CLR_MS_F_NCLEAR: src = M.d_nclear; bytes = sizeof(int) * G; break;
  case LOIKB_CLR_MS_F_INSTANCE: src = M.d_iclr; bytes = sizeof(double) * (size_t)S->B; break;
  default: g_last_error = "clearance_get_multistart_result: unknown field"; return LOIKB_ERR_ARG;
  }
  return get_copy_out(S, src, bytes, out, out_flags);
}

// ---- include/loik_amd_multistart.h (kernels in loik_pose_multistart.hpp) ------------------------------------------------------
int loikb_multistart_version(void) { return LOIKB_MULTISTART_VERSION; }

static int ms_alloc(loikb_solver_impl* S)
{
  loikb_solver_impl::MultiStartState& M = S->ms;
  if (M.d_count) return LOIKB_OK;
  const size_t B = (size_t)S->B, nc = (size_t)std::max(S->nc, 1), nq = (size_t)S->nq, nv = (size_t)S->nb;
  int rc;
  if ((rc = alloc_dev(S, (void**)&M.d_tgt_in, sizeof(double) * B * nc * 12)) || (rc = alloc_dev(S, (void**)&M.d_tgt, sizeof(double) * B * nc * 12)) ||
      (rc = alloc_dev(S, (void**)&M.d_q0, sizeof(double) * B * nq)) || (rc = alloc_dev(S, (void**)&M.d_table, sizeof(int) * nq)) ||
      (rc = alloc_dev(S, (void**)&M.d_dofq, sizeof(int) * nv)) || (rc = alloc_dev(S, (void**)&M.d_lo, sizeof(double) * nv)) ||
      (rc = alloc_dev(S, (void**)&M.d_hi, sizeof(double) * nv)) || (rc = alloc_dev(S, (void**)&M.d_w, sizeof(double) * nv)) ||
      (rc = alloc_dev(S, (void**)&M.d_round, sizeof(int) * B)) || (rc = alloc_dev(S, (void**)&M.d_winner, sizeof(int) * B)) ||
      (rc = alloc_dev(S, (void**)&M.d_gstatus, sizeof(int) * B)) || (rc = alloc_dev(S, (void**)&M.d_nreached, sizeof(int) * B)) ||
      (rc = alloc_dev(S, (void**)&M.d_cost, sizeof(double) * B)) || (rc = alloc_dev(S, (void**)&M.d_wq, sizeof(double) * B * nq)) ||
      (rc = alloc_dev(S, (void**)&M.d_werr, sizeof(double) * B * nc * 6)) || (rc = alloc_dev(S, (void**)&M.d_count, sizeof(unsigned int) * 2))) {
    M.d_count = nullptr;   // (as pose_alloc: what was allocated goes with the handle; the next call allocates afresh)
    return rc;
  }
  return LOIKB_OK;
}

// The ranges in force into M.up_lo / up_hi / up_table: those of loikb_multistart_set_ranges, else the joint limits of the handle.
// A DoF is sampled iff both ends are finite.  Returns the number of sampled DoFs; touches nothing on the device.
static int ms_resolve_ranges(loikb_solver_impl* S)
{
  loikb_solver_impl::MultiStartState& M = S->ms;
  const loikb_solver_impl::PoseState& P = S->pose;
  const double inf = std::numeric_limits<double>::infinity();
  M.up_lo.assign(S->nv, -inf);
  M.up_hi.assign(S->nv, inf);
  M.up_table.assign(S->nq, -1);
  int sampled = 0;
  for (int j = 0; j < S->nv; ++j) {
    if (M.have_ranges) { M.up_lo[j] = M.lo[j]; M.up_hi[j] = M.hi[j]; }
    else if (P.have_limits) { M.up_lo[j] = P.lim[j].lo; M.up_hi[j] = P.lim[j].hi; }
    if (std::isfinite(M.up_lo[j]) && std::isfinite(M.up_hi[j]) && S->lim_q[j] >= 0) { M.up_table[S->lim_q[j]] = j; ++sampled; }
  }
  return sampled;
}

// the tables of the sampler and of the selection onto the device (queued; the sources are members of the handle)
static int ms_upload_tables(loikb_solver_impl* S)
{
  loikb_solver_impl::MultiStartState& M = S->ms;
  HIPCHK(hipMemcpyAsync(M.d_lo, M.up_lo.data(), sizeof(double) * S->nv, hipMemcpyHostToDevice, S->stream));
  HIPCHK(hipMemcpyAsync(M.d_hi, M.up_hi.data(), sizeof(double) * S->nv, hipMemcpyHostToDevice, S->stream));
  HIPCHK(hipMemcpyAsync(M.d_table, M.up_table.data(), sizeof(int) * S->nq, hipMemcpyHostToDevice, S->stream));
  HIPCHK(hipMemcpyAsync(M.d_dofq, S->lim_q.data(), sizeof(int) * S->nv, hipMemcpyHostToDevice, S->stream));
  if (!M.w.empty()) HIPCHK(hipMemcpyAsync(M.d_w, M.w.data(), sizeof(double) * S->nv, hipMemcpyHostToDevice, S->stream));
  return LOIKB_OK;
}

// the goals' q0 rows into M.d_q0: the caller's [G][nq] (host / device), one shared host row, or the resident row g * K
static int ms_set_q0(loikb_solver_impl* S, const double* q0, int flags, int G, int K)
{
  loikb_solver_impl::MultiStartState& M = S->ms;
  const bool shared = q0 && (flags & LOIKB_Q_SHARED), dev = q0 && (flags & LOIKB_IN_DEVICE) && !shared;
  const void* src = S->d_q;
  size_t stride = (size_t)K * S->nq;
  int rc;
  if (q0) {
    if ((rc = to_device(S, q0, sizeof(double) * (shared ? (size_t)S->nq : (size_t)G * S->nq), dev, &src))) return rc;
    stride = shared ? 0 : (size_t)S->nq;
  }
  hipLaunchKernelGGL(k_ms_set_q0, grid1((size_t)G * S->nq), dim3(256), 0, S->stream, (const double*)src, stride, S->nq, G, M.d_q0);
  HIPCHK(hipGetLastError());
  return LOIKB_OK;
}

static unsigned long long ms_mix_host(unsigned long long x)
{
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// the seeds of `round` into the resident q (status == nullptr: every row; else the rows without REACHED).  The handle is left as
// loikb_solve_pose(q != NULL) leaves it after its copy: q resident, the inputs changed.
static int ms_sample(loikb_solver_impl* S, unsigned long long seed, int K, int round, const int* status)
{
  loikb_solver_impl::MultiStartState& M = S->ms;
  const unsigned long long key = ms_mix_host(seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)round + 1ull));
  hipLaunchKernelGGL(k_ms_sample, grid1((size_t)S->B * S->nq), dim3(256), 0, S->stream, S->d_q, (const double*)M.d_q0, S->nq, S->B, K,
                     (const int*)M.d_table, (const double*)M.d_lo, (const double*)M.d_hi, key, round, status, M.d_round);
  HIPCHK(hipGetLastError());
  S->have_q = true;
  ++S->inputs_epoch;
  return LOIKB_OK;
}

int loikb_multistart_set_ranges(loikb_solver* S, const double* s_lo, const double* s_hi, const double* weights, int n)
{
  if (!S) return LOIKB_ERR_ARG;
  loikb_solver_impl::MultiStartState& M = S->ms;
  int rc;
  if ((s_lo || s_hi) && (rc = check_dof_pairs(S, "multistart_set_ranges", "s_lo", "s_hi", s_lo, s_hi, n))) return rc;
  if (weights) {
    if (n != S->nv) { g_last_error = "multistart_set_ranges: need one weight per DoF, n == model.nv"; return LOIKB_ERR_ARG; }
    for (int j = 0; j < n; ++j)
      if (!(weights[j] >= 0.0) || !std::isfinite(weights[j])) { g_last_error = "multistart_set_ranges: a weight is negative or not finite"; return LOIKB_ERR_ARG; }
  }
  M.have_ranges = s_lo != nullptr;
  if (s_lo) { M.lo.assign(s_lo, s_lo + n); M.hi.assign(s_hi, s_hi + n); }
  if (weights) M.w.assign(weights, weights + n);
  else M.w.clear();
  return LOIKB_OK;
}

int loikb_multistart_sample(loikb_solver* S, const double* q0, int q0_flags, unsigned long long seed, int seeds_per_goal, int round)
{
  if (!S) return LOIKB_ERR_ARG;
  const int K = seeds_per_goal;
  if (K < 1 || S->B % K != 0 || round < 0) { g_last_error = "multistart_sample: need seeds_per_goal >= 1 that divides the batch, round >= 0"; return LOIKB_ERR_ARG; }
  if (!S->have_problem) { g_last_error = "multistart_sample before SolveInit()"; return LOIKB_ERR_STATE; }
  if (!q0 && !S->have_q) { g_last_error = "multistart_sample: no configurations resident on the device yet"; return LOIKB_ERR_STATE; }
  if (ms_resolve_ranges(S) == 0 && (K > 1 || round > 0)) {
    g_last_error = "multistart_sample: no DoF to sample (set ranges with loikb_multistart_set_ranges or joint limits with a finite pair)";
    return LOIKB_ERR_STATE;
  }
  HIPCHK(hipSetDevice(S->device));
  int rc;
  if ((rc = ms_alloc(S)) || (rc = ms_upload_tables(S)) || (rc = ms_set_q0(S, q0, q0_flags, S->B / K, K)) || (rc = ms_sample(S, seed, K, round, nullptr))) {
    (void)hipStreamSynchronize(S->stream);
    return rc;
  }
  HIPCHK(hipStreamSynchronize(S->stream));   // (the caller's q0 has been read)
  return LOIKB_OK;
}

int loikb_solve_pose_multistart(loikb_solver* S, const double* q0, const double* targets, int in_flags, const loikb_pose_params* pose,
                                const loikb_multistart_params* ms)
{
  if (!S || !targets || !pose || !ms) return LOIKB_ERR_ARG;
  const int K = ms->seeds_per_goal, R = ms->rounds;
  if (K < 1 || S->B % K != 0 || R < 1 || ms->pick < LOIKB_MS_PICK_NEAREST || ms->pick > LOIKB_MS_PICK_FIRST || ms->flags != 0) {
    g_last_error = "solve_pose_multistart: need seeds_per_goal >= 1 that divides the batch, rounds >= 1, pick 0 or 1, flags 0";
    return LOIKB_ERR_ARG;
  }
  if (S->pose.have_accel) {
    g_last_error = "solve_pose_multistart: the handle has joint acceleration limits (loikb_set_joint_accel_limits); the seeds of a multi-start are teleported into the resident q between rounds, a rate limit means nothing there -- clear the acceleration limits first";
    return LOIKB_ERR_STATE;
  }
  if (int pre = pose_preconditions(S, pose, !q0)) return pre;
  if (S->pose.col.have_ms && S->pose.col.ns == 0) {
    g_last_error = "solve_pose_multistart: the handle has the collision-aware selection (loikb_clearance_set_multistart) and no spheres (loikb_collision_set_spheres)";
    return LOIKB_ERR_STATE;
  }
  if (ms_resolve_ranges(S) == 0 && (K > 1 || R > 1)) {
    g_last_error = "solve_pose_multistart: no DoF to sample (set ranges with loikb_multistart_set_ranges or joint limits with a finite pair)";
    return LOIKB_ERR_STATE;
  }
  const auto t_call = std::chrono::steady_clock::now();
  HIPCHK(hipSetDevice(S->device));
  int rc;
  if ((rc = ms_alloc(S))) return rc;
  loikb_solver_impl::MultiStartState& M = S->ms;
  const bool have_clr = S->pose.col.have_ms;   // the collision-aware selection (loik_amd_collision.h)
  const double margin = S->pose.col.ms.margin;
  if (have_clr && (rc = ms_clr_alloc(S))) return rc;
  const int B = S->B, G = B / K, nc = S->nc_active;
  const bool dev = in_flags & LOIKB_IN_DEVICE, tgt_shared = in_flags & LOIKB_POSE_TARGET_SHARED;
  // the targets, checked as loikb_solve_pose checks them, before anything of the handle changes
  if ((rc = pose_check_targets(S, M.d_tgt_in, targets, (size_t)(tgt_shared ? 1 : G) * nc, dev, M.d_count,
                               "solve_pose: a target rotation is not orthonormal with determinant 1 (tolerance 1e-9)")))
    return rc;
  const auto t_sample = std::chrono::steady_clock::now();
  double sample_ms = 0.0, solve_ms = 0.0, select_ms = 0.0;
  hipLaunchKernelGGL(k_ms_expand_targets, grid1((size_t)B * nc * 12), dim3(256), 0, S->stream, (const double*)M.d_tgt_in, (int)tgt_shared, nc, K, B, M.d_tgt);
  HIPCHK(hipGetLastError());
  if ((rc = ms_upload_tables(S)) || (rc = ms_set_q0(S, q0, in_flags, G, K)) || (rc = ms_sample(S, ms->seed, K, 0, nullptr))) {
    (void)hipStreamSynchronize(S->stream);
    return rc;
  }
  HIPCHK(hipStreamSynchronize(S->stream));   // (the caller's q0 has been read)
  sample_ms += ms_since(t_sample);
  M.G = 0;
  const loikb_solver_impl::PoseState& P = S->pose;
  auto select = [&](int count_only) -> int {
    const double* cost_in = nullptr;   // the dexterous pick (loik_amd_jacobian.h): the final selection's cost of a reached seed
    if (!count_only && P.have_dex) {
      int rcd;
      if ((rcd = ms_dex_cost(S))) return rcd;
      cost_in = M.d_dexcost;
    }
    HIPCHK(hipMemsetAsync(M.d_count, 0, sizeof(unsigned int), S->stream));
    hipLaunchKernelGGL(k_ms_select, dim3((unsigned)G), dim3(MS_SELECT_THREADS), 0, S->stream, (const int*)P.d_status, (const double*)P.d_err,
                       (const double*)S->d_q, (const double*)M.d_q0, (const int*)M.d_dofq, M.w.empty() ? (const double*)nullptr : (const double*)M.d_w,
                       S->nv, S->nq, nc, K, (int)(ms->pick == LOIKB_MS_PICK_FIRST), count_only, M.d_count, M.d_winner, M.d_gstatus, M.d_cost,
                       M.d_nreached, M.d_wq, M.d_werr, cost_in, have_clr ? (const double*)M.d_clr : nullptr, (const int*)M.d_clrwit, margin,
                       M.d_iclr, M.d_wclr, M.d_wwit, M.d_nclear);
    HIPCHK(hipGetLastError());
    return LOIKB_OK;
  };
  int rounds_run = 0;
  for (int r = 0; r < R; ++r) {
    const auto t_solve = std::chrono::steady_clock::now();
    if ((rc = loikb_solve_pose(S, nullptr, M.d_tgt, LOIKB_IN_DEVICE, pose))) return rc;
    solve_ms += ms_since(t_solve);
    ++rounds_run;
    // clr[b] of the resident q the round left: one launch, read on the device by the selection and the re-sampler's status word
    if (have_clr && (rc = col_launch(S, (const double*)S->d_q, B, M.d_clr, M.d_clrwit))) return rc;
    if (r == R - 1) break;
    // goals that own a reached seed: one counter back to the host
    const auto t_count = std::chrono::steady_clock::now();
    if ((rc = select(1))) return rc;
    unsigned int answered = 0;
    HIPCHK(hipMemcpyAsync(&answered, M.d_count, sizeof(answered), hipMemcpyDeviceToHost, S->stream));
    HIPCHK(hipStreamSynchronize(S->stream));
    select_ms += ms_since(t_count);
    if (answered == (unsigned int)G) break;
    const auto t_again = std::chrono::steady_clock::now();
    const int* again = P.d_status;
    if (have_clr) {   // class 0c is drawn anew: a loop-private status word, the pose status the caller reads is not edited
      hipLaunchKernelGGL(k_ms_loop_status, grid1(B), dim3(256), 0, S->stream, (const int*)P.d_status, (const double*)M.d_clr, margin, B, M.d_lstatus);
      HIPCHK(hipGetLastError());
      again = M.d_lstatus;
    }
    if ((rc = ms_sample(S, ms->seed, K, r + 1, again))) return rc;
    HIPCHK(hipStreamSynchronize(S->stream));
    sample_ms += ms_since(t_again);
  }
  const auto t_select = std::chrono::steady_clock::now();
  if ((rc = select(0))) return rc;
  HIPCHK(hipStreamSynchronize(S->stream));
  select_ms += ms_since(t_select);
  M.G = G;
  M.nc = nc;
  M.clr_valid = have_clr;
  const double total = ms_since(t_call);
  M.timing[0] = rounds_run; M.timing[1] = total; M.timing[2] = solve_ms; M.timing[3] = sample_ms; M.timing[4] = select_ms;
  M.timing[5] = total - solve_ms - sample_ms - select_ms;
  return LOIKB_OK;
}

int loikb_multistart_get(loikb_solver* S, int field, void* out, int out_flags)
{
  if (!S || !out) return LOIKB_ERR_ARG;
  const loikb_solver_impl::MultiStartState& M = S->ms;
  if (M.G == 0) { g_last_error = "multistart_get before solve_pose_multistart"; return LOIKB_ERR_STATE; }
  HIPCHK(hipSetDevice(S->device));
  const void* src = nullptr;
  size_t bytes = 0;
  const size_t G = (size_t)M.G;
  switch (field) {
  case LOIKB_MS_F_WINNER: src = M.d_winner; bytes = sizeof(int) * G; break;
  case LOIKB_MS_F_GOAL_STATUS: src = M.d_gstatus; bytes = sizeof(int) * G; break;
  case LOIKB_MS_F_Q: src = M.d_wq; bytes = sizeof(double) * G * S->nq; break;
  case LOIKB_MS_F_ERR: src = M.d_werr; bytes = sizeof(double) * G * M.nc * 6; break;
  case LOIKB_MS_F_COST: src = M.d_cost; bytes = sizeof(double) * G; break;
  case LOIKB_MS_F_NREACHED: src = M.d_nreached; bytes = sizeof(int) * G; break;
  case LOIKB_MS_F_ROUND: src = M.d_round; bytes = sizeof(int) * (size_t)S->B; break;
  case LOIKB_MS_F_TIMING: return get_timing_out(M.timing, sizeof(M.timing), out, out_flags & LOIKB_OUT_DEVICE);
  default: g_last_error = "multistart_get: unknown field"; return LOIKB_ERR_ARG;
  }
  return get_copy_out(S, src, bytes, out, out_flags);
}

// ---- include/loik_amd_path.h (kernels in loik_pose_path.hpp) ------------------------------------------------------------------
int loikb_path_version(void) { return LOIKB_PATH_VERSION; }

// The buffers of the path and track states that are sized by the waypoint / step count are grown (never shrunk) with replace():
// a call that fails to grow one keeps the results of the last; their contents are not kept across a growth.  (No size is zero:
// both entry points insist on a count >= 1.)

// the [B] arrays on first use, and room for T waypoints in the staging buffer.  Holds no result of an earlier call.
static int path_alloc_inputs(loikb_solver_impl* S, int T)
{
  loikb_solver_impl::PathState& W = S->path;
  const size_t B = (size_t)S->B, nc = (size_t)std::max(S->nc, 1);
  int rc;
  if (!W.d_cursor) {
    if ((rc = alloc_dev(S, (void**)&W.d_ws, sizeof(int) * B)) || (rc = alloc_dev(S, (void**)&W.d_wfrom, sizeof(int) * B)) ||
        (rc = alloc_dev(S, (void**)&W.d_lstatus, sizeof(int) * B)) || (rc = alloc_dev(S, (void**)&W.d_pstatus, sizeof(int) * B)) ||
        (rc = alloc_dev(S, (void**)&W.d_cursor, sizeof(int) * B))) {
      W.d_cursor = nullptr;   // (as pose_alloc: what was allocated goes with the handle; the next call allocates afresh)
      return rc;
    }
  }
  return replace(W.d_wp, sizeof(double) * B * (size_t)T * nc * 12);
}

// WSTEPS and, with record, Q for T waypoints: they hold the results of the last call, so they are regrown only by a call that
// has passed every check
static int path_alloc_results(loikb_solver_impl* S, int T, bool record)
{
  loikb_solver_impl::PathState& W = S->path;
  const size_t B = (size_t)S->B;
  int rc;
  if ((rc = replace(W.d_wsteps, sizeof(int) * B * (size_t)T))) return rc;
  return record ? replace(W.d_Q, sizeof(double) * B * (size_t)T * S->nq) : LOIKB_OK;
}

int loikb_solve_pose_path(loikb_solver* S, const double* q, const double* waypoints, int in_flags, const loikb_pose_params* p,
                          const loikb_path_params* path)
{
  if (!S || !waypoints || !p || !path) return LOIKB_ERR_ARG;
  if (path->n_waypoints < 1 || path->max_steps_per_waypoint < 0 || path->record < 0 || path->record > 1 || path->flags != 0) {
    g_last_error = "solve_pose_path: need n_waypoints >= 1, max_steps_per_waypoint >= 0, record 0 or 1, flags 0";
    return LOIKB_ERR_ARG;
  }
  if (int pre = pose_preconditions(S, p, !q)) return pre;
  if (S->pose.have_step) {
    g_last_error = "solve_pose_path: the handle has step control set (loik_amd_step.h), which this loop does not run -- clear it with loikb_pose_set_step_control(s, NULL) first";
    return LOIKB_ERR_STATE;
  }
  const auto t_call = std::chrono::steady_clock::now();
  HIPCHK(hipSetDevice(S->device));
  const int B = S->B, nc = S->nc_active, T = path->n_waypoints, budget = path->max_steps_per_waypoint;
  const bool dev = in_flags & LOIKB_IN_DEVICE, wp_shared = in_flags & LOIKB_POSE_TARGET_SHARED, record = path->record != 0;
  if ((size_t)(wp_shared ? 1 : B) * T * nc > (size_t)0x7fffffff) { g_last_error = "solve_pose_path: too many waypoints"; return LOIKB_ERR_ARG; }
  int rc;
  if ((rc = pose_alloc(S)) || (rc = path_alloc_inputs(S, T))) return rc;
  loikb_solver_impl::PoseState& P = S->pose;
  loikb_solver_impl::PathState& W = S->path;
  // the waypoints, all of them, checked before anything of the handle changes
  if ((rc = pose_check_targets(S, W.d_wp, waypoints, (size_t)(wp_shared ? 1 : B) * T * nc, dev, P.d_count,
                               "solve_pose_path: a waypoint rotation is not orthonormal with determinant 1 (tolerance 1e-9)")))
    return rc;
  if ((rc = path_alloc_results(S, T, record))) return rc;
  ++S->inputs_epoch;
  if ((rc = pose_begin(S, q, dev))) return rc;
  W.T = T;
  W.recorded = record;
  const size_t nBT = (size_t)B * T, nQ = record ? nBT * S->nq : 0;
  hipLaunchKernelGGL(k_path_setup, grid1(std::max(std::max(nBT, nQ), (size_t)B)), dim3(256), 0, S->stream, B, nBT, nQ, W.d_cursor, W.d_ws,
                     W.d_wfrom, W.d_lstatus, W.d_pstatus, W.d_wsteps, W.d_Q);
  HIPCHK(hipGetLastError());
  PoseBoxScope box{S};
  if ((rc = pose_box_begin(S, box))) return rc;
  const double k = p->gain / p->dt;
  const PoseTask* tasks = P.have_tasks ? (const PoseTask*)P.d_tasks : nullptr;
  const double* A_sh = S->a_shared ? (const double*)P.d_A : nullptr;
  // (the loop-private word: a stalled instance is "stopped" to the integrate and the limit box, and to them alone)
  rc = pose_loop(S, p, box, W.d_lstatus, t_call, [&](int go) -> int {
    with_real(S, [&](auto t) {
      hipLaunchKernelGGL(k_path_retarget<decltype(t)>, grid1(B), dim3(256), 0, S->stream, (const double*)S->d_q, S->nq, S->d_jd, S->d_idx_q,
                         (const int*)P.d_clink, nc, tasks, (const double*)W.d_wp, (int)wp_shared, T, A_sh, (const char*)S->home.tiles, S->L, B,
                         k, p->tol_pose, go, budget, P.d_b, P.d_err, W.d_lstatus, P.d_status, W.d_pstatus, P.d_steps, W.d_cursor, W.d_ws,
                         W.d_wfrom, W.d_wsteps, P.d_count);
    });
    HIPCHK(hipGetLastError());
    if (record) {   // (q is the one the re-target saw: the step's integrate is queued behind)
      hipLaunchKernelGGL(k_path_record, grid1((size_t)B * S->nq), dim3(256), 0, S->stream, (const double*)S->d_q, S->nq, B, T,
                         (const int*)W.d_wfrom, (const int*)W.d_cursor, W.d_Q);
      HIPCHK(hipGetLastError());
    }
    return LOIKB_OK;
  });
  if (rc) return rc;
  memcpy(W.timing, P.timing, sizeof(W.timing));
  return LOIKB_OK;
}

int loikb_path_get(loikb_solver* S, int field, void* out, int out_flags)
{
  if (!S || !out) return LOIKB_ERR_ARG;
  const loikb_solver_impl::PathState& W = S->path;
  if (W.T == 0) { g_last_error = "path_get before solve_pose_path"; return LOIKB_ERR_STATE; }
  HIPCHK(hipSetDevice(S->device));
  const void* src = nullptr;
  size_t bytes = 0;
  const size_t B = (size_t)S->B;
  switch (field) {
  case LOIKB_PATH_F_CURSOR: src = W.d_cursor; bytes = sizeof(int) * B; break;
  case LOIKB_PATH_F_STATUS: src = W.d_pstatus; bytes = sizeof(int) * B; break;
  case LOIKB_PATH_F_WSTEPS: src = W.d_wsteps; bytes = sizeof(int) * B * W.T; break;
  case LOIKB_PATH_F_Q:
    if (!W.recorded) { g_last_error = "path_get: the last solve_pose_path ran with record = 0"; return LOIKB_ERR_STATE; }
    src = W.d_Q; bytes = sizeof(double) * B * W.T * S->nq;
    break;
  case LOIKB_PATH_F_TIMING: return get_timing_out(W.timing, sizeof(W.timing), out, out_flags & LOIKB_OUT_DEVICE);
  default: g_last_error = "path_get: unknown field"; return LOIKB_ERR_ARG;
  }
  return get_copy_out(S, src, bytes, out, out_flags);
}

// ---- include/loik_amd_track.h (kernels in loik_pose_track.hpp) ----------------------------------------------------------------
int loikb_track_version(void) { return LOIKB_TRACK_VERSION; }

// the [B] arrays on first use, and room for the T + 1 samples in the staging buffer.  Holds no result of an earlier call.
static int track_alloc_inputs(loikb_solver_impl* S, int T)
{
  loikb_solver_impl::TrackState& K = S->track;
  const size_t B = (size_t)S->B, nc = (size_t)std::max(S->nc, 1);
  int rc;
  if (!K.d_ontrack) {
    if ((rc = alloc_dev(S, (void**)&K.d_worst, sizeof(double) * B)) || (rc = alloc_dev(S, (void**)&K.d_worst_at, sizeof(int) * B)) ||
        (rc = alloc_dev(S, (void**)&K.d_ontrack, sizeof(int) * B))) {
      K.d_ontrack = nullptr;   // (as pose_alloc: what was allocated goes with the handle; the next call allocates afresh)
      return rc;
    }
  }
  return replace(K.d_smp, sizeof(double) * B * ((size_t)T + 1) * nc * 12);
}

// ERRMAX, INNER and, as `record` says, Q and Z for T steps: they hold the results of the last call, so they are regrown only by a
// call that has passed every check
static int track_alloc_results(loikb_solver_impl* S, int T, int record)
{
  loikb_solver_impl::TrackState& K = S->track;
  const size_t B = (size_t)S->B;
  int rc;
  if ((rc = replace(K.d_errmax, sizeof(double) * B * ((size_t)T + 1))) || (rc = replace(K.d_inner, sizeof(int) * B * (size_t)T))) return rc;
  if ((record & LOIKB_TRACK_REC_Q) && (rc = replace(K.d_Q, sizeof(double) * B * ((size_t)T + 1) * S->nq))) return rc;
  if ((record & LOIKB_TRACK_REC_Z) && (rc = replace(K.d_Z, sizeof(double) * B * (size_t)T * S->nb))) return rc;
  return LOIKB_OK;
}

int loikb_track_pose(loikb_solver* S, const double* q, const double* samples, int in_flags, const loikb_track_params* p)
{
  if (!S || !samples || !p) return LOIKB_ERR_ARG;
  if (p->n_steps < 1 || p->feedforward < LOIKB_TRACK_FF_NONE || p->feedforward > LOIKB_TRACK_FF_DIFFERENCE || p->record < 0 ||
      p->record > (LOIKB_TRACK_REC_Q | LOIKB_TRACK_REC_Z) || p->flags != 0) {
    g_last_error = "track_pose: need n_steps >= 1, feedforward 0 or 1, record 0..3, flags 0";
    return LOIKB_ERR_ARG;
  }
  // the loop's parameters as a pose solve has them: T steps at most, and tol_track where the tolerance is checked
  const loikb_pose_params pose{p->dt, p->gain, p->tol_track, p->n_steps, 0};
  if (int pre = pose_preconditions(S, &pose, !q)) return pre;
  if (S->pose.have_step) {
    g_last_error = "track_pose: the handle has step control set (loik_amd_step.h), which this loop does not run -- clear it with loikb_pose_set_step_control(s, NULL) first";
    return LOIKB_ERR_STATE;
  }
  const auto t_call = std::chrono::steady_clock::now();
  HIPCHK(hipSetDevice(S->device));
  const int B = S->B, nc = S->nc_active, T = p->n_steps, Tn = T + 1, record = p->record, ff = p->feedforward;
  const bool dev = in_flags & LOIKB_IN_DEVICE, smp_shared = in_flags & LOIKB_POSE_TARGET_SHARED;
  if ((size_t)(smp_shared ? 1 : B) * Tn * nc > (size_t)0x7fffffff || (size_t)B * Tn * std::max(S->nq, S->nb) > (size_t)0x7fffffff) {
    g_last_error = "track_pose: too many samples";
    return LOIKB_ERR_ARG;
  }
  int rc;
  if ((rc = pose_alloc(S)) || (rc = track_alloc_inputs(S, T))) return rc;
  loikb_solver_impl::PoseState& P = S->pose;
  loikb_solver_impl::TrackState& K = S->track;
  // the samples, all of them, checked before anything of the handle changes
  if ((rc = pose_check_targets(S, K.d_smp, samples, (size_t)(smp_shared ? 1 : B) * Tn * nc, dev, P.d_count,
                               "track_pose: a sample rotation is not orthonormal with determinant 1 (tolerance 1e-9)")))
    return rc;
  if ((rc = track_alloc_results(S, T, record))) return rc;
  ++S->inputs_epoch;
  if ((rc = pose_begin(S, q, dev))) return rc;
  K.T = T;
  K.record = record;
  double* Q = (record & LOIKB_TRACK_REC_Q) ? K.d_Q : nullptr;
  double* Z = (record & LOIKB_TRACK_REC_Z) ? K.d_Z : nullptr;
  const size_t nE = (size_t)B * Tn, nI = (size_t)B * T, nQ = Q ? nE * S->nq : 0, nZ = Z ? nI * S->nb : 0;
  hipLaunchKernelGGL(k_track_setup, grid1(std::max(std::max(nE, nQ), nZ)), dim3(256), 0, S->stream, B, nE, nI, nQ, nZ, P.d_status, P.d_steps,
                     K.d_ontrack, K.d_errmax, K.d_inner, Q, Z);
  HIPCHK(hipGetLastError());
  PoseBoxScope box{S};
  if ((rc = pose_box_begin(S, box))) return rc;
  const double k = p->gain / p->dt, inv_dt = 1.0 / p->dt;
  const PoseTask* tasks = P.have_tasks ? (const PoseTask*)P.d_tasks : nullptr;
  const double* A_sh = S->a_shared ? (const double*)P.d_A : nullptr;
  int ks = -1;   // the step whose solve ran last: record(ks) stores Q[ks + 1] (before the loop: the starting q), Z[ks], INNER[ks]
  auto record_step = [&]() -> int {
    with_real(S, [&](auto t) {
      hipLaunchKernelGGL(k_track_record<decltype(t)>, grid1((size_t)B * std::max(S->nq, S->nb)), dim3(256), 0, S->stream, (const double*)S->d_q,
                         S->nq, S->nb, B, Tn, ks, (const int*)P.d_status, (const char*)S->home.tiles, S->L,
                         box.active ? (const int*)P.d_lflags : nullptr, Q, Z, K.d_inner);
    });
    HIPCHK(hipGetLastError());
    return LOIKB_OK;
  };
  if ((rc = record_step())) return rc;
  rc = pose_loop(S, &pose, box, P.d_status, t_call,
                 [&](int go) -> int {   // sample ks + 1: the loop re-targets once per step and once more to judge
                   with_real(S, [&](auto t) {
                     hipLaunchKernelGGL(k_track_retarget<decltype(t)>, grid1(B), dim3(256), 0, S->stream, (const double*)S->d_q, S->nq, S->d_jd,
                                        S->d_idx_q, (const int*)P.d_clink, nc, tasks, (const double*)K.d_smp, (int)smp_shared, Tn, ks + 1, ff, A_sh,
                                        (const char*)S->home.tiles, S->L, B, k, inv_dt, p->tol_track, go, P.d_b, P.d_err, P.d_status, P.d_steps,
                                        K.d_errmax, K.d_ontrack, P.d_count);
                   });
                   HIPCHK(hipGetLastError());
                   return LOIKB_OK;
                 },
                 [&]() -> int { ++ks; return record_step(); });
  if (rc) return rc;
  hipLaunchKernelGGL(k_track_finish, grid1(B), dim3(256), 0, S->stream, (const double*)K.d_errmax, B, Tn, K.d_worst, K.d_worst_at);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(S->stream));
  memcpy(K.timing, P.timing, sizeof(K.timing));
  return LOIKB_OK;
}

int loikb_track_get(loikb_solver* S, int field, void* out, int out_flags)
{
  if (!S || !out) return LOIKB_ERR_ARG;
  const loikb_solver_impl::TrackState& K = S->track;
  if (K.T == 0) { g_last_error = "track_get before track_pose"; return LOIKB_ERR_STATE; }
  HIPCHK(hipSetDevice(S->device));
  const void* src = nullptr;
  size_t bytes = 0;
  const size_t B = (size_t)S->B, T = (size_t)K.T;
  switch (field) {
  case LOIKB_TRACK_F_Q:
    if (!(K.record & LOIKB_TRACK_REC_Q)) { g_last_error = "track_get: the last track_pose ran without LOIKB_TRACK_REC_Q"; return LOIKB_ERR_STATE; }
    src = K.d_Q; bytes = sizeof(double) * B * (T + 1) * S->nq;
    break;
  case LOIKB_TRACK_F_Z:
    if (!(K.record & LOIKB_TRACK_REC_Z)) { g_last_error = "track_get: the last track_pose ran without LOIKB_TRACK_REC_Z"; return LOIKB_ERR_STATE; }
    src = K.d_Z; bytes = sizeof(double) * B * T * S->nb;
    break;
  case LOIKB_TRACK_F_ERRMAX: src = K.d_errmax; bytes = sizeof(double) * B * (T + 1); break;
  case LOIKB_TRACK_F_INNER: src = K.d_inner; bytes = sizeof(int) * B * T; break;
  case LOIKB_TRACK_F_ONTRACK: src = K.d_ontrack; bytes = sizeof(int) * B; break;
  case LOIKB_TRACK_F_WORST: src = K.d_worst; bytes = sizeof(double) * B; break;
  case LOIKB_TRACK_F_WORST_AT: src = K.d_worst_at; bytes = sizeof(int) * B; break;
  case LOIKB_TRACK_F_TIMING: return get_timing_out(K.timing, sizeof(K.timing), out, out_flags & LOIKB_OUT_DEVICE);
  default: g_last_error = "track_get: unknown field"; return LOIKB_ERR_ARG;
  }
  return get_copy_out(S, src, bytes, out, out_flags);
}

}  // extern "C"
