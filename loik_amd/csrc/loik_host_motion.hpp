// loik_host_motion.hpp -- the motion layer of the host driver: certified motion checks and difference() (include/loik_amd_motion.h),
// shortcutting (loik_amd_shortcut.h), retiming (loik_amd_retime.h), blending (loik_amd_blend.h) and RRT-Connect planning
// (loik_amd_plan.h).  Included by loik_host.hip right after loik_host_pose.hpp, whose QueryOut, regrow_drained, clr_model and
// check_dof_pairs it uses, and whose collision state (the sphere model, the world, the slab d_mslab) it reads: it is no header of its own.
//
// What the five kernels share is here once: motion_work (where a wavefront's records live, LDS or a slab, and the launch shape that follows)
// with motion_dispatch (the one launch statement of a kernel), the staging of the inputs (motion_inputs, path_inputs, stage_dof_rows) and
// the argument checks (motion_check_paths, motion_check_params, rate_limits_bad, traj_outputs_bad, motion_need_spheres).

// ---- the workspace rule ---------------------------------------------------------------------------------------------------------
// wavefronts that a <true> (slab) instantiation keeps a slab for: the grid of a model whose records do not fit the LDS
constexpr int MOTION_SLAB_WAVES = 512;
// wavefronts of the <false> instantiations that stride over paths: each keeps a path to its end and strides on
constexpr int SHORTCUT_WAVES = 8192;

struct MotionWork {
  bool slab;          // the records of a wavefront are a slab of global memory, not LDS
  size_t lds;         // dynamic LDS bytes of a workgroup
  int waves;          // the grid: one wavefront per workgroup
  size_t slab_bytes;  // of the slab of all wavefronts (slab only)
};

// The rule: `fixed` bytes are LDS always (the centres), `aux` bytes (the records and tables of a wavefront) are LDS when both fit the 64 KB
// beside what the compiler keeps for itself in K_LDS, the <false> instantiation (difference_joint's dynamically indexed rotation, for
// one), else a slab per resident wavefront.  That size is a property of the code object: the runtime is asked once per kernel and process,
// and a failed query is not kept.  n items; the LDS route runs min(n, lds_cap) wavefronts, the slab route min(n, MOTION_SLAB_WAVES),
// either at most `fit`
template <auto K_LDS> static int motion_work(MotionWork* w, size_t fixed, size_t aux, int n, int lds_cap = SHORTCUT_WAVES, size_t fit = SIZE_MAX)
{
  static std::atomic<long long> own{-1};
  if (own.load(std::memory_order_relaxed) < 0) {
    hipFuncAttributes fa;
    HIPCHK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(K_LDS)));
    own.store((long long)fa.sharedSizeBytes, std::memory_order_relaxed);
  }
  w->slab = fixed + aux + (size_t)own.load(std::memory_order_relaxed) > 65536;
  w->lds = fixed + (w->slab ? 0 : aux);
  w->waves = (int)std::min<size_t>((size_t)std::min(n, w->slab ? MOTION_SLAB_WAVES : lds_cap), fit);
  w->slab_bytes = aux * (size_t)w->waves;
  return LOIKB_OK;
}

// The launch: `launch(std::bool_constant<SLAB>, double* d_slab)` holds the kernel's one launch statement; the slab (the motion check's,
// whichever kernel uses it) is grown first on the slab route.  Queued
template <class F> static int motion_dispatch(loikb_solver_impl* S, const MotionWork& w, F&& launch)
{
  if (w.slab) {
    DevBuf<double>& slab = S->pose.col.d_mslab;
    if (int rc = regrow_drained(S, slab, w.slab_bytes)) return rc;
    launch(std::true_type{}, slab.as<double>());
  } else {
    launch(std::false_type{}, (double*)nullptr);
  }
  HIPCHK(hipGetLastError());
  return LOIKB_OK;
}

// ---- staging ----------------------------------------------------------------------------------------------------------------------
// the two input arrays of a call on the device: device pointers pass through, host arrays go side by side into the staging buffer
// (to_device has room for one).  b may be NULL.  Queued
template <class T2> static int motion_inputs(loikb_solver_impl* S, const double* a, size_t abytes, const T2* b, size_t bbytes, bool dev,
                                             const double** da, const T2** db)
{
  if (dev) { *da = a; *db = b; return LOIKB_OK; }
  const size_t off = (abytes + 255) & ~(size_t)255;
  int rc;
  if ((rc = regrow(S->d_stage, off + bbytes))) return rc;
  HIPCHK(hipMemcpyAsync(S->d_stage, a, abytes, hipMemcpyHostToDevice, S->stream));
  if (b) HIPCHK(hipMemcpyAsync(S->d_stage.as<char>() + off, b, bbytes, hipMemcpyHostToDevice, S->stream));
  *da = S->d_stage.as<const double>();
  *db = b ? reinterpret_cast<const T2*>(S->d_stage.as<char>() + off) : nullptr;
  return LOIKB_OK;
}

// ... of the entry points that take paths: q_path [B][T][nq] and len [B] or NULL
static int path_inputs(loikb_solver_impl* S, const double* q_path, const int* len, int B, int T, int in_flags, const double** dq, const int** dlen)
{
  return motion_inputs(S, q_path, sizeof(double) * (size_t)B * T * S->nq, len, sizeof(int) * (size_t)B, in_flags & LOIKB_IN_DEVICE, dq, dlen);
}

// two host rows [nv] side by side at the front of S->d_getscr[1], grown to `bytes` (0: the two rows).  Queued
static int stage_dof_rows(loikb_solver_impl* S, const double* r0, const double* r1, size_t bytes, double** d_rows)
{
  const size_t row = sizeof(double) * (size_t)S->nv;
  if (int rc = regrow(S->d_getscr[1], std::max(bytes, 2 * row))) return rc;
  HIPCHK(hipMemcpyAsync(S->d_getscr[1], r0, row, hipMemcpyHostToDevice, S->stream));
  HIPCHK(hipMemcpyAsync(S->d_getscr[1].as<char>() + row, r1, row, hipMemcpyHostToDevice, S->stream));
  *d_rows = S->d_getscr[1].as<double>();
  return LOIKB_OK;
}

// ---- argument checks ----------------------------------------------------------------------------------------------------------------
// LOIKB_ERR_ARG with "<who>: <bad>" when there is a `bad`
static int motion_arg_error(const char* who, const char* bad)
{
  if (!bad) return LOIKB_OK;
  g_last_error = std::string(who) + ": " + bad;
  return LOIKB_ERR_ARG;
}

// the paths every entry point but the motion check's takes
static int motion_check_paths(const char* who, const double* q_path, int B, int T)
{
  return motion_arg_error(who, T < 2 ? "need T >= 2"
                                     : (B < 0 || (size_t)B * (size_t)T > (size_t)0x7fffffff || (B > 0 && !q_path)) ? "need B >= 0, B * T < 2^31 and q_path when B > 0"
                                     : nullptr);
}

// the members every params struct of the layer begins its checks with: margin, tol, max_evals, flags
template <class P> static int motion_check_params(const P* p, const char* who)
{
  return motion_arg_error(who, !p ? "p == NULL"
                                   : !std::isfinite(p->margin) ? "the margin is not finite"
                                   : !(std::isfinite(p->tol) && p->tol >= 1e-9) ? "tol is not finite and >= 1e-9"
                                   : (p->max_evals < 1 || p->max_evals > 65536) ? "max_evals is outside 1 .. 65536"
                                   : p->flags != 0 ? "flags != 0" : nullptr);
}

// what retime_paths and blend_paths check first: the pointers, then the rate limits per DoF
static const char* rate_limits_bad(const loikb_solver_impl* S, const double* v_max, const double* a_max, const void* p, const double* out_duration,
                                   const int* out_info)
{
  const char* bad = !v_max ? "v_max == NULL" : !a_max ? "a_max == NULL" : !p ? "p == NULL" : !out_duration ? "need out_duration"
                    : !out_info ? "need out_info" : nullptr;
  for (int j = 0; !bad && j < S->nv; ++j) {
    if (!(std::isfinite(v_max[j]) && v_max[j] > 0.0)) bad = "a v_max that is not finite and > 0";
    else if (!(std::isfinite(a_max[j]) && a_max[j] > 0.0)) bad = "an a_max that is not finite and > 0";
  }
  return bad;
}

// ... and last: the sampled trajectory, S = n_rows rows per path
static const char* traj_outputs_bad(const double* q_path, int B, int n_rows, const double* out_traj, const double* out_vel)
{
  return (out_vel && !out_traj) ? "out_vel without out_traj"
         : (out_traj && n_rows < 1) ? "out_traj with S < 1"
         : (out_traj && (size_t)B * (size_t)n_rows > (size_t)0x7fffffff) ? "need B * S < 2^31"
         : (out_traj && out_traj == q_path) ? "out_traj == q_path" : nullptr;
}

// the state every certified entry point needs
static int motion_need_spheres(const loikb_solver_impl* S, const char* who)
{
  if (S->pose.col.ns != 0) return LOIKB_OK;
  g_last_error = std::string(who) + ": no spheres set (loikb_collision_set_spheres)";
  return LOIKB_ERR_STATE;
}

// bytes of the centres of the sphere model, LDS in every kernel that reads the model
static size_t centre_bytes(const Collision& C) { return sizeof(double) * 4 * (size_t)C.ns; }

extern "C" {

// ---- include/loik_amd_motion.h (kernels in loik_pose_motion.hpp) ---------------------------------------------------------------
int loikb_motion_version(void) { return LOIKB_MOTION_VERSION; }

int loikb_difference(loikb_solver* S, const double* q0, const double* q1, int n, int in_flags, double* out_v, int out_flags)
{
  if (!S) return LOIKB_ERR_ARG;
  if (n < 0 || (n > 0 && (!q0 || !q1 || !out_v))) { g_last_error = "difference: need n >= 0 and q0, q1, out_v when n > 0"; return LOIKB_ERR_ARG; }
  if (n == 0) return LOIKB_OK;
  HIPCHK(hipSetDevice(S->device));
  const size_t qbytes = sizeof(double) * (size_t)n * S->nq;
  QueryOut o(S, out_flags);
  const double *d0, *d1;
  double* d_v;
  o.add(out_v, sizeof(double) * (size_t)n * S->nv, &d_v);
  int rc;
  if ((rc = motion_inputs(S, q0, qbytes, q1, qbytes, in_flags & LOIKB_IN_DEVICE, &d0, &d1)) || (rc = o.reserve())) return rc;
  hipLaunchKernelGGL(k_difference, grid1((size_t)n, 64), dim3(64), 0, S->stream, d0, d1, S->nq, S->d_jd, S->d_idx_q, S->nb, n, 0, d_v);
  HIPCHK(hipGetLastError());
  return o.finish();   // (the caller's arrays have been read)
}

// One advancement launch over n segments: qa rows by motion_row(i, T) of dqa, dv [n][nv].  The LDS route runs one workgroup per
// segment.  Queued
static int motion_launch(loikb_solver_impl* S, const double* dqa, const double* ddv, int n, int T, const loikb_motion_params& p, double* d_val,
                         int* d_info)
{
  const Collision& C = S->pose.col;
  MotionWork w;
  if (int rc = motion_work<&k_motion_clearance<false>>(&w, centre_bytes(C), sizeof(double) * motion_aux_doubles(S->nb, (int)C.car.size(), C.ns), n, n)) return rc;
  const ClrModel m = clr_model(S);
  const MotionPrm prm{p.margin, p.tol, p.max_evals};
  return motion_dispatch(S, w, [&](auto slab, double* d_slab) {
    hipLaunchKernelGGL(k_motion_clearance<decltype(slab)::value>, dim3(w.waves), dim3(64), w.lds, S->stream, dqa, ddv, S->nq, S->d_jd, S->d_idx_q,
                       S->nb, n, T, m, prm, d_slab, d_val, d_info);
  });
}

// the shared body of the two checks: dqa as motion_launch takes it, ddv [n][nv] or nullptr = the differences of the path (T > 0).
// Queued; the caller finishes `o`
static int motion_run(loikb_solver_impl* S, const double* dqa, const double* ddv, int n, int T, const loikb_motion_params& p, double* out_val,
                      int* out_info, QueryOut& o)
{
  int rc;
  if (!ddv) {
    if ((rc = regrow(S->d_getscr[1], sizeof(double) * (size_t)n * S->nv))) return rc;
    hipLaunchKernelGGL(k_difference, grid1((size_t)n, 64), dim3(64), 0, S->stream, dqa, (const double*)nullptr, S->nq, S->d_jd, S->d_idx_q, S->nb, n, T,
                       S->d_getscr[1].as<double>());
    HIPCHK(hipGetLastError());
    ddv = S->d_getscr[1].as<const double>();
  }
  double* d_val;
  int* d_info;
  o.add(out_val, sizeof(double) * 3 * (size_t)n, &d_val);
  o.add(out_info, sizeof(int) * 5 * (size_t)n, &d_info);
  if ((rc = o.reserve())) return rc;
  return motion_launch(S, dqa, ddv, n, T, p, d_val, d_info);
}

int loikb_motion_clearance(loikb_solver* S, const double* qa, const double* dv, int n, int in_flags, const loikb_motion_params* p, double* out_val,
                           int* out_info, int out_flags)
{
  if (!S) return LOIKB_ERR_ARG;
  if (n < 0 || (n > 0 && (!qa || !dv || !out_val || !out_info))) { g_last_error = "motion_clearance: need n >= 0 and qa, dv, out_val, out_info when n > 0"; return LOIKB_ERR_ARG; }
  int rc;
  if ((rc = motion_check_params(p, "motion_clearance")) || (rc = motion_need_spheres(S, "motion_clearance"))) return rc;
  if (n == 0) return LOIKB_OK;
  HIPCHK(hipSetDevice(S->device));
  QueryOut o(S, out_flags);
  const double *dqa, *ddv;
  if ((rc = motion_inputs(S, qa, sizeof(double) * (size_t)n * S->nq, dv, sizeof(double) * (size_t)n * S->nv, in_flags & LOIKB_IN_DEVICE, &dqa, &ddv)) ||
      (rc = motion_run(S, dqa, ddv, n, 0, *p, out_val, out_info, o)))
    return rc;
  return o.finish();   // (the caller's arrays have been read)
}

int loikb_motion_clearance_path(loikb_solver* S, const double* q_path, int B, int T, int in_flags, const loikb_motion_params* p, double* out_val,
                                int* out_info, int out_flags)
{
  if (!S) return LOIKB_ERR_ARG;
  if (T < 2) { g_last_error = "motion_clearance_path: need T >= 2"; return LOIKB_ERR_ARG; }
  if (B < 0 || (size_t)B * (size_t)(T - 1) > (size_t)0x7fffffff || (B > 0 && (!q_path || !out_val || !out_info))) {
    g_last_error = "motion_clearance_path: need B >= 0, fewer than 2^31 segments and q_path, out_val, out_info when B > 0";
    return LOIKB_ERR_ARG;
  }
  int rc;
  if ((rc = motion_check_params(p, "motion_clearance_path")) || (rc = motion_need_spheres(S, "motion_clearance_path"))) return rc;
  if (B == 0) return LOIKB_OK;
  HIPCHK(hipSetDevice(S->device));
  QueryOut o(S, out_flags);
  const double *dq, *none;
  if ((rc = motion_inputs(S, q_path, sizeof(double) * (size_t)B * T * S->nq, (const double*)nullptr, 0, in_flags & LOIKB_IN_DEVICE, &dq, &none)) ||
      (rc = motion_run(S, dq, nullptr, B * (T - 1), T, *p, out_val, out_info, o)))
    return rc;
  return o.finish();
}

// ---- include/loik_amd_shortcut.h (kernels in loik_pose_shortcut.hpp) -----------------------------------------------------------
int loikb_shortcut_version(void) { return LOIKB_SHORTCUT_VERSION; }

int loikb_shortcut_paths(loikb_solver* S, const double* q_path, const int* len, int B, int T, int in_flags, const loikb_shortcut_params* p,
                         double* out_path, int* out_keep, int* out_info, double* out_val, int out_flags)
{
  if (!S) return LOIKB_ERR_ARG;
  int rc;
  if ((rc = motion_check_paths("shortcut_paths", q_path, B, T))) return rc;
  if (!out_path || !out_info) { g_last_error = "shortcut_paths: need out_path and out_info"; return LOIKB_ERR_ARG; }
  if ((rc = motion_check_params(p, "shortcut_paths"))) return rc;
  if (p->rounds < 0 || p->rounds > 1048576) { g_last_error = "shortcut_paths: rounds is outside 0 .. 1048576"; return LOIKB_ERR_ARG; }
  if (out_path == q_path) { g_last_error = "shortcut_paths: out_path == q_path"; return LOIKB_ERR_ARG; }
  if ((rc = motion_need_spheres(S, "shortcut_paths"))) return rc;
  if (B == 0) return LOIKB_OK;
  HIPCHK(hipSetDevice(S->device));
  QueryOut o(S, out_flags);
  const Collision& C = S->pose.col;
  MotionWork w;
  const double* dq;
  const int* dlen;
  double *d_path, *d_val;
  int *d_info, *d_keep;
  if ((rc = path_inputs(S, q_path, len, B, T, in_flags, &dq, &dlen)) ||
      (rc = motion_work<&k_shortcut_paths<false>>(&w, centre_bytes(C), sizeof(double) * shortcut_aux_doubles(S->nb, (int)C.car.size(), C.ns), B)))
    return rc;
  o.add(out_path, sizeof(double) * (size_t)B * T * S->nq, &d_path);
  o.add(out_val, sizeof(double) * 2 * (size_t)B, &d_val);
  o.add(out_info, sizeof(int) * 6 * (size_t)B, &d_info);
  o.add(out_keep, sizeof(int) * (size_t)B * T, &d_keep);
  // every wavefront has a keep row in the scratch when the caller wants none
  if ((rc = o.reserve()) || (!out_keep && (rc = regrow(S->d_getscr[1], sizeof(int) * (size_t)w.waves * T)))) return rc;
  int* d_kscr = out_keep ? nullptr : S->d_getscr[1].as<int>();
  const ClrModel m = clr_model(S);
  const ShortcutPrm prm{p->margin, p->tol, p->max_evals, p->rounds, p->seed};
  rc = motion_dispatch(S, w, [&](auto slab, double* d_slab) {
    hipLaunchKernelGGL(k_shortcut_paths<decltype(slab)::value>, dim3(w.waves), dim3(64), w.lds, S->stream, dq, dlen, B, T, S->nq, S->d_jd, S->d_idx_q,
                       S->nb, m, prm, d_slab, d_kscr, d_path, d_keep, d_info, d_val);
  });
  return rc ? rc : o.finish();   // (the caller's arrays have been read)
}

int loikb_path_length(loikb_solver* S, const double* q_path, const int* len, int B, int T, int in_flags, double* out_length, int out_flags)
{
  if (!S) return LOIKB_ERR_ARG;
  int rc;
  if ((rc = motion_check_paths("path_length", q_path, B, T))) return rc;
  if (!out_length) { g_last_error = "path_length: need out_length"; return LOIKB_ERR_ARG; }
  if (B == 0) return LOIKB_OK;
  HIPCHK(hipSetDevice(S->device));
  QueryOut o(S, out_flags);
  const double* dq;
  const int* dlen;
  double* d_len;
  o.add(out_length, sizeof(double) * (size_t)B, &d_len);
  if ((rc = path_inputs(S, q_path, len, B, T, in_flags, &dq, &dlen)) || (rc = o.reserve())) return rc;
  hipLaunchKernelGGL(k_path_length, dim3(std::min(B, SHORTCUT_WAVES)), dim3(64), 0, S->stream, dq, dlen, B, T, S->nq, S->d_jd, S->d_idx_q, S->nb, d_len);
  HIPCHK(hipGetLastError());
  return o.finish();   // (the caller's arrays have been read)
}

// ---- include/loik_amd_retime.h (kernel in loik_pose_retime.hpp) -----------------------------------------------------------------
int loikb_retime_version(void) { return LOIKB_RETIME_VERSION; }

// The two limit rows go into S->d_getscr[1]; the tables of a wavefront are all there is to place (no model, no centres)
int loikb_retime_paths(loikb_solver* S, const double* q_path, const int* len, int B, int T, int in_flags, const double* v_max,
                       const double* a_max, const loikb_retime_params* p, int n_rows, double* out_traj, double* out_vel, double* out_seg,
                       double* out_duration, int* out_info, int out_flags)
{
  if (!S) return LOIKB_ERR_ARG;
  int rc;
  if ((rc = motion_check_paths("retime_paths", q_path, B, T))) return rc;
  const char* bad = rate_limits_bad(S, v_max, a_max, p, out_duration, out_info);
  if (!bad)
    bad = !(std::isfinite(p->dt) && p->dt > 0.0) ? "dt is not finite and > 0"
          : (p->flags & ~LOIKB_RETIME_SNAP) ? "unknown flags"
          : traj_outputs_bad(q_path, B, n_rows, out_traj, out_vel);
  if ((rc = motion_arg_error("retime_paths", bad))) return rc;
  if (B == 0) return LOIKB_OK;
  HIPCHK(hipSetDevice(S->device));
  QueryOut o(S, out_flags);
  MotionWork w;
  const double* dq;
  const int* dlen;
  double *d_traj, *d_vel, *d_seg, *d_dur, *d_lim;
  int* d_info;
  if ((rc = path_inputs(S, q_path, len, B, T, in_flags, &dq, &dlen)) ||
      (rc = motion_work<&k_retime_paths<false>>(&w, 0, sizeof(double) * retime_tab_doubles(T, S->nb), B)))
    return rc;
  if (!out_traj) n_rows = 0;
  o.add(out_traj, sizeof(double) * (size_t)B * n_rows * S->nq, &d_traj);
  o.add(out_vel, sizeof(double) * (size_t)B * n_rows * S->nv, &d_vel);
  o.add(out_seg, sizeof(double) * (size_t)B * (T - 1) * 4, &d_seg);
  o.add(out_duration, sizeof(double) * (size_t)B, &d_dur);
  o.add(out_info, sizeof(int) * 4 * (size_t)B, &d_info);
  if ((rc = o.reserve()) || (rc = stage_dof_rows(S, v_max, a_max, 0, &d_lim))) return rc;
  const RetimePrm prm{p->dt, (p->flags & LOIKB_RETIME_SNAP) != 0, n_rows};
  rc = motion_dispatch(S, w, [&](auto slab, double* d_slab) {
    hipLaunchKernelGGL(k_retime_paths<decltype(slab)::value>, dim3(w.waves), dim3(64), w.lds, S->stream, dq, dlen, B, T, S->nq, S->d_jd, S->d_idx_q,
                       S->nb, (const double*)d_lim, prm, d_slab, d_traj, d_vel, d_seg, d_dur, d_info);
  });
  return rc ? rc : o.finish();   // (the caller's arrays have been read)
}

// ---- include/loik_amd_blend.h (kernel in loik_pose_blend.hpp) -------------------------------------------------------------------
int loikb_blend_version(void) { return LOIKB_BLEND_VERSION; }

// The two limit rows go into S->d_getscr[1], as retime_paths puts them; the records and the tables of a wavefront are placed beside the centres
int loikb_blend_paths(loikb_solver* S, const double* q_path, const int* len, int B, int T, int in_flags, const double* v_max, const double* a_max,
                      const loikb_blend_params* p, int n_rows, double* out_traj, double* out_vel, double* out_duration, int* out_info,
                      double* out_corner, int* out_corner_info, double* out_piece, int out_flags)
{
  if (!S) return LOIKB_ERR_ARG;
  int rc;
  if ((rc = motion_check_paths("blend_paths", q_path, B, T))) return rc;
  if (T >= (1 << 30)) { g_last_error = "blend_paths: need T < 2^30"; return LOIKB_ERR_ARG; }   // (2 T - 3 pieces are counted in ints)
  if ((rc = motion_arg_error("blend_paths", rate_limits_bad(S, v_max, a_max, p, out_duration, out_info))) ||
      (rc = motion_check_params(p, "blend_paths")))
    return rc;
  const char* bad = !(std::isfinite(p->reach) && p->reach > 0.0) ? "reach is not finite and > 0"
                    : !(std::isfinite(p->dt) && p->dt > 0.0) ? "dt is not finite and > 0"
                    : (p->max_tries < 0 || p->max_tries > 16) ? "max_tries is outside 0 .. 16"
                    : traj_outputs_bad(q_path, B, n_rows, out_traj, out_vel);
  if ((rc = motion_arg_error("blend_paths", bad)) || (rc = motion_need_spheres(S, "blend_paths"))) return rc;
  if (B == 0) return LOIKB_OK;
  HIPCHK(hipSetDevice(S->device));
  QueryOut o(S, out_flags);
  const Collision& C = S->pose.col;
  MotionWork w;
  const double* dq;
  const int* dlen;
  double *d_traj, *d_vel, *d_dur, *d_corner, *d_piece, *d_lim;
  int *d_info, *d_cinfo;
  if ((rc = path_inputs(S, q_path, len, B, T, in_flags, &dq, &dlen)) ||
      (rc = motion_work<&k_blend_paths<false>>(&w, centre_bytes(C), sizeof(double) * blend_aux_doubles(S->nb, (int)C.car.size(), C.ns, T), B)))
    return rc;
  if (!out_traj) n_rows = 0;
  o.add(out_traj, sizeof(double) * (size_t)B * n_rows * S->nq, &d_traj);
  o.add(out_vel, sizeof(double) * (size_t)B * n_rows * S->nv, &d_vel);
  o.add(out_duration, sizeof(double) * (size_t)B, &d_dur);
  o.add(out_corner, sizeof(double) * (size_t)B * (T - 2) * 5, &d_corner);
  o.add(out_piece, sizeof(double) * (size_t)B * (2 * (size_t)T - 3) * 4, &d_piece);
  o.add(out_info, sizeof(int) * 4 * (size_t)B, &d_info);
  o.add(out_corner_info, sizeof(int) * (size_t)B * (T - 2) * 6, &d_cinfo);
  if ((rc = o.reserve()) || (rc = stage_dof_rows(S, v_max, a_max, 0, &d_lim))) return rc;
  const ClrModel m = clr_model(S);
  const BlendPrm prm{p->margin, p->tol, p->reach, p->dt, p->max_evals, p->max_tries, n_rows};
  rc = motion_dispatch(S, w, [&](auto slab, double* d_slab) {
    hipLaunchKernelGGL(k_blend_paths<decltype(slab)::value>, dim3(w.waves), dim3(64), w.lds, S->stream, dq, dlen, B, T, S->nq, S->d_jd, S->d_idx_q,
                       S->nb, m, (const double*)d_lim, prm, d_slab, d_traj, d_vel, d_dur, d_info, d_corner, d_cinfo, d_piece);
  });
  return rc ? rc : o.finish();   // (the caller's arrays have been read)
}

// ---- include/loik_amd_plan.h (kernel in loik_pose_plan.hpp) ---------------------------------------------------------------------
int loikb_plan_version(void) { return LOIKB_PLAN_VERSION; }

// S->d_getscr[1] holds the two range rows, then the trees of every resident wavefront, then coord [nv] (the coordinate of a sampled DoF,
// else -1) and the wavefronts' parents and path nodes.  The records of a wavefront are placed as the shortcutting's, and no more
// wavefronts run than LOIKB_PLAN_SCRATCH_BYTES has trees for
int loikb_plan_paths(loikb_solver* S, const double* q_start, const double* q_goal, int B, int in_flags, const double* s_lo, const double* s_hi,
                     const loikb_plan_params* p, int T, double* out_path, int* out_info, double* out_length, int out_flags)
{
  if (!S) return LOIKB_ERR_ARG;
  int rc;
  if (T < 2) { g_last_error = "plan_paths: need T >= 2"; return LOIKB_ERR_ARG; }
  if (B < 0 || (size_t)B * (size_t)T > (size_t)0x7fffffff || (B > 0 && (!q_start || !q_goal))) {
    g_last_error = "plan_paths: need B >= 0, B * T < 2^31 and q_start, q_goal when B > 0";
    return LOIKB_ERR_ARG;
  }
  if (B > 0 && (!out_path || !out_info)) { g_last_error = "plan_paths: need out_path and out_info"; return LOIKB_ERR_ARG; }
  if ((rc = motion_check_params(p, "plan_paths"))) return rc;
  const char* bad = !(std::isfinite(p->step) && p->step > 0.0) ? "step is not finite and > 0"
                    : (p->max_iters < 0 || p->max_iters > 1048576) ? "max_iters is outside 0 .. 1048576"
                    : (p->max_nodes < 2 || p->max_nodes > 65536) ? "max_nodes is outside 2 .. 65536" : nullptr;
  if ((rc = motion_arg_error("plan_paths", bad))) return rc;
  if (!s_lo || !s_hi) { g_last_error = "plan_paths: need s_lo and s_hi"; return LOIKB_ERR_ARG; }
  const int nv = S->nv;
  if ((rc = check_dof_pairs(S, "plan_paths", "s_lo", "s_hi", s_lo, s_hi, nv))) return rc;
  std::vector<int> coord(nv, -1);
  int sampled = 0;
  for (int j = 0; j < nv; ++j)
    if (std::isfinite(s_lo[j]) && std::isfinite(s_hi[j])) { coord[j] = S->lim_q[j]; ++sampled; }
  if (sampled == 0) { g_last_error = "plan_paths: no DoF to sample (s_lo and s_hi need a finite pair)"; return LOIKB_ERR_ARG; }
  if (out_path && (out_path == q_start || out_path == q_goal)) { g_last_error = "plan_paths: out_path == q_start or q_goal"; return LOIKB_ERR_ARG; }
  if ((rc = motion_need_spheres(S, "plan_paths"))) return rc;
  if (B == 0) return LOIKB_OK;
  HIPCHK(hipSetDevice(S->device));
  QueryOut o(S, out_flags);
  const Collision& C = S->pose.col;
  const size_t qbytes = sizeof(double) * (size_t)B * S->nq;
  const size_t wd = plan_scr_doubles(p->max_nodes, S->nq), wi = plan_scr_ints(p->max_nodes, T);
  const size_t fit = std::max<size_t>(1, (size_t)LOIKB_PLAN_SCRATCH_BYTES / (wd * sizeof(double) + wi * sizeof(int)));
  MotionWork w;
  const double *dqs, *dqg;
  double *d_path, *d_len, *d_lo;
  int* d_info;
  if ((rc = motion_inputs(S, q_start, qbytes, q_goal, qbytes, in_flags & LOIKB_IN_DEVICE, &dqs, &dqg)) ||
      (rc = motion_work<&k_plan_paths<false>>(&w, centre_bytes(C), sizeof(double) * shortcut_aux_doubles(S->nb, (int)C.car.size(), C.ns), B, SHORTCUT_WAVES, fit)))
    return rc;
  o.add(out_path, sizeof(double) * (size_t)B * T * S->nq, &d_path);
  o.add(out_length, sizeof(double) * (size_t)B, &d_len);
  o.add(out_info, sizeof(int) * 8 * (size_t)B, &d_info);
  const size_t dbytes = sizeof(double) * ((size_t)2 * nv + wd * (size_t)w.waves);
  if ((rc = o.reserve()) || (rc = stage_dof_rows(S, s_lo, s_hi, dbytes + sizeof(int) * ((size_t)nv + wi * (size_t)w.waves), &d_lo))) return rc;
  int* d_coord = (int*)(S->d_getscr[1].as<char>() + dbytes);
  HIPCHK(hipMemcpyAsync(d_coord, coord.data(), sizeof(int) * nv, hipMemcpyHostToDevice, S->stream));
  const ClrModel m = clr_model(S);
  const PlanPrm prm{p->margin, p->tol, p->step, p->max_evals, p->max_iters, p->max_nodes, p->seed};
  rc = motion_dispatch(S, w, [&](auto slab, double* d_slab) {
    hipLaunchKernelGGL(k_plan_paths<decltype(slab)::value>, dim3(w.waves), dim3(64), w.lds, S->stream, dqs, dqg, B, T, S->nq, S->d_jd, S->d_idx_q, S->nb,
                       m, prm, (const double*)d_lo, (const double*)(d_lo + nv), (const int*)d_coord, d_slab, d_lo + 2 * nv, d_coord + nv, d_path,
                       d_info, d_len);
  });
  return rc ? rc : o.finish();   // (the caller's arrays and coord have been read)
}

}  // extern "C"
