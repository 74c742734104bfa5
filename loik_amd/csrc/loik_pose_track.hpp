// Timed pose trajectories of the batched pose IK (include/loik_amd_track.h): what loikb_track_pose runs in place of the re-target
// kernels of loikb_solve_pose, and the buffers around it.
//
//   k_track_setup    : the per-call state -- status and steps zero, ERRMAX / Q / Z NaN, INNER / ONTRACK zero
//   k_track_retarget : steps 1 to 5 of the rule of loik_amd_track.h for sample k of instance b: the error against X_k, stopped or
//                      running, ERRMAX and ONTRACK, the feed-forward twist from X_k to X_{k+1} and b_c, one thread per instance.
//                      Both control laws behind pose_b_track: the joint-frame one (A shared, or per instance from the tiles: hence
//                      the template on the handle's precision) and, with `tasks`, the task law
//   k_track_record   : after the step: q into Q[b][k+1], the solve's z into Z[b][k], the INNER bits, one thread per coordinate
//   k_track_finish   : WORST and WORST_AT from ERRMAX, one thread per instance
//
// k_pose_integrate and the limit kernels are reused as they are, on the public pose status: an instance of this loop is running or
// stopped, never reached.  The error, the err store, b and the tail are the retarget rule of loik_pose.hpp, so a call without
// feed-forward is loikb_solve_pose bit for bit.  fp64 and untuned, as loik_pose.hpp says.
#pragma once

#include "loik_pose_path.hpp"

namespace loikb {

// feed-forward modes and record bits (loik_amd_track.h)
enum : int { TRACK_FF_NONE = 0, TRACK_FF_DIFFERENCE = 1 };
enum : int { TRACK_REC_Q = 1, TRACK_REC_Z = 2 };
// INNER bits
enum : int { TRACK_IN_NOT_CONVERGED = 1, TRACK_IN_INFEASIBLE = 2, TRACK_IN_LIMIT = 4, TRACK_IN_ACCEL = 8 };

__device__ __forceinline__ double track_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// status = steps = ontrack = 0, INNER 0, ERRMAX / Q / Z NaN (nQ, nZ = 0 without record).  One grid over the longest of them.
__global__ void k_track_setup(int B, size_t nE, size_t nI, size_t nQ, size_t nZ, int* __restrict__ status, int* __restrict__ steps,
                              int* __restrict__ ontrack, double* __restrict__ errmax, int* __restrict__ inner, double* __restrict__ Q,
                              double* __restrict__ Z)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)B) { status[i] = 0; steps[i] = 0; ontrack[i] = 0; }
  if (i < nE) errmax[i] = track_nan();
  if (i < nI) inner[i] = 0;
  if (i < nQ) Q[i] = track_nan();
  if (i < nZ) Z[i] = track_nan();
}

// rule 4. of loik_amd_track.h: the twist f [linear; angular] that carries the actual frame along with the desired one from X0 to
// X1 (placements [12]) in time 1 / inv_dt, in the frame of the error and masked by `kind` as the error is.  fr: what pose_error
// left of the error against X0.
__device__ __forceinline__ void track_feedforward(int kind, const double* X0, const double* X1, double inv_dt, const PoseErrFrame& fr,
                                                  double* f)
{
  for (int r = 0; r < 6; ++r) f[r] = 0.0;
  if (kind == TASK_POSITION) {   // R^T (t1 - t0) / dt
    for (int r = 0; r < 3; ++r)
      f[r] = inv_dt * (fr.R[r] * (X1[9] - X0[9]) + fr.R[3 + r] * (X1[10] - X0[10]) + fr.R[6 + r] * (X1[11] - X0[11]));
    return;
  }
  if (kind & TASK_FREE_Z) {   // (loik_amd_axis.h) the difference rule again: (w_axis(R^T R1) - w_axis(R^T R0)) / dt, R^T (t1 - t0) / dt
    double w0[3], w1[3], d1[3];
    for (int r = 0; r < 3; ++r) d1[r] = fr.R[r] * X1[2] + fr.R[3 + r] * X1[5] + fr.R[6 + r] * X1[8];
    pose_axis_error(fr.Re[2], fr.Re[5], fr.Re[8], w0);
    pose_axis_error(d1[0], d1[1], d1[2], w1);
    for (int r = 0; r < 2; ++r) f[3 + r] = inv_dt * (w1[r] - w0[r]);
    if (kind == TASK_POSE_AXIS)
      for (int r = 0; r < 3; ++r)
        f[r] = inv_dt * (fr.R[r] * (X1[9] - X0[9]) + fr.R[3 + r] * (X1[10] - X0[10]) + fr.R[6 + r] * (X1[11] - X0[11]));
    return;
  }
  double Rd[9], pd[3], u[6];   // X0^-1 X1 = (R0^T R1, R0^T (t1 - t0))
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Rd[3 * r + c] = X0[r] * X1[c] + X0[3 + r] * X1[3 + c] + X0[6 + r] * X1[6 + c];
    pd[r] = X0[r] * (X1[9] - X0[9]) + X0[3 + r] * (X1[10] - X0[10]) + X0[6 + r] * (X1[11] - X0[11]);
  }
  if (kind == TASK_ORIENTATION) {
    pose_log3(Rd, u + 3);
    mat3_vec(fr.Re, u + 3, f + 3);
    for (int r = 0; r < 3; ++r) f[3 + r] *= inv_dt;
    return;
  }
  pose_log6(Rd, pd, u);
  double rv[3], rw[3];
  mat3_vec(fr.Re, u, rv);
  mat3_vec(fr.Re, u + 3, rw);
  const double* p = fr.pe;
  const double pxw[3] = {p[1] * rw[2] - p[2] * rw[1], p[2] * rw[0] - p[0] * rw[2], p[0] * rw[1] - p[1] * rw[0]};
  for (int r = 0; r < 3; ++r) {
    f[r] = inv_dt * (rv[r] + pxw[r]);
    f[3 + r] = inv_dt * rw[r];
  }
}

// One re-target of the tracking loop for instance b (the numbered rule of loik_amd_track.h), against sample `ks` of its Tn = T + 1
// samples.  smp: [B][Tn][nc][12] or, shared, [Tn][nc][12].  A running instance gets err = e_c of the resident q, is stopped (e or q
// not finite) or gets ERRMAX[b][ks] and its ONTRACK count; with `step` set (ks < Tn - 1) it gets b_c = A_c (k e_c + f_c) (k = gain /
// dt; ff: TRACK_FF_*), steps[b] counts the step and `running` the instance.  Instances that do not run get b_c = 0.
template <typename T>
__global__ void k_track_retarget(const double* __restrict__ q, int nq, const JointDesc* __restrict__ jd, const int* __restrict__ idx_q,
                                 const int* __restrict__ c_link, int nc, const PoseTask* __restrict__ tasks, const double* __restrict__ smp,
                                 int smp_shared, int Tn, int ks, int ff, const double* __restrict__ A_sh, const char* tiles, Layout L, int B,
                                 double k, double inv_dt, double tol, int step, double* __restrict__ b_out, double* __restrict__ err,
                                 int* __restrict__ status, int* __restrict__ steps, double* __restrict__ errmax, int* __restrict__ ontrack,
                                 unsigned int* __restrict__ running)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int st = status[b];
  bool run = !(st & (POSE_REACHED | POSE_STOPPED));
  if (run) {
    const double* q_row = q + (size_t)b * nq;
    bool finite = true;
    for (int i = 0; i < nq; ++i) finite = finite && isfinite(q_row[i]);
    double emax = 0.0;
    for (int c = 0; c < nc; ++c) {
      const double* X = smp + (((smp_shared ? 0 : (size_t)b * Tn) + ks) * nc + c) * 12;
      const PoseTask* tk = tasks ? tasks + c : nullptr;
      double e[6], f[6];
      PoseErrFrame fr;
      pose_error_impl<true>(q_row, jd, idx_q, c_link[c], tk, X, e, &fr);
      pose_store_err(e, err + ((size_t)b * nc + c) * 6, finite, emax);
      if (step) {
        const bool have_f = ff == TRACK_FF_DIFFERENCE;
        if (have_f) track_feedforward(tk ? tk->kind : TASK_POSE, X, X + (size_t)nc * 12, inv_dt, fr, f);
        pose_b_track<T>(e, k, have_f ? f : nullptr, tk != nullptr, A_sh, tiles, L, b, c, b_out + ((size_t)c * B + b) * 6);
      }
    }
    if (!finite) {
      st |= POSE_STOPPED;
    } else {
      errmax[(size_t)b * Tn + ks] = emax;
      if (emax <= tol) ontrack[b] += 1;
    }
    run = !(st & (POSE_REACHED | POSE_STOPPED));
    status[b] = st;
  }
  if (step) pose_count_or_idle(run, b, nc, B, b_out, steps, running);
}

// After step ks (ks = -1: before the first, the starting q): thread (b, i) carries coordinate i of an instance that is not stopped, so
// loads and stores of a wavefront run along the rows.  Q[b][ks + 1][i] = q[b][i] (i < nq, Q != nullptr); Z[b][ks][i] = z of DoF i of the
// step's solve, from the joint records of the tiles as advance_q_instance reads it (i < nv, Z != nullptr); thread i = 0 writes
// INNER[b][ks] from the tiles' status word and, with lflags ([B][nv], nullptr without joint limits), the step's limit flags: bit 4
// from their position bits (1, 2), bit 8 from their acceleration bits (4, 8: loik_amd_accel.h).
template <typename T>
__global__ void k_track_record(const double* __restrict__ q, int nq, int nv, int B, int Tn, int ks, const int* __restrict__ status,
                               const char* tiles, Layout L, const int* __restrict__ lflags, double* __restrict__ Q,
                               double* __restrict__ Z, int* __restrict__ inner)
{
  const int per = nq > nv ? nq : nv;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * per) return;
  const int b = (int)(idx / per), i = (int)(idx - (size_t)b * per);
  if (status[b] & POSE_STOPPED) return;
  if (Q && i < nq) Q[((size_t)b * Tn + ks + 1) * nq + i] = q[(size_t)b * nq + i];
  if (ks < 0) return;
  const char* lp = lane_ptr<T>(const_cast<char*>(tiles), L, b);
  if (Z && i < nv) Z[((size_t)b * (Tn - 1) + ks) * nv + i] = (double)ldp<T>(lp + (size_t)i * JREC * pair_bytes<T>(), JP_WZ).y;
  if (i == 0) {
    const int in = (int)*elem_ptr<T>(const_cast<char*>(lp) + (size_t)L.off_s * pair_bytes<T>(), SP_ST, 0);
    int w = ((in & ST_CONVERGED) ? 0 : TRACK_IN_NOT_CONVERGED) | ((in & ST_PRIMAL_INF) ? TRACK_IN_INFEASIBLE : 0);
    if (lflags)
      for (int j = 0; j < nv; ++j) {
        const int f = lflags[(size_t)b * nv + j];
        if (f & 3) w |= TRACK_IN_LIMIT;
        if (f & 12) w |= TRACK_IN_ACCEL;
      }
    inner[(size_t)b * (Tn - 1) + ks] = w;
  }
}

// WORST[b] = the maximum of ERRMAX[b][1 .. Tn - 1] over its finite entries and WORST_AT[b] the first sample that attains it; NaN and
// -1 when no entry is finite
__global__ void k_track_finish(const double* __restrict__ errmax, int B, int Tn, double* __restrict__ worst, int* __restrict__ worst_at)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double w = track_nan();
  int at = -1;
  for (int t = 1; t < Tn; ++t) {
    const double v = errmax[(size_t)b * Tn + t];
    if (isfinite(v) && (at < 0 || v > w)) { w = v; at = t; }
  }
  worst[b] = w;
  worst_at[b] = at;
}

}  // namespace loikb
