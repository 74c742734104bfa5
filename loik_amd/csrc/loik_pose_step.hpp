// Backtracking step control and stall detection of the batched pose IK (include/loik_amd_step.h): what a loikb_solve_pose step
// launches in place of the k_pose_integrate + k_pose_limit_clamp pair when step control is set on the handle.
//
//   k_pose_step_control : for a running instance, the inner solve's outcome into its status (as k_pose_integrate folds it), then
//                         the trials q_m = q (+) (alpha_m dt) z, m = 0..M, each clamped to the joint ranges as the step's clamp
//                         does it and judged by the merit Phi = sum_c |e_c|^2 of the loop's own error; the accepted trial (or
//                         the plain step, or the stall verdict) and the per-instance counters.  One thread per instance
//
// The error of a trial is pose_error of the retarget rule (loik_pose.hpp), the integrate is advance_q_instance, the clamp is
// pose_clamp_coord: nothing of them is restated here, so trial 0 is the plain loop's q bit for bit.  fp64 whatever the handle's
// precision; the template parameter only says how z is read from the tiles.  The library is built with -ffp-contract=on, which
// contracts within a statement only: the merit's squares and the acceptance bound are split into statements so that no fused
// multiply-add forms (the rule of loik_amd_step.h, which tests/pose_step_numpy.py restates in numpy).  Untuned, as loik_pose.hpp
// says of its kernels: M + 1 forward kinematics per running instance beside a solve of milliseconds.
#pragma once

#include "loik_pose.hpp"

namespace loikb {

// loikb_step_params as the kernel takes it
struct StepCtl {
  double shrink, sufficient;
  int max_backtracks, patience;
};

// Phi of one configuration row against the instance's targets tg [nc][12]; false when an entry of the row or of its errors is
// not finite
__device__ __forceinline__ bool step_merit(const double* q_row, int nq, const JointDesc* __restrict__ jd, const int* __restrict__ idx_q,
                                           const int* __restrict__ c_link, int nc, const PoseTask* tasks, const double* tg, double& phi)
{
  bool finite = true;
  for (int i = 0; i < nq; ++i) finite = finite && isfinite(q_row[i]);
  phi = 0.0;
  for (int c = 0; c < nc; ++c) {
    double e[6];
    pose_error(q_row, jd, idx_q, c_link[c], tasks ? tasks + c : nullptr, tg + (size_t)c * 12, e);
    for (int r = 0; r < 6; ++r) {
      finite = finite && isfinite(e[r]);
      const double sq = e[r] * e[r];
      phi += sq;
    }
  }
  return finite;
}

// row <- row (+) step z of instance b (z from its joint records lp), then the step's clamp when the handle has joint limits
template <typename T>
__device__ __forceinline__ void step_move(double* row, const JointDesc* __restrict__ jd, const int* __restrict__ idx_q, int nb, const char* lp,
                                          double step, const PoseLimit* __restrict__ lim, const unsigned char* __restrict__ inrange, int B, int b)
{
  advance_q_instance<T>(row, jd, idx_q, nb, lp, step);
  if (!lim) return;
  for (int j = 0; j < nb; ++j)
    if (inrange[(size_t)j * B + b]) {
      const PoseLimit m = lim[j];
      row[m.qi] = pose_clamp_coord(row[m.qi], m);
    }
}

// The step of loik_amd_step.h for instance b.  err: the rows this step's re-target stored (Phi0); tgt / tgt_shared / tasks: what
// that re-target ran with; lim / inrange: nullptr on a handle without joint position limits, else the table and what the step's
// k_pose_limit_box left; trial [B][nq]: one scratch row per instance; frun [B]: the run of failed searches.
template <typename T>
__global__ void k_pose_step_control(double* __restrict__ q, int nq, const JointDesc* __restrict__ jd, const int* __restrict__ idx_q, Layout L,
                                    int B, const char* tiles, double dt, const int* __restrict__ c_link, int nc,
                                    const PoseTask* __restrict__ tasks, const double* __restrict__ tgt, int tgt_shared,
                                    const double* __restrict__ err, const PoseLimit* __restrict__ lim,
                                    const unsigned char* __restrict__ inrange, StepCtl ctl, double* __restrict__ trial,
                                    int* __restrict__ status, int* __restrict__ steps, double* __restrict__ alpha,
                                    int* __restrict__ backtracks, int* __restrict__ failed, int* __restrict__ frun)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int st = status[b];
  if (st & POSE_IDLE) return;
  const char* lp = lane_ptr<T>(const_cast<char*>(tiles), L, b);
  const int inner = (int)*elem_ptr<T>(const_cast<char*>(lp) + (size_t)L.off_s * pair_bytes<T>(), SP_ST, 0);
  if (!(inner & ST_CONVERGED)) st |= POSE_NOT_CONVERGED;
  if (inner & ST_PRIMAL_INF) st |= POSE_INFEASIBLE;
  double* q_row = q + (size_t)b * nq;
  double* t_row = trial + (size_t)b * nq;
  const double* tg = tgt + (tgt_shared ? 0 : (size_t)b * nc) * 12;
  double phi0 = 0.0;
  for (int c = 0; c < nc; ++c)
    for (int r = 0; r < 6; ++r) {
      const double e = err[((size_t)b * nc + c) * 6 + r];
      const double sq = e * e;
      phi0 += sq;
    }
  double a = 1.0;
  int accepted = -1;
  for (int m = 0; m <= ctl.max_backtracks; ++m) {
    for (int i = 0; i < nq; ++i) t_row[i] = q_row[i];
    const double adt = a * dt;
    step_move<T>(t_row, jd, idx_q, L.nb, lp, adt, lim, inrange, B, b);
    double phi;
    const bool finite = step_merit(t_row, nq, jd, idx_q, c_link, nc, tasks, tg, phi);
    const double sa = ctl.sufficient * a;
    const double bound = (1.0 - sa) * phi0;
    if (finite && phi <= bound) { accepted = m; break; }
    a *= ctl.shrink;
  }
  if (accepted >= 0) {
    for (int i = 0; i < nq; ++i) q_row[i] = t_row[i];
    alpha[b] = a;
    backtracks[b] += accepted;
    frun[b] = 0;
  } else {
    const int run = frun[b] + 1;
    failed[b] += 1;
    frun[b] = run;
    if (ctl.patience > 0 && run >= ctl.patience) {   // stalled: q stays, the step the re-target counted is taken back
      st |= POSE_STALLED;
      steps[b] -= 1;
    } else {   // the plain step (trial 0 again, from the same numbers)
      step_move<T>(q_row, jd, idx_q, L.nb, lp, dt, lim, inrange, B, b);
      alpha[b] = 1.0;
    }
  }
  status[b] = st;
}

}  // namespace loikb
