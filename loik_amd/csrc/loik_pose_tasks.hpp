// Tool frames and position-only / orientation-only tasks of the batched pose IK (include/loik_amd_tasks.h): what a handle
// with a task specification runs in place of k_pose_retarget, and the frame placements behind loikb_frame_placements.
//
//   k_pose_retarget_tasks : e_c in the task frame oMf_c = oMi_c iMf_c by the constraint's kind, b_c = (gain / dt) S_c e_c, the
//                           reached test on S_c e_c; the bookkeeping of k_pose_retarget, one thread per instance
//   k_frame_placements    : oMf = oMi(link) iMf of requested (link, frame) pairs from the resident q, one thread per
//                           (instance, entry)
//
// The error, the err store, b and the tail are the retarget rule of loik_pose.hpp, which k_pose_retarget runs too: there is one
// definition.  The task kernel needs neither the tiles nor A (pose_b_task), hence no template on the handle's precision.  fp64
// and untuned, as loik_pose.hpp says of its kernels.
#pragma once

#include "loik_pose.hpp"

namespace loikb {

// One step of the pose loop for instance b on a handle with tasks.  The contract of k_pose_retarget with the error, b and the
// reached test of loik_amd_tasks.h: instances already reached or stopped keep their status; the others get err = S_c e_c of the
// resident q, are marked stopped (q or one of the six entries of e not finite) or reached (max_c |S_c e_c|_inf <= tol), and
// otherwise stay running: with `step` set, b_c = k S_c e_c (k = gain / dt) goes to b_out, steps[b] counts the step and
// `running` the instance.  Instances that do not run get b_c = 0.
__global__ void k_pose_retarget_tasks(const double* __restrict__ q, int nq, const JointDesc* __restrict__ jd,
                                      const int* __restrict__ idx_q, const int* __restrict__ c_link, int nc,
                                      const PoseTask* __restrict__ tasks, const double* __restrict__ tgt, int tgt_shared, int B,
                                      double k, double tol, int step, double* __restrict__ b_out, double* __restrict__ err,
                                      int* __restrict__ status, int* __restrict__ steps, unsigned int* __restrict__ running)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int st = status[b];
  bool run = !(st & POSE_IDLE);
  if (run) {
    const double* q_row = q + (size_t)b * nq;
    bool finite = true;
    for (int i = 0; i < nq; ++i) finite = finite && isfinite(q_row[i]);
    double emax = 0.0;
    for (int c = 0; c < nc; ++c) {
      double e[6];
      pose_error(q_row, jd, idx_q, c_link[c], tasks + c, tgt + ((tgt_shared ? 0 : (size_t)b * nc) + c) * 12, e);
      pose_store_err(e, err + ((size_t)b * nc + c) * 6, finite, emax);
      if (step) pose_b_task(e, k, b_out + ((size_t)c * B + b) * 6);
    }
    if (!finite) st |= POSE_STOPPED;
    else if (emax <= tol) st |= POSE_REACHED;
    run = !(st & POSE_IDLE);
    status[b] = st;
  }
  if (step) pose_count_or_idle(run, b, nc, B, b_out, steps, running);
}

// out[b][e] = (R row-major, t) of oMi(dev_link[e]) * frames[e]: k_link_placements' arithmetic, then the composition with iMf
__global__ void k_frame_placements(const double* __restrict__ q, int nq, const JointDesc* __restrict__ jd,
                                   const int* __restrict__ idx_q, const int* __restrict__ dev_link,
                                   const double* __restrict__ frames, int n, int B, double* __restrict__ out)
{
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)B * n) return;
  const int b = (int)(idx / n), e = (int)(idx - (long long)b * n);
  double Ri[9], ti[3], R[9], t[3];
  link_placement(q + (size_t)b * nq, jd, idx_q, dev_link[e], Ri, ti);
  frame_compose(Ri, ti, frames + (size_t)e * 12, frames + (size_t)e * 12 + 9, R, t);
  double* o = out + (size_t)idx * 12;
  for (int k = 0; k < 9; ++k) o[k] = R[k];
  for (int k = 0; k < 3; ++k) o[9 + k] = t[k];
}

}  // namespace loikb
