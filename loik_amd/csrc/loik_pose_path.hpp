// Waypoint paths of the batched pose IK (include/loik_amd_path.h): what loikb_solve_pose_path runs in place of the re-target
// kernels of loikb_solve_pose, and the buffers around it.
//
//   k_path_setup    : the per-call state -- cursor, count, the two status words, WSTEPS zero, the Q rows NaN
//   k_path_retarget : the rule of loik_amd_path.h for instance b: the error against waypoint `cursor`, stopped / crossed (and the
//                     next waypoint at once) / stalled / running with b_c, one thread per instance.  Both control laws: the
//                     joint-frame law of k_pose_retarget (A shared, or per instance from the tiles: hence the template on the
//                     handle's precision) and, with `tasks`, the task law of k_pose_retarget_tasks
//   k_path_record   : q of instance b into the Q rows of the waypoints the last re-target crossed, one thread per coordinate
//
// k_pose_integrate and the limit kernels are reused as they are: they take "does this instance run" from a status word with the
// POSE_* bits, and the path loop hands them its own, LOOP-PRIVATE word, in which a stalled instance carries
// POSE_STOPPED | PATH_L_STALLED -- so it is not integrated, gets the base box and keeps its limit flags, exactly like an instance
// that stopped.  The re-target folds the private word into the public pose status (stalled: neither REACHED nor STOPPED) and the
// path status every time it handles the instance.
//
// The error, the err store and b are the retarget rule of loik_pose.hpp, the one definition the two pose kernels run too, so a
// path of one waypoint is loikb_solve_pose bit for bit.  fp64 and untuned, as loik_pose.hpp says.
#pragma once

#include "loik_pose_tasks.hpp"

namespace loikb {

// path status bits (loik_amd_path.h) and the private bit of the loop's status word
enum : int { PATH_COMPLETE = 1, PATH_STALLED = 2 };
enum : int { PATH_L_STALLED = 16 };

// cursor = count = wfrom = 0, status words 0, WSTEPS 0, Q NaN (nQ = 0 without record).  One grid over the longest of the three.
__global__ void k_path_setup(int B, size_t nBT, size_t nQ, int* __restrict__ cursor, int* __restrict__ ws, int* __restrict__ wfrom,
                             int* __restrict__ lstatus, int* __restrict__ pstatus, int* __restrict__ wsteps, double* __restrict__ Q)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)B) { cursor[i] = 0; ws[i] = 0; wfrom[i] = 0; lstatus[i] = 0; pstatus[i] = 0; }
  if (i < nBT) wsteps[i] = 0;
  if (i < nQ) Q[i] = __longlong_as_double(0x7ff8000000000000ll);
}

// One re-target of the path loop for instance b (the numbered rule of loik_amd_path.h).  wp: [B][Tn][nc][12] or, shared,
// [Tn][nc][12].  lstatus: the loop-private word (above); status / pstatus: the public pose and path status, rewritten from it.
// wfrom[b] = the cursor this re-target found, so that k_path_record stores the rows [wfrom, cursor).  `budget`: steps per
// waypoint, 0 = none.  With `step` a running instance gets b_c, steps / ws / WSTEPS[cursor] count one and `running` counts it;
// every other instance gets b_c = 0.
template <typename T>
__global__ void k_path_retarget(const double* __restrict__ q, int nq, const JointDesc* __restrict__ jd, const int* __restrict__ idx_q,
                                const int* __restrict__ c_link, int nc, const PoseTask* __restrict__ tasks, const double* __restrict__ wp,
                                int wp_shared, int Tn, const double* __restrict__ A_sh, const char* tiles, Layout L, int B, double k,
                                double tol, int step, int budget, double* __restrict__ b_out, double* __restrict__ err,
                                int* __restrict__ lstatus, int* __restrict__ status, int* __restrict__ pstatus, int* __restrict__ steps,
                                int* __restrict__ cursor, int* __restrict__ ws, int* __restrict__ wfrom, int* __restrict__ wsteps,
                                unsigned int* __restrict__ running)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int ls = lstatus[b];
  int w = cursor[b];
  wfrom[b] = w;
  bool run = !(ls & (POSE_REACHED | POSE_STOPPED));
  if (run) {
    const double* q_row = q + (size_t)b * nq;
    bool q_finite = true;
    for (int i = 0; i < nq; ++i) q_finite = q_finite && isfinite(q_row[i]);
    int s = ws[b];
    for (;;) {
      bool finite = q_finite;
      double emax = 0.0;
      for (int c = 0; c < nc; ++c) {
        double e[6];
        pose_error(q_row, jd, idx_q, c_link[c], tasks ? tasks + c : nullptr, wp + (((wp_shared ? 0 : (size_t)b * Tn) + w) * nc + c) * 12, e);
        pose_store_err(e, err + ((size_t)b * nc + c) * 6, finite, emax);
        if (step) {
          double* bo = b_out + ((size_t)c * B + b) * 6;
          if (tasks) pose_b_task(e, k, bo);
          else pose_b_joint<T>(e, k, A_sh, tiles, L, b, c, bo);
        }
      }
      if (!finite) { ls |= POSE_STOPPED; break; }
      if (emax <= tol) {   // waypoint w reached: its count is final, the next one is examined at once
        wsteps[(size_t)b * Tn + w] = s;
        ++w;
        s = 0;
        if (w == Tn) { ls |= POSE_REACHED; break; }
        continue;
      }
      if (budget > 0 && s == budget) ls |= POSE_STOPPED | PATH_L_STALLED;
      break;
    }
    run = !(ls & (POSE_REACHED | POSE_STOPPED));
    if (run && step) ++s;
    cursor[b] = w;
    ws[b] = s;
    if (w < Tn) wsteps[(size_t)b * Tn + w] = s;
    lstatus[b] = ls;
    status[b] = (ls & PATH_L_STALLED) ? (ls & ~(POSE_STOPPED | PATH_L_STALLED)) : ls;
    pstatus[b] = ((ls & POSE_REACHED) ? PATH_COMPLETE : 0) | ((ls & PATH_L_STALLED) ? PATH_STALLED : 0);
  }
  if (step) pose_count_or_idle(run, b, nc, B, b_out, steps, running);
}

// Q[b][w] = q[b] for the waypoints w in [wfrom[b], cursor[b]) the last re-target crossed: thread (b, i) carries coordinate i, so
// loads and stores of a wavefront run along the rows (nq contiguous doubles each)
__global__ void k_path_record(const double* __restrict__ q, int nq, int B, int Tn, const int* __restrict__ wfrom,
                              const int* __restrict__ cursor, double* __restrict__ Q)
{
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * nq) return;
  const int b = (int)(idx / nq), i = (int)(idx - (size_t)b * nq);
  const int w0 = wfrom[b], w1 = cursor[b];
  if (w0 >= w1) return;
  const double v = q[idx];
  for (int w = w0; w < w1; ++w) Q[((size_t)b * Tn + w) * nq + i] = v;
}

}  // namespace loikb
