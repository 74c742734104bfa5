// Batched pose IK (include/loik_amd_pose.h): the per-step work around the tailored Solve when the library drives
// "take these B seeds to this pose" itself.
//
//   k_link_placements : oMi of requested links from the RESIDENT q (not the tiles' JP_CS pairs, which belong to the q of the
//                       last FwdPassInit), one thread per (instance, link)
//   k_pose_retarget   : e_c = log6(oMi_c^-1 oMdes_c) per active constraint, b_c = A_c (gain / dt) e_c, the reached / stopped
//                       bookkeeping and the count of instances still running, one thread per instance.  Its rule -- the error, the
//                       err store, the two control laws, the tail -- is the `retarget rule` section below, the one definition
//                       that k_pose_retarget_tasks (loik_pose_tasks.hpp), k_path_retarget (loik_pose_path.hpp) and
//                       k_track_retarget (loik_pose_track.hpp) are written over too
//   k_pose_integrate  : q <- q (+) dt z for the running instances only (advance_q_instance: the arithmetic of loikb_integrate)
// and, on a handle with joint position limits (include/loik_amd_limits.h), around the same solve:
//   k_pose_limit_box  : the step's velocity box [lo, hi] = the base box cut to the velocities that keep q (+) dt z in range, into
//                       JP_LBUB of the home tiles, one thread per (instance, DoF)
//   k_pose_limit_clamp: after k_pose_integrate (a kernel of its own: a handle without limits runs the integrate alone), a
//                       limited coordinate that was in range before the step is clamped to its range
//   k_box_copy        : JP_LBUB of every joint of every instance <-> a [nb][B] scratch: a per-instance base box is saved before
//                       the first step and restored after the last
//
// Everything here is fp64 whatever the handle's precision: the configurations are fp64 on the device anyway, and the
// tolerances a pose solve is asked for (1e-6 and below) are out of fp32's reach in a 30-joint chain.  These kernels are a few
// microseconds beside a solve of milliseconds and are not tuned.
#pragma once

#include "loik_device.hpp"

namespace loikb {

// pose status bits (loik_amd_pose.h)
enum : int { POSE_REACHED = 1, POSE_NOT_CONVERGED = 2, POSE_INFEASIBLE = 4, POSE_STOPPED = 8 };
// ... and the bit of loik_amd_step.h (set by k_pose_step_control alone, loik_pose_step.hpp), with the mask of an instance that no
// longer runs in a loikb_solve_pose step: reached, stopped or stalled
enum : int { POSE_STALLED = 16, POSE_IDLE = POSE_REACHED | POSE_STOPPED | POSE_STALLED };

// liMi of device joint i from its coordinates: the fp64 twin of joint_xform (which reads the same numbers from the tiles'
// JP_CS pairs).  p = joint_q_pairs(q of the joint) for a joint that reads q; JF_NOQ joints (the later joints of a free-flyer /
// spherical / translation / planar chain) are their placement alone.
__device__ __forceinline__ void pose_joint_xform(const JointDesc& d, const double* p, double* R, double* t)
{
  if (d.flags & JF_NOQ) {
    make_liMi<double>(d, (d.flags & JF_REVOLUTE) ? 1.0 : 0.0, 0.0, R, t);
    return;
  }
  if (d.rot >= ROT_FREE) {
    double Rq[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tq[3] = {0, 0, 0}, rt[3];
    if (d.rot == ROT_FREE) {
      tq[0] = p[0]; tq[1] = p[1]; tq[2] = p[2];
      quat_to_rot<double>(p[3], p[4], p[5], p[6], Rq);
    } else if (d.rot == ROT_SPH) {
      quat_to_rot<double>(p[0], p[1], p[2], p[3], Rq);
    } else if (d.rot == ROT_PLANAR) {   // (x, y, cos, sin)
      tq[0] = p[0]; tq[1] = p[1];
      Rq[0] = p[2]; Rq[1] = -p[3]; Rq[3] = p[3]; Rq[4] = p[2];
    } else {
      tq[0] = p[0]; tq[1] = p[1]; tq[2] = p[2];
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) R[3 * i + j] = d.Rp[3 * i] * Rq[j] + d.Rp[3 * i + 1] * Rq[3 + j] + d.Rp[3 * i + 2] * Rq[6 + j];
    mat3_vec(d.Rp, tq, rt);
    for (int k = 0; k < 3; ++k) t[k] = d.tp[k] + rt[k];
    return;
  }
  if (d.flags & JF_HELICAL) {   // p = (q, 0): Rot(axis, q), translation pitch q axis
    double s, c, ra[3];
    sincos(p[0], &s, &c);
    make_liMi<double>(d, c, s, R, t);
    mat3_vec(d.Rp, d.axis, ra);
    for (int k = 0; k < 3; ++k) t[k] += (d.pitch * p[0]) * ra[k];
    return;
  }
  make_liMi<double>(d, p[0], p[1], R, t);
}

// oMi of device joint j for one configuration row: the product of liMi along the root path, composed leaf-side first
__device__ __forceinline__ void link_placement(const double* __restrict__ q_row, const JointDesc* __restrict__ jd,
                                               const int* __restrict__ idx_q, int j, double* Ra, double* ta)
{
  for (int k = 0; k < 9; ++k) Ra[k] = (k % 4 == 0) ? 1.0 : 0.0;
  for (int k = 0; k < 3; ++k) ta[k] = 0.0;
  while (j > 0) {
    const JointDesc& d = jd[j];
    double p[8] = {0, 0, 0, 0, 0, 0, 0, 0}, R[9], t[3], Rn[9], tn[3];
    if (!(d.flags & JF_NOQ)) (void)joint_q_pairs(q_row + idx_q[j], d, p);
    pose_joint_xform(d, p, R, t);
    for (int r = 0; r < 3; ++r) {   // (R, t) * (Ra, ta)
      for (int c = 0; c < 3; ++c) Rn[3 * r + c] = R[3 * r] * Ra[c] + R[3 * r + 1] * Ra[3 + c] + R[3 * r + 2] * Ra[6 + c];
      tn[r] = t[r] + R[3 * r] * ta[0] + R[3 * r + 1] * ta[1] + R[3 * r + 2] * ta[2];
    }
    for (int k = 0; k < 9; ++k) Ra[k] = Rn[k];
    for (int k = 0; k < 3; ++k) ta[k] = tn[k];
    j = d.parent;
  }
}

// out[b][e] = (R row-major, t) of device joint dev_link[e] (0: the universe, the identity)
__global__ void k_link_placements(const double* __restrict__ q, int nq, const JointDesc* __restrict__ jd,
                                  const int* __restrict__ idx_q, const int* __restrict__ dev_link, int n, int B,
                                  double* __restrict__ out)
{
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)B * n) return;
  const int b = (int)(idx / n), e = (int)(idx - (long long)b * n);
  double R[9], t[3];
  link_placement(q + (size_t)b * nq, jd, idx_q, dev_link[e], R, t);
  double* o = out + (size_t)idx * 12;
  for (int k = 0; k < 9; ++k) o[k] = R[k];
  for (int k = 0; k < 3; ++k) o[9 + k] = t[k];
}

// log3 (pinocchio::log3): w with exp([w]x) = R, |w| <= pi.  theta = atan2(|vee(R - R^T)| / 2, (tr R - 1) / 2) is accurate on
// the whole range; w = theta / (2 sin theta) vee(R - R^T) with the series of theta / sin theta for theta -> 0, and for
// theta -> pi (where vee(R - R^T) = 2 sin theta a vanishes) the axis from the symmetric part, a a^T = (sym R - cos I) / (1 - cos),
// its sign from vee(R - R^T).  The same branches are restated in tests/pose_numpy.py.
__device__ __forceinline__ void pose_log3(const double* R, double* w)
{
  const double vx = R[7] - R[5], vy = R[2] - R[6], vz = R[3] - R[1];
  const double s = 0.5 * sqrt(vx * vx + vy * vy + vz * vz);
  const double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
  const double theta = atan2(s, c);
  if (c < -0.8) {
    int k = 0;
    if (R[4] > R[3 * k + k]) k = 1;
    if (R[8] > R[3 * k + k]) k = 2;
    const double omc = 1.0 - c;
    double a[3];
    a[k] = sqrt(fmax(0.0, (R[4 * k] - c) / omc));
    for (int j = 0; j < 3; ++j)
      if (j != k) a[j] = 0.5 * (R[3 * k + j] + R[3 * j + k]) / (omc * a[k]);
    const double sg = (a[0] * vx + a[1] * vy + a[2] * vz) < 0.0 ? -theta : theta;
    for (int j = 0; j < 3; ++j) w[j] = sg * a[j];
    return;
  }
  const double t2 = theta * theta;
  const double f = theta < 1e-4 ? 0.5 * (1.0 + t2 / 6.0 + 7.0 * t2 * t2 / 360.0) : 0.5 * theta / s;
  w[0] = f * vx; w[1] = f * vy; w[2] = f * vz;
}

// the axis error of loik_amd_axis.h: the minimal rotation w (frame axes, w_z = 0) that carries the frame's z axis onto
// d = (dx, dy, dz), the desired z axis seen from the frame (the third column of Re).  theta = atan2(s, dz) with s = |(dx, dy)| is
// accurate at both ends and theta / s -> 1, so there is no series branch; s == 0 exactly is parallel (w = 0) or antiparallel
// (w = (pi, 0, 0): any axis in the xy plane would do, x is the rule).  A d that is not finite gives NaN (0 * inf would hide an
// infinite entry otherwise).  The same branches are restated in tests/pose_axis_numpy.py.
__device__ __forceinline__ void pose_axis_error(double dx, double dy, double dz, double* w)
{
  const double s = sqrt(dx * dx + dy * dy);
  w[2] = 0.0;
  if (!(isfinite(s) && isfinite(dz))) {
    w[0] = w[1] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  if (s == 0.0) {
    w[0] = dz < 0.0 ? 3.14159265358979323846 : 0.0;
    w[1] = 0.0;
    return;
  }
  const double f = atan2(s, dz) / s;
  w[0] = -(f * dy);
  w[1] = f * dx;
}

// log6 (pinocchio::log6) of (R, p): [v; w], w = log3(R), v = V^-1(w) p = p - w x p / 2 + beta w x (w x p),
// beta = (1 - (theta / 2) cot(theta / 2)) / theta^2, its series below theta = 1e-3
__device__ __forceinline__ void pose_log6(const double* R, const double* p, double* nu)
{
  double w[3];
  pose_log3(R, w);
  const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const double theta = sqrt(t2);
  double beta;
  if (theta < 1e-3) {
    beta = 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0;
  } else {
    double sh, ch;
    sincos(0.5 * theta, &sh, &ch);
    beta = (1.0 - 0.5 * theta * ch / sh) / t2;
  }
  const double wp[3] = {w[1] * p[2] - w[2] * p[1], w[2] * p[0] - w[0] * p[2], w[0] * p[1] - w[1] * p[0]};
  const double wwp[3] = {w[1] * wp[2] - w[2] * wp[1], w[2] * wp[0] - w[0] * wp[2], w[0] * wp[1] - w[1] * wp[0]};
  for (int k = 0; k < 3; ++k) {
    nu[k] = p[k] - 0.5 * wp[k] + beta * wwp[k];
    nu[3 + k] = w[k];
  }
}

// targets [n][12]: counts the rotations that are not orthonormal with determinant +1 (tolerance `tol` per entry of R^T R - I,
// and of det R - 1) or not finite
__global__ void k_pose_check_targets(const double* __restrict__ tgt, int n, double tol, unsigned int* __restrict__ bad)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* R = tgt + (size_t)i * 12;
  bool ok = true;
  for (int k = 0; k < 12; ++k) ok = ok && isfinite(R[k]);
  for (int a = 0; a < 3 && ok; ++a)
    for (int b = 0; b < 3; ++b) {
      const double g = R[a] * R[b] + R[3 + a] * R[3 + b] + R[6 + a] * R[6 + b] - (a == b ? 1.0 : 0.0);
      ok = ok && fabs(g) <= tol;
    }
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  ok = ok && fabs(det - 1.0) <= tol;
  if (!ok) atomicAdd(bad, 1u);
}

// ---- the retarget rule: what one re-target does for one instance, stated once.  k_pose_retarget, k_pose_retarget_tasks,
// k_path_retarget and k_track_retarget are loops over these functions; a new control law goes here, beside pose_b_joint,
// pose_b_task and pose_b_track.  The library is built with -ffp-contract=on, which contracts within a statement only: a
// statement split or merged here changes bits.

// task kinds (loik_amd_tasks.h) and the free-spin modifier bit with its two kinds (loik_amd_axis.h)
enum : int { TASK_POSE = 0, TASK_POSITION = 1, TASK_ORIENTATION = 2 };
enum : int { TASK_FREE_Z = 4, TASK_POSE_AXIS = TASK_POSE | TASK_FREE_Z, TASK_AXIS = TASK_ORIENTATION | TASK_FREE_Z };

// one entry per active constraint, built by loikb_pose_set_tasks: iMf = (Rf row-major, pf)
struct PoseTask {
  int kind, pad;
  double Rf[9], pf[3];
};

// (Rw, tw) = (R, t) * (Rf, pf); with the identity frame this returns (R, t) bit for bit (finite entries)
__device__ __forceinline__ void frame_compose(const double* R, const double* t, const double* Rf, const double* pf, double* Rw,
                                              double* tw)
{
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Rw[3 * r + c] = R[3 * r] * Rf[c] + R[3 * r + 1] * Rf[3 + c] + R[3 * r + 2] * Rf[6 + c];
    tw[r] = t[r] + (R[3 * r] * pf[0] + R[3 * r + 1] * pf[1] + R[3 * r + 2] * pf[2]);
  }
}

// what pose_error forms on its way to e, for a law that needs more than e (the feed-forward of loik_pose_track.hpp):
// (Re, pe) = oMf^-1 oMdes, the desired frame seen from the actual one, and R = the world rotation of the task (or joint) frame
struct PoseErrFrame {
  double Re[9], pe[3], R[9];
};

// e of the constraint on `link` against the desired placement D [12], in the task frame oMf = oMi iMf and by the task's kind;
// tk = nullptr: the joint frame, the full pose (e = log6(oMi^-1 oMdes)).  FRAME: (Re, pe) and R go to `fr` as well; without it the
// function is, instruction for instruction, what it was before a caller asked for them
template <bool FRAME>
__device__ __forceinline__ void pose_error_impl(const double* q_row, const JointDesc* __restrict__ jd, const int* __restrict__ idx_q, int link,
                                                const PoseTask* tk, const double* D, double* e, PoseErrFrame* fr)
{
  double Ri[9], ti[3], Rw[9], tw[3], Re[9], pe[3];
  link_placement(q_row, jd, idx_q, link, Ri, ti);
  const double *R = Ri, *t = ti;
  if (tk) {
    frame_compose(Ri, ti, tk->Rf, tk->pf, Rw, tw);
    R = Rw; t = tw;
  }
  for (int r = 0; r < 3; ++r) {   // oMf^-1 oMdes = (R^T Rd, R^T (td - t))
    for (int cc = 0; cc < 3; ++cc) Re[3 * r + cc] = R[r] * D[cc] + R[3 + r] * D[3 + cc] + R[6 + r] * D[6 + cc];
    pe[r] = R[r] * (D[9] - t[0]) + R[3 + r] * (D[10] - t[1]) + R[6 + r] * (D[11] - t[2]);
  }
  if constexpr (FRAME) {
    for (int k = 0; k < 9; ++k) { fr->Re[k] = Re[k]; fr->R[k] = R[k]; }
    for (int k = 0; k < 3; ++k) fr->pe[k] = pe[k];
  }
  const int kind = tk ? tk->kind : TASK_POSE;
  if (kind & TASK_FREE_Z) {   // POSE_AXIS: [pe; w_axis(Re)], AXIS: [0; w_axis(Re)]
    pose_axis_error(Re[2], Re[5], Re[8], e + 3);
    for (int r = 0; r < 3; ++r) e[r] = kind == TASK_POSE_AXIS ? pe[r] : 0.0;
  } else if (kind == TASK_POSITION) {
    for (int r = 0; r < 3; ++r) { e[r] = pe[r]; e[3 + r] = 0.0; }
  } else if (kind == TASK_ORIENTATION) {
    pose_log3(Re, e + 3);
    for (int r = 0; r < 3; ++r) e[r] = 0.0;
  } else {
    pose_log6(Re, pe, e);
  }
}

__device__ __forceinline__ void pose_error(const double* q_row, const JointDesc* __restrict__ jd, const int* __restrict__ idx_q, int link,
                                           const PoseTask* tk, const double* D, double* e)
{
  pose_error_impl<false>(q_row, jd, idx_q, link, tk, D, e, nullptr);
}

// e into its err row eo, folded into the instance's `finite` and `emax`
__device__ __forceinline__ void pose_store_err(const double* e, double* __restrict__ eo, bool& finite, double& emax)
{
  for (int r = 0; r < 6; ++r) {
    eo[r] = e[r];
    finite = finite && isfinite(e[r]);
    emax = fmax(emax, fabs(e[r]));
  }
}

// the joint-frame law bo = A_c (k e): A from `A_sh` [nc][36] (shared A), else the per-instance A of constraint c's record in the
// tiles of instance b (hence the template on the handle's precision)
template <typename T>
__device__ __forceinline__ void pose_b_joint(const double* e, double k, const double* __restrict__ A_sh, const char* tiles, const Layout& L,
                                             int b, int c, double* __restrict__ bo)
{
  const char* crec = lane_ptr<T>(const_cast<char*>(tiles), L, b) + (size_t)(L.off_c + c * L.crec) * pair_bytes<T>();
  for (int r = 0; r < 6; ++r) {
    double a = 0.0;
    for (int m = 0; m < 6; ++m) {
      const int x = 6 * r + m;
      const double A = A_sh ? A_sh[c * 36 + x] : (double)*elem_ptr<T>(const_cast<char*>(crec), CP_A + x / 2, x & 1);
      a += A * (k * e[m]);
    }
    bo[r] = a;
  }
}

// the task law bo = k e (loik_amd_tasks.h: A_c v = S_c v_f by construction, so b_c is the masked error itself)
__device__ __forceinline__ void pose_b_task(const double* e, double k, double* __restrict__ bo)
{
  for (int r = 0; r < 6; ++r) bo[r] = k * e[r];
}

// the tracking law (loik_amd_track.h) bo = A_c (k e + f), with `task` bo = k e + f: f [6] = the feed-forward twist in the frame
// of e, masked by the task's kind as e is.  It is the law above applied to u = k e + f with gain 1 (1.0 * u is u); f = nullptr is
// the law above on (e, k) itself, the same statement on the same numbers: no feed-forward keeps the bits of the other loops
template <typename T>
__device__ __forceinline__ void pose_b_track(const double* e, double k, const double* f, bool task, const double* __restrict__ A_sh,
                                             const char* tiles, const Layout& L, int b, int c, double* __restrict__ bo)
{
  double u[6];
  if (f) {
    for (int r = 0; r < 6; ++r) u[r] = k * e[r] + f[r];
    e = u;
    k = 1.0;
  }
  if (task) pose_b_task(e, k, bo);
  else pose_b_joint<T>(e, k, A_sh, tiles, L, b, c, bo);
}

// the tail of a re-target with `step` set: an instance that runs counts the step and itself, one that does not gets b_c = 0
// (its inner solve is idle work: its q does not move)
__device__ __forceinline__ void pose_count_or_idle(bool run, int b, int nc, int B, double* __restrict__ b_out, int* __restrict__ steps,
                                                   unsigned int* __restrict__ running)
{
  if (run) {
    steps[b] += 1;
    atomicAdd(running, 1u);
  } else {
    for (int c = 0; c < nc; ++c)
      for (int r = 0; r < 6; ++r) b_out[((size_t)c * B + b) * 6 + r] = 0.0;
  }
}

// One step of the pose loop for instance b.  Instances already reached or stopped keep their status; the others get
// err = e_c of the resident q, are marked reached (max_c |e_c|_inf <= tol) or stopped (e or q not finite), and otherwise stay
// running: with `step` set, b_c = A_c k e_c (k = gain / dt) goes to b_out, steps[b] counts the step and `running` the instance.
// Instances that do not run get b_c = 0.
template <typename T>
__global__ void k_pose_retarget(const double* __restrict__ q, int nq, const JointDesc* __restrict__ jd, const int* __restrict__ idx_q,
                                const int* __restrict__ c_link, int nc, const double* __restrict__ tgt, int tgt_shared,
                                const double* __restrict__ A_sh, const char* tiles, Layout L, int B, double k, double tol, int step,
                                double* __restrict__ b_out, double* __restrict__ err, int* __restrict__ status,
                                int* __restrict__ steps, unsigned int* __restrict__ running)
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
      pose_error(q_row, jd, idx_q, c_link[c], nullptr, tgt + ((tgt_shared ? 0 : (size_t)b * nc) + c) * 12, e);
      pose_store_err(e, err + ((size_t)b * nc + c) * 6, finite, emax);
      if (step) pose_b_joint<T>(e, k, A_sh, tiles, L, b, c, b_out + ((size_t)c * B + b) * 6);
    }
    if (!finite) st |= POSE_STOPPED;
    else if (emax <= tol) st |= POSE_REACHED;
    run = !(st & POSE_IDLE);
    status[b] = st;
  }
  if (step) pose_count_or_idle(run, b, nc, B, b_out, steps, running);
}

// q <- q (+) dt z for the instances still running, and the inner solve's outcome into their pose status
template <typename T>
__global__ void k_pose_integrate(double* __restrict__ q, int nq, const JointDesc* __restrict__ jd, const int* __restrict__ idx_q,
                                 Layout L, int B, const char* tiles, double dt, int* __restrict__ status)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int st = status[b];
  if (st & (POSE_REACHED | POSE_STOPPED)) return;
  const char* lp = lane_ptr<T>(const_cast<char*>(tiles), L, b);
  const int inner = (int)*elem_ptr<T>(const_cast<char*>(lp) + (size_t)L.off_s * pair_bytes<T>(), SP_ST, 0);
  if (!(inner & ST_CONVERGED)) st |= POSE_NOT_CONVERGED;
  if (inner & ST_PRIMAL_INF) st |= POSE_INFEASIBLE;
  status[b] = st;
  advance_q_instance<T>(q + (size_t)b * nq, jd, idx_q, L.nb, lp, dt);
}

// ---- joint position limits (include/loik_amd_limits.h) ----------------------------------------------------------------------
// One entry per DoF j (device joint j + 1), built by loikb_set_joint_limits: qi = where the DoF's coordinate sits in a row of
// q, or -1 when the DoF has no finite limit (the kernels do no joint-type dispatch: only plain-sum coordinates get here).
struct PoseLimit {
  int qi, pad;
  double lo, hi;
};

// The box of the next inner solve, thread (b, j = blockIdx.y): lanes run over the instances, so the stores into the tiles are
// the 64 side-by-side pairs of one record row.  Base box: `base_sh` (lb[nb], ub[nb] of the uniform buffer) or `base_pi`
// ([nb][B] pairs saved by k_box_copy).  A running instance's limited DoF gets
//   lo = clamp((q_lo - q) / dt, lb, ub), hi = clamp((q_hi - q) / dt, lb, ub)      (fp64; rounded to T by the store)
// its flags (bit 0: lo > lb, bit 1: hi < ub) and `inrange` (the coordinate is inside its range before the step: what
// k_pose_limit_clamp keys off); everything else gets the base box, flags 0 (instances that do not run keep the flags of the
// last step that moved them).
template <typename T>
__global__ void k_pose_limit_box(const double* __restrict__ q, int nq, const PoseLimit* __restrict__ lim, int B, double dt,
                                 const int* __restrict__ status, const T* __restrict__ base_sh, const double2* __restrict__ base_pi,
                                 char* tiles, Layout L, int* __restrict__ flags, unsigned char* __restrict__ inrange)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (b >= B) return;
  double lb, ub;
  if (base_sh) { lb = (double)base_sh[j]; ub = (double)base_sh[L.nb + j]; }
  else { const double2 v = base_pi[(size_t)j * B + b]; lb = v.x; ub = v.y; }
  double lo = lb, hi = ub;
  unsigned char in = 0;
  if (!(status[b] & POSE_IDLE)) {
    const PoseLimit m = lim[j];
    int f = 0;
    if (m.qi >= 0) {
      const double qj = q[(size_t)b * nq + m.qi];
      lo = fmin(fmax((m.lo - qj) / dt, lb), ub);
      hi = fmin(fmax((m.hi - qj) / dt, lb), ub);
      f = (lo > lb ? 1 : 0) | (hi < ub ? 2 : 0);
      in = (m.lo <= qj && qj <= m.hi) ? 1 : 0;
    }
    flags[(size_t)b * L.nb + j] = f;
  }
  inrange[(size_t)j * B + b] = in;
  stp<T>(lane_ptr<T>(tiles, L, b) + (size_t)j * JREC * pair_bytes<T>(), JP_LBUB, (T)lo, (T)hi);
}

// the clamp of one limited coordinate (a NaN stays)
__device__ __forceinline__ double pose_clamp_coord(double v, const PoseLimit& m) { return v < m.lo ? m.lo : (v > m.hi ? m.hi : v); }

// after the step's integrate: q_j <- clamp(q_j, q_lo, q_hi) where `inrange` says so (a NaN stays: the next re-target stops the instance)
__global__ void k_pose_limit_clamp(double* __restrict__ q, int nq, const PoseLimit* __restrict__ lim, int B,
                                   const unsigned char* __restrict__ inrange)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (b >= B || !inrange[(size_t)j * B + b]) return;
  const PoseLimit m = lim[j];
  double* x = q + (size_t)b * nq + m.qi;
  *x = pose_clamp_coord(*x, m);
}

// JP_LBUB of DoF j of instance b -> scratch[j][b] (restore = 0) or back (restore = 1); fp64 holds a T exactly
template <typename T>
__global__ void k_box_copy(char* tiles, Layout L, int B, double2* __restrict__ scratch, int restore)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (b >= B) return;
  char* rec = lane_ptr<T>(tiles, L, b) + (size_t)j * JREC * pair_bytes<T>();
  if (restore) {
    const double2 v = scratch[(size_t)j * B + b];
    stp<T>(rec, JP_LBUB, (T)v.x, (T)v.y);
  } else {
    const typename Vec2<T>::type lu = ldp<T>(rec, JP_LBUB);
    scratch[(size_t)j * B + b] = make_double2((double)lu.x, (double)lu.y);
  }
}

}  // namespace loikb
