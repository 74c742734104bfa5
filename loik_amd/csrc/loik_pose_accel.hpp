// Joint acceleration limits of the batched pose IK (include/loik_amd_accel.h): what a pose loop launches in place of
// k_pose_limit_box when the handle has acceleration limits, and the per-instance velocity state around it.
//
//   k_pose_dyn_box   : the step's velocity box [lo, hi] by the rule of loik_amd_accel.h -- the acceleration window around the
//                      velocity of the previous step, and the position limits as the velocity the joint can still brake from --
//                      into JP_LBUB of the home tiles, one thread per (instance, DoF).  Grid, lane mapping and stores are
//                      k_pose_limit_box's
//   k_accel_keep_z   : behind the step's solve: the z of the running instances from the home tiles into the [nb][B] velocity
//                      state, 0 for the others
//   k_accel_load_v0  : before the first step: the start velocity [B][nv] (or 0) into the velocity state
//   k_accel_get_v    : the velocity state as [B][nv] for loikb_accel_get_velocity, 0 for instances that reached or stopped
//
// k_pose_limit_box, k_pose_integrate and k_pose_limit_clamp are what they were: a handle without acceleration limits launches
// none of the kernels here.  fp64 and untuned, as loik_pose.hpp says: these are a few loads and stores per (instance, DoF), lanes
// over the instances so that the velocity state, `inrange` and the tiles are read and written side by side.
#pragma once

#include "loik_pose.hpp"

namespace loikb {

// limit flag bits beside LOIKB_LIMIT_LOWER / LOIKB_LIMIT_UPPER (loik_amd_accel.h)
enum : int { LIMIT_POS_LOWER = 1, LIMIT_POS_UPPER = 2, LIMIT_ACCEL_LOWER = 4, LIMIT_ACCEL_UPPER = 8 };

// vmax(d) of loik_amd_accel.h: the largest velocity from which q <- q + dt z still stops within distance d when |z| drops by s
// per step.  Braking from z travels dt (z + (z - s) + (z - 2 s) + ...), convex and piecewise linear in z with breakpoints at
// z = n s; on the piece n the inverse is (d / dt + s n (n + 1) / 2) / (n + 1).  n = the estimate from the square root, then
// corrected in integers (a step or two: the estimate is off by rounding only).  d < 0, d or s infinite, dt s below the normal
// range: d / dt, the rule of loik_amd_limits.h.  An estimate of 2^31 and beyond is used as it is (its piece lies above vmax by a
// relative 2^-31 at most; every n gives an upper bound).
__device__ __forceinline__ double accel_vmax(double d, double dt, double s)
{
  const double ds = dt * s;
  if (!(d >= 0.0) || isinf(d) || isinf(s) || !(ds >= 2.2250738585072014e-308)) return d / dt;
  double n = floor((sqrt(1.0 + 8.0 * (d / ds)) - 1.0) / 2.0);
  n = fmin(n, 4503599627370496.0);
  if (n < 2147483648.0) {
    while (n > 0.0 && ds * n * (n + 1.0) / 2.0 > d) n -= 1.0;
    while (ds * (n + 1.0) * (n + 2.0) / 2.0 <= d) n += 1.0;
  }
  return (d / dt + s * n * (n + 1.0) / 2.0) / (n + 1.0);
}

// The box of the next inner solve, thread (b, j = blockIdx.y) as in k_pose_limit_box.  lim: the position-limit table or nullptr
// (no position limits on the handle); a_max [nb] (+inf: none); zp [nb][B]: the velocity applied in the previous step.  A running
// instance gets, in fp64 and then rounded to T by the store,
//   U = vmax(q_hi - q) (+inf without an upper limit), Lw = -vmax(q - q_lo) (-inf without a lower one), s = a_max dt
//   hi = min(max(U, zp - s), zp + s), lo = min(max(Lw, zp - s), zp + s), lo = min(lo, hi), both then clamped to the base box
// its four flag bits and `inrange` (what k_pose_limit_clamp keys off); the others get the base box and keep their flags.
template <typename T>
__global__ void k_pose_dyn_box(const double* __restrict__ q, int nq, const PoseLimit* __restrict__ lim, const double* __restrict__ a_max,
                               const double* __restrict__ zp, int B, double dt, const int* __restrict__ status,
                               const T* __restrict__ base_sh, const double2* __restrict__ base_pi, char* tiles, Layout L,
                               int* __restrict__ flags, unsigned char* __restrict__ inrange)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (b >= B) return;
  double lb, ub;
  if (base_sh) { lb = (double)base_sh[j]; ub = (double)base_sh[L.nb + j]; }
  else { const double2 v = base_pi[(size_t)j * B + b]; lb = v.x; ub = v.y; }
  double lo = lb, hi = ub;
  unsigned char in = 0;
  if (!(status[b] & (POSE_REACHED | POSE_STOPPED))) {
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const double s = a_max[j] * dt, v = zp[(size_t)j * B + b];
    double U = inf, Lw = -inf;
    if (lim && lim[j].qi >= 0) {
      const PoseLimit m = lim[j];
      const double qj = q[(size_t)b * nq + m.qi];
      U = accel_vmax(m.hi - qj, dt, s);
      Lw = -accel_vmax(qj - m.lo, dt, s);
      in = (m.lo <= qj && qj <= m.hi) ? 1 : 0;
    }
    const double wlo = v - s, whi = v + s;
    hi = fmin(fmax(U, wlo), whi);
    lo = fmin(fmin(fmax(Lw, wlo), whi), hi);
    const int f = ((Lw > lb && Lw >= wlo) ? LIMIT_POS_LOWER : 0) | ((U < ub && U <= whi) ? LIMIT_POS_UPPER : 0) |
                  ((wlo > lb && wlo > Lw) ? LIMIT_ACCEL_LOWER : 0) | ((whi < ub && whi < U) ? LIMIT_ACCEL_UPPER : 0);
    lo = fmin(fmax(lo, lb), ub);
    hi = fmin(fmax(hi, lb), ub);
    flags[(size_t)b * L.nb + j] = f;
  }
  inrange[(size_t)j * B + b] = in;
  stp<T>(lane_ptr<T>(tiles, L, b) + (size_t)j * JREC * pair_bytes<T>(), JP_LBUB, (T)lo, (T)hi);
}

// zp[j][b] = the z of DoF j that the step's integrate applies to instance b (from the joint records of the home tiles, as
// advance_q_instance reads it), 0 for an instance that does not run
template <typename T>
__global__ void k_accel_keep_z(const char* tiles, Layout L, int B, const int* __restrict__ status, double* __restrict__ zp)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (b >= B) return;
  double v = 0.0;
  if (!(status[b] & (POSE_REACHED | POSE_STOPPED)))
    v = (double)ldp<T>(lane_ptr<T>(const_cast<char*>(tiles), L, b) + (size_t)j * JREC * pair_bytes<T>(), JP_WZ).y;
  zp[(size_t)j * B + b] = v;
}

// zp[j][b] = v0[b][j] (v0 = nullptr: 0)
__global__ void k_accel_load_v0(const double* __restrict__ v0, int B, int nv, double* __restrict__ zp)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (b >= B) return;
  zp[(size_t)j * B + b] = v0 ? v0[(size_t)b * nv + j] : 0.0;
}

// out[b][j] = zp[j][b], 0 for an instance whose loop status says reached or stopped (status = nullptr: no step ran, all 0)
__global__ void k_accel_get_v(const double* __restrict__ zp, const int* __restrict__ status, int B, int nv, double* __restrict__ out)
{
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * nv) return;
  const int b = (int)(idx / nv), j = (int)(idx - (size_t)b * nv);
  out[idx] = (!status || (status[b] & (POSE_REACHED | POSE_STOPPED))) ? 0.0 : zp[(size_t)j * B + b];
}

}  // namespace loikb
