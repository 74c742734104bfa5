// Certified collision checks of joint-space motions and the inverse of the integrator (include/loik_amd_motion.h).
//
//   k_difference            : v with q0 (+) v = q1 under advance_q_joint's arithmetic, one thread per row; a row that is not finite
//                             yields NaN in that row.  With T > 0 the rows are the consecutive samples of q_path [B][T][nq].
//   k_motion_clearance<SLAB>: conservative advancement of segments q(s) = qa (+) s dv.  One wavefront owns a segment and is a
//                             workgroup of its own: the trip count differs from segment to segment, so no wavefront ever waits
//                             for another one (the __syncthreads below order the lanes of the one wavefront; the loop decision
//                             is wave-uniform, and the loop is bounded by max_evals in its own condition).  The advancement itself
//                             is motion_advance, which k_shortcut_paths (loik_pose_shortcut.hpp) calls too:
//                               0. a lane per device joint computes (lin, ang, |p| + tau) of the joint over the segment; a lane
//                                  per sphere walks its root path over those records and keeps Lambda;
//                               per sample, steps 1 to 4 of k_clearance on q(s):
//                               1. a lane per device joint integrates its own coordinates (advance_q_joint) and builds liM;
//                               2. a lane per carrier composes its world placement, a lane per sphere writes its centre;
//                               3. the world pairs (with a grid set the sphere's voxel too: clr_sphere_grid, whose value never
//                                  exceeds the true clearance, so the step below stays valid) and the self pairs, each lane keeping
//                                  its best (clearance, ordinal) and its least (v - margin) / lambda_pair;
//                               4. one wave64 butterfly carries the ordered minimum and delta; every lane decides alike.
//                             The centres [ns][4] are in LDS.  Lambda [ns], liM [nb][12] and the carriers' oMi [ncar][12] sit
//                             beside them when all of it fits 64 KB; SLAB = true takes those three from a handle-owned global
//                             slab per resident wavefront.  Either way the wavefronts stride over the segments.
//
// fp64 whatever the handle's precision, as loik_pose.hpp.
#pragma once

#include "loik_pose_collision.hpp"

namespace loikb {

enum : int { MOTION_FREE = 0, MOTION_BLOCKED = 1, MOTION_UNDECIDED = 2, MOTION_INVALID = 3 };

// doubles beside the centres of one wavefront: Lambda [ns], liM [nb][12], the carriers' oMi [ncar][12] (LDS, or one slab)
__host__ __device__ inline size_t motion_aux_doubles(int nb, int ncar, int ns) { return (size_t)ns + (size_t)12 * nb + (size_t)12 * ncar; }

// row i of a batch of segments: itself, or with T > 0 sample t of path b, i = b (T - 1) + t
__device__ __forceinline__ size_t motion_row(int i, int T) { return T > 0 ? (size_t)i + (size_t)(i / (T - 1)) : (size_t)i; }

// v of one device joint (not JF_NOQ): q0 (+) v = q1
__device__ __forceinline__ void difference_joint(const double* __restrict__ a, const double* __restrict__ b, const JointDesc& d, double* v)
{
  const int rot = d.rot;
  if (rot == ROT_FREE) {   // log6(M0^-1 M1)
    double R0[9], R1[9], R[9], p[3];
    quat_to_rot<double>(a[3], a[4], a[5], a[6], R0);
    quat_to_rot<double>(b[3], b[4], b[5], b[6], R1);
    const double e[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) R[3 * r + c] = R0[r] * R1[c] + R0[3 + r] * R1[3 + c] + R0[6 + r] * R1[6 + c];
      p[r] = R0[r] * e[0] + R0[3 + r] * e[1] + R0[6 + r] * e[2];
    }
    pose_log6(R, p, v);
  } else if (rot == ROT_SPH) {   // log3 of conj(q0) q1
    const double ac[4] = {-a[0], -a[1], -a[2], a[3]};
    double qr[4], R[9];
    quat_mul_xyzw(ac, b, qr);
    quat_to_rot<double>(qr[0], qr[1], qr[2], qr[3], R);
    pose_log3(R, v);
  } else if (rot == ROT_PLANAR) {   // the SE(2) log: w = the relative angle, (vx, vy) = V(w)^-1 R0^T (t1 - t0) with integrate's V
    const double c = a[2] * b[2] + a[3] * b[3], s = a[2] * b[3] - a[3] * b[2];
    const double w = atan2(s, c);
    const double ex = b[0] - a[0], ey = b[1] - a[1];
    const double px = a[2] * ex + a[3] * ey, py = a[2] * ey - a[3] * ex;
    double sw, cw, sh, ch, al, bq;
    if (fabs(w) > 1e-4) { sincos(w, &sw, &cw); sincos(0.5 * w, &sh, &ch); al = sw / w; bq = sh * (sh / (0.5 * w)); }
    else { al = 1.0 - w * w / 6.0; bq = 0.5 * w * (1.0 - w * w / 12.0); }
    const double det = al * al + bq * bq;
    v[0] = (al * px + bq * py) / det;
    v[1] = (al * py - bq * px) / det;
    v[2] = w;
  } else if (d.flags & JF_CS_DIRECT) {   // atan2 of the relative (sin, cos)
    v[0] = atan2(a[0] * b[1] - a[1] * b[0], a[0] * b[0] + a[1] * b[1]);
  } else {
    v[0] = b[0] - a[0];
    if (rot == ROT_TRANS) { v[1] = b[1] - a[1]; v[2] = b[2] - a[2]; }
  }
}

// out [n][nv]; q0, q1 [n][nq], or with T > 0 q0 = q_path [B][T][nq], n = B (T - 1) (q1 is not read).  64 threads a workgroup: the
// compiler keeps pose_log3's dynamically indexed rotation in LDS, 72 bytes a thread of the largest workgroup it must allow for
__global__ void __launch_bounds__(64) k_difference(const double* __restrict__ q0, const double* __restrict__ q1, int nq, const JointDesc* __restrict__ jd,
                             const int* __restrict__ idx_q, int nb, int n, int T, double* __restrict__ out)
{
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const int i = (int)idx;
  const double* a = q0 + motion_row(i, T) * nq;
  const double* b = T > 0 ? a + nq : q1 + (size_t)i * nq;
  double* o = out + (size_t)i * nb;   // (DoF k is device joint k + 1: nv == nb)
  bool fin = true;
  for (int k = 0; k < nq; ++k) fin = fin && isfinite(a[k]) && isfinite(b[k]);
  if (!fin) {
    for (int k = 0; k < nb; ++k) o[k] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  for (int j = 1; j <= nb; ++j) {
    const JointDesc& d = jd[j];
    if (d.flags & JF_NOQ) continue;
    double v[6];
    difference_joint(a + idx_q[j], b + idx_q[j], d, v);
    const int m = joint_nv(d);
#pragma unroll
    for (int k = 0; k < 6; ++k)   // (constant bounds: v stays in registers)
      if (k < m) o[j - 1 + k] = v[k];
  }
}

struct MotionPrm {
  double margin, tol;
  int max_evals;
};

// what the advancement of one segment leaves: every lane of the wavefront holds the same values
struct MotionAdv {
  double s_free, min_sampled, s_at_min;
  unsigned int min_ord;   // the ordinal of min_sampled, CLR_NO_ORDINAL over an empty set of pairs
  int status, evals;
  int min_vox;            // clr_grid_voxel of min_ord at the sample of min_sampled
};

// The advancement of one segment q(s) = q_row (+) s d_row by the 64 lanes of one wavefront that is a workgroup of its own, from the motion
// bound to the status: the body of k_motion_clearance, shared with k_shortcut_paths (loik_pose_shortcut.hpp).  q_row [nq] and d_row
// [nb] are finite and written before the call (the first barrier below orders d_row when the wavefront itself wrote it); cen [ns][4]
// is LDS, lam [ns], xf [nb][12] and cp [ncar][12] LDS or the wavefront's slab.  Every lane takes the same way through every branch
// GRID_CALL: the grid pair behind a call (clr_sphere_grid_call) instead of in line; the values are the same
template <bool GRID_CALL = false>
__device__ __forceinline__ MotionAdv motion_advance(const double* q_row, const double* d_row, const JointDesc* __restrict__ jd,
                                                    const int* __restrict__ idx_q, int nb, const ClrModel& m, const MotionPrm& prm, double* cen,
                                                    double* lam, double* xf, double* cp, int lane)
{
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const ClrOrdinals no(m);
  const unsigned int nps = no.nps, self0 = no.self0();
  const int lp = m.lp, P = 1 << lp, S = 64 >> lp;
  const double block_below = prm.margin + prm.tol;

  // 0. the motion bound: (lin, ang, |p| + tau) of every joint into its liM record, then Lambda of every sphere
  __syncthreads();   // (the last segment's readers of xf and lam are done)
  for (int k = lane; k < nb; k += 64) {
    const JointDesc& d = jd[k + 1];
    double lin = 0.0, ang = 0.0, tau = 0.0;
    if (!(d.flags & JF_NOQ)) {
      const double* q = q_row + idx_q[k + 1];
      const double* e = d_row + k;
      if (d.rot == ROT_FREE) {
        lin = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        ang = sqrt(e[3] * e[3] + e[4] * e[4] + e[5] * e[5]);
        tau = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]) + lin;
      } else if (d.rot == ROT_SPH) {
        ang = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
      } else if (d.rot == ROT_TRANS) {
        const double t0 = q[0] + e[0], t1 = q[1] + e[1], t2 = q[2] + e[2];
        lin = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        tau = fmax(sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), sqrt(t0 * t0 + t1 * t1 + t2 * t2));
      } else if (d.rot == ROT_PLANAR) {
        lin = sqrt(e[0] * e[0] + e[1] * e[1]);
        ang = fabs(e[2]);
        tau = sqrt(q[0] * q[0] + q[1] * q[1]) + lin;
      } else if (d.flags & JF_HELICAL) {
        lin = fabs(d.pitch * e[0]);
        ang = fabs(e[0]);
        tau = fabs(d.pitch) * fmax(fabs(q[0]), fabs(q[0] + e[0]));
      } else if (d.flags & JF_REVOLUTE) {
        ang = fabs(e[0]);
      } else {
        lin = fabs(e[0]);
        tau = fmax(fabs(q[0]), fabs(q[0] + e[0]));
      }
    }
    double* o = xf + (size_t)12 * k;
    o[0] = lin; o[1] = ang;
    o[2] = sqrt(d.tp[0] * d.tp[0] + d.tp[1] * d.tp[1] + d.tp[2] * d.tp[2]) + tau;
  }
  __syncthreads();
  for (int s = lane; s < m.ns; s += 64) {
    const double* c = m.sph + (size_t)4 * s;
    double reach = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), L = 0.0;
    for (int j = m.car[m.scar[s]]; j > 0; j = jd[j].parent) {   // leaf side first: reach = rho of joint j
      const double* r = xf + (size_t)12 * (j - 1);
      L += r[0] + r[1] * reach;
      reach += r[2];
    }
    lam[s] = L;
  }

  double s_cur = 0.0, min_s = inf, s_min = 0.0;
  unsigned int min_ord = CLR_NO_ORDINAL;
  int status = MOTION_UNDECIDED, evals = 0, min_vox = -1;
  for (int k = 0; k < prm.max_evals; ++k) {
    __syncthreads();   // (Lambda is written; the last sample's readers of xf, cp and cen are done)
    // 1. liM of every joint at q(s)
    for (int j = lane; j < nb; j += 64) {
      const JointDesc& d = jd[j + 1];
      double p[8] = {0, 0, 0, 0, 0, 0, 0, 0}, R[9], t[3];
      if (!(d.flags & JF_NOQ)) {
        double qs[7], v[6];
        const int mq = joint_nq(d), mv = joint_nv(d);
        for (int c = 0; c < 7; ++c) qs[c] = c < mq ? q_row[idx_q[j + 1] + c] : 0.0;
        for (int c = 0; c < 6; ++c) v[c] = c < mv ? s_cur * d_row[j + c] : 0.0;
        advance_q_joint(qs, d, v);
        (void)joint_q_pairs(qs, d, p);
      }
      pose_joint_xform(d, p, R, t);
      double* o = xf + (size_t)12 * j;
      for (int c = 0; c < 9; ++c) o[c] = R[c];
      for (int c = 0; c < 3; ++c) o[9 + c] = t[c];
    }
    __syncthreads();
    // 2. oMi of the carriers, the centres
    for (int c = lane; c < m.ncar; c += 64) {
      double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
      for (int j = m.car[c]; j > 0; j = jd[j].parent) {
        const double* x = xf + (size_t)12 * (j - 1);
        xform_premul(x, x + 9, R, t);
      }
      double* o = cp + (size_t)12 * c;
      for (int i = 0; i < 9; ++i) o[i] = R[i];
      for (int i = 0; i < 3; ++i) o[9 + i] = t[i];
    }
    __syncthreads();
    for (int s = lane; s < m.ns; s += 64) clr_centre(cp + (size_t)12 * m.scar[s], m.sph + (size_t)4 * s, cen + (size_t)4 * s);
    __syncthreads();
    // 3. the pairs: the ordered minimum as k_clearance keeps it, and delta
    double best = inf, delta = inf;
    unsigned int bord = CLR_NO_ORDINAL;
    for (int a = lane & (P - 1); a < m.ns; a += P) {
      const double c[4] = {cen[4 * a], cen[4 * a + 1], cen[4 * a + 2], cen[4 * a + 3]};
      const double la = lam[a];
      for (int o = lane >> lp; o < m.nws; o += S) {
        const double* W = m.wsph + (size_t)4 * o;
        const double e0 = c[0] - W[0], e1 = c[1] - W[1], e2 = c[2] - W[2];
        const double v = sqrt(e0 * e0 + e1 * e1 + e2 * e2) - c[3] - W[3];
        const unsigned int ord = (unsigned int)a * (unsigned int)m.nws + (unsigned int)o;
        if (clr_before(v, ord, best, bord)) { best = v; bord = ord; }
        if (la > 0.0) delta = fmin(delta, (v - prm.margin) / la);
      }
      for (int o = lane >> lp; o < m.nwb; o += S) {
        const double v = clr_sphere_box(c, m.wbox + (size_t)15 * o);
        const unsigned int ord = nps + (unsigned int)a * (unsigned int)m.nwb + (unsigned int)o;
        if (clr_before(v, ord, best, bord)) { best = v; bord = ord; }
        if (la > 0.0) delta = fmin(delta, (v - prm.margin) / la);
      }
      if (m.g.G && (lane >> lp) == 0) {
        const double v = (GRID_CALL ? clr_sphere_grid_call(c[0], c[1], c[2], c[3], m.g) : clr_sphere_grid(c[0], c[1], c[2], c[3], m.g)).v;
        const unsigned int ord = no.grid0() + (unsigned int)a;
        if (clr_before(v, ord, best, bord)) { best = v; bord = ord; }
        if (la > 0.0) delta = fmin(delta, (v - prm.margin) / la);
      }
    }
    for (unsigned int i = lane; i < (unsigned int)m.npairs; i += 64) {
      const int a = m.pairs[2 * (size_t)i], b = m.pairs[2 * (size_t)i + 1];
      const double* c = cen + (size_t)4 * a;
      const double* d = cen + (size_t)4 * b;
      const double e0 = c[0] - d[0], e1 = c[1] - d[1], e2 = c[2] - d[2];
      const double v = sqrt(e0 * e0 + e1 * e1 + e2 * e2) - c[3] - d[3];
      const double lab = lam[a] + lam[b];
      if (clr_before(v, self0 + i, best, bord)) { best = v; bord = self0 + i; }
      if (lab > 0.0) delta = fmin(delta, (v - prm.margin) / lab);
    }
    // 4. the butterfly: every lane ends with the same (best, bord, delta)
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(best, off), od = __shfl_xor(delta, off);
      const unsigned int oo = (unsigned int)__shfl_xor((int)bord, off);
      if (clr_before(ov, oo, best, bord)) { best = ov; bord = oo; }
      delta = fmin(delta, od);
    }
    evals = k + 1;
    if (k == 0 || best < min_s) { min_s = best; s_min = s_cur; min_ord = bord; min_vox = clr_grid_voxel(bord, no, m, cen); }
    if (best < block_below) { status = MOTION_BLOCKED; break; }
    if (s_cur == 1.0) { status = MOTION_FREE; break; }
    if (k + 1 == prm.max_evals) break;   // UNDECIDED at this sample
    s_cur = fmin(s_cur + delta, 1.0);
  }
  return MotionAdv{s_cur, min_s, s_min, min_ord, status, evals, min_vox};
}

// out_val [n][3] = (s_free, min_sampled, s_at_min); out_info [n][5] = (status, evals, kind, a, b).  qa rows by motion_row(i, T),
// dv [n][nv].  slab [gridDim.x][motion_aux_doubles]: SLAB only
template <bool SLAB>
__global__ void __launch_bounds__(64)
k_motion_clearance(const double* __restrict__ qa, const double* __restrict__ dv, int nq, const JointDesc* __restrict__ jd,
                   const int* __restrict__ idx_q, int nb, int n, int T, ClrModel m, MotionPrm prm, double* __restrict__ slab,
                   double* __restrict__ out_val, int* __restrict__ out_info)
{
  extern __shared__ __attribute__((aligned(16))) double mot_lds[];
  const int lane = threadIdx.x;
  double* cen = mot_lds;
  double* lam = SLAB ? slab + (size_t)blockIdx.x * motion_aux_doubles(nb, m.ncar, m.ns) : mot_lds + (size_t)4 * m.ns;
  double* xf = lam + m.ns;
  double* cp = xf + (size_t)12 * nb;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const ClrOrdinals no(m);

  for (long long seg = blockIdx.x; seg < n; seg += gridDim.x) {   // (64 bits: seg + gridDim.x may pass 2^31)
    const double* q_row = qa + motion_row((int)seg, T) * nq;
    const double* d_row = dv + (size_t)seg * nb;
    bool fin = true;
    for (int k = lane; k < nq; k += 64) fin &= (bool)isfinite(q_row[k]);
    for (int k = lane; k < nb; k += 64) fin &= (bool)isfinite(d_row[k]);
    if (__ballot(!fin) != 0ull) {   // (wave-uniform)
      if (lane == 0) {
        double* ov = out_val + (size_t)seg * 3;
        int* oi = out_info + (size_t)seg * 5;
        ov[0] = ov[1] = ov[2] = nan;
        oi[0] = MOTION_INVALID; oi[1] = 0; oi[2] = CLR_NONE; oi[3] = -1; oi[4] = -1;
      }
      continue;
    }

    const MotionAdv adv = motion_advance(q_row, d_row, jd, idx_q, nb, m, prm, cen, lam, xf, cp, lane);
    if (lane != 0) continue;
    double* ov = out_val + (size_t)seg * 3;
    int* oi = out_info + (size_t)seg * 5;
    ov[0] = adv.s_free; ov[1] = adv.min_sampled; ov[2] = adv.s_at_min;
    oi[0] = adv.status; oi[1] = adv.evals;
    clr_witness(adv.min_ord, adv.min_vox, no, m, oi + 2);
  }
}

}  // namespace loikb
