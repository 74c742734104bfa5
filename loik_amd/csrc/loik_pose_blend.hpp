// Certified parabolic blends: retiming of joint-space paths through their corners (include/loik_amd_blend.h).
//
//   k_blend_paths<SLAB>: one wavefront is one workgroup and owns one path from its first corner to its last sample, then strides to the
//                        next path, as k_retime_paths does and for its reason.  No communication between wavefronts and no spin-wait;
//                        every loop is bounded by T, S, nq, nb, max_tries or max_evals in its own condition, and every decision -- the
//                        status of a corner, the try taken, the lowering of a rate -- is wave-uniform.
//                          1. per segment, a lane per segment in chunks of 64: dv_k with difference_joint, its norm, A_k and V_k;
//                          2. per corner, the wavefront together: ZERO_LEG and COUPLED (a lane per device joint, one ballot), then the
//                             tries, each P0 and P2 into two [nb] rows and blend_advance on the curve; of a try that is FREE the rate
//                             limit, a lane per DoF and one butterfly of maxima;
//                          3. the forward and the backward pass over the rates, every lane the same arithmetic on the same table;
//                          4. per piece, a lane per piece in chunks of 64: the profile of a leg or the duration of a blend, the starts
//                             summed in path order over __shfl as k_retime_paths sums its segments;
//                          5. per sample, a lane per sample in chunks of 64: the lane bisects the starts, evaluates its piece and walks
//                             the device joints with advance_q_joint.
//                        blend_advance is motion_advance (loik_pose_motion.hpp) with the curve in place of the segment: the bound of
//                        the header from the two control segments, q(u) = q_k (+) w(u) per sample, and from there the same pairs, the
//                        same order and the same four rules.
//                        The centres [ns][4] are in LDS.  Lambda, liM, the carriers' oMi, P0 and P2, and the tables of the path -- the
//                        segments [T - 1][3], the corners [T - 2][5], the pieces [2 T - 3][8] and dv [T - 1][nb] -- sit beside them when
//                        all of it fits 64 KB; SLAB = true takes them from the global slab of the wavefront.
//
// fp64 whatever the handle's precision, as loik_pose.hpp.
#pragma once

#include "loik_pose_retime.hpp"

namespace loikb {

enum : int { BLEND_TAKEN = 0, BLEND_BLOCKED = 1, BLEND_UNDECIDED = 2, BLEND_COUPLED = 3, BLEND_ZERO_LEG = 4, BLEND_OFF = 5 };

// doubles of one wavefront's path tables: segments [T - 1][3], corners [T - 2][5], pieces [2 T - 3][8], dv [T - 1][nb]
__host__ __device__ inline size_t blend_tab_doubles(int T, int nb)
{
  return (size_t)3 * (T - 1) + (size_t)5 * (T - 2) + (size_t)8 * (2 * (size_t)T - 3) + (size_t)(T - 1) * (size_t)nb;
}
// doubles beside the centres of one wavefront: the records of k_motion_clearance, P0 and P2, the path tables
__host__ __device__ inline size_t blend_aux_doubles(int nb, int ncar, int ns, int T)
{
  return motion_aux_doubles(nb, ncar, ns) + (size_t)2 * nb + blend_tab_doubles(T, nb);
}

struct BlendPrm {
  double margin, tol, reach, dt;
  int max_evals, max_tries;
  int S;   // rows of out_traj (ignored when out_traj is nullptr)
};

// (lin, ang, tau) of device joint d (not JF_NOQ) over the segment (q, e): the table of include/loik_amd_motion.h.  motion_advance
// (loik_pose_motion.hpp) has the same table inline in its step 0 and stays as it is: the two must be kept in step
__device__ __forceinline__ void blend_travel(const JointDesc& d, const double* q, const double* e, double& lin, double& ang, double& tau)
{
  lin = 0.0; ang = 0.0; tau = 0.0;
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

// The advancement of one blend q(u) = q_row (+) ((1 - u)^2 p0 + u^2 p2) by the 64 lanes of one wavefront that is a workgroup of its own.
// q_row [nq], p0 and p2 [nb] are finite and written before the call (the first barrier below orders p0 and p2); cen [ns][4] is LDS, lam
// [ns], xf [nb][12] and cp [ncar][12] LDS or the wavefront's slab.  Every lane takes the same way through every branch and returns the
// same values; s_free and s_at_min of the result are values of u
__device__ __forceinline__ MotionAdv blend_advance(const double* q_row, const double* p0, const double* p2, const JointDesc* __restrict__ jd,
                                                   const int* __restrict__ idx_q, int nb, const ClrModel& m, const MotionPrm& prm, double* cen,
                                                   double* lam, double* xf, double* cp, int lane)
{
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const ClrOrdinals no(m);
  const unsigned int nps = no.nps, self0 = no.self0();
  const int lp = m.lp, P = 1 << lp, S = 64 >> lp;
  const double block_below = prm.margin + prm.tol;

  // 0. the bound of the curve: (lin, ang, |p| + tau) of every joint from its two control segments, then Lambda of every sphere
  __syncthreads();   // (p0 and p2 are written; the last curve's readers of xf and lam are done)
  for (int k = lane; k < nb; k += 64) {
    const JointDesc& d = jd[k + 1];
    double lin = 0.0, ang = 0.0, tau = 0.0;
    if (!(d.flags & JF_NOQ)) {
      const double* q = q_row + idx_q[k + 1];
      double l0, a0, t0, l2, a2, t2;
      blend_travel(d, q, p0 + k, l0, a0, t0);
      blend_travel(d, q, p2 + k, l2, a2, t2);
      lin = 2.0 * fmax(l0, l2); ang = 2.0 * fmax(a0, a2); tau = fmax(t0, t2);
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

  double u_cur = 0.0, min_s = inf, u_min = 0.0;
  unsigned int min_ord = CLR_NO_ORDINAL;
  int status = MOTION_UNDECIDED, evals = 0, min_vox = -1;
  for (int k = 0; k < prm.max_evals; ++k) {
    __syncthreads();   // (Lambda is written; the last sample's readers of xf, cp and cen are done)
    // 1. liM of every joint at q(u)
    const double wa = (1.0 - u_cur) * (1.0 - u_cur), wb = u_cur * u_cur;
    for (int j = lane; j < nb; j += 64) {
      const JointDesc& d = jd[j + 1];
      double p[8] = {0, 0, 0, 0, 0, 0, 0, 0}, R[9], t[3];
      if (!(d.flags & JF_NOQ)) {
        double qs[7], v[6];
        const int mq = joint_nq(d), mv = joint_nv(d);
        for (int c = 0; c < 7; ++c) qs[c] = c < mq ? q_row[idx_q[j + 1] + c] : 0.0;
        for (int c = 0; c < 6; ++c) v[c] = c < mv ? wa * p0[j + c] + wb * p2[j + c] : 0.0;
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
        const double v = clr_sphere_grid(c[0], c[1], c[2], c[3], m.g).v;
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
    if (k == 0 || best < min_s) { min_s = best; u_min = u_cur; min_ord = bord; min_vox = clr_grid_voxel(bord, no, m, cen); }
    if (best < block_below) { status = MOTION_BLOCKED; break; }
    if (u_cur == 1.0) { status = MOTION_FREE; break; }
    if (k + 1 == prm.max_evals) break;   // UNDECIDED at this sample
    u_cur = fmin(u_cur + delta, 1.0);
  }
  return MotionAdv{u_cur, min_s, u_min, min_ord, status, evals, min_vox};
}

// q_path [B][T][nq], len [B] or nullptr; lim [2][nb] = v_max, a_max -> out_traj [B][S][nq] or nullptr (timing only), out_vel [B][S][nb] or
// nullptr, out_duration [B], out_info [B][4] = (n_samples, L, corners taken, flags), out_corner [B][T - 2][5], out_cinfo [B][T - 2][6] and
// out_piece [B][2 T - 3][4], each or nullptr.  slab [gridDim.x][blend_aux_doubles]: SLAB only
template <bool SLAB>
__global__ void __launch_bounds__(64)
k_blend_paths(const double* __restrict__ q_path, const int* __restrict__ len, int B, int T, int nq, const JointDesc* __restrict__ jd,
              const int* __restrict__ idx_q, int nb, ClrModel m, const double* __restrict__ lim, BlendPrm prm, double* slab,
              double* __restrict__ out_traj, double* __restrict__ out_vel, double* __restrict__ out_duration, int* __restrict__ out_info,
              double* __restrict__ out_corner, int* __restrict__ out_cinfo, double* __restrict__ out_piece)
{
  extern __shared__ __attribute__((aligned(16))) double bl_lds[];
  const int lane = threadIdx.x;
  double* cen = bl_lds;
  double* lam = SLAB ? slab + (size_t)blockIdx.x * blend_aux_doubles(nb, m.ncar, m.ns, T) : bl_lds + (size_t)4 * m.ns;
  double* xf = lam + m.ns;
  double* cp = xf + (size_t)12 * nb;
  double* pc = cp + (size_t)12 * m.ncar;       // P0 [nb], P2 [nb]
  double* sg = pc + (size_t)2 * nb;            // [T - 1][3] = (norm, A, V)
  double* co = sg + (size_t)3 * (T - 1);       // [T - 2][5] = (l, r_in, r_out, w, min_sampled); row c is corner c + 1
  double* pt = co + (size_t)5 * (T - 2);       // [2 T - 3][8] = (start, D, v0, v1, v_p, A, s0, l) of a leg, (start, D, w, w, r_in, r_out, 0, 0) of a blend
  double* dvt = pt + (size_t)8 * (2 * (size_t)T - 3);
  const double* v_max = lim;
  const double* a_max = lim + nb;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double dt = prm.dt;
  const int S = out_traj ? prm.S : 0;
  const int NC = T - 2, NP = 2 * T - 3;
  const MotionPrm mprm{prm.margin, prm.tol, prm.max_evals};
  const ClrOrdinals no(m);

  for (long long b = blockIdx.x; b < B; b += gridDim.x) {   // (64 bits: b + gridDim.x may pass 2^31)
    const int n = len ? len[b] : T;
    const double* qp = q_path + (size_t)b * T * nq;
    double* ot = out_traj ? out_traj + (size_t)b * S * nq : nullptr;
    double* ov = out_vel ? out_vel + (size_t)b * S * nb : nullptr;
    double* oc = out_corner ? out_corner + (size_t)b * NC * 5 : nullptr;
    int* oci = out_cinfo ? out_cinfo + (size_t)b * NC * 6 : nullptr;
    double* op = out_piece ? out_piece + (size_t)b * NP * 4 : nullptr;
    int* oi = out_info + (size_t)b * 4;
    const bool skipped = n < 2 || n > T;   // (wave-uniform) nothing of a skipped path is read

    // 1. the segments
    __syncthreads();   // (the last path's readers of the tables are done)
    bool bad = false;
    for (int base = 0; !skipped && base < n - 1; base += 64) {
      const int k = base + lane;
      if (k >= n - 1) continue;
      const double* qa = qp + (size_t)k * nq;
      const double* qb = qa + nq;
      double* dv = dvt + (size_t)k * nb;
      bool fin = true, same = true;
      rows_fin_same(qa, qb, nq, fin, same);
      double cv = 0.0, ca = 0.0, acc = 0.0;
      if (!fin) bad = true;
      else if (same) {   // (equal rows are 0 apart, exactly: path_length_wave's rule)
        for (int j = 0; j < nb; ++j) dv[j] = 0.0;
      } else {
        for (int j = 1; j <= nb; ++j) {
          const JointDesc& d = jd[j];
          if (d.flags & JF_NOQ) continue;
          double v[6] = {0, 0, 0, 0, 0, 0};
          const int mv = joint_nv(d), mq = joint_nq(d);
          bool still = true;
          for (int c = 0; c < mq; ++c) still = still && qa[idx_q[j] + c] == qb[idx_q[j] + c];
          if (!still) difference_joint(qa + idx_q[j], qb + idx_q[j], d, v);   // (equal coordinates of a joint are 0 apart, exactly: the rows' rule, per joint)
#pragma unroll
          for (int c = 0; c < 6; ++c)   // (constant bounds: v stays in registers)
            if (c < mv) {
              const double x = fabs(v[c]);
              dv[j - 1 + c] = v[c];
              bad = bad || !isfinite(x);
              acc += v[c] * v[c];
              cv = fmax(cv, x / v_max[j - 1 + c]);
              ca = fmax(ca, x / a_max[j - 1 + c]);
            }
        }
      }
      const bool moves = !bad && cv > 0.0 && ca > 0.0;
      double* r = sg + (size_t)3 * k;
      r[0] = moves ? sqrt(acc) : 0.0; r[1] = moves ? 1.0 / ca : 0.0; r[2] = moves ? 1.0 / cv : 0.0;
    }
    bad = __ballot(bad) != 0ull;   // (wave-uniform from here)
    __syncthreads();               // (the segments are written)

    if (skipped || bad) {
      const int flags = skipped ? RETIME_SKIPPED : RETIME_INVALID;
      if (lane == 0) { out_duration[b] = nan; oi[0] = 0; oi[1] = skipped ? 0 : n; oi[2] = 0; oi[3] = flags; }
      if (oc)
        for (size_t e = lane; e < (size_t)5 * NC; e += 64) oc[e] = nan;
      if (oci)
        for (size_t e = lane; e < (size_t)6 * NC; e += 64) { const int c = (int)(e % 6); oci[e] = c == 0 ? BLEND_OFF : c >= 4 ? -1 : c == 3 ? CLR_NONE : 0; }
      if (op)
        for (size_t e = lane; e < (size_t)4 * NP; e += 64) op[e] = nan;
      for (size_t e = lane; e < (size_t)S * nq; e += 64) ot[e] = nan;
      if (ov)
        for (size_t e = lane; e < (size_t)S * nb; e += 64) ov[e] = nan;
      continue;
    }

    // 2. the corners, one after the other, the wavefront together
    int taken_n = 0;
    for (int k = 1; k < n - 1; ++k) {
      const double n0 = sg[(size_t)3 * (k - 1)], n1 = sg[(size_t)3 * k];
      const double* dva = dvt + (size_t)(k - 1) * nb;
      const double* dvb = dvt + (size_t)k * nb;
      const double* qk = qp + (size_t)k * nq;
      int status = BLEND_OFF, tries = 0, evals = 0;
      double l_take = 0.0, r_in = 0.0, r_out = 0.0, w = 0.0, min_s = 0.0;
      unsigned int min_ord = CLR_NO_ORDINAL;
      int min_vox = -1;
      if (prm.max_tries > 0) {
        if (!(n0 > 0.0) || !(n1 > 0.0)) status = BLEND_ZERO_LEG;
        else {
          bool coupled = false;
          for (int j = lane + 1; j <= nb; j += 64) {
            const JointDesc& d = jd[j];
            if ((d.flags & JF_NOQ) || !(d.rot == ROT_FREE || d.rot == ROT_SPH || d.rot == ROT_PLANAR)) continue;
            const int mv = joint_nv(d);
            bool ma = false, mb = false;
            for (int c = 0; c < mv; ++c) { ma = ma || dva[j - 1 + c] != 0.0; mb = mb || dvb[j - 1 + c] != 0.0; }
            coupled = coupled || (ma && mb);
          }
          if (__ballot(coupled) != 0ull) status = BLEND_COUPLED;
          else {
            const double base = fmin(prm.reach, fmin(0.5 * n0, 0.5 * n1));
            for (int i = 0; i < prm.max_tries; ++i) {
              const double l = ldexp(base, -i);
              const double ri = l / n0, ro = l / n1;
              __syncthreads();   // (the last try's readers of P0 and P2 are done)
              for (int j = lane; j < nb; j += 64) { pc[j] = -ri * dva[j]; pc[nb + j] = ro * dvb[j]; }
              const MotionAdv adv = blend_advance(qk, pc, pc + nb, jd, idx_q, nb, m, mprm, cen, lam, xf, cp, lane);
              tries = i + 1;
              evals += adv.evals;
              min_s = adv.min_sampled; min_ord = adv.min_ord; min_vox = adv.min_vox;
              status = adv.status == MOTION_FREE ? BLEND_TAKEN : adv.status == MOTION_BLOCKED ? BLEND_BLOCKED : BLEND_UNDECIDED;
              if (status == BLEND_TAKEN) { l_take = l; r_in = ri; r_out = ro; break; }
            }
          }
        }
      }
      if (status == BLEND_TAKEN) {   // the rate limit, from the P0 and P2 of the try taken
        double ma = 0.0, m0 = 0.0, m2 = 0.0;
        for (int j = lane; j < nb; j += 64) {
          const double a = pc[j], c = pc[nb + j];
          ma = fmax(ma, 2.0 * fabs(a + c) / a_max[j]);
          m0 = fmax(m0, 2.0 * fabs(a) / v_max[j]);
          m2 = fmax(m2, 2.0 * fabs(c) / v_max[j]);
        }
        for (int off = 32; off > 0; off >>= 1) {
          ma = fmax(ma, __shfl_xor(ma, off)); m0 = fmax(m0, __shfl_xor(m0, off)); m2 = fmax(m2, __shfl_xor(m2, off));
        }
        w = 1.0 / fmax(sqrt(ma), fmax(m0, m2));
        ++taken_n;
      }
      if (lane == 0) {
        double* r = co + (size_t)5 * (k - 1);
        r[0] = l_take; r[1] = r_in; r[2] = r_out; r[3] = w; r[4] = min_s;
        if (oci) {
          int* o = oci + (size_t)6 * (k - 1);
          o[0] = status; o[1] = tries; o[2] = evals;
          clr_witness(min_ord, min_vox, no, m, o + 3);
        }
      }
    }
    __syncthreads();   // (the corners are written)

    // 3. the rates: forward, then backward; every lane computes the same, lane 0 writes
    {
      double vout = 0.0;   // the s-rate at which leg k starts
      for (int k = 0; k < n - 2; ++k) {   // leg k ends in corner k + 1, row k
        double* r = co + (size_t)5 * k;
        const double s0 = k > 0 ? co[(size_t)5 * (k - 1) + 2] : 0.0;
        const double ri = r[1], ro = r[2];
        double wk = r[3];
        if (wk > 0.0) {
          const double bound = vout * vout + 2.0 * sg[(size_t)3 * k + 1] * (1.0 - s0 - ri);
          const double vin = 2.0 * ri * wk;
          if (vin * vin > bound) {
            wk = sqrt(bound) / (2.0 * ri);
            if (lane == 0) r[3] = wk;
          }
        }
        vout = 2.0 * ro * wk;
      }
      __syncthreads();
      double vin = 0.0;    // the s-rate at which leg k ends
      for (int k = n - 2; k >= 1; --k) {   // leg k starts in corner k, row k - 1
        double* r = co + (size_t)5 * (k - 1);
        const double ri1 = k < n - 2 ? co[(size_t)5 * k + 1] : 0.0;
        const double ri = r[1], ro = r[2];
        double wk = r[3];
        if (wk > 0.0) {
          const double bound = vin * vin + 2.0 * sg[(size_t)3 * k + 1] * (1.0 - ro - ri1);
          const double vo = 2.0 * ro * wk;
          if (vo * vo > bound) {
            wk = sqrt(bound) / (2.0 * ro);
            if (lane == 0) r[3] = wk;
          }
        }
        vin = 2.0 * ri * wk;
      }
      __syncthreads();
    }

    // 4. the pieces in chunks of 64, each chunk's durations summed in path order behind the chunks before it
    const int np = 2 * n - 3;
    double total = 0.0;
    for (int base = 0; base < np; base += 64) {
      const int p = base + lane;
      double rec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      double D = 0.0;
      if (p < np) {
        if (p & 1) {   // corner k = (p + 1) / 2, row (p - 1) / 2
          const double* r = co + (size_t)5 * (p >> 1);
          if (r[3] > 0.0) { D = 1.0 / r[3]; rec[2] = rec[3] = r[3]; rec[4] = r[1]; rec[5] = r[2]; }
        } else {
          const int k = p >> 1;
          const double* rs = k > 0 ? co + (size_t)5 * (k - 1) : nullptr;
          const double* re = k < n - 2 ? co + (size_t)5 * k : nullptr;
          const double s0 = rs ? rs[2] : 0.0, v0 = rs ? 2.0 * rs[2] * rs[3] : 0.0;
          const double ri = re ? re[1] : 0.0, v1 = re ? 2.0 * re[1] * re[3] : 0.0;
          const double sl = 1.0 - s0 - ri, A = sg[(size_t)3 * k + 1], V = sg[(size_t)3 * k + 2];
          if (A > 0.0 && sl > 0.0) {
            const double vp = fmax(fmin(V, sqrt(0.5 * (2.0 * A * sl + v0 * v0 + v1 * v1))), fmax(v0, v1));
            const double t1 = (vp - v0) / A, t3 = (vp - v1) / A;
            const double s1 = (vp * vp - v0 * v0) / (2.0 * A), s3 = (vp * vp - v1 * v1) / (2.0 * A);
            D = t1 + fmax(sl - s1 - s3, 0.0) / vp + t3;
            rec[2] = v0; rec[3] = v1; rec[4] = vp; rec[5] = A; rec[6] = s0; rec[7] = sl;
          }
        }
      }
      double start = 0.0;
      const int cnt = min(64, np - base);
      for (int l = 0; l < cnt; ++l) {
        if (l == lane) start = total;
        total += __shfl(D, l);
      }
      if (p < np) {
        double* r = pt + (size_t)8 * p;
        r[0] = start; r[1] = D;
        for (int c = 2; c < 8; ++c) r[c] = rec[c];
      }
    }

    // the totals
    int ns = 0, flags = 0;
    {
      const double c = ceil(total / dt);
      const bool sat = !(c < 2147483647.0);
      ns = sat ? 2147483647 : (int)c + 1;
      if (out_traj && (sat || ns > S)) flags |= RETIME_TRUNCATED;
    }
    if (lane == 0) { out_duration[b] = total; oi[0] = ns; oi[1] = n; oi[2] = taken_n; oi[3] = flags; }
    __syncthreads();   // (the pieces are written)
    if (oc)
      for (size_t e = lane; e < (size_t)5 * NC; e += 64) oc[e] = e < (size_t)5 * (n - 2) ? co[e] : 0.0;
    if (oci)
      for (size_t e = (size_t)6 * (n - 2) + lane; e < (size_t)6 * NC; e += 64) { const int c = (int)(e % 6); oci[e] = c == 0 ? BLEND_OFF : c >= 4 ? -1 : c == 3 ? CLR_NONE : 0; }
    if (op)
      for (size_t e = lane; e < (size_t)4 * NP; e += 64) {
        const size_t p = e >> 2;
        op[e] = p < (size_t)np && pt[8 * p + 1] > 0.0 ? pt[8 * p + (e & 3)] : 0.0;
      }

    // 5. the samples
    const double* q_last = qp + (size_t)(n - 1) * nq;
    for (long long base = 0; base < S; base += 64) {
      const long long i = base + lane;
      if (i >= S) continue;
      double* oq = ot + (size_t)i * nq;
      double* od = ov ? ov + (size_t)i * nb : nullptr;
      const double t = (double)i * dt;
      if (t >= total) {   // at rest on the last waypoint
        for (int c = 0; c < nq; ++c) oq[c] = q_last[c];
        if (od)
          for (int c = 0; c < nb; ++c) od[c] = 0.0;
        continue;
      }
      // the last piece that has started: [lo, lo + w) holds it
      int lo = 0;
      for (int w = np; w > 1;) {
        const int half = w >> 1;
        if (pt[(size_t)8 * (lo + half)] <= t) { lo += half; w -= half; }
        else w = half;
      }
      const double* r = pt + (size_t)8 * lo;
      const double tau = t - r[0], D = r[1];
      const int k = (lo + 1) >> 1;   // the waypoint whose chart holds the piece
      const double* qk = qp + (size_t)k * nq;
      // the chart coordinates x = ca * da + cb * db and the velocity va * da + vb * db, da = dv_{k-1} (blend only), db = dv_k
      double ca_ = 0.0, cb = 0.0, va = 0.0, vb = 0.0;
      if (lo & 1) {
        const double w = r[2], u = fmin(w * tau, 1.0);
        ca_ = -r[4] * ((1.0 - u) * (1.0 - u)); cb = r[5] * (u * u);
        va = 2.0 * (1.0 - u) * r[4] * w; vb = 2.0 * u * r[5] * w;
      } else {
        const double v0 = r[2], v1 = r[3], vp = r[4], A = r[5], s0 = r[6], sl = r[7];
        const double t1 = (vp - v0) / A, t3 = (vp - v1) / A;
        double sig, sd;
        if (tau < t1) { sig = v0 * tau + 0.5 * A * tau * tau; sd = v0 + A * tau; }
        else if (tau <= D - t3) { sig = (vp * vp - v0 * v0) / (2.0 * A) + vp * (tau - t1); sd = vp; }
        else {
          const double rem = fmax(D - tau, 0.0);
          sig = sl - (v1 * rem + 0.5 * A * rem * rem); sd = v1 + A * rem;
        }
        cb = s0 + sig; vb = sd;
      }
      const double* da = dvt + (size_t)(k > 0 ? k - 1 : 0) * nb;
      const double* db = dvt + (size_t)k * nb;
      const bool blend = lo & 1;
      for (int j = 1; j <= nb; ++j) {
        const JointDesc& d = jd[j];
        if (d.flags & JF_NOQ) continue;
        double qs[7], v[6];
        const int mq = joint_nq(d), mv = joint_nv(d), iq = idx_q[j];
        for (int c = 0; c < 7; ++c) qs[c] = c < mq ? qk[iq + c] : 0.0;
        for (int c = 0; c < 6; ++c) v[c] = c >= mv ? 0.0 : blend ? ca_ * da[j - 1 + c] + cb * db[j - 1 + c] : cb * db[j - 1 + c];
        if (blend || cb != 0.0) advance_q_joint(qs, d, v);   // (a leg at parameter 0: the waypoint bit for bit)
#pragma unroll
        for (int c = 0; c < 7; ++c)   // (constant bounds: qs stays in registers)
          if (c < mq) oq[iq + c] = qs[c];
        if (od) {
#pragma unroll
          for (int c = 0; c < 6; ++c)
            if (c < mv) od[j - 1 + c] = blend ? va * da[j - 1 + c] + vb * db[j - 1 + c] : vb * db[j - 1 + c];
        }
      }
    }
  }
}

}  // namespace loikb
