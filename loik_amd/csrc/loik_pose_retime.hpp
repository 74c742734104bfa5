// Time-optimal retiming of joint-space paths (include/loik_amd_retime.h).
//
//   k_retime_paths<SLAB>: one wavefront is one workgroup and owns one path from its first segment to its last sample, then strides to
//                         the next path: the sample counts differ from path to path, so no path waits for another one.  No
//                         communication between wavefronts and no spin-wait; every loop is bounded by T, S, nq or nb in its own condition.
//                           1. per segment, a lane per segment in chunks of 64: dv_k with difference_joint (stored once: a sample never
//                              takes a logarithm), cv, ca and the segment's record;
//                           2. the starts (with SNAP the ticks) summed in path order over __shfl, as path_length_wave sums its
//                              segments, so every lane holds the same bits; the records go into the table;
//                           3. per sample, a lane per sample in chunks of 64: the lane bisects the starts, evaluates the profile and
//                              walks the device joints with advance_q_joint.  Consecutive lanes write consecutive rows.
//                         The table [T - 1][5] = (start | tick bits, duration, t_acc, peak, A) and the dv rows [T - 1][nb] are in LDS
//                         when they fit; SLAB = true takes both from the global slab of the wavefront.
//
// fp64 whatever the handle's precision, as loik_pose.hpp.
#pragma once

#include "loik_pose_shortcut.hpp"

namespace loikb {

enum : int { RETIME_TRUNCATED = 1, RETIME_INVALID = 2, RETIME_SKIPPED = 4 };

// doubles of one wavefront's tables: the records [T - 1][5], then dv [T - 1][nb]
__host__ __device__ inline size_t retime_tab_doubles(int T, int nb) { return (size_t)(T - 1) * (size_t)(5 + nb); }

struct RetimePrm {
  double dt;
  int snap;
  int S;   // rows of out_traj (ignored when out_traj is nullptr)
};

// q_path [B][T][nq], len [B] or nullptr; lim [2][nb] = v_max, a_max -> out_traj [B][S][nq] or nullptr (timing only), out_vel [B][S][nb] or
// nullptr, out_seg [B][T - 1][4] or nullptr, out_duration [B], out_info [B][4] = (n_samples, L, moved segments, flags).
// slab [gridDim.x][retime_tab_doubles]: SLAB only
template <bool SLAB>
__global__ void __launch_bounds__(64)
k_retime_paths(const double* __restrict__ q_path, const int* __restrict__ len, int B, int T, int nq, const JointDesc* __restrict__ jd,
               const int* __restrict__ idx_q, int nb, const double* __restrict__ lim, RetimePrm prm, double* slab, double* __restrict__ out_traj,
               double* __restrict__ out_vel, double* __restrict__ out_seg, double* __restrict__ out_duration, int* __restrict__ out_info)
{
  extern __shared__ __attribute__((aligned(16))) double rt_lds[];
  const int lane = threadIdx.x;
  double* tab = SLAB ? slab + (size_t)blockIdx.x * retime_tab_doubles(T, nb) : rt_lds;
  double* dvt = tab + (size_t)5 * (T - 1);
  const double* v_max = lim;
  const double* a_max = lim + nb;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double dt = prm.dt;
  const int S = out_traj ? prm.S : 0;

  for (long long b = blockIdx.x; b < B; b += gridDim.x) {   // (64 bits: b + gridDim.x may pass 2^31)
    const int n = len ? len[b] : T;
    const double* qp = q_path + (size_t)b * T * nq;
    double* ot = out_traj ? out_traj + (size_t)b * S * nq : nullptr;
    double* ov = out_vel ? out_vel + (size_t)b * S * nb : nullptr;
    double* os = out_seg ? out_seg + (size_t)b * (T - 1) * 4 : nullptr;
    int* oi = out_info + (size_t)b * 4;
    const bool skipped = n < 2 || n > T;   // (wave-uniform) nothing of a skipped path is read

    // 1. and 2.: the segments in chunks of 64, each chunk's durations summed in path order behind the chunks before it
    __syncthreads();   // (the last path's readers of the tables are done)
    bool bad = false;
    double total = 0.0;
    long long ticks = 0;
    int moved = 0;
    for (int base = 0; !skipped && base < n - 1; base += 64) {
      const int k = base + lane;
      double D = 0.0, t_acc = 0.0, peak = 0.0, A = 0.0;
      long long nk = 0;
      if (k < n - 1) {
        const double* qa = qp + (size_t)k * nq;
        const double* qb = qa + nq;
        double* dv = dvt + (size_t)k * nb;
        bool fin = true, same = true;
        rows_fin_same(qa, qb, nq, fin, same);
        double cv = 0.0, ca = 0.0;
        if (!fin) bad = true;
        else if (same) {   // (equal rows are 0 apart, exactly: path_length_wave's rule)
          for (int j = 0; j < nb; ++j) dv[j] = 0.0;
        } else {
          for (int j = 1; j <= nb; ++j) {
            const JointDesc& d = jd[j];
            if (d.flags & JF_NOQ) continue;
            double v[6];
            difference_joint(qa + idx_q[j], qb + idx_q[j], d, v);
            const int mv = joint_nv(d);
#pragma unroll
            for (int c = 0; c < 6; ++c)   // (constant bounds: v stays in registers)
              if (c < mv) {
                const double x = fabs(v[c]);
                dv[j - 1 + c] = v[c];
                bad = bad || !isfinite(x);
                cv = fmax(cv, x / v_max[j - 1 + c]);
                ca = fmax(ca, x / a_max[j - 1 + c]);
              }
          }
        }
        if (!bad && cv > 0.0 && ca > 0.0) {
          A = 1.0 / ca;
          if (ca >= cv * cv) {   // triangular: the velocity limit is never reached
            const double rt = sqrt(ca);
            D = 2.0 * rt; t_acc = rt; peak = 1.0 / rt;
          } else {
            t_acc = ca / cv;
            D = cv + t_acc; peak = 1.0 / cv;
          }
          if (prm.snap) {
            const double nd = ceil(D / dt);
            nk = nd < 2147483648.0 ? (long long)nd : 2147483648ll;
            D = dt * nd;
            peak = 2.0 / (D + sqrt(fmax(D * D - 4.0 * ca, 0.0)));
            t_acc = peak * ca;
          }
        }
      }
      moved += __popcll(__ballot(D > 0.0));
      double start = 0.0;
      long long tick = 0;
      const int cnt = min(64, n - 1 - base);
      for (int l = 0; l < cnt; ++l) {
        if (l == lane) { start = total; tick = ticks; }
        total += __shfl(D, l);
        ticks += ((long long)__shfl((int)(nk >> 32), l) << 32) | (long long)(unsigned int)__shfl((int)nk, l);
      }
      if (k < n - 1) {
        double* r = tab + (size_t)5 * k;
        r[0] = prm.snap ? __longlong_as_double(tick) : start;
        r[1] = D; r[2] = t_acc; r[3] = peak; r[4] = A;
      }
    }
    if (prm.snap) total = dt * (double)ticks;
    bad = __ballot(bad) != 0ull;   // (wave-uniform from here)

    // the totals
    int ns = 0, flags = skipped ? RETIME_SKIPPED : bad ? RETIME_INVALID : 0;
    if (flags == 0) {
      bool sat;
      if (prm.snap) { sat = ticks + 1 > 2147483647ll; ns = sat ? 2147483647 : (int)ticks + 1; }
      else {
        const double c = ceil(total / dt);
        sat = !(c < 2147483647.0);
        ns = sat ? 2147483647 : (int)c + 1;
      }
      if (out_traj && (sat || ns > S)) flags |= RETIME_TRUNCATED;
    }
    if (lane == 0) {
      out_duration[b] = flags & (RETIME_SKIPPED | RETIME_INVALID) ? nan : total;
      oi[0] = ns; oi[1] = skipped ? 0 : n; oi[2] = flags & RETIME_INVALID ? 0 : moved; oi[3] = flags;
    }
    __syncthreads();   // (the tables are written)
    if (flags & (RETIME_SKIPPED | RETIME_INVALID)) {
      if (os)
        for (size_t e = lane; e < (size_t)4 * (T - 1); e += 64) os[e] = nan;
      for (size_t e = lane; e < (size_t)S * nq; e += 64) ot[e] = nan;
      if (ov)
        for (size_t e = lane; e < (size_t)S * nb; e += 64) ov[e] = nan;
      continue;
    }
    if (os)
      for (size_t e = lane; e < (size_t)4 * (T - 1); e += 64) {   // (size_t: 4 T may pass 2^31)
        const int k = (int)(e >> 2), c = (int)(e & 3);
        double x = 0.0;
        if (k < n - 1) {
          x = tab[(size_t)5 * k + c];
          if (c == 0) x = !(tab[(size_t)5 * k + 1] > 0.0) ? 0.0 : prm.snap ? dt * (double)__double_as_longlong(x) : x;   // (no motion: zeros)
        }
        os[e] = x;
      }

    // 3. the samples
    const double* q_last = qp + (size_t)(n - 1) * nq;
    for (long long base = 0; base < S; base += 64) {
      const long long i = base + lane;
      if (i >= S) continue;
      double* oq = ot + (size_t)i * nq;
      double* od = ov ? ov + (size_t)i * nb : nullptr;
      const double t = (double)i * dt;
      if (prm.snap ? i >= ticks : t >= total) {   // at rest on the last waypoint
        for (int c = 0; c < nq; ++c) oq[c] = q_last[c];
        if (od)
          for (int c = 0; c < nb; ++c) od[c] = 0.0;
        continue;
      }
      // the last segment that has started: [lo, lo + w) holds it
      int lo = 0;
      for (int w = n - 1; w > 1;) {
        const int half = w >> 1;
        const double key = tab[(size_t)5 * (lo + half)];
        if (prm.snap ? __double_as_longlong(key) <= i : key <= t) { lo += half; w -= half; }
        else w = half;
      }
      const double* r = tab + (size_t)5 * lo;
      const double tau = prm.snap ? (double)(i - __double_as_longlong(r[0])) * dt : t - r[0];
      const double D = r[1], t_acc = r[2], peak = r[3], A = r[4];
      double s, sd;
      if (tau < t_acc) { s = 0.5 * A * tau * tau; sd = A * tau; }
      else if (tau <= D - t_acc) { s = peak * (tau - 0.5 * t_acc); sd = peak; }
      else {
        const double rem = fmax(D - tau, 0.0);
        s = 1.0 - 0.5 * A * rem * rem; sd = A * rem;
      }
      const double* qk = qp + (size_t)lo * nq;
      const double* dv = dvt + (size_t)lo * nb;
      for (int j = 1; j <= nb; ++j) {
        const JointDesc& d = jd[j];
        if (d.flags & JF_NOQ) continue;
        double qs[7], v[6];
        const int mq = joint_nq(d), mv = joint_nv(d), iq = idx_q[j];
        for (int c = 0; c < 7; ++c) qs[c] = c < mq ? qk[iq + c] : 0.0;
        for (int c = 0; c < 6; ++c) v[c] = c < mv ? s * dv[j - 1 + c] : 0.0;
        if (s != 0.0) advance_q_joint(qs, d, v);   // (s == 0: the waypoint bit for bit)
#pragma unroll
        for (int c = 0; c < 7; ++c)   // (constant bounds: qs stays in registers)
          if (c < mq) oq[iq + c] = qs[c];
        if (od) {
#pragma unroll
          for (int c = 0; c < 6; ++c)
            if (c < mv) od[j - 1 + c] = sd * dv[j - 1 + c];
        }
      }
    }
  }
}

}  // namespace loikb
