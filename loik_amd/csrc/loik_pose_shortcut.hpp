// Certified shortcutting of joint-space paths and their lengths (include/loik_amd_shortcut.h).
//
//   k_shortcut_paths<SLAB>: one wavefront is one workgroup and owns one path from its first round to its last, then strides to the
//                           next path: the trip counts (rounds that draw, samples of a drawn segment) differ from path to path, so no
//                           path ever waits for another one -- the reason k_motion_clearance gives for one wavefront per segment.
//                           No communication between wavefronts and no spin-wait; the round loop is bounded by `rounds` in its own
//                           condition and the advancement by max_evals (motion_advance).  Every decision -- the draw, the status, the
//                           splice -- is wave-uniform.  Per round:
//                             1. the draw (i, j) from two words of the multi-start sampler (ms_mix), the key made here;
//                             2. dv = difference(q[keep[i]], q[keep[j]]), a lane per device joint with difference_joint, into a [nb]
//                                row beside Lambda;
//                             3. motion_advance (loik_pose_motion.hpp) on that segment: the body of k_motion_clearance, not a copy;
//                             4. FREE: keep[j ..] moves down onto keep[i + 1 ..], lane-strided, a barrier between the reads and
//                                the writes of every chunk of 64.
//                           The keep list is the path's out_keep row, or a row of a handle-owned scratch per resident wavefront.
//                           LDS as k_motion_clearance: the centres, and Lambda, liM, the carriers' oMi and dv beside them when it
//                           fits; SLAB = true takes those four from the global slab of the wavefront.
//   k_path_length         : a wavefront per path, a lane per segment; path_length_wave is what k_shortcut_paths reports too.
//
// fp64 whatever the handle's precision, as loik_pose.hpp.
#pragma once

#include "loik_pose_motion.hpp"
#include "loik_pose_multistart.hpp"

namespace loikb {

// doubles beside the centres of one wavefront: the records of k_motion_clearance, then dv [nb]
__host__ __device__ inline size_t shortcut_aux_doubles(int nb, int ncar, int ns) { return motion_aux_doubles(nb, ncar, ns) + (size_t)nb; }

struct ShortcutPrm {
  double margin, tol;
  int max_evals, rounds;
  unsigned long long seed;
};

// two rows of nq doubles: fin stays set when every entry of both is finite, same when they are equal entry by entry; the caller sets both
// first (path_length_wave and the segment pass of k_retime_paths, loik_pose_retime.hpp, ask the same question of a segment's ends)
__device__ __forceinline__ void rows_fin_same(const double* a, const double* b, int nq, bool& fin, bool& same)
{
  for (int k = 0; k < nq; ++k) {
    fin = fin && isfinite(a[k]) && isfinite(b[k]);
    same = same && a[k] == b[k];
  }
}

// The length of the path q[keep[0]], ..., q[keep[L - 1]] (keep == nullptr: q[0], ..., q[L - 1]) of rows of nq doubles: the sum over
// k < L - 1 of || difference(q_k, q_{k+1}) ||_2.  A lane per segment computes its difference joint by joint as k_difference does and sums
// the squares in DoF order; the segments are then summed in path order, so every lane returns the same bits.  A segment with an end
// that is not finite is NaN, and so is the sum; a segment between two finite rows that are equal entry by entry is exactly 0.  All 64
// lanes of the wavefront call it together
__device__ __forceinline__ double path_length_wave(const double* __restrict__ q, const int* keep, int L, int nq, const JointDesc* __restrict__ jd,
                                                   const int* __restrict__ idx_q, int nb, int lane)
{
  double total = 0.0;
  for (int base = 0; base < L - 1; base += 64) {
    const int t = base + lane;
    double nrm = 0.0;
    if (t < L - 1) {
      const double* a = q + (size_t)(keep ? keep[t] : t) * nq;
      const double* b = q + (size_t)(keep ? keep[t + 1] : t + 1) * nq;
      bool fin = true, same = true;
      rows_fin_same(a, b, nq, fin, same);
      if (!fin) nrm = __longlong_as_double(0x7ff8000000000000ll);
      else if (!same) {   // (equal rows are 0 apart, exactly: a repeated waypoint adds nothing, whatever log3 makes of a quaternion's rounding)
        double acc = 0.0;
        for (int j = 1; j <= nb; ++j) {
          const JointDesc& d = jd[j];
          if (d.flags & JF_NOQ) continue;
          double v[6];
          difference_joint(a + idx_q[j], b + idx_q[j], d, v);
          const int mv = joint_nv(d);
#pragma unroll
          for (int k = 0; k < 6; ++k)   // (constant bounds: v stays in registers)
            if (k < mv) acc += v[k] * v[k];
        }
        nrm = sqrt(acc);
      }
    }
    const int cnt = min(64, L - 1 - base);
    for (int l = 0; l < cnt; ++l) total += __shfl(nrm, l);
  }
  return total;
}

// out_length [B]; len [B] or nullptr (= T everywhere).  len in {0, 1}: 0; outside 0 .. T: NaN
__global__ void __launch_bounds__(64) k_path_length(const double* __restrict__ q_path, const int* __restrict__ len, int B, int T, int nq,
                                                    const JointDesc* __restrict__ jd, const int* __restrict__ idx_q, int nb,
                                                    double* __restrict__ out_length)
{
  const int lane = threadIdx.x;
  for (long long b = blockIdx.x; b < B; b += gridDim.x) {   // (64 bits: b + gridDim.x may pass 2^31)
    const int n = len ? len[b] : T;
    double v = __longlong_as_double(0x7ff8000000000000ll);
    if (n >= 0 && n <= T) v = path_length_wave(q_path + (size_t)b * T * nq, nullptr, n, nq, jd, idx_q, nb, lane);   // (n wave-uniform)
    if (lane == 0) out_length[b] = v;
  }
}

// q_path [B][T][nq], len [B] or nullptr -> out_path [B][T][nq], out_info [B][6] = (L, tried, accepted, blocked, undecided, invalid),
// out_keep [B][T] or nullptr, out_val [B][2] = (length before, length after) or nullptr.  keep_scr [gridDim.x][T]: the keep rows
// when out_keep is nullptr.  slab [gridDim.x][shortcut_aux_doubles]: SLAB only
template <bool SLAB>
__global__ void __launch_bounds__(64)
k_shortcut_paths(const double* __restrict__ q_path, const int* __restrict__ len, int B, int T, int nq, const JointDesc* __restrict__ jd,
                 const int* __restrict__ idx_q, int nb, ClrModel m, ShortcutPrm prm, double* slab, int* keep_scr, double* __restrict__ out_path,
                 int* out_keep, int* __restrict__ out_info, double* __restrict__ out_val)
{
  extern __shared__ __attribute__((aligned(16))) double sc_lds[];
  const int lane = threadIdx.x;
  double* cen = sc_lds;
  double* lam = SLAB ? slab + (size_t)blockIdx.x * shortcut_aux_doubles(nb, m.ncar, m.ns) : sc_lds + (size_t)4 * m.ns;
  double* xf = lam + m.ns;
  double* cp = xf + (size_t)12 * nb;
  double* dvr = cp + (size_t)12 * m.ncar;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const MotionPrm mprm{prm.margin, prm.tol, prm.max_evals};

  for (long long b = blockIdx.x; b < B; b += gridDim.x) {   // (64 bits: b + gridDim.x may pass 2^31)
    const int n = len ? len[b] : T;
    const double* qp = q_path + (size_t)b * T * nq;
    double* op = out_path + (size_t)b * T * nq;
    int* oi = out_info + (size_t)b * 6;
    if (n < 2 || n > T) {   // (wave-uniform) skipped: nothing of it is read
      for (size_t e = lane; e < (size_t)T * nq; e += 64) op[e] = nan;
      if (out_keep)
        for (int k = lane; k < T; k += 64) out_keep[(size_t)b * T + k] = -1;
      if (lane < 6) oi[lane] = 0;
      if (out_val && lane < 2) out_val[(size_t)b * 2 + lane] = nan;
      continue;
    }
    int* keep = out_keep ? out_keep + (size_t)b * T : keep_scr + (size_t)blockIdx.x * T;
    __syncthreads();   // (the last path's readers of a scratch keep row are done)
    for (int k = lane; k < T; k += 64) keep[k] = k < n ? k : -1;
    __syncthreads();
    double len_in = 0.0;
    if (out_val) len_in = path_length_wave(qp, keep, n, nq, jd, idx_q, nb, lane);

    int L = n, tried = 0, accepted = 0, blocked = 0, undecided = 0, invalid = 0;
    const unsigned long long hi = (unsigned long long)(unsigned int)b << 32;
    for (int r = 0; r < prm.rounds && L >= 3; ++r) {
      // 1. the draw: 0 <= i, i + 2 <= j <= L - 1
      const unsigned long long key = ms_mix(prm.seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)r + 1ull));
      const int i = (int)(ms_mix(key ^ hi) % (unsigned long long)(L - 2));
      const int j = i + 2 + (int)(ms_mix(key ^ (hi | 1ull)) % (unsigned long long)(L - 2 - i));
      const double* qa = qp + (size_t)__builtin_amdgcn_readfirstlane(keep[i]) * nq;
      const double* qb = qp + (size_t)__builtin_amdgcn_readfirstlane(keep[j]) * nq;
      ++tried;
      // 2. dv: NaN in k_difference's terms when an end is not finite, and then INVALID as a dv that is not finite itself
      bool fin = true;
      for (int k = lane; k < nq; k += 64) fin &= (bool)isfinite(qa[k]) && (bool)isfinite(qb[k]);
      bool ok = __ballot(!fin) == 0ull;   // (wave-uniform)
      if (ok) {
        __syncthreads();   // (the last round's readers of dv are done)
        for (int k = lane + 1; k <= nb; k += 64) {
          const JointDesc& d = jd[k];
          if (d.flags & JF_NOQ) continue;
          double v[6];
          difference_joint(qa + idx_q[k], qb + idx_q[k], d, v);
          const int mv = joint_nv(d);
#pragma unroll
          for (int c = 0; c < 6; ++c)   // (constant bounds: v stays in registers)
            if (c < mv) dvr[k - 1 + c] = v[c];
        }
        __syncthreads();
        for (int k = lane; k < nb; k += 64) fin &= (bool)isfinite(dvr[k]);
        ok = __ballot(!fin) == 0ull;
      }
      if (!ok) { ++invalid; continue; }
      // 3. the certified check of k_motion_clearance
      // (the grid pair behind a call in the LDS instantiation only: with it in line the ROCm 7.2 compiler's register allocator crashes on that
      //  kernel, and on no other.  Nothing about the slab asks for it: profiles/grid_measured.md)
      constexpr bool GRID_CALL = !SLAB;
      const MotionAdv adv = motion_advance<GRID_CALL>(qa, dvr, jd, idx_q, nb, m, mprm, cen, lam, xf, cp, lane);
      if (adv.status == MOTION_BLOCKED) { ++blocked; continue; }
      if (adv.status != MOTION_FREE) { ++undecided; continue; }
      // 4. the splice: keep[k - cut] = keep[k] for k = j .. L - 1, in chunks of 64 from the low end (a chunk's writes land below its
      //    own reads and on entries that earlier chunks have read)
      ++accepted;
      const int cut = j - i - 1;
      for (int base = j; base < L; base += 64) {
        const int k = base + lane;
        const int v = k < L ? keep[k] : 0;
        __syncthreads();
        if (k < L) keep[k - cut] = v;
        __syncthreads();
      }
      L -= cut;
    }

    // the outputs: the kept rows bit for bit, the last one repeated; -1 after the kept indices
    __syncthreads();
    for (size_t e = lane; e < (size_t)T * nq; e += 64) {
      const int k = (int)(e / (size_t)nq), c = (int)(e - (size_t)k * nq);
      op[e] = qp[(size_t)keep[min(k, L - 1)] * nq + c];
    }
    double len_out = 0.0;
    if (out_val) len_out = path_length_wave(qp, keep, L, nq, jd, idx_q, nb, lane);
    __syncthreads();   // (keep[L - 1 ..] has been read)
    for (int k = L + lane; k < T; k += 64) keep[k] = -1;
    if (lane == 0) {
      oi[0] = L; oi[1] = tried; oi[2] = accepted; oi[3] = blocked; oi[4] = undecided; oi[5] = invalid;
      if (out_val) { out_val[(size_t)b * 2] = len_in; out_val[(size_t)b * 2 + 1] = len_out; }
    }
  }
}

}  // namespace loikb
