// Multi-start pose IK (include/loik_amd_multistart.h): the three device steps that turn B = G * K independent pose solves into G
// answered goals, around loikb_solve_pose, which is called as it is.
//
//   k_ms_expand_targets : targets [G][nc][12] (or one shared block) -> [B][nc][12], instance b = g * K + k reads goal g
//   k_ms_set_q0         : the goals' q0 rows [G][nq] from the caller's [G][nq] / one shared row / the resident row g * K of each goal
//   k_ms_sample         : the seeds of a round into the resident q [B][nq]: lanes run along the coordinates of a row, then over the
//                         rows, so the stores are contiguous.  A per-coordinate table says "sampled DoF j" or "copy from q0" (-1).
//                         With a status pointer it is the re-sampler: rows with REACHED are left alone.
//   k_ms_select         : one workgroup per goal: each lane strides over the goal's K instances and keeps its own best
//                         (class, cost, b); wave64 butterfly (__shfl_xor), then the workgroup's wavefronts through LDS.  The keys
//                         are totally ordered (b is unique), so the order in which lanes combine cannot change the winner.
//                         count_only: nothing but the "goals with a reached seed" counter the restart loop reads.
//                         With a clearance pointer (loik_amd_collision.h) the reached seeds split into class 0 (clear by the
//                         margin) and class 0c (in collision, cost -clearance) between classes 0 and 1; only class 0 answers a goal.
//
// fp64 throughout, as loik_pose.hpp.  These kernels are microseconds beside a pose loop of milliseconds and are not tuned.
#pragma once

#include "loik_pose.hpp"

namespace loikb {

__global__ void k_ms_expand_targets(const double* __restrict__ src, int shared, int nc, int K, int B, double* __restrict__ dst)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, row = (size_t)nc * 12;
  if (i >= (size_t)B * row) return;
  const size_t b = i / row, r = i - b * row;
  dst[i] = src[(shared ? 0 : (b / K) * row) + r];
}

// dst[g][c] = src[g * stride + c]: stride nq (per goal), 0 (one shared row), K * nq (the resident q of instance g * K)
__global__ void k_ms_set_q0(const double* __restrict__ src, size_t stride, int nq, int G, double* __restrict__ dst)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)G * nq) return;
  const size_t g = i / nq, c = i - g * nq;
  dst[i] = src[g * stride + c];
}

__device__ __forceinline__ unsigned long long ms_mix(unsigned long long x)
{
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// key = ms_mix(seed + 0x9E3779B97F4A7C15 * (round + 1)), made on the host.  table [nq]: the DoF (idx_v order) whose sample the
// coordinate gets, -1: the coordinate of the goal's q0 row.  Seed k = 0 of round 0 is the q0 row itself.
__global__ void k_ms_sample(double* __restrict__ q, const double* __restrict__ q0, int nq, int B, int K, const int* __restrict__ table,
                            const double* __restrict__ s_lo, const double* __restrict__ s_hi, unsigned long long key, int round,
                            const int* __restrict__ status, int* __restrict__ round_out)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * nq) return;
  const int b = (int)(i / nq), c = (int)(i - (size_t)b * nq);
  if (status && (status[b] & POSE_REACHED)) return;
  const int g = b / K, j = table[c];
  double v = q0[(size_t)g * nq + c];
  if (j >= 0 && !(round == 0 && b == g * K)) {
    const unsigned long long word = ms_mix(key ^ (((unsigned long long)(unsigned)b << 32) | (unsigned long long)(unsigned)j));
    const double u = (double)(word >> 11) * 0x1.0p-53;   // (53 bits: both the conversion and the scaling are exact)
    const double lo = s_lo[j], hi = s_hi[j];
    const double x = __dadd_rn(lo, __dmul_rn(u, hi - lo));   // (the product rounded before the sum: no fma)
    v = x < hi ? x : hi;
  }
  q[i] = v;
  if (c == 0) round_out[b] = round;
}

// the classes as the key holds them: twice the class of loik_amd_multistart.h, so that class 0c of loik_amd_collision.h sits between
enum : int { MS_CLS_REACHED = 0, MS_CLS_COLLIDING = 1, MS_CLS_RUNNING = 2, MS_CLS_STOPPED = 4, MS_CLS_NOTHING = 6 };

struct MsKey {
  int cls;       // MS_CLS_*: reached, (reached in collision,) running out of steps, stopped, nothing (a lane without an instance)
  double cost;
  int b;
};

// a < b in (class, cost, b) with a NaN cost after every number
__device__ __forceinline__ bool ms_before(const MsKey& a, const MsKey& b)
{
  if (a.cls != b.cls) return a.cls < b.cls;
  const bool an = a.cost != a.cost, bn = b.cost != b.cost;
  if (an != bn) return bn;
  if (!an && a.cost != b.cost) return a.cost < b.cost;
  return a.b < b.b;
}

constexpr int MS_SELECT_THREADS = 256;

// dofq [nv]: the coordinate of a plain-sum DoF in a row of q, -1 for every other DoF (lim_q of the host); w [nv] or NULL = 1;
// cost_in [B] or NULL: the cost of a reached instance is read from it instead (the dexterous pick of loik_amd_jacobian.h);
// clr [B][3] or NULL: k_clearance's minima of the resident q (entry 0 is read), with wit_in [B][3] its witnesses: a reached instance
// with !(clr >= margin) is class 0c with cost -clr; then inst_clr [B], wclr [G], wwit [G][3], nclear [G] are written (not count_only)
__global__ void __launch_bounds__(MS_SELECT_THREADS)
k_ms_select(const int* __restrict__ status, const double* __restrict__ err, const double* __restrict__ q, const double* __restrict__ q0,
            const int* __restrict__ dofq, const double* __restrict__ w, int nv, int nq, int nc, int K, int pick_first, int count_only,
            unsigned int* __restrict__ goals_reached, int* __restrict__ winner, int* __restrict__ goal_status, double* __restrict__ cost_out,
            int* __restrict__ nreached, double* __restrict__ q_out, double* __restrict__ err_out, const double* __restrict__ cost_in,
            const double* __restrict__ clr, const int* __restrict__ wit_in, double margin, double* __restrict__ inst_clr,
            double* __restrict__ wclr, int* __restrict__ wwit, int* __restrict__ nclear)
{
  __shared__ MsKey sh_key[MS_SELECT_THREADS / 64];
  __shared__ int sh_n[MS_SELECT_THREADS / 64], sh_n0[MS_SELECT_THREADS / 64];
  const int g = blockIdx.x, tid = threadIdx.x;
  MsKey best{MS_CLS_NOTHING, 0.0, 0x7fffffff};
  int n = 0, n0 = 0;
  for (int k = tid; k < K; k += MS_SELECT_THREADS) {
    const int b = g * K + k, st = status[b];
    MsKey cur{MS_CLS_REACHED, 0.0, b};
    if (st & POSE_REACHED) ++n;
    const double cb = clr ? clr[(size_t)3 * b] : 0.0;
    if (clr && !count_only) inst_clr[b] = cb;
    if (st & POSE_STOPPED) cur.cls = MS_CLS_STOPPED;
    else if (!(st & POSE_REACHED)) {
      cur.cls = MS_CLS_RUNNING;
      if (!count_only) {
        const double* e = err + (size_t)b * nc * 6;
        double m = 0.0;
        for (int x = 0; x < nc * 6; ++x) {
          const double a = fabs(e[x]);
          if (a > m || a != a) m = a;   // (a NaN sticks)
        }
        cur.cost = m;
      }
    } else if (clr && !(cb >= margin)) {
      cur.cls = MS_CLS_COLLIDING;
      cur.cost = -cb;   // (the least penetration first; a NaN last)
    } else if (!count_only && cost_in) {
      cur.cost = cost_in[b];
    } else if (!count_only && !pick_first) {
      const double *row = q + (size_t)b * nq, *ref = q0 + (size_t)g * nq;
      double sum = 0.0;
      for (int j = 0; j < nv; ++j) {
        const int c = dofq[j];
        if (c < 0) continue;
        const double d = row[c] - ref[c];
        sum += (w ? w[j] : 1.0) * (d * d);
      }
      cur.cost = sum;
    }
    if (cur.cls == MS_CLS_REACHED) ++n0;
    if (ms_before(cur, best)) best = cur;
  }
  for (int off = 32; off > 0; off >>= 1) {
    MsKey o;
    o.cls = __shfl_xor(best.cls, off);
    o.cost = __shfl_xor(best.cost, off);
    o.b = __shfl_xor(best.b, off);
    n += __shfl_xor(n, off);
    n0 += __shfl_xor(n0, off);
    if (ms_before(o, best)) best = o;
  }
  if ((tid & 63) == 0) { sh_key[tid >> 6] = best; sh_n[tid >> 6] = n; sh_n0[tid >> 6] = n0; }
  __syncthreads();
  best = sh_key[0];
  n = sh_n[0];
  n0 = sh_n0[0];
  for (int v = 1; v < MS_SELECT_THREADS / 64; ++v) {
    if (ms_before(sh_key[v], best)) best = sh_key[v];
    n += sh_n[v];
    n0 += sh_n0[v];
  }
  if (count_only) {
    if (tid == 0 && best.cls == MS_CLS_REACHED) atomicAdd(goals_reached, 1u);
    return;
  }
  if (tid == 0) {
    winner[g] = best.b;
    // LOIKB_MS_GOAL_REACHED / BEST_EFFORT / FAILED, or LOIKB_MS_GOAL_IN_COLLISION = 8
    goal_status[g] = best.cls == MS_CLS_COLLIDING ? 8 : 1 << (best.cls >> 1);
    cost_out[g] = best.cost;
    nreached[g] = n;
    if (best.cls == MS_CLS_REACHED) atomicAdd(goals_reached, 1u);
    if (clr) {
      wclr[g] = clr[(size_t)3 * best.b];
      for (int x = 0; x < 3; ++x) wwit[3 * g + x] = wit_in[(size_t)3 * best.b + x];
      nclear[g] = n0;
    }
  }
  for (int c = tid; c < nq; c += MS_SELECT_THREADS) q_out[(size_t)g * nq + c] = q[(size_t)best.b * nq + c];
  for (int x = tid; x < nc * 6; x += MS_SELECT_THREADS) err_out[(size_t)g * nc * 6 + x] = err[(size_t)best.b * nc * 6 + x];
}

}  // namespace loikb
