// Certified RRT-Connect planning of joint-space paths (include/loik_amd_plan.h).
//
//   k_plan_paths<SLAB>: one wavefront is one workgroup and owns one query from its first check to its outputs, then strides to the next
//                       query: the trip counts (iterations, nodes of a connect, samples of an edge) differ from query to query, so no
//                       query ever waits for another one -- the reason k_shortcut_paths gives for one wavefront per path.  No
//                       communication between wavefronts and no spin-wait; the iteration loop is bounded by max_iters, the
//                       extensions of an iteration by max_nodes and the advancement by max_evals (motion_advance), each in its own
//                       condition.  Every decision -- the nearest node, reach or step, the status of an edge -- is wave-uniform.
//                       The two checks of step 0 and the extensions of an iteration are trips of ONE loop body, so the kernel holds
//                       one copy of each phase and their live ranges stay apart:
//                         1. (first extension of a tree in an iteration) the nearest node: lanes stride over the tree's rows, each
//                            keeps its least (dist2, index), one wave64 butterfly carries the ordered minimum;
//                         2. dv = diff(node_k, target) into the dv row, a lane per device joint (difference_joint), and d;
//                         3. the new configuration: the target itself, or node_k (+) (step / d) dv with advance_q_joint, into the
//                            tree's next free row;
//                         4. dv of the edge in its output direction, and motion_advance (loik_pose_motion.hpp) on it: the body of
//                            k_motion_clearance, not a copy;
//                         5. the bookkeeping: a node and its parent, trapped, or the bridge.
//                       The trees are rows [node][nq] with a parent per node in a handle-owned scratch per resident wavefront, beside
//                       them the sample q_rand and the node list of the found path.  LDS as k_shortcut_paths: the centres, and Lambda,
//                       liM, the carriers' oMi and dv beside them when it fits; SLAB = true takes those four from the global slab of
//                       the wavefront.
//
// fp64 whatever the handle's precision, as loik_pose.hpp.
#pragma once

#include "loik_pose_shortcut.hpp"

namespace loikb {

enum : int { PLAN_FOUND = 0, PLAN_EXHAUSTED_ITERS = 1, PLAN_EXHAUSTED_NODES = 2, PLAN_START_BLOCKED = 3, PLAN_GOAL_BLOCKED = 4, PLAN_TOO_LONG = 5,
             PLAN_INVALID = 6, PLAN_RUNNING = -1 };

struct PlanPrm {
  double margin, tol, step;
  int max_evals, max_iters, max_nodes;
  unsigned long long seed;
};

// the scratch of one resident wavefront: doubles = two trees of max_nodes rows and q_rand; ints = two parent lists and the path's nodes
__host__ __device__ inline size_t plan_scr_doubles(int max_nodes, int nq) { return ((size_t)2 * max_nodes + 1) * (size_t)nq; }
__host__ __device__ inline size_t plan_scr_ints(int max_nodes, int T) { return (size_t)2 * max_nodes + (size_t)T; }

// dv [nb] = diff(a, b) of two finite rows by the 64 lanes: a lane per device joint with difference_joint; rows that are equal entry by
// entry give 0 exactly.  The caller puts a barrier before (the last readers of dv) and after
__device__ __forceinline__ void plan_diff_row(const double* a, const double* b, int nq, const JointDesc* __restrict__ jd, const int* __restrict__ idx_q,
                                              int nb, double* dvr, int lane)
{
  bool same = true;
  for (int k = lane; k < nq; k += 64) same &= a[k] == b[k];
  const bool zero = __ballot(!same) == 0ull;   // (wave-uniform)
  for (int k = lane + 1; k <= nb; k += 64) {
    const JointDesc& d = jd[k];
    if (d.flags & JF_NOQ) continue;
    double v[6] = {0, 0, 0, 0, 0, 0};
    if (!zero) difference_joint(a + idx_q[k], b + idx_q[k], d, v);
    const int mv = joint_nv(d);
#pragma unroll
    for (int c = 0; c < 6; ++c)   // (constant bounds: v stays in registers)
      if (c < mv) dvr[k - 1 + c] = v[c];
  }
}

// q_start, q_goal [B][nq]; s_lo, s_hi [nb] with s_coord [nb] = the coordinate of a sampled DoF in a row of q, -1: not sampled.
// out_path [B][T][nq], out_info [B][8], out_length [B] or nullptr.  scr_d [gridDim.x][plan_scr_doubles], scr_i [gridDim.x][plan_scr_ints].
// slab [gridDim.x][shortcut_aux_doubles]: SLAB only
template <bool SLAB>
__global__ void __launch_bounds__(64)
k_plan_paths(const double* __restrict__ q_start, const double* __restrict__ q_goal, int B, int T, int nq, const JointDesc* __restrict__ jd,
             const int* __restrict__ idx_q, int nb, ClrModel m, PlanPrm prm, const double* __restrict__ s_lo, const double* __restrict__ s_hi,
             const int* __restrict__ s_coord, double* slab, double* scr_d, int* scr_i, double* out_path, int* __restrict__ out_info,
             double* __restrict__ out_length)
{
  extern __shared__ __attribute__((aligned(16))) double pl_lds[];
  const int lane = threadIdx.x;
  double* cen = pl_lds;
  double* lam = SLAB ? slab + (size_t)blockIdx.x * shortcut_aux_doubles(nb, m.ncar, m.ns) : pl_lds + (size_t)4 * m.ns;
  double* xf = lam + m.ns;
  double* cp = xf + (size_t)12 * nb;
  double* dvr = cp + (size_t)12 * m.ncar;
  const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
  const MotionPrm mprm{prm.margin, prm.tol, prm.max_evals};
  const int N = prm.max_nodes;
  double* rows = scr_d + (size_t)blockIdx.x * plan_scr_doubles(N, nq);   // tree t, node i: rows + (t N + i) nq
  double* qrand = rows + (size_t)2 * N * nq;
  int* par = scr_i + (size_t)blockIdx.x * plan_scr_ints(N, T);            // tree t, node i: par[t N + i]
  int* pidx = par + (size_t)2 * N;                                        // the found path: row k of it is rows + pidx[k] nq

  for (long long b = blockIdx.x; b < B; b += gridDim.x) {   // (64 bits: b + gridDim.x may pass 2^31)
    const double* qs = q_start + (size_t)b * nq;
    const double* qg = q_goal + (size_t)b * nq;
    double* op = out_path + (size_t)b * T * nq;
    int* oi = out_info + (size_t)b * 8;
    int status = PLAN_RUNNING, L = 0, iters = 0, edges = 0, edges_free = 0, bridge0 = 0, bridge1 = 0;
    int n[2] = {0, 0};
    long long evals = 0;

    bool fin = true;
    for (int k = lane; k < nq; k += 64) fin &= (bool)isfinite(qs[k]) && (bool)isfinite(qg[k]);
    if (__ballot(!fin) != 0ull) status = PLAN_INVALID;   // (wave-uniform)
    if (status == PLAN_RUNNING) {
      __syncthreads();   // (the last query's readers of the rows and of dv are done)
      for (int k = lane; k < nq; k += 64) { rows[k] = qs[k]; rows[(size_t)N * nq + k] = qg[k]; }
      if (lane == 0) { par[0] = -1; par[N] = -1; }
      plan_diff_row(qs, qg, nq, jd, idx_q, nb, dvr, lane);
      __syncthreads();
      for (int k = lane; k < nb; k += 64) fin &= (bool)isfinite(dvr[k]);
      if (__ballot(!fin) != 0ull) status = PLAN_INVALID;
      else n[0] = n[1] = 1;
    }

    // r = -2: check(start, goal), an extension of tree 0 from its root that reaches the goal whatever the step; r = -1: check(goal,
    // goal), the same of tree 1; r >= 0: the iterations
    for (int r = -2; r < prm.max_iters && status == PLAN_RUNNING; ++r) {
      const bool pre = r < 0;
      const int a = pre ? -1 - r : (r & 1);   // (r = -2: a = 1, so that tree 1 - a = 0 is checked; r = -1: tree 1)
      if (!pre) {
        ++iters;
        const unsigned long long key = ms_mix(prm.seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)r + 1ull));
        const unsigned long long hi32 = (unsigned long long)(unsigned int)b << 32;
        __syncthreads();   // (the last iteration's readers of q_rand are done)
        for (int k = lane; k < nq; k += 64) qrand[k] = qs[k];
        __syncthreads();
        for (int j = lane; j < nb; j += 64) {
          const int c = s_coord[j];
          if (c < 0) continue;
          const unsigned long long word = ms_mix(key ^ (hi32 | (unsigned long long)(unsigned int)j));
          const double u = (double)(word >> 11) * 0x1.0p-53;   // (53 bits: both the conversion and the scaling are exact)
          const double lo = s_lo[j], hi = s_hi[j];
          const double x = __dadd_rn(lo, __dmul_rn(u, hi - lo));   // (the product rounded before the sum: no fma)
          qrand[c] = x < hi ? x : hi;
        }
      }
      // c = 0: tree a extends towards q_rand; c >= 1: tree 1 - a connects to the node that made.  A connect adds at most max_nodes - 1 nodes
      int k = 0;
      for (int c = pre ? 1 : 0; c <= N; ++c) {
        const int t = c == 0 ? a : 1 - a;
        double* tree = rows + (size_t)t * N * nq;
        const double* target = pre ? qg : c == 0 ? qrand : rows + ((size_t)a * N + (n[a] - 1)) * nq;
        __syncthreads();   // (q_rand, the last node and its parent are written; the last trip's readers of dv are done)
        // 1. the nearest node
        if (pre) k = 0;
        else if (c > 1) k = n[t] - 1;
        else {
          double best = inf;
          int bi = 0;
          for (int i = lane; i < n[t]; i += 64) {
            const double* row = tree + (size_t)i * nq;
            bool same = true;
            for (int e = 0; e < nq; ++e) same = same && row[e] == target[e];
            double acc = 0.0;
            if (!same)
              for (int j = 1; j <= nb; ++j) {
                const JointDesc& d = jd[j];
                if (d.flags & JF_NOQ) continue;
                double v[6];
                difference_joint(row + idx_q[j], target + idx_q[j], d, v);
                const int mv = joint_nv(d);
#pragma unroll
                for (int e = 0; e < 6; ++e)   // (constant bounds: v stays in registers)
                  if (e < mv) acc += v[e] * v[e];
              }
            if (acc < best) { best = acc; bi = i; }   // (a lane's indices ascend: the first of equal minima stays)
          }
          for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(best, off);
            const int ob = __shfl_xor(bi, off);
            if (ov < best || (ov == best && ob < bi)) { best = ov; bi = ob; }
          }
          k = bi;   // (0 <= k < n[t]: a lane without a node holds (inf, 0))
        }
        const double* node = tree + (size_t)k * nq;
        // 2. dv towards the target and its length, the squares summed in DoF order by every lane alike
        plan_diff_row(node, target, nq, jd, idx_q, nb, dvr, lane);
        __syncthreads();
        double d2 = 0.0;
        for (int j = 0; j < nb; ++j) d2 += dvr[j] * dvr[j];
        const double dist = sqrt(d2);
        const bool reach = pre || dist <= prm.step;
        if ((!reach || c == 0) && n[t] >= N) { status = PLAN_EXHAUSTED_NODES; break; }
        // 3. the new configuration: the target's row itself in a connect that reaches, else the tree's next row
        const double* fresh = target;
        if (!reach || c == 0) {
          double* slot = tree + (size_t)n[t] * nq;
          for (int e = lane; e < nq; e += 64) slot[e] = reach ? target[e] : node[e];
          if (!reach) {
            const double cstep = prm.step / dist;
            __syncthreads();
            for (int j = lane; j < nb; j += 64) {
              const JointDesc& d = jd[j + 1];
              if (d.flags & JF_NOQ) continue;
              double qj[7], v[6];
              const int mq = joint_nq(d), mv = joint_nv(d);
              for (int e = 0; e < 7; ++e) qj[e] = e < mq ? node[idx_q[j + 1] + e] : 0.0;
              for (int e = 0; e < 6; ++e) v[e] = e < mv ? cstep * dvr[j + e] : 0.0;
              advance_q_joint(qj, d, v);
              for (int e = 0; e < 7; ++e)
                if (e < mq) slot[idx_q[j + 1] + e] = qj[e];
            }
          }
          fresh = slot;
        }
        // 4. the edge in the direction of the output: node -> new on tree 0, new -> node on tree 1
        const double* from = t == 0 ? node : fresh;
        const double* to = t == 0 ? fresh : node;
        __syncthreads();   // (the new row is written; the readers of dv are done)
        plan_diff_row(from, to, nq, jd, idx_q, nb, dvr, lane);
        const MotionAdv adv = motion_advance(from, dvr, jd, idx_q, nb, m, mprm, cen, lam, xf, cp, lane);
        ++edges;
        evals += adv.evals;
        const bool free_edge = adv.status == MOTION_FREE;
        if (free_edge) ++edges_free;
        // 5. the bookkeeping
        if (pre) {
          if (r == -2 && free_edge) { status = PLAN_FOUND; bridge0 = 0; bridge1 = 0; }
          else if (r == -2 && adv.status == MOTION_BLOCKED && adv.s_free == 0.0) status = PLAN_START_BLOCKED;
          else if (r == -1 && adv.status == MOTION_BLOCKED) status = PLAN_GOAL_BLOCKED;
          break;
        }
        if (!free_edge) break;   // trapped
        if (c > 0 && reach) {
          status = PLAN_FOUND;
          bridge0 = t == 0 ? k : n[0] - 1;
          bridge1 = t == 1 ? k : n[1] - 1;
          break;
        }
        if (lane == 0) par[t * N + n[t]] = k;
        ++n[t];
      }
    }
    if (status == PLAN_RUNNING) status = PLAN_EXHAUSTED_ITERS;

    // the path: the parents of the bridge on tree 0 back to front, then those of the bridge on tree 1
    __syncthreads();
    if (status == PLAN_FOUND) {
      int l0 = 1, l1 = 1;
      for (int i = 0, x = bridge0; i < N && par[x] >= 0; ++i) { x = par[x]; ++l0; }
      for (int i = 0, x = bridge1; i < N && par[N + x] >= 0; ++i) { x = par[N + x]; ++l1; }
      L = l0 + l1;
      if (L > T) status = PLAN_TOO_LONG;
      else if (lane == 0) {
        for (int i = 0, x = bridge0; i < l0; ++i) { pidx[l0 - 1 - i] = x; x = par[x]; }
        for (int i = 0, x = bridge1; i < l1; ++i) { pidx[l0 + i] = N + x; x = par[N + x]; }
      }
    }
    __syncthreads();
    double len = nan;
    if (status == PLAN_FOUND) {
      for (size_t e = lane; e < (size_t)T * nq; e += 64) {
        const int w = (int)(e / (size_t)nq), c = (int)(e - (size_t)w * nq);
        op[e] = rows[(size_t)pidx[min(w, L - 1)] * nq + c];
      }
      if (out_length) {
        __syncthreads();   // (the rows of the path are written)
        len = path_length_wave(op, nullptr, L, nq, jd, idx_q, nb, lane);
      }
    } else {
      for (size_t e = lane; e < (size_t)T * nq; e += 64) op[e] = nan;
    }
    if (lane == 0) {
      oi[0] = status; oi[1] = L; oi[2] = iters; oi[3] = n[0]; oi[4] = n[1]; oi[5] = edges; oi[6] = edges_free;
      oi[7] = (int)(evals < 0x7fffffffll ? evals : 0x7fffffffll);
      if (out_length) out_length[b] = len;
    }
  }
}

}  // namespace loikb
