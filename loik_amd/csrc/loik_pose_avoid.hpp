// Collision avoidance in the pose loops and clearance gradients (include/loik_amd_avoid.h).
//
//   k_avoid_box<HBM, MODE, T> : one wavefront per configuration, several per workgroup (the launch rule of k_clearance).
//                        1. liM of every device joint into LDS (k_clearance's stage 1, unchanged);
//                        2. a lane per device joint composes its world placement along its root path, leaf side first as k_clearance
//                           does for the carriers, and on the same walk sets its row of the ancestor table (bit j of row L: device joint
//                           j + 1 is on the root path of L + 1 -- the walk k_frame_jacobians marks `pos` with, kept for every joint
//                           because a configuration has a constraint per sphere, not one link).  A lane per sphere then writes the world
//                           centre, the radius and the carrier joint into LDS;
//                        3. k_clearance's pair loops, reduced per sphere slot: the 64 >> lp lanes that share a sphere end their walk
//                           over the world with a butterfly across the obstacle slots, under clr_before with the ordinal of the object
//                           (world spheres first, then boxes); the self pairs whose first index is a are one contiguous stretch of the
//                           sorted list, found by bisection (its trip count depends on the list alone), and a lane per sphere walks it.
//                           Both go into the table tv / to [ns][2].  A handle that latched the nearest-voxel transform of a voxel world
//                           (m.g.F not null: loik_pose_gridnear.hpp) has one more world object per sphere, the grid, at ordinal
//                           nws + nwb: the lane with obstacle slot 0 adds its pair at the lower bound of clr_sphere_grid before the
//                           butterfly, as k_clearance does, and avd_entry takes the normal of the cube gridnear_cube chooses;
//                        6. (before 4, its result feeds MODE_GRAD) the overall minimum of the table under clr_before with
//                           k_clearance's ordinals: the same values under the same total order, so the same bits as k_clearance;
//                        4. the entries under d_influence are compacted with a ballot and a prefix count into a list; the lane that
//                           owns an entry writes n, r = kappa max(d - d_safe, 0) / dt, the two spheres and m (the population count of
//                           the ancestor row, or of the exclusive or of two rows);
//                        5. a lane per DoF (striding past 64) takes its joint's world axis and origin from the placements, walks the
//                           list, forms g = n . (lin + ang x (c - o)) for the entries whose path holds it (ancestor-table bits: on
//                           both paths of a self pair is exactly 0), folds A_lo / A_hi in registers, clamps into the step's interval
//                           and stores.
//                      MODE_GRAD: the list is the witness pair alone, the store its gradient row with k_clearance's outputs.
//                      MODE_QUERY: the box of a shared [lb, ub] into plain arrays, with the table (loikb_avoid_box).
//                      MODE_STEP: the interval k_pose_limit_box / k_pose_dyn_box left in JP_LBUB of the home tiles (or the base box when
//                      neither ran) is narrowed in place for the running instances, rounded toward zero in an fp32 handle; the flags,
//                      the count of narrowed steps and the least clearance seen are kept per instance.
//                      No trip count depends on q but the length of the compacted list.  HBM = true: the placements of every device
//                      joint come from a handle-owned buffer, written by k_avoid_placements with the rounding of the LDS stages: the
//                      centres, and with them the minima and the witness, have the bits of k_clearance<false>.  (A model so large that
//                      k_clearance takes its own placements from k_link_placements -- more than about 600 joints and carriers together --
//                      gets k_link_placements' rounding of the translations there, and the two minima may differ in the last bits.)
//   k_avoid_placements : oMi of every device joint with the rounding of the LDS stages
//   k_avoid_reset    : the result buffers of a pose loop that runs with the latch
//
// fp64 whatever the handle's precision, as loik_pose.hpp.
#pragma once

#include "loik_pose_gridnear.hpp"

namespace loikb {

enum : int { AVD_GRAD = 0, AVD_QUERY = 1, AVD_STEP = 2 };
constexpr int AVD_MAX_SPHERES = 256;   // LOIKB_AVOID_MAX_SPHERES
constexpr int AVD_ENTRY = 5;           // doubles of a list entry: n [3], r, (a | b << 16, m) as two ints
constexpr unsigned int AVD_NO_SPHERE = 0xffffu;

__host__ __device__ inline int avd_anc_words(int nb) { return (nb + 31) >> 5; }

// LDS doubles of one wavefront: centres [ns][4], tv [ns][2], list [2 ns][AVD_ENTRY], then (ints) to [ns][2], sj [ns], anc [nb][W];
// without HBM placements also liM [nb][12] and oMi [nb][12] of every device joint.  ns = 256, nb = 64: 6 080 doubles, 47.5 KB
__host__ __device__ inline size_t avd_wave_doubles(int nb, int ns, bool hbm)
{
  return (size_t)(4 + 2 + 2 * AVD_ENTRY + 1) * ns + (size_t)(ns + 1) / 2 + ((size_t)nb * avd_anc_words(nb) + 1) / 2 + (hbm ? (size_t)0 : (size_t)24 * nb);
}

struct AvoidPrm {
  double d_safe, d_inf, kappa, dt;
};

// where a mode reads and writes (device pointers; the members of the other modes are not touched)
struct AvoidIO {
  // AVD_GRAD
  double* out_min;          // [n][3]
  int* out_wit;             // [n][3]
  double* out_grad;         // [n][nb]
  // AVD_QUERY
  const double *lb, *ub;    // [nb] shared
  double *out_lo, *out_hi;  // [n][nb]
  double* out_pairs;        // [n][ns][2]
  int* out_partner;         // [n][ns][2]
  // AVD_STEP (n = B)
  const int* status;        // [B]
  const void* base_sh;      // lb [nb], ub [nb] of the uniform buffer (T), or nullptr
  const double2* base_pi;   // [nb][B] the per-instance base box
  int from_tiles;           // k_pose_limit_box / k_pose_dyn_box wrote JP_LBUB this step: that is the interval
  char* tiles;
  Layout L;
  double* min_seen;         // [B]
  int* asteps;              // [B]
  int* aflags;              // [B][nb]
};

template <typename T> __device__ __forceinline__ T avd_round_in(double x);
template <> __device__ __forceinline__ double avd_round_in<double>(double x) { return x; }
template <> __device__ __forceinline__ float avd_round_in<float>(double x) { return __double2float_rz(x); }

// the ancestor-table row of device joint dj (0: the universe, no row) has bit j
__device__ __forceinline__ bool avd_on_path(const unsigned int* anc, int W, int dj, int j)
{
  return dj > 0 && ((anc[(size_t)(dj - 1) * W + (j >> 5)] >> (j & 31)) & 1u);
}

// One list entry at `e`: the pair of sphere a with the world object `o` (world spheres first, then boxes, then -- o = nws + nwb, which only
// a handle that latched the nearest-voxel transform can hold -- the voxel grid), or with the second sphere of self pair `o`, at clearance d
__device__ __forceinline__ void avd_entry(double* e, const double* cen, const int* sj, const unsigned int* anc, int W, const ClrModel& m, int a,
                                          bool self, unsigned int o, double d, const AvoidPrm& prm)
{
  const double* c = cen + 4 * a;
  double n0 = 0.0, n1 = 0.0, n2 = 0.0;
  unsigned int bs = AVD_NO_SPHERE;
  if (self || o < (unsigned int)m.nws) {
    const double* w;
    if (self) { bs = m.pairs[2 * (size_t)o + 1]; w = cen + 4 * bs; }
    else w = m.wsph + (size_t)4 * o;
    const double e0 = c[0] - w[0], e1 = c[1] - w[1], e2 = c[2] - w[2];
    const double len = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    if (len != 0.0) { n0 = e0 / len; n1 = e1 / len; n2 = e2 / len; }
  } else if (o >= (unsigned int)(m.nws + m.nwb)) {   // the grid: the normal of the cube chosen among the features around the centre
    GridNearPair gn;
    gridnear_cube(c[0], c[1], c[2], m.g, gn);
    n0 = gn.n[0]; n1 = gn.n[1]; n2 = gn.n[2];
  } else {
    const double* __restrict__ Wb = m.wbox + (size_t)15 * (o - (unsigned int)m.nws);
    const double e0 = c[0] - Wb[9], e1 = c[1] - Wb[10], e2 = c[2] - Wb[11];
    const double p0 = Wb[0] * e0 + Wb[3] * e1 + Wb[6] * e2, p1 = Wb[1] * e0 + Wb[4] * e1 + Wb[7] * e2, p2 = Wb[2] * e0 + Wb[5] * e1 + Wb[8] * e2;
    const double d0 = fabs(p0) - Wb[12], d1 = fabs(p1) - Wb[13], d2 = fabs(p2) - Wb[14];
    const double s0 = p0 >= 0.0 ? 1.0 : -1.0, s1 = p1 >= 0.0 ? 1.0 : -1.0, s2 = p2 >= 0.0 ? 1.0 : -1.0;
    double v0, v1, v2;
    if (d0 > 0.0 || d1 > 0.0 || d2 > 0.0) {
      const double o0 = fmax(d0, 0.0), o1 = fmax(d1, 0.0), o2 = fmax(d2, 0.0);
      const double len = sqrt(o0 * o0 + o1 * o1 + o2 * o2);
      v0 = s0 * o0 / len; v1 = s1 * o1 / len; v2 = s2 * o2 / len;
    } else {   // inside: the face of the largest d, the lowest index on a tie
      const int k = (d0 >= d1 && d0 >= d2) ? 0 : (d1 >= d2 ? 1 : 2);
      v0 = k == 0 ? s0 : 0.0; v1 = k == 1 ? s1 : 0.0; v2 = k == 2 ? s2 : 0.0;
    }
    n0 = Wb[0] * v0 + Wb[1] * v1 + Wb[2] * v2;
    n1 = Wb[3] * v0 + Wb[4] * v1 + Wb[5] * v2;
    n2 = Wb[6] * v0 + Wb[7] * v1 + Wb[8] * v2;
  }
  // m: the DoFs on the root path of a's joint, or on exactly one of the two paths
  const int ja = sj[a], jb = bs != AVD_NO_SPHERE ? sj[bs] : 0;
  int cnt = 0;
  for (int w = 0; w < W; ++w) {
    const unsigned int ra = ja > 0 ? anc[(size_t)(ja - 1) * W + w] : 0u, rb = jb > 0 ? anc[(size_t)(jb - 1) * W + w] : 0u;
    cnt += __popc(ra ^ rb);
  }
  e[0] = n0; e[1] = n1; e[2] = n2;
  e[3] = prm.kappa * fmax(d - prm.d_safe, 0.0) / prm.dt;
  int* ei = reinterpret_cast<int*>(e + 4);
  ei[0] = (int)((unsigned int)a | (bs << 16));
  ei[1] = cnt;
}

// place [n][nb][12]: HBM only
template <bool HBM, int MODE, typename T>
__global__ void __launch_bounds__(64 * CLR_WAVES)
k_avoid_box(const double* __restrict__ q, int nq, const JointDesc* __restrict__ jd, const int* __restrict__ idx_q, int nb, int n, ClrModel m,
            const double* __restrict__ place, AvoidPrm prm, AvoidIO io)
{
  extern __shared__ __attribute__((aligned(16))) double avd_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;   // (the host launches CLR_WAVES or fewer)
  long long idx = (long long)blockIdx.x * waves + wave;
  const bool live = idx < n;
  if (!live) idx = n - 1;   // a wavefront past the end walks the last configuration and stores nothing: every wavefront meets every barrier
  const int b = __builtin_amdgcn_readfirstlane((int)idx);
  const int ns = m.ns, W = avd_anc_words(nb);
  double* cen = avd_lds + (size_t)wave * avd_wave_doubles(nb, ns, HBM);
  double* tv = cen + (size_t)4 * ns;
  double* list = tv + (size_t)2 * ns;
  unsigned int* to = reinterpret_cast<unsigned int*>(list + (size_t)2 * AVD_ENTRY * ns);
  int* sj = reinterpret_cast<int*>(to + (size_t)2 * ns);
  unsigned int* anc = reinterpret_cast<unsigned int*>(sj + (size_t)((ns + 1) & ~1));
  const double* q_row = q + (size_t)b * nq;
  bool fin = true;
  for (int k = lane; k < nq; k += 64) fin &= (bool)isfinite(q_row[k]);
  const bool finite = __ballot(!fin) == 0ull;

  const double* wp;   // oMi [nb][12] of every device joint
  if constexpr (!HBM) {
    double* xf = reinterpret_cast<double*>(anc + (((size_t)nb * W + 1) & ~(size_t)1));
    double* wpl = xf + (size_t)12 * nb;
    for (int k = lane; k < nb; k += 64) {   // liM of every joint
      const JointDesc& d = jd[k + 1];
      double p[8] = {0, 0, 0, 0, 0, 0, 0, 0}, R[9], t[3];
      if (!(d.flags & JF_NOQ)) (void)joint_q_pairs(q_row + idx_q[k + 1], d, p);
      pose_joint_xform(d, p, R, t);
      double* o = xf + (size_t)12 * k;
      for (int c = 0; c < 9; ++c) o[c] = R[c];
      for (int c = 0; c < 3; ++c) o[9 + c] = t[c];
    }
    __syncthreads();
    for (int k = lane; k < nb; k += 64) {   // oMi of every joint, composed leaf side first, and its ancestor row
      double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
      unsigned int* row = anc + (size_t)k * W;
      for (int w = 0; w < W; ++w) row[w] = 0u;
      for (int j = k + 1; j > 0; j = jd[j].parent) {
        const double* x = xf + (size_t)12 * (j - 1);
        xform_premul(x, x + 9, R, t);
        row[(j - 1) >> 5] |= 1u << ((j - 1) & 31);
      }
      double* o = wpl + (size_t)12 * k;
      for (int c = 0; c < 9; ++c) o[c] = R[c];
      for (int c = 0; c < 3; ++c) o[9 + c] = t[c];
    }
    wp = wpl;
  } else {
    for (int k = lane; k < nb; k += 64) {
      unsigned int* row = anc + (size_t)k * W;
      for (int w = 0; w < W; ++w) row[w] = 0u;
      for (int j = k + 1; j > 0; j = jd[j].parent) row[(j - 1) >> 5] |= 1u << ((j - 1) & 31);
    }
    wp = place + (size_t)b * nb * 12;
  }
  __syncthreads();
  for (int s = lane; s < ns; s += 64) {
    const int dj = m.car[m.scar[s]];
    sj[s] = dj;
    double P[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    if (dj > 0)
      for (int c = 0; c < 12; ++c) P[c] = wp[(size_t)12 * (dj - 1) + c];
    clr_centre(P, m.sph + (size_t)4 * s, cen + (size_t)4 * s);
  }
  __syncthreads();

  const double inf = __longlong_as_double(0x7ff0000000000000ll), nan = __longlong_as_double(0x7ff8000000000000ll);
  // 3. the world, a sphere slot at a time: P = 2^lp sphere slots times 64 / P obstacle slots as in k_clearance; every lane walks every
  // trip (a slot past the end repeats the last sphere and stores nothing), so the butterfly across the obstacle slots is whole
  const int lp = m.lp, P = 1 << lp, S = 64 >> lp;
  for (int a0 = 0; a0 < ns; a0 += P) {
    const int ar = a0 + (lane & (P - 1));
    const int a = ar < ns ? ar : ns - 1;
    const double c[4] = {cen[4 * a], cen[4 * a + 1], cen[4 * a + 2], cen[4 * a + 3]};
    double bv = inf;
    unsigned int bo = CLR_NO_ORDINAL;
    for (int o = lane >> lp; o < m.nws; o += S) {
      const double* Ws = m.wsph + (size_t)4 * o;
      const double e0 = c[0] - Ws[0], e1 = c[1] - Ws[1], e2 = c[2] - Ws[2];
      const double v = sqrt(e0 * e0 + e1 * e1 + e2 * e2) - c[3] - Ws[3];
      if (clr_before(v, (unsigned int)o, bv, bo)) { bv = v; bo = (unsigned int)o; }
    }
    for (int o = lane >> lp; o < m.nwb; o += S) {
      const double v = clr_sphere_box(c, m.wbox + (size_t)15 * o);
      const unsigned int ord = (unsigned int)(m.nws + o);
      if (clr_before(v, ord, bv, bo)) { bv = v; bo = ord; }
    }
    if (m.g.F && (lane >> lp) == 0) {   // (wavefront-uniform: a handle that latched the nearest-voxel transform, with a grid set)
      const double v = clr_sphere_grid(c[0], c[1], c[2], c[3], m.g).v;
      const unsigned int ord = (unsigned int)(m.nws + m.nwb);
      if (clr_before(v, ord, bv, bo)) { bv = v; bo = ord; }
    }
    for (int off = P; off < 64; off <<= 1) {
      const double ov = __shfl_xor(bv, off);
      const unsigned int oo = (unsigned int)__shfl_xor((int)bo, off);
      if (clr_before(ov, oo, bv, bo)) { bv = ov; bo = oo; }
    }
    if (ar < ns && (lane >> lp) == 0) { tv[2 * a] = bv; to[2 * a] = bo; }
  }
  // ... and the self pairs whose first index is a: [i0, i1) of the sorted list
  for (int a = lane; a < ns; a += 64) {
    int i0 = 0, i1 = 0;
    for (int side = 0; side < 2; ++side) {
      int lo = 0, hi = m.npairs;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int)m.pairs[2 * (size_t)mid] < a + side) lo = mid + 1; else hi = mid;
      }
      if (side == 0) i0 = lo; else i1 = lo;
    }
    const double* c = cen + (size_t)4 * a;
    double bv = inf;
    unsigned int bo = CLR_NO_ORDINAL;
    for (int i = i0; i < i1; ++i) {
      const double* d = cen + (size_t)4 * m.pairs[2 * (size_t)i + 1];
      const double e0 = c[0] - d[0], e1 = c[1] - d[1], e2 = c[2] - d[2];
      const double v = sqrt(e0 * e0 + e1 * e1 + e2 * e2) - c[3] - d[3];
      if (clr_before(v, (unsigned int)i, bv, bo)) { bv = v; bo = (unsigned int)i; }
    }
    tv[2 * a + 1] = bv; to[2 * a + 1] = bo;
  }
  __syncthreads();

  // 6. the overall minimum with k_clearance's ordinals
  const unsigned int nps = (unsigned int)ns * (unsigned int)m.nws, npb = (unsigned int)ns * (unsigned int)m.nwb;
  const unsigned int npg = m.g.F ? (unsigned int)ns : 0u, nwo = (unsigned int)(m.nws + m.nwb);   // the grid pairs, grid0() + a of ClrOrdinals
  double best = inf, mw = inf, msf = inf;
  unsigned int bord = CLR_NO_ORDINAL;
  for (int t = lane; t < 2 * ns; t += 64) {
    const double v = tv[t];
    const unsigned int o = to[t], a = (unsigned int)t >> 1;
    if (o == CLR_NO_ORDINAL) continue;
    unsigned int g;
    if (t & 1) { g = nps + npb + npg + o; msf = v < msf ? v : msf; }
    else {
      g = o < (unsigned int)m.nws ? a * (unsigned int)m.nws + o : (o < nwo ? nps + a * (unsigned int)m.nwb + (o - (unsigned int)m.nws) : nps + npb + a);
      mw = v < mw ? v : mw;
    }
    if (clr_before(v, g, best, bord)) { best = v; bord = g; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(best, off), ow = __shfl_xor(mw, off), os = __shfl_xor(msf, off);
    const unsigned int oo = (unsigned int)__shfl_xor((int)bord, off);
    if (clr_before(ov, oo, best, bord)) { best = ov; bord = oo; }
    mw = ow < mw ? ow : mw;
    msf = os < msf ? os : msf;
  }

  // 4. the list
  int count = 0;
  int kind = CLR_NONE, wa = -1, wb = -1;
  if constexpr (MODE == AVD_GRAD) {
    if (finite && bord != CLR_NO_ORDINAL) {
      unsigned int o;   // the table's ordinal of the witness
      bool self = false;
      if (bord < nps) { kind = CLR_WORLD_SPHERE; wa = (int)(bord / (unsigned int)m.nws); wb = (int)(bord - (unsigned int)wa * (unsigned int)m.nws); o = (unsigned int)wb; }
      else if (bord < nps + npb) {
        const unsigned int r = bord - nps;
        kind = CLR_WORLD_BOX; wa = (int)(r / (unsigned int)m.nwb); wb = (int)(r - (unsigned int)wa * (unsigned int)m.nwb); o = (unsigned int)(m.nws + wb);
      } else if (bord - nps - npb < npg) {
        kind = CLR_WORLD_GRID; wa = (int)(bord - nps - npb); o = nwo;
        const double* cw = cen + (size_t)4 * wa;
        wb = (int)clr_sphere_grid(cw[0], cw[1], cw[2], cw[3], m.g).vox;
      } else {
        o = bord - nps - npb - npg;
        kind = CLR_SELF; wa = m.pairs[2 * (size_t)o]; wb = m.pairs[2 * (size_t)o + 1]; self = true;
      }
      if (lane == 0) avd_entry(list, cen, sj, anc, W, m, wa, self, o, best, prm);
      count = 1;
    }
  } else {
    for (int t0 = 0; t0 < 2 * ns; t0 += 64) {
      const int t = t0 + lane;
      const bool act = finite && t < 2 * ns && tv[t < 2 * ns ? t : 0] < prm.d_inf;
      const unsigned long long bal = __ballot(act);
      if (act) {
        const int at = count + __popcll(bal & ((1ull << lane) - 1ull));
        avd_entry(list + (size_t)AVD_ENTRY * at, cen, sj, anc, W, m, t >> 1, t & 1, to[t], tv[t], prm);
      }
      count += __popcll(bal);
    }
  }
  __syncthreads();

  // 5. a lane per DoF
  bool narrowed = false;
  const bool running = MODE == AVD_STEP ? !(io.status[b] & POSE_IDLE) : true;
  for (int j = lane; j < nb; j += 64) {
    const JointDesc& d = jd[j + 1];
    double sl[3], sa[3];
    joint_motion_vector(d, sl, sa);
    const double* Pj = wp + (size_t)12 * j;
    double al[3], aa[3];
    for (int r = 0; r < 3; ++r) {
      al[r] = Pj[3 * r] * sl[0] + Pj[3 * r + 1] * sl[1] + Pj[3 * r + 2] * sl[2];
      aa[r] = Pj[3 * r] * sa[0] + Pj[3 * r + 1] * sa[1] + Pj[3 * r + 2] * sa[2];
    }
    const double o0 = Pj[9], o1 = Pj[10], o2 = Pj[11];
    double A_lo = -inf, A_hi = inf, grad = 0.0;
    for (int k = 0; k < count; ++k) {
      const double* e = list + (size_t)AVD_ENTRY * k;
      const int* ei = reinterpret_cast<const int*>(e + 4);
      const unsigned int ab = (unsigned int)ei[0], sa_i = ab & 0xffffu, sb_i = ab >> 16;
      const bool ina = avd_on_path(anc, W, sj[sa_i], j), inb = sb_i != AVD_NO_SPHERE && avd_on_path(anc, W, sj[sb_i], j);
      if (ina == inb) continue;   // on neither path, or on both: exactly 0
      const double* c = cen + (size_t)4 * (ina ? sa_i : sb_i);
      const double u0 = c[0] - o0, u1 = c[1] - o1, u2 = c[2] - o2;
      const double c0 = al[0] + (aa[1] * u2 - aa[2] * u1), c1 = al[1] + (aa[2] * u0 - aa[0] * u2), c2 = al[2] + (aa[0] * u1 - aa[1] * u0);
      double g = e[0] * c0 + e[1] * c1 + e[2] * c2;
      if (inb) g = -g;
      if constexpr (MODE == AVD_GRAD) grad = g;
      else {
        const double mk = (double)ei[1];
        if (g > 0.0) A_lo = fmax(A_lo, -e[3] / (mk * g));
        else if (g < 0.0) A_hi = fmin(A_hi, e[3] / (mk * fabs(g)));
      }
    }
    if (!live) continue;
    if constexpr (MODE == AVD_GRAD) io.out_grad[(size_t)idx * nb + j] = finite ? grad : nan;
    else if constexpr (MODE == AVD_QUERY) {
      const double lo = io.lb[j], hi = io.ub[j];
      io.out_lo[(size_t)idx * nb + j] = fmin(fmax(A_lo, lo), hi);
      io.out_hi[(size_t)idx * nb + j] = fmin(fmax(A_hi, lo), hi);
    } else {
      char* rec = lane_ptr<T>(io.tiles, io.L, b) + (size_t)j * JREC * pair_bytes<T>();
      double lo, hi;
      if (io.from_tiles) { const typename Vec2<T>::type lu = ldp<T>(rec, JP_LBUB); lo = (double)lu.x; hi = (double)lu.y; }
      else if (io.base_sh) { lo = (double)static_cast<const T*>(io.base_sh)[j]; hi = (double)static_cast<const T*>(io.base_sh)[nb + j]; }
      else { const double2 v = io.base_pi[(size_t)j * n + b]; lo = v.x; hi = v.y; }
      if (running) {
        const T nl = avd_round_in<T>(fmin(fmax(A_lo, lo), hi)), nh = avd_round_in<T>(fmin(fmax(A_hi, lo), hi));
        const int f = ((double)nl > lo ? 1 : 0) | ((double)nh < hi ? 2 : 0);
        narrowed |= f != 0;
        io.aflags[(size_t)b * nb + j] = f;
        stp<T>(rec, JP_LBUB, nl, nh);
      } else if (!io.from_tiles) stp<T>(rec, JP_LBUB, (T)lo, (T)hi);
    }
  }

  if constexpr (MODE == AVD_STEP) {
    const bool any = __ballot(narrowed) != 0ull;
    if (lane != 0 || !live || !running) return;
    const double cur = io.min_seen[b];
    io.min_seen[b] = finite ? (best < cur ? best : cur) : nan;
    if (any) io.asteps[b] += 1;
    return;
  }
  if (!live) return;
  if constexpr (MODE == AVD_QUERY) {
    for (int t = lane; t < 2 * ns; t += 64) {
      const unsigned int o = to[t];
      int partner = -1;
      if (finite && o != CLR_NO_ORDINAL) partner = (t & 1) ? (int)m.pairs[2 * (size_t)o + 1] : (int)o;
      io.out_pairs[(size_t)idx * 2 * ns + t] = finite ? tv[t] : nan;
      io.out_partner[(size_t)idx * 2 * ns + t] = partner;
    }
  }
  if constexpr (MODE == AVD_GRAD) {
    if (lane != 0) return;
    double* om = io.out_min + (size_t)idx * 3;
    om[0] = finite ? best : nan;
    om[1] = finite ? mw : nan;
    om[2] = finite ? msf : nan;
    int* ow = io.out_wit + (size_t)idx * 3;
    ow[0] = kind; ow[1] = wa; ow[2] = wb;
  }
}

// out [n][nb][12] = oMi of every device joint, for k_avoid_box<true>: liM by pose_joint_xform and the product by xform_premul, leaf side
// first -- the arithmetic of the LDS stages, hence the same bits, where k_link_placements rounds its translation otherwise
__global__ void k_avoid_placements(const double* __restrict__ q, int nq, const JointDesc* __restrict__ jd, const int* __restrict__ idx_q, int nb, int n,
                                   double* __restrict__ out)
{
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)n * nb) return;
  const int b = (int)(idx / nb), k = (int)(idx - (long long)b * nb);
  const double* q_row = q + (size_t)b * nq;
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
  for (int j = k + 1; j > 0; j = jd[j].parent) {
    const JointDesc& d = jd[j];
    double p[8] = {0, 0, 0, 0, 0, 0, 0, 0}, Rx[9], tx[3];
    if (!(d.flags & JF_NOQ)) (void)joint_q_pairs(q_row + idx_q[j], d, p);
    pose_joint_xform(d, p, Rx, tx);
    xform_premul(Rx, tx, R, t);
  }
  double* o = out + (size_t)idx * 12;
  for (int c = 0; c < 9; ++c) o[c] = R[c];
  for (int c = 0; c < 3; ++c) o[9 + c] = t[c];
}

// min_seen [B] = +inf, asteps [B] = 0, aflags [B][nb] = 0
__global__ void k_avoid_reset(int B, int nb, double* __restrict__ min_seen, int* __restrict__ asteps, int* __restrict__ aflags)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)B) { min_seen[i] = __longlong_as_double(0x7ff0000000000000ll); asteps[i] = 0; }
  if (i < (size_t)B * nb) aflags[i] = 0;
}

}  // namespace loikb
