// Collision clearance of sphere models (include/loik_amd_collision.h).
//
//   k_clearance<HBM> : the minimum clearance of one configuration over all (robot sphere, world sphere), (robot sphere, world box),
//                      (robot sphere, voxel grid: include/loik_amd_grid.h) and listed (robot sphere, robot sphere) pairs, with the pair
//                      that achieves it.  One wavefront per configuration,
//                      several configurations per workgroup (the kernel goes by blockDim, as k_frame_jacobians).
//                        1. the lanes build liM_j of every device joint in parallel into LDS (pose_joint_xform: k_link_placements'
//                           arithmetic);
//                        2. a lane per sphere-carrying joint composes its world placement along its root path from those records,
//                           then a lane per sphere writes the world centre and the radius into LDS;
//                        3. the world pairs: the wavefront is 2^lp sphere slots times 64 / 2^lp obstacle slots (2^lp the power of two
//                           that holds min(ns, 64)); a lane reads its sphere from LDS once and walks its share of the world spheres
//                           and boxes with it in registers, so no pair index is divided.  The obstacle records are read from global
//                           memory by every wavefront (they stay in L2).  With a grid set the lane whose obstacle slot is 0 reads
//                           the one voxel of its sphere (clr_sphere_grid).  Then the lanes stride over the self-pair list, two LDS
//                           reads a pair;
//                        4. each lane keeps its best (clearance, ordinal) and its world and self minima; a wave64 butterfly under
//                           the total order (clearance, ordinal) -- a NaN after every number, ties to the lower ordinal, the rule of
//                           k_ms_select -- ends the reduction, lane 0 stores.
//                      No trip count depends on q; a row of q that is not finite ends as NaN minima by a select before the store.
//                      HBM = true is the instantiation for a model whose liM records and carrier placements do not fit one
//                      wavefront's share of 64 KB: steps 1 and 2 are k_link_placements' output in a handle-owned buffer, the LDS holds the
//                      centres alone.
//   k_ms_loop_status : the loop-private status word the re-sampler of a collision-aware multi-start reads: REACHED cleared on the
//                      rows that reached their goal in collision
//
// fp64 whatever the handle's precision, as loik_pose.hpp.
#pragma once

#include "loik_pose_jacobian.hpp"

namespace loikb {

enum : int { CLR_NONE = 0, CLR_WORLD_SPHERE = 1, CLR_WORLD_BOX = 2, CLR_SELF = 3, CLR_WORLD_GRID = 4 };

constexpr int CLR_WAVES = 4;                    // wavefronts = configurations of one workgroup, at most: the host launches fewer when
                                                // their LDS would not fit
constexpr int CLR_MAX_SPHERES = 2048;           // the centres [ns][4] of one wavefront fit 64 KB of LDS
constexpr unsigned int CLR_NO_ORDINAL = 0xffffffffu;

// LDS doubles of one wavefront: the centres [ns][4]; without HBM placements also liM [nb][12] and the carriers' oMi [ncar][12]
__host__ __device__ inline size_t clr_wave_doubles(int nb, int ncar, int ns, bool hbm)
{
  return (size_t)4 * ns + (hbm ? (size_t)0 : (size_t)12 * nb + (size_t)12 * ncar);
}

// the voxel world (include/loik_amd_grid.h) as the kernels read it
struct ClrGrid {
  const unsigned int* G;         // [n[2]][n[1]][n[0]] the field of k_grid_x / k_grid_pass (loik_pose_grid.hpp)
  int n[3];                      // nx, ny, nz
  double o[3], hi[3];            // the low corner of voxel (0, 0, 0); the high corner of the grid's box, o + n h as the host rounded it
  double h, inv_h;               // the edge, 1 / edge as the host rounded it
  const unsigned int* F;         // the nearest-voxel transform (loik_pose_gridnear.hpp), laid out as G; nullptr unless the handle latched it
};

// the model as the kernel reads it (device pointers)
struct ClrModel {
  const double* sph;             // [ns][4] (x, y, z, r) in the frame of the carrier
  const int* scar;               // [ns] the carrier of each sphere: an index into car
  const int* car;                // [ncar] the distinct device joints that carry spheres (0: the universe)
  const double* wsph;            // [nws][4]
  const double* wbox;            // [nwb][15] R row-major, p, h
  const unsigned short* pairs;   // [npairs][2] sphere indices a < b
  int ns, ncar, nws, nwb, npairs;
  int lp;                        // log2 of the sphere slots of a wavefront in the world-pair loops: the least with 2^lp >= min(ns, 64)
  ClrGrid g;                     // the voxel world; g.G == nullptr when no grid is set
};

constexpr unsigned int GRID_EMPTY = 0xffffffffu;   // G of every voxel of a grid without an occupied one

// (v, o) before (bv, bo) in (clearance, ordinal), a NaN after every number
__device__ __forceinline__ bool clr_before(double v, unsigned int o, double bv, unsigned int bo)
{
  const bool an = v != v, bn = bv != bv;
  if (an != bn) return bn;
  if (!an && v != bv) return v < bv;
  return o < bo;
}

// o[0..3] = (R c + t, r): P = (R row-major, t) the carrier's world placement, c = (x, y, z, r)
__device__ __forceinline__ void clr_centre(const double* P, const double* __restrict__ c, double* o)
{
  for (int r = 0; r < 3; ++r) o[r] = P[9 + r] + (P[3 * r] * c[0] + P[3 * r + 1] * c[1] + P[3 * r + 2] * c[2]);
  o[3] = c[3];
}

// sphere (centre c, radius c[3]) against the oriented box W = (R, t, h): the signed distance of the centre, less the radius
__device__ __forceinline__ double clr_sphere_box(const double* c, const double* __restrict__ W)
{
  const double e0 = c[0] - W[9], e1 = c[1] - W[10], e2 = c[2] - W[11];
  const double d0 = fabs(W[0] * e0 + W[3] * e1 + W[6] * e2) - W[12];
  const double d1 = fabs(W[1] * e0 + W[4] * e1 + W[7] * e2) - W[13];
  const double d2 = fabs(W[2] * e0 + W[5] * e1 + W[8] * e2) - W[14];
  const double o0 = fmax(d0, 0.0), o1 = fmax(d1, 0.0), o2 = fmax(d2, 0.0);
  return sqrt(o0 * o0 + o1 * o1 + o2 * o2) + fmin(fmax(d0, fmax(d1, d2)), 0.0) - c[3];
}

struct GridPair {
  double v;
  unsigned int vox;
};

// the pair of include/loik_amd_grid.h: sphere (centre c, radius c[3]) against the grid.  vox = the linear index of the voxel read: the one
// that holds the centre clamped into the grid's box.  Always a voxel of the grid, whatever c holds (fmax and fmin drop a NaN): the read
// is in bounds
__device__ __forceinline__ GridPair clr_sphere_grid(double c0, double c1, double c2, double r, const ClrGrid& g)
{
  const double c[3] = {c0, c1, c2};
  double e2 = 0.0, o2 = 0.0;
  unsigned int lin = 0;
#pragma unroll
  for (int k = 2; k >= 0; --k) {
    const double p = fmin(fmax(c[k], g.o[k]), g.hi[k]);
    const int i = (int)fmin(fmax(floor((p - g.o[k]) * g.inv_h), 0.0), (double)(g.n[k] - 1));
    const double x = g.o[k] + ((double)i + 0.5) * g.h;
    e2 += (p - x) * (p - x);
    o2 += (c[k] - p) * (c[k] - p);
    lin = lin * (unsigned int)g.n[k] + (unsigned int)i;
  }
  const unsigned int gv = g.G[lin];
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const double mc = gv == GRID_EMPTY ? inf : (0.5 * g.h) * sqrt((double)gv) - sqrt(e2);
  const double dout = sqrt(o2), mp = fmax(mc, 0.0);
  return GridPair{(dout > 0.0 ? sqrt(dout * dout + mp * mp) : mc) - r, lin};
}

// clr_sphere_grid behind a call, for the one kernel whose register allocation the compiler does not survive with the pair in line
// (k_shortcut_paths<false>, at 254 VGPRs before the grid existed).  The same arithmetic, hence the same bits
__device__ __noinline__ GridPair clr_sphere_grid_call(double c0, double c1, double c2, double r, const ClrGrid& g) { return clr_sphere_grid(c0, c1, c2, r, g); }

// the pairs in ordinal order: ns * nws world-sphere pairs, ns * nwb world-box pairs, ns grid pairs when a grid is set, npairs self pairs
struct ClrOrdinals {
  unsigned int nps, npb, npg;
  __device__ __forceinline__ explicit ClrOrdinals(const ClrModel& m)
      : nps((unsigned int)m.ns * (unsigned int)m.nws), npb((unsigned int)m.ns * (unsigned int)m.nwb), npg(m.g.G ? (unsigned int)m.ns : 0u) {}
  __device__ __forceinline__ unsigned int grid0() const { return nps + npb; }
  __device__ __forceinline__ unsigned int self0() const { return nps + npb + npg; }
  __device__ __forceinline__ bool is_grid(unsigned int ord) const { return ord - grid0() < npg; }
};

// the voxel that a grid pair's value was read from: cen [ns][4] the centres of the sample the ordinal belongs to; -1 for every other pair
__device__ __forceinline__ int clr_grid_voxel(unsigned int ord, const ClrOrdinals& n, const ClrModel& m, const double* cen)
{
  if (!n.is_grid(ord)) return -1;
  const double* c = cen + (size_t)4 * (ord - n.grid0());
  return (int)clr_sphere_grid(c[0], c[1], c[2], c[3], m.g).vox;
}

// w[0..2] = (kind, a, b) of the pair with ordinal ord, { CLR_NONE, -1, -1 } for CLR_NO_ORDINAL; vox: clr_grid_voxel of the pair
__device__ __forceinline__ void clr_witness(unsigned int ord, int vox, const ClrOrdinals& n, const ClrModel& m, int* w)
{
  int kind = CLR_NONE, wa = -1, wb = -1;
  if (ord != CLR_NO_ORDINAL) {
    if (ord < n.nps) { kind = CLR_WORLD_SPHERE; wa = (int)(ord / (unsigned int)m.nws); wb = (int)(ord - (unsigned int)wa * (unsigned int)m.nws); }
    else if (ord < n.grid0()) {
      const unsigned int r = ord - n.nps;
      kind = CLR_WORLD_BOX; wa = (int)(r / (unsigned int)m.nwb); wb = (int)(r - (unsigned int)wa * (unsigned int)m.nwb);
    } else if (ord < n.self0()) {
      kind = CLR_WORLD_GRID; wa = (int)(ord - n.grid0()); wb = vox;
    } else {
      const size_t r = ord - n.self0();
      kind = CLR_SELF; wa = m.pairs[2 * r]; wb = m.pairs[2 * r + 1];
    }
  }
  w[0] = kind; w[1] = wa; w[2] = wb;
}

// out_min [n][3] = (min, min_world, min_self); out_wit [n][3] = (kind, a, b) or nullptr.  place [n][ncar][12]: HBM only
template <bool HBM>
__global__ void __launch_bounds__(64 * CLR_WAVES)
k_clearance(const double* __restrict__ q, int nq, const JointDesc* __restrict__ jd, const int* __restrict__ idx_q, int nb, int n, ClrModel m,
            const double* __restrict__ place, double* __restrict__ out_min, int* __restrict__ out_wit)
{
  extern __shared__ __attribute__((aligned(16))) double clr_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;   // (the host launches CLR_WAVES or fewer)
  long long idx = (long long)blockIdx.x * waves + wave;
  const bool live = idx < n;
  if (!live) idx = n - 1;   // a wavefront past the end walks the last configuration and stores nothing: every wavefront meets every barrier
  const int b = __builtin_amdgcn_readfirstlane((int)idx);
  double* cen = clr_lds + (size_t)wave * clr_wave_doubles(nb, m.ncar, m.ns, HBM);
  const double* q_row = q + (size_t)b * nq;
  bool fin = true;
  for (int k = lane; k < nq; k += 64) fin &= (bool)isfinite(q_row[k]);
  const bool finite = __ballot(!fin) == 0ull;

  if constexpr (!HBM) {
    double* xf = cen + (size_t)4 * m.ns;
    double* cp = xf + (size_t)12 * nb;
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
    for (int c = lane; c < m.ncar; c += 64) {   // oMi of the carriers, composed leaf side first as link_placement does
      double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
      for (int j = m.car[c]; j > 0; j = jd[j].parent) {
        const double* x = xf + (size_t)12 * (j - 1);
        xform_premul(x, x + 9, R, t);
      }
      double* o = cp + (size_t)12 * c;
      for (int k = 0; k < 9; ++k) o[k] = R[k];
      for (int k = 0; k < 3; ++k) o[9 + k] = t[k];
    }
    __syncthreads();
    for (int s = lane; s < m.ns; s += 64) clr_centre(cp + (size_t)12 * m.scar[s], m.sph + (size_t)4 * s, cen + (size_t)4 * s);
  } else {
    const double* pl = place + (size_t)b * m.ncar * 12;
    for (int s = lane; s < m.ns; s += 64) clr_centre(pl + (size_t)12 * m.scar[s], m.sph + (size_t)4 * s, cen + (size_t)4 * s);
  }
  __syncthreads();

  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  double best = inf, mw = inf, msf = inf;
  unsigned int bord = CLR_NO_ORDINAL;
  const ClrOrdinals no(m);
  const unsigned int nps = no.nps, self0 = no.self0();
  // world pairs: the wavefront is P = 2^lp sphere slots (the power of two that holds min(ns, 64)) times 64 / P obstacle slots, so a
  // lane keeps its sphere in registers while it walks its share of the obstacles, and no index needs a division
  const int lp = m.lp, P = 1 << lp, S = 64 >> lp;
  for (int a = lane & (P - 1); a < m.ns; a += P) {
    const double c[4] = {cen[4 * a], cen[4 * a + 1], cen[4 * a + 2], cen[4 * a + 3]};
    for (int o = lane >> lp; o < m.nws; o += S) {
      const double* W = m.wsph + (size_t)4 * o;
      const double e0 = c[0] - W[0], e1 = c[1] - W[1], e2 = c[2] - W[2];
      const double v = sqrt(e0 * e0 + e1 * e1 + e2 * e2) - c[3] - W[3];
      const unsigned int ord = (unsigned int)a * (unsigned int)m.nws + (unsigned int)o;
      mw = v < mw ? v : mw;
      if (clr_before(v, ord, best, bord)) { best = v; bord = ord; }
    }
    for (int o = lane >> lp; o < m.nwb; o += S) {
      const double v = clr_sphere_box(c, m.wbox + (size_t)15 * o);
      const unsigned int ord = nps + (unsigned int)a * (unsigned int)m.nwb + (unsigned int)o;
      mw = v < mw ? v : mw;
      if (clr_before(v, ord, best, bord)) { best = v; bord = ord; }
    }
    if (m.g.G && (lane >> lp) == 0) {
      const double v = clr_sphere_grid(c[0], c[1], c[2], c[3], m.g).v;
      const unsigned int ord = no.grid0() + (unsigned int)a;
      mw = v < mw ? v : mw;
      if (clr_before(v, ord, best, bord)) { best = v; bord = ord; }
    }
  }
  for (unsigned int i = lane; i < (unsigned int)m.npairs; i += 64) {
    const double* c = cen + (size_t)4 * m.pairs[2 * (size_t)i];
    const double* d = cen + (size_t)4 * m.pairs[2 * (size_t)i + 1];
    const double e0 = c[0] - d[0], e1 = c[1] - d[1], e2 = c[2] - d[2];
    const double v = sqrt(e0 * e0 + e1 * e1 + e2 * e2) - c[3] - d[3];
    msf = v < msf ? v : msf;
    if (clr_before(v, self0 + i, best, bord)) { best = v; bord = self0 + i; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(best, off), ow = __shfl_xor(mw, off), os = __shfl_xor(msf, off);
    const unsigned int oo = (unsigned int)__shfl_xor((int)bord, off);
    if (clr_before(ov, oo, best, bord)) { best = ov; bord = oo; }
    mw = ow < mw ? ow : mw;
    msf = os < msf ? os : msf;
  }
  if (lane != 0 || !live) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double* om = out_min + (size_t)idx * 3;
  om[0] = finite ? best : nan;
  om[1] = finite ? mw : nan;
  om[2] = finite ? msf : nan;
  if (!out_wit) return;
  if (!finite) bord = CLR_NO_ORDINAL;
  clr_witness(bord, clr_grid_voxel(bord, no, m, cen), no, m, out_wit + (size_t)idx * 3);
}

// lstatus[b] = status[b], less POSE_REACHED where the instance reached its goal in collision (class 0c of loik_amd_collision.h).
// clr [B][3]: k_clearance's minima, entry 0 is read
__global__ void k_ms_loop_status(const int* __restrict__ status, const double* __restrict__ clr, double margin, int B, int* __restrict__ lstatus)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int st = status[b];
  const bool colliding = (st & POSE_REACHED) && !(st & POSE_STOPPED) && !(clr[(size_t)3 * b] >= margin);
  lstatus[b] = colliding ? (st & ~POSE_REACHED) : st;
}

}  // namespace loikb
