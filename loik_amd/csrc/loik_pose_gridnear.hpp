// The nearest-voxel transform of a voxel world and the pair with a direction (include/loik_amd_gridnear.h).
//
//   F[v] = the linear index of the occupied voxel that attains G[v] (loik_pose_grid.hpp), the lowest index among several, GRID_NO_VOXEL
//   when no voxel is occupied.  The passes are those of the field with the key (G << 32) | F in the place of G: adding g << 32 leaves the
//   low word alone, and a 64-bit minimum orders by G first and by the index second, so the three separable passes end at the
//   lexicographic minimum of (G, index) over all occupied voxels.  The occupancy is read back from the finished field (G[v] == 0 exactly
//   at the occupied voxels), so one build serves a grid that is being set and one that was set before the latch.
//
//   k_gridnear_x    : key[x] = min over the occupied u of the x line of (g(x - u) << 32) | index(u); k_grid_x's workgroups and LDS line.
//   k_gridnear_pass : key[k] = min over u of key[u] + (g(k - u) << 32) along y (then z); k_grid_pass's access pattern with a tile [n][W] of
//                     64-bit keys, at most 64 KB, so W is half of that kernel's: 32 lanes along x for an axis of up to 256 voxels, 16
//                     beyond.  A 64-bit LDS read is banked by 32-lane halves over 64 dwords: 32 consecutive keys are one conflict-free
//                     row, and at W = 16 the lanes l and l + 16 of a half read the same key, a broadcast.
//                     The keys live in a transient buffer; the last kernel of a build writes the low words to F instead.
//   k_grid_nearest_query : a lane per sphere, the pair of the header into plain arrays.
//
// gridnear_cube, the choice of the cube and its normal, is also what avd_entry (loik_pose_avoid.hpp) calls for the grid pair of a sphere.
#pragma once

#include "loik_pose_grid.hpp"

namespace loikb {

constexpr unsigned int GRID_NO_VOXEL = 0xffffffffu;
constexpr unsigned long long GRIDNEAR_FAR = ((unsigned long long)GRID_FAR << 32) | GRID_NO_VOXEL;

// the lines (lanes along x) of one k_gridnear_pass tile over an axis of n voxels: n * W * 8 bytes <= 64 KB
__host__ __device__ inline int gridnear_tile_width(int n) { return n > 256 ? 16 : 32; }

// G [nlines][nx] (finished) -> K [nlines][nx], or the low words to F when F is not null
__global__ void __launch_bounds__(GRID_THREADS)
k_gridnear_x(const unsigned int* __restrict__ G, unsigned long long* __restrict__ K, unsigned int* __restrict__ F, int nx, long long nlines)
{
  __shared__ unsigned char line_occ[GRID_MAX_DIM];
  const int per = grid_x_lines(nx);
  const long long first = (long long)blockIdx.x * per;
  const int here = (int)(nlines - first < per ? nlines - first : per);   // (the host launches no workgroup past the end: here >= 1)
  const int nvox = here * nx;                                             // <= 512
  const size_t base = (size_t)first * nx;
  for (int i = threadIdx.x; i < nvox; i += GRID_THREADS) line_occ[i] = G[base + i] == 0u ? 1 : 0;
  __syncthreads();
  for (int i = threadIdx.x; i < nvox; i += GRID_THREADS) {
    const int l = i / nx, x = i - l * nx;
    const unsigned char* o = line_occ + l * nx;
    const unsigned long long lin0 = (unsigned long long)(base + (size_t)l * nx);
    unsigned long long best = GRIDNEAR_FAR;
    for (int u = 0; u < nx; ++u) {
      const unsigned long long v = ((unsigned long long)grid_g(x - u) << 32) | (lin0 + (unsigned long long)u);
      best = (o[u] != 0 && v < best) ? v : best;
    }
    if (F) F[base + i] = (unsigned int)best;
    else K[base + i] = best;
  }
}

// One min-plus pass over the keys, the geometry of k_grid_pass.  blockDim.x == GRID_THREADS; LDS n * W keys.  F not null: the last pass
__global__ void __launch_bounds__(GRID_THREADS)
k_gridnear_pass(unsigned long long* __restrict__ K, unsigned int* __restrict__ F, int n, int nx, size_t stride, size_t slab, int W)
{
  extern __shared__ unsigned long long gridnear_tile[];
  const int tx = threadIdx.x % W, ty = threadIdx.x / W, R = GRID_THREADS / W;
  const int x = blockIdx.x * W + tx;
  const bool in = x < nx;   // (a partial tile at the end of x: its idle lanes read and write nothing, and meet the barrier)
  const size_t col = (size_t)blockIdx.y * slab + (size_t)(in ? x : 0);
  for (int k = ty; k < n; k += R) gridnear_tile[k * W + tx] = in ? K[col + (size_t)k * stride] : GRIDNEAR_FAR;
  __syncthreads();
  if (!in) return;
  for (int k = ty; k < n; k += R) {
    unsigned long long best = GRIDNEAR_FAR;
    for (int u = 0; u < n; ++u) {
      const unsigned long long v = gridnear_tile[u * W + tx] + ((unsigned long long)grid_g(k - u) << 32);
      best = v < best ? v : best;
    }
    if ((unsigned int)(best >> 32) >= GRID_FAR) best = GRIDNEAR_FAR;
    if (F) F[col + (size_t)k * stride] = (unsigned int)best;
    else K[col + (size_t)k * stride] = best;
  }
}

struct GridNearPair {
  double v, du;          // the lower bound of the grid header (less r); the distance of the centre to the chosen cube (NOT less r)
  unsigned int vox, u;   // the voxel read; the chosen cube, GRID_NO_VOXEL with an empty grid
  double n[3];           // the outward normal of the chosen cube at the centre, 0 with an empty grid
};

// The cube of include/loik_amd_gridnear.h for a centre: du, u and n of `out` (v and vox are left alone).  Every index is clamped into the
// grid, whatever c holds, and every feature read is an occupied voxel of the grid or GRID_NO_VOXEL, which is skipped: all reads are in
// bounds.  This is all avd_entry needs: the lower bound of the pair is in its table already
__device__ __forceinline__ void gridnear_cube(double c0, double c1, double c2, const ClrGrid& g, GridNearPair& out)
{
  const double c[3] = {c0, c1, c2};
  int lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double p = fmin(fmax(c[k], g.o[k]), g.hi[k]);
    const int i = (int)fmin(fmax(floor((p - g.o[k]) * g.inv_h), 0.0), (double)(g.n[k] - 1));
    const double x = g.o[k] + ((double)i + 0.5) * g.h;
    const int j = i - (p < x ? 1 : 0);
    lo[k] = j > 0 ? j : 0;
    hi[k] = j + 1 < g.n[k] - 1 ? j + 1 : g.n[k] - 1;
  }
  const double inf = __longlong_as_double(0x7ff0000000000000ll), hh = 0.5 * g.h;
  out.du = inf; out.u = GRID_NO_VOXEL; out.n[0] = out.n[1] = out.n[2] = 0.0;
  double be[3] = {0.0, 0.0, 0.0};
#pragma unroll 1   // (a loop, not eight copies: k_avoid_box keeps its registers and its zero scratch with the search in line)
  for (int s = 0; s < 8; ++s) {
    const int w0 = (s & 1) ? hi[0] : lo[0], w1 = (s & 2) ? hi[1] : lo[1], w2 = (s & 4) ? hi[2] : lo[2];
    const unsigned int u = g.F[((size_t)w2 * g.n[1] + w1) * g.n[0] + w0];
    if (u == GRID_NO_VOXEL) continue;
    const unsigned int ux = u % (unsigned int)g.n[0], uyz = u / (unsigned int)g.n[0];
    const unsigned int uy = uyz % (unsigned int)g.n[1], uz = uyz / (unsigned int)g.n[1];
    const double e0 = c0 - (g.o[0] + ((double)ux + 0.5) * g.h), e1 = c1 - (g.o[1] + ((double)uy + 0.5) * g.h), e2 = c2 - (g.o[2] + ((double)uz + 0.5) * g.h);
    const double o0 = fmax(fabs(e0) - hh, 0.0), o1 = fmax(fabs(e1) - hh, 0.0), o2 = fmax(fabs(e2) - hh, 0.0);
    const double d = sqrt(o0 * o0 + o1 * o1 + o2 * o2);
    if (d < out.du || (d == out.du && u < out.u)) { out.du = d; out.u = u; be[0] = e0; be[1] = e1; be[2] = e2; }
  }
  if (out.u == GRID_NO_VOXEL) return;
  // the world-box normal of loik_amd_avoid.h with R = I
  const double d0 = fabs(be[0]) - hh, d1 = fabs(be[1]) - hh, d2 = fabs(be[2]) - hh;
  const double s0 = be[0] >= 0.0 ? 1.0 : -1.0, s1 = be[1] >= 0.0 ? 1.0 : -1.0, s2 = be[2] >= 0.0 ? 1.0 : -1.0;
  if (d0 > 0.0 || d1 > 0.0 || d2 > 0.0) {
    const double o0 = fmax(d0, 0.0), o1 = fmax(d1, 0.0), o2 = fmax(d2, 0.0);
    const double len = sqrt(o0 * o0 + o1 * o1 + o2 * o2);
    out.n[0] = s0 * o0 / len; out.n[1] = s1 * o1 / len; out.n[2] = s2 * o2 / len;
  } else {   // inside: the face of the largest d, the lowest index on a tie
    const int k = (d0 >= d1 && d0 >= d2) ? 0 : (d1 >= d2 ? 1 : 2);
    out.n[0] = k == 0 ? s0 : 0.0; out.n[1] = k == 1 ? s1 : 0.0; out.n[2] = k == 2 ? s2 : 0.0;
  }
}

// the whole pair: v and vox are clr_sphere_grid's, the same bits
__device__ __forceinline__ GridNearPair gridnear_pair(double c0, double c1, double c2, double r, const ClrGrid& g)
{
  const GridPair gp = clr_sphere_grid(c0, c1, c2, r, g);
  GridNearPair out;
  out.v = gp.v; out.vox = gp.vox;
  gridnear_cube(c0, c1, c2, g, out);
  return out;
}

// sph [n][4] -> val [n][2] = (v, d_u - r), vox [n][2] = (i, u), nrm [n][3]; a row that is not finite: NaN, (-1, -1), NaN
__global__ void k_grid_nearest_query(const double* __restrict__ sph, int n, ClrGrid g, double* __restrict__ val, int* __restrict__ vox, double* __restrict__ nrm)
{
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double c0 = sph[4 * i], c1 = sph[4 * i + 1], c2 = sph[4 * i + 2], r = sph[4 * i + 3];
  if (!(isfinite(c0) && isfinite(c1) && isfinite(c2) && isfinite(r))) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    val[2 * i] = nan; val[2 * i + 1] = nan;
    vox[2 * i] = -1; vox[2 * i + 1] = -1;
    nrm[3 * i] = nan; nrm[3 * i + 1] = nan; nrm[3 * i + 2] = nan;
    return;
  }
  const GridNearPair p = gridnear_pair(c0, c1, c2, r, g);
  val[2 * i] = p.v; val[2 * i + 1] = p.du - r;
  vox[2 * i] = (int)p.vox; vox[2 * i + 1] = (int)p.u;
  nrm[3 * i] = p.n[0]; nrm[3 * i + 1] = p.n[1]; nrm[3 * i + 2] = p.n[2];
}

}  // namespace loikb
