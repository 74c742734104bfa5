// Voxel worlds from depth images and point clouds (include/loik_amd_depth.h): the occupancy of a frame, written on the device.
//
// The occupancy is one byte a voxel, [nz][ny][nx], in a handle-owned buffer; the kernels run in the order below on the handle's stream,
// and the result goes to k_grid_x (loik_pose_grid.hpp).  Every fp64 operation whose rounding decides an index or a comparison is a
// __dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn in the order the header writes it, so that nothing is contracted into an fma and a
// reference can follow the arithmetic (the convention of loik_pose_plan.hpp).
//
//   k_depth_prior_carve : FUSE alone (REPLACE is a memset).  occ[v] = P[v] = (G[v] == 0) of the grid that is set, less the voxels this
//                         frame sees through.  Voxel-centric, the lanes along x: a thread owns DEPTH_RUN = 4 consecutive voxels of the
//                         flattened array, reads their G as one 16-byte word and writes their bytes as one 4-byte word (the buffers
//                         are allocations, so run 4 t is aligned whatever nx is; a run may cross into the next x line, every voxel
//                         takes its own coordinates).  Only the last thread can own a ragged run, nvox not a multiple of 4: it goes
//                         voxel by voxel.  Only the voxels with P = 1 project -- a small share of a world -- and each reads one pixel
//                         of an image that stays in cache.  Counts the voxels of P.  A bounded number of workgroups stride over the grid, so
//                         that the counter takes a bounded number of adds (depth_block_add).
//   k_depth_scatter     : a thread per pixel (or point): the return's voxel, a plain byte store of 1.  Racing writers all store the
//                         same value.  Counts the returns and those inside the grid: reduced in the wavefront, one atomicAdd per workgroup.
//   k_depth_centres     : the world centre and the padded radius of every (filter configuration, sphere), from k_link_placements'
//                         output through clr_centre: the centres k_clearance<true> reads.
//   k_depth_filter      : a wavefront per (configuration, sphere) walks the voxels of the sphere's bounding box, clipped to the grid,
//                         and clears those whose centre lies within the padded radius.  A box wholly outside the grid is empty.
//   k_depth_count       : the occupied voxels of the result, 16 bytes a thread and step.
//   k_depth_occupancy   : G == 0 -> a byte, for the getter; the access pattern of k_depth_prior_carve.
#pragma once

#include "loik_pose_gridnear.hpp"

namespace loikb {

enum : int { DEPTH_F32 = 0, DEPTH_U16 = 1 };
constexpr int DEPTH_RUN = 4;        // voxels of one thread of k_depth_prior_carve / k_depth_occupancy
constexpr int DEPTH_THREADS = 256;
constexpr int DEPTH_MAX_BLOCKS = 2048;   // of the kernels that stride over the voxels: eight workgroups a CU, and as many atomicAdds at most

// the workgroups of a kernel whose threads take `per` voxels a step
__host__ __device__ inline unsigned int depth_blocks(size_t nvox, int per)
{
  const size_t b = (nvox + (size_t)per * DEPTH_THREADS - 1) / ((size_t)per * DEPTH_THREADS);
  return (unsigned int)(b < (size_t)DEPTH_MAX_BLOCKS ? b : (size_t)DEPTH_MAX_BLOCKS);
}

// the camera as the kernels read it
struct DepthCam {
  const void* img;     // [height][width] float or unsigned short
  int type, width, height;
  double fx, fy, cx, cy;
  double R[9], p[3];   // T_world_cam
  double scale, z_min, z_max;
};

// the grid as the kernels of this file read it (ClrGrid's numbers without the field)
struct DepthGrid {
  int n[3];
  double o[3], h, inv_h;
};

// the metric z-depth of pixel i, and whether it is a return
__device__ __forceinline__ bool depth_pixel(const DepthCam& c, size_t i, double* d)
{
  const double raw = c.type == DEPTH_F32 ? (double)static_cast<const float*>(c.img)[i] : (double)static_cast<const unsigned short*>(c.img)[i];
  *d = __dmul_rn(raw, c.scale);
  return isfinite(*d) && *d >= c.z_min && *d <= c.z_max;
}

// the centre of voxel i along axis k: origin + (i + 0.5) h, the product rounded first
__device__ __forceinline__ double depth_voxel_centre(const DepthGrid& g, int k, int i) { return __dadd_rn(g.o[k], __dmul_rn((double)i + 0.5, g.h)); }

// whether this frame sees through the voxel (x, y, z): step 2 of the header
__device__ __forceinline__ bool depth_carves(const DepthCam& c, const DepthGrid& g, double band, int x, int y, int z)
{
  const double e0 = __dsub_rn(depth_voxel_centre(g, 0, x), c.p[0]), e1 = __dsub_rn(depth_voxel_centre(g, 1, y), c.p[1]),
               e2 = __dsub_rn(depth_voxel_centre(g, 2, z), c.p[2]);
  double xc[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) xc[j] = __dadd_rn(__dadd_rn(__dmul_rn(c.R[j], e0), __dmul_rn(c.R[3 + j], e1)), __dmul_rn(c.R[6 + j], e2));
  if (!(xc[2] > 0.0)) return false;
  const double u = floor(__dadd_rn(__dadd_rn(__ddiv_rn(__dmul_rn(c.fx, xc[0]), xc[2]), c.cx), 0.5));
  const double v = floor(__dadd_rn(__dadd_rn(__ddiv_rn(__dmul_rn(c.fy, xc[1]), xc[2]), c.cy), 0.5));
  if (!(u >= 0.0 && u < (double)c.width && v >= 0.0 && v < (double)c.height)) return false;   // (a NaN or an infinity is outside)
  double d;
  if (!depth_pixel(c, (size_t)(int)v * c.width + (size_t)(int)u, &d)) return false;
  return __dadd_rn(xc[2], band) < d;
}

__device__ __forceinline__ unsigned long long depth_wave_sum(unsigned long long v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// *dst += the sum of v over the workgroup (DEPTH_THREADS threads, every one of them calls): reduced in the wavefronts, then across them
// through LDS, then one atomicAdd.  Adds to one address serialise in the L2 at about 10 ns each (profiles/depth_measured.md), so the
// kernels that count launch a bounded number of workgroups and add once per workgroup
__device__ __forceinline__ void depth_block_add(unsigned long long v, unsigned long long* dst)
{
  __shared__ unsigned long long part[DEPTH_THREADS / 64];
  v = depth_wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < DEPTH_THREADS / 64; ++w) t += part[w];
    if (t) atomicAdd(dst, t);
  }
}

// occ [nvox] = (G == 0) less the carve; stats[2] += the voxels with G == 0.  carve = 0: the prior alone (cam is not read)
__global__ void __launch_bounds__(DEPTH_THREADS)
k_depth_prior_carve(const unsigned int* __restrict__ G, unsigned char* __restrict__ occ, size_t nvox, DepthGrid g, DepthCam cam, int carve, double band,
                    unsigned long long* __restrict__ stats)
{
  const size_t step = (size_t)gridDim.x * DEPTH_THREADS * DEPTH_RUN;
  unsigned long long prior = 0;
  for (size_t v0 = ((size_t)blockIdx.x * DEPTH_THREADS + threadIdx.x) * DEPTH_RUN; v0 < nvox; v0 += step) {
    const int here = nvox - v0 < (size_t)DEPTH_RUN ? (int)(nvox - v0) : DEPTH_RUN;
    unsigned int gv[DEPTH_RUN] = {1u, 1u, 1u, 1u};
    if (here == DEPTH_RUN) {
      const uint4 w = *reinterpret_cast<const uint4*>(G + v0);
      gv[0] = w.x; gv[1] = w.y; gv[2] = w.z; gv[3] = w.w;
    } else {
#pragma unroll
      for (int k = 0; k < DEPTH_RUN; ++k)
        if (k < here) gv[k] = G[v0 + k];
    }
    unsigned int bytes = 0;
#pragma unroll
    for (int k = 0; k < DEPTH_RUN; ++k) {
      if (gv[k] != 0u) continue;
      ++prior;
      bool keep = true;
      if (carve) {
        const size_t v = v0 + k, line = v / (size_t)g.n[0];
        const int x = (int)(v - line * (size_t)g.n[0]), z = (int)(line / (size_t)g.n[1]), y = (int)(line - (size_t)z * (size_t)g.n[1]);
        keep = !depth_carves(cam, g, band, x, y, z);
      }
      if (keep) bytes |= 1u << (8 * k);
    }
    if (here == DEPTH_RUN) *reinterpret_cast<unsigned int*>(occ + v0) = bytes;
    else for (int k = 0; k < here; ++k) occ[v0 + k] = (unsigned char)((bytes >> (8 * k)) & 1u);
  }
  depth_block_add(prior, stats + 2);
}

// out [nvox] = (G == 0)
__global__ void __launch_bounds__(DEPTH_THREADS) k_depth_occupancy(const unsigned int* __restrict__ G, unsigned char* __restrict__ out, size_t nvox)
{
  const size_t v0 = ((size_t)blockIdx.x * DEPTH_THREADS + threadIdx.x) * DEPTH_RUN;
  if (v0 >= nvox) return;
  if (nvox - v0 >= (size_t)DEPTH_RUN) {
    const uint4 w = *reinterpret_cast<const uint4*>(G + v0);
    *reinterpret_cast<unsigned int*>(out + v0) = (w.x == 0u ? 1u : 0u) | (w.y == 0u ? 0x100u : 0u) | (w.z == 0u ? 0x10000u : 0u) | (w.w == 0u ? 0x1000000u : 0u);
  } else {
    for (size_t v = v0; v < nvox; ++v) out[v] = G[v] == 0u ? 1 : 0;
  }
}

// the voxel of the world point (x0, x1, x2): true and *lin when it lies in the grid
__device__ __forceinline__ bool depth_voxel_of(const DepthGrid& g, double x0, double x1, double x2, size_t* lin)
{
  const double x[3] = {x0, x1, x2};
  size_t l = 0;
  bool in = true;
#pragma unroll
  for (int k = 2; k >= 0; --k) {
    const double f = floor(__dmul_rn(__dsub_rn(x[k], g.o[k]), g.inv_h));
    const bool ok = f >= 0.0 && f < (double)g.n[k];   // (a NaN is outside)
    in = in && ok;
    l = l * (size_t)g.n[k] + (size_t)(ok ? (int)f : 0);
  }
  *lin = l;
  return in;
}

// n = width * height pixels of cam (points == nullptr), or n world points [n][3].  stats[0] += returns | those in the grid << 32: n is below
// 2^31, so neither half overflows
__global__ void __launch_bounds__(DEPTH_THREADS)
k_depth_scatter(DepthCam cam, const double* __restrict__ points, long long n, DepthGrid g, unsigned char* __restrict__ occ, unsigned long long* __restrict__ stats)
{
  const long long i = (long long)blockIdx.x * DEPTH_THREADS + threadIdx.x;
  bool ret = false, in = false;
  if (i < n) {
    double xw[3];
    if (points) {
      for (int k = 0; k < 3; ++k) xw[k] = points[3 * i + k];
      ret = isfinite(xw[0]) && isfinite(xw[1]) && isfinite(xw[2]);
    } else {
      double d;
      ret = depth_pixel(cam, (size_t)i, &d);
      const int v = (int)(i / cam.width), u = (int)(i - (long long)v * cam.width);
      const double xc[3] = {__dmul_rn(__ddiv_rn(__dsub_rn((double)u, cam.cx), cam.fx), d), __dmul_rn(__ddiv_rn(__dsub_rn((double)v, cam.cy), cam.fy), d), d};
#pragma unroll
      for (int k = 0; k < 3; ++k)
        xw[k] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(cam.R[3 * k], xc[0]), __dmul_rn(cam.R[3 * k + 1], xc[1])), __dmul_rn(cam.R[3 * k + 2], xc[2])), cam.p[k]);
    }
    size_t lin;
    in = ret && depth_voxel_of(g, xw[0], xw[1], xw[2], &lin);
    if (in) occ[lin] = 1;
  }
  depth_block_add((ret ? 1ull : 0ull) | (in ? 1ull << 32 : 0ull), stats);   // (both counters in one word: one add a workgroup)
}

// cen [nf][ns][4] = (the world centre, r + pad) from place [nf][ncar][12], k_link_placements' output
__global__ void k_depth_centres(const double* __restrict__ place, ClrModel m, int nf, double pad, double* __restrict__ cen)
{
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)nf * m.ns) return;
  const int b = (int)(i / m.ns), s = (int)(i - (long long)b * m.ns);
  double o[4];
  clr_centre(place + ((size_t)b * m.ncar + m.scar[s]) * 12, m.sph + (size_t)4 * s, o);
  o[3] = __dadd_rn(o[3], pad);
  for (int k = 0; k < 4; ++k) cen[4 * i + k] = o[k];
}

// a wavefront per row of cen [n][4] = (c, R): occ = 0 at every voxel whose centre lies within R of c
__global__ void __launch_bounds__(DEPTH_THREADS) k_depth_filter(const double* __restrict__ cen, int n, DepthGrid g, unsigned char* __restrict__ occ)
{
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (DEPTH_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= n) return;
  const double c[3] = {cen[4 * row], cen[4 * row + 1], cen[4 * row + 2]}, R = cen[4 * row + 3];
  if (!(isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]))) return;
  // the box, one voxel wider than the sphere's on every side (the rounding of an index can then never cut a voxel off), clipped to the
  // grid in fp64 before anything becomes an integer
  int lo[3], ext[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = fmax(floor((c[k] - R - g.o[k]) * g.inv_h) - 1.0, 0.0), b = fmin(floor((c[k] + R - g.o[k]) * g.inv_h) + 1.0, (double)(g.n[k] - 1));
    if (!(a <= b)) return;   // wholly outside the grid along this axis
    lo[k] = (int)a;
    ext[k] = (int)b - (int)a + 1;
  }
  const double R2 = __dmul_rn(R, R);
  const long long cells = (long long)ext[0] * ext[1] * ext[2];
  for (long long t = lane; t < cells; t += 64) {
    const long long line = t / ext[0];
    const int x = lo[0] + (int)(t - line * ext[0]), z = lo[2] + (int)(line / ext[1]), y = lo[1] + (int)(line - (line / ext[1]) * ext[1]);
    const double d0 = __dsub_rn(depth_voxel_centre(g, 0, x), c[0]), d1 = __dsub_rn(depth_voxel_centre(g, 1, y), c[1]),
                 d2 = __dsub_rn(depth_voxel_centre(g, 2, z), c[2]);
    const double s = __dadd_rn(__dadd_rn(__dmul_rn(d0, d0), __dmul_rn(d1, d1)), __dmul_rn(d2, d2));
    if (s <= R2) occ[((size_t)z * g.n[1] + y) * g.n[0] + x] = 0;
  }
}

// stats[3] += the nonzero bytes of occ [nvox]
__global__ void __launch_bounds__(DEPTH_THREADS) k_depth_count(const unsigned char* __restrict__ occ, size_t nvox, unsigned long long* __restrict__ stats)
{
  const size_t step = (size_t)gridDim.x * DEPTH_THREADS * 16;
  unsigned long long cnt = 0;
  for (size_t v0 = ((size_t)blockIdx.x * DEPTH_THREADS + threadIdx.x) * 16; v0 < nvox; v0 += step) {
    if (nvox - v0 >= 16) {
      const uint4 w = *reinterpret_cast<const uint4*>(occ + v0);
      // (every byte is 0 or 1)
      cnt += __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);
    } else {
      for (size_t v = v0; v < nvox; ++v) cnt += occ[v] != 0;
    }
  }
  depth_block_add(cnt, stats + 3);
}

}  // namespace loikb
