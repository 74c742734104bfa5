// The distance field of a voxel world (include/loik_amd_grid.h), built on the device.
//
//   G[v] = min over occupied u of g(vx - ux) + g(vy - uy) + g(vz - uz), g(0) = 0, g(d) = (2 |d| - 1)^2, GRID_EMPTY when no voxel is
//   occupied: (h / 2) sqrt(G[v]) is the distance from the centre of v to the union of the closed cubes of the occupied voxels.  The sum
//   is separable, so three min-plus passes compute it, in place in the one [nz][ny][nx] buffer, in integers throughout:
//
//   k_grid_x    : G[x] = min over the occupied u of the x line of g(x - u).  A workgroup takes whole lines (as many as fit 256 voxels; a
//                 line longer than that alone), keeps their occupancy in LDS and gives every voxel a thread that scans its line there:
//                 all lanes of a line read the same byte, a broadcast.
//   k_grid_pass : G[k] = min over u of G[u] + g(k - u) along y (then z).  The lanes lie along x, so that every global access of a
//                 wavefront is one run of consecutive words; a workgroup holds a tile [n][W] of W neighbouring lines in LDS, reads it
//                 once, and every thread scans the column of its lane for its share of the outputs: the lanes of a wavefront read
//                 consecutive LDS words (W = 64), or two broadcast halves (W = 32).  W comes from the axis length (grid_tile_width): a
//                 tile is never more than 64 KB, so at least two workgroups share a CU at the cap of 512 and a short axis keeps many.
//                 The tile is complete in LDS before the first output is written, and no other workgroup touches its lines: in place.
//
// A voxel without an occupied one in reach carries GRID_FAR in LDS, far above every sum and small enough that adding a g cannot wrap.
#pragma once

#include "loik_pose_collision.hpp"

namespace loikb {

constexpr int GRID_MAX_DIM = 512;                  // of one axis
constexpr size_t GRID_MAX_VOXELS = (size_t)1 << 26;
constexpr unsigned int GRID_FAR = 0xf0000000u;     // (the largest G is 3 * 1021^2)
constexpr int GRID_THREADS = 256;

__host__ __device__ inline unsigned int grid_g(int d)
{
  const unsigned int a = (unsigned int)(d < 0 ? -d : d);
  return a == 0 ? 0u : (2u * a - 1u) * (2u * a - 1u);
}

// the lines of one k_grid_x workgroup
__host__ __device__ inline int grid_x_lines(int nx) { return nx >= GRID_THREADS ? 1 : GRID_THREADS / nx; }

// the lines (lanes along x) of one k_grid_pass tile over an axis of n voxels: n * W * 4 bytes <= 64 KB
__host__ __device__ inline int grid_tile_width(int n) { return n > 256 ? 32 : 64; }

// occ [nlines][nx] -> G [nlines][nx]
__global__ void __launch_bounds__(GRID_THREADS) k_grid_x(const unsigned char* __restrict__ occ, unsigned int* __restrict__ G, int nx, long long nlines)
{
  __shared__ unsigned char line_occ[GRID_MAX_DIM];
  const int per = grid_x_lines(nx);
  const long long first = (long long)blockIdx.x * per;
  const int here = (int)(nlines - first < per ? nlines - first : per);   // (the host launches no workgroup past the end: here >= 1)
  const int nvox = here * nx;                                             // <= 512
  const size_t base = (size_t)first * nx;
  for (int i = threadIdx.x; i < nvox; i += GRID_THREADS) line_occ[i] = occ[base + i];
  __syncthreads();
  for (int i = threadIdx.x; i < nvox; i += GRID_THREADS) {
    const int l = i / nx, x = i - l * nx;
    const unsigned char* o = line_occ + l * nx;
    unsigned int best = GRID_EMPTY;
    for (int u = 0; u < nx; ++u) {
      const unsigned int v = grid_g(x - u);
      best = (o[u] != 0 && v < best) ? v : best;
    }
    G[base + i] = best;
  }
}

// One min-plus pass along an axis of n voxels whose neighbours are `stride` words apart.  Workgroup (bx, by): the lines x0 .. x0 + W - 1,
// x0 = bx W, of the slab by: `slab` words from one slab to the next.  blockDim.x == GRID_THREADS; LDS n * W words
__global__ void __launch_bounds__(GRID_THREADS) k_grid_pass(unsigned int* __restrict__ G, int n, int nx, size_t stride, size_t slab, int W)
{
  extern __shared__ unsigned int grid_tile[];
  const int tx = threadIdx.x % W, ty = threadIdx.x / W, R = GRID_THREADS / W;
  const int x = blockIdx.x * W + tx;
  const bool in = x < nx;   // (a partial tile at the end of x: its idle lanes read and write nothing, and meet the barrier)
  unsigned int* col = G + (size_t)blockIdx.y * slab + (size_t)(in ? x : 0);
  for (int k = ty; k < n; k += R) {
    const unsigned int v = in ? col[(size_t)k * stride] : GRID_EMPTY;
    grid_tile[k * W + tx] = v < GRID_FAR ? v : GRID_FAR;
  }
  __syncthreads();
  if (!in) return;
  for (int k = ty; k < n; k += R) {
    unsigned int best = GRID_FAR;
    for (int u = 0; u < n; ++u) {
      const unsigned int v = grid_tile[u * W + tx] + grid_g(k - u);
      best = v < best ? v : best;
    }
    col[(size_t)k * stride] = best < GRID_FAR ? best : GRID_EMPTY;
  }
}

}  // namespace loikb
