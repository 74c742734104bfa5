/*
 * loik_amd_grid.h -- voxel worlds: an occupancy grid as a world object, its distance field built and read on the device
 * (libloik_amd.so).
 *
 * loikb_collision_set_world (loik_amd_collision.h) takes the world as a list of spheres and oriented boxes, and every clearance
 * evaluation costs one pair per robot sphere and object.  This header takes the world a sensor delivers: an occupancy grid.  The
 * device turns it into an exact distance field once per set; after that every robot sphere reads one voxel per evaluation, however
 * cluttered the world is.  The grid is one more kind of world object beside the spheres and the boxes: loikb_clearance, the
 * collision-aware multi-start, loikb_motion_clearance(_path), loikb_shortcut_paths, loikb_plan_paths and loikb_blend_paths read it,
 * and what they certify stays what their headers say (below).  A handle that never sets a grid computes what it computed before this
 * header existed, bit for bit; so does one that set a grid and cleared it.
 *
 * The grid.  dims = { nx, ny, nz }, each 1 .. LOIKB_GRID_MAX_DIM, nx ny nz <= LOIKB_GRID_MAX_VOXELS.  origin[3] (finite) is the world
 * position of the low corner of voxel (0, 0, 0); h (finite, > 0) is the edge of a voxel.  The grid is axis-aligned in the world frame
 * and shared by every instance.  occ is uint8 [nz][ny][nx], nonzero = occupied: a host pointer, or a device pointer with
 * LOIKB_IN_DEVICE.  The obstacle O is the union of the closed cubes of the occupied voxels.
 *
 * The field.  For every voxel v, G[v] is an unsigned 32-bit integer:
 *
 *   G[v] = min over the occupied u of g(vx - ux) + g(vy - uy) + g(vz - uz),   g(0) = 0, g(d) = (2 |d| - 1)^2,
 *   G[v] = LOIKB_GRID_EMPTY when no voxel is occupied.
 *
 * (h / 2) sqrt(G[v]) is the exact Euclidean distance from the centre of v to O: along one axis the nearest point of a cube d voxels
 * away is (|d| - 1/2) h from the centre.  The arithmetic is integer throughout (the largest value is 3 * 1021^2), so the device's
 * field equals the minimum taken over all occupied voxels one by one, exactly.
 *
 * The pair.  Robot sphere a with world centre c and radius r against the grid, in fp64, n = dims, k = 0, 1, 2:
 *
 *   hi_k = origin_k + n_k h                    computed once by the host, product first, each operation rounded
 *   p_k  = min(max(c_k, origin_k), hi_k)                                    the centre clamped into the grid's box
 *   i_k  = (int) min(max(floor((p_k - origin_k) * inv_h), 0), n_k - 1)      inv_h = 1 / h computed once by the host
 *   x_k  = origin_k + (i_k + 0.5) h                                         the centre of the voxel read
 *   m    = (0.5 h) sqrt((double) G[i]) - |p - x|                            +inf when G[i] is LOIKB_GRID_EMPTY
 *   dout = |c - p|
 *   v    = (dout > 0 ? sqrt(dout^2 + max(m, 0)^2) : m) - r
 *
 * v + r is a lower bound of the distance from c to O wherever that distance is positive, and it is <= 0 whenever c lies in O; for a
 * centre inside the grid's box it is below the distance by at most sqrt(3) h.  The first property holds for whichever voxel i is
 * read, so the rounding of the index can never make the bound unsound.  Where v <= 0 it is NOT a penetration depth: it says that
 * the sphere may touch O and nothing about how deep.  The collision-aware multi-start's ordering of the goals without a free seed
 * by "least penetration" (class 0c of loik_amd_collision.h) is therefore coarser on a voxel world.
 *
 * Where it enters.  The pairs of a configuration, in ordinal order (loik_amd_collision.h: ties of the minimum go to the lowest
 * ordinal), are the world-sphere pairs, the world-box pairs, then with a grid set the ns grid pairs in sphere order, then the self
 * pairs.  min_world includes the grid pairs.  The witness of a grid pair is { LOIKB_CLR_WORLD_GRID, a, b }: a the robot sphere, b the
 * linear index (iz ny + iy) nx + ix of the voxel that was read at the sample the witness belongs to.  ns * (nws + nwb + 1) + the
 * self pairs must stay below 2^31 (LOIKB_ERR_ARG from the setter that would exceed it).
 *
 * What the motion layer certifies.  v never exceeds the true clearance, so the step (v - margin) / Lambda_a of the conservative
 * advancement (loik_amd_motion.h) stays valid unchanged: a segment, a shortcut, a planned edge or a blend reported FREE is free of O
 * at the margin, with the guarantee of that header.  BLOCKED may be conservative by sqrt(3) h: a motion that passes O closer than
 * margin + tol + sqrt(3) h may be reported BLOCKED although it is free.
 *
 * What does not read it.  Collision avoidance (loik_amd_avoid.h) needs the direction to the obstacle, and this bound has none.  It
 * does not ignore the grid silently: while a grid is set loikb_avoid_set with parameters, loikb_clearance_gradient and
 * loikb_avoid_box return LOIKB_ERR_STATE with a message that names the grid, and loikb_collision_set_world_grid with a grid returns
 * LOIKB_ERR_STATE while collision avoidance is set on the handle.
 *
 * loikb_collision_set_world_grid is a fourth latch beside the spheres, the world and the self pairs.  It validates everything, then
 * builds the field on the handle's stream, and is complete on return: occ may be freed or overwritten.  It replaces the grid set
 * before; occ == NULL clears it (dims, origin and h are then not read).  It does not touch the spheres and boxes of
 * loikb_collision_set_world, and that call does not touch the grid.  LOIKB_ERR_ARG: a NULL handle, a NULL dims or origin with a
 * non-NULL occ, a dimension outside 1 .. LOIKB_GRID_MAX_DIM, more than LOIKB_GRID_MAX_VOXELS voxels, an origin or h that is not
 * finite, h <= 0, an h whose inverse or a box corner origin + n h that is not finite, in_flags other than 0 or LOIKB_IN_DEVICE, more
 * than 2^31 pairs.  On any error nothing of the handle changes.
 *
 * loikb_collision_get_world_grid returns 1 when a grid is set and 0 when not (a NULL handle included); with a grid set it fills dims,
 * origin, h (each may be NULL) and, when G is not NULL, copies the field [nz][ny][nx] to G: a host pointer, or a device pointer with
 * LOIKB_OUT_DEVICE.  A negative LOIKB_ERR_* when the copy fails, or when out_flags is neither (LOIKB_ERR_ARG, whether a grid is set or
 * not).
 */
#ifndef LOIK_AMD_GRID_H
#define LOIK_AMD_GRID_H

#include "loik_amd_collision.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_GRID_VERSION 1  /* bumped whenever an entry point of this header changes */

#define LOIKB_GRID_MAX_DIM 512
#define LOIKB_GRID_MAX_VOXELS (1u << 26)
#define LOIKB_GRID_EMPTY 0xFFFFFFFFu

#define LOIKB_CLR_WORLD_GRID 4  /* the witness kind after LOIKB_CLR_SELF = 3 of loik_amd_collision.h */

int loikb_grid_version(void);

int loikb_collision_set_world_grid(loikb_solver *s, const unsigned char *occ, const int dims[3] /* nx, ny, nz */,
                                   const double origin[3], double h, int in_flags);
int loikb_collision_get_world_grid(loikb_solver *s, int dims[3], double origin[3], double *h,
                                   unsigned int *G /* or NULL */, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_GRID_H */
