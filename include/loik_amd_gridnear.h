/*
 * loik_amd_gridnear.h -- voxel worlds: the nearest-voxel transform of an occupancy grid, and collision avoidance that reads the grid
 * (libloik_amd.so).
 *
 * loik_amd_grid.h makes an occupancy grid a world object that every clearance evaluation and every certificate of the motion layer
 * reads, through a lower bound v of the clearance.  A bound is a number; the velocity damper of loik_amd_avoid.h needs a direction.  This
 * header builds what gives it one: next to the distance field G the device builds the feature transform F, the occupied voxel that
 * attains G; a sphere then finds a real cube near it among the features of the voxels around it, and the outward normal of that cube is
 * the direction of the pair.  It is opt-in, a fifth latch: a handle that never sets it launches what it launched before this header
 * existed and returns the same bits, and the refusals of loik_amd_grid.h stay the default.
 *
 * The transform.  For every voxel v, F[v] is an unsigned 32-bit integer: the linear index (uz ny + uy) nx + ux of an occupied voxel u
 * that attains G[v] of loik_amd_grid.h; among several minimisers the lowest linear index; LOIKB_GRID_NO_VOXEL when no voxel is
 * occupied.  It is integer and exact: the device's F equals the choice made by a brute force over all occupied voxels one by one, bit
 * for bit, as G does.  The device carries the key (G << 32) | F through the three min-plus passes of the field, so that a 64-bit minimum
 * breaks the ties by itself; only F stays resident.
 *
 * The pair with a direction.  Sphere (c, r); p, i, x and v are exactly those of loik_amd_grid.h, the same bits.  Per axis k
 *
 *   j_k = i_k - (p_k < x_k ? 1 : 0),     the two indices max(j_k, 0) and min(j_k + 1, n_k - 1):
 *
 * the up to eight voxels whose centres surround p.  The candidates are the F of those voxels.  For a candidate u with cube centre
 * t_u = origin + (u + 0.5) h and half edge h / 2
 *
 *   d_u = | max(|c - t_u| - h / 2, 0) |        (componentwise absolute value and maximum, then the Euclidean norm)
 *
 * and the chosen cube is the one of least d_u, the lowest u on a tie.  Its normal n is the world-box normal of loik_amd_avoid.h with
 * R = I, t = t_u and half extents (h / 2, h / 2, h / 2): outside the cube sgn(e) o max(|e| - h / 2, 0) / d_u with e = c - t_u, inside it
 * the face of the largest |e_k| - h / 2, the lowest index on a tie.  With an empty grid there is no cube: u = LOIKB_GRID_NO_VOXEL,
 * d_u = +inf and n = 0.
 *
 * What holds:  v <= true clearance <= d_u - r, the upper side for c outside O.  The upper bound is the exact distance to one real
 * cube of O, the lower one the sound bound of loik_amd_grid.h.  Eight candidates do not guarantee the nearest cube of all.
 *
 * Where the pair enters avoidance.  With the latch on and a grid set, loikb_avoid_set, loikb_clearance_gradient and loikb_avoid_box
 * accept the grid, and loikb_collision_set_world_grid is accepted while avoidance is latched.  The grid is one more world object of
 * every sphere: its ordinal among the sphere's world objects is nws + nwb, after the boxes, and overall the pairs keep the ordinals of
 * loikb_clearance.  Its clearance is v, the LOWER bound: avoidance may think an obstacle nearer than it is, never farther, and
 * loikb_clearance_gradient keeps its promise of the minima and the witness of loikb_clearance, { LOIKB_CLR_WORLD_GRID, a, the voxel
 * read }.  Its normal is n above, m is that of a world pair, and the partner loikb_avoid_box reports is nws + nwb.  The price: v is
 * below the distance by up to sqrt(3) h, so a sphere cannot come nearer to O than d_safe plus up to sqrt(3) h.  The gradient row is
 * n^T Jc: the derivative of the distance to the chosen cube, not of v, which is piecewise constant in the voxel read.
 *
 * An empty grid under the latch.  Every grid pair then has v = +inf and still holds its ordinal.  It is under no d_influence and
 * narrows nothing: the box of loikb_avoid_box and of the pose loops is that of a handle without a grid, bit for bit.  +inf comes after
 * every number, so beside any other world object the grid is never a sphere's partner, and beside any other pair never the witness.
 * With no other world object it is the sphere's partner, nws + nwb = 0, at clearance +inf, where a handle without a grid reports -1;
 * and in a configuration with no other pair at all, where every minimum is +inf, ties go to the lowest ordinal as always: the witness
 * of loikb_clearance and loikb_clearance_gradient is { LOIKB_CLR_WORLD_GRID, 0, the voxel read for sphere 0 }, where a handle without a
 * grid reports { LOIKB_CLR_NONE, -1, -1 }, and the gradient row is 0.
 *
 * loikb_collision_grid_set_nearest(s, 1) sets the latch.  If a grid is set it builds F for it on the handle's stream, complete on
 * return; every later loikb_collision_set_world_grid builds G and F, both into spare buffers that change places with the resident
 * ones after both builds succeeded, so a failed set leaves both as they were.  While the latch is on the handle keeps F, its spare and
 * the keys of a build (16 bytes a voxel in all), so that a set at sensor rate allocates nothing.
 * on = 0 drops F, frees all three, and the handle is as if never latched;
 * it returns LOIKB_ERR_STATE while a grid is set and avoidance is latched.  LOIKB_ERR_ARG: a NULL handle, on other than 0 or 1.  On
 * any error nothing of the handle changes.
 *
 * loikb_collision_grid_get_nearest returns 1 when the latch is on and a grid is set, and 0 when not (a NULL handle included); with 1
 * and F not NULL it copies the transform [nz][ny][nx] to F: a host pointer, or a device pointer with LOIKB_OUT_DEVICE.  A negative
 * LOIKB_ERR_* when the copy fails or out_flags is neither (LOIKB_ERR_ARG, whatever the state).
 *
 * loikb_grid_nearest_query evaluates the pair for n spheres given in the world frame: spheres [n][4] = x y z r (host, or device with
 * LOIKB_IN_DEVICE); out_val [n][2] = { v, d_u - r }, out_vox [n][2] = { i, u } as linear indices (u = -1 with an empty grid),
 * out_normal [n][3] (host, or all three device with LOIKB_OUT_DEVICE).  A row with a number that is not finite gives NaN values, a
 * NaN normal and { -1, -1 }.  LOIKB_ERR_ARG: a NULL handle, n < 0, a NULL array with n > 0, in_flags other than 0 or LOIKB_IN_DEVICE.
 * LOIKB_ERR_STATE: no grid set, or the latch off.  n == 0 is LOIKB_OK and writes nothing.
 */
#ifndef LOIK_AMD_GRIDNEAR_H
#define LOIK_AMD_GRIDNEAR_H

#include "loik_amd_grid.h"
#include "loik_amd_avoid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_GRIDNEAR_VERSION 1  /* bumped whenever an entry point of this header changes */

#define LOIKB_GRID_NO_VOXEL 0xFFFFFFFFu

int loikb_gridnear_version(void);

int loikb_collision_grid_set_nearest(loikb_solver *s, int on);
int loikb_collision_grid_get_nearest(loikb_solver *s, unsigned int *F /* [nz][ny][nx] or NULL */, int out_flags);
int loikb_grid_nearest_query(loikb_solver *s, const double *spheres /* [n][4] x y z r, world */, int n, int in_flags,
                             double *out_val /* [n][2] */, int *out_vox /* [n][2] */, double *out_normal /* [n][3] */, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_GRIDNEAR_H */
