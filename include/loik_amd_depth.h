/*
 * loik_amd_depth.h -- voxel worlds from depth images and point clouds, integrated on the device (libloik_amd.so).
 *
 * loik_amd_grid.h takes an occupancy grid.  A depth camera delivers a depth image and a lidar delivers points; this header takes
 * those.  The device back-projects the returns, bins them into voxels, keeps what earlier frames saw, clears what this frame sees
 * through, cuts the robot's own body out, and hands the occupancy to the build of loikb_collision_set_world_grid: the field G, and
 * with the latch of loik_amd_gridnear.h the transform F.  What is read afterwards is what that header describes, unchanged: a handle
 * given the occupancy of loikb_collision_grid_get_occupancy through loikb_collision_set_world_grid holds the same bits.  A handle
 * that never calls these entry points returns the bits it returned before this header existed.
 *
 * The grid.  dims, origin and h obey the rules of loikb_collision_set_world_grid; hi and inv_h = 1 / h are rounded by the host once,
 * as there.  The camera: a pinhole without distortion, pixel (u, v) with its centre at integer (u, v), the image [height][width]
 * row-major, the camera frame x right, y down, z forward; T_world_cam = (R row-major, p) places it in the world.  A pixel holds the
 * z-depth, not the range: d = (double) pixel * depth_scale in metres, and the pixel is a RETURN iff d is finite and
 * z_min <= d <= z_max.  0, NaN, inf and everything outside the range are no return.
 *
 * Every operation below is one fp64 operation rounded to nearest, in the order written and never fused, so that a reference can
 * follow the arithmetic: where the inputs are dyadic the device's occupancy is that of exact arithmetic, bit for bit.
 *
 * 1. The prior.  P[v] = 0 with LOIKB_DEPTH_REPLACE: the frame alone.  With LOIKB_DEPTH_FUSE, P[v] = (G[v] == 0) of the grid that is
 *    set, whichever call set it; that grid must have exactly these dims, origin and h (the same bits), else LOIKB_ERR_STATE.  FUSE
 *    with no grid set starts from the empty prior: REPLACE.
 *
 * 2. The carve (FUSE with carve = 1; the points route has no camera, so carve must be 0 there).  For every voxel with P = 1 and
 *    centre x_w,k = origin_k + (i_k + 0.5) h:  e = x_w - p,  x_c,j = (R_0j e_0 + R_1j e_1) + R_2j e_2.  If x_c,z > 0 the pixel is
 *    u = floor(((fx x_c,x) / x_c,z + cx) + 0.5), v likewise with fy and cy.  If 0 <= u < width, 0 <= v < height, the pixel holds a
 *    return d and x_c,z + band < d, the voxel is cleared.  A pixel without a return carves nothing, and neither does a voxel behind
 *    the camera.  What band is for: the test is made at the voxel's centre, and it clears a voxel that the ray only grazes, whose
 *    far corner may lie behind the measured surface.  No point of a voxel is farther from its centre than (sqrt(3) / 2) h, so with
 *    band >= (sqrt(3) / 2) h a cleared voxel lies wholly in front of the measured surface along that pixel's ray; add the sensor's
 *    depth noise to it.  band = 0 carves the most and may eat one layer of a surface seen at a slant.
 *
 * 3. The points.  A return (u, v, d) is the camera point x_c = (((u - cx) / fx) d, ((v - cy) / fy) d, d), the world point
 *    x_w,k = ((R_k0 x_c,0 + R_k1 x_c,1) + R_k2 x_c,2) + p_k, and the voxel i_k = floor((x_w,k - origin_k) inv_h).  The voxel is set
 *    when 0 <= i_k < n_k on all three axes: a point exactly on the low face is in, one exactly on the high face is out.  Any other
 *    point is dropped and counted as outside.  loikb_collision_grid_integrate_points starts at x_w: a point with a number that is not
 *    finite is no return.  The scatter is per pixel, one point one voxel.  A gather per voxel (project the voxel's centre, compare
 *    depths) would miss anything thinner than a voxel -- a cable, a table edge seen from the side -- and a world that loses thin
 *    obstacles certifies nothing; the carve may gather, because missing a voxel there only keeps it occupied.  The points win over
 *    the carve: a voxel that holds one of this frame's points is occupied, whatever step 2 decided.
 *
 * 4. The self-filter.  q_filter [n_filter][nq], 0 <= n_filter <= LOIKB_DEPTH_MAX_FILTER: configurations of the robot at the time of
 *    the frame (the current one; with motion blur the ones around it).  For every one of them and every sphere (c, r) of
 *    loikb_collision_set_spheres -- the world centre c from the placements loikb_clearance uses -- every voxel whose centre x_w is
 *    within r + filter_pad of c,  ((x_w,0 - c_0)^2 + (x_w,1 - c_1)^2) + (x_w,2 - c_2)^2 <= (r + filter_pad)^2,  is cleared.  The
 *    filter wins over the points.  A voxel the robot's surface fell into has its centre up to (sqrt(3) / 2) h away from that surface:
 *    filter_pad must cover (sqrt(3) / 2) h plus the sensor's noise for the robot's own surface to disappear.  A configuration with a
 *    number that is not finite filters nothing.  q_filter == NULL with n_filter > 0 means the first n_filter resident configurations
 *    (n_filter <= the batch, and a resident q).  In FUSE the filter also clears the prior: the robot's body is free wherever it is.
 *
 * 5. The build.  The resulting occupancy goes through the build of loikb_collision_set_world_grid -- the same kernels, G and with
 *    the latch F -- into the spare buffers, which change places with the resident ones after the stream has drained.  Complete on
 *    return: the image, the points and q_filter may be freed or overwritten.  The refusal of that call holds here: with collision
 *    avoidance latched and the nearest-voxel transform not, LOIKB_ERR_STATE.
 *
 * stats, when not NULL, receives four integer device counters, deterministic whatever the order of the threads: { the returns
 * (valid pixels, finite points), the returns that fell into the grid, the occupied voxels of the prior P, the occupied voxels of the
 * result }.
 *
 * in_flags: LOIKB_IN_DEVICE says that the image or the points are device memory, LOIKB_DEPTH_Q_DEVICE that q_filter is.  Everything
 * runs on the handle's stream.  The work buffers belong to the handle and only grow: a call at sensor rate allocates nothing after
 * the first of its size.
 *
 * LOIKB_ERR_ARG: a NULL handle, image, camera, dims, origin or params (NULL points with n > 0; n < 0); width or height outside
 * 1 .. LOIKB_DEPTH_MAX_IMAGE; intrinsics that are not finite, fx or fy <= 0; a T_world_cam that is not finite or whose R is not
 * orthonormal with determinant 1 to 1e-9 per entry; a depth_scale that is not finite or <= 0; not 0 < z_min <= z_max < inf; a grid
 * that loikb_collision_set_world_grid would refuse; a mode other than REPLACE or FUSE; carve other than 0 or 1, carve = 1 with
 * REPLACE or on the points route; band or filter_pad negative or not finite; params flags other than 0; a depth_type other than
 * LOIKB_DEPTH_F32 or LOIKB_DEPTH_U16; in_flags with any other bit; n_filter outside 0 .. LOIKB_DEPTH_MAX_FILTER.
 * LOIKB_ERR_STATE: FUSE onto a grid of another geometry; n_filter > 0 without collision spheres; q_filter == NULL with
 * n_filter > the batch or without a resident q; the avoidance refusal above.  Everything is validated before anything changes, and
 * on any error nothing of the handle changes: the grid, its occupancy and its field are as they were.
 *
 * loikb_collision_grid_get_occupancy returns 1 when a grid is set and 0 when not (a NULL handle included); with 1 and occ not NULL
 * it writes (G[v] == 0) as 0 / 1 bytes [nz][ny][nx] to occ, for whichever call set the grid: a host pointer, or a device pointer
 * with LOIKB_OUT_DEVICE.  A negative LOIKB_ERR_* when the copy fails or out_flags is neither (LOIKB_ERR_ARG, whatever the state).
 *
 * Out of scope: log-odds or TSDF weights (a voxel is occupied or not), lens distortion, rotated or per-instance grids, and
 * incremental updates of the field (every call builds it whole).
 */
#ifndef LOIK_AMD_DEPTH_H
#define LOIK_AMD_DEPTH_H

#include "loik_amd_gridnear.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_DEPTH_VERSION 1  /* bumped whenever an entry point of this header changes */

#define LOIKB_DEPTH_F32 0  /* float metres (times depth_scale) */
#define LOIKB_DEPTH_U16 1  /* unsigned 16-bit image units (times depth_scale) */

#define LOIKB_DEPTH_REPLACE 0
#define LOIKB_DEPTH_FUSE 1

#define LOIKB_DEPTH_Q_DEVICE 2  /* in_flags: q_filter is device memory (LOIKB_IN_DEVICE = 1 is for the image or the points) */

#define LOIKB_DEPTH_MAX_IMAGE 4096  /* of width and of height */
#define LOIKB_DEPTH_MAX_FILTER 64

typedef struct loikb_depth_camera {
  int width, height;       /* 1 .. LOIKB_DEPTH_MAX_IMAGE each; image [height][width], row-major */
  double fx, fy, cx, cy;   /* pinhole, in pixels; pixel (u, v) has its centre at integer (u, v) */
  double T_world_cam[12];  /* R row-major [9], p [3]: the camera frame (x right, y down, z forward) in the world */
  double depth_scale;      /* metres per image unit: 1.0 for float metres, 0.001 for uint16 millimetres */
  double z_min, z_max;     /* metric z-depth d is a return iff z_min <= d <= z_max and d is finite; 0 < z_min <= z_max */
} loikb_depth_camera;

typedef struct loikb_depth_params {
  int mode;           /* LOIKB_DEPTH_REPLACE: the frame alone; LOIKB_DEPTH_FUSE: onto the occupancy of the grid that is set */
  int carve;          /* FUSE only, 0 / 1: clear the prior voxels that this frame sees through */
  double band;        /* carve margin in metres, >= 0 */
  double filter_pad;  /* self-filter padding in metres, >= 0 */
  int flags;          /* 0 */
} loikb_depth_params;

int loikb_depth_version(void);

int loikb_collision_grid_integrate_depth(loikb_solver *s, const void *depth, int depth_type, const loikb_depth_camera *cam,
                                         const int dims[3], const double origin[3], double h, const loikb_depth_params *prm,
                                         const double *q_filter /* [n_filter][nq] or NULL */, int n_filter, int in_flags,
                                         long long stats[4] /* or NULL */);
int loikb_collision_grid_integrate_points(loikb_solver *s, const double *points /* [n][3], world */, int n, const int dims[3],
                                          const double origin[3], double h, const loikb_depth_params *prm,
                                          const double *q_filter /* [n_filter][nq] or NULL */, int n_filter, int in_flags,
                                          long long stats[4] /* or NULL */);
int loikb_collision_grid_get_occupancy(loikb_solver *s, unsigned char *occ /* [nz][ny][nx] or NULL */, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_DEPTH_H */
