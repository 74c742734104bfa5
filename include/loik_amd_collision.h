/*
 * loik_amd_collision.h -- collision clearance of a sphere model of the robot against a world of spheres and oriented boxes and
 * against itself, and a multi-start (loik_amd_multistart.h) that answers a goal only with a collision-free seed (libloik_amd.so).
 *
 * The pose layer takes a batch of seeds to targets; this header says whether the configurations it leaves are inside something.
 * Everything is fp64 from fp64 q, whatever the handle's precision, as with the other pose kernels.  All ids are the caller's
 * joint ids; the link of a multi-DoF joint is the last joint of its chain on the device, as in loikb_frame_jacobians.
 *
 * The model is three latches on the handle.  Setting one validates everything first, uploads once and replaces what was set
 * before; no solve reads any of them.
 *
 *   spheres     (x, y, z, r) in the frame of a link, r >= 0.  Link 0, the universe, is legal: a sphere fixed in the world that
 *               belongs to the robot.  At most LOIKB_CLR_MAX_SPHERES.  ns = 0 clears the spheres and the self pairs.
 *   world       spheres (x, y, z, r) and oriented boxes (R row-major [9], p [3], half extents h [3] > 0), shared by the whole batch.
 *               nws = nwb = 0 clears the world.
 *   self pairs  with enable = 1 the list of sphere pairs (a < b), in lexicographic order, that satisfy all of: the links of a and b
 *               differ; neither link is the other's parent in the caller's tree; the link pair is not in ignore_links (either
 *               order).  The list is rebuilt whenever the spheres are set.  enable = 0 drops the list and the ignore pairs.
 *
 * Pair clearances, c a sphere centre in the world (c = oMi(link) (x, y, z)):
 *
 *   sphere, sphere   |c1 - c2| - r1 - r2
 *   sphere, box      p = R^T (c - t),  d = |p| - h componentwise,
 *                    clearance = || max(d, 0) ||_2 + min(max(d_x, d_y, d_z), 0) - r
 *                    (the exact signed distance of the centre to the box, negative inside, less the radius)
 *
 * The query.  out_min[i] = { min, min_world, min_self }: the minimum over all pairs, over the (robot sphere, world object) pairs, over
 * the listed self pairs.  The minimum over an empty set is +inf.  out_witness[i] = { kind, a, b }, the pair that achieves min:
 * kind LOIKB_CLR_*, a the robot sphere, b the world sphere, the world box or the other robot sphere; { LOIKB_CLR_NONE, -1, -1 } for an
 * empty set.  The winner is the minimum in the total order (clearance, ordinal): the ordinal counts the world-sphere pairs first,
 * a major and b minor, then the world-box pairs in the same order, then the self pairs in list order.  Exact ties go to the lowest
 * ordinal, so the result does not depend on the order in which the device combines partial minima (the rule of the multi-start
 * selection).  min == min(min_world, min_self) exactly.  A configuration whose q holds a NaN or an infinity gets NaN in all three
 * minima and the witness { LOIKB_CLR_NONE, -1, -1 }; the other configurations are not affected.
 *
 * The collision-aware multi-start.  With loikb_clearance_set_multistart set on the handle, loikb_solve_pose_multistart runs one
 * clearance query over the resident q after each round's pose loop, clr[b] = its min, and
 *
 *   - a REACHED, not STOPPED instance is class 0 when clr >= margin and class 0c otherwise (a NaN included).  Class 0 keeps its
 *     cost (nearest, first, or dexterous with the latch of loik_amd_jacobian.h).  Class 0c has the cost -clr, so the least
 *     penetration comes first, and a goal won by it has the status LOIKB_MS_GOAL_IN_COLLISION.  The order is 0 < 0c < 1 < 2;
 *   - only class 0 answers a goal: the restarts continue while some goal has only colliding answers;
 *   - the re-sampler treats class 0c as not reached and draws those rows anew (from a loop-private copy of the status: the pose
 *     status the caller reads is not edited);
 *   - loikb_clearance_get_multistart_result returns the winner's clearance and witness, the class-0 count of each goal and clr.
 *
 * A handle on which the latch was never set, or was cleared, runs exactly what it ran before this header existed.
 *
 * Errors.  LOIKB_ERR_ARG: NULL handle or out_min, a NULL array with a positive count, a negative count, a link id outside
 * 0..njoints-1, a number that is not finite, a negative radius, a half extent that is not > 0, a box rotation that is not
 * orthonormal with determinant 1 (tolerance 1e-9), more than LOIKB_CLR_MAX_SPHERES spheres, q = NULL with n != B, flags != 0, a
 * margin that is not finite, an ignore pair outside 0..njoints-1, a field that is not LOIKB_CLR_MS_F_*.  LOIKB_ERR_STATE: q = NULL with
 * no configurations resident on the device yet, the query, the latch or a latched multi-start with no spheres set, enable = 1 with
 * no spheres set, the result getter before a latched multi-start.  n == 0 is LOIKB_OK and writes nothing.  On any error nothing of the
 * handle changes; loikb_last_error() names the offending index.
 */
#ifndef LOIK_AMD_COLLISION_H
#define LOIK_AMD_COLLISION_H

#include "loik_amd_multistart.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_COLLISION_VERSION 1  /* bumped whenever a struct or an entry point of this header changes */

#define LOIKB_CLR_MAX_SPHERES 2048

/* the kind of a witness */
enum { LOIKB_CLR_NONE = 0, LOIKB_CLR_WORLD_SPHERE = 1, LOIKB_CLR_WORLD_BOX = 2, LOIKB_CLR_SELF = 3 };

/* the fourth goal status of a multi-start with the latch below: the best answer of the goal reached it in collision */
enum { LOIKB_MS_GOAL_IN_COLLISION = 8 };

typedef struct loikb_clearance_params {
  double margin;  /* finite: a reached seed answers its goal when its clearance is >= margin */
  int flags;      /* reserved, 0 */
} loikb_clearance_params;

int loikb_collision_version(void);

/* links [ns]: the caller's joint ids; spheres [ns][4] = (x, y, z, r) in the link's frame (host) */
int loikb_collision_set_spheres(loikb_solver *s, const int *links, const double *spheres, int ns);

/* wspheres [nws][4] = (x, y, z, r); wboxes [nwb][15] = (R row-major, p, h) (host) */
int loikb_collision_set_world(loikb_solver *s, const double *wspheres, int nws, const double *wboxes, int nwb);

/* ignore_links [ni][2]: pairs of the caller's joint ids whose spheres are never tested against each other (host) */
int loikb_collision_set_self_pairs(loikb_solver *s, int enable, const int *ignore_links, int ni);

/* the length of the self-pair list (0: off, or no pair) */
int loikb_collision_num_self_pairs(const loikb_solver *s);

/* q [n][nq] (host, or device with LOIKB_IN_DEVICE), any n >= 0; q = NULL: the resident q, n must equal the batch.
 * out_min [n][3] doubles, out_witness [n][3] ints or NULL (host, or both device with LOIKB_OUT_DEVICE), complete on return. */
int loikb_clearance(loikb_solver *s, const double *q, int n, int in_flags, double *out_min, int *out_witness, int out_flags);

/* The collision-aware selection for every later loikb_solve_pose_multistart on this handle.  p = NULL clears it (the handle
 * behaves as if never set).                                                                                               */
int loikb_clearance_set_multistart(loikb_solver *s, const loikb_clearance_params *p);

/* returns 1 and fills *out (if not NULL) when the latch is set, 0 when it is not */
int loikb_clearance_get_multistart(const loikb_solver *s, loikb_clearance_params *out);

/* results of the last loikb_solve_pose_multistart, which ran with the latch (LOIKB_ERR_STATE otherwise) */
enum { LOIKB_CLR_MS_F_CLEARANCE = 0,  /* double [G]: the winner's min                                    */
       LOIKB_CLR_MS_F_WITNESS,        /* int [G][3]: the winner's witness                                */
       LOIKB_CLR_MS_F_NCLEAR,         /* int [G]: the goal's class-0 instances after the last round      */
       LOIKB_CLR_MS_F_INSTANCE };     /* double [B]: clr of the last round                               */
int loikb_clearance_get_multistart_result(loikb_solver *s, int field, void *out, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_COLLISION_H */
