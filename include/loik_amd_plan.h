/*
 * loik_amd_plan.h -- certified RRT-Connect planning of joint-space paths (libloik_amd.so).
 *
 * loikb_motion_clearance (loik_amd_motion.h) says that a segment is free, loikb_shortcut_paths (loik_amd_shortcut.h) shortens a path
 * and loikb_retime_paths (loik_amd_retime.h) times one; this header makes one.  loikb_plan_paths runs a batch of bidirectional
 * RRT-Connect queries on the device, a wavefront per query from its first check to its outputs, so that no query waits for another
 * one.  Every edge of either tree is accepted only when the conservative advancement of loik_amd_motion.h certifies it FREE.
 * Everything is fp64 whatever the handle's precision.  Pointers are host, or device with LOIKB_IN_DEVICE / LOIKB_OUT_DEVICE (q_start
 * and q_goal alike, all outputs alike; s_lo and s_hi are always host and are copied by the call); a call is complete on return.  The
 * call does not read the resident q or the data object and edits neither; a handle that never calls it launches exactly what it
 * launched before this header existed.
 *
 * Definitions.  diff(x, y) is difference(x, y) in the arithmetic of loikb_difference, bit for bit, except that two finite rows that
 * are equal entry by entry give 0 exactly (the rule of loikb_path_length).  dist2(x, y) is the sum of the squares of diff(x, y) in DoF
 * order.  check(from, to) is the advancement of loikb_motion_clearance on the segment from (+) s difference(from, to), s in [0, 1],
 * with (margin, tol, max_evals): the same pairs, the same order, hence the same status.  Every edge is checked from its start-side end
 * to its goal-side end, the direction in which it appears in the output, so loikb_motion_clearance_path on a found path repeats the
 * planner's own checks bit for bit.
 *
 * The rule, per query b.  Tree 0 is rooted at q_start[b], tree 1 at q_goal[b]; each holds at most max_nodes nodes, its root included.
 *
 *   0. A start or goal with an entry that is not finite, or a difference(start, goal) that is not finite: INVALID.  check(start,
 *      goal): FREE is FOUND with L = 2 after 0 iterations; BLOCKED at its first sample (s_free == 0) is START_BLOCKED.  Then
 *      check(goal, goal), the zero segment (two samples): BLOCKED is GOAL_BLOCKED.
 *   1. Iteration r = 0 .. max_iters - 1: tree a = r mod 2 extends.  The sample q_rand uses the arithmetic of the multi-start sampler
 *      (loik_amd_multistart.h): key = mix(seed + 0x9E3779B97F4A7C15 * (r + 1)), word = mix(key ^ ((b << 32) | j)),
 *      u = (word >> 11) * 2^-53, q_j = min(lo_j + fl(u * (hi_j - lo_j)), hi_j), the product rounded before the sum.  DoF j is sampled
 *      iff s_lo[j] and s_hi[j] are both finite; every other coordinate of q_rand is the start row's.
 *   2. The nearest node of a tree to a target is the one with the least dist2(node, target); ties go to the lowest node index.
 *   3. One extension of tree t from its node k towards a target: dv = diff(node_k, target), d = sqrt(dist2(node_k, target)).
 *      d <= step: the new configuration is the target, bit for bit (a reach).  Otherwise it is node_k (+) c dv, c = step / d, in the
 *      arithmetic of loikb_integrate.  An extension that would add a node to a tree that already holds max_nodes -- every extension
 *      that is not a reach, and the reach of q_rand in 4a -- ends the query with EXHAUSTED_NODES, without a check.  The edge is
 *      check(node_k, new) on tree 0 and check(new, node_k) on tree 1; anything but FREE is trapped.
 *   4. a. Tree a extends from its nearest node towards q_rand.  Trapped: the next iteration.  Otherwise the new configuration is
 *         added to tree a with parent k, reach or not.
 *      b. Tree 1 - a connects to that node: the first extension starts from its nearest node, each later one from the node just
 *         added.  An extension that is not a reach adds its node and repeats; trapped ends the iteration; a reach whose edge is FREE
 *         adds nothing and ends the query with FOUND.
 *   5. FOUND: the path runs from the root of tree 0 along parents' edges to the bridge and on to the root of tree 1; L is its number
 *      of waypoints.  L > T: TOO_LONG, L is reported.  max_iters used up: EXHAUSTED_ITERS.
 *
 * Outputs.  out_info[b] = { status, L, iterations run, nodes of tree 0, nodes of tree 1, edges checked, edges FREE, samples taken }:
 * status is LOIKB_PLAN_*; L is 0 unless the status is FOUND or TOO_LONG; the checks of step 0 count as edges; the samples are the
 * sum of the advancements' evals and saturate at INT_MAX; an INVALID query has all of them 0.  out_path[b]: with FOUND row 0 is
 * q_start[b] and row L - 1 is q_goal[b], bit for bit, and the rows from L on repeat the last row, so that the result is a [B][T]
 * path that loikb_shortcut_paths, loikb_retime_paths and loikb_motion_clearance_path accept as it is; with every other status all T
 * rows are NaN.  out_length[b] (may be NULL) is the found path's length in the sense of loikb_path_length, bit for bit with that call
 * on out_path, and NaN with every other status.
 *
 * What a result certifies.  Every segment of a FOUND path was certified MOTION_FREE by this call, with the guarantee of
 * loik_amd_motion.h: no sampled clearance below margin + tol and the bound of the advancement in between.  EXHAUSTED_ITERS and
 * EXHAUSTED_NODES are not a proof of infeasibility: they say that this seed, these ranges and these budgets found nothing.
 * START_BLOCKED and GOAL_BLOCKED say that the start (goal) configuration itself is closer than margin + tol.  The call never clamps
 * the start or the goal to the ranges: s_lo and s_hi bound the samples only.
 *
 * Ranges.  s_lo, s_hi [nv] in idx_v order.  A finite entry is legal only on a DoF whose coordinate a plain sum advances, the rule
 * and the message of loikb_set_joint_limits; lo <= hi; at least one DoF must be sampled.
 *
 * Scratch.  The trees live in handle-owned device memory, per resident wavefront 2 * max_nodes rows of nq doubles with their
 * parents.  The grid is the smallest of B, the wavefronts loikb_shortcut_paths would launch, and what LOIKB_PLAN_SCRATCH_BYTES
 * allows (at least one wavefront); the wavefronts stride over the queries.
 *
 * Errors.  LOIKB_ERR_ARG: NULL handle, B < 0, T < 2, B * T >= 2^31, a NULL q_start, q_goal, out_path or out_info with B > 0, a NULL
 * s_lo, s_hi or p, a margin that is not finite, a tol that is not finite or < 1e-9, max_evals outside 1 .. 65536, a step that is not
 * finite or <= 0, max_iters outside 0 .. 1048576, max_nodes outside 2 .. 65536, flags != 0, a NaN range, lo > hi, a finite range on a
 * DoF that cannot carry one, no DoF sampled, out_path == q_start or q_goal.  LOIKB_ERR_STATE: no spheres set
 * (loikb_collision_set_spheres).  The arguments are checked first, then the state, as in loik_amd_shortcut.h; after both B == 0 is
 * LOIKB_OK and writes nothing.  A call that fails writes nothing.
 */
#ifndef LOIK_AMD_PLAN_H
#define LOIK_AMD_PLAN_H

#include "loik_amd_motion.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_PLAN_VERSION 1  /* bumped whenever a struct or an entry point of this header changes */

#define LOIKB_PLAN_SCRATCH_BYTES (256ull << 20)  /* the budget of the trees of all resident wavefronts */

enum {
  LOIKB_PLAN_FOUND = 0,
  LOIKB_PLAN_EXHAUSTED_ITERS = 1,
  LOIKB_PLAN_EXHAUSTED_NODES = 2,
  LOIKB_PLAN_START_BLOCKED = 3,
  LOIKB_PLAN_GOAL_BLOCKED = 4,
  LOIKB_PLAN_TOO_LONG = 5,
  LOIKB_PLAN_INVALID = 6
};

typedef struct loikb_plan_params {
  double margin;            /* as loikb_motion_params                                               */
  double tol;               /* as loikb_motion_params (finite, >= 1e-9)                             */
  double step;              /* finite, > 0: the longest edge, in the norm of loikb_path_length      */
  unsigned long long seed;  /* stream key of the samples                                            */
  int max_evals;            /* as loikb_motion_params (1 .. 65536), per checked edge                */
  int max_iters;            /* 0 .. 1048576 samples drawn per query                                 */
  int max_nodes;            /* 2 .. 65536 nodes per tree, root included                             */
  int flags;                /* reserved, 0                                                          */
} loikb_plan_params;

int loikb_plan_version(void);

/* q_start, q_goal [B][nq]; s_lo, s_hi [nv] on the host (idx_v order, copied by the call).
 * out_path [B][T][nq]; out_info [B][8] ints; out_length [B] or NULL.                                                  */
int loikb_plan_paths(loikb_solver *s, const double *q_start, const double *q_goal, int B, int in_flags,
                     const double *s_lo, const double *s_hi, const loikb_plan_params *p, int T,
                     double *out_path, int *out_info, double *out_length, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_PLAN_H */
