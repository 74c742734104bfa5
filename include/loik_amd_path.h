/*
 * loik_amd_path.h -- waypoint paths for the batched pose IK of loik_amd_pose.h (libloik_amd.so): "take these B seeds along
 * these B paths", every instance at its own pace.
 *
 * A sampling planner, a Cartesian trajectory or a teleoperation stream wants a configuration for every pose along a path, each
 * found from the one before.  One loikb_solve_pose per waypoint does that, but forces the batch into lock step: a waypoint costs
 * as many whole-batch inner solves as its slowest instance needs, the others idle through solves with b = 0.
 * loikb_solve_pose_path runs the same device loop with a cursor per instance: an instance that reached its waypoint goes on to
 * the next in the same step, whatever the others do.  The inner solves of the call are then the longest per-instance total,
 * not the sum over the waypoints of the per-waypoint maximum.
 *
 * Each instance carries a cursor w (the waypoint it is heading for, 0 at the start) and a count ws of the steps it spent on
 * waypoint w.  A re-target of a running instance repeats this rule:
 *
 *   1. e = the error of the resident q against waypoint w: e_c = log6(oMi_c^-1 oMdes_{w,c}) per active constraint, or the masked
 *      task-frame error of loik_amd_tasks.h when a task specification is in force;
 *   2. e or q not finite: the instance is STOPPED (LOIKB_POSE_ST_STOPPED);
 *   3. max_c |e_c|_inf <= tol_pose: with `record` the row of q goes to Q[b][w]; WSTEPS[b][w] = ws; then w += 1, ws = 0.
 *      w == T: the instance is LOIKB_POSE_ST_REACHED (the path is COMPLETE).  Otherwise the NEXT waypoint is examined in the
 *      same re-target, from 1.: reaching a waypoint never costs an idle solve, and a run of waypoints that q already satisfies is
 *      crossed at once;
 *   4. otherwise, if max_steps_per_waypoint > 0 and ws == max_steps_per_waypoint: the instance is STALLED.  It no longer runs
 *      or moves; its pose status has neither REACHED nor STOPPED;
 *   5. otherwise the instance runs: b_c = A_c (gain / dt) e_c (with tasks: (gain / dt) S_c e_c), steps and ws count one.
 *
 * Everything else is loikb_solve_pose's loop, word for word: instances that do not run get b = 0 and their z is discarded; the
 * re-target after pose->max_steps steps (the budget of the WHOLE path) writes no b and counts nothing, but applies 1. to 4.; the
 * loop ends when no instance runs; the inner solve's outcome goes into the pose status of the instances that ran in it; with
 * joint position limits on the handle (loik_amd_limits.h) the step box, the clamp and the restore are those of loikb_solve_pose;
 * the data object holds afterwards what it holds after loikb_solve_pose.  T = 1 with max_steps_per_waypoint = 0 IS
 * loikb_solve_pose, bit for bit.
 *
 * After the call loikb_pose_get and loikb_pose_get_limit_flags describe it as the last pose solve: STEPS is the total over the
 * path, STATUS the bits above, ERR the error against waypoint min(cursor, T - 1) at the final q, TIMING the call's.
 *
 * Waypoints are placements [R row-major (9), t (3)] as the targets of loikb_solve_pose, one per active constraint and waypoint:
 * [B][T][nc][12], or [T][nc][12] for the whole batch with LOIKB_POSE_TARGET_SHARED.  Interpolation is the caller's: the library
 * visits the waypoints it is given.
 *
 * Errors.  LOIKB_ERR_ARG: n_waypoints < 1, max_steps_per_waypoint < 0, record outside 0..1, flags != 0, NULL pointers, and
 * everything loikb_solve_pose rejects; the rotation check covers ALL waypoints.  LOIKB_ERR_STATE as loikb_solve_pose.  On any
 * error the handle is unchanged.  A handle that never calls an entry point of this header runs exactly what it ran before this
 * header existed.
 */
#ifndef LOIK_AMD_PATH_H
#define LOIK_AMD_PATH_H

#include "loik_amd_pose.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_PATH_VERSION 1  /* bumped whenever a struct or an entry point of this header changes */

typedef struct loikb_path_params {
  int n_waypoints;             /* T >= 1                                                              */
  int max_steps_per_waypoint;  /* >= 0; 0: only pose->max_steps (the budget of the WHOLE path) bounds  */
  int record;                  /* 1: keep q at every reached waypoint (LOIKB_PATH_F_Q), 0: do not      */
  int flags;                   /* reserved, 0                                                          */
} loikb_path_params;

int loikb_path_version(void);

/* waypoints [B][T][nc][12], or [T][nc][12] with LOIKB_POSE_TARGET_SHARED; q as loikb_solve_pose; LOIKB_IN_DEVICE as there */
int loikb_solve_pose_path(loikb_solver *s, const double *q, const double *waypoints, int in_flags, const loikb_pose_params *pose,
                          const loikb_path_params *path);

/* results of the last loikb_solve_pose_path (LOIKB_ERR_STATE before the first) */
enum {
  LOIKB_PATH_F_CURSOR = 0,  /* int [B]: waypoints reached                                                                  */
  LOIKB_PATH_F_STATUS,      /* int [B]: LOIKB_PATH_ST_* (0: neither -- out of steps, or stopped)                            */
  LOIKB_PATH_F_WSTEPS,      /* int [B][T]: steps spent on each waypoint; at the cursor: so far; later entries are 0        */
  LOIKB_PATH_F_Q,           /* double [B][T][nq]: q at each reached waypoint, NaN rows from the cursor on; record = 1 only */
  LOIKB_PATH_F_TIMING       /* double [4]: as LOIKB_POSE_F_TIMING                                                          */
};
enum {
  LOIKB_PATH_ST_COMPLETE = 1,  /* every waypoint reached: cursor == T, the pose status has REACHED   */
  LOIKB_PATH_ST_STALLED = 2    /* max_steps_per_waypoint steps spent on waypoint `cursor` without reaching it */
};
int loikb_path_get(loikb_solver *s, int field, void *out, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_PATH_H */
