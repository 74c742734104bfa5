/*
 * loik_amd_axis.h -- axis-symmetric tool tasks for the batched pose IK of loik_amd_pose.h: the rotation about the task frame's z
 * axis is free (libloik_amd.so).
 *
 * A drill, a spindle, a torch, a nozzle, a probe, a suction cup or a camera that must point somewhere constrains five degrees of
 * freedom, or two, and leaves the spin about its own axis to the solver.  This header adds that as a modifier bit on the kinds of
 * loik_amd_tasks.h; the axis is always the z axis of the task frame iMf (a caller who wants another axis rotates iMf).
 *
 * Notation as in loik_amd_tasks.h:
 *     (Re, pe) = oMf^-1 oMdes,  Re = (R Rf)^T Rd,  pe = (R Rf)^T (td - t - R pf)
 *     d = (Re[2], Re[5], Re[8])        the third column of Re: the desired z axis seen from the task frame
 *
 * The axis error w_axis(Re) is the minimal rotation that carries the frame's z onto d, in frame axes:
 *     s = sqrt(d_x^2 + d_y^2),  theta = atan2(s, d_z)
 *     s == 0:  w = (pi, 0, 0) if d_z < 0, else (0, 0, 0)     exactly antiparallel: any axis in the xy plane would do, x is the rule
 *     else:    w = (theta / s) (-d_y, d_x, 0)
 * w_z is identically 0, which is what makes the mask consistent.  A d that is not finite gives a w that is not finite, and the
 * instance is STOPPED, as for every kind.
 *
 *     LOIKB_TASK_POSE_AXIS   e = [pe; w_axis(Re)]      S = diag(1,1,1,1,1,0)
 *     LOIKB_TASK_AXIS        e = [0;  w_axis(Re)]      S = diag(0,0,0,1,1,0)   the target's translation is ignored
 *
 * Everything else is loik_amd_tasks.h's, unchanged: A_c = S_c X_c^-1 written by loikb_pose_set_tasks through the
 * UpdateEqConstraint path (one or four zero rows), b_c = (gain / dt) S_c e_c, reached when max_c |S_c e_c|_inf <= tol_pose,
 * LOIKB_POSE_F_ERR with exact zeros in the masked-out entries, loikb_pose_get_tasks returning the kinds as set, the lifetime /
 * drop rule, joint limits, acceleration limits and f32 handles with fp64 FK and logarithms.  loikb_pose_set_tasks accepts the
 * kinds 0, 1, 2, 4 and 6; 3, 5 (POSITION | FREE_Z means nothing), 7 and everything outside 0..7 stay LOIKB_ERR_ARG.
 * loikb_solve_pose_multistart, loikb_solve_pose_path and loikb_track_pose run the same rule; the feed-forward of
 * loikb_track_pose for these kinds is stated in loik_amd_track.h.
 *
 * Not here: look-at a POINT (its constraint matrix depends on the distance, so it is per instance); masks in world axes (the same
 * reason); a choice of axis other than by iMf; a tolerance per kind.
 */
#ifndef LOIK_AMD_AXIS_H
#define LOIK_AMD_AXIS_H

#include "loik_amd_tasks.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_AXIS_VERSION 1  /* bumped whenever an entry point of this header changes */

int loikb_axis_version(void);

/* the modifier bit this header adds to the kinds of loikb_pose_set_tasks, and the two kinds it makes */
enum { LOIKB_TASK_FREE_Z = 4,                                          /* the rotation about the task frame's z axis is free */
       LOIKB_TASK_POSE_AXIS = LOIKB_TASK_POSE | LOIKB_TASK_FREE_Z,      /* 4: position of the frame origin + direction of its z axis (5 DoF) */
       LOIKB_TASK_AXIS = LOIKB_TASK_ORIENTATION | LOIKB_TASK_FREE_Z };  /* 6: direction of the frame's z axis only (2 DoF)                    */

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_AXIS_H */
