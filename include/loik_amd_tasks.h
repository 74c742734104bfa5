/*
 * loik_amd_tasks.h -- tool frames and position-only / orientation-only tasks for the batched pose IK of loik_amd_pose.h
 * (libloik_amd.so).
 *
 * loikb_solve_pose measures e_c = log6(oMi_c^-1 oMdes_c) of the constrained link's JOINT frame, all six entries.  With a task
 * specification on the handle, each active constraint c has a kind and a frame iMf_c fixed on its link (Pinocchio's oMf):
 *
 *     (R, t) = oMi of the link, (Rf, pf) = iMf, (Rd, td) = the target; twists are [linear; angular]
 *     oMf  = (R Rf, t + R pf)                                      the placement of the task frame
 *     X^-1 = [[Rf^T, -Rf^T [pf]x], [0, Rf^T]]                      v_f = X^-1 v_i: the velocity of the frame origin, in frame axes
 *
 *     LOIKB_TASK_POSE         e = log6(oMf^-1 oMdes)                          S = I
 *     LOIKB_TASK_POSITION     e = [(R Rf)^T (td - t - R pf); 0]               S = diag(1,1,1,0,0,0)   the target's rotation is ignored
 *     LOIKB_TASK_ORIENTATION  e = [0; log3((R Rf)^T Rd)]                      S = diag(0,0,0,1,1,1)   the target's translation is ignored
 *
 * A frame offset and a row mask are both a constraint matrix, A_c = S_c X_c^-1, which loikb_pose_set_tasks writes for the caller;
 * the inner solver does not know about tasks.  (A target is validated as loik_amd_pose.h says whatever the kind: pass the
 * identity rotation to a position task.)
 *
 * loikb_solve_pose with tasks in force, per step and instance (everything else as loik_amd_pose.h says: the status bits, steps,
 * the idle b = 0 solves, the data object, the timing, joint limits, max_steps = 0, f32 handles with fp64 FK):
 *   - e_c as above, b_c = (gain / dt) S_c e_c   (no product with A: A_c v = S_c v_f)
 *   - reached when max_c |S_c e_c|_inf <= tol_pose
 *   - LOIKB_POSE_F_ERR is the masked task-frame error: zeros in the masked-out entries
 * A handle on which loikb_pose_set_tasks was never called, or whose specification was dropped, runs exactly what it ran before
 * this header existed.
 *
 * Lifetime.  The specification describes the A the handle holds, so every call that rewrites an A or the constraint set drops
 * it: loikb_solve_init, loikb_solve_full, loikb_add_eq_constraint, loikb_remove_eq_constraint, loikb_update_eq_constraint and
 * loikb_solve_tailored with Ai != NULL, and loikb_pose_clear_tasks (which leaves A as it is).  Afterwards loikb_pose_get_tasks
 * returns 0 and loikb_solve_pose runs the joint-frame, six-entry loop on whatever A is there.  Updates of b alone, of the
 * references, of the velocity box or of the joint limits keep it.
 */
#ifndef LOIK_AMD_TASKS_H
#define LOIK_AMD_TASKS_H

#include "loik_amd_pose.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_TASKS_VERSION 1  /* bumped whenever an entry point of this header changes */

enum { LOIKB_TASK_POSE = 0, LOIKB_TASK_POSITION = 1, LOIKB_TASK_ORIENTATION = 2 };

int loikb_tasks_version(void);

/* One task per active constraint, in loikb_active_constraint_ids order.  kinds [nc]; frames [nc][12] = iMf as
 * [R row-major (9), p (3)], NULL = the identity for all.  Host pointers.
 * A FORMULATION EDIT: the former A of every active constraint is replaced by the shared matrix A_c = S_c X_c^-1 and its b by 0,
 * through the UpdateEqConstraint path (what depends on A is invalidated as loikb_update_eq_constraint does).
 * LOIKB_ERR_STATE: before SolveInit; the handle's A is per instance (a task matrix is one per constraint for the whole batch).
 * LOIKB_ERR_ARG: nc != loikb_num_eq_c(s); kinds NULL; a kind outside 0..2; a frame rotation that is not finite and orthonormal
 * with determinant 1 (1e-9 per entry, the targets' rule); a p that is not finite.  On any error the handle is unchanged.    */
int loikb_pose_set_tasks(loikb_solver *s, int nc, const int *kinds, const double *frames);

/* drops the specification; A and b stay as they are */
int loikb_pose_clear_tasks(loikb_solver *s);

/* returns the number of tasks in force (0: none); writes min(that, cap) kinds and frames; either pointer may be NULL */
int loikb_pose_get_tasks(const loikb_solver *s, int *kinds, double *frames, int cap);

/* oMf = oMi(links[e]) * frames[e] for the resident q: out [B][n][12] (host, or device with LOIKB_OUT_DEVICE); links are the
 * caller's joint ids, frames [n][12] (host) are validated as above; frames NULL = loikb_forward_kinematics.  Independent of
 * the task specification.                                                                                                  */
int loikb_frame_placements(loikb_solver *s, const int *links, const double *frames, int n, double *out, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_TASKS_H */
