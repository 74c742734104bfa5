/*
 * loik_amd_pose.h -- batched pose IK on top of the C-ABI of loik_amd.h (libloik_amd.so): "take these B seeds to this pose".
 *
 * LoIK is a differential IK solver, the inner solve of global IK and of sampling-based planners.  loikb_solve_pose runs the
 * outer loop on the device as well: per step and instance
 *
 *     e_c = log6(oMi_c^-1 * oMdes_c)                     for every active task constraint c (links in loikb_active_constraint_ids order)
 *     b_c = A_c * (gain / dt) * e_c                      A_c: the constraint's current matrix (shared or per instance)
 *     z   = tailored Solve on the resident q             (loikb_solve_tailored(s, NULL, -1, ...): honours warm_start)
 *     q   = q (+) dt * z                                 (loikb_integrate's update, for the instances still running only)
 *
 * until max_c |e_c|_inf <= tol_pose ("reached"), e or q stops being finite ("stopped"), or max_steps steps were taken.
 * Frames: oMi is the world placement of the link (Pinocchio's data.oMi), log6 is Pinocchio's: the twist [linear; angular]
 * in the LINK frame that carries oMi to oMdes in unit time (oMdes = oMi * exp6(e)).  With A = I and gain = 1 a step asks the
 * inner solve for the link velocity that would close the whole error in dt; the velocity box of SolveInit and the inner
 * solve's tolerance decide how much of it one step gets.  FK and log6 run in fp64 whatever the handle's precision.
 *
 * Placements are [R row-major (9), t (3)] = 12 doubles, as LOIKB_F_LIMI.  Link ids are the caller's joint ids (0 = universe).
 * For a multi-DoF or composite joint the placement is that of the link carrying its body: the frame a constraint on that
 * joint acts on.
 *
 * Preconditions of loikb_solve_pose: loikb_solve_init has set the formulation (task links, A, H_ref, v_ref, velocity box), else
 * LOIKB_ERR_STATE; at least one active constraint.  The problem is left as it was but for the b_c, which hold the last inner
 * solve's (0 for the instances that did not run in it).
 * After the call:
 *   - q (LOIKB_F_Q) is the resident configuration: the last step's for running instances, the one they reached / stopped at
 *     for the others (reached instances do not move);
 *   - every inner solve runs on the whole batch: instances that no longer run solve with b = 0 and their z is discarded.  So
 *     the data object (z, yis, iter, ... of loikb_get) is that of the LAST inner solve for every instance: for an instance
 *     still running then, the solve of its final step (made at the q before that step's integrate), also when the re-target
 *     after it finds the instance reached and the call ends without another solve; for the others, a solve with b = 0 at
 *     their final q.  max_steps = 0 runs no solve: the data object is left as it was;
 *   - the pose fields below describe each instance's final q.
 * Errors: LOIKB_ERR_ARG for dt <= 0, gain <= 0, tol_pose < 0, max_steps < 0, a target rotation that is not orthonormal with
 * determinant 1 within 1e-9 per entry (or not finite), a link id out of range, NULL pointers.
 */
#ifndef LOIK_AMD_POSE_H
#define LOIK_AMD_POSE_H

#include "loik_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_POSE_VERSION 1  /* bumped whenever a struct or an entry point of this header changes */

typedef struct loikb_pose_params {
  double dt;        /* integration step of q <- q (+) dt z, > 0                        */
  double gain;      /* b = A (gain / dt) e, > 0                                        */
  double tol_pose;  /* reached when max_c |e_c|_inf <= tol_pose, >= 0                  */
  int max_steps;    /* outer steps at most, >= 0 (0: only the error of q is filled)   */
  int flags;        /* reserved, 0                                                     */
} loikb_pose_params;

/* in_flags of loikb_solve_pose: LOIKB_IN_DEVICE (targets and q are device pointers) | LOIKB_POSE_TARGET_SHARED */
enum { LOIKB_POSE_TARGET_SHARED = 32 };  /* targets [nc][12] for the whole batch; else [B][nc][12] */

int loikb_pose_version(void);

/* q: NULL = the resident configurations, else [B][nq] (host, or device with LOIKB_IN_DEVICE) replaces them first */
int loikb_solve_pose(loikb_solver *s, const double *q, const double *targets, int in_flags, const loikb_pose_params *p);

/* world placements oMi of links[0..n) for the resident q: out [B][n][12] (host, or device with LOIKB_OUT_DEVICE) */
int loikb_forward_kinematics(loikb_solver *s, const int *links, int n, double *out, int out_flags);

/* results of the last loikb_solve_pose (LOIKB_ERR_STATE before the first) */
enum {
  LOIKB_POSE_F_STEPS = 0,  /* int [B]: steps that moved the instance                                               */
  LOIKB_POSE_F_STATUS,     /* int [B]: LOIKB_POSE_ST_* bits                                                        */
  LOIKB_POSE_F_ERR,        /* double [B][nc][6]: e_c of the final q, [linear; angular]                            */
  LOIKB_POSE_F_TIMING      /* double [4]: steps run, wall ms of the call, ms in the inner solves, ms in the rest     */
};
enum {
  LOIKB_POSE_ST_REACHED = 1,         /* max_c |e_c|_inf <= tol_pose                                       */
  LOIKB_POSE_ST_NOT_CONVERGED = 2,   /* some inner solve of the instance did not converge (max_iter)     */
  LOIKB_POSE_ST_INFEASIBLE = 4,      /* some inner solve of the instance certified primal infeasibility  */
  LOIKB_POSE_ST_STOPPED = 8          /* stopped: e or q not finite                                       */
};
int loikb_pose_get(loikb_solver *s, int field, void *out, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_POSE_H */
