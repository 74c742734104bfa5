/*
 * loik_amd_step.h -- backtracking step control and stall detection for the batched pose IK of loik_amd_pose.h (libloik_amd.so).
 *
 * loikb_solve_pose takes the full step q <- q (+) dt z every time, whatever it does to the pose error: with a gain above 2 the
 * loop overshoots and diverges, next to a singular posture it runs to max_steps without progress, and nothing ends an instance
 * that is going nowhere.  With step control set on the handle, every step of loikb_solve_pose searches the step length along the
 * direction z the inner solve returned, accepts the first length that reduces the pose error enough, and can end an instance
 * whose searches keep failing.
 *
 * The merit.  Phi(q) = sum_c sum_r e_c[r]^2, where e_c is the error the loop's own re-target forms for the active constraint c:
 * with tasks on the handle (loik_amd_tasks.h, loik_amd_axis.h) the task-frame error masked by the task's kind, otherwise the
 * joint-frame log6(oMi_c^-1 oMdes_c).  fp64, accumulated c-major then r, the square rounded before the add (no fused
 * multiply-add).
 *
 * One step of a running instance, after the step's inner solve has left z:
 *
 *     Phi0 = Phi of the resident q: the numbers this step's re-target stored in the err rows
 *     trials m = 0, 1, ..., M (max_backtracks):
 *         alpha_0 = 1, alpha_{m+1} = alpha_m * shrink               (repeated multiplication)
 *         q_m = q (+) (alpha_m dt) z                                the arithmetic of loikb_integrate
 *         on a handle with joint position limits (loik_amd_limits.h) q_m is then clamped as the step's clamp does it: the
 *         limited coordinates that were in range before the step, to their range.  The step's box was built for the full dt,
 *         so a shorter step stays in range too.  Trial 0 is the q of the plain loop, bit for bit.
 *         accept the FIRST m with every entry of q_m and of its errors finite and
 *             Phi(q_m) <= (1 - sufficient * alpha_m) * Phi0          (the product sufficient * alpha_m rounded before the difference)
 *     accepted:  q <- q_m, alpha[b] = alpha_m, backtracks[b] += m, the run of failures is cleared
 *     no trial accepted:  failed[b] += 1, the run of failures grows by 1, and
 *         patience > 0 and the run has reached it:  the instance is STALLED (LOIKB_POSE_ST_STALLED): its q is left unchanged, the
 *             count the re-target gave this step is taken back (steps[b] -= 1), and it no longer runs -- like a reached instance
 *             it stays where it is and gets b_c = 0 in the later solves of the call
 *         otherwise:  the plain step, q <- q_0, alpha[b] = 1: exactly what the loop does without this header, NaN included
 *
 * The inner solve's NOT_CONVERGED and INFEASIBLE bits fold into the status of every running instance, on a failed step as well.
 * The search moves q only; the data object and the b_c afterwards are what loik_amd_pose.h says.  A failed search at the inner
 * solve's accuracy floor is common next to the target, hence the plain step as the fall-back and an explicit patience for the
 * stall verdict; patience = 0 never stalls.
 *
 * Who honours it.  loikb_solve_pose, and loikb_solve_pose_multistart through it: by that header's text a STALLED instance is
 * "without REACHED", so it is re-sampled, and it is class 1 in the selection.  Joint position limits are honoured as above.
 * Joint acceleration limits (loik_amd_accel.h) set together with step control: loikb_solve_pose returns LOIKB_ERR_STATE -- a
 * scaled step is not the velocity the braking box was built for.  loikb_solve_pose_path and loikb_track_pose return
 * LOIKB_ERR_STATE while step control is set (clear it with loikb_pose_set_step_control(s, NULL)).
 *
 * A handle on which step control was never set, or was cleared, launches exactly the kernels it launched before this header
 * existed; LOIKB_POSE_ST_STALLED is then never set.
 */
#ifndef LOIK_AMD_STEP_H
#define LOIK_AMD_STEP_H

#include "loik_amd_pose.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_STEP_VERSION 1  /* bumped whenever an entry point of this header changes */

typedef struct loikb_step_params {
  double shrink;       /* in (0, 1): alpha_{m+1} = alpha_m * shrink, alpha_0 = 1           (default 0.5)  */
  double sufficient;   /* in [0, 1): accept when Phi(q_m) <= (1 - sufficient * alpha_m) Phi0 (default 1e-4) */
  int max_backtracks;  /* M in 0..30: trials m = 0..M                                       (default 6)    */
  int patience;        /* >= 0: STALLED after this many failed searches in a row; 0 = never (default 0)    */
  int flags;           /* reserved, 0 */
} loikb_step_params;

/* a new bit in the word of LOIKB_POSE_F_STATUS: `patience` searches in a row accepted no trial; the instance was left where it was */
enum { LOIKB_POSE_ST_STALLED = 16 };

int loikb_step_version(void);

/* Step control for every later loikb_solve_pose on this handle.  p = NULL clears it (the handle behaves as if never set).
 * LOIKB_ERR_ARG, and nothing changes: shrink outside (0, 1), sufficient outside [0, 1), NaN, max_backtracks outside 0..30,
 * patience < 0, flags != 0.                                                                                              */
int loikb_pose_set_step_control(loikb_solver *s, const loikb_step_params *p);

/* returns 1 and fills *out (if not NULL) when step control is set, 0 when it is not */
int loikb_pose_get_step_control(const loikb_solver *s, loikb_step_params *out);

/* results of the last loikb_solve_pose, which must have run with step control (LOIKB_ERR_STATE otherwise) */
enum { LOIKB_STEP_F_ALPHA = 0,   /* double [B]: alpha of the last step that moved the instance, 0 if none */
       LOIKB_STEP_F_BACKTRACKS,  /* int [B]: sum over accepted searches of the accepted m                */
       LOIKB_STEP_F_FAILED };    /* int [B]: searches in which no trial was accepted                     */

/* out: host, or device with LOIKB_OUT_DEVICE */
int loikb_step_get(loikb_solver *s, int field, void *out, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_STEP_H */
