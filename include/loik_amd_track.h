/*
 * loik_amd_track.h -- timed pose trajectories for the batched pose IK of loik_amd_pose.h (libloik_amd.so): "keep these B robots
 * on these B trajectories", every instance in step with the clock.
 *
 * A controller, a trajectory generator or a teleoperation replay samples a desired pose every dt and wants ONE inner solve per
 * sample, a feed-forward velocity so that the robot does not lag the target, and the whole joint trajectory back: q(t_k) and
 * the velocities applied.  loikb_solve_pose_path keeps no time (every instance runs at its own pace and q is recorded only
 * where a tolerance was met); T calls of loikb_solve_pose with one step each are pure feedback, lag by one sample's motion at
 * gain 1, and leave the histories to the caller.  loikb_track_pose runs the device loop of loikb_solve_pose over T + 1 samples
 * X_0 .. X_T per instance, spaced dt apart.
 *
 * For step k = 0 .. T - 1 a running instance with the resident q_k does this:
 *
 *   1. e_c = the error of q_k against X_{k,c}: e_c = log6(oMi_c^-1 X_{k,c}) per active constraint, or the masked task-frame
 *      error of loik_amd_tasks.h when a task specification is in force.  Below (Re, pe) = oMf^-1 X_{k,c} is the desired frame
 *      seen from the actual one (oMf: the task frame, or the joint frame oMi), and R the world rotation of that frame;
 *   2. e or q not finite: the instance is STOPPED (LOIKB_POSE_ST_STOPPED).  It no longer runs or moves, and its later rows stay
 *      NaN / 0 as listed with the fields;
 *   3. ERRMAX[b][k] = max_c |e_c|_inf; <= tol_track: ONTRACK[b] counts one.  An instance is never "reached": every instance
 *      that is not stopped runs all T steps;
 *   4. the feed-forward twist f_c = [linear; angular], in the frame of e_c.  LOIKB_TRACK_FF_NONE: f_c = 0.
 *      LOIKB_TRACK_FF_DIFFERENCE, by the kind of the task:
 *        pose (and the joint-frame loop): u = log6(X_k^-1 X_{k+1}) / dt, the body twist of the desired frame, carried to the
 *                     actual frame by the action of (Re, pe): f_w = Re u_w, f_v = Re u_v + pe x (Re u_w);
 *        position:    f_v = R^T (t_{k+1} - t_k) / dt, f_w = 0;
 *        orientation: f_w = Re log3(R_k^T R_{k+1}) / dt, f_v = 0;
 *        the free-spin kinds (LOIKB_TASK_FREE_Z: the rotation about the task frame's z axis is free), by the difference rule of
 *                     the position task, in the actual frame, with w_axis the axis error of those kinds:
 *                     f_w = (w_axis(R^T R_{k+1}) - w_axis(R^T R_k)) / dt, and f_v = R^T (t_{k+1} - t_k) / dt for the kind with
 *                     a position part, f_v = 0 for the kind without.
 *      With e = 0 a frame that moves with f stays on the desired frame; for position tasks and for the free-spin kinds with
 *      gain = 1, dt f + e is exactly the error against X_{k+1};
 *   5. b_c = A_c ((gain / dt) e_c + f_c) (A shared or per instance); with tasks b_c = (gain / dt) S_c e_c + S_c f_c;
 *   6. the step of loikb_solve_pose, unchanged: the limit box if the handle has joint position limits (loik_amd_limits.h), the b
 *      edits, the tailored solve on the resident q, q <- q (+) dt z, the clamp.  With LOIKB_TRACK_REC_Z, Z[b][k] = the solve's z;
 *      with LOIKB_TRACK_REC_Q, Q[b][k + 1] = the integrated, clamped q (Q[b][0] = the starting q).  INNER[b][k] gets bit 1 when
 *      the inner solve did not converge, bit 2 when it certified primal infeasibility, bit 4 when a position-limit flag of the
 *      step (bits 1, 2 of loik_amd_limits.h) is non-zero, bit 8 when an acceleration flag of the step (bits 4, 8 of
 *      loik_amd_accel.h) is.
 *
 * After step T - 1 one judging re-target fills ERRMAX[b][T], ERR and ONTRACK against X_T; it writes no b and counts no step.
 * With LOIKB_TRACK_FF_NONE the loop is loikb_solve_pose's, bit for bit, as long as that one reaches nothing.
 *
 * Everything else is loikb_solve_pose's: instances that do not run get b = 0 and keep their q; afterwards the data object,
 * loikb_pose_get (STEPS, STATUS, ERR = against X_T, TIMING) and loikb_pose_get_limit_flags describe the call as they describe a
 * loikb_solve_pose; joint limits and task specifications on the handle are honoured through the same code; f32 handles work, with
 * the kinematics, the logarithms and every trajectory buffer in fp64.
 *
 * Samples are placements [R row-major (9), t (3)] as the targets of loikb_solve_pose, one per active constraint and sample:
 * [B][T+1][nc][12], or [T+1][nc][12] for the whole batch with LOIKB_POSE_TARGET_SHARED.  Interpolation between samples, twists
 * supplied by the caller and a dt per instance are not offered.
 *
 * Errors.  LOIKB_ERR_ARG: dt or gain not > 0 and finite, tol_track not >= 0, n_steps < 1, feedforward outside 0..1, record outside
 * 0..3, flags != 0, NULL pointers, and everything loikb_solve_pose rejects; the rotation check covers ALL T + 1 samples.
 * LOIKB_ERR_STATE as loikb_solve_pose.  On any error the handle is unchanged.  A handle that never calls an entry point of this
 * header runs exactly what it ran before this header existed.
 */
#ifndef LOIK_AMD_TRACK_H
#define LOIK_AMD_TRACK_H

#include "loik_amd_pose.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_TRACK_VERSION 1  /* bumped whenever a struct or an entry point of this header changes */

enum {
  LOIKB_TRACK_FF_NONE = 0,       /* pure feedback                                             */
  LOIKB_TRACK_FF_DIFFERENCE = 1  /* the twist from X_k to X_{k+1} over dt, rule 4.            */
};
enum {
  LOIKB_TRACK_REC_Q = 1,  /* keep q at every sample (LOIKB_TRACK_F_Q)            */
  LOIKB_TRACK_REC_Z = 2   /* keep the z of every step (LOIKB_TRACK_F_Z)          */
};

typedef struct loikb_track_params {
  double dt;          /* sample spacing and integration step, > 0, finite                    */
  double gain;        /* feedback gain: b gets (gain / dt) e, > 0, finite                    */
  double tol_track;   /* >= 0: a sample counts as "on track" when max_c |e_c|_inf <= tol     */
  int n_steps;        /* T >= 1: T steps, T + 1 samples X_0 .. X_T                            */
  int feedforward;    /* LOIKB_TRACK_FF_NONE = 0, LOIKB_TRACK_FF_DIFFERENCE = 1             */
  int record;         /* bits: LOIKB_TRACK_REC_Q = 1, LOIKB_TRACK_REC_Z = 2                 */
  int flags;          /* reserved, 0                                                         */
} loikb_track_params;

int loikb_track_version(void);

/* samples [B][T+1][nc][12], or [T+1][nc][12] with LOIKB_POSE_TARGET_SHARED; q as loikb_solve_pose; LOIKB_IN_DEVICE as there */
int loikb_track_pose(loikb_solver *s, const double *q, const double *samples, int in_flags, const loikb_track_params *p);

/* results of the last loikb_track_pose (LOIKB_ERR_STATE before the first) */
enum {
  LOIKB_TRACK_F_Q = 0,     /* double [B][T+1][nq]: q at every sample, NaN rows after a stop; LOIKB_ERR_STATE without REC_Q        */
  LOIKB_TRACK_F_Z,         /* double [B][T][nv]: z of every step, NaN rows for steps not run; LOIKB_ERR_STATE without REC_Z      */
  LOIKB_TRACK_F_ERRMAX,    /* double [B][T+1]: max_c |e_c|_inf at every sample, NaN from a stop on                              */
  LOIKB_TRACK_F_INNER,     /* int [B][T]: 1 = inner solve not converged, 2 = primal infeasible, 4 = a joint limit cut the box,
                              8 = an acceleration limit did (loik_amd_accel.h)                                                   */
  LOIKB_TRACK_F_ONTRACK,   /* int [B]: samples 0 .. T with ERRMAX <= tol_track                                                  */
  LOIKB_TRACK_F_WORST,     /* double [B]: the maximum of ERRMAX[b][1..T] over its finite entries (NaN when there is none)       */
  LOIKB_TRACK_F_WORST_AT,  /* int [B]: the first sample that attains it (-1 when there is none)                                 */
  LOIKB_TRACK_F_TIMING     /* double [4]: as LOIKB_POSE_F_TIMING                                                                */
};
int loikb_track_get(loikb_solver *s, int field, void *out, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_TRACK_H */
