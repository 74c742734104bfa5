/*
 * loik_amd_accel.h -- joint acceleration limits for the batched pose IK of loik_amd_pose.h, with position limits that are
 * anticipated by braking (libloik_amd.so).
 *
 * The pose loops (loikb_solve_pose, loikb_solve_pose_path, loikb_track_pose) integrate q <- q (+) dt z.  Without this header the
 * only bounds on a step are the velocity box of SolveInit and the position-limit box of loik_amd_limits.h,
 * clamp((q_lo - q) / dt, lb, ub): nothing bounds the change of z from one step to the next, and a joint may run into its position
 * limit at full speed and stop in one sample.  With acceleration limits set on the handle, every step of a pose loop sees this box
 * instead, per running instance and DoF j:
 *
 *     a_j  the acceleration limit (+inf: none), s = a_j dt
 *     zp   the velocity applied to this instance in its previous step; 0 at the start of a loop unless
 *          loikb_accel_set_start_velocity gave one
 *     q, q_lo, q_hi, lb, ub   as in loik_amd_limits.h; position limits only on the DoFs that may carry one there
 *
 *     vmax(d): the largest velocity from which the joint still stops within distance d, braking by s per step
 *       d < 0 or s = inf:  d / dt                                     (s = inf gives the rule of loik_amd_limits.h)
 *       else: n = floor((sqrt(1 + 8 d / (dt s)) - 1) / 2), then corrected in integers:
 *               while n > 0 and dt s n (n + 1) / 2 > d: n -= 1
 *               while dt s (n + 1) (n + 2) / 2 <= d:    n += 1
 *             vmax = (d / dt + s n (n + 1) / 2) / (n + 1)
 *       (d = inf gives inf.  Guards for numbers no drive has: with dt s below the normal range of a double the rule is d / dt; an
 *        estimate n >= 2^31 is used uncorrected.)
 *
 *     U  =  vmax(q_hi - q)   (+inf without an upper position limit)
 *     Lw = -vmax(q - q_lo)   (-inf without a lower one)
 *     hi = min(max(U,  zp - s), zp + s)          the acceleration window wins where the position term cannot be met
 *     lo = min(max(Lw, zp - s), zp + s);   lo = min(lo, hi)
 *     lo = clamp(lo, lb, ub);  hi = clamp(hi, lb, ub)                 the base box as in loik_amd_limits.h
 *
 * all in fp64; in an fp32 handle the pair is then rounded to fp32, as every box is.
 *
 * Why.  The integrator is q += dt z.  Braking from z by s per step travels dt (z + (z - s) + (z - 2 s) + ...), which is piecewise
 * linear and convex in z with breakpoints at z = n s; vmax is its inverse.  Take a state whose zp is inside the base box and which
 * can still brake in time (zp - s <= U, zp + s >= Lw): every z in [lo, hi] leads to such a state again, so lo <= hi always, and
 *   - |z_k - z_{k-1}| <= s for consecutive steps of a running instance;
 *   - a limited coordinate that starts in range at rest stays in range, whatever the inner solve picks inside the box;
 *   - the joint arrives at a limit with a velocity it can stop from.
 * The clamp after the integrate (loik_amd_limits.h) stays and makes containment exact.
 *
 * WHAT IS GUARANTEED, AND WHAT IS NOT.
 *   - The acceleration bound holds between consecutive steps of a running instance.  In an fp32 handle each edge of the box is
 *     rounded to fp32 once, so the bound there is s + 2^-22 (|zp| + s).
 *   - A loikb_solve_pose or loikb_solve_pose_path instance that reaches its target stops where it is, as it does without this
 *     header: its last velocity is not ramped down.  loikb_track_pose, where nothing is ever "reached", is the loop whose whole
 *     recorded z obeys the bound.
 *   - A start velocity outside the base box, or a state that can no longer brake in time, is led back at the rate s.  It is not
 *     rejected.
 *   - Instances that no longer run get the base box, as in loik_amd_limits.h, and their velocity state is set to 0.
 *
 * The limit flags (loikb_pose_get_limit_flags, valid after a loop that ran with either kind of limit) are those of the last step
 * that moved the instance, in the same [B][nv] word:
 *     LOIKB_LIMIT_LOWER       = 1   the lower position limit shaped the box: Lw > lb and Lw >= zp - s
 *     LOIKB_LIMIT_UPPER       = 2   the upper position limit shaped the box: U < ub and U <= zp + s
 *     LOIKB_LIMIT_ACCEL_LOWER = 4   zp - s > lb and zp - s > Lw
 *     LOIKB_LIMIT_ACCEL_UPPER = 8   zp + s < ub and zp + s < U
 * With a_j = inf everywhere bits 1 and 2 are those of loik_amd_limits.h.  LOIKB_TRACK_F_INNER (loik_amd_track.h) gains bit 8: an
 * acceleration flag of the step is non-zero; its bit 4 keeps its meaning (a position flag is non-zero).
 *
 * Everything else is unchanged, bit for bit: the contracts of the pose loops, the base box back in force on every return path
 * (the handle is in per-instance-box mode while a loop with either kind of limit runs), the data object, LOIKB_POSE_F_*, and a
 * handle with position limits only.  A handle on which acceleration limits were never set, or were cleared, launches exactly the
 * kernels it launched before this header existed.  loikb_solve_pose_multistart on a handle with acceleration limits returns
 * LOIKB_ERR_STATE: its seeds are teleported between rounds, a rate limit means nothing there.
 */
#ifndef LOIK_AMD_ACCEL_H
#define LOIK_AMD_ACCEL_H

#include "loik_amd_limits.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_ACCEL_VERSION 1  /* bumped whenever an entry point of this header changes */

int loikb_accel_version(void);

/* the two flag bits this header adds to the word of loikb_pose_get_limit_flags */
enum { LOIKB_LIMIT_ACCEL_LOWER = 4, LOIKB_LIMIT_ACCEL_UPPER = 8 };

/* Joint acceleration limits of the robot, honoured by every later pose loop on this handle.
 * a_max: [nv] in Pinocchio's idx_v order, shared by the batch; entries > 0, +inf = no limit on that DoF.  NULL, or no finite
 * entry at all: clear the limits (the handle behaves as if never set).  A finite limit is accepted on any DoF: velocity space is
 * a plain vector.  LOIKB_ERR_ARG: n != nv, NaN, an entry <= 0.  Host pointer.                                              */
int loikb_set_joint_accel_limits(loikb_solver *s, const double *a_max, int n);

/* The velocity the instances move with when the next pose loop on this handle starts: zp of its first step, then forgotten
 * (whether or not that loop runs with acceleration limits).  v0: [B][nv], finite; host, or device with LOIKB_IN_DEVICE.
 * NULL: zero, the default.                                                                                                  */
int loikb_accel_set_start_velocity(loikb_solver *s, const double *v0, int in_flags);

/* double [B][nv] after a pose loop with acceleration limits set: the velocity applied in the last step that moved each
 * instance; 0 for an instance that never moved and for one that reached or stopped.  Handing it to
 * loikb_accel_set_start_velocity continues a loikb_track_pose where the last one ended.  LOIKB_ERR_STATE when the last pose
 * loop ran without acceleration limits (or there was none).  out: host, or device with LOIKB_OUT_DEVICE.                     */
int loikb_accel_get_velocity(loikb_solver *s, double *out, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_ACCEL_H */
