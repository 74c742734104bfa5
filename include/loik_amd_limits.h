/*
 * loik_amd_limits.h -- joint position limits for the batched pose IK of loik_amd_pose.h, and the velocity-box update of the
 * problem formulation (libloik_amd.so).
 *
 * loikb_solve_pose integrates q <- q (+) dt z for up to max_steps steps; the only inequality of the inner solve is the velocity
 * box lb <= z <= ub of SolveInit.  With joint position limits set on the handle, every step intersects that box, per instance
 * and DoF, with the velocities that keep the next configuration in range:
 *
 *     lo_j = clamp((q_lo_j - q_j) / dt, lb_j, ub_j)        hi_j = clamp((q_hi_j - q_j) / dt, lb_j, ub_j)
 *     clamp(x, a, b) = min(max(x, a), b)
 *
 * The inner solve's z is box-projected, hence inside [lo, hi]: it can only propose steps that stay in range.
 *
 * loikb_solve_pose on a handle with limits (everything loik_amd_pose.h says about the loop holds; what is added):
 *   - Before each inner solve, for every instance still running and every DoF, the box the solve sees is [lo_j, hi_j], computed
 *     in fp64 from the resident q, the call's dt and the BASE box: the velocity box in force when loikb_solve_pose was called
 *     (shared or per instance).  In an fp32 handle the pair is then rounded to fp32, as every box is.  A DoF without a finite
 *     limit keeps the base box bit for bit.  Instances that no longer run (reached / stopped) get the base box: their solve is
 *     idle work with b = 0.  q_lo <= q_hi and lb <= ub give lo <= hi for any q; a coordinate outside its range is driven back
 *     at the box's rate, not rejected.
 *   - After the integrate of a step, a limited coordinate that was inside [q_lo, q_hi] before the step is clamped to it (a
 *     kernel of its own behind k_pose_integrate, which is the one a handle without limits runs).  With z inside [lo, hi] the
 *     clamp moves it by rounding only: a few ulp in an fp64 handle, up to the fp32 rounding of the box in an fp32 handle.  It
 *     makes the guarantee exact: A LIMITED COORDINATE THAT STARTS IN RANGE IS IN RANGE, EXACTLY, IN THE RETURNED q and at
 *     every step.
 *   - While the call runs the handle is in per-instance-box mode whatever mode SolveInit chose.  On return the problem is
 *     "left as it was" in the sense of loik_amd_pose.h: the base box is back in force, in the sharing mode it had, bit for bit;
 *     on an error return after the box was touched as well.
 *   - The pose status bits, steps, err and the data-object contract (which inner solve z, iter, ... belong to) are unchanged.
 *     An instance whose target lies outside its range ends max_steps without REACHED, resting against its limits:
 *     loikb_pose_get_limit_flags tells which.
 * A handle on which limits were never set, or were cleared, runs exactly what it ran before this header existed.
 */
#ifndef LOIK_AMD_LIMITS_H
#define LOIK_AMD_LIMITS_H

#include "loik_amd_pose.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_LIMITS_VERSION 1  /* bumped whenever an entry point of this header changes */

int loikb_limits_version(void);

/* Joint position limits of the robot, honoured by every later loikb_solve_pose on this handle.
 * q_lo, q_hi: [nv] in Pinocchio's idx_v order, one pair per DoF, shared by the batch (a property of the robot).
 * -inf / +inf = no limit on that side.  Both NULL: clear the limits (the handle behaves as if never set).
 * No finite entry at all is the same as clearing.
 * A finite limit is accepted only on a DoF whose configuration coordinate is a plain scalar that loikb_integrate
 * advances by a plain sum: bounded revolute, prismatic, helical (1-DoF types), the three coordinates of a translation
 * joint, the angles of SphericalZYX, and such joints inside a composite.  A finite limit on any other DoF (free-flyer,
 * spherical, planar, unbounded (cos, sin) revolute) -> LOIKB_ERR_ARG with a loikb_last_error() that names the DoF.
 * Also LOIKB_ERR_ARG: n != nv, NaN, q_lo > q_hi, exactly one of the pointers NULL.  Host pointers.                    */
int loikb_set_joint_limits(loikb_solver *s, const double *q_lo, const double *q_hi, int n);

/* UpdateIneqConstraints(lb, ub) of the reference's problem formulation (ik-id-description-optimized.hpp:325-339), which
 * upstream reaches only through SolveInit: replaces the velocity box of the problem SolveInit set and nothing else (no
 * reset of iterates, duals, norms or constraints).  lb / ub: [B][nv], or [nv] with LOIKB_BOUNDS_SHARED (a host pointer, as
 * every shared input); LOIKB_IN_DEVICE as in solve_init.  LOIKB_ERR_STATE before SolveInit, LOIKB_ERR_INEQ_DIM for
 * nbound != nv.  Stays in force for loikb_solve / loikb_solve_tailored / loikb_solve_pose until the next SolveInit.       */
int loikb_update_ineq_constraints(loikb_solver *s, const double *lb, const double *ub, int nbound, int in_flags);

/* int [B][nv] after a loikb_solve_pose with limits set: bit 0 = the DoF's lower position limit shaped the box of the
 * instance's LAST step that moved it (lo_j > lb_j), bit 1 = the upper one (hi_j < ub_j); 0 for an instance that never
 * moved.  LOIKB_ERR_STATE when the last solve_pose ran without limits.  out: host, or device with LOIKB_OUT_DEVICE.    */
enum { LOIKB_LIMIT_LOWER = 1, LOIKB_LIMIT_UPPER = 2 };
int loikb_pose_get_limit_flags(loikb_solver *s, int *out, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_LIMITS_H */
