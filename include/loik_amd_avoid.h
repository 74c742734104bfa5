/*
 * loik_amd_avoid.h -- collision avoidance in every pose loop, and the gradient of a pair clearance (libloik_amd.so).
 *
 * loik_amd_collision.h and loik_amd_motion.h report: they say how far a configuration or a recorded motion is from the world and
 * from the robot itself.  This header makes the pose loops (loikb_solve_pose, loikb_solve_pose_path, loikb_track_pose,
 * loikb_solve_pose_multistart) keep away from what those headers measure.  The solver's only inequality is the velocity box
 * lb <= z <= ub, and it stays the only one: with the latch of this header set, the box of every inner solve is narrowed on the
 * device from the resident q, after the position limits (loik_amd_limits.h) and the acceleration limits (loik_amd_accel.h) have
 * had their say, by a first-order velocity damper.  No engine changes; a handle that never sets the latch, or cleared it,
 * launches exactly what it launched before this header existed.  All arithmetic is fp64 from fp64 q, whatever the handle's
 * precision.
 *
 * The gradient of a pair clearance.  c is the world centre of robot sphere a on link L, Jc the 3 x nv linear part of the
 * LOIKB_JAC_LOCAL_WORLD_ALIGNED Jacobian (loikb_frame_jacobians) of a frame at c on L, in the caller's nv order.  With the unit
 * normal n, the row g [nv] has d(clearance)/dt = g . z under loikb_integrate:
 *
 *   world sphere (centre w)   n = (c - w) / |c - w|, or 0 when |c - w| == 0;  g = n^T Jc
 *   world box (R, t, h)       p = R^T (c - t), d = |p| - h, sgn(x) = +1 for x >= 0 else -1.  If any d_k > 0:
 *                             n = R (sgn(p) o max(d, 0)) / || max(d, 0) ||; otherwise n = R (sgn(p_k) e_k) with k the lowest index
 *                             that attains max d;  g = n^T Jc
 *   self pair (a, b)          n = (c_a - c_b) / |c_a - c_b|, or 0 at coincidence;  g = n^T (Jc_a - Jc_b); the columns of DoFs on
 *                             both root paths are exactly 0
 *
 * m is the number of DoFs on the pair's path: the root path of L for a world pair, the symmetric difference of the two root
 * paths for a self pair.  A sphere on link 0 has m = 0 against the world and constrains nothing.
 *
 * The constraints of one configuration.  Every robot sphere a has at most two: its nearest world object, the minimum in the
 * total order (clearance, ordinal) of loikb_clearance over all world spheres and boxes against a, and its nearest listed self
 * partner, over the listed self pairs whose first index is a.  A constraint is active when its clearance d < d_influence: at
 * most 2 ns constraints, a table that cannot overflow.  The partner of a sphere is reported as the index of the world sphere,
 * nws + the index of the world box, or the index of the other robot sphere; -1 over an empty set.
 *
 * The box.  For an active constraint k, r_k = kappa max(d_k - d_safe, 0) / dt, and for DoF j
 *
 *   g_kj > 0   lo >= -r_k / (m_k g_kj)         g_kj < 0   hi <= r_k / (m_k |g_kj|)         g_kj == 0  nothing
 *
 * A_lo_j is the largest lower candidate (-inf without one), A_hi_j the least upper one (+inf), so A_lo_j <= 0 <= A_hi_j.  With
 * [lo_j, hi_j] the step's interval after position and acceleration limits (the base box when neither is set) the solve sees
 * lo'_j = clamp(A_lo_j, lo_j, hi_j), hi'_j = clamp(A_hi_j, lo_j, hi_j), the clamp of loik_amd_limits.h.  An fp32 handle rounds the
 * pair toward zero, not to nearest: inward, so the inscribed box stays inscribed.
 *
 * What this guarantees, and what it does not.
 *   - If every [lo_j, hi_j] contains 0, every z of the new box has g_k . z >= -r_k for every active k: each DoF may spend 1 / m_k
 *     of the approach budget.  To first order in dt |z|, d_k(next) - d_safe >= (1 - kappa) (d_k - d_safe).
 *   - At or below d_safe no DoF may approach.  Retreat is free, not forced.
 *   - A box inscribed in a half-space is more conservative than the half-space: it forbids some sliding motions that the linear
 *     inequality g_k . z >= -r_k would allow.  That is the price of leaving the engines alone.
 *   - It is a first-order rule.  The certificate of a recorded path remains loikb_motion_clearance_path.
 *   - Where a position limit drives an out-of-range coordinate back, its interval excludes 0; the limit wins there.
 *   - A row of q that is not finite gets the base interval and contributes NaN to the reported clearance.
 *   - Only the nearest world object and the nearest self partner of a sphere constrain it; a second object inside d_influence is
 *     seen when it becomes the nearest.
 *
 * loikb_clearance_gradient is loikb_clearance plus the gradient row of the witness pair: out_min and out_witness as there (the
 * same total order over the same values: the same bits, but for a model of more than about 600 joints and sphere-carrying links
 * together, where the two calls round the placements differently and agree to a few ulp), out_grad [n][nv]; zeros for an empty pair
 * set, a NaN row for a q that is not finite.
 * loikb_avoid_box is the rule above as a pure query with explicit parameters, a shared [lb, ub] and no rounding.
 * loikb_avoid_set latches the parameters for every later pose loop on the handle; such a loop leaves the three results of
 * loikb_avoid_get_result.  At most LOIKB_AVOID_MAX_SPHERES spheres: the table, the list and the placements of every joint of one
 * configuration live in one wavefront's share of the LDS.
 *
 * Errors.  Arguments are checked first, then state.  LOIKB_ERR_ARG: NULL handle or a NULL output with n > 0, a negative n, q = NULL
 * with n != B, flags != 0, a d_safe or d_influence that is not finite, d_influence <= d_safe, kappa outside (0, 1], a dt that is
 * not finite or not > 0, a NaN in lb / ub or lb > ub, a field that is not LOIKB_AVOID_F_*.  LOIKB_ERR_STATE: no spheres set, more
 * than LOIKB_AVOID_MAX_SPHERES spheres (loikb_avoid_set and loikb_avoid_box; loikb_collision_set_spheres while the latch is set,
 * which also refuses to clear the spheres), q = NULL with no configurations resident, the result getter when the last pose loop
 * ran without the latch.  n == 0 is LOIKB_OK and writes nothing.  On any error nothing of the handle changes.
 */
#ifndef LOIK_AMD_AVOID_H
#define LOIK_AMD_AVOID_H

#include "loik_amd_motion.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_AVOID_VERSION 1  /* bumped whenever a struct or an entry point of this header changes */

#define LOIKB_AVOID_MAX_SPHERES 256

typedef struct loikb_avoid_params {
  double d_safe;       /* finite: no DoF may approach at or below this clearance                */
  double d_influence;  /* finite, > d_safe: a constraint is active below this clearance         */
  double kappa;        /* 0 < kappa <= 1: the share of d - d_safe one step may spend             */
  int flags;           /* reserved, 0 */
} loikb_avoid_params;

int loikb_avoid_version(void);

/* q [n][nq] (host, or device with LOIKB_IN_DEVICE), any n >= 0; q = NULL: the resident q, n must equal the batch.
 * out_min [n][3] doubles, out_witness [n][3] ints, out_grad [n][nv] doubles (host, or all device with LOIKB_OUT_DEVICE). */
int loikb_clearance_gradient(loikb_solver *s, const double *q, int n, int in_flags, double *out_min, int *out_witness, double *out_grad,
                             int out_flags);

/* The latch of every later pose loop on this handle.  p = NULL clears it (the handle behaves as if never set). */
int loikb_avoid_set(loikb_solver *s, const loikb_avoid_params *p);

/* returns 1 and fills *out (if not NULL) when the latch is set, 0 when it is not */
int loikb_avoid_get(const loikb_solver *s, loikb_avoid_params *out);

/* q as above; lb, ub [nv] (host) shared by the rows; out_lo, out_hi [n][nv] doubles; out_pairs [n][ns][2] doubles = each sphere's
 * nearest-world and nearest-self clearance (+inf over an empty set); out_partner [n][ns][2] ints = the partner of each, or -1
 * (host, or all four device with LOIKB_OUT_DEVICE; none may be NULL when n > 0). */
int loikb_avoid_box(loikb_solver *s, const double *q, int n, int in_flags, double dt, const double *lb, const double *ub,
                    const loikb_avoid_params *p, double *out_lo, double *out_hi, double *out_pairs, int *out_partner, int out_flags);

/* results of the last pose loop, which ran with the latch (LOIKB_ERR_STATE otherwise) */
enum { LOIKB_AVOID_F_MIN_SEEN = 0,   /* double [B]: the least overall clearance at the start of any step the instance ran (+inf: none) */
       LOIKB_AVOID_F_ACTIVE_STEPS,   /* int [B]: the steps in which a constraint narrowed the instance's box                         */
       LOIKB_AVOID_F_FLAGS };        /* int [B][nv]: bit 0 = lower side narrowed, bit 1 = upper side narrowed, at the instance's last
                                        step that moved it (the convention of loikb_pose_get_limit_flags)                            */
/* With step control (loik_amd_step.h) the box is narrowed before the search, so a step whose search ends LOIKB_POSE_ST_STALLED -- which
 * neither moves the instance nor counts in its steps -- still counts in ACTIVE_STEPS and MIN_SEEN, and FLAGS are those of that step. */
int loikb_avoid_get_result(loikb_solver *s, int field, void *out, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_AVOID_H */
