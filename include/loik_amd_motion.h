/*
 * loik_amd_motion.h -- certified collision checks of joint-space motions, and the inverse of loikb_integrate (libloik_amd.so).
 *
 * loikb_clearance (loik_amd_collision.h) answers at the configurations it is handed; between two of them a thin obstacle passes
 * unnoticed.  This header checks a whole segment with a guarantee, and names the segment between two configurations when nq != nv.
 * Everything is fp64 whatever the handle's precision, as with the other pose kernels.  Pointers are host, or device with
 * LOIKB_IN_DEVICE / LOIKB_OUT_DEVICE (all inputs of a call alike, all outputs alike).  No call of this header reads the resident
 * q or the data object, and none edits either; a handle that never calls one launches exactly what it launched before this
 * header existed.
 *
 * loikb_difference.  v [n][nv] with q0 (+) v = q1 under the arithmetic of loikb_integrate (pinocchio::difference), per joint
 * type: plain subtraction on scalar coordinates and on translation / ZYX blocks; atan2 of the relative (sin, cos) for an
 * unbounded revolute joint; log3 of the relative quaternion for a spherical joint; log6(M0^-1 M1) for a free-flyer; the SE(2) log
 * for a planar joint; sub-joint by sub-joint inside a composite.  A row of q0 or q1 with an entry that is not finite yields NaN in
 * that row of v only.  A quaternion block is taken as it is, not normalised (Eigen's toRotationMatrix, as pinocchio::difference): one
 * whose norm is 1 + e costs up to about 4 e absolute in v (times |t1 - t0| in a free-flyer's linear part) at every angle, a vanishing
 * one included, so hand in unit quaternions where steps that small matter.
 *
 * loikb_motion_clearance.  Segment i is q(s) = qa_i (+) s dv_i for s in [0, 1] (pinocchio::interpolate), checked against the
 * sphere model, the world and the self pairs latched on the handle (loik_amd_collision.h) by conservative advancement.
 *
 * The motion bound, once per segment and per robot sphere a on link L:
 *
 *   Lambda_a  = sum over the joints J on the root path of L of [ lin_J + ang_J * rho_{J,a} ]
 *   rho_{J,a} = |c_a| + sum over the joints K on that path strictly below J, down to L, of ( |p_K| + tau_K )
 *
 * c_a the sphere's local centre, p_K the translation of K's fixed placement, and lin / ang / tau the linear travel, the angular
 * travel and the largest own translation of the joint over the segment (d the joint's block of dv, q_a its block of qa, t_a the
 * translation part of q_a):
 *
 *   joint                 lin          ang                    tau
 *   revolute (any kind)   0            |d|                    0
 *   prismatic             |d|          0                      max(|q_a|, |q_a + d|)
 *   helical, pitch h      |h d|        |d|                    |h| max(|q_a|, |q_a + d|)
 *   translation           ||d||        0                      max(||t_a||, ||t_a + d||)
 *   spherical             0            ||d||                  0
 *   SphericalZYX          0            |d0| + |d1| + |d2|     0
 *   free-flyer            ||d_lin||    ||d_ang||              ||t_a|| + ||d_lin||
 *   planar                ||d_xy||     |d_theta|              ||t_a|| + ||d_xy||
 *   composite             its sub-joints as a chain, with their placements (a universal joint is two revolutes)
 *
 * A sphere on link 0 has Lambda = 0.  s Lambda_a bounds the length of the path of the centre of a over [s0, s0 + s]: a joint
 * moves the centre by its own linear travel plus its angular travel times the distance of the centre from the joint's frame,
 * and rho bounds that distance over the whole segment.  tests/test_motion_numpy.py measures every row of the table against the
 * length of dense polylines of the centres.
 *
 * The advancement.  s_0 = 0.  At sample s_k every pair clearance v of the clearance query is evaluated at q(s_k): the same pairs,
 * the same formulas, the same total order (clearance, ordinal).  With m = the minimum:
 *
 *   1. m < margin + tol:     BLOCKED at s_k;
 *   2. s_k == 1:             FREE;
 *   3. k + 1 == max_evals:   UNDECIDED at s_k;
 *   4. otherwise             s_{k+1} = min(s_k + delta, 1), delta = the minimum of (v - margin) / lambda_pair over the pairs with
 *                            lambda_pair > 0; lambda_pair = Lambda_a for a world pair and Lambda_a + Lambda_b for a self pair;
 *                            delta = +inf over an empty set.
 *
 * No pair can lose more than v - margin before s_{k+1}, so the clearance is >= margin on the whole of [0, s_free) and FREE
 * certifies the closed segment.  delta >= tol / max lambda > 0: the loop ends, and max_evals bounds it in any case.  Without tol
 * the advancement converges onto a contact and never decides; that is why tol is in the contract.
 *
 * out_val[i] = { s_free, min_sampled, s_at_min }: s_free is 1, or the blocking sample, or the last sample; min_sampled the least
 * clearance over the samples taken, ties to the earliest sample, and s_at_min where it was taken.  out_info[i] = { status, evals,
 * kind, a, b }: status LOIKB_MOTION_*, evals the samples taken, (kind, a, b) the witness of min_sampled in the encoding of
 * loikb_clearance ({ LOIKB_CLR_NONE, -1, -1 } over an empty set of pairs).  A segment whose qa or dv holds an entry that is not
 * finite gets LOIKB_MOTION_INVALID, evals 0, NaN in all three values and the witness { LOIKB_CLR_NONE, -1, -1 }; the other segments
 * are not affected.
 *
 * loikb_motion_clearance_path.  Segment (b, t) runs from q_path[b][t] to q_path[b][t + 1]: the difference of consecutive samples,
 * then the check above, on the device with no host round trip.
 *
 * Errors.  LOIKB_ERR_ARG: NULL handle, n < 0 (B < 0), a NULL array with n > 0, p == NULL, a margin that is not finite, a tol that
 * is not finite or < 1e-9, max_evals outside 1 .. 65536, flags != 0, T < 2.  LOIKB_ERR_STATE: a motion check with no spheres set
 * (loikb_collision_set_spheres).  The arguments are checked first, then the state, as in loikb_clearance; after both n == 0 (B == 0) is
 * LOIKB_OK and writes nothing.
 */
#ifndef LOIK_AMD_MOTION_H
#define LOIK_AMD_MOTION_H

#include "loik_amd_collision.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_MOTION_VERSION 1  /* bumped whenever a struct or an entry point of this header changes */

/* the status of a segment */
enum { LOIKB_MOTION_FREE = 0, LOIKB_MOTION_BLOCKED = 1, LOIKB_MOTION_UNDECIDED = 2, LOIKB_MOTION_INVALID = 3 };

typedef struct loikb_motion_params {
  double margin;  /* finite: the clearance certified on [0, s_free)                       */
  double tol;     /* finite, >= 1e-9: a sample below margin + tol blocks                  */
  int max_evals;  /* 1 .. 65536: samples of one segment, at most                          */
  int flags;      /* reserved, 0                                                          */
} loikb_motion_params;

int loikb_motion_version(void);

/* q0, q1 [n][nq] -> out_v [n][nv], any n >= 0; complete on return */
int loikb_difference(loikb_solver *s, const double *q0, const double *q1, int n, int in_flags, double *out_v, int out_flags);

/* qa [n][nq], dv [n][nv], any n >= 0 -> out_val [n][3] doubles, out_info [n][5] ints; complete on return */
int loikb_motion_clearance(loikb_solver *s, const double *qa, const double *dv, int n, int in_flags, const loikb_motion_params *p,
                           double *out_val, int *out_info, int out_flags);

/* q_path [B][T][nq], T >= 2 -> out_val [B][T-1][3] doubles, out_info [B][T-1][5] ints; complete on return */
int loikb_motion_clearance_path(loikb_solver *s, const double *q_path, int B, int T, int in_flags, const loikb_motion_params *p,
                                double *out_val, int *out_info, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_MOTION_H */
