/*
 * loik_amd_blend.h -- certified parabolic blends: retiming of joint-space paths through their corners (libloik_amd.so).
 *
 * loikb_retime_paths (loik_amd_retime.h) stays on the segments of its input and therefore stops at every waypoint.  loikb_blend_paths
 * replaces a corner by a parabola that it certifies itself, with the motion bound and the conservative advancement of
 * loik_amd_motion.h, and runs through it without a stop; a corner whose parabola it cannot certify stops as before.  Everything is fp64
 * whatever the handle's precision.  v_max and a_max are host arrays [nv] in idx_v order, copied by the call; every other pointer is
 * host, or device with LOIKB_IN_DEVICE / LOIKB_OUT_DEVICE (all inputs of a call alike, all outputs alike); a call is complete on return.
 * The call reads neither the resident q nor the data object and edits neither; it needs the sphere model of loik_amd_collision.h; a
 * handle that never calls it launches exactly what it launched before this header existed.
 *
 * The certificate.  Every sample, and the continuous trajectory between the samples, lies on one of two things.  One is a
 * sub-interval of an input segment, q_k (+) s dv_k with s in [0, 1]: this call does not check those, so they are certified if the
 * input was, exactly as in loik_amd_retime.h.  The other is a blend curve that this call certified at a clearance >= margin over the
 * whole of u in [0, 1].  Where a leg meets a blend the two agree to rounding, not bit for bit.  The result is not time-optimal: it is
 * the fastest trajectory on this geometry with blends traversed at a constant rate.
 *
 * The geometry.  Path b of q_path [B][T][nq] has L = len[b] waypoints (len == NULL: T everywhere), as in loik_amd_retime.h.
 * dv_k = difference(q_k, q_{k+1}), two finite rows that are equal entry by entry give 0 exactly -- and so does, joint by joint, a
 * joint (a sub-joint of a composite) whose own coordinates are equal entry by entry in the two rows: that is what "exactly zero" below
 * rests on -- and |dv_k| is the norm of loikb_path_length (the squares summed in DoF order).  Corner k = 1 .. L - 2 with half-length l
 * is the curve, in the chart at q_k,
 *
 *   q(u) = q_k (+) w(u),   w(u) = (1 - u)^2 P0 + u^2 P2,   u in [0, 1]
 *   P0 = -r_in dv_{k-1},   P2 = r_out dv_k,   r_in = l / |dv_{k-1}|,   r_out = l / |dv_k|
 *
 * integrated with the arithmetic of the pose loops' integrator.  It leaves the incoming leg at s = 1 - r_in and joins the outgoing leg
 * at s = r_out, tangent to both, and |w(u)| <= l: every point of it is within l of the corner in the joint-space norm.
 * Try i = 0 .. max_tries - 1 uses l_i = 2^-i min(reach, |dv_{k-1}| / 2, |dv_k| / 2);
 * the first try whose curve is certified FREE is taken, and if none is the corner stops as in loik_amd_retime.h.  Corners are
 * independent of one another: the halves give r_out,k + r_in,k+1 <= 1.
 *
 *   When a corner is blendable.  A 1-DoF joint, a translation block and a SphericalZYX block are plain: the coordinate or angle is
 *   q_k + w.  A spherical, free-flyer or planar block is blendable only when its block of dv_{k-1} or its block of dv_k is exactly
 *   zero: it then moves along one one-parameter ray.  Composites are judged sub-joint by sub-joint.  Otherwise the corner is
 *   LOIKB_BLEND_COUPLED and stops.  A corner with |dv_{k-1}| == 0 or |dv_k| == 0 is LOIKB_BLEND_ZERO_LEG and stops (that is looked at
 *   first).
 *
 *   The motion bound.  Per joint J, with lin, ang and tau of the table of loik_amd_motion.h evaluated for the segments (q_k, P0) and
 *   (q_k, P2):
 *
 *     lin_J = 2 max(lin_J(P0), lin_J(P2)),  ang_J = 2 max(ang_J(P0), ang_J(P2)),  tau_J = max(tau_J(q_k, P0), tau_J(q_k, P2))
 *     Lambda_a = sum over the joints J on the root path of [ lin_J + ang_J rho_{J,a} ]      (rho as in loik_amd_motion.h, with this tau)
 *
 *   A composite counts as the chain of its sub-joints, and so does a SphericalZYX joint, which the device model holds as three
 *   revolute joints about z, y and x: ang is taken angle by angle, the sum over i of 2 max(|P0_i|, |P2_i|), which is at least
 *   2 max(|P0_0| + |P0_1| + |P0_2|, |P2_0| + |P2_1| + |P2_2|).
 *
 *   w'(u) = -2 (1 - u) P0 + 2 u P2 is a convex combination of -2 P0 and 2 P2, so every norm and every ZYX sum of a block of w'(u) is at
 *   most 2 max(|P0|, |P2|) of that block; and the coordinates stay in the triangle (q_k + P0, q_k, q_k + P2), on which a norm is largest
 *   at a corner.  So du Lambda_a bounds the length of the path of the centre of sphere a over [u, u + du].
 *   tests/test_blend_numpy.py measures it against dense polylines of the centres.
 *
 *   The advancement is that of loik_amd_motion.h with s -> u, q(u) as above and lambda from this Lambda: the same pairs, formulas and
 *   total order, and the same four rules -- BLOCKED below margin + tol, FREE at u == 1, UNDECIDED at max_evals, else a step by the
 *   minimum of (v - margin) / lambda_pair.
 *
 * The timing.  A_k = 1 / ca_k and V_k = 1 / cv_k per leg as in loik_amd_retime.h.  A blended corner is traversed at a constant rate
 * du/dt = w_k: its velocity is w'(u) w_k and its acceleration the constant 2 (P0 + P2) w_k^2.  The rate is at most
 *
 *   1 / w_max = max( sqrt(max_j 2 |P0 + P2|_j / a_max_j),  max_j 2 |P0_j| / v_max_j,  max_j 2 |P2_j| / v_max_j )
 *
 * The s-rate of the leg where it meets the blend is 2 r_in w_k on entry and 2 r_out w_k on exit; a stopped corner and the two ends of
 * the path have rate 0 and r = 0.  The straight piece of leg k has the s-length l_k = 1 - r_out,k - r_in,k+1.  One forward pass in path
 * order lowers w_{k+1} until v_in,k+1^2 <= v_out,k^2 + 2 A_k l_k, one backward pass lowers w_k until v_out,k^2 <= v_in,k+1^2 + 2 A_k l_k
 * (w = sqrt(bound) / (2 r) where it is lowered): the largest feasible rates.  Each straight piece is then the time-optimal profile from
 * v0 to v1: accelerate at A to v_p = max(min(V, sqrt((2 A l + v0^2 + v1^2) / 2)), v0, v1) (the outer max guards a rounding only), cruise,
 * decelerate at A; t_1 = (v_p - v0) / A, t_3 = (v_p - v1) / A, s_1 = (v_p^2 - v0^2) / (2 A), s_3 = (v_p^2 - v1^2) / (2 A),
 * D = t_1 + (l - s_1 - s_3) / v_p + t_3.  A piece with l == 0, and a leg with dv_k == 0, has duration 0.  A blend has duration 1 / w_k.
 *
 * The pieces in path order are leg 0, blend 1, leg 1, ..., leg L - 2: piece 2 k is leg k and piece 2 k - 1 is corner k (duration 0
 * when it stops), 2 L - 3 in all.  Their starts are summed in that order, in doubles; D is the sum, n_samples = ceil(D / dt) + 1,
 * saturated at 2^31 - 1 as in loik_amd_retime.h.  Sample i sits at t = i dt.  If t >= D it is the last waypoint bit for bit with velocity 0.
 * Otherwise its piece is the last one with t_start <= t, and tau = t - t_start:
 *
 *   on a leg     tau < t_1:          sigma = v0 tau + (1/2) A tau^2,            sdot = v0 + A tau
 *                tau <= D_p - t_3:   sigma = s_1 + v_p (tau - t_1),             sdot = v_p
 *                after that:         sigma = l - (v1 r + (1/2) A r^2),          sdot = v1 + A r,   r = max(D_p - tau, 0)
 *                out_traj = q_k (+) (r_out,k + sigma) dv_k (a parameter of 0: q_k bit for bit), out_vel = sdot dv_k
 *   on a blend   u = min(w_k tau, 1),  out_traj = q_k (+) w(u),  out_vel = w'(u) w_k
 *
 * Rows i >= n_samples repeat the last waypoint with velocity 0.  There is no SNAP in this version.
 *
 * Outputs.  out_traj [B][S][nq] or NULL for a timing-only call (S is then ignored and TRUNCATED never set), out_vel [B][S][nv] or
 * NULL, out_duration [B] = D, out_info [B][4] = { n_samples, L, corners TAKEN, flags } with LOIKB_BLEND_TRUNCATED / INVALID / SKIPPED
 * in the meaning of the flags of loik_amd_retime.h, and (each may be NULL)
 *
 *   out_corner      [B][T-2][5] doubles = { l taken or 0, r_in, r_out, w, min_sampled of the deciding try }; row c is corner c + 1.  r_in,
 *                   r_out and w are 0 unless the corner is TAKEN; min_sampled is 0 when no try was made.
 *   out_corner_info [B][T-2][6] ints = { status, tries made, evals summed over the tries, witness kind, a, b }, the witness of the
 *                   deciding try's min_sampled in the encoding of loikb_clearance, { LOIKB_CLR_NONE, -1, -1 } when no try was made.
 *                   The deciding try is the one taken, else the last one.
 *   out_piece       [B][2T-3][4] doubles = { t_start, duration, v0 or w, v1 or w }; zeros for a piece of duration 0 and beyond the path's
 *                   pieces.
 *
 * Rows of corners beyond L - 2 are { 0 .. } and { LOIKB_BLEND_OFF, 0, 0, LOIKB_CLR_NONE, -1, -1 }.  An INVALID or SKIPPED path has NaN in
 * its duration, out_corner, out_piece and sample rows, OFF rows in out_corner_info and 0 in n_samples and the corner count; the other
 * paths of the batch are not affected.  T == 2 has no corner: out_corner and out_corner_info are then not written.
 *
 * Errors.  LOIKB_ERR_ARG: NULL handle, T < 2, T >= 2^30, B < 0, B * T >= 2^31, a NULL q_path with B > 0, a NULL v_max, a_max, p,
 * out_duration or out_info, a limit that is not finite or <= 0, a margin that is not finite, a tol that is not finite or < 1e-9, a reach or a dt that
 * is not finite or <= 0, max_evals outside 1 .. 65536, max_tries outside 0 .. 16, flags != 0, out_traj given with S < 1 or with
 * B * S >= 2^31, out_vel given without out_traj, out_traj == q_path.  LOIKB_ERR_STATE: no spheres set (loikb_collision_set_spheres).  The
 * arguments are checked first, then the state; after both B == 0 is LOIKB_OK and writes nothing.  A call that fails writes nothing.
 */
#ifndef LOIK_AMD_BLEND_H
#define LOIK_AMD_BLEND_H

#include "loik_amd_retime.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_BLEND_VERSION 1  /* bumped whenever a struct or an entry point of this header changes */

#define LOIKB_BLEND_TRUNCATED 1  /* out_info[b][3] */
#define LOIKB_BLEND_INVALID 2
#define LOIKB_BLEND_SKIPPED 4

/* the status of a corner, out_corner_info[b][c][0] */
enum {
  LOIKB_BLEND_TAKEN = 0,      /* a try was certified FREE                  */
  LOIKB_BLEND_BLOCKED = 1,    /* the last try was blocked                  */
  LOIKB_BLEND_UNDECIDED = 2,  /* the last try was undecided                */
  LOIKB_BLEND_COUPLED = 3,    /* a coupled joint moves on both legs        */
  LOIKB_BLEND_ZERO_LEG = 4,   /* an adjacent leg is zero                   */
  LOIKB_BLEND_OFF = 5         /* max_tries == 0, or the corner is beyond L - 2 */
};

typedef struct loikb_blend_params {
  double margin;  /* finite: the clearance certified on every blend taken           */
  double tol;     /* finite, >= 1e-9: a sample below margin + tol blocks a try      */
  double reach;   /* finite, > 0: the largest half-length of a blend                */
  double dt;      /* the sample period, finite and > 0                              */
  int max_evals;  /* 1 .. 65536: samples of one try, at most                        */
  int max_tries;  /* 0 .. 16: halvings of the half-length; 0 stops at every corner  */
  int flags;      /* reserved, 0                                                    */
} loikb_blend_params;

int loikb_blend_version(void);

/* q_path [B][T][nq]; len [B] ints or NULL (= T everywhere); v_max, a_max [nv] on the host.
 * out_traj [B][S][nq] or NULL (timing only); out_vel [B][S][nv] or NULL; out_duration [B]; out_info [B][4] ints;
 * out_corner [B][T-2][5], out_corner_info [B][T-2][6] ints, out_piece [B][2T-3][4], each or NULL.                  */
int loikb_blend_paths(loikb_solver *s, const double *q_path, const int *len, int B, int T, int in_flags,
                      const double *v_max, const double *a_max, const loikb_blend_params *p, int S,
                      double *out_traj, double *out_vel, double *out_duration, int *out_info,
                      double *out_corner, int *out_corner_info, double *out_piece, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_BLEND_H */
