/*
 * loik_amd_retime.h -- time-optimal retiming of joint-space paths (libloik_amd.so).
 *
 * loikb_motion_clearance_path (loik_amd_motion.h) certifies a path and loikb_shortcut_paths (loik_amd_shortcut.h) shortens one; both end
 * in a list of waypoints with no time attached.  loikb_retime_paths turns such a path into samples q(t), v(t) at a fixed period dt that
 * respect a velocity limit and an acceleration limit per DoF, on the device, a wavefront per path from its first segment to its last
 * sample.  Everything is fp64 whatever the handle's precision.  v_max and a_max are host arrays [nv] in idx_v order, shared by the
 * batch and copied by the call (as a_max of loikb_set_joint_accel_limits); every other pointer is host, or device with LOIKB_IN_DEVICE /
 * LOIKB_OUT_DEVICE (all inputs of a call alike, all outputs alike); a call is complete on return.  The call reads neither the resident q
 * nor the data object and edits neither; it needs no spheres; a handle that never calls it launches exactly what it launched before
 * this header existed.
 *
 * What the result is.  Every sample lies on a segment of the input: q(t) = q_k (+) s dv_k with s in [0, 1], so a path whose segments
 * were certified MOTION_FREE stays certified, and no new check is needed.  The trajectory is time-optimal among those that follow the
 * path exactly under the two limits.  It stops at every waypoint: a trajectory that stays on a piecewise-straight path has no other
 * way round a corner, and that is the price of following the path exactly.  Corner blending leaves the certified geometry and is out
 * of scope.
 *
 * The rule.  Path b of q_path [B][T][nq] has L = len[b] waypoints, its leading rows (len == NULL: T everywhere); the rows after them
 * are not read.
 *
 *   Segment timing.  Segment k < L - 1 has dv_k = difference(q_k, q_{k+1}) in the arithmetic of loikb_difference; two rows that are
 *   finite and equal entry by entry give dv_k = 0 exactly (loikb_path_length's rule).  cv = max_j |dv_kj| / v_max_j and
 *   ca = max_j |dv_kj| / a_max_j.  The path parameter s runs over [0, 1] from rest to rest with the acceleration A = 1 / ca:
 *
 *     triangular, ca >= cv cv:  D_k = 2 sqrt(ca),   t_acc = sqrt(ca),  peak sdot = 1 / sqrt(ca)
 *     trapezoid,  otherwise  :  D_k = cv + ca / cv, t_acc = ca / cv,   peak sdot = 1 / cv
 *
 *   A segment with dv_k = 0 (cv or ca not above 0) has duration 0, a record of zeros in out_seg, and is never sampled.
 *
 *   LOIKB_RETIME_SNAP.  A positive duration is stretched to D'_k = dt n_k with n_k = ceil(D_k / dt).  The acceleration stays A, the
 *   peak is lowered to sdot' = 2 / (D' + sqrt(max(D' D' - 4 ca, 0))), and t_acc' = sdot' ca.  Segment starts are the integer tick sums
 *   N_k = n_0 + ... + n_{k-1}, t_start_k = dt N_k, so every waypoint falls on a sample: sample N_k is q_k bit for bit.  (In a tick sum
 *   one segment counts for at most 2^31 ticks: no sample index reaches past such a segment.)  Without the flag t_start_k is the sum of
 *   the durations before k in path order, in doubles.
 *
 *   Totals.  D is the sum of the durations in path order (with SNAP dt N_{L-1}).  n_samples = ceil(D / dt) + 1, with SNAP
 *   N_{L-1} + 1; a count that would pass 2^31 - 1 saturates there, and the path is then TRUNCATED whatever S is.
 *
 *   Sample i sits at t = i dt.  If t >= D (with SNAP: i >= N_{L-1}) it is the last waypoint bit for bit with velocity 0.  Otherwise k
 *   is the last segment with t_start_k <= t (with SNAP: N_k <= i) -- it has a positive duration -- and tau = t - t_start_k (with SNAP
 *   (i - N_k) dt, from integers):
 *
 *     tau < t_acc            :  s = (1/2) A tau^2,           sdot = A tau
 *     tau <= D_k - t_acc     :  s = peak (tau - t_acc / 2),  sdot = peak
 *     after that             :  s = 1 - (1/2) A r^2,         sdot = A r,   r = max(D_k - tau, 0)
 *
 *   out_traj[b][i] = q_k (+) s dv_k with the arithmetic of the pose loops' integrator (s == 0: q_k bit for bit), and
 *   out_vel[b][i] = sdot dv_k.  Rows i >= n_samples repeat the last waypoint with velocity 0: the result is rectangular, every
 *   instance in step, as loikb_track_pose takes it.
 *
 * Outputs.  out_traj [B][S][nq], or NULL for a timing-only call: S is then ignored, nothing is sampled and TRUNCATED is never set.
 * out_vel [B][S][nv] or NULL.  out_seg [B][T-1][4] = { t_start, duration, t_acc, peak sdot } per segment, 0 for segments at or after
 * L - 1 (may be NULL).  out_duration [B] = D.  out_info [B][4] = { n_samples, L, segments with a positive duration, flags }:
 *
 *   LOIKB_RETIME_TRUNCATED  n_samples > S; the first S rows are still written.
 *   LOIKB_RETIME_INVALID    a waypoint of the path (or a difference between two of them) is not finite: the duration, out_seg and all
 *                           rows of the path are NaN, n_samples and the segment count are 0.
 *   LOIKB_RETIME_SKIPPED    len[b] is outside 2 .. T: out_info is 0 apart from the flag; the duration, out_seg and the rows are NaN.
 *
 * The other paths of the batch are not affected by an INVALID or SKIPPED one.
 *
 * Errors.  LOIKB_ERR_ARG: NULL handle, T < 2, B < 0, B * T >= 2^31, a NULL q_path with B > 0, a NULL v_max, a_max, p, out_duration or
 * out_info, a limit that is not finite or <= 0, a dt that is not finite or <= 0, unknown flags, out_traj given with S < 1 or with
 * B * S >= 2^31, out_vel given without out_traj, out_traj == q_path.  The arguments are checked first, as in loik_amd_shortcut.h; after
 * that B == 0 is LOIKB_OK and writes nothing.  A call that fails writes nothing.
 */
#ifndef LOIK_AMD_RETIME_H
#define LOIK_AMD_RETIME_H

#include "loik_amd_motion.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_RETIME_VERSION 1  /* bumped whenever a struct or an entry point of this header changes */

#define LOIKB_RETIME_SNAP 1       /* loikb_retime_params.flags: stretch every segment to whole samples */

#define LOIKB_RETIME_TRUNCATED 1  /* out_info[b][3] */
#define LOIKB_RETIME_INVALID 2
#define LOIKB_RETIME_SKIPPED 4

typedef struct loikb_retime_params {
  double dt;  /* the sample period, finite and > 0 */
  int flags;  /* 0 or LOIKB_RETIME_SNAP            */
} loikb_retime_params;

int loikb_retime_version(void);

/* q_path [B][T][nq]; len [B] ints or NULL (= T everywhere); v_max, a_max [nv] on the host.
 * out_traj [B][S][nq] or NULL (timing only); out_vel [B][S][nv] or NULL; out_seg [B][T-1][4] or NULL; out_duration [B];
 * out_info [B][4] ints.                                                                                                    */
int loikb_retime_paths(loikb_solver *s, const double *q_path, const int *len, int B, int T, int in_flags,
                       const double *v_max, const double *a_max, const loikb_retime_params *p, int S,
                       double *out_traj, double *out_vel, double *out_seg, double *out_duration, int *out_info, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_RETIME_H */
