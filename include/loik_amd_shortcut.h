/*
 * loik_amd_shortcut.h -- certified shortcutting of joint-space paths, and their lengths (libloik_amd.so).
 *
 * loikb_motion_clearance_path (loik_amd_motion.h) says that a path is free; this header improves one.  Recorded IK paths and planner
 * paths are jagged and over-long, and the standard remedy replaces sub-paths by straight joint-space segments that are themselves free
 * of collision.  loikb_shortcut_paths runs that loop on the device, a wavefront per path from its first round to its last, so that no
 * path waits for another one.  Everything is fp64 whatever the handle's precision.  Pointers are host, or device with LOIKB_IN_DEVICE /
 * LOIKB_OUT_DEVICE (all inputs of a call alike, all outputs alike); a call is complete on return.  No call of this header reads the
 * resident q or the data object, and none edits either; a handle that never calls one launches exactly what it launched before this
 * header existed.
 *
 * The rule.  Path b of q_path [B][T][nq] has len[b] waypoints, its leading rows (len == NULL: T everywhere); the rows after them are
 * not read.  The path keeps a list `keep` of input row indices, initially keep = 0 .. len[b] - 1 and L = len[b].  For round
 * r = 0 .. rounds - 1, while L >= 3:
 *
 *   word(r, b, j) = mix(mix(seed + 0x9E3779B97F4A7C15 * (r + 1)) ^ ((b << 32) | j)), the word of the multi-start sampler
 *                   (loik_amd_multistart.h: mix is the finalizer of splitmix64), in wrapping 64-bit unsigned arithmetic;
 *   i  = word(r, b, 0) mod (L - 2);
 *   j  = i + 2 + word(r, b, 1) mod (L - 2 - i), so 0 <= i and i + 2 <= j <= L - 1;
 *   dv = difference(q[keep[i]], q[keep[j]]) in the arithmetic of loikb_difference, bit for bit;
 *   the segment q[keep[i]] (+) s dv, s in [0, 1], is checked exactly as loikb_motion_clearance checks it with (margin, tol, max_evals):
 *   the same pairs, the same order, the same advancement, hence the same status;
 *   FREE: keep[i + 1 .. j - 1] are removed, L -= j - i - 1: an accepted shortcut;
 *   BLOCKED, UNDECIDED, INVALID: the path is left as it is; each outcome is counted on its own.
 *
 * `tried` counts the rounds that drew a segment: a path with L == 2 draws nothing more.  The first and the last waypoint are always
 * kept.  A FREE segment is accepted as it is, whatever it does to the length: on a robot with nq != nv the length is not guaranteed
 * to decrease (on one with nq == nv it cannot grow, by the triangle inequality).
 *
 * What the result certifies.  A segment of the output is either a segment of the input (keep[k + 1] == keep[k] + 1) or a segment that
 * this call certified FREE with the guarantee of loik_amd_motion.h.  The call never certifies a segment of the input: it does not
 * look at one unless a draw names it, and a caller who needs the inherited segments checked runs loikb_motion_clearance_path on the
 * result.
 *
 * Outputs.  out_info[b] = { L, tried, accepted, blocked, undecided, invalid }.  out_keep[b][k] = keep[k] for k < L and -1 after
 * (out_keep may be NULL).  out_path[b][k] = q_path[b][keep[k]] for k < L, copied bit for bit, and the rows after that repeat the last
 * kept waypoint, so that the result is a [B][T] path every other entry point accepts.  out_val[b] = { length before, length after }
 * in the sense of loikb_path_length (out_val may be NULL).
 *
 * Skipped paths.  A path with len[b] outside 2 .. T is skipped: its out_info is all 0, its out_keep all -1, its rows of out_path and
 * out_val NaN.  The other paths are not affected.
 *
 * Waypoints that are not finite.  A tried segment with an end that is not finite counts as INVALID (its difference is NaN, as
 * loikb_difference has it), and a length over such a waypoint is NaN.  Nothing else changes; a shortcut over such a waypoint removes it.
 *
 * loikb_path_length.  out_length[b] = the sum over consecutive waypoints k < len[b] - 1 of || difference(q_k, q_{k+1}) ||_2: the squares
 * summed in DoF order, the segments in path order.  Two consecutive waypoints that are finite and equal entry by entry are exactly 0
 * apart (the difference of a quaternion with itself is only 0 to rounding), so the repeated last row of an out_path adds nothing:
 * loikb_path_length of an out_path with len == NULL is the length after, bit for bit.  len[b] of 0 or 1 gives 0, len[b] outside 0 .. T
 * gives NaN.  It needs no spheres.
 *
 * Errors.  LOIKB_ERR_ARG: NULL handle, T < 2, B < 0, B * T >= 2^31, a NULL q_path with B > 0, a NULL out_path or out_info (out_length),
 * p == NULL, a margin that is not finite, a tol that is not finite or < 1e-9, max_evals outside 1 .. 65536, rounds outside
 * 0 .. 1048576, flags != 0, out_path == q_path.  LOIKB_ERR_STATE: loikb_shortcut_paths with no spheres set
 * (loikb_collision_set_spheres).  The arguments are checked first, then the state, as in loik_amd_motion.h; after both B == 0 is
 * LOIKB_OK and writes nothing.  A call that fails writes nothing.
 */
#ifndef LOIK_AMD_SHORTCUT_H
#define LOIK_AMD_SHORTCUT_H

#include "loik_amd_motion.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_SHORTCUT_VERSION 1  /* bumped whenever a struct or an entry point of this header changes */

typedef struct loikb_shortcut_params {
  double margin;            /* as loikb_motion_params                                  */
  double tol;               /* as loikb_motion_params (finite, >= 1e-9)                */
  int max_evals;            /* as loikb_motion_params (1 .. 65536), per tried segment  */
  int rounds;               /* 0 .. 1048576 shortcut attempts per path                 */
  unsigned long long seed;  /* stream key of the draws                                 */
  int flags;                /* reserved, 0                                             */
} loikb_shortcut_params;

int loikb_shortcut_version(void);

/* q_path [B][T][nq]; len [B] ints or NULL (= T everywhere): the leading rows of each path that are waypoints.
 * out_path [B][T][nq], out_info [B][6] ints; out_keep [B][T] ints or NULL; out_val [B][2] doubles or NULL.          */
int loikb_shortcut_paths(loikb_solver *s, const double *q_path, const int *len, int B, int T, int in_flags,
                         const loikb_shortcut_params *p, double *out_path, int *out_keep, int *out_info, double *out_val, int out_flags);

/* out_length [B]: sum over consecutive waypoints k < len[b] - 1 of || difference(q_k, q_{k+1}) ||_2 */
int loikb_path_length(loikb_solver *s, const double *q_path, const int *len, int B, int T, int in_flags, double *out_length, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_SHORTCUT_H */
