/*
 * loik_amd_multistart.h -- multi-start pose IK on top of loik_amd_pose.h (libloik_amd.so): "answer these G goals, K seeds each".
 *
 * loikb_solve_pose takes each of B seeds to a target and is a local method: a seed on the wrong side of a joint limit or next
 * to a singular posture ends max_steps without REACHED.  A sampling planner or a global IK therefore runs many seeds per goal
 * and keeps the best.  The three steps that turn B independent local solves into G answered goals run on the device here:
 * drawing seeds inside the joint ranges, re-seeding the instances that failed, and a segmented selection of the winning seed
 * per goal.  A handle of batch B = G * K answers G goals with K seeds each; instance b = g * K + k is seed k of goal g.
 *
 * The sampler.  All integer arithmetic is uint64, wrapping:
 *
 *     mix(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
 *     key  = mix(seed + 0x9E3779B97F4A7C15 * (round + 1))
 *     word = mix(key ^ ((uint64)b << 32 | (uint64)j))          b = batch index, j = DoF index in idx_v order
 *     u    = (double)(word >> 11) * 2^-53                       in [0, 1)
 *     q_j  = min(s_lo_j + round_to_double(u * (s_hi_j - s_lo_j)), s_hi_j)
 *
 * (the product is rounded before the sum: no fused multiply-add).  The sampler writes the WHOLE row of instance b: the
 * coordinate of a sampled DoF gets q_j, every other coordinate -- unsampled DoFs, the coordinates of free-flyer, spherical,
 * planar and unbounded joints -- gets the q0 row of its goal, so a row that went NaN in an earlier round is whole again.
 * Exception: in round 0, seed k = 0 of every goal is the q0 row itself, unsampled; hence K = 1, R = 1 is loikb_solve_pose.
 * The handle is left as loikb_solve_pose(q != NULL) leaves it after it replaced the resident q: the next solve's FwdPassInit
 * runs from the new q.
 *
 * Ranges.  A DoF is sampled iff its s_lo and s_hi are both finite.  Without loikb_multistart_set_ranges (or after it was
 * called with both pointers NULL) the ranges are the handle's joint limits (loikb_set_joint_limits), as they are when the
 * entry point runs.  A finite range is accepted only on a DoF whose coordinate a plain sum advances: the rule, and the
 * message, of loikb_set_joint_limits.  s_lo == s_hi is legal: the coordinate is then constant.
 *
 * loikb_solve_pose_multistart:
 *   1. the targets are validated as loikb_solve_pose validates them, and expanded on the device to [B][nc][12];
 *   2. round 0: every instance is sampled;
 *   3. loikb_solve_pose runs on the resident q with the expanded targets -- everything that call honours holds: tasks, joint
 *      limits, gain, dt, max_steps = 0, f32 handles;
 *   4. the goals that own an instance with REACHED and not STOPPED are counted on the device; one counter comes back;
 *   5. if all G goals have one, or the round was the last of `rounds`, the loop ends; otherwise every instance WITHOUT REACHED
 *      (seed k = 0 and stopped instances included) is re-sampled with the next round number and step 3 runs again.  Reached
 *      instances are not re-sampled and, by the pose contract, do not move.
 * A round costs a whole-batch pose loop: the instances of a goal that is already answered run until their own loop ends.
 * Afterwards loikb_pose_get, loikb_get and loikb_pose_get_limit_flags describe the LAST loikb_solve_pose, as their headers say,
 * and the problem is left as loikb_solve_pose leaves it.
 *
 * The selection.  One winner per goal: the lexicographic minimum of (class, cost, b) over the goal's K instances.
 *
 *     class 0   REACHED, not STOPPED             PICK_NEAREST: sum_j w_j (q_j - q0_j)^2 over the plain-sum DoFs, in fp64
 *                                                PICK_FIRST:   0, so the lowest b wins
 *     class 1   neither REACHED nor STOPPED      the largest |entry| of the instance's LOIKB_POSE_F_ERR
 *     class 2   STOPPED                          0
 *
 * Goal status by the winner's class: 0 -> LOIKB_MS_GOAL_REACHED, 1 -> LOIKB_MS_GOAL_BEST_EFFORT, 2 -> LOIKB_MS_GOAL_FAILED.
 * A NaN cost orders after every number; exact ties go to the lowest b.  The result is deterministic.
 *
 * Errors.  LOIKB_ERR_ARG: B % K != 0, K < 1, R < 1, round < 0, a pick outside 0..1, flags != 0, NULL pointers, and what
 * loikb_solve_pose rejects.  LOIKB_ERR_STATE: before SolveInit; K > 1 or R > 1 (loikb_multistart_sample: K > 1 or round > 0)
 * while no DoF is sampled (no ranges and no limits set, or no pair finite).  On any error the handle is unchanged.
 * A handle that never calls an entry point of this header runs exactly what it ran before this header existed.
 */
#ifndef LOIK_AMD_MULTISTART_H
#define LOIK_AMD_MULTISTART_H

#include "loik_amd_pose.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_MULTISTART_VERSION 1  /* bumped whenever a struct or an entry point of this header changes */

enum { LOIKB_MS_PICK_NEAREST = 0, LOIKB_MS_PICK_FIRST = 1 };

typedef struct loikb_multistart_params {
  int seeds_per_goal;        /* K >= 1, B % K == 0, G = B / K                                   */
  int rounds;                /* R >= 1: round 0 plus up to R-1 restarts                          */
  unsigned long long seed;   /* stream key of the sampler                                        */
  int pick;                  /* LOIKB_MS_PICK_NEAREST (0) | LOIKB_MS_PICK_FIRST (1)              */
  int flags;                 /* reserved, 0                                                      */
} loikb_multistart_params;

int loikb_multistart_version(void);

/* ranges the seeds are drawn from: s_lo, s_hi [nv] (idx_v order, host).  A DoF is sampled iff both are finite.
 * Both NULL = the handle's joint limits (loikb_set_joint_limits).  weights [nv] >= 0, or NULL = 1: the nearest-seed metric.
 * LOIKB_ERR_ARG: n != nv, NaN, s_lo > s_hi, exactly one of s_lo, s_hi NULL, a negative or non-finite weight, a finite range
 * on a DoF that is not plain-sum (loikb_last_error() names the DoF).                                                       */
int loikb_multistart_set_ranges(loikb_solver *s, const double *s_lo, const double *s_hi, const double *weights, int n);

/* writes the seeds of round `round` into the resident q of ALL instances and does nothing else (what a caller who drives
 * its own loop needs).  q0 [G][nq], or [nq] with LOIKB_Q_SHARED (a host pointer); device with LOIKB_IN_DEVICE; NULL = the
 * resident q of each goal's instance g*K.                                                                                */
int loikb_multistart_sample(loikb_solver *s, const double *q0, int q0_flags, unsigned long long seed, int seeds_per_goal, int round);

/* q0 as above; targets [G][nc][12], or [nc][12] with LOIKB_POSE_TARGET_SHARED; LOIKB_IN_DEVICE: q0 (unless shared) and
 * targets are device pointers.                                                                                           */
int loikb_solve_pose_multistart(loikb_solver *s, const double *q0, const double *targets, int in_flags,
                                const loikb_pose_params *pose, const loikb_multistart_params *ms);

/* results of the last loikb_solve_pose_multistart (LOIKB_ERR_STATE before the first) */
enum { LOIKB_MS_F_WINNER = 0,   /* int [G]: batch index b of the chosen instance                                  */
       LOIKB_MS_F_GOAL_STATUS,  /* int [G]: LOIKB_MS_GOAL_* bits                                                  */
       LOIKB_MS_F_Q,            /* double [G][nq]: the winner's q                                                 */
       LOIKB_MS_F_ERR,          /* double [G][nc][6]: the winner's LOIKB_POSE_F_ERR row                           */
       LOIKB_MS_F_COST,         /* double [G]: the winner's cost (above)                                          */
       LOIKB_MS_F_NREACHED,     /* int [G]: instances of the goal with REACHED after the last round               */
       LOIKB_MS_F_ROUND,        /* int [B]: the round whose sampler call wrote the seed the instance ended from   */
       LOIKB_MS_F_TIMING };     /* double [6]: rounds run, wall ms, ms in solve_pose, ms sampling, ms selecting, ms rest */
enum { LOIKB_MS_GOAL_REACHED = 1, LOIKB_MS_GOAL_BEST_EFFORT = 2, LOIKB_MS_GOAL_FAILED = 4 };
int loikb_multistart_get(loikb_solver *s, int field, void *out, int out_flags);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_MULTISTART_H */
