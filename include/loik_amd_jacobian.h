/*
 * loik_amd_jacobian.h -- frame Jacobians and dexterity measures of the resident configurations, and a dexterous winner for the
 * multi-start of loik_amd_multistart.h (libloik_amd.so).
 *
 * The pose layer takes a batch of seeds to targets; this header says how good the configurations it leaves are.  Two getters
 * read the resident q of every instance -- the q of the last SolveInit / tailored Solve / loikb_integrate / pose loop -- and a
 * latch makes loikb_solve_pose_multistart pick, among the reached seeds of a goal, the one farthest from a singular posture.
 * Everything is fp64 from the resident fp64 q, whatever the handle's precision, as with the other pose kernels.
 *
 * The Jacobian.  J[b][e] is the 6 x nv matrix with v_f = J nu: v_f = [linear; angular] the velocity of the frame
 * f = oMi(links[e]) * iMf(e) for the resident q of instance b, nu in the caller's idx_v order (the velocity of a quaternion joint
 * in the joint's local frame, as everywhere else in this library).  Every DoF k is a 1-DoF joint of the device tree with the
 * motion vector S_k = [0; axis] (revolute), [axis; 0] (prismatic) or [pitch axis; axis] (helical) in its own frame j_k:
 *
 *     column k = X(fM_jk) S_k     when j_k is on the root path of links[e],      X(R, t) = [[R, [t]x R], [0, R]]
 *     column k = 0.0 exactly      otherwise
 *
 *     LOIKB_JAC_LOCAL                expressed in f
 *     LOIKB_JAC_LOCAL_WORLD_ALIGNED  blockdiag(oRf, oRf) J_local: the origin of f, the axes of the world
 *     LOIKB_JAC_WORLD                X(oMf) J_local: the spatial velocity at the world's origin
 *
 * (Pinocchio's three ReferenceFrames.)  Link 0, the universe, gives a zero matrix.  frames = NULL is the identity frame on every
 * link (the joint frames), bit for bit what identity frames give.
 *
 * Dexterity.  For each entry, with the row mask r (bit i = row i of the LOCAL Jacobian: the rows of the tool frame, the same
 * rows loikb_pose_set_tasks masks), m = popcount(r) and L = p->length (the length that makes a linear velocity comparable to an
 * angular one):
 *
 *     J^ = D S_r J_local,   D = diag(1/L, 1/L, 1/L, 1, 1, 1),   S_r zeroes the rows that r does not select
 *     G  = J^ J^T  (6 x 6),   lambda_0 >= ... >= lambda_5 its eigenvalues
 *     sigma_k = sqrt(max(lambda_k, 0)) for k < m,   sigma_k = 0.0 exactly for k >= m
 *     manipulability = prod_{k < m} sigma_k                       (Yoshikawa's measure of the selected rows)
 *     inv_condition  = sigma_{m-1} / sigma_0,  0 when sigma_0 == 0
 *
 * out[b][e] = { sigma_0 .. sigma_5, manipulability, inv_condition } (LOIKB_DEX_*).  links = NULL means "the handle's tasks": n must
 * equal loikb_num_eq_c(), the links are the active constraint links in their order, and the frames and rows are those of
 * loikb_pose_set_tasks (rows 0x3f / 0x07 / 0x38 for POSE / POSITION / ORIENTATION, less 0x20 with LOIKB_TASK_FREE_Z); on a handle
 * without tasks the identity frames and 0x3f.  The frames and rows arguments are not read then.
 *
 * Accuracy.  The values come from the Gram matrix G (a cyclic Jacobi eigen-solve with a fixed bound of sweeps), not from an SVD of
 * J^: sigma^2 is accurate to a few u sigma_0^2 (u = 1.1e-16), so a sigma_k below about 1e-7 sigma_0 is "zero" with no more digits
 * than that.  That rests on the solve converging within its bound of 12 sweeps, which a 6 x 6 with finite entries does in 5 to 7
 * (the convergence is quadratic); the bound exists for input that is not finite and is not expected to bind otherwise.  A link
 * with fewer than m DoFs on its root path has trailing sigma of that size or exactly 0.  An instance whose q holds a NaN or an
 * infinity (a STOPPED instance of a pose loop) gets NaN in all LOIKB_DEX_N entries of all its frames; the other instances are
 * not affected.
 *
 * The dexterous pick.  With loikb_dexterity_set_multistart_pick set on the handle, the final selection of
 * loikb_solve_pose_multistart ranks the REACHED seeds of a goal by
 *
 *     cost = - min_c sigma_{m_c - 1}         (c over the active constraints, links = NULL mode above, L = p->length)
 *
 * the smallest singular value of the worst-conditioned task, largest first, in place of what ms->pick says for them (ms->pick is
 * still validated to 0..1).  Seeds that were not reached, the order (class, cost, instance), NaN last and the restart loop stay
 * as loik_amd_multistart.h says.  LOIKB_MS_F_COST returns that cost for a reached winner.  A handle on which the latch was never
 * set, or was cleared, runs exactly what it ran before this header existed.
 *
 * Errors.  LOIKB_ERR_ARG: NULL handle or out, n < 0, links NULL with n > 0 (loikb_frame_jacobians), a link id outside
 * 0..njoints-1, a frame that is not finite or whose rotation is not orthonormal with determinant 1 (tolerance 1e-9),
 * reference_frame outside 0..2, a rows entry outside 1..0x3f, p NULL (loikb_frame_dexterity), length not finite or not > 0,
 * flags != 0, links == NULL with n != loikb_num_eq_c().  LOIKB_ERR_STATE: no configurations resident on the device yet,
 * links == NULL before SolveInit.  n == 0 is LOIKB_OK and writes nothing.  On any error nothing of the handle changes; neither
 * getter changes what a later solve computes.
 */
#ifndef LOIK_AMD_JACOBIAN_H
#define LOIK_AMD_JACOBIAN_H

#include "loik_amd_multistart.h"
#include "loik_amd_tasks.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOIKB_JACOBIAN_VERSION 1  /* bumped whenever an entry point of this header changes */

enum { LOIKB_JAC_LOCAL = 0, LOIKB_JAC_LOCAL_WORLD_ALIGNED = 1, LOIKB_JAC_WORLD = 2 };

typedef struct loikb_dexterity_params {
  double length;  /* L > 0, finite: a linear velocity of L per second weighs what an angular one of 1 rad per second does (default 1) */
  int flags;      /* reserved, 0 */
} loikb_dexterity_params;

/* the entries of one dexterity record */
enum { LOIKB_DEX_SIGMA0 = 0, LOIKB_DEX_SIGMA1 = 1, LOIKB_DEX_SIGMA2 = 2, LOIKB_DEX_SIGMA3 = 3, LOIKB_DEX_SIGMA4 = 4, LOIKB_DEX_SIGMA5 = 5,
       LOIKB_DEX_MANIPULABILITY = 6, LOIKB_DEX_INV_CONDITION = 7, LOIKB_DEX_N = 8 };

int loikb_jacobian_version(void);

/* out [B][n][6][nv] (host, or device with LOIKB_OUT_DEVICE), complete on return.  links [n]: the caller's joint ids; frames [n][12]
 * iMf = (R row-major, p), NULL = the joint frames; reference_frame: LOIKB_JAC_*                                                  */
int loikb_frame_jacobians(loikb_solver *s, const int *links, const double *frames, int n, int reference_frame, double *out,
                          int out_flags);

/* out [B][n][LOIKB_DEX_N] (host, or device with LOIKB_OUT_DEVICE), complete on return.  rows [n]: 6-bit row masks, NULL = 0x3f;
 * links = NULL: the handle's tasks (see above)                                                                                  */
int loikb_frame_dexterity(loikb_solver *s, const int *links, const double *frames, const int *rows, int n,
                          const loikb_dexterity_params *p, double *out, int out_flags);

/* The dexterous pick for every later loikb_solve_pose_multistart on this handle.  p = NULL clears it (the handle behaves as if
 * never set).  LOIKB_ERR_ARG, and nothing changes: length not finite or not > 0, flags != 0.                                  */
int loikb_dexterity_set_multistart_pick(loikb_solver *s, const loikb_dexterity_params *p);

/* returns 1 and fills *out (if not NULL) when the pick is latched, 0 when it is not */
int loikb_dexterity_get_multistart_pick(const loikb_solver *s, loikb_dexterity_params *out);

#ifdef __cplusplus
}
#endif

#endif /* LOIK_AMD_JACOBIAN_H */
