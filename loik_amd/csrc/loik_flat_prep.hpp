// loik_flat_prep.hpp -- the PREPARED record of a fresh instance: what k_fslots has in hand of an instance anyway (the joints' world
// placements, S^w, the record's scalars) plus the instance's constraint blocks at the world origin, written down once, instance-major
// and in the lane order of k_flat2, so that k_flat2 takes a fresh instance up in ONE trip to memory with no LDS rounds.
//
// Why: k_fslots and k_flat2's load_instance both ran joint_xform, the pointer-jumping oMi chain, S^w and the congruences to the world
// origin for every instance -- the second time out of the wavefront-tiled records, whose 16-byte pairs cost a 64-byte line each, behind
// a global queue that spreads a tile's lines over all eight L2s.  k_fslots reads the tiles XCD by XCD; it is now
// the only reader of a fresh instance's inputs.
//
// Every value of the block is formed by the functions, in the order of operations, of load_instance (loik_flat2.hpp): the bits
// k_flat2 takes from the block are the bits it computed itself (tests/test_flat_prep.py compares the two paths byte for byte).
//
// Block of one instance (doubles; indexed by the instance's slot, like the decade slots):
//   PR_RT  [12][32]  R0 (9), t0 (3) of joint j                 -- both lanes of a joint read the same 256-byte row
//   PR_JS  [4][32]   nu, S^T f + w, lb, ub of joint j           -- (lb / ub only when the box is per instance)
//   PR_SW  [3][64]   lane (j, h)'s half of S^w
//   PR_SC  [32]      the scalar record's fields load_instance reads: isc[0 .. 10] as they go to LDS, then mu, k, iter, status,
//                    tail iterations, mu flips
//   PR_C   [nc][C2D] the constraint blocks as load_instance leaves them in LDS
#pragma once

#include "loik_lean.hpp"

namespace loikb {

// Constraint block of an instance in the LDS of k_flat2 / k_flat1 (doubles; every 6-vector starts at an even offset).  What the loop
// needs of a task constraint (A, b) on joint c is its image at the world origin: AW = X*_{0<-c} A^T ([world component k][row q],
// and transposed), because  A v_c = AW^T v^w_c  (the constrained link's velocity as the path sum leaves it, no frame change) and
// X* (A^T y) = AW y.  A itself stays for the stored record's A^T y.
enum : int { C2_LANE = 0, C2_B = 2, C2_Y = 8, C2_ATYW = 14 /* A^T y at the world origin: the next FwdPass1's */, C2_ATBW = 20,
             C2_ATYF = 26 /* the constraint's force in this iteration's f */, C2_CW = 32, C2_DLT = 38 /* first-iteration corrections */,
             C2_VC = 44 /* v^w of the constrained joint */, C2_ATY = 50 /* A^T y as the record brought it */, C2_AW = 56, C2_AWT = 92,
             C2_A = 128, C2D = 164 };

constexpr int PREP_G = 32;   // lanes per instance in k_fslots for which the block is written (k_flat2's robots: 17..32 joints)
enum : int { PR_RT = 0, PR_JS = PR_RT + 12 * PREP_G, PR_SW = PR_JS + 4 * PREP_G, PR_SC = PR_SW + 3 * WAVE, PR_C = PR_SC + 32 };
// PR_SC: entries 0 .. 10 are FI_BNORM .. FI_C2 of the instance's LDS scalars, in that order
enum : int { PRS_BNORM = 0, PRS_TGIN = 1, PRS_STY = 2, PRS_MU = 11, PRS_KEXP, PRS_ITER, PRS_STATUS, PRS_TAILIT, PRS_FLIP, PRS_N };

__host__ __device__ __forceinline__ int flat_prep_stride(int nc) { return PR_C + nc * C2D; }

// (AW y)_k and (A^T y)_k of a constraint block: the ONE order of operations wherever they are formed (k_flat2's load, loop
// and store; here)
template <typename T>
__device__ __forceinline__ T prep_awy_of(const T* blk, int k)
{
  const T* r = blk + C2_AW + 6 * k;
  const T* y = blk + C2_Y;
  return ((r[0] * y[0] + r[1] * y[1]) + r[2] * y[2]) + ((r[3] * y[3] + r[4] * y[4]) + r[5] * y[5]);
}
template <typename T>
__device__ __forceinline__ T prep_aty_of(const T* blk, int k)
{
  const T* A_ = blk + C2_A + k;
  const T* y = blk + C2_Y;
  return ((A_[0] * y[0] + A_[6] * y[1]) + A_[12] * y[2]) + ((A_[18] * y[3] + A_[24] * y[4]) + A_[30] * y[5]);
}

constexpr int PREP_NC = 4;   // task constraints whose blocks k_fslots builds: two instances' blocks fit its placement rows
static_assert((WAVE / PREP_G) * PREP_NC * C2D <= (WAVE + 1) * 22, "the constraint blocks are built in k_fslots' placement rows");

// What the block takes from the tile records besides the joint angle.  k_fslots runs one wavefront per SIMD and waits for every trip to
// memory in full: these loads are issued WITH its first one (JP_CS) and used after the placements -- one trip, not three more.
template <typename T>
struct FlatPrepIn {
  typename Vec2<T>::type nus, lu;
  T sc;                 // entry `jlane` of PR_SC
  T cv[PREP_NC];        // lane 6 w + k: b / y / A^T y (w = 0, 1, 2), component k, of constraint c
  T ca[PREP_NC][2];     // entries jlane and PREP_G + jlane of A of constraint c
};
template <typename T>
__device__ __forceinline__ void flat_prep_fetch(FlatPrepIn<T>& in, bool has_inst, const Params<T>& P, const Bufs<T>& Bf, const char* ip, const char* rec,
                                                int jlane, bool isj_lane)
{
  const Layout& L = P.L;
  in.nus.x = in.nus.y = T(0); in.lu.x = in.lu.y = T(0);
  in.sc = T(0);
#pragma unroll
  for (int c = 0; c < PREP_NC; ++c) { in.cv[c] = T(0); in.ca[c][0] = in.ca[c][1] = T(0); }
  if (!has_inst) return;
  if (isj_lane) {
    in.nus = ldp<T>(rec, JP_NUS);
    if (!(P.mode & MODE_BND_SHARED)) in.lu = ldp<T>(rec, JP_LBUB);
  }
  // MODE_VIRTUAL_RESET: the tiles have not seen this solve's reset_tile(RS_RECURSION | RS_SOLVER).  What it would have written -- the
  // scalar record but bnorm (SP_BI's low half) and SP_TAG, and the constraints' y and A^T y -- is taken as the constants it writes:
  // mu = mu0, everything else +0.  What it keeps (nu, S^T f + w, bnorm, the tag, b, A, the box) is loaded as ever.
  const bool virt = (P.mode & MODE_VIRTUAL_RESET) != 0;
  if (virt && jlane < PRS_N && jlane != PRS_BNORM && jlane != PRS_TGIN) {
    in.sc = jlane == PRS_MU ? P.mu0 : T(0);
  } else if (jlane < PRS_N) {
    const char* srec = ip + (size_t)L.off_s * pair_bytes<T>();
    // (pair, half) of entry `jlane` of PR_SC
    const int sc_i = jlane == 3 ? SC_TOL_PRIMAL : jlane == 4 ? SC_TOL_DUAL : jlane == 5 ? SC_DELTA_Y_QP : jlane == 6 ? SC_AT_DELTA_Y_QP
                   : jlane == 7 ? SC_UB_DY_PLUS : jlane == 8 ? SC_LB_DY_MINUS : jlane == 9 ? SC_COND1 : jlane == 10 ? SC_COND2
                   : jlane == PRS_TAILIT ? SC_TAIL_ITER : -1;
    const int pair = sc_i >= 0 ? SP_SCAL + sc_i / 2
                   : jlane == PRS_BNORM || jlane == PRS_ITER ? SP_BI : jlane == PRS_TGIN ? SP_TAG : jlane == PRS_STY || jlane == PRS_STATUS ? SP_ST
                   : jlane == PRS_FLIP ? SP_FLIP : SP_MU;
    const int hi = sc_i >= 0 ? (sc_i & 1) : (jlane == PRS_ITER || jlane == PRS_STY || jlane == PRS_KEXP) ? 1 : 0;
    in.sc = *reinterpret_cast<const T*>(srec + (size_t)pair * pair_bytes<T>() + (size_t)hi * sizeof(T));
  }
#pragma unroll
  for (int c = 0; c < PREP_NC; ++c) {
    if (c >= L.nc) break;
    const char* crec = ip + (size_t)(L.off_c + c * L.crec) * pair_bytes<T>();
    if (jlane < (virt ? 6 : 18)) {   // (virtual reset: b only)
      const int which = jlane / 6, k = jlane % 6;
      const int pair = which == 0 ? CP_B : which == 1 ? CP_Y : CP_ATY;
      in.cv[c] = *reinterpret_cast<const T*>(crec + (size_t)(pair + k / 2) * pair_bytes<T>() + (k & 1) * sizeof(T));
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = jlane + i * PREP_G;
      if (e < LCA)
        in.ca[c][i] = (P.mode & MODE_A_SHARED) ? Bf.uni[c * LCA + e]
                                               : *reinterpret_cast<const T*>(crec + (size_t)(CP_A + e / 2) * pair_bytes<T>() + (e & 1) * sizeof(T));
    }
  }
}

// k_fslots, after its world placements: the lane group of an instance (G = PREP_G lanes, lane `jlane` <-> joint jlane + 1) writes the
// instance's block.  `cb`: nc * C2D scalars of LDS of the lane group's own, free until the next tail_sync after the call.
// Called by every lane of the wavefront (the group of a missing instance stores nothing).
template <typename T>
__device__ __forceinline__ void flat_prep_write(T* __restrict__ blk, bool has_inst, const Params<T>& P, const FlatPrepIn<T>& in, int jlane, int cslot,
                                                const T* R0, const T* t0, const T* Sw, T* cb)
{
  const Layout& L = P.L;
  if (has_inst) {
#pragma unroll
    for (int k = 0; k < 9; ++k) blk[PR_RT + k * PREP_G + jlane] = R0[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) blk[PR_RT + (9 + k) * PREP_G + jlane] = t0[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) { blk[PR_SW + k * WAVE + jlane] = Sw[k]; blk[PR_SW + k * WAVE + PREP_G + jlane] = Sw[3 + k]; }
    blk[PR_JS + jlane] = in.nus.x; blk[PR_JS + PREP_G + jlane] = in.nus.y;
    blk[PR_JS + 2 * PREP_G + jlane] = in.lu.x; blk[PR_JS + 3 * PREP_G + jlane] = in.lu.y;
    if (jlane < PRS_N) blk[PR_SC + jlane] = in.sc;
  }
  // ---- the constraint blocks, in LDS as load_instance builds them, then out in rows
  const int nce = L.nc * C2D;
  for (int e = jlane; e < nce; e += PREP_G) cb[e] = T(0);
  tail_sync();
#pragma unroll
  for (int c = 0; c < PREP_NC; ++c) {
    if (c >= L.nc || !has_inst) break;
    T* c_ = cb + c * C2D;
    if (jlane < 18) {
      const int which = jlane / 6, k = jlane % 6;
      c_[(which == 0 ? C2_B : which == 1 ? C2_Y : C2_ATY) + k] = in.cv[c];
    }
    c_[C2_A + jlane] = in.ca[c][0];
    if (jlane + PREP_G < LCA) c_[C2_A + PREP_G + jlane] = in.ca[c][1];
  }
  if (cslot >= 0) cb[cslot * C2D + C2_LANE] = (T)jlane;
  tail_sync();
  if (cslot >= 0) {  // the constrained joint's lane: column q of AW = row q of A carried to the world origin
    T* c_ = cb + cslot * C2D;
    const T* A_ = c_ + C2_A;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      T aj[6], o[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) aj[k] = A_[6 * q + k];
      act_force(R0, t0, aj, o);
#pragma unroll
      for (int k = 0; k < 6; ++k) { c_[C2_AW + 6 * k + q] = o[k]; c_[C2_AWT + 6 * q + k] = o[k]; }
    }
    T ay[6], o[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) ay[k] = c_[C2_ATY + k];
    act_force(R0, t0, ay, o);
#pragma unroll
    for (int k = 0; k < 6; ++k) c_[C2_ATYW + k] = o[k];
  }
  tail_sync();
  if (jlane < 6 * L.nc) {  // A^T b at the world origin and the first iteration's corrections: lane 6 c + k owns row k of constraint c
    const int ccl = jlane / 6, k = jlane - 6 * ccl;
    T* const ccb = cb + ccl * C2D;
    T ab = T(0);
#pragma unroll
    for (int q = 0; q < 6; ++q) ab += ccb[C2_AW + 6 * k + q] * ccb[C2_B + q];
    ccb[C2_ATBW + k] = ab;
    const T aw = prep_awy_of<T>(ccb, k), at = prep_aty_of<T>(ccb, k);
    ccb[C2_CW + k] = ccb[C2_ATYW + k] - aw;
    ccb[C2_DLT + k] = at - ccb[C2_ATY + k];
  }
  tail_sync();
  if (has_inst)
    for (int e = jlane; e < nce; e += PREP_G) blk[PR_C + e] = cb[e];
}

}  // namespace loikb
