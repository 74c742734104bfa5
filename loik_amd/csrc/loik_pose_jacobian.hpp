// Frame Jacobians and dexterity measures of the resident configurations (include/loik_amd_jacobian.h).
//
//   k_frame_jacobians : J [B][n][6][nv] of requested (link, frame) pairs in one of the three reference frames.  The output is the
//                       cost (6 nv doubles per pair: 100 MB for Talos-32 at 65 536 instances), so the work is laid out for the
//                       stores: one wavefront per (instance, entry), one lane per DoF (striding for nv > 64), a row's 8-byte
//                       stores side by side across the lanes.  The wavefront writes the root path into LDS, the on-path lanes
//                       build liM_j of their joint in parallel (pose_joint_xform) into LDS, then each on-path lane composes
//                       jMf along its stretch of the path (every lane reads the same LDS record at the same trip: a broadcast)
//                       and stores X(fM_j) S_j; off-path lanes store zeros.
//   k_frame_dexterity : the singular values, manipulability and inverse condition number of the masked, scaled LOCAL Jacobian, one
//                       thread per (instance, entry).  ONE walk up the root path keeps T = fM_j (from iMf^-1, times liM_j^-1 per
//                       step) and accumulates the 21 entries of G = J^ J^T in registers: J is never stored.  Then a cyclic Jacobi
//                       eigen-solve of the 6 x 6 with every (p, q) pair a template instantiation, so that every index into the
//                       private matrix is a compile-time constant (a runtime-indexed private array goes to scratch), and a fixed
//                       bound of sweeps: a NaN runs the bound out and ends as NaN outputs, it cannot loop.
//   k_dex_cost        : the per-instance cost of the dexterous multi-start pick, - min_c sigma_{m_c - 1}, from k_frame_dexterity's
//                       records of the active constraints
//
// fp64 whatever the handle's precision, as loik_pose.hpp.
#pragma once

#include "loik_pose.hpp"

namespace loikb {

enum : int { JAC_LOCAL = 0, JAC_LOCAL_WORLD_ALIGNED = 1, JAC_WORLD = 2 };
enum : int { DEX_MANIPULABILITY = 6, DEX_INV_CONDITION = 7, DEX_N = 8 };

constexpr int JAC_WAVES = 4;   // wavefronts = (instance, entry) pairs of one workgroup of k_frame_jacobians, at most: the host launches
                               // fewer when their LDS would not fit, and the kernel goes by blockDim
// LDS doubles of one wavefront: liM [nb][12], then path [nb] and pos [nb] as ints (one double's room for both of a joint)
__host__ __device__ inline size_t jac_wave_doubles(int nb) { return (size_t)nb * 13; }

// S of device joint d in its own frame: lin, ang
__device__ __forceinline__ void joint_motion_vector(const JointDesc& d, double* lin, double* ang)
{
  const bool rev = d.flags & JF_REVOLUTE;
  const double pl = rev ? ((d.flags & JF_HELICAL) ? d.pitch : 0.0) : 1.0;
  for (int k = 0; k < 3; ++k) {
    ang[k] = rev ? d.axis[k] : 0.0;
    lin[k] = pl * d.axis[k];
  }
}

// (R, t) <- (Ra, ta) * (R, t)
__device__ __forceinline__ void xform_premul(const double* Ra, const double* ta, double* R, double* t)
{
  double Rn[9], tn[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Rn[3 * r + c] = Ra[3 * r] * R[c] + Ra[3 * r + 1] * R[3 + c] + Ra[3 * r + 2] * R[6 + c];
    tn[r] = ta[r] + (Ra[3 * r] * t[0] + Ra[3 * r + 1] * t[1] + Ra[3 * r + 2] * t[2]);
  }
  for (int k = 0; k < 9; ++k) R[k] = Rn[k];
  for (int k = 0; k < 3; ++k) t[k] = tn[k];
}

// out[b][e][r][k], lanes along k.  dev_link [n]: device joints (0: the universe); frames [n][12]; nb = nv
__global__ void __launch_bounds__(64 * JAC_WAVES)
k_frame_jacobians(const double* __restrict__ q, int nq, const JointDesc* __restrict__ jd, const int* __restrict__ idx_q,
                  const int* __restrict__ dev_link, const double* __restrict__ frames, int n, int B, int nb, int ref,
                  double* __restrict__ out)
{
  extern __shared__ double jac_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;   // (the host launches JAC_WAVES or fewer)
  const long long total = (long long)B * n;
  long long idx = (long long)blockIdx.x * waves + wave;
  const bool live = idx < total;
  if (!live) idx = total - 1;   // a wavefront past the end walks the last pair and stores nothing: every wavefront meets every barrier
  const int b = __builtin_amdgcn_readfirstlane((int)(idx / n));
  const int e = __builtin_amdgcn_readfirstlane((int)(idx - (long long)b * n));
  double* xf = jac_lds + (size_t)wave * jac_wave_doubles(nb);
  int* path = reinterpret_cast<int*>(xf + (size_t)12 * nb);
  int* pos = path + nb;
  const double* q_row = q + (size_t)b * nq;
  const int link = dev_link[e];

  for (int k = lane; k < nb; k += 64) pos[k] = -1;
  __syncthreads();
  int len = 0;   // the root path, leaf side first: path[m] = the joint at position m, pos[j - 1] = the position of joint j
  for (int i = link; i > 0 && len < nb; i = jd[i].parent) {
    if (lane == 0) { path[len] = i; pos[i - 1] = len; }
    ++len;
  }
  __syncthreads();
  for (int k = lane; k < nb; k += 64) {   // liM of the on-path joints
    if (pos[k] < 0) continue;
    const JointDesc& d = jd[k + 1];
    double p[8] = {0, 0, 0, 0, 0, 0, 0, 0}, R[9], t[3];
    if (!(d.flags & JF_NOQ)) (void)joint_q_pairs(q_row + idx_q[k + 1], d, p);
    pose_joint_xform(d, p, R, t);
    double* o = xf + (size_t)12 * k;
    for (int c = 0; c < 9; ++c) o[c] = R[c];
    for (int c = 0; c < 3; ++c) o[9 + c] = t[c];
  }
  __syncthreads();
  const double* F = frames + (size_t)e * 12;
  for (int k = lane; k < nb; k += 64) {
    double col[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int dp = pos[k];
    if (dp >= 0) {
      // jMf of the joint at position dp: iMf carried up dp joints
      double R[9], t[3];
      for (int c = 0; c < 9; ++c) R[c] = F[c];
      for (int c = 0; c < 3; ++c) t[c] = F[9 + c];
      for (int m = 0; m < dp; ++m) {
        const double* x = xf + (size_t)12 * (path[m] - 1);
        xform_premul(x, x + 9, R, t);
      }
      // X(fM_j) S_j, fM_j = (R^T, -R^T t): ang = R^T S_ang, lin = R^T S_lin + (-R^T t) x ang = R^T (S_lin - t x S_ang)
      double sl[3], sa[3], u[3];
      joint_motion_vector(jd[k + 1], sl, sa);
      u[0] = sl[0] - (t[1] * sa[2] - t[2] * sa[1]);
      u[1] = sl[1] - (t[2] * sa[0] - t[0] * sa[2]);
      u[2] = sl[2] - (t[0] * sa[1] - t[1] * sa[0]);
      for (int r = 0; r < 3; ++r) {
        col[r] = R[r] * u[0] + R[3 + r] * u[1] + R[6 + r] * u[2];
        col[3 + r] = R[r] * sa[0] + R[3 + r] * sa[1] + R[6 + r] * sa[2];
      }
      if (ref != JAC_LOCAL) {   // on to oMf, then the rotation (and for WORLD the lever) of the frame in the world
        for (int m = dp; m < len; ++m) {
          const double* x = xf + (size_t)12 * (path[m] - 1);
          xform_premul(x, x + 9, R, t);
        }
        double l[3], a[3];
        for (int r = 0; r < 3; ++r) {
          l[r] = R[3 * r] * col[0] + R[3 * r + 1] * col[1] + R[3 * r + 2] * col[2];
          a[r] = R[3 * r] * col[3] + R[3 * r + 1] * col[4] + R[3 * r + 2] * col[5];
        }
        if (ref == JAC_WORLD) {
          l[0] += t[1] * a[2] - t[2] * a[1];
          l[1] += t[2] * a[0] - t[0] * a[2];
          l[2] += t[0] * a[1] - t[1] * a[0];
        }
        for (int r = 0; r < 3; ++r) { col[r] = l[r]; col[3 + r] = a[r]; }
      }
    }
    if (live) {
      double* o = out + (size_t)idx * 6 * nb + k;
      for (int r = 0; r < 6; ++r) o[(size_t)r * nb] = col[r];
    }
  }
}

// ---- the 6 x 6 symmetric eigen-solve of k_frame_dexterity: the upper triangle of a[6][6], compile-time indices only -----------
// The bound is what ends a NaN.  It is not expected to bind for finite input: cyclic Jacobi converges quadratically and a 6 x 6 meets
// the exit test of dex_eigenvalues in 5 .. 7 sweeps, which is what the accuracy contract of the header rests on.
constexpr int DEX_MAX_SWEEPS = 12;

template <int P, int Q, int R>
__device__ __forceinline__ void dex_rotate_other(double (&a)[6][6], double s, double tau)
{
  if constexpr (R != P && R != Q) {
    double& x = a[R < P ? R : P][R < P ? P : R];
    double& y = a[R < Q ? R : Q][R < Q ? Q : R];
    const double xv = x, yv = y;
    x = xv - s * (yv + tau * xv);
    y = yv + s * (xv - tau * yv);
  }
}

// one Jacobi rotation that annihilates a[P][Q] (Rutishauser's formulas); `late`: an entry that no longer changes either diagonal
// neighbour is set to zero instead
template <int P, int Q>
__device__ __forceinline__ void dex_rotate(double (&a)[6][6], bool late)
{
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double g = 100.0 * fabs(apq), app = a[P][P], aqq = a[Q][Q];
  if (late && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) { a[P][Q] = 0.0; return; }
  const double h = aqq - app;
  double t;
  if (fabs(h) + g == fabs(h)) t = apq / h;
  else {
    const double theta = 0.5 * h / apq;
    t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
    if (theta < 0.0) t = -t;
  }
  const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
  a[P][P] = app - t * apq;
  a[Q][Q] = aqq + t * apq;
  a[P][Q] = 0.0;
  dex_rotate_other<P, Q, 0>(a, s, tau); dex_rotate_other<P, Q, 1>(a, s, tau); dex_rotate_other<P, Q, 2>(a, s, tau);
  dex_rotate_other<P, Q, 3>(a, s, tau); dex_rotate_other<P, Q, 4>(a, s, tau); dex_rotate_other<P, Q, 5>(a, s, tau);
}

#define LOIKB_DEX_PAIRS(X) X(0, 1) X(0, 2) X(0, 3) X(0, 4) X(0, 5) X(1, 2) X(1, 3) X(1, 4) X(1, 5) X(2, 3) X(2, 4) X(2, 5) X(3, 4) X(3, 5) X(4, 5)

// the eigenvalues of the symmetric a (upper triangle) onto its diagonal
__device__ __forceinline__ void dex_eigenvalues(double (&a)[6][6])
{
#pragma unroll 1
  for (int sweep = 0; sweep < DEX_MAX_SWEEPS; ++sweep) {
    double off = 0.0, tr = 0.0;
#define LOIKB_DEX_OFF(P, Q) off += fabs(a[P][Q]);
    LOIKB_DEX_PAIRS(LOIKB_DEX_OFF)
#undef LOIKB_DEX_OFF
    tr = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]) + fabs(a[3][3]) + fabs(a[4][4]) + fabs(a[5][5]);
    if (off <= 0x1.0p-60 * tr) break;   // (Gershgorin: what is left moves no eigenvalue by more than u |G| / 100; false for a NaN)
    const bool late = sweep >= 3;
#define LOIKB_DEX_ROT(P, Q) dex_rotate<P, Q>(a, late);
    LOIKB_DEX_PAIRS(LOIKB_DEX_ROT)
#undef LOIKB_DEX_ROT
  }
}

template <int I, int J>
__device__ __forceinline__ void dex_order(double (&d)[6])
{
  const double x = d[I], y = d[J];
  if (x < y) { d[I] = y; d[J] = x; }
}

// out[b][e][DEX_N].  rows [n]: 6-bit masks; length: L
__global__ void __launch_bounds__(256)
k_frame_dexterity(const double* __restrict__ q, int nq, const JointDesc* __restrict__ jd, const int* __restrict__ idx_q,
                  const int* __restrict__ dev_link, const double* __restrict__ frames, const int* __restrict__ rows, int n, int B,
                  double length, double* __restrict__ out)
{
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)B * n) return;
  const int b = (int)(idx / n), e = (int)(idx - (long long)b * n);
  const double* q_row = q + (size_t)b * nq;
  bool finite = true;
  for (int i = 0; i < nq; ++i) finite = finite && isfinite(q_row[i]);
  const double* F = frames + (size_t)e * 12;
  const int rmask = rows[e];
  // T = fM_j, from iMf^-1 = (Rf^T, -Rf^T pf)
  double TR[9], Tt[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) TR[3 * r + c] = F[3 * c + r];
    Tt[r] = -(F[r] * F[9] + F[3 + r] * F[10] + F[6 + r] * F[11]);
  }
  double a[6][6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) a[i][j] = 0.0;
  double wt[6];   // D S_r: what a row of the LOCAL Jacobian is multiplied by (applied as a division for the length)
#pragma unroll
  for (int r = 0; r < 6; ++r) wt[r] = ((rmask >> r) & 1) ? 1.0 : 0.0;
  for (int j = dev_link[e]; j > 0;) {
    const JointDesc& d = jd[j];
    double sl[3], sa[3], c[6];
    joint_motion_vector(d, sl, sa);
    mat3_vec(TR, sa, c + 3);
    mat3_vec(TR, sl, c);
    c[0] += Tt[1] * c[5] - Tt[2] * c[4];
    c[1] += Tt[2] * c[3] - Tt[0] * c[5];
    c[2] += Tt[0] * c[4] - Tt[1] * c[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { c[r] = wt[r] * (c[r] / length); c[3 + r] = wt[3 + r] * c[3 + r]; }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int k = i; k < 6; ++k) a[i][k] += c[i] * c[k];
    // T <- T liM_j^-1 = (TR R^T, Tt - TR R^T t)
    double p[8] = {0, 0, 0, 0, 0, 0, 0, 0}, R[9], t[3], Rn[9];
    if (!(d.flags & JF_NOQ)) (void)joint_q_pairs(q_row + idx_q[j], d, p);
    pose_joint_xform(d, p, R, t);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) Rn[3 * r + k] = TR[3 * r] * R[3 * k] + TR[3 * r + 1] * R[3 * k + 1] + TR[3 * r + 2] * R[3 * k + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) Tt[r] = Tt[r] - (Rn[3 * r] * t[0] + Rn[3 * r + 1] * t[1] + Rn[3 * r + 2] * t[2]);
#pragma unroll
    for (int k = 0; k < 9; ++k) TR[k] = Rn[k];
    j = d.parent;
  }
  dex_eigenvalues(a);
  double lam[6] = {a[0][0], a[1][1], a[2][2], a[3][3], a[4][4], a[5][5]};
  finite = finite && isfinite(lam[0] + lam[1] + lam[2] + lam[3] + lam[4] + lam[5]);
  // descending: the 15 exchanges of a bubble network
  dex_order<0, 1>(lam); dex_order<1, 2>(lam); dex_order<2, 3>(lam); dex_order<3, 4>(lam); dex_order<4, 5>(lam);
  dex_order<0, 1>(lam); dex_order<1, 2>(lam); dex_order<2, 3>(lam); dex_order<3, 4>(lam);
  dex_order<0, 1>(lam); dex_order<1, 2>(lam); dex_order<2, 3>(lam);
  dex_order<0, 1>(lam); dex_order<1, 2>(lam);
  dex_order<0, 1>(lam);
  const int m = __popc((unsigned)rmask & 0x3fu);
  double manip = 1.0, last = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    lam[k] = k < m ? sqrt(fmax(lam[k], 0.0)) : 0.0;
    if (k < m) manip *= lam[k];
    if (k == m - 1) last = lam[k];
  }
  double invc = lam[0] == 0.0 ? 0.0 : last / lam[0];
  double* o = out + (size_t)idx * DEX_N;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
  for (int k = 0; k < 6; ++k) o[k] = finite ? lam[k] : nan;
  o[DEX_MANIPULABILITY] = finite ? manip : nan;
  o[DEX_INV_CONDITION] = finite ? invc : nan;
}

// cost[b] = - min_c dex[b][c][m_c - 1], m_c = popcount(rows[c]); a NaN sticks
__global__ void k_dex_cost(const double* __restrict__ dex, const int* __restrict__ rows, int nc, int B, double* __restrict__ cost)
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double m = dex[((size_t)b * nc) * DEX_N + __popc((unsigned)rows[0] & 0x3fu) - 1];
  for (int c = 1; c < nc; ++c) {
    const double v = dex[((size_t)b * nc + c) * DEX_N + __popc((unsigned)rows[c] & 0x3fu) - 1];
    if (v < m || v != v) m = v;
  }
  cost[b] = -m;
}

}  // namespace loikb
