// Vector-Jacobian products of forward kinematics and the Jacobian by reverse mode, one row per call (float64, 1..MP_MAX_DOF joints,
// unrolled).  Header-only like mp_adjoint.h: the HIP kernel k_fk_jac_vjp (mp_kernels.hip) and the CPU twin (mp_cpu.cpp) instantiate
// the same templates.
//
//   L = <gT, T(q)> + <gJ, J(q)>,  T the end-effector pose (4 x 4), J the Jacobian (6 x n, twists [w; v]) in the space (FRAME 0) or the
//   body (FRAME 1) frame, gT / gJ the cotangents  ->  g_q = dL/dq  (n)
//
// Method.  With [V] = [[w]x, v; 0, 0], ad_V = [[[w]x, 0], [[v]x, [w]x]] and w(W) = (W21 - W12, W02 - W20, W10 - W01, W03, W13, W23):
//   dT/dq_i = [J_s,i] T = T [J_b,i];  dJ_s,i/dq_j = ad(J_s,j) J_s,i for j < i (0 otherwise);  dJ_b,i/dq_j = ad(J_b,i) J_b,j for j > i.
// Hence  space:  g_j = J_s,j . (w(gT T^T) - P_j),  P_j = sum_{i>j} ad(J_s,i)^T gJ_i   (a suffix sum: one sweep from the tip)
//        body:   g_j = J_b,j . (w(T^T gT) + Q_j),  Q_j = sum_{i<j} ad(J_b,i)^T gJ_i   (a prefix sum: one sweep from the base)
// with ad(w, v)^T (a, b) = (a x w + b x v, b x w).  The bottom row of gT meets only the constant bottom row of T and drops out.  The
// primal is mp_fk_jac of mp_core.h (the space Jacobian in the compiled link frames); the body Jacobian is Ad(T^-1) of it.  About 40
// operations a joint on top of FK + J: O(n) per row, no 4 x 4 x n or 6 x n x n tensor formed.
#pragma once

#include "mp_core.h"

// FK + Jacobian in FRAME (0 = space, 1 = body) for one row: T 4 x 4 row-major, J 6 x N row-major
template <typename T, int N, int FRAME, typename MT>
MP_HD void mp_kin_primal(const MT& M, const T (&q)[N], T (&TT)[16], T (&JJ)[6 * N]) {
  static_assert(FRAME == 0 || FRAME == 1, "frame: 0 = space, 1 = body");
  MpJointState<T, N> js;
  mp_joint_state<T, N>(M, q, js);
  mp_fk_jac<T, N, true>(M, js, TT, JJ);
  if (FRAME == 1) {  // J_b = Ad(T^-1) J_s:  w_b = R^T w_s,  v_b = R^T (v_s - p x w_s)
    const T px = TT[3], py = TT[7], pz = TT[11];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const T wx = JJ[0 * N + i], wy = JJ[1 * N + i], wz = JJ[2 * N + i];
      const T ux = JJ[3 * N + i] - (py * wz - pz * wy), uy = JJ[4 * N + i] - (pz * wx - px * wz), uz = JJ[5 * N + i] - (px * wy - py * wx);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        JJ[k * N + i] = TT[k] * wx + TT[4 + k] * wy + TT[8 + k] * wz;
        JJ[(3 + k) * N + i] = TT[k] * ux + TT[4 + k] * uy + TT[8 + k] * uz;
      }
    }
  }
}

// w(gT T^T) (space) or w(T^T gT) (body): the twist the pose cotangent pairs with, 6 values [w; v]
template <typename T, int FRAME>
MP_HD void mp_kin_pose_cotangent(const T (&TT)[16], const T (&gT)[16], T (&w)[6]) {
  T W[3][3];
  if (FRAME == 0) {  // (gT T^T)_ab = sum_c gT_ac R_bc + gT_a3 p_b  (a, b < 3);  (gT T^T)_a3 = gT_a3
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) W[a][b] = gT[4 * a] * TT[4 * b] + gT[4 * a + 1] * TT[4 * b + 1] + gT[4 * a + 2] * TT[4 * b + 2] +
                                            gT[4 * a + 3] * TT[4 * b + 3];
    w[3] = gT[3]; w[4] = gT[7]; w[5] = gT[11];
  } else {  // (T^T gT)_ab = sum_c R_ca gT_cb  (a, b < 3);  (T^T gT)_a3 = sum_c R_ca gT_c3
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) W[a][b] = TT[a] * gT[b] + TT[4 + a] * gT[4 + b] + TT[8 + a] * gT[8 + b];
#pragma unroll
    for (int a = 0; a < 3; ++a) w[3 + a] = TT[a] * gT[3] + TT[4 + a] * gT[7] + TT[8 + a] * gT[11];
  }
  w[0] = W[2][1] - W[1][2]; w[1] = W[0][2] - W[2][0]; w[2] = W[1][0] - W[0][1];
}

// The accumulation sweep: g_q from J (in FRAME), the pose term w and the Jacobian cotangent gJ (6 x N row-major)
template <typename T, int N, int FRAME>
MP_HD void mp_kin_sweep(const T (&JJ)[6 * N], const T (&w)[6], const T (&gJ)[6 * N], T (&gq)[N]) {
  T A[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};  // P (space, from the tip) or Q (body, from the base)
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int i = FRAME == 0 ? N - 1 - k : k;
    const T wx = JJ[0 * N + i], wy = JJ[1 * N + i], wz = JJ[2 * N + i], vx = JJ[3 * N + i], vy = JJ[4 * N + i], vz = JJ[5 * N + i];
    const T s = FRAME == 0 ? T(-1) : T(1);
    gq[i] = wx * (w[0] + s * A[0]) + wy * (w[1] + s * A[1]) + wz * (w[2] + s * A[2]) + vx * (w[3] + s * A[3]) + vy * (w[4] + s * A[4]) +
            vz * (w[5] + s * A[5]);
    const T ax = gJ[0 * N + i], ay = gJ[1 * N + i], az = gJ[2 * N + i], bx = gJ[3 * N + i], by = gJ[4 * N + i], bz = gJ[5 * N + i];
    // A += ad(J_i)^T gJ_i = (a x w + b x v, b x w)
    A[0] += (ay * wz - az * wy) + (by * vz - bz * vy);
    A[1] += (az * wx - ax * wz) + (bz * vx - bx * vz);
    A[2] += (ax * wy - ay * wx) + (bx * vy - by * vx);
    A[3] += by * wz - bz * wy;
    A[4] += bz * wx - bx * wz;
    A[5] += bx * wy - by * wx;
  }
}

// One row r of the C entry: q (rows, N), gT (rows, 16) / gJ (rows, 6N) or null (= 0); T / J / gq outputs, each may be null (the
// cotangents are read only for gq).  A row with a non-finite q or cotangent comes back NaN in every output.  (The kernel moves the
// same rows through LDS; this is its arithmetic on plain rows, for the CPU twin.)
template <typename T, int N, int FRAME, typename MT>
MP_HD void mp_fk_jac_vjp_row(const MT& M, const T* q, const T* gT, const T* gJ, T* Tout, T* Jout, T* gq, long r) {
  T a[N], TT[16], JJ[6 * N];
#pragma unroll
  for (int j = 0; j < N; ++j) a[j] = q[r * N + j];
  MpBad<T> bad;
  bad.add(a);
  mp_kin_primal<T, N, FRAME>(M, a, TT, JJ);
  T g[N];
  if (gq) {
    T ct[16], cj[6 * N], w[6];
#pragma unroll
    for (int k = 0; k < 16; ++k) ct[k] = gT ? gT[r * 16 + k] : T(0);
#pragma unroll
    for (int k = 0; k < 6 * N; ++k) cj[k] = gJ ? gJ[r * 6 * N + k] : T(0);
    bad.add(ct);
    bad.add(cj);
    mp_kin_pose_cotangent<T, FRAME>(TT, ct, w);
    mp_kin_sweep<T, N, FRAME>(JJ, w, cj, g);
  }
  const bool poison = bad.any();
  if (Tout) {
    mp_poison_if(poison, TT);
    for (int k = 0; k < 16; ++k) Tout[r * 16 + k] = TT[k];
  }
  if (Jout) {
    mp_poison_if(poison, JJ);
    for (int k = 0; k < 6 * N; ++k) Jout[r * 6 * N + k] = JJ[k];
  }
  if (gq) {
    mp_poison_if(poison, g);
    for (int k = 0; k < N; ++k) gq[r * N + k] = g[k];
  }
}
