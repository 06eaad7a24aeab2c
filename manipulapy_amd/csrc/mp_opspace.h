// Operational-space (task-space) dynamics and task-space computed torque, one row per call (float64, 1..MP_MAX_DOF joints, unrolled).
// Header-only like mp_deriv.h: the HIP kernels k_opspace / k_opspace_torque (mp_kernels.hip) and the CPU twins (mp_cpu.cpp)
// instantiate the same templates.
//
//   frame 0 = space, 1 = body, 2 = hybrid (J_h = blkdiag(R, R) J_b: angular velocity and tool-origin velocity, both in space axes);
//   task  0 = full (6 rows, [w; v]), 1 = linear (rows 3..5), 2 = angular (rows 0..2);  J = the selected m x n block;
//   h = c(q, qd) + g(q) (no tip wrench: a tip wrench is the caller's J^T F), damping lambda >= 0
//
//   A = J M^-1 J^T + lambda^2 1 (m x m)     Lambda = A^-1      Jbar = M^-1 J^T Lambda (n x m)      Jdot qd (m)
//   mu = Lambda (J M^-1 c - Jdot qd)        p = Lambda J M^-1 g
//   tau(a*, tau0) = J^T (Lambda a* + mu + p) + (1 - J^T Jbar^T) tau0
//
// Method.  FK + the space Jacobian (mp_fk_jac) once; Jdot qd by one O(n) sweep over the columns in registers: with V_i = sum_{j<i}
// J_j qd_j, Jdot_s qd = sum_i ad(V_i) J_i qd_i, ad(w, v)(a, b) = (w x a, v x a + w x b).  Body: Ad(T^-1) of the columns and of Jdot qd
// (the derivative of Ad(T^-1) meets V in ad(V_b) V_b = 0).  Hybrid: v -> v + w x p for the columns, and for Jdot qd the derivative of
// that shift, alpha x p + w x (v + w x p), the w x v term of the rotating axes.  Then the task rows are moved to the front and the
// unused rows zeroed, so that everything below runs on 6 rows whatever `task` is: frame and task stay run-time, wave-uniform values
// and there is one instance per joint count.  A zeroed row gets a unit diagonal in A: the factor of blkdiag(A_m, 1) is that of A_m.
// M = L L^T by the composite-rigid-body pass and Cholesky in place; W = L^-1 J^T overwrites J (row k of W over row k of J);
// A = W^T W + lambda^2 1 is factored by Cholesky too; M^-1 is never formed:  J M^-1 x = W^T (L^-1 x),  M^-1 J^T y = L^-T (W y),
// J^T y = L (W y).  Hence the torque without ever reading J again:
//   tau = L W f + tau0,   A f = a* - Jdot qd + W^T L^-1 (h - tau0)
// A pivot of A that is not positive (to within MP_OS_PIVOT_EPS of its diagonal term) makes the Lambda-dependent outputs of the row
// NaN - T, J and Jdot qd stay valid; a non-finite input makes every output of the row NaN.  A task with more rows than the chain has
// joints (m > N) has rank(A) <= N < m at every pose: with lambda = 0 its rows are NaN by that count alone, without factorising -
// rounding noise lifts the last pivots of such an A over the threshold on part of the rows (mp_opspace_rank_deficient).
#pragma once

#include "mp_core.h"

// a pivot d of A counts as positive when d > MP_OS_PIVOT_EPS * A_jj: 2^-46 = 64 eps, the rounding left in d by the <= 5 products
// subtracted from A_jj and by W.  (A matrix this close to singular has cond(A) > 1e13; nothing useful is lost.)
#define MP_OS_PIVOT_EPS 1.4210854715202004e-14

// Cholesky in place: the lower triangle of A becomes L with 1 / L_jj on the diagonal (as mp_spd_solve), dg = L_jj.  `rel`: the
// relative pivot threshold.  Returns whether every pivot was positive.
template <int NN>
MP_HD bool mp_os_chol(double (&A)[NN][NN], double (&dg)[NN], double rel) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NN; ++j) {
    const double ajj = A[j][j];
    double d = ajj;
#pragma unroll
    for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
    ok = ok && (d > rel * ajj);
    const double inv = mp_rsqrt(d);
    dg[j] = d * inv;
    A[j][j] = inv;
#pragma unroll
    for (int i = j + 1; i < NN; ++i) {
      double v = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
      A[i][j] = v * inv;
    }
  }
  return ok;
}
// b <- L^-1 b
template <int NN>
MP_HD void mp_os_fwd(const double (&L)[NN][NN], double* b) {
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    double v = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= L[i][k] * b[k];
    b[i] = v * L[i][i];
  }
}
// b <- L^-T b
template <int NN>
MP_HD void mp_os_back(const double (&L)[NN][NN], double (&b)[NN]) {
#pragma unroll
  for (int i = NN - 1; i >= 0; --i) {
    double v = b[i];
#pragma unroll
    for (int k = i + 1; k < NN; ++k) v -= L[k][i] * b[k];
    b[i] = v * L[i][i];
  }
}

MP_HD int mp_opspace_dim(int task) { return task == 0 ? 6 : 3; }
// m > N without damping: A = J M^-1 J^T (m x m) is singular whatever the pose.  Wave-uniform: task and lam2 are launch arguments.
template <int N>
MP_HD bool mp_opspace_rank_deficient(int task, double lam2) {
  return lam2 == 0.0 && mp_opspace_dim(task) > N;
}
// a row of COUNT NaNs to `ptr` when it is given
template <int COUNT, typename OUT>
MP_HD void mp_os_nan_out(const OUT& out, double* ptr) {
  if (!ptr) return;
  double o[COUNT];
#pragma unroll
  for (int k = 0; k < COUNT; ++k) o[k] = 0.0;
  mp_poison_if(true, o);
  out(ptr, o);
}

// FK, the Jacobian in `frame` with the rows of `task` first and the others zero (6 x N row-major), and Jdot qd in the same order
template <int N, typename MT>
MP_HD void mp_opspace_kin(const MT& M, int frame, int task, const MpJointState<double, N>& js, const double (&qd)[N], double (&TT)[16],
                          double (&J)[6 * N], double (&jd)[6]) {
  mp_fk_jac<double, N, true>(M, js, TT, J);
  double wx = 0, wy = 0, wz = 0, vx = 0, vy = 0, vz = 0;  // V_i = sum_{j<i} J_j qd_j
  double ax = 0, ay = 0, az = 0, bx = 0, by = 0, bz = 0;  // Jdot_s qd = (alpha, beta)
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double cw0 = J[0 * N + i], cw1 = J[1 * N + i], cw2 = J[2 * N + i], cv0 = J[3 * N + i], cv1 = J[4 * N + i], cv2 = J[5 * N + i];
    const double r = qd[i];
    ax += (wy * cw2 - wz * cw1) * r;
    ay += (wz * cw0 - wx * cw2) * r;
    az += (wx * cw1 - wy * cw0) * r;
    bx += ((vy * cw2 - vz * cw1) + (wy * cv2 - wz * cv1)) * r;
    by += ((vz * cw0 - vx * cw2) + (wz * cv0 - wx * cv2)) * r;
    bz += ((vx * cw1 - vy * cw0) + (wx * cv1 - wy * cv0)) * r;
    wx += cw0 * r; wy += cw1 * r; wz += cw2 * r;
    vx += cv0 * r; vy += cv1 * r; vz += cv2 * r;
  }
  const double px = TT[3], py = TT[7], pz = TT[11];
  if (frame != 0) {  // both moving frames sit at the tool origin:  v <- v + w x p
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double c0 = J[0 * N + i], c1 = J[1 * N + i], c2 = J[2 * N + i];
      J[3 * N + i] += c1 * pz - c2 * py;
      J[4 * N + i] += c2 * px - c0 * pz;
      J[5 * N + i] += c0 * py - c1 * px;
    }
    // the tool origin's velocity, then  beta <- beta + alpha x p  (+ w x pdot in the hybrid frame, whose axes do not turn with the tool)
    const double ux = vx + (wy * pz - wz * py), uy = vy + (wz * px - wx * pz), uz = vz + (wx * py - wy * px);
    bx += ay * pz - az * py;
    by += az * px - ax * pz;
    bz += ax * py - ay * px;
    if (frame == 2) {
      bx += wy * uz - wz * uy;
      by += wz * ux - wx * uz;
      bz += wx * uy - wy * ux;
    } else {  // body: rotate everything into the tool's axes, R^T
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const double c0 = J[0 * N + i], c1 = J[1 * N + i], c2 = J[2 * N + i], d0 = J[3 * N + i], d1 = J[4 * N + i], d2 = J[5 * N + i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          J[k * N + i] = TT[k] * c0 + TT[4 + k] * c1 + TT[8 + k] * c2;
          J[(3 + k) * N + i] = TT[k] * d0 + TT[4 + k] * d1 + TT[8 + k] * d2;
        }
      }
      const double a0 = ax, a1 = ay, a2 = az, b0 = bx, b1 = by, b2 = bz;
      ax = TT[0] * a0 + TT[4] * a1 + TT[8] * a2; ay = TT[1] * a0 + TT[5] * a1 + TT[9] * a2; az = TT[2] * a0 + TT[6] * a1 + TT[10] * a2;
      bx = TT[0] * b0 + TT[4] * b1 + TT[8] * b2; by = TT[1] * b0 + TT[5] * b1 + TT[9] * b2; bz = TT[2] * b0 + TT[6] * b1 + TT[10] * b2;
    }
  }
  // task rows first, the rest zero
  const bool lin = task == 1, half = task != 0;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double top = J[k * N + i], bot = J[(3 + k) * N + i];
      J[k * N + i] = lin ? bot : top;
      J[(3 + k) * N + i] = half ? 0.0 : bot;
    }
  jd[0] = lin ? bx : ax; jd[1] = lin ? by : ay; jd[2] = lin ? bz : az;
  jd[3] = half ? 0.0 : bx; jd[4] = half ? 0.0 : by; jd[5] = half ? 0.0 : bz;
}

// M = L L^T (L over M, dg = its diagonal), W = L^-1 J^T over J, A = W^T W + lam2 1 factored in place (unit diagonal on the rows
// `task` leaves out).  Returns whether both factorisations had positive pivots.
template <int N, typename MT>
MP_HD bool mp_opspace_factor(const MT& M, int task, double lam2, const MpJointState<double, N>& js, double (&L)[N][N], double (&dg)[N],
                             double (&W)[6 * N], double (&A)[6][6]) {
  mp_mass_matrix_crba<double, N>(M, js, L);
  bool ok = mp_os_chol<N>(L, dg, 0.0);
#pragma unroll
  for (int k = 0; k < 6; ++k) mp_os_fwd<N>(L, &W[k * N]);
  const bool half = task != 0;
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int l = 0; l <= k; ++l) {
      double s = (k == l) ? lam2 : 0.0;
#pragma unroll
      for (int i = 0; i < N; ++i) s += W[k * N + i] * W[l * N + i];
      if (k == l && k >= 3) s = half ? 1.0 : s;
      A[k][l] = s;
    }
  double da[6];
  ok = mp_os_chol<6>(A, da, MP_OS_PIVOT_EPS) && ok;
  return ok;
}
MP_HD void mp_os_solve_A(const double (&A)[6][6], double (&b)[6]) {
  mp_os_fwd<6>(A, b);
  mp_os_back<6>(A, b);
}

template <int COUNT>
MP_HD void mp_os_head(const double* src, double (&dst)[COUNT]) {
#pragma unroll
  for (int k = 0; k < COUNT; ++k) dst[k] = src[k];
}

// Plain row stores (the CPU twin): row r of a (rows, COUNT) array
struct MpOsRowOut {
  long r;
  template <int COUNT>
  MP_HD void operator()(double* base, const double (&v)[COUNT]) const {
    for (int k = 0; k < COUNT; ++k) base[r * COUNT + k] = v[k];
  }
};

// One row of mp_opspace_f64: q = a, qd = b already loaded, `poison` = a non-finite input.  `out(ptr, values)` stores one row of an
// output (per row on the CPU, wave-cooperatively in the kernel: every lane of a wave arrives here with the same frame / task and
// the same null pointers).  Outputs: T (16), J (m n), Jdqd (m), Lam (m m), Jbar (n m), mu (m), p (m); any may be null.
template <int N, typename MT, typename OUT>
MP_HD void mp_opspace_row(const MT& M, const MpCall<double>& C, int frame, int task, double lam2, const double (&a)[N],
                          const double (&b)[N], bool poison, const OUT& out, double* Tout, double* Jout, double* Jdqd, double* Lam,
                          double* Jbar, double* mu, double* p) {
  const bool full = task == 0;
  MpJointState<double, N> js;
  mp_joint_state<double, N>(M, a, js);
  double TT[16], J[6 * N], jd[6];
  mp_opspace_kin<N>(M, frame, task, js, b, TT, J, jd);
  if (Tout) {
    mp_poison_if(poison, TT);
    out(Tout, TT);
  }
  if (Jout) {
    if (full) {
      double o[6 * N];
      mp_os_head(J, o);
      mp_poison_if(poison, o);
      out(Jout, o);
    } else {
      double o[3 * N];
      mp_os_head(J, o);
      mp_poison_if(poison, o);
      out(Jout, o);
    }
  }
  if (Jdqd) {
    if (full) {
      double o[6];
      mp_os_head(jd, o);
      mp_poison_if(poison, o);
      out(Jdqd, o);
    } else {
      double o[3];
      mp_os_head(jd, o);
      mp_poison_if(poison, o);
      out(Jdqd, o);
    }
  }
  if (!Lam && !Jbar && !mu && !p) return;
  if (mp_opspace_rank_deficient<N>(task, lam2)) {
    if (full) {
      mp_os_nan_out<36>(out, Lam); mp_os_nan_out<6 * N>(out, Jbar); mp_os_nan_out<6>(out, mu); mp_os_nan_out<6>(out, p);
    } else {
      mp_os_nan_out<9>(out, Lam); mp_os_nan_out<3 * N>(out, Jbar); mp_os_nan_out<3>(out, mu); mp_os_nan_out<3>(out, p);
    }
    return;
  }
  double L[N][N], dg[N], A[6][6];
  const bool bad = !mp_opspace_factor<N>(M, task, lam2, js, L, dg, J, A) || poison;  // J holds W from here on
  if (mu || p) {
    const double z3[3] = {0.0, 0.0, 0.0};
    double zero[N];
#pragma unroll
    for (int k = 0; k < N; ++k) zero[k] = 0.0;
    if (mu) {
      double c[N], rc[6];
      mp_rnea<double, N, false>(M, z3, z3, z3, js, b, zero, c);
      mp_os_fwd<N>(L, c);
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        double s = -jd[k];
#pragma unroll
        for (int i = 0; i < N; ++i) s += J[k * N + i] * c[i];
        rc[k] = s;
      }
      mp_os_solve_A(A, rc);
      mp_poison_if(bad, rc);
      if (full) {
        out(mu, rc);
      } else {
        double o[3];
        mp_os_head(rc, o);
        out(mu, o);
      }
    }
    if (p) {
      double g[N], rg[6];
      mp_rnea<double, N, false>(M, C.a0, z3, z3, js, zero, zero, g);
      mp_os_fwd<N>(L, g);
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) s += J[k * N + i] * g[i];
        rg[k] = s;
      }
      mp_os_solve_A(A, rg);
      mp_poison_if(bad, rg);
      if (full) {
        out(p, rg);
      } else {
        double o[3];
        mp_os_head(rg, o);
        out(p, o);
      }
    }
  }
  if (!Lam && !Jbar) return;
  double LL[6][6];  // Lambda, column by column (symmetric)
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double e[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) e[k] = (k == j) ? 1.0 : 0.0;
    mp_os_solve_A(A, e);
#pragma unroll
    for (int k = 0; k < 6; ++k) LL[k][j] = e[k];
  }
  if (Lam) {
    if (full) {
      double o[36];
#pragma unroll
      for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int l = 0; l < 6; ++l) o[k * 6 + l] = LL[k][l];
      mp_poison_if(bad, o);
      out(Lam, o);
    } else {
      double o[9];
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int l = 0; l < 3; ++l) o[k * 3 + l] = LL[k][l];
      mp_poison_if(bad, o);
      out(Lam, o);
    }
  }
  if (Jbar) {  // column j:  L^-T (W Lambda_j)
    double JB[N][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double x[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s += J[k * N + i] * LL[k][j];
        x[i] = s;
      }
      mp_os_back<N>(L, x);
#pragma unroll
      for (int i = 0; i < N; ++i) JB[i][j] = x[i];
    }
    if (full) {
      double o[6 * N];
#pragma unroll
      for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) o[i * 6 + j] = JB[i][j];
      mp_poison_if(bad, o);
      out(Jbar, o);
    } else {
      double o[3 * N];
#pragma unroll
      for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[i * 3 + j] = JB[i][j];
      mp_poison_if(bad, o);
      out(Jbar, o);
    }
  }
}

// One row of mp_opspace_torque_f64: q = a, qd = b, the task acceleration acc (its m values first, the rest zero), tau0 = t0 (zeros
// for none); tau <- the task-space computed torque.  `poison` = a non-finite input; a non-positive pivot poisons the row too.
template <int N, typename MT>
MP_HD void mp_opspace_torque_row(const MT& M, const MpCall<double>& C, int frame, int task, double lam2, const double (&a)[N],
                                 const double (&b)[N], const double (&acc)[6], const double (&t0)[N], bool poison, double (&tau)[N]) {
  if (mp_opspace_rank_deficient<N>(task, lam2)) {
#pragma unroll
    for (int i = 0; i < N; ++i) tau[i] = 0.0;
    mp_poison_if(true, tau);
    return;
  }
  MpJointState<double, N> js;
  mp_joint_state<double, N>(M, a, js);
  double TT[16], W[6 * N], jd[6];
  mp_opspace_kin<N>(M, frame, task, js, b, TT, W, jd);
  double L[N][N], dg[N], A[6][6];
  const bool bad = !mp_opspace_factor<N>(M, task, lam2, js, L, dg, W, A) || poison;
  double h[N];
  {
    const double z3[3] = {0.0, 0.0, 0.0};
    double zero[N];
#pragma unroll
    for (int k = 0; k < N; ++k) zero[k] = 0.0;
    mp_rnea<double, N, false>(M, C.a0, z3, z3, js, b, zero, h);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) h[i] -= t0[i];
  mp_os_fwd<N>(L, h);
  double f[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double s = acc[k] - jd[k];
#pragma unroll
    for (int i = 0; i < N; ++i) s += W[k * N + i] * h[i];
    f[k] = s;
  }
  mp_os_solve_A(A, f);
  double v[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s += W[k * N + i] * f[k];
    v[i] = s;
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {  // J^T f = L v
    double s = dg[i] * v[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s += L[i][k] * v[k];
    tau[i] = s + t0[i];
  }
  mp_poison_if(bad, tau);
}

// The CPU twins' rows: plain (rows, *) arrays
template <int N, typename MT>
MP_HD void mp_opspace_cpu_row(const MT& M, const MpCall<double>& C, int frame, int task, double lam2, const double* q, const double* qd,
                              double* Tout, double* Jout, double* Jdqd, double* Lam, double* Jbar, double* mu, double* p, long r) {
  double a[N], b[N];
#pragma unroll
  for (int k = 0; k < N; ++k) { a[k] = q[r * N + k]; b[k] = qd[r * N + k]; }
  MpBad<double> bad;
  bad.add(a); bad.add(b);
  const MpOsRowOut out{r};
  mp_opspace_row<N>(M, C, frame, task, lam2, a, b, bad.any(), out, Tout, Jout, Jdqd, Lam, Jbar, mu, p);
}
template <int N, typename MT>
MP_HD void mp_opspace_torque_cpu_row(const MT& M, const MpCall<double>& C, int frame, int task, double lam2, const double* q,
                                     const double* qd, const double* acc, const double* tau0, double* tau, long r) {
  const int m = mp_opspace_dim(task);
  double a[N], b[N], x[6], t0[N], t[N];
#pragma unroll
  for (int k = 0; k < N; ++k) { a[k] = q[r * N + k]; b[k] = qd[r * N + k]; t0[k] = tau0 ? tau0[r * N + k] : 0.0; }
#pragma unroll
  for (int k = 0; k < 6; ++k) x[k] = k < m ? acc[r * m + k] : 0.0;
  MpBad<double> bad;
  bad.add(a); bad.add(b); bad.add(x); bad.add(t0);
  mp_opspace_torque_row<N>(M, C, frame, task, lam2, a, b, x, t0, bad.any(), t);
#pragma unroll
  for (int k = 0; k < N; ++k) tau[r * N + k] = t[k];
}
