// Inverse-dynamics regressor: tau = Y(q, qd, qdd, g) pi + tau_ext(q, Ftip), one row per call (float64, 1..MP_MAX_DOF joints,
// unrolled).  Header-only like mp_deriv.h: the HIP kernels (mp_kernels.hip) and the CPU twins (mp_cpu.cpp) instantiate it.
//
// Parameters.  Per link k, pi_k = [m, hx, hy, hz, Ixx, Ixy, Ixz, Iyy, Iyz, Izz] in the PUBLIC convention: link k's CoM frame at
// the home pose (Mlist_per_link[k]), h = m c with c the centre of mass from that frame's origin, I about that origin.  The
// compiled link frames hold pi_link,k = D_k pi_k (a constant 10 x 10 map the model compiler builds next to its inertia step,
// mp_model_compile.cpp, mp_inertial_map); Y is returned in the public convention, (n, 10n) a row, [j][10 k + c].
//
// Method.  One primal pass (mp_deriv_primal, the same compiled frames and axis-aligned steps, gravity as a base acceleration)
// gives every link's twist V_k and acceleration A_k.  The body wrench of link k, I_k A_k + V_k x* I_k V_k, is linear in
// pi_link,k; column c of Y's block k is that wrench at pi_link = D_k e_c (column c of D_k: the map folds into the wrench, so the
// row never holds a link-frame block), carried down the chain with the force steps of the backward pass and projected on
// every joint axis j <= k.  Y[j][block k] = 0 for k < j.  O(10 n^2) link steps a row.
//
// tau_ext is the tip wrench's share, which no inertial parameter scales: the wrench carried to link n and back.
//
// A row with a non-finite input (in the normal-equations pass, its right-hand side too) gets NaN in its whole row of Y and of
// tau_ext.
#pragma once

#include "mp_deriv.h"

constexpr int MP_REG_P = 10;   // inertial parameters a link

// Twist and acceleration of every link in its own frame, after the joint's terms
template <typename T, int N>
struct MpRegFwd {
  MpJointState<T, N> js;
  T wx[N], wy[N], wz[N], vx[N], vy[N], vz[N];
  T ax[N], ay[N], az[N], bx[N], by[N], bz[N];
};
template <typename T, int N>
struct MpRegHook {
  MpRegFwd<T, N>* F;
  MP_HD void operator()(int i, T wx, T wy, T wz, T vx, T vy, T vz, T ax, T ay, T az, T bx, T by, T bz) const {
    F->wx[i] = wx; F->wy[i] = wy; F->wz[i] = wz; F->vx[i] = vx; F->vy[i] = vy; F->vz[i] = vz;
    F->ax[i] = ax; F->ay[i] = ay; F->az[i] = az; F->bx[i] = bx; F->by[i] = by; F->bz[i] = bz;
  }
};

template <typename T, int N, typename MT>
MP_HD void mp_reg_forward(const MT& M, const MpCall<T>& C, const T (&q)[N], const T (&qd)[N], const T (&qdd)[N], MpRegFwd<T, N>& F) {
  MpDerivPrimal<T, N> P;
  T tau[N];
  mp_deriv_primal<T, N, false>(M, C, q, qd, qdd, P, tau, MpRegHook<T, N>{&F});
  F.js = P.js;
}

// Body wrench (n, f) of link k for the link-frame parameters p = [m, h, I]: the primal's wrench with (m, h, I) read from p
template <typename T, int N, typename PT>
MP_HD void mp_reg_wrench(const MpRegFwd<T, N>& F, int k, const PT* p, T& fnx, T& fny, T& fnz, T& ffx, T& ffy, T& ffz) {
  const T m = p[0], hx = p[1], hy = p[2], hz = p[3], Ixx = p[4], Ixy = p[5], Ixz = p[6], Iyy = p[7], Iyz = p[8], Izz = p[9];
  const T wx = F.wx[k], wy = F.wy[k], wz = F.wz[k], vx = F.vx[k], vy = F.vy[k], vz = F.vz[k];
  const T dwx = F.ax[k], dwy = F.ay[k], dwz = F.az[k], dvx = F.bx[k], dvy = F.by[k], dvz = F.bz[k];
  const T pnx = Ixx * wx + Ixy * wy + Ixz * wz + (hy * vz - hz * vy);
  const T pny = Ixy * wx + Iyy * wy + Iyz * wz + (hz * vx - hx * vz);
  const T pnz = Ixz * wx + Iyz * wy + Izz * wz + (hx * vy - hy * vx);
  const T pfx = m * vx - (hy * wz - hz * wy);
  const T pfy = m * vy - (hz * wx - hx * wz);
  const T pfz = m * vz - (hx * wy - hy * wx);
  fnx = Ixx * dwx + Ixy * dwy + Ixz * dwz + (hy * dvz - hz * dvy) + (wy * pnz - wz * pny) + (vy * pfz - vz * pfy);
  fny = Ixy * dwx + Iyy * dwy + Iyz * dwz + (hz * dvx - hx * dvz) + (wz * pnx - wx * pnz) + (vz * pfx - vx * pfz);
  fnz = Ixz * dwx + Iyz * dwy + Izz * dwz + (hx * dvy - hy * dvx) + (wx * pny - wy * pnx) + (vx * pfy - vy * pfx);
  ffx = m * dvx - (hy * dwz - hz * dwy) + (wy * pfz - wz * pfy);
  ffy = m * dvy - (hz * dwx - hx * dwz) + (wz * pfx - wx * pfz);
  ffz = m * dvz - (hx * dwy - hy * dwx) + (wx * pfy - wy * pfx);
}

// One column of Y's block k: the wrench of link k at the link-frame parameters p, carried down to joint 0; y[j] = 0 for j > k.
// `k` may be a run-time value (the per-link tests on it are then wave-uniform branches).
template <typename T, int N, typename MT, typename PT>
MP_HD void mp_reg_column(const MT& M, const MpRegFwd<T, N>& F, int k, const PT* p, T (&y)[N]) {
  T nx, ny, nz, fx, fy, fz;
  mp_reg_wrench<T, N>(F, k, p, nx, ny, nz, fx, fy, fz);
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    if (i > k) { y[i] = 0.0; continue; }
    const auto& J = mp_joint_of(M, i);
    y[i] = J.rev * nz + (1.0 - J.rev) * fz;
    if (i > 0) {
      mp_force_up_B(F.js.c[i], F.js.s[i], F.js.d[i], nx, ny, nz, fx, fy, fz);
      mp_force_up_A(J.ca, J.sa, J.a, nx, ny, nz, fx, fy, fz);
    }
  }
}

// tau_ext: the tip wrench carried down to link n (mp_deriv_primal's steps) and back up
template <typename T, int N, typename MT>
MP_HD void mp_reg_tau_ext(const MT& M, const MpCall<T>& C, const MpJointState<T, N>& js, T (&te)[N]) {
  T nx = C.F1n[0], ny = C.F1n[1], nz = C.F1n[2], fx = C.F1f[0], fy = C.F1f[1], fz = C.F1f[2];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const auto& J = mp_joint_of(M, i);
    if (i > 0) mp_force_down_A(J.ca, J.sa, J.a, nx, ny, nz, fx, fy, fz);
    mp_force_down_B(js.c[i], js.s[i], js.d[i], nx, ny, nz, fx, fy, fz);
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    const auto& J = mp_joint_of(M, i);
    te[i] = J.rev * nz + (1.0 - J.rev) * fz;
    if (i > 0) {
      mp_force_up_B(js.c[i], js.s[i], js.d[i], nx, ny, nz, fx, fy, fz);
      mp_force_up_A(J.ca, J.sa, J.a, nx, ny, nz, fx, fy, fz);
    }
  }
}

// ------------------------------------------------------------------------------------------- rows
// Dmap: n x 10 x 10 doubles, [k][a][c] = d pi_link,k[a] / d pi_k[c] (mp_inertial_map).  Row `r` of (rows, n) inputs; Y is
// (rows, n, 10n) with element [r][j][10 k + c] at r 10 n^2 + j 10 n + 10 k + c (64-bit offsets: Y passes 2^31 elements at
// ~5.4e6 rows, n = 8).  tau_ext (rows, n) may be null.
template <int N, bool HAS_FTIP, typename MT>
MP_HD void mp_id_regressor_row(const MT& M, const double* Dmap, const MpCall<double>& C, const double* q, const double* qd,
                               const double* qdd, double* Y, double* tau_ext, long r) {
  using T = double;
  constexpr int W = MP_REG_P * N;
  T a[N], b[N], c[N];
#pragma unroll
  for (int k = 0; k < N; ++k) { a[k] = q[r * N + k]; b[k] = qd[r * N + k]; c[k] = qdd[r * N + k]; }
  MpBad<T> bad;
  bad.add(a); bad.add(b); bad.add(c);
  const bool poison = bad.any();
  MpRegFwd<T, N> F;
  mp_reg_forward<T, N>(M, C, a, b, c, F);
  const long base = r * (long)(N * W);
#pragma unroll
  for (int k = 0; k < N; ++k) {
#pragma unroll
    for (int cc = 0; cc < MP_REG_P; ++cc) {
      T p[MP_REG_P];
#pragma unroll
      for (int e = 0; e < MP_REG_P; ++e) p[e] = Dmap[(k * MP_REG_P + e) * MP_REG_P + cc];
      T y[N];
      mp_reg_column<T, N>(M, F, k, p, y);
      mp_poison_if(poison, y);
#pragma unroll
      for (int j = 0; j < N; ++j) Y[base + j * W + k * MP_REG_P + cc] = y[j];
    }
  }
  if (tau_ext) {
    T te[N];
    if (HAS_FTIP) mp_reg_tau_ext<T, N>(M, C, F.js, te);
    else {
#pragma unroll
      for (int j = 0; j < N; ++j) te[j] = 0.0;
    }
    mp_poison_if(poison, te);
#pragma unroll
    for (int j = 0; j < N; ++j) tau_ext[r * N + j] = te[j];
  }
}

// Normal equations: the part of one row that a worker `sub` of `lanes` builds - the columns c = sub, sub + lanes, ... of every
// block, `put(j, col, value)` for j = 0..n-1 (zeros included), and (sub == 0) the residual rhs - tau_ext, `res(j, value)`.
// Every worker of a row repeats its primal pass (a few hundred operations against ~10 n^2 link steps for the columns).
template <int N, bool HAS_FTIP, int LANES, typename MT, typename PUT, typename RES>
MP_HD void mp_id_regressor_normal_part(const MT& M, const double* Dmap, const MpCall<double>& C, const double* q, const double* qd,
                                       const double* qdd, const double* rhs, long r, int sub, const PUT& put, const RES& res) {
  using T = double;
  T a[N], b[N], c[N], t[N];
#pragma unroll
  for (int k = 0; k < N; ++k) { a[k] = q[r * N + k]; b[k] = qd[r * N + k]; c[k] = qdd[r * N + k]; t[k] = rhs[r * N + k]; }
  MpBad<T> bad;
  bad.add(a); bad.add(b); bad.add(c); bad.add(t);
  const bool poison = bad.any();
  MpRegFwd<T, N> F;
  mp_reg_forward<T, N>(M, C, a, b, c, F);
#pragma unroll
  for (int k = 0; k < N; ++k) {
#pragma unroll
    for (int cc = 0; cc < (MP_REG_P + LANES - 1) / LANES; ++cc) {
      const int col = sub + cc * LANES;
      if (col < MP_REG_P) {
        T p[MP_REG_P];
#pragma unroll
        for (int e = 0; e < MP_REG_P; ++e) p[e] = Dmap[(k * MP_REG_P + e) * MP_REG_P + col];
        T y[N];
        mp_reg_column<T, N>(M, F, k, p, y);
        mp_poison_if(poison, y);
#pragma unroll
        for (int j = 0; j < N; ++j) put(j, k * MP_REG_P + col, y[j]);
      }
    }
  }
  if (sub == 0) {
    T te[N];
    if (HAS_FTIP) mp_reg_tau_ext<T, N>(M, C, F.js, te);
    else {
#pragma unroll
      for (int j = 0; j < N; ++j) te[j] = 0.0;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) te[j] = t[j] - te[j];
    mp_poison_if(poison, te);
#pragma unroll
    for (int j = 0; j < N; ++j) res(j, te[j]);
  }
}
