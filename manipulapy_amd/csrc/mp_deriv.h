// Analytical first derivatives of inverse and forward dynamics, one row per call (float64, 1..MP_MAX_DOF joints, unrolled).
// Header-only like mp_core.h: the HIP kernels (mp_kernels.hip) and the CPU twins (mp_cpu.cpp) instantiate the same templates.
//
//   inverse dynamics   tau = ID(q, qd, qdd, g, Ftip)          ->  dtau_dq, dtau_dqd, dtau_dqdd = M(q)
//   forward dynamics   qdd = FD(q, qd, tau, g, Ftip)          ->  dqdd_dq = -M^-1 dtau_dq,  dqdd_dqd = -M^-1 dtau_dqd,
//                                                                 dqdd_dtau = M^-1   (dtau_* taken at that qdd)
// Layout of every (n, n) block: [i][j] = d out_i / d in_j (torch.autograd.functional.jacobian's convention), rows contiguous.
// Derivatives are those of the UNCLIPPED tau (the torque limits of the model are not applied, as in mp_rnea).
//
// Method: forward-mode tangents through the recursive Newton-Euler pass of mp_rnea_impl, in the same compiled link frames and with
// the same axis-aligned steps.  One primal pass keeps, per link, what the tangent sweeps read back (MpDerivPrimal: sin / cos / shift,
// the link twist, the pre-joint acceleration and tip-wrench components, the transmitted wrench after its Rz step); then one sweep
// per direction:
//   q_j  - the tangent is born at link j, where the joint's own step Rz(theta_j) Tz(d_j) moves with q_j.  d/dtheta of that step
//          applied to a motion vector u is (u'y, -u'x, 0 | ...) of the stepped vector u' (one planar rotation by 90 degrees), and
//          the same for the tip wrench on the way down and for the transmitted wrench on the way up (mp_deriv_dstep_* below);
//   qd_j - born at link j through the joint-rate terms S qd and V x S qd.
// Links before j carry a zero tangent, so the sweep for direction j starts there: sum over j of (n - j) links forward and n back,
// O(n^2) per row (~n^2 + n^2 / 2 link steps for each of the two direction families).  The tip wrench's term Js^T F depends on q
// through the transforms that carry F down to link n: its tangent rides the sweep like the twist's.
#pragma once

#include "mp_core.h"

// Primal per-link state the tangent sweeps read (float64: ~20 values a link)
template <typename T, int N>
struct MpDerivPrimal {
  MpJointState<T, N> js;
  T wx[N], wy[N], wz[N], vx[N], vy[N], vz[N];  // link twist in link frame i (after the joint's own rate is added)
  T awx[N], awy[N], avx[N], avy[N];            // acceleration after the Rz step, before the joint's terms (x / y components)
  T tnx[N], tny[N], tfx[N], tfy[N];            // tip wrench after the Rz step of link i (HAS_FTIP only)
  T unx[N], uny[N], ufx[N], ufy[N];            // wrench transmitted by joint i after its Rz step towards link i - 1 (i > 0)
};

// d/dq of the Rz(theta) Tz(d) motion step at the stepped vector (w', v'):  revolute  (w'y, -w'x, 0 | v'y, -v'x, 0),
// prismatic (0, 0, 0 | w'y, -w'x, 0); `rev` blends.  Also the step of a force vector down the chain, with (n, f) for (v, w).
template <typename T, typename S>
MP_HD void mp_deriv_dstep_down(S rev, T wx, T wy, T vx, T vy, T& dwx, T& dwy, T& dvx, T& dvy) {
  const S p = S(1) - rev;
  dwx = rev * wy;
  dwy = -(rev * wx);
  dvx = rev * vy + p * wy;
  dvy = -(rev * vx + p * wx);
}
// d/dq of the force step up the chain (mp_force_up_B) at the stepped wrench (n', f'):  revolute (-n'y, n'x, 0 | -f'y, f'x, 0),
// prismatic (-f'y, f'x, 0 | 0, 0, 0)
template <typename T, typename S>
MP_HD void mp_deriv_dstep_up(S rev, T nx, T ny, T fx, T fy, T& dnx, T& dny, T& dfx, T& dfy) {
  const S p = S(1) - rev;
  dnx = -(rev * ny + p * fy);
  dny = rev * nx + p * fx;
  dfx = -(rev * fy);
  dfy = rev * fx;
}

// No per-link observer (what every derivative pass uses)
struct MpDerivNoHook {
  template <typename T> MP_HD void operator()(int, T, T, T, T, T, T, T, T, T, T, T, T) const {}
};

// The primal recursion (mp_rnea_impl's arithmetic, in the same order) keeping what the sweeps need; tau is not clipped.
// `hook(i, twist w, v, acceleration dw, dv)` sees each link's final twist and acceleration in link frame i (the dynamics
// regressor, mp_regressor.h, reads them there).
template <typename T, int N, bool HAS_FTIP, typename MT, typename H = MpDerivNoHook>
MP_HD void mp_deriv_primal(const MT& M, const MpCall<T>& C, const T (&q)[N], const T (&qd)[N], const T (&qdd)[N],
                           MpDerivPrimal<T, N>& P, T (&tau)[N], const H& hook = H()) {
  mp_joint_state<T, N>(M, q, P.js);
  T fnx[N], fny[N], fnz[N], ffx[N], ffy[N], ffz[N];
  T wx = 0, wy = 0, wz = 0, vx = 0, vy = 0, vz = 0;
  T dwx = 0, dwy = 0, dwz = 0, dvx = C.a0[0], dvy = C.a0[1], dvz = C.a0[2];
  T tnx = 0, tny = 0, tnz = 0, tfx = 0, tfy = 0, tfz = 0;
  if (HAS_FTIP) { tnx = C.F1n[0]; tny = C.F1n[1]; tnz = C.F1n[2]; tfx = C.F1f[0]; tfy = C.F1f[1]; tfz = C.F1f[2]; }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const auto& J = mp_joint_of(M, i);
    if (i > 0) {
      mp_motion_A(J.ca, J.sa, J.a, wx, wy, wz, vx, vy, vz);
      mp_motion_A(J.ca, J.sa, J.a, dwx, dwy, dwz, dvx, dvy, dvz);
      if (HAS_FTIP) mp_force_down_A(J.ca, J.sa, J.a, tnx, tny, tnz, tfx, tfy, tfz);
    }
    const T c = P.js.c[i], s = P.js.s[i], d = P.js.d[i];
    mp_motion_B(c, s, d, wx, wy, wz, vx, vy, vz);
    mp_motion_B(c, s, d, dwx, dwy, dwz, dvx, dvy, dvz);
    if (HAS_FTIP) {
      mp_force_down_B(c, s, d, tnx, tny, tnz, tfx, tfy, tfz);
      P.tnx[i] = tnx; P.tny[i] = tny; P.tfx[i] = tfx; P.tfy[i] = tfy;
    }
    P.awx[i] = dwx; P.awy[i] = dwy; P.avx[i] = dvx; P.avy[i] = dvy;
    const T qdr = J.rev * qd[i], qdp = qd[i] - qdr;
    const T ar = J.rev * qdd[i], ap = qdd[i] - ar;
    wz += qdr;
    vz += qdp;
    dwx += qdr * wy;
    dwy -= qdr * wx;
    dwz += ar;
    dvx += qdr * vy + qdp * wy;
    dvy -= qdr * vx + qdp * wx;
    dvz += ap;
    P.wx[i] = wx; P.wy[i] = wy; P.wz[i] = wz; P.vx[i] = vx; P.vy[i] = vy; P.vz[i] = vz;
    hook(i, wx, wy, wz, vx, vy, vz, dwx, dwy, dwz, dvx, dvy, dvz);
    const T pnx = J.Ixx * wx + J.Ixy * wy + J.Ixz * wz + (J.hy * vz - J.hz * vy);
    const T pny = J.Ixy * wx + J.Iyy * wy + J.Iyz * wz + (J.hz * vx - J.hx * vz);
    const T pnz = J.Ixz * wx + J.Iyz * wy + J.Izz * wz + (J.hx * vy - J.hy * vx);
    const T pfx = J.m * vx - (J.hy * wz - J.hz * wy);
    const T pfy = J.m * vy - (J.hz * wx - J.hx * wz);
    const T pfz = J.m * vz - (J.hx * wy - J.hy * wx);
    fnx[i] = J.Ixx * dwx + J.Ixy * dwy + J.Ixz * dwz + (J.hy * dvz - J.hz * dvy) + (wy * pnz - wz * pny) + (vy * pfz - vz * pfy);
    fny[i] = J.Ixy * dwx + J.Iyy * dwy + J.Iyz * dwz + (J.hz * dvx - J.hx * dvz) + (wz * pnx - wx * pnz) + (vz * pfx - vx * pfz);
    fnz[i] = J.Ixz * dwx + J.Iyz * dwy + J.Izz * dwz + (J.hx * dvy - J.hy * dvx) + (wx * pny - wy * pnx) + (vx * pfy - vy * pfx);
    ffx[i] = J.m * dvx - (J.hy * dwz - J.hz * dwy) + (wy * pfz - wz * pfy);
    ffy[i] = J.m * dvy - (J.hz * dwx - J.hx * dwz) + (wz * pfx - wx * pfz);
    ffz[i] = J.m * dvz - (J.hx * dwy - J.hy * dwx) + (wx * pfy - wy * pfx);
  }
  if (HAS_FTIP) {
    fnx[N - 1] += tnx; fny[N - 1] += tny; fnz[N - 1] += tnz;
    ffx[N - 1] += tfx; ffy[N - 1] += tfy; ffz[N - 1] += tfz;
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    const auto& J = mp_joint_of(M, i);
    tau[i] = J.rev * fnz[i] + (1.0 - J.rev) * ffz[i];
    if (i > 0) {
      T nx = fnx[i], ny = fny[i], nz = fnz[i], fx = ffx[i], fy = ffy[i], fz = ffz[i];
      mp_force_up_B(P.js.c[i], P.js.s[i], P.js.d[i], nx, ny, nz, fx, fy, fz);
      P.unx[i] = nx; P.uny[i] = ny; P.ufx[i] = fx; P.ufy[i] = fy;
      mp_force_up_A(J.ca, J.sa, J.a, nx, ny, nz, fx, fy, fz);
      fnx[i - 1] += nx; fny[i - 1] += ny; fnz[i - 1] += nz;
      ffx[i - 1] += fx; ffy[i - 1] += fy; ffz[i - 1] += fz;
    }
  }
}

// One tangent sweep: dtau (column j of dtau_dq when WRT_Q, of dtau_dqd otherwise).  `j` may be a run-time value: the per-link
// tests on it are wave-uniform branches.
template <typename T, int N, bool HAS_FTIP, bool WRT_Q, typename MT>
MP_HD void mp_deriv_sweep(const MT& M, const MpDerivPrimal<T, N>& P, const T (&qd)[N], int j, T (&dtau)[N]) {
  T bnx[N], bny[N], bnz[N], bfx[N], bfy[N], bfz[N];  // tangent of the body wrenches (links >= j)
  T wx = 0, wy = 0, wz = 0, vx = 0, vy = 0, vz = 0;            // tangent of the twist
  T ax = 0, ay = 0, az = 0, bx = 0, by = 0, bz = 0;            // tangent of the acceleration
  T tnx = 0, tny = 0, tnz = 0, tfx = 0, tfy = 0, tfz = 0;      // tangent of the tip wrench
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (i < j) continue;
    const auto& J = mp_joint_of(M, i);
    const T c = P.js.c[i], s = P.js.s[i], d = P.js.d[i];
    if (i > j) {
      mp_motion_A(J.ca, J.sa, J.a, wx, wy, wz, vx, vy, vz);
      mp_motion_A(J.ca, J.sa, J.a, ax, ay, az, bx, by, bz);
      if (HAS_FTIP) mp_force_down_A(J.ca, J.sa, J.a, tnx, tny, tnz, tfx, tfy, tfz);
      mp_motion_B(c, s, d, wx, wy, wz, vx, vy, vz);
      mp_motion_B(c, s, d, ax, ay, az, bx, by, bz);
      if (HAS_FTIP) mp_force_down_B(c, s, d, tnx, tny, tnz, tfx, tfy, tfz);
    } else if (WRT_Q) {  // i == j: the joint's own step moves (the tangents before it are zero)
      // the twist after the Rz step: x / y components are those after the joint's rate is added
      mp_deriv_dstep_down(J.rev, P.wx[i], P.wy[i], P.vx[i], P.vy[i], wx, wy, vx, vy);
      mp_deriv_dstep_down(J.rev, P.awx[i], P.awy[i], P.avx[i], P.avy[i], ax, ay, bx, by);
      if (HAS_FTIP) mp_deriv_dstep_down(J.rev, P.tfx[i], P.tfy[i], P.tnx[i], P.tny[i], tfx, tfy, tnx, tny);
    }
    // the joint's terms:  w += S_w qd,  v += S_v qd,  a += S qdd + V x S qd   (their tangents)
    const T pw = wx, qw = wy, pv = vx, qv = vy;  // (twist tangent x / y: the rate adds only to z)
    const T qdr = J.rev * qd[i], qdp = qd[i] - qdr;
    ax += qdr * qw;
    ay -= qdr * pw;
    bx += qdr * qv + qdp * qw;
    by -= qdr * pv + qdp * pw;
    if (!WRT_Q && i == j) {  // d/dqd_j: S_j enters the twist, V x S_j the acceleration
      const double r = J.rev, p = 1.0 - J.rev;
      wz += r;
      vz += p;
      ax += r * P.wy[i];
      ay -= r * P.wx[i];
      bx += r * P.vy[i] + p * P.wy[i];
      by -= r * P.vx[i] + p * P.wx[i];
    }
    // body wrench F = G a + [w x Pn + v x Pf ; w x Pf],  P = G V:  dF = G da + [dw x Pn + w x dPn + dv x Pf + v x dPf ; dw x Pf + w x dPf]
    const T Wx = P.wx[i], Wy = P.wy[i], Wz = P.wz[i], Vx = P.vx[i], Vy = P.vy[i], Vz = P.vz[i];
    const T pnx = J.Ixx * Wx + J.Ixy * Wy + J.Ixz * Wz + (J.hy * Vz - J.hz * Vy);
    const T pny = J.Ixy * Wx + J.Iyy * Wy + J.Iyz * Wz + (J.hz * Vx - J.hx * Vz);
    const T pnz = J.Ixz * Wx + J.Iyz * Wy + J.Izz * Wz + (J.hx * Vy - J.hy * Vx);
    const T pfx = J.m * Vx - (J.hy * Wz - J.hz * Wy);
    const T pfy = J.m * Vy - (J.hz * Wx - J.hx * Wz);
    const T pfz = J.m * Vz - (J.hx * Wy - J.hy * Wx);
    const T qnx = J.Ixx * wx + J.Ixy * wy + J.Ixz * wz + (J.hy * vz - J.hz * vy);
    const T qny = J.Ixy * wx + J.Iyy * wy + J.Iyz * wz + (J.hz * vx - J.hx * vz);
    const T qnz = J.Ixz * wx + J.Iyz * wy + J.Izz * wz + (J.hx * vy - J.hy * vx);
    const T qfx = J.m * vx - (J.hy * wz - J.hz * wy);
    const T qfy = J.m * vy - (J.hz * wx - J.hx * wz);
    const T qfz = J.m * vz - (J.hx * wy - J.hy * wx);
    bnx[i] = J.Ixx * ax + J.Ixy * ay + J.Ixz * az + (J.hy * bz - J.hz * by) + (wy * pnz - wz * pny) + (Wy * qnz - Wz * qny) +
             (vy * pfz - vz * pfy) + (Vy * qfz - Vz * qfy);
    bny[i] = J.Ixy * ax + J.Iyy * ay + J.Iyz * az + (J.hz * bx - J.hx * bz) + (wz * pnx - wx * pnz) + (Wz * qnx - Wx * qnz) +
             (vz * pfx - vx * pfz) + (Vz * qfx - Vx * qfz);
    bnz[i] = J.Ixz * ax + J.Iyz * ay + J.Izz * az + (J.hx * by - J.hy * bx) + (wx * pny - wy * pnx) + (Wx * qny - Wy * qnx) +
             (vx * pfy - vy * pfx) + (Vx * qfy - Vy * qfx);
    bfx[i] = J.m * bx - (J.hy * az - J.hz * ay) + (wy * pfz - wz * pfy) + (Wy * qfz - Wz * qfy);
    bfy[i] = J.m * by - (J.hz * ax - J.hx * az) + (wz * pfx - wx * pfz) + (Wz * qfx - Wx * qfz);
    bfz[i] = J.m * bz - (J.hx * ay - J.hy * ax) + (wx * pfy - wy * pfx) + (Wx * qfy - Wy * qfx);
  }
  if (HAS_FTIP) {
    bnx[N - 1] += tnx; bny[N - 1] += tny; bnz[N - 1] += tnz;
    bfx[N - 1] += tfx; bfy[N - 1] += tfy; bfz[N - 1] += tfz;
  }
  // backward: the tangent of the transmitted wrench; joint j's up step moves with q_j
  T nx = 0, ny = 0, nz = 0, fx = 0, fy = 0, fz = 0;
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    const auto& J = mp_joint_of(M, i);
    if (i >= j) { nx += bnx[i]; ny += bny[i]; nz += bnz[i]; fx += bfx[i]; fy += bfy[i]; fz += bfz[i]; }
    dtau[i] = J.rev * nz + (1.0 - J.rev) * fz;
    if (i > 0) {
      mp_force_up_B(P.js.c[i], P.js.s[i], P.js.d[i], nx, ny, nz, fx, fy, fz);
      if (WRT_Q && i == j) {
        T dnx, dny, dfx, dfy;
        mp_deriv_dstep_up(J.rev, P.unx[i], P.uny[i], P.ufx[i], P.ufy[i], dnx, dny, dfx, dfy);
        nx += dnx; ny += dny; fx += dfx; fy += dfy;
      }
      mp_force_up_A(J.ca, J.sa, J.a, nx, ny, nz, fx, fy, fz);
    }
  }
}

// Direction loop: unrolled (every sweep's `i < j` folds at compile time; n x the code) or rolled (one copy, wave-uniform branches).
// Unrolled is faster everywhere on MI355X (4e6 rows; UR5 ID 2.34 against 2.72 ms, Panda 5.69 against 7.49 ms): profiles/HISTORY.md.
#ifndef MP_DERIV_UNROLL
#define MP_DERIV_UNROLL 1
#endif
#if MP_DERIV_UNROLL
#define MP_DERIV_DIRS _Pragma("unroll")
#else
#define MP_DERIV_DIRS MP_ROLLED
#endif

// Cholesky of the SPD M in place (the factorisation half of mp_spd_solve, mp_core.h) and one solve with the factor.
template <typename T, int N>
MP_HD void mp_deriv_chol(T (&A)[N][N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    T d = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
    const T inv = mp_rsqrt(d);
    A[j][j] = inv;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      T v = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
      A[i][j] = v * inv;
    }
  }
}
template <typename T, int N>
MP_HD void mp_deriv_chol_solve(const T (&A)[N][N], T (&b)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    T v = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= A[i][k] * b[k];
    b[i] = v * A[i][i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    T v = b[i];
#pragma unroll
    for (int k = i + 1; k < N; ++k) v -= A[k][i] * b[k];
    b[i] = v * A[i][i];
  }
}

// ------------------------------------------------------------------------------------------- rows
// Row `r` of (rows, n) inputs; 64-bit offsets throughout (the (rows, n, n) outputs pass 2^31 elements at ~3.4e7 rows, n = 8).
// A row with a non-finite input gets NaN in every output of that row only.  Column j of an (n, n) output is written as it is
// produced: element [r][i][j] at r n^2 + i n + j.

// inverse dynamics: tau (may be null), dtau_dq, dtau_dqd, M = dtau_dqdd (may be null)
template <int N, bool HAS_FTIP, typename MT>
MP_HD void mp_id_deriv_row(const MT& M, const MpCall<double>& C, const double* q, const double* qd, const double* qdd, double* tau,
                           double* dq, double* dqd, double* Mout, long r) {
  using T = double;
  T a[N], b[N], c[N];
#pragma unroll
  for (int k = 0; k < N; ++k) { a[k] = q[r * N + k]; b[k] = qd[r * N + k]; c[k] = qdd[r * N + k]; }
  MpBad<T> bad;
  bad.add(a); bad.add(b); bad.add(c);
  const bool poison = bad.any();
  MpDerivPrimal<T, N> P;
  T t[N];
  mp_deriv_primal<T, N, HAS_FTIP>(M, C, a, b, c, P, t);
  const long base = r * (long)(N * N);
  if (tau) {
    mp_poison_if(poison, t);
#pragma unroll
    for (int k = 0; k < N; ++k) tau[r * N + k] = t[k];
  }
  if (Mout) {
    T Mq[N][N];
    mp_mass_matrix_crba<T, N>(M, P.js, Mq);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      mp_poison_if(poison, Mq[i]);
#pragma unroll
      for (int k = 0; k < N; ++k) Mout[base + i * N + k] = Mq[i][k];
    }
  }
  MP_DERIV_DIRS
  for (int j = 0; j < N; ++j) {
    T col[N];
    mp_deriv_sweep<T, N, HAS_FTIP, true>(M, P, b, j, col);
    mp_poison_if(poison, col);
#pragma unroll
    for (int i = 0; i < N; ++i) dq[base + i * N + j] = col[i];
  }
  MP_DERIV_DIRS
  for (int j = 0; j < N; ++j) {
    T col[N];
    mp_deriv_sweep<T, N, HAS_FTIP, false>(M, P, b, j, col);
    mp_poison_if(poison, col);
#pragma unroll
    for (int i = 0; i < N; ++i) dqd[base + i * N + j] = col[i];
  }
}

// forward dynamics: qdd (may be null), dqdd_dq, dqdd_dqd, Minv = dqdd_dtau (may be null).  qdd from the bias recursion, M by the
// composite-rigid-body pass and ONE Cholesky factorisation; then every column (n of dtau_dq, n of dtau_dqd, n unit vectors for
// M^-1) is solved with that factor.
template <int N, bool HAS_FTIP, typename MT>
MP_HD void mp_fd_deriv_row(const MT& M, const MpCall<double>& C, const double* q, const double* qd, const double* tau, double* qdd,
                           double* dq, double* dqd, double* Minv, long r) {
  using T = double;
  T a[N], b[N], t[N], acc[N];
#pragma unroll
  for (int k = 0; k < N; ++k) { a[k] = q[r * N + k]; b[k] = qd[r * N + k]; t[k] = tau[r * N + k]; }
  MpBad<T> bad;
  bad.add(a); bad.add(b); bad.add(t);
  const bool poison = bad.any();
  MpDerivPrimal<T, N> P;
  {
    T zero[N], bias[N];
#pragma unroll
    for (int k = 0; k < N; ++k) zero[k] = 0.0;
    mp_deriv_primal<T, N, HAS_FTIP>(M, C, a, b, zero, P, bias);   // (qdd = 0: the bias torques; P is rebuilt below)
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = t[k] - bias[k];
  }
  T L[N][N];
  mp_mass_matrix_crba<T, N>(M, P.js, L);
  mp_deriv_chol<T, N>(L);
  mp_deriv_chol_solve<T, N>(L, acc);
  {
    T tau2[N];
    mp_deriv_primal<T, N, HAS_FTIP>(M, C, a, b, acc, P, tau2);      // the primal at the forward-dynamics qdd
  }
  const long base = r * (long)(N * N);
  if (qdd) {
    T o[N];
#pragma unroll
    for (int k = 0; k < N; ++k) o[k] = acc[k];
    mp_poison_if(poison, o);
#pragma unroll
    for (int k = 0; k < N; ++k) qdd[r * N + k] = o[k];
  }
  MP_DERIV_DIRS
  for (int j = 0; j < N; ++j) {
    T col[N];
    mp_deriv_sweep<T, N, HAS_FTIP, true>(M, P, b, j, col);
    mp_deriv_chol_solve<T, N>(L, col);
#pragma unroll
    for (int i = 0; i < N; ++i) col[i] = -col[i];
    mp_poison_if(poison, col);
#pragma unroll
    for (int i = 0; i < N; ++i) dq[base + i * N + j] = col[i];
  }
  MP_DERIV_DIRS
  for (int j = 0; j < N; ++j) {
    T col[N];
    mp_deriv_sweep<T, N, HAS_FTIP, false>(M, P, b, j, col);
    mp_deriv_chol_solve<T, N>(L, col);
#pragma unroll
    for (int i = 0; i < N; ++i) col[i] = -col[i];
    mp_poison_if(poison, col);
#pragma unroll
    for (int i = 0; i < N; ++i) dqd[base + i * N + j] = col[i];
  }
  if (Minv) {
    MP_DERIV_DIRS
    for (int j = 0; j < N; ++j) {
      T col[N];
#pragma unroll
      for (int i = 0; i < N; ++i) col[i] = (i == j) ? 1.0 : 0.0;
      mp_deriv_chol_solve<T, N>(L, col);
      mp_poison_if(poison, col);
#pragma unroll
      for (int i = 0; i < N; ++i) Minv[base + i * N + j] = col[i];
    }
  }
}
