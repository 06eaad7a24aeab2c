// Vector-Jacobian products of inverse and forward dynamics by reverse mode, one row per call (float64, 1..MP_MAX_DOF joints,
// unrolled).  Header-only like mp_deriv.h: the HIP kernels (mp_kernels.hip) and the CPU twins (mp_cpu.cpp) instantiate the same
// templates.
//
//   inverse dynamics   tau = ID(q, qd, qdd, g, Ftip), cotangent lam = g_tau  ->  g_q = (dtau/dq)^T lam, g_qd = (dtau/dqd)^T lam,
//                                                                                g_qdd = M lam
//   forward dynamics   qdd = FD(q, qd, tau, g, Ftip), cotangent lam = g_qdd  ->  mu = M^-1 lam, g_tau = mu, and (g_q, g_qd) of the
//                                                                                inverse dynamics at (q, qd, qdd) with cotangent -mu
// Derivatives are those of the UNCLIPPED tau, as in mp_deriv.h; the tip wrench's dependence on q is included.
//
// Method: the adjoint of mp_deriv_primal (V_i, A_i forward; f_i = I A_i + V_i x* I V_i; F_i = f_i + X_{i+1}^T F_{i+1};
// tau_i = S_i^T F_i).  With L = lam . tau the adjoint of F_i is F'_i = X_i F'_{i-1} + S_i lam_i, a motion vector carried out
// along the chain by the same motion steps as the twist (pass 1, it needs only q and lam).  Pass 2 walks back from the tip:
//   A'_i = I_i F'_i + X_{i+1}^T A'_{i+1}                                    g_qdd_i = S_i^T A'_i
//   V'_i = (the local term of the bias wrench) + s_i x* A'_i + X_{i+1}^T V'_{i+1},  s_i = S_i qd_i
//                                                                           g_qd_i = S_i^T V'_i + A'_i . (V_i x S_i)
//   g_q_i = the 90-degree rotations of mp_deriv_dstep_down / _up at the stepped x / y parts MpDerivPrimal keeps (twist,
//           acceleration, tip wrench, transmitted wrench), contracted with V'_i, A'_i, the tip wrench's adjoint and A_i F'_{i-1}
//           instead of propagated as tangents.
// A' and V' ride down the chain as force vectors (mp_force_up_*).  F' is NOT stashed: pass 2 recovers F'_{i-1} from F'_i by the
// inverse motion step (X^-1 of a motion vector is the force-up step with the (n, f) slots holding (v, w)), and A_i F'_{i-1} is that
// step's half-way value.  The tip wrench's adjoint starts at F'_{N-1} and goes down the same way.  Two link steps per link in pass 1,
// about ten in pass 2, on top of one primal pass: O(n) per row, against the O(n^2) tangent sweeps of mp_deriv.h.
#pragma once

#include "mp_deriv.h"

// I v for a link's spatial inertia and a motion vector v = (w, v):  (Irot w + h x v, m v - h x w)
template <typename T, typename JT>
MP_HD void mp_adj_inertia(const JT& J, T wx, T wy, T wz, T vx, T vy, T vz, T& nx, T& ny, T& nz, T& fx, T& fy, T& fz) {
  nx = J.Ixx * wx + J.Ixy * wy + J.Ixz * wz + (J.hy * vz - J.hz * vy);
  ny = J.Ixy * wx + J.Iyy * wy + J.Iyz * wz + (J.hz * vx - J.hx * vz);
  nz = J.Ixz * wx + J.Iyz * wy + J.Izz * wz + (J.hx * vy - J.hy * vx);
  fx = J.m * vx - (J.hy * wz - J.hz * wy);
  fy = J.m * vy - (J.hz * wx - J.hx * wz);
  fz = J.m * vz - (J.hx * wy - J.hy * wx);
}

// The reverse pass of the inverse dynamics at (q, qd, qdd) for the cotangent lam: g_q, g_qd, g_qdd (= M lam).  tau is the primal
// torque (unclipped).
template <typename T, int N, bool HAS_FTIP, typename MT>
MP_HD void mp_id_adjoint(const MT& M, const MpCall<T>& C, const T (&q)[N], const T (&qd)[N], const T (&qdd)[N], const T (&lam)[N],
                         T (&tau)[N], T (&gq)[N], T (&gqd)[N], T (&gqdd)[N]) {
  MpDerivPrimal<T, N> P;
  mp_deriv_primal<T, N, HAS_FTIP>(M, C, q, qd, qdd, P, tau);
  // pass 1: F'_{N-1} (w part fa pairs with moments, v part fb with forces)
  T fax = 0, fay = 0, faz = 0, fbx = 0, fby = 0, fbz = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const auto& J = mp_joint_of(M, i);
    if (i > 0) mp_motion_A(J.ca, J.sa, J.a, fax, fay, faz, fbx, fby, fbz);
    mp_motion_B(P.js.c[i], P.js.s[i], P.js.d[i], fax, fay, faz, fbx, fby, fbz);
    faz += J.rev * lam[i];
    fbz += (1.0 - J.rev) * lam[i];
  }
  // pass 2
  T anx = 0, any = 0, anz = 0, afx = 0, afy = 0, afz = 0;   // A' (force vector: n pairs with the angular part)
  T vnx = 0, vny = 0, vnz = 0, vfx = 0, vfy = 0, vfz = 0;   // V'
  T tax = fax, tay = fay, taz = faz, tbx = fbx, tby = fby, tbz = fbz;   // adjoint of the tip wrench (HAS_FTIP only)
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    const auto& J = mp_joint_of(M, i);
    const T Wx = P.wx[i], Wy = P.wy[i], Wz = P.wz[i], Vx = P.vx[i], Vy = P.vy[i], Vz = P.vz[i];
    // A'_i += I F'_i
    {
      T nx, ny, nz, fx, fy, fz;
      mp_adj_inertia(J, fax, fay, faz, fbx, fby, fbz, nx, ny, nz, fx, fy, fz);
      anx += nx; any += ny; anz += nz; afx += fx; afy += fy; afz += fz;
    }
    gqdd[i] = J.rev * anz + (1.0 - J.rev) * afz;
    // V'_i += the bias wrench's term:  f = ... + W x pn + V x pf | W x pf,  (pn, pf) = I V
    {
      T pnx, pny, pnz, pfx, pfy, pfz;
      mp_adj_inertia(J, Wx, Wy, Wz, Vx, Vy, Vz, pnx, pny, pnz, pfx, pfy, pfz);
      // adjoints of pn (= fa x W) and of pf (= fa x V + fb x W), taken back through I
      const T bnx = fay * Wz - faz * Wy, bny = faz * Wx - fax * Wz, bnz = fax * Wy - fay * Wx;
      const T bfx = (fay * Vz - faz * Vy) + (fby * Wz - fbz * Wy);
      const T bfy = (faz * Vx - fax * Vz) + (fbz * Wx - fbx * Wz);
      const T bfz = (fax * Vy - fay * Vx) + (fbx * Wy - fby * Wx);
      T inx, iny, inz, ifx, ify, ifz;
      mp_adj_inertia(J, bnx, bny, bnz, bfx, bfy, bfz, inx, iny, inz, ifx, ify, ifz);
      vnx += (pny * faz - pnz * fay) + (pfy * fbz - pfz * fby) + inx;
      vny += (pnz * fax - pnx * faz) + (pfz * fbx - pfx * fbz) + iny;
      vnz += (pnx * fay - pny * fax) + (pfx * fby - pfy * fbx) + inz;
      vfx += (pfy * faz - pfz * fay) + ifx;
      vfy += (pfz * fax - pfx * faz) + ify;
      vfz += (pfx * fay - pfy * fax) + ifz;
    }
    // the joint's rate term of the acceleration, a += V x s:  its V part and its explicit qd part
    const T qdr = J.rev * qd[i], qdp = qd[i] - qdr;
    vnx -= qdr * any + qdp * afy;
    vny += qdr * anx + qdp * afx;
    vfx -= qdr * afy;
    vfy += qdr * afx;
    gqd[i] = J.rev * vnz + (1.0 - J.rev) * vfz + J.rev * (anx * Wy - any * Wx + afx * Vy - afy * Vx) +
             (1.0 - J.rev) * (afx * Wy - afy * Wx);
    // q_i moves the joint's own step of the twist, the acceleration and the tip wrench on the way out ...
    T g;
    {
      T dwx, dwy, dvx, dvy;
      mp_deriv_dstep_down(J.rev, Wx, Wy, Vx, Vy, dwx, dwy, dvx, dvy);
      g = vnx * dwx + vny * dwy + vfx * dvx + vfy * dvy;
      mp_deriv_dstep_down(J.rev, P.awx[i], P.awy[i], P.avx[i], P.avy[i], dwx, dwy, dvx, dvy);
      g += anx * dwx + any * dwy + afx * dvx + afy * dvy;
      if (HAS_FTIP) {
        T dfx, dfy, dnx, dny;
        mp_deriv_dstep_down(J.rev, P.tfx[i], P.tfy[i], P.tnx[i], P.tny[i], dfx, dfy, dnx, dny);
        g += tax * dnx + tay * dny + tbx * dfx + tby * dfy;
      }
    }
    if (i > 0) {
      const T c = P.js.c[i], s = P.js.s[i], d = P.js.d[i];
      // ... and the up step of the wrench joint i transmits: paired with A_i F'_{i-1} = B_i^-1 (F'_i - S_i lam_i)
      faz -= J.rev * lam[i];
      fbz -= (1.0 - J.rev) * lam[i];
      mp_force_up_B(c, s, d, fbx, fby, fbz, fax, fay, faz);
      T dnx, dny, dfx, dfy;
      mp_deriv_dstep_up(J.rev, P.unx[i], P.uny[i], P.ufx[i], P.ufy[i], dnx, dny, dfx, dfy);
      g += fax * dnx + fay * dny + fbx * dfx + fby * dfy;
      mp_force_up_A(J.ca, J.sa, J.a, fbx, fby, fbz, fax, fay, faz);
      // A', V' (force vectors) and the tip wrench's adjoint (a motion vector) to link i - 1
      mp_force_up_B(c, s, d, anx, any, anz, afx, afy, afz);
      mp_force_up_A(J.ca, J.sa, J.a, anx, any, anz, afx, afy, afz);
      mp_force_up_B(c, s, d, vnx, vny, vnz, vfx, vfy, vfz);
      mp_force_up_A(J.ca, J.sa, J.a, vnx, vny, vnz, vfx, vfy, vfz);
      if (HAS_FTIP) {
        mp_force_up_B(c, s, d, tbx, tby, tbz, tax, tay, taz);
        mp_force_up_A(J.ca, J.sa, J.a, tbx, tby, tbz, tax, tay, taz);
      }
    }
    gq[i] = g;
  }
}

// ------------------------------------------------------------------------------------------- rows
// Row `r` of (rows, n) arrays; 64-bit offsets.  A row with a non-finite input or cotangent gets NaN in every output of that row only.

// inverse dynamics: gq, gqd, gqdd (may be null) for the cotangent gtau
template <int N, bool HAS_FTIP, typename MT>
MP_HD void mp_id_vjp_row(const MT& M, const MpCall<double>& C, const double* q, const double* qd, const double* qdd, const double* gtau,
                         double* gq, double* gqd, double* gqdd, long r) {
  using T = double;
  T a[N], b[N], c[N], l[N];
#pragma unroll
  for (int k = 0; k < N; ++k) { a[k] = q[r * N + k]; b[k] = qd[r * N + k]; c[k] = qdd[r * N + k]; l[k] = gtau[r * N + k]; }
  MpBad<T> bad;
  bad.add(a); bad.add(b); bad.add(c); bad.add(l);
  const bool poison = bad.any();
  T tau[N], o1[N], o2[N], o3[N];
  mp_id_adjoint<T, N, HAS_FTIP>(M, C, a, b, c, l, tau, o1, o2, o3);
  mp_poison_if(poison, o1);
  mp_poison_if(poison, o2);
#pragma unroll
  for (int k = 0; k < N; ++k) { gq[r * N + k] = o1[k]; gqd[r * N + k] = o2[k]; }
  if (gqdd) {
    mp_poison_if(poison, o3);
#pragma unroll
    for (int k = 0; k < N; ++k) gqdd[r * N + k] = o3[k];
  }
}

// forward dynamics: qdd (may be null), gq, gqd, gtau (may be null) for the cotangent gqdd.  qdd from the bias recursion, M by the
// composite-rigid-body pass and one Cholesky factorisation (as mp_fd_deriv_row), mu = M^-1 gqdd with that factor.
template <int N, bool HAS_FTIP, typename MT>
MP_HD void mp_fd_vjp_row(const MT& M, const MpCall<double>& C, const double* q, const double* qd, const double* tau, const double* gqdd,
                         double* qdd, double* gq, double* gqd, double* gtau, long r) {
  using T = double;
  T a[N], b[N], t[N], mu[N], acc[N];
#pragma unroll
  for (int k = 0; k < N; ++k) { a[k] = q[r * N + k]; b[k] = qd[r * N + k]; t[k] = tau[r * N + k]; mu[k] = gqdd[r * N + k]; }
  MpBad<T> bad;
  bad.add(a); bad.add(b); bad.add(t); bad.add(mu);
  const bool poison = bad.any();
  T L[N][N];
  {
    MpDerivPrimal<T, N> P;
    T zero[N], bias[N];
#pragma unroll
    for (int k = 0; k < N; ++k) zero[k] = 0.0;
    mp_deriv_primal<T, N, HAS_FTIP>(M, C, a, b, zero, P, bias);   // (qdd = 0: the bias torques)
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = t[k] - bias[k];
    mp_mass_matrix_crba<T, N>(M, P.js, L);
  }
  mp_deriv_chol<T, N>(L);
  mp_deriv_chol_solve<T, N>(L, acc);
  mp_deriv_chol_solve<T, N>(L, mu);
  T nmu[N], tau2[N], o1[N], o2[N], o3[N];
#pragma unroll
  for (int k = 0; k < N; ++k) nmu[k] = -mu[k];
  mp_id_adjoint<T, N, HAS_FTIP>(M, C, a, b, acc, nmu, tau2, o1, o2, o3);
  mp_poison_if(poison, o1);
  mp_poison_if(poison, o2);
#pragma unroll
  for (int k = 0; k < N; ++k) { gq[r * N + k] = o1[k]; gqd[r * N + k] = o2[k]; }
  if (qdd) {
    mp_poison_if(poison, acc);
#pragma unroll
    for (int k = 0; k < N; ++k) qdd[r * N + k] = acc[k];
  }
  if (gtau) {
    mp_poison_if(poison, mu);
#pragma unroll
    for (int k = 0; k < N; ++k) gtau[r * N + k] = mu[k];
  }
}
