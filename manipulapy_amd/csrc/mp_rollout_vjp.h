// Reverse mode (vector-Jacobian product) through the semi-implicit-Euler roll-out of forward_dynamics_trajectory, one
// trajectory per call (float64, 1..MP_MAX_DOF joints, unrolled).  Header-only like mp_deriv.h: the HIP kernel (mp_kernels.hip,
// k_fd_traj_vjp on the time-major layout) and the CPU twin (mp_cpu.cpp) instantiate the same template.
//
// Forward (mp_body_fd_traj_tm): step i >= 1 runs intRes sub-steps of h = dt / intRes with tau row i and Ftip row i:
//     a = FD(q, qd, tau_i, F_i),  v = qd + h a,  u = q + h v,  q' = clip(u, qmin, qmax),  qd' = v
// row i = (q, qd, a of the last sub-step), row 0 = (q0, qd0, 0).  Given the cotangents Gp, Gv, Ga of the three (N, n) row arrays
// (each may be null = zero), the adjoint walks the steps backwards with lq / lv the adjoints of the state after a sub-step:
//     end of step i:        lq += Gp[i],  lv += Gv[i]
//     sub-step, last first: m = [qmin <= u <= qmax] (inclusive, as torch.clamp's backward),  lu = m lq,  lvv = lv + h lu,
//                           la = h lvv (+ Ga[i] on the step's last sub-step),  mu = M(q)^-1 la,  gtau[i] += mu,
//                           lq = lu - (dtau_ID/dq)^T mu,  lv = lvv - (dtau_ID/dqd)^T mu      (at (q, qd, a), tip wrench included)
//     finally:              gtheta0 = lq + Gp[0],  gdtheta0 = lv + Gv[0],  gtau[0] = 0
// Component j of (dtau/dq)^T mu is mu . (tangent sweep j of mp_deriv_sweep): the (n, n) blocks are never formed.
//
// Memory: phase 1 re-runs the roll-out with the forward's own mp_forward_dynamics and clip (so the clip masks are the forward
// call's) and keeps the state at every row in `ck`; phase 2 walks the steps backwards, recomputes a step's sub-step states from
// the previous row into `sub` (intRes - 1 of them: the last sub-step starts from registers) and applies the adjoint above.
// A trajectory whose inputs or forward state hold a non-finite value gets NaN in every one of its gradients.
#pragma once

#include "mp_core.h"
#include "mp_deriv.h"

// Pointers address THIS trajectory's row 0; row i of an array of width W sits at base + i * rs * W (rs = B on the time-major
// device layout, 1 on batch-major host arrays), and the same for the workspace with its own row strides: `ck` holds the state
// (q, qd) of rows 0..Nt-1 at ck + i * cs * 2N, `sub` the sub-step states at sub + k * ss * 2N.  64-bit offsets throughout.
template <int N, bool HAS_FTIP, typename MT>
MP_HD void mp_fd_traj_vjp(const MT& M, const MpCall<double>& C, const double* th0, const double* dth0, const double* taumat,
                          const double* Fmat, long rs, long Nt, double h, int intRes, const double* Gp, const double* Gv,
                          const double* Ga, double* ck, long cs, double* sub, long ss, double* gth0, double* gdth0, double* gtau) {
  using T = double;
  const long rN = rs * N, r6 = rs * 6, c2 = cs * (2 * N), s2 = ss * (2 * N);
  T q[N], qd[N];
#pragma unroll
  for (int j = 0; j < N; ++j) { q[j] = th0[j]; qd[j] = dth0[j]; }
  MpBad<T> bad;
  bad.add(q); bad.add(qd);
  auto put = [&](double* p, const T (&a)[N], const T (&b)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) { p[j] = a[j]; p[N + j] = b[j]; }
  };
  auto get = [&](const double* p, T (&a)[N], T (&b)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) { a[j] = p[j]; b[j] = p[N + j]; }
  };
  // the inputs of step i: torques, and the step's wrench seen from frame 1
  auto inputs = [&](long i, T (&t)[N], T (&tn)[3], T (&tf)[3]) {
#pragma unroll
    for (int j = 0; j < N; ++j) t[j] = taumat[i * rN + j];
#pragma unroll
    for (int k = 0; k < 3; ++k) { tn[k] = T(0); tf[k] = T(0); }
    if (HAS_FTIP) {
      T F[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) F[k] = Fmat[i * r6 + k];
      bad.add(F);
      mp_wrench_to_frame1(M, F, tn, tf);
    }
  };
  // one forward sub-step, the arithmetic of mp_body_fd_traj_tm
  auto advance = [&](const T (&t)[N], const T (&tn)[3], const T (&tf)[3]) {
    T a[N];
    mp_forward_dynamics<T, N, HAS_FTIP>(M, C.a0, tn, tf, q, qd, t, a);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      qd[j] = qd[j] + a[j] * h;
      q[j] = mp_clip(q[j] + qd[j] * h, M.qmin[j], M.qmax[j]);
    }
  };

  // ---- phase 1: the roll-out, keeping the state of every row
  put(ck, q, qd);
  for (long i = 1; i < Nt; ++i) {
    T t[N], tn[3], tf[3];
    inputs(i, t, tn, tf);
    bad.add(t);
    for (int k = 0; k < intRes; ++k) advance(t, tn, tf);
    bad.add(q); bad.add(qd);
    put(ck + i * c2, q, qd);
  }
  const bool poison = bad.any();

  // ---- phase 2: the adjoint, steps and sub-steps last to first
  T lq[N], lv[N];
#pragma unroll
  for (int j = 0; j < N; ++j) { lq[j] = T(0); lv[j] = T(0); }
  for (long i = Nt - 1; i >= 1; --i) {
    if (Gp) {
#pragma unroll
      for (int j = 0; j < N; ++j) lq[j] += Gp[i * rN + j];
    }
    if (Gv) {
#pragma unroll
      for (int j = 0; j < N; ++j) lv[j] += Gv[i * rN + j];
    }
    T t[N], tn[3], tf[3];
    inputs(i, t, tn, tf);
    MpCall<T> Ci = C;  // the step's wrench where mp_deriv_primal reads it
    if (HAS_FTIP) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { Ci.F1n[k] = tn[k]; Ci.F1f[k] = tf[k]; }
    }
    // sub-step states: sub-step k starts from sub[k] (k < intRes - 1) or, for the last, from (q, qd) as left here
    get(ck + (i - 1) * c2, q, qd);
    for (int k = 0; k + 1 < intRes; ++k) {
      put(sub + k * s2, q, qd);
      advance(t, tn, tf);
    }
    T vn[N], gt[N];  // vn: the velocity after the sub-step being reversed (v = qd'); gt: this step's torque gradient
    {
      T qe[N];
      get(ck + i * c2, qe, vn);
    }
#pragma unroll
    for (int j = 0; j < N; ++j) gt[j] = T(0);
    for (int k = intRes - 1; k >= 0; --k) {
      if (k + 1 < intRes) get(sub + k * s2, q, qd);
      T lu[N], lvv[N], mu[N];
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const T u = q[j] + vn[j] * h;
        lu[j] = (u >= M.qmin[j] && u <= M.qmax[j]) ? lq[j] : T(0);
        lvv[j] = lv[j] + h * lu[j];
        mu[j] = h * lvv[j];
      }
      if (Ga && k == intRes - 1) {
#pragma unroll
        for (int j = 0; j < N; ++j) mu[j] += Ga[i * rN + j];
      }
      // the primal at (q, qd, a) and the Cholesky factor of M(q), as mp_fd_deriv_row builds them
      MpDerivPrimal<T, N> P;
      T L[N][N], acc[N];
      {
        T zero[N], bias[N];
#pragma unroll
        for (int j = 0; j < N; ++j) zero[j] = T(0);
        mp_deriv_primal<T, N, HAS_FTIP>(M, Ci, q, qd, zero, P, bias);
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = t[j] - bias[j];
      }
      mp_mass_matrix_crba<T, N>(M, P.js, L);
      mp_deriv_chol<T, N>(L);
      mp_deriv_chol_solve<T, N>(L, acc);
      {
        T tau2[N];
        mp_deriv_primal<T, N, HAS_FTIP>(M, Ci, q, qd, acc, P, tau2);
      }
      mp_deriv_chol_solve<T, N>(L, mu);
#pragma unroll
      for (int j = 0; j < N; ++j) gt[j] += mu[j];
      MP_DERIV_DIRS
      for (int j = 0; j < N; ++j) {
        T col[N];
        mp_deriv_sweep<T, N, HAS_FTIP, true>(M, P, qd, j, col);
        T s = T(0);
#pragma unroll
        for (int r = 0; r < N; ++r) s += mu[r] * col[r];
        lq[j] = lu[j] - s;
      }
      MP_DERIV_DIRS
      for (int j = 0; j < N; ++j) {
        T col[N];
        mp_deriv_sweep<T, N, HAS_FTIP, false>(M, P, qd, j, col);
        T s = T(0);
#pragma unroll
        for (int r = 0; r < N; ++r) s += mu[r] * col[r];
        lv[j] = lvv[j] - s;
      }
#pragma unroll
      for (int j = 0; j < N; ++j) vn[j] = qd[j];
    }
    mp_poison_if(poison, gt);
#pragma unroll
    for (int j = 0; j < N; ++j) gtau[i * rN + j] = gt[j];
  }
  if (Gp) {
#pragma unroll
    for (int j = 0; j < N; ++j) lq[j] += Gp[j];
  }
  if (Gv) {
#pragma unroll
    for (int j = 0; j < N; ++j) lv[j] += Gv[j];
  }
  T z[N];
#pragma unroll
  for (int j = 0; j < N; ++j) z[j] = T(0);
  mp_poison_if(poison, lq); mp_poison_if(poison, lv); mp_poison_if(poison, z);
#pragma unroll
  for (int j = 0; j < N; ++j) { gth0[j] = lq[j]; gdth0[j] = lv[j]; gtau[j] = z[j]; }
}
