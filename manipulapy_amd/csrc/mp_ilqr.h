// Batched iLQR about a semi-implicit-Euler roll-out: the Riccati backward pass and the closed-loop roll-out, one trajectory per call
// (float64, 1..MP_MAX_DOF joints, intRes = 1, no tip wrench).  Header-only like mp_rollout_vjp.h: the HIP kernels (mp_kernels.hip,
// k_ilqr_backward / k_ilqr_rollout on the time-major layout) and the CPU twins (mp_cpu.cpp) instantiate the same templates.
//
// Indexing is the roll-out's (mp_rollout_vjp.h): rows i = 0..Nt-1, row 0 the given state, torque row i >= 1 drives step i, h = dt:
//     a = FD(q_{i-1}, qd_{i-1}, u_i),  qd_i = qd_{i-1} + h a,  w = q_{i-1} + h qd_i,  q_i = clip(w),  m = [qmin <= w <= qmax]
// With x = (q, qd), Aq = da/dq, Av = da/dqd, Mi = M^-1 at (q_{i-1}, qd_{i-1}, u_i) the step's Jacobians are
//     A_i = [[m (1 + h^2 Aq), m h (1 + h Av)], [h Aq, 1 + h Av]],     B_i = [[m h^2 Mi], [h Mi]]        (m scales rows)
// and they are never formed: with z = h m w1 + w2 for w = (w1, w2)
//     A^T w = (m w1 + h Aq^T z,  z + h Av^T z),      B^T w = h Mi^T z
// so every product below is a handful of n x n block products.
//
// Cost, diagonal weights shared by the batch, e = x - xref:
//     J = 1/2 sum_{i=1}^{Nt-1} u_i^T wr u_i + 1/2 sum_{i=1}^{Nt-2} e_i^T wq e_i + 1/2 e_{Nt-1}^T wf e_{Nt-1}
// Backward pass, i = Nt-1 .. 1 from S = diag(wf), s = wf e_{Nt-1}:
//     Qx = A^T s, Qu = wr u_i + B^T s, Qxx = A^T S A, Qux = B^T S A, Quu = diag(wr) + B^T S B
//     K_i = -(Quu + reg 1)^-1 Qux,  k_i = -(Quu + reg 1)^-1 Qu   (Cholesky),   dV1 += k^T Qu,  dV2 += 1/2 k^T Quu k
//     s <- Qx + K^T (Quu k + Qu) + Qux^T k,   S <- Qxx + K^T (Quu K + Qux) + Qux^T K   (symmetric: upper triangle computed, mirrored)
//     if i - 1 >= 1:  s += wq e_{i-1},  S += diag(wq)
// status: 0 fine; i > 0: the factor of Quu + reg 1 met a pivot at or below MP_ILQR_PIVOT_EPS of its diagonal term first at step i
// (gains, k and dV of the trajectory are then zero); -1: a non-finite input (gains, k and dV are NaN).
//
// Two forms of the backward pass: mp_ilqr_backward below, one lane (or host thread) per trajectory - the CPU twin, and on the device
// the variant kept for comparison - and the cooperative form further down, 16 lanes a trajectory with the matrices in LDS, which is
// the kernel the device entry runs.
// Memory of the one-lane form: S (2n x 2n), P = A^T S, R = B^T S and Qux live in a caller-provided workspace of mp_ilqr_work_doubles(n) doubles per
// trajectory, element e at W[e * ws] (ws = B on the device: neighbouring lanes touch neighbouring doubles; 1 on the host); K_i is
// read back from the output array.  Every element of S is read once and written once a step.
#pragma once

#include "mp_core.h"
#include "mp_opspace.h"

#define MP_ILQR_PIVOT_EPS MP_OS_PIVOT_EPS   // 2^-46, the test mp_opspace.h applies to its pivots

MP_HD long mp_ilqr_work_doubles(int n) { return 12L * n * n; }

template <int N>
struct MpIlqrStep {
  double Aq[N][N], Av[N][N], Mi[N][N], m[N], h;
};

// out (2N) <- A^T w; z (N) <- h m w1 + w2, which B^T w = h Mi^T z reuses
template <int N, typename ST>
MP_HD void mp_ilqr_At(const ST& T, const double* w, double* out, double* z) {
#pragma unroll
  for (int j = 0; j < N; ++j) z[j] = T.h * T.m[j] * w[j] + w[N + j];
#pragma unroll
  for (int c = 0; c < N; ++c) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) { a += T.Aq[k][c] * z[k]; b += T.Av[k][c] * z[k]; }
    out[c] = T.m[c] * w[c] + T.h * a;
    out[N + c] = z[c] + T.h * b;
  }
}
template <int N, typename ST>
MP_HD void mp_ilqr_Bt(const ST& T, const double* z, double* out) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) a += T.Mi[k][j] * z[k];
    out[j] = T.h * a;
  }
}

// Pointers address THIS trajectory's row 0.  Row i of pos / vel / tau sits at base + i * rs * N, of xref at xref + i * xs * 2N, of
// K / k at K + i * ks * 2N N / k + i * ks * N; the derivative blocks of step i (row-major n x n, as mp_fd_deriv_row writes them) at
// dq / dqd / Minv + (i - 1) * bs * N N.  64-bit offsets throughout.
template <int N, typename MT>
MP_HD void mp_ilqr_backward(const MT& M, const double* pos, const double* vel, const double* tau, long rs, long Nt, double h,
                            const double* dq, const double* dqd, const double* Minv, long bs, const double* xref, long xs,
                            const double* wq, const double* wr, const double* wf, double reg, double* W, long ws, double* K, double* k,
                            long ks, double* dV, int* status) {
  constexpr int X = 2 * N;
  const long rN = rs * N, xX = xs * X, kK = ks * (X * N), kN = ks * N, bNN = bs * (N * N);
  double* const Sw = W;
  double* const Pw = W + (long)(X * X) * ws;
  double* const Rw = W + (long)(2 * X * X) * ws;
  double* const Qw = W + (long)(2 * X * X + N * X) * ws;
#define MP_ILQR_S(r, c) Sw[(long)((r) * X + (c)) * ws]
#define MP_ILQR_P(r, c) Pw[(long)((r) * X + (c)) * ws]
#define MP_ILQR_R(j, c) Rw[(long)((j) * X + (c)) * ws]
#define MP_ILQR_Q(j, c) Qw[(long)((j) * X + (c)) * ws]
  MpBad<double> bad;
  bad.add(reg);
  double s[X];
  auto error = [&](long i, double* e) {
    for (int j = 0; j < N; ++j) {
      const double p = pos[i * rN + j], v = vel[i * rN + j], a = xref[i * xX + j], b = xref[i * xX + N + j];
      bad.add(p); bad.add(v); bad.add(a); bad.add(b);
      e[j] = p - a;
      e[N + j] = v - b;
    }
  };
  {
    double e[X];
    error(Nt - 1, e);
    for (int r = 0; r < X; ++r) {
      s[r] = wf[r] * e[r];
      for (int c = 0; c < X; ++c) MP_ILQR_S(r, c) = r == c ? wf[r] : 0.0;
    }
  }
  for (int j = 0; j < N; ++j) { k[j] = 0.0; }
  for (int j = 0; j < X * N; ++j) K[j] = 0.0;
  double dv1 = 0.0, dv2 = 0.0;
  int fail = 0;
#pragma nounroll
  for (long i = Nt - 1; i >= 1; --i) {
    MpIlqrStep<N> T;
    T.h = h;
    double u[N];
    {
      const double *a = dq + (i - 1) * bNN, *b = dqd + (i - 1) * bNN, *c = Minv + (i - 1) * bNN;
      for (int r = 0; r < N; ++r)
        for (int j = 0; j < N; ++j) {
          T.Aq[r][j] = a[r * N + j]; T.Av[r][j] = b[r * N + j]; T.Mi[r][j] = c[r * N + j];
          bad.add(T.Aq[r][j]); bad.add(T.Av[r][j]); bad.add(T.Mi[r][j]);
        }
      for (int j = 0; j < N; ++j) {
        const double p = pos[(i - 1) * rN + j], v = vel[i * rN + j];
        bad.add(p); bad.add(v);
        const double w = p + v * h;
        T.m[j] = (w >= M.qmin[j] && w <= M.qmax[j]) ? 1.0 : 0.0;
        u[j] = tau[i * rN + j];
        bad.add(u[j]);
      }
    }
    double Qx[X], Qu[N], z[N], col[X], o[X];
    mp_ilqr_At<N>(T, s, Qx, z);
    mp_ilqr_Bt<N>(T, z, Qu);
    for (int j = 0; j < N; ++j) Qu[j] += wr[j] * u[j];
    // P = A^T S and R = B^T S, column by column (S is symmetric)
#pragma nounroll
    for (int c = 0; c < X; ++c) {
      for (int r = 0; r < X; ++r) col[r] = MP_ILQR_S(r, c);
      mp_ilqr_At<N>(T, col, o, z);
      for (int r = 0; r < X; ++r) MP_ILQR_P(r, c) = o[r];
      mp_ilqr_Bt<N>(T, z, o);
      for (int j = 0; j < N; ++j) MP_ILQR_R(j, c) = o[j];
    }
    // Qxx = P A: row r is (A^T P[r, :]^T)^T; it replaces S
#pragma nounroll
    for (int r = 0; r < X; ++r) {
      for (int c = 0; c < X; ++c) col[c] = MP_ILQR_P(r, c);
      mp_ilqr_At<N>(T, col, o, z);
      for (int c = 0; c < X; ++c) MP_ILQR_S(r, c) = o[c];
    }
    // Qux = R A and Quu = diag(wr) + R B, row by row
    double Quu[N][N];
#pragma nounroll
    for (int j = 0; j < N; ++j) {
      for (int c = 0; c < X; ++c) col[c] = MP_ILQR_R(j, c);
      mp_ilqr_At<N>(T, col, o, z);
      for (int c = 0; c < X; ++c) MP_ILQR_Q(j, c) = o[c];
      mp_ilqr_Bt<N>(T, z, o);
      for (int l = 0; l < N; ++l) Quu[j][l] = o[l] + (j == l ? wr[j] : 0.0);
    }
    double L[N][N], dg[N];
    for (int r = 0; r < N; ++r)
      for (int c = 0; c < N; ++c) L[r][c] = Quu[r][c] + (r == c ? reg : 0.0);
    const bool ok = mp_os_chol<N>(L, dg, MP_ILQR_PIVOT_EPS);
    if (!ok && fail == 0) fail = (int)i;
    double kk[N], g[N];
    for (int j = 0; j < N; ++j) kk[j] = Qu[j];
    mp_os_fwd<N>(L, kk);
    mp_os_back<N>(L, kk);
    for (int j = 0; j < N; ++j) { kk[j] = -kk[j]; k[i * kN + j] = kk[j]; }
    {
      double a = 0.0, b = 0.0;
      for (int j = 0; j < N; ++j) {
        double t = 0.0;
        for (int l = 0; l < N; ++l) t += Quu[j][l] * kk[l];
        g[j] = t + Qu[j];
        a += kk[j] * Qu[j];
        b += kk[j] * t;
      }
      dv1 += a;
      dv2 += 0.5 * b;
    }
    double* Ki = K + i * kK;
#pragma nounroll
    for (int c = 0; c < X; ++c) {
      double b[N];
      for (int j = 0; j < N; ++j) b[j] = MP_ILQR_Q(j, c);
      mp_os_fwd<N>(L, b);
      mp_os_back<N>(L, b);
      for (int j = 0; j < N; ++j) Ki[j * X + c] = -b[j];
    }
    // s <- Qx + K^T (Quu k + Qu) + Qux^T k;  S <- Qxx + K^T G + Qux^T K with G = Quu K + Qux, upper triangle and mirrored
#pragma nounroll
    for (int c = 0; c < X; ++c) {
      double Kc[N], Qc[N], Gc[N];
      for (int j = 0; j < N; ++j) { Kc[j] = Ki[j * X + c]; Qc[j] = MP_ILQR_Q(j, c); }
      double sc = Qx[c];
      for (int j = 0; j < N; ++j) {
        double t = Qc[j];
        for (int l = 0; l < N; ++l) t += Quu[j][l] * Kc[l];
        Gc[j] = t;
        sc += Kc[j] * g[j] + Qc[j] * kk[j];
      }
      s[c] = sc;
#pragma nounroll
      for (int r = 0; r <= c; ++r) {
        double v = r == c ? MP_ILQR_S(r, c) : 0.5 * (MP_ILQR_S(r, c) + MP_ILQR_S(c, r));
        for (int j = 0; j < N; ++j) v += Ki[j * X + r] * Gc[j] + MP_ILQR_Q(j, r) * Kc[j];
        MP_ILQR_S(r, c) = v;
        MP_ILQR_S(c, r) = v;
      }
    }
    if (i - 1 >= 1) {
      double e[X];
      error(i - 1, e);
      for (int r = 0; r < X; ++r) {
        s[r] += wq[r] * e[r];
        MP_ILQR_S(r, r) += wq[r];
      }
    }
  }
#undef MP_ILQR_S
#undef MP_ILQR_P
#undef MP_ILQR_R
#undef MP_ILQR_Q
  const bool poison = bad.any();
  if (poison || fail) {
    double f = 0.0;
    mp_poison_if(poison, f);
    for (long i = 1; i < Nt; ++i) {
      for (int j = 0; j < X * N; ++j) K[i * kK + j] = f;
      for (int j = 0; j < N; ++j) k[i * kN + j] = f;
    }
    dv1 = f;
    dv2 = f;
  }
  dV[0] = dv1;
  dV[1] = dv2;
  *status = poison ? -1 : fail;
}

// The closed-loop roll-out u_i = tau_i + alpha k_i + K_i (x_{i-1} - xbar_{i-1}) with the roll-out's own step arithmetic (`advance` of
// mp_rollout_vjp.h at intRes = 1) and the cost J above.  K and k may both be null (open loop; pos / vel are then not read).  opos /
// ovel / otau may be null (cost only); their row i sits at base + i * os * N, row 0 = (theta0, dtheta0, tau row 0).  A trajectory
// with a non-finite input or state gets a NaN cost and NaN rows.
template <int N, typename MT>
MP_HD void mp_ilqr_rollout(const MT& M, const MpCall<double>& C, const double* th0, const double* dth0, const double* tau,
                           const double* pos, const double* vel, long rs, const double* K, const double* k, long ks, double alpha,
                           const double* xref, long xs, const double* wq, const double* wr, const double* wf, long Nt, double h,
                           double* cost, double* opos, double* ovel, double* otau, long os) {
  using T = double;
  constexpr int X = 2 * N;
  const long rN = rs * N, xX = xs * X, kK = ks * (X * N), kN = ks * N, oN = os * N;
  T q[N], qd[N], tn[3] = {0.0, 0.0, 0.0}, tf[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < N; ++j) { q[j] = th0[j]; qd[j] = dth0[j]; }
  MpBad<T> bad;
  bad.add(q); bad.add(qd); bad.add(alpha);
  if (opos) {
#pragma unroll
    for (int j = 0; j < N; ++j) { opos[j] = q[j]; ovel[j] = qd[j]; otau[j] = tau[j]; }
  }
  T J = 0.0;
  for (long i = 1; i < Nt; ++i) {
    T u[N];
#pragma unroll
    for (int j = 0; j < N; ++j) u[j] = tau[i * rN + j];
    if (K) {
      T dx[X];
#pragma unroll
      for (int j = 0; j < N; ++j) {
        dx[j] = q[j] - pos[(i - 1) * rN + j];
        dx[N + j] = qd[j] - vel[(i - 1) * rN + j];
      }
      const double* Ki = K + i * kK;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        T v = u[j] + alpha * k[i * kN + j];
#pragma unroll
        for (int c = 0; c < X; ++c) v += Ki[j * X + c] * dx[c];
        u[j] = v;
      }
    }
    bad.add(u);
    T a[N];
    mp_forward_dynamics<T, N, false>(M, C.a0, tn, tf, q, qd, u, a);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      qd[j] = qd[j] + a[j] * h;
      q[j] = mp_clip(q[j] + qd[j] * h, M.qmin[j], M.qmax[j]);
    }
    bad.add(q); bad.add(qd);
    const double* w = i == Nt - 1 ? wf : wq;
    T ju = 0.0, je = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const T r0 = xref[i * xX + j], r1 = xref[i * xX + N + j];
      bad.add(r0); bad.add(r1);
      const T e0 = q[j] - r0, e1 = qd[j] - r1;
      ju += wr[j] * u[j] * u[j];
      je += w[j] * e0 * e0 + w[N + j] * e1 * e1;
    }
    J += 0.5 * ju + 0.5 * je;
    if (opos) {
#pragma unroll
      for (int j = 0; j < N; ++j) { opos[i * oN + j] = q[j]; ovel[i * oN + j] = qd[j]; otau[i * oN + j] = u[j]; }
    }
  }
  const bool poison = bad.any();
  mp_poison_if(poison, J);
  *cost = J;
  if (poison && opos) {
    T f = 0.0;
    mp_poison_if(true, f);
    for (long i = 0; i < Nt; ++i)
      for (int j = 0; j < N; ++j) { opos[i * oN + j] = f; ovel[i * oN + j] = f; otau[i * oN + j] = f; }
  }
}

// ---------------------------------------------------------------------------------------------------------------- cooperative form
// The same recursion with 16 lanes a trajectory: lane c owns column c of the state (2n <= 16; the lanes past 2n only help with loads),
// and S, R = B^T S (later G = Quu K + Qux), Qux, K, Quu and the step's three blocks live in memory the 16 lanes share (LDS on the
// device, 912 doubles at n = 8): no workspace in global memory, no scratch-sized private arrays.  The step is cut into six phases with
// a barrier after each; whatever crosses a barrier is in MpIlqrShared or in the lane's own MpIlqrLane.  Small things every lane needs
// (s, Qx, Qu, the factor of Quu, k, dV) are computed by every lane redundantly instead of being exchanged.  The S storage holds, in
// turn, S, P = A^T S (written by columns, read by rows), Qxx (written by rows) and the new S.  The entries of the new S are formed by
// the arithmetic of mp_ilqr_backward (upper triangle's formula on both sides), so the two forms agree to rounding.
// The phases are plain functions of (phase, lane): the kernel runs them with a barrier in between, the host runs each phase over the
// 16 lanes in turn (mp_ilqr_backward_coop_host) - the same code, which is how the cooperative form is tested without a GPU.
template <int N>
struct MpIlqrShared {
  double S[2 * N][2 * N], R[N][2 * N], Q[N][2 * N], K[N][2 * N], Quu[N][N], Aq[N][N], Av[N][N], Mi[N][N], s[2 * N];
  int bad;
};
template <int N>
struct MpIlqrLane {
  double s[2 * N], Qx[2 * N], a[2 * N], Qu[N], m[N], rc[N], Kc[N], Gc[N], dv1, dv2;
  int fail;
  MpBad<double> bad;
};
template <int N>
struct MpIlqrStepRef {
  const double (*Aq)[N];
  const double (*Av)[N];
  const double (*Mi)[N];
  double m[N];
  double h;
};
struct MpIlqrArgs {   // pointers address the trajectory's row 0, strides as mp_ilqr_backward
  const double *pos, *vel, *tau;
  long rs, Nt;
  double h;
  const double *dq, *dqd, *Minv;
  long bs;
  const double* xref;
  long xs;
  const double *wq, *wr, *wf;
  double reg;
  double *K, *k;
  long ks;
  double* dV;
  int* status;
  bool write;   // false: a lane group past the end of the batch, which computes along and stores nothing
};
enum { MP_ILQR_PH_INIT = -1, MP_ILQR_PH_FLAG = 6, MP_ILQR_PH_FINAL = 7, MP_ILQR_LANES = 16 };

template <int N, typename MT>
MP_HD void mp_ilqr_coop_phase(int ph, long i, const MT& M, const MpIlqrArgs& A, MpIlqrShared<N>& sh, MpIlqrLane<N>& L, int lane) {
  constexpr int X = 2 * N;
  const long rN = A.rs * N, xX = A.xs * X, kK = A.ks * (X * N), kN = A.ks * N, bNN = A.bs * (N * N);
  const bool col = lane < X;
  const int c = col ? lane : 0;
  MpIlqrStepRef<N> T;
  T.Aq = sh.Aq; T.Av = sh.Av; T.Mi = sh.Mi; T.h = A.h;
#pragma unroll
  for (int j = 0; j < N; ++j) T.m[j] = L.m[j];
  // e = x - xref of row r, every component, by this lane alone
  auto error = [&](long r, double* e) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const double p = A.pos[r * rN + j], v = A.vel[r * rN + j], a = A.xref[r * xX + j], b = A.xref[r * xX + N + j];
      L.bad.add(p); L.bad.add(v); L.bad.add(a); L.bad.add(b);
      e[j] = p - a;
      e[N + j] = v - b;
    }
  };
  switch (ph) {
    case MP_ILQR_PH_INIT: {
      L.bad = MpBad<double>();
      L.bad.add(A.reg);
      L.dv1 = 0.0; L.dv2 = 0.0; L.fail = 0;
      double e[X];
      error(A.Nt - 1, e);
#pragma unroll
      for (int r = 0; r < X; ++r) L.s[r] = A.wf[r] * e[r];
      if (col) {
#pragma unroll
        for (int r = 0; r < X; ++r) sh.S[r][c] = r == c ? A.wf[r] : 0.0;
      }
      if (lane == 0) sh.bad = 0;
      if (A.write) {
        for (int e0 = lane; e0 < X * N; e0 += MP_ILQR_LANES) A.K[e0] = 0.0;
        if (lane < N) A.k[lane] = 0.0;
      }
    } break;
    case 0: {   // the new S of the step before; this step's blocks
      if (i < A.Nt - 1 && col) {
#pragma unroll
        for (int r = 0; r < X; ++r) sh.S[r][c] = L.a[r] + (r == c ? A.wq[r] : 0.0);
      }
      const double *a = A.dq + (i - 1) * bNN, *b = A.dqd + (i - 1) * bNN, *d = A.Minv + (i - 1) * bNN;
      for (int e0 = lane; e0 < N * N; e0 += MP_ILQR_LANES) {
        const double x = a[e0], y = b[e0], w = d[e0];
        L.bad.add(x); L.bad.add(y); L.bad.add(w);
        (&sh.Aq[0][0])[e0] = x; (&sh.Av[0][0])[e0] = y; (&sh.Mi[0][0])[e0] = w;
      }
    } break;
    case 1: {   // mask, Qx, Qu; column c of P = A^T S and of R = B^T S
      double u[N], z[N];
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const double p = A.pos[(i - 1) * rN + j], v = A.vel[i * rN + j];
        L.bad.add(p); L.bad.add(v);
        const double w = p + v * A.h;
        L.m[j] = (w >= M.qmin[j] && w <= M.qmax[j]) ? 1.0 : 0.0;
        T.m[j] = L.m[j];
        u[j] = A.tau[i * rN + j];
        L.bad.add(u[j]);
      }
      mp_ilqr_At<N>(T, L.s, L.Qx, z);
      mp_ilqr_Bt<N>(T, z, L.Qu);
#pragma unroll
      for (int j = 0; j < N; ++j) L.Qu[j] += A.wr[j] * u[j];
      if (col) {
        double sc[X];
#pragma unroll
        for (int r = 0; r < X; ++r) sc[r] = sh.S[r][c];
        mp_ilqr_At<N>(T, sc, L.a, z);
        mp_ilqr_Bt<N>(T, z, L.rc);
      }
    } break;
    case 2: {
      if (col) {
#pragma unroll
        for (int r = 0; r < X; ++r) sh.S[r][c] = L.a[r];
#pragma unroll
        for (int j = 0; j < N; ++j) sh.R[j][c] = L.rc[j];
      }
    } break;
    case 3: {   // row c of Qxx = P A; lanes j < N: row j of Qux = R A and of Quu = diag(wr) + R B
      double z[N], row[X], o[X];
      if (col) {
#pragma unroll
        for (int k = 0; k < X; ++k) row[k] = sh.S[c][k];
        mp_ilqr_At<N>(T, row, L.a, z);
      }
      if (lane < N) {
#pragma unroll
        for (int k = 0; k < X; ++k) row[k] = sh.R[lane][k];
        mp_ilqr_At<N>(T, row, o, z);
#pragma unroll
        for (int k = 0; k < X; ++k) sh.Q[lane][k] = o[k];
        mp_ilqr_Bt<N>(T, z, o);
#pragma unroll
        for (int l = 0; l < N; ++l) sh.Quu[lane][l] = o[l] + (lane == l ? A.wr[l] : 0.0);
      }
    } break;
    case 4: {   // Qxx into S by rows; the factor of Quu + reg 1, k and dV by every lane; column c of K, of G and entry c of the new s
      if (col) {
#pragma unroll
        for (int k = 0; k < X; ++k) sh.S[c][k] = L.a[k];
      }
      double Quu[N][N], Lm[N][N], dg[N], kk[N], g[N];
#pragma unroll
      for (int r = 0; r < N; ++r) {
#pragma unroll
        for (int l = 0; l < N; ++l) { Quu[r][l] = sh.Quu[r][l]; Lm[r][l] = Quu[r][l] + (r == l ? A.reg : 0.0); }
      }
      const bool ok = mp_os_chol<N>(Lm, dg, MP_ILQR_PIVOT_EPS);
      if (!ok && L.fail == 0) L.fail = (int)i;
#pragma unroll
      for (int j = 0; j < N; ++j) kk[j] = L.Qu[j];
      mp_os_fwd<N>(Lm, kk);
      mp_os_back<N>(Lm, kk);
#pragma unroll
      for (int j = 0; j < N; ++j) kk[j] = -kk[j];
      {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          double t = 0.0;
#pragma unroll
          for (int l = 0; l < N; ++l) t += Quu[j][l] * kk[l];
          g[j] = t + L.Qu[j];
          a += kk[j] * L.Qu[j];
          b += kk[j] * t;
        }
        L.dv1 += a;
        L.dv2 += 0.5 * b;
      }
      if (A.write && lane < N) {
        double kl = kk[0];   // (selected, not indexed: the array stays in registers)
#pragma unroll
        for (int j = 1; j < N; ++j) kl = lane == j ? kk[j] : kl;
        A.k[i * kN + lane] = kl;
      }
      if (col) {
        double b[N], Qc[N];
#pragma unroll
        for (int j = 0; j < N; ++j) { Qc[j] = sh.Q[j][c]; b[j] = Qc[j]; }
        mp_os_fwd<N>(Lm, b);
        mp_os_back<N>(Lm, b);
        double sc = L.Qx[0];
#pragma unroll
        for (int r = 1; r < X; ++r) sc = c == r ? L.Qx[r] : sc;
#pragma unroll
        for (int j = 0; j < N; ++j) L.Kc[j] = -b[j];
#pragma unroll
        for (int j = 0; j < N; ++j) {
          double t = Qc[j];
#pragma unroll
          for (int l = 0; l < N; ++l) t += Quu[j][l] * L.Kc[l];
          L.Gc[j] = t;
          sc += L.Kc[j] * g[j] + Qc[j] * kk[j];
          sh.K[j][c] = L.Kc[j];
          sh.R[j][c] = t;
          if (A.write) A.K[i * kK + j * X + c] = L.Kc[j];
        }
        sh.s[c] = sc;
      }
    } break;
    case 5: {   // column c of the new S (kept in the lane until phase 0 of the next step); the new s
      if (col) {
        double nc[X];
#pragma unroll
        for (int r = 0; r < X; ++r) {
          double v = r == c ? sh.S[r][c] : (r < c ? 0.5 * (sh.S[r][c] + sh.S[c][r]) : 0.5 * (sh.S[c][r] + sh.S[r][c]));
          if (r <= c) {
#pragma unroll
            for (int j = 0; j < N; ++j) v += sh.K[j][r] * L.Gc[j] + sh.Q[j][r] * L.Kc[j];
          } else {
#pragma unroll
            for (int j = 0; j < N; ++j) v += L.Kc[j] * sh.R[j][r] + sh.Q[j][c] * sh.K[j][r];
          }
          nc[r] = v;
        }
#pragma unroll
        for (int r = 0; r < X; ++r) L.a[r] = nc[r];
      }
#pragma unroll
      for (int r = 0; r < X; ++r) L.s[r] = sh.s[r];
      if (i - 1 >= 1) {
        double e[X];
        error(i - 1, e);
#pragma unroll
        for (int r = 0; r < X; ++r) L.s[r] += A.wq[r] * e[r];
      }
    } break;
    case MP_ILQR_PH_FLAG: {
      if (L.bad.any()) sh.bad = 1;
    } break;
    default: {   // MP_ILQR_PH_FINAL
      const bool poison = sh.bad != 0;
      double dv1 = L.dv1, dv2 = L.dv2;
      if (poison || L.fail) {
        double f = 0.0;
        mp_poison_if(poison, f);
        if (A.write) {
          for (long r = 1; r < A.Nt; ++r) {
            for (int e0 = lane; e0 < X * N; e0 += MP_ILQR_LANES) A.K[r * kK + e0] = f;
            if (lane < N) A.k[r * kN + lane] = f;
          }
        }
        dv1 = f; dv2 = f;
      }
      if (A.write && lane == 0) {
        A.dV[0] = dv1;
        A.dV[1] = dv2;
        *A.status = poison ? -1 : L.fail;
      }
    } break;
  }
}

// The cooperative form on the host: every phase over the 16 lanes in turn
template <int N, typename MT>
inline void mp_ilqr_backward_coop_host(const MT& M, const MpIlqrArgs& A) {
  MpIlqrShared<N> sh;
  MpIlqrLane<N> L[MP_ILQR_LANES];
  auto all = [&](int ph, long i) {
    for (int lane = 0; lane < MP_ILQR_LANES; ++lane) mp_ilqr_coop_phase<N>(ph, i, M, A, sh, L[lane], lane);
  };
  all(MP_ILQR_PH_INIT, 0);
  for (long i = A.Nt - 1; i >= 1; --i)
    for (int ph = 0; ph < 6; ++ph) all(ph, i);
  all(MP_ILQR_PH_FLAG, 0);
  all(MP_ILQR_PH_FINAL, 0);
}
