// Time-optimal path parameterisation under torque, acceleration and velocity limits (TOPP by reachability analysis), one grid row or
// one path per call (float64, 1..MP_MAX_DOF joints).  Header-only like mp_ilqr.h: the HIP kernels (mp_kernels.hip, k_path_coeffs /
// k_toppra_sweep / k_path_rows) and the CPU twins (mp_cpu.cpp) instantiate the same templates.
//
// Path grid s_i = i / (Nt - 1), D = 1 / (Nt - 1), rows i = 0..Nt-1 of q, q' = dq/ds, q'' = d2q/ds2.  With qd = q' sd, qdd = q' sdd + q'' sd^2
// the torque is affine in (u, x) = (sdd, sd^2):  tau = a u + b x + c,
//     a = M(q) q',   b = M(q) q'' + C(q, q') q',   c = g(q) + Js^T Ftip.
// mp_path_coeffs_row takes the three vectors from three recursions over the row's link frames that share its loads and its joint state
// (sin / cos are taken once): (velocity 0, acceleration q', no gravity), (velocity q', acceleration q'', no gravity), (everything 0, base
// acceleration -g, the wrench).  Nothing is a difference of inverse-dynamics results.  The recursions run one after another, not
// interleaved: one set's 6 n body wrenches are live at a time instead of 18 n (288 registers at n = 8).  The zero-velocity sets skip the
// velocity-product terms at compile time.  xbar = min_j (vmax_j / |q'_j|)^2 over the joints with q'_j != 0 (+inf when there is none).
//
// Constraints on (u, x) at row i, each lo <= p u + q x + r <= hi with an infinite side absent (it never enters the arithmetic):
//     torque  (a_j, b_j, c_j, tau_lo_j, tau_hi_j),   acceleration (q'_j, q''_j, 0, -amax_j, amax_j; optional),
//     transition  (2 D, 1, 0, K_{i+1,lo}, K_{i+1,hi}),   speed 0 <= x <= xbar_i.
// A row with p != 0 is one lower and one upper LINE u >= ls x + lc / u <= us x + uc; p = 0 bounds x directly (or, q = 0 too, decides
// emptiness).  For fixed x the feasible u is [alpha(x), beta(x)], alpha the largest lower line, beta the smallest upper line, and
// beta - alpha is concave and piecewise linear.  K_i = [min x, max x]: start at the end of [xlo, xhi], evaluate the two active lines, jump
// to their intersection, repeat - Newton on a concave function from outside the feasible interval, monotone, one piece a step.  It ends
// when beta >= alpha, when the active pair is the pair just intersected (the vertex itself, beta - alpha < 0 by rounding only), or with
// "empty" when the tangent does not lead back or leads past the end of [xlo, xhi] (each search is exact on its own).  The lines sit in
// registers and are scanned with compile-time indices: the active pair is carried by value, nothing is indexed at run time.
//
// Backward pass i = Nt-2 .. 0 from K_{Nt-1} = [sd_end^2, sd_end^2]; forward pass from x_0 = sd_start^2 with u_i = beta(x_i),
// x_{i+1} = clip(x_i + 2 D u_i, K_{i+1}), u_{Nt-1} = u_{Nt-2}; t_{i+1} = t_i + 2 D / (sqrt x_i + sqrt x_{i+1}) (+inf through a stop).
// status: 0 fine; i + 1: the set is first empty, going backward, at row i; -2: sd_end^2 > xbar_{Nt-1} (K all NaN) or sd_start^2 outside
// K_0 (K kept); -1: a non-finite coefficient, xbar (a row whose q' is all zero) or end speed.  Order: -1, the end speed, i + 1, the start
// speed.  status != 0: x, u, t, duration and the rows are NaN, K is NaN from the failing row down (all of it for -1 and the end speed).
//
// Every per-step load has an address known in advance: the next row's coefficients are requested before the current row is solved.
#pragma once

#include "mp_core.h"

struct MpToppraLimits {   // wave-uniform: travels as a kernel argument
  double tau_lo[MP_MAX_DOF], tau_hi[MP_MAX_DOF], amax[MP_MAX_DOF];
};
struct MpToppraVmax {
  double v[MP_MAX_DOF];
};

MP_HD bool mp_tp_finite(double v) { return (mp_hi_word(v) & 0x7ff00000) != 0x7ff00000; }
MP_HD double mp_tp_inf() { return __builtin_inf(); }
MP_HD double mp_tp_nan() { return __builtin_bit_cast(double, 0x7ff8000000000000ull); }

// mp_rnea_impl of mp_core.h with a compile-time "no velocity" form: VEL = false takes qd = 0 (w = v = 0, no momentum terms).  Same
// order of operations as mp_rnea_impl, so VEL = false gives what that recursion gives at qd = 0.
template <int N, bool VEL, bool HAS_FTIP, typename MT>
MP_HD void mp_tp_rnea(const MT& M, const double (&a0)[3], const double (&tipn)[3], const double (&tipf)[3], const MpJointState<double, N>& js,
                      const double (&qd)[N], const double (&qdd)[N], double (&tau)[N]) {
  using T = double;
  T fnx[N], fny[N], fnz[N], ffx[N], ffy[N], ffz[N];
  T wx = 0, wy = 0, wz = 0, vx = 0, vy = 0, vz = 0;
  T dwx = 0, dwy = 0, dwz = 0, dvx = a0[0], dvy = a0[1], dvz = a0[2];
  T tnx = 0, tny = 0, tnz = 0, tfx = 0, tfy = 0, tfz = 0;
  if (HAS_FTIP) { tnx = tipn[0]; tny = tipn[1]; tnz = tipn[2]; tfx = tipf[0]; tfy = tipf[1]; tfz = tipf[2]; }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const auto& J = mp_joint_of(M, i);
    if (i > 0) {
      if (VEL) mp_motion_A(J.ca, J.sa, J.a, wx, wy, wz, vx, vy, vz);
      mp_motion_A(J.ca, J.sa, J.a, dwx, dwy, dwz, dvx, dvy, dvz);
      if (HAS_FTIP) mp_force_down_A(J.ca, J.sa, J.a, tnx, tny, tnz, tfx, tfy, tfz);
    }
    const T c = js.c[i], s = js.s[i], d = js.d[i];
    if (VEL) mp_motion_B(c, s, d, wx, wy, wz, vx, vy, vz);
    mp_motion_B(c, s, d, dwx, dwy, dwz, dvx, dvy, dvz);
    if (HAS_FTIP) mp_force_down_B(c, s, d, tnx, tny, tnz, tfx, tfy, tfz);
    const T ar = J.rev * qdd[i], ap = qdd[i] - ar;
    if (VEL) {
      const T qdr = J.rev * qd[i], qdp = qd[i] - qdr;
      wz += qdr;
      vz += qdp;
      dwx += qdr * wy;
      dwy -= qdr * wx;
      dvx += qdr * vy + qdp * wy;
      dvy -= qdr * vx + qdp * wx;
    }
    dwz += ar;
    dvz += ap;
    fnx[i] = J.Ixx * dwx + J.Ixy * dwy + J.Ixz * dwz + (J.hy * dvz - J.hz * dvy);
    fny[i] = J.Ixy * dwx + J.Iyy * dwy + J.Iyz * dwz + (J.hz * dvx - J.hx * dvz);
    fnz[i] = J.Ixz * dwx + J.Iyz * dwy + J.Izz * dwz + (J.hx * dvy - J.hy * dvx);
    ffx[i] = J.m * dvx - (J.hy * dwz - J.hz * dwy);
    ffy[i] = J.m * dvy - (J.hz * dwx - J.hx * dwz);
    ffz[i] = J.m * dvz - (J.hx * dwy - J.hy * dwx);
    if (VEL) {
      const T pnx = J.Ixx * wx + J.Ixy * wy + J.Ixz * wz + (J.hy * vz - J.hz * vy);
      const T pny = J.Ixy * wx + J.Iyy * wy + J.Iyz * wz + (J.hz * vx - J.hx * vz);
      const T pnz = J.Ixz * wx + J.Iyz * wy + J.Izz * wz + (J.hx * vy - J.hy * vx);
      const T pfx = J.m * vx - (J.hy * wz - J.hz * wy);
      const T pfy = J.m * vy - (J.hz * wx - J.hx * wz);
      const T pfz = J.m * vz - (J.hx * wy - J.hy * wx);
      fnx[i] = fnx[i] + (wy * pnz - wz * pny) + (vy * pfz - vz * pfy);
      fny[i] = fny[i] + (wz * pnx - wx * pnz) + (vz * pfx - vx * pfz);
      fnz[i] = fnz[i] + (wx * pny - wy * pnx) + (vx * pfy - vy * pfx);
      ffx[i] = ffx[i] + (wy * pfz - wz * pfy);
      ffy[i] = ffy[i] + (wz * pfx - wx * pfz);
      ffz[i] = ffz[i] + (wx * pfy - wy * pfx);
    }
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
      mp_force_up_B(js.c[i], js.s[i], js.d[i], nx, ny, nz, fx, fy, fz);
      mp_force_up_A(J.ca, J.sa, J.a, nx, ny, nz, fx, fy, fz);
      fnx[i - 1] += nx; fny[i - 1] += ny; fnz[i - 1] += nz;
      ffx[i - 1] += fx; ffy[i - 1] += fy; ffz[i - 1] += fz;
    }
  }
}

// Row r of plain row-major arrays: a, b, c (n each) and xbar.  A non-finite input poisons the row's four outputs.
template <int N, bool HAS_FTIP, typename MT>
MP_HD void mp_path_coeffs_row(const MT& M, const MpCall<double>& C, const MpToppraVmax& V, const double* q, const double* dq,
                              const double* ddq, double* a, double* b, double* c, double* xbar, long r) {
  double p[N], p1[N], p2[N], zero[N];
#pragma unroll
  for (int k = 0; k < N; ++k) { p[k] = q[r * N + k]; p1[k] = dq[r * N + k]; p2[k] = ddq[r * N + k]; zero[k] = 0.0; }
  MpBad<double> bad;
  bad.add(p); bad.add(p1); bad.add(p2);
  const bool poison = bad.any();
  MpJointState<double, N> js;
  mp_joint_state<double, N>(M, p, js);
  const double z3[3] = {0.0, 0.0, 0.0};
  const double tn[3] = {C.F1n[0], C.F1n[1], C.F1n[2]}, tf[3] = {C.F1f[0], C.F1f[1], C.F1f[2]};
  double oa[N], ob[N], oc[N];
  mp_tp_rnea<N, false, false>(M, z3, z3, z3, js, zero, p1, oa);
  mp_tp_rnea<N, true, false>(M, z3, z3, z3, js, p1, p2, ob);
  mp_tp_rnea<N, false, HAS_FTIP>(M, C.a0, tn, tf, js, zero, zero, oc);
  double xb = mp_tp_inf();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double ratio = V.v[k] / mp_abs(p1[k]);
    if (p1[k] != 0.0) xb = mp_min(xb, ratio * ratio);
  }
  mp_poison_if(poison, oa);
  mp_poison_if(poison, ob);
  mp_poison_if(poison, oc);
  mp_poison_if(poison, xb);
#pragma unroll
  for (int k = 0; k < N; ++k) { a[r * N + k] = oa[k]; b[r * N + k] = ob[k]; c[r * N + k] = oc[k]; }
  xbar[r] = xb;
}

// Row r of the result: qd = q' sqrt x, qdd = q' u + q'' x, tau = a u + b x + c (x / u NaN on a failed path: NaN rows)
template <int N>
MP_HD void mp_path_rows_row(const double* a, const double* b, const double* c, const double* dq, const double* ddq, double x, double u,
                            double* oqd, double* oqdd, double* otau, long r) {
  const double sd = mp_sqrt(x);
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double d1 = dq[r * N + k], d2 = ddq[r * N + k];
    oqd[r * N + k] = d1 * sd;
    oqdd[r * N + k] = d1 * u + d2 * x;
    otau[r * N + k] = a[r * N + k] * u + b[r * N + k] * x + c[r * N + k];
  }
}

// ------------------------------------------------------------------------------------------------ the two-variable LP
template <int NL>
struct MpTpLines {
  double ls[NL], lc[NL], us[NL], uc[NL];   // u >= ls x + lc,  u <= us x + uc  (an absent line: slope 0, constant -+inf)
  double xlo, xhi;
  bool empty;
};

// lo <= p u + q x + r <= hi into one slot of the lines, or into [xlo, xhi] / `empty` when p = 0
MP_HD void mp_tp_pair(double p, double q, double r, double lo, double hi, double& ls, double& lc, double& us, double& uc, double& xlo,
                      double& xhi, bool& empty) {
  ls = 0.0; lc = -mp_tp_inf(); us = 0.0; uc = mp_tp_inf();
  const bool flo = mp_tp_finite(lo), fhi = mp_tp_finite(hi);
  if (p != 0.0) {
    const double s = -q / p, vlo = (lo - r) / p, vhi = (hi - r) / p;
    if (p > 0.0) {
      if (flo) { ls = s; lc = vlo; }
      if (fhi) { us = s; uc = vhi; }
    } else {
      if (fhi) { ls = s; lc = vhi; }
      if (flo) { us = s; uc = vlo; }
    }
  } else if (q != 0.0) {
    const double vlo = (lo - r) / q, vhi = (hi - r) / q;
    if (q > 0.0) {
      if (flo) xlo = mp_max(xlo, vlo);
      if (fhi) xhi = mp_min(xhi, vhi);
    } else {
      if (fhi) xlo = mp_max(xlo, vhi);
      if (flo) xhi = mp_min(xhi, vlo);
    }
  } else if ((flo && r < lo) || (fhi && r > hi)) {
    empty = true;
  }
}

template <int N, bool ACC>
struct MpTpCoef {
  double a[N], b[N], c[N], dq[ACC ? N : 1], ddq[ACC ? N : 1], xbar;
};

// Row i of one path: the coefficient arrays address the path's row 0, row i sits i * rs rows further (rs = B time-major, 1 batch-major)
template <int N, bool ACC>
MP_HD void mp_tp_load(const double* a, const double* b, const double* c, const double* xbar, const double* dq, const double* ddq, long rs,
                      long i, MpTpCoef<N, ACC>& o) {
  const long r = i * rs;
#pragma unroll
  for (int k = 0; k < N; ++k) { o.a[k] = a[r * N + k]; o.b[k] = b[r * N + k]; o.c[k] = c[r * N + k]; }
  if (ACC) {
#pragma unroll
    for (int k = 0; k < N; ++k) { o.dq[k] = dq[r * N + k]; o.ddq[k] = ddq[r * N + k]; }
  }
  o.xbar = xbar[r];
}
template <int N, bool ACC>
MP_HD void mp_tp_check(const MpTpCoef<N, ACC>& o, MpBad<double>& bad) {
  bad.add(o.a); bad.add(o.b); bad.add(o.c); bad.add(o.xbar);
  if (ACC) { bad.add(o.dq); bad.add(o.ddq); }
}

template <int N, bool ACC>
MP_HD void mp_tp_lines(const MpTpCoef<N, ACC>& co, const MpToppraLimits& lim, double klo, double khi, double two_d,
                       MpTpLines<(ACC ? 2 : 1) * N + 1>& L) {
  L.xlo = 0.0; L.xhi = co.xbar; L.empty = false;
#pragma unroll
  for (int j = 0; j < N; ++j)
    mp_tp_pair(co.a[j], co.b[j], co.c[j], lim.tau_lo[j], lim.tau_hi[j], L.ls[j], L.lc[j], L.us[j], L.uc[j], L.xlo, L.xhi, L.empty);
  if (ACC) {
#pragma unroll
    for (int j = 0; j < N; ++j)
      mp_tp_pair(co.dq[j], co.ddq[j], 0.0, -lim.amax[j], lim.amax[j], L.ls[N + j], L.lc[N + j], L.us[N + j], L.uc[N + j], L.xlo, L.xhi,
                 L.empty);
  }
  constexpr int T = (ACC ? 2 : 1) * N;
  mp_tp_pair(two_d, 1.0, 0.0, klo, khi, L.ls[T], L.lc[T], L.us[T], L.uc[T], L.xlo, L.xhi, L.empty);
}

// alpha(x) and beta(x) with their active lines, by value
template <int NL>
MP_HD void mp_tp_eval(const MpTpLines<NL>& L, double x, double& lv, double& ls, double& lc, double& uv, double& us, double& uc) {
  lv = -mp_tp_inf(); ls = 0.0; lc = -mp_tp_inf();
  uv = mp_tp_inf(); us = 0.0; uc = mp_tp_inf();
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    const double v = L.ls[k] * x + L.lc[k];
    if (v > lv) { lv = v; ls = L.ls[k]; lc = L.lc[k]; }
    const double w = L.us[k] * x + L.uc[k];
    if (w < uv) { uv = w; us = L.us[k]; uc = L.uc[k]; }
  }
}

// The largest (want_max) or smallest feasible x; false: the set is empty.  Exact on its own, whichever end is asked for: a step that
// would leave [xlo, xhi] is clamped to the end, and an end where beta - alpha is negative by more than rounding (64 ulp of the two
// values) means "empty"; so does a run that has not settled after one step per piece.
template <int NL>
MP_HD bool mp_tp_extreme(const MpTpLines<NL>& L, bool want_max, double& xout) {
  if (L.empty || !(L.xlo <= L.xhi)) return false;
  double x = want_max ? L.xhi : L.xlo;
  double pls = mp_tp_nan(), plc = pls, pus = pls, puc = pls;   // the pair intersected last (NaN: none, equal to nothing)
  bool settled = false;
  MP_ROLLED
  for (int it = 0; it < 2 * NL + 2; ++it) {
    double lv, ls, lc, uv, us, uc;
    mp_tp_eval<NL>(L, x, lv, ls, lc, uv, us, uc);
    const double gap = uv - lv;
    settled = true;
    if (gap >= 0.0) break;
    if (want_max ? !(x > L.xlo) : !(x < L.xhi)) {                  // at the far end of the interval: nowhere left to go
      if (gap >= -1.4210854715202004e-14 * (mp_abs(uv) + mp_abs(lv))) break;
      return false;
    }
    if (ls == pls && lc == plc && us == pus && uc == puc) break;   // at this pair's own intersection: negative by rounding only
    const double sg = us - ls;
    if (want_max ? !(sg < 0.0) : !(sg > 0.0)) return false;        // the tangent does not lead back
    const double xn = (lc - uc) / sg;
    if (want_max ? !(xn < x) : !(xn > x)) break;                   // no progress left in float64: x is the vertex
    x = want_max ? mp_max(xn, L.xlo) : mp_min(xn, L.xhi);
    pls = ls; plc = lc; pus = us; puc = uc;
    settled = false;
  }
  if (!settled) return false;
  xout = x;
  return true;
}

// ------------------------------------------------------------------------------------------------ one path
// a / b / c / dq / ddq address the path's row 0 (rows of n), xbar / x / u / t its element 0, K its pair 0; row i sits i * rs rows
// further.  dq / ddq are read when ACC or when the three row outputs are given (oqd / oqdd / otau: all or none; the fused epilogue).
template <int N, bool ACC>
MP_HD void mp_toppra_sweep(const MpToppraLimits& lim, const double* a, const double* b, const double* c, const double* xbar,
                           const double* dq, const double* ddq, long rs, long Nt, double sd_start, double sd_end, double* K, double* x,
                           double* u, double* t, double* dur, int* status, double* oqd, double* oqdd, double* otau) {
  constexpr int NL = (ACC ? 2 : 1) * N + 1;
  const double two_d = 2.0 / (double)(Nt - 1);
  const double x_start = sd_start * sd_start, x_end = sd_end * sd_end;
  const double nan = mp_tp_nan();
  MpBad<double> bad;
  bad.add(x_start); bad.add(x_end);
  MpTpCoef<N, ACC> cur, nxt;
  mp_tp_load<N, ACC>(a, b, c, xbar, dq, ddq, rs, Nt - 1, cur);
  mp_tp_load<N, ACC>(a, b, c, xbar, dq, ddq, rs, Nt - 2, nxt);
  mp_tp_check(cur, bad);
  const bool end_bad = !(x_end <= cur.xbar);
  double klo = x_end, khi = x_end;
  K[(Nt - 1) * rs * 2] = klo; K[(Nt - 1) * rs * 2 + 1] = khi;
  int st = 0;
  for (long i = Nt - 2; i >= 0; --i) {
    cur = nxt;
    if (i > 0) mp_tp_load<N, ACC>(a, b, c, xbar, dq, ddq, rs, i - 1, nxt);   // next row's loads go out before this row is solved
    mp_tp_check(cur, bad);
    if (st == 0 && !end_bad && !bad.any()) {
      MpTpLines<NL> L;
      mp_tp_lines<N, ACC>(cur, lim, klo, khi, two_d, L);
      double hi_, lo_;
      if (mp_tp_extreme<NL>(L, true, hi_) && mp_tp_extreme<NL>(L, false, lo_)) { klo = lo_; khi = hi_; }
      else st = (int)(i + 1);
    }
    K[i * rs * 2] = st ? nan : klo;
    K[i * rs * 2 + 1] = st ? nan : khi;
  }
  bool wipe = false;
  if (bad.any()) { st = -1; wipe = true; }
  else if (end_bad) { st = -2; wipe = true; }
  else if (st == 0 && !(klo <= x_start && x_start <= khi)) st = -2;
  *status = st;
  if (st != 0) {
    for (long i = 0; i < Nt; ++i) {
      if (wipe) { K[i * rs * 2] = nan; K[i * rs * 2 + 1] = nan; }
      x[i * rs] = nan; u[i * rs] = nan; t[i * rs] = nan;
      if (otau) {
#pragma unroll
        for (int k = 0; k < N; ++k) { oqd[i * rs * N + k] = nan; oqdd[i * rs * N + k] = nan; otau[i * rs * N + k] = nan; }
      }
    }
    *dur = nan;
    return;
  }
  // forward pass
  double xi = x_start, ti = 0.0, ui = 0.0;
  x[0] = xi; t[0] = 0.0;
  mp_tp_load<N, ACC>(a, b, c, xbar, dq, ddq, rs, 0, nxt);
  double nlo = K[rs * 2], nhi = K[rs * 2 + 1];
  for (long i = 0; i + 1 < Nt; ++i) {
    cur = nxt;
    klo = nlo; khi = nhi;
    if (i + 2 < Nt) {
      mp_tp_load<N, ACC>(a, b, c, xbar, dq, ddq, rs, i + 1, nxt);
      nlo = K[(i + 2) * rs * 2]; nhi = K[(i + 2) * rs * 2 + 1];
    }
    MpTpLines<NL> L;
    mp_tp_lines<N, ACC>(cur, lim, klo, khi, two_d, L);
    double lv, ls, lc, uv, us, uc;
    mp_tp_eval<NL>(L, xi, lv, ls, lc, uv, us, uc);
    ui = uv;
    const double xn = mp_min(mp_max(xi + two_d * ui, klo), khi);
    u[i * rs] = ui;
    if (otau) mp_path_rows_row<N>(a, b, c, dq, ddq, xi, ui, oqd, oqdd, otau, i * rs);
    ti += two_d / (mp_sqrt(xi) + mp_sqrt(xn));
    x[(i + 1) * rs] = xn; t[(i + 1) * rs] = ti;
    xi = xn;
  }
  u[(Nt - 1) * rs] = ui;
  if (otau) mp_path_rows_row<N>(a, b, c, dq, ddq, xi, ui, oqd, oqdd, otau, (Nt - 1) * rs);
  *dur = ti;
}
