// Fixed-rate sampling of time-optimal trajectories, one (path, sample) row per call (float64, 1..MP_MAX_DOF joints).  Header-only like
// mp_blend.h: the HIP kernel k_traj_sample (mp_kernels.hip) and the CPU twin (mp_cpu.cpp) instantiate the same templates.  The contract
// - screen, k_end, the hold row, the moving row, the two sources of the geometry, the outputs - is stated once, in
// include/manipula_hip.h (mp_trajectory_sample_*); this is how it is computed.
//
// A path's verdict is an OR of per-element flags over its tables (mp_ts_scan: any order gives the same bits, so the kernel's 64 lanes
// share the scan of a path and the twin walks it alone), then mp_ts_head turns the flags and the duration into status, count and
// needed.  mp_ts_row is one row: the search of the time stamps, the constant-acceleration step inside the interval, the geometry at
// the s it lands on (the quintic Hermite interpolant of the grid, or the blended curve itself through mp_blend_sample_at) and, when
// TAU, one Newton-Euler recursion at the row's own (q, qd, qdd).  Everything sits in registers under compile-time indices; the
// tables are read from memory at run-time indices.  Sums of two products are written through mp_two_products
// (mp_blend.h): which of the two the compiler would fuse depends on the code around them, and the kernel's variants with and without
// the torques must give the same s, q, qd, qdd bit for bit.
#pragma once

#include "mp_blend.h"
#include "mp_toppra.h"

constexpr int MP_TS_OK = 0, MP_TS_TRUNCATED = 1, MP_TS_STOPS = 2, MP_TS_UNTIMED = 3, MP_TS_INVALID = -1;  // = MP_SAMPLE_*
constexpr int MP_TS_GRID = 0, MP_TS_CURVE = 1;                                                             // the source
constexpr int MP_TS_NO_TAU = 0, MP_TS_TAU = 1, MP_TS_TAU_FTIP = 2;                                         // the torque variant
constexpr int MP_TS_F_NAN = 1, MP_TS_F_STOP = 2, MP_TS_F_BAD = 4;                                          // the scan's flags
constexpr double MP_TS_MAX_RATIO = 2147483646.0;  // T / dt below this: needed = k_end + 1 fits an int32

struct MpSampleIn {          // wave-uniform: travels as a kernel argument
  const double *t, *x;       // (B, grid)
  const double *q, *dq, *ddq;                   // grid source: (B, grid, n)
  const int *bstatus, *bcount;                  // curve source: the tables of the blend
  const double *points, *cut, *knot, *length;
  double dt;
  long B;
  int M, grid, w_in, pad;
};
struct MpSampleOut {         // any of them null
  int *status, *count, *needed;
  double *s, *sd, *sdd;
  double *pos, *vel, *acc, *tau;
};
struct MpSampleHead {
  double T;
  int status, count, needed;
};
template <int N>
struct MpSampleRow {
  double s, sd, sdd;
  double q[N], qd[N], qdd[N], tau[N];
};

// The flags of elements first, first + stride, ... of path b's tables: t and x by grid point, and (grid source) q, dq, ddq as
// grid * n flat entries each.
template <int SOURCE>
MP_HD int mp_ts_scan(const MpSampleIn& I, int n, long b, int first, int stride) {
  const double* t = I.t + b * I.grid;
  const double* x = I.x + b * I.grid;
  int f = 0;
  for (int i = first; i < I.grid; i += stride) {
    const double ti = t[i], xi = x[i];
    if (ti != ti || xi != xi) f |= MP_TS_F_NAN;
    if (ti == mp_tp_inf()) f |= MP_TS_F_STOP;
    if ((i == 0 && ti != 0.0) || (i + 1 < I.grid && t[i + 1] < ti) || xi < 0.0 || xi == mp_tp_inf()) f |= MP_TS_F_BAD;
  }
  if (SOURCE == MP_TS_GRID) {
    const long flat = (long)I.grid * n, o = b * flat;
    MpBad<double> bad;
    for (long e = first; e < flat; e += stride) {
      bad.add(I.q[o + e]);
      bad.add(I.dq[o + e]);
      bad.add(I.ddq[o + e]);
    }
    if (bad.any()) f |= MP_TS_F_BAD;
  }
  return f;
}

// Path b's verdict from its flags: the screen in the contract's order, then k_end by ceil and one correction each way.  (One exit
// and plain selects: the head stays in registers.)
template <int SOURCE>
MP_HD MpSampleHead mp_ts_head(const MpSampleIn& I, long b, int flags) {
  bool curve = true, geometry = true;
  if (SOURCE == MP_TS_CURVE) {
    const int st = I.bstatus[b], m = I.bcount[b];
    curve = (st == MP_BL_DONE || st == MP_BL_STRAIGHT || st == MP_BL_POINT) && m >= 1 && m <= I.w_in;
    geometry = mp_tp_finite(I.length[b]);
  }
  const bool untimed = (flags & MP_TS_F_NAN) != 0 || !curve;
  const bool stops = !untimed && (flags & MP_TS_F_STOP) != 0;
  const double T = I.t[b * I.grid + (I.grid - 1)];
  const double ratio = T / I.dt;
  const bool invalid = !untimed && !stops && ((flags & MP_TS_F_BAD) != 0 || !geometry || !(ratio < MP_TS_MAX_RATIO));
  const bool dead = untimed || stops || invalid;
  long k = dead ? 0 : (long)__builtin_ceil(ratio);
  if (k > 0 && (double)(k - 1) * I.dt >= T) k -= 1;
  else if ((double)k * I.dt < T) k += 1;
  const bool cut = k + 1 > (long)I.M;
  MpSampleHead H;
  H.T = dead ? mp_tp_nan() : T;
  H.needed = dead ? 0 : (int)(k + 1);
  H.count = dead ? 0 : (cut ? I.M : (int)(k + 1));
  H.status = untimed ? MP_TS_UNTIMED : stops ? MP_TS_STOPS : invalid ? MP_TS_INVALID : cut ? MP_TS_TRUNCATED : MP_TS_OK;
  return H;
}

// The quintic Hermite interpolant of grid points i and i + 1 at u = (s - s_i) / D in [0, 1], nm1 = grid - 1 = 1 / D: q, dq/ds, d2q/ds2.
// Written around q_i + H3 (q_{i+1} - q_i) so that a constant path is reproduced exactly; u = 0 is q_i bit for bit.
template <int N>
MP_HD void mp_ts_hermite(const double* q0, const double* d0, const double* e0, double u, double nm1, double (&q)[N], double (&dq)[N],
                         double (&ddq)[N]) {
  const double h = 1.0 / nm1, u2 = u * u, u3 = u2 * u;
  const double H3 = u3 * (10.0 + u * (-15.0 + 6.0 * u)), H1 = u + u3 * (-6.0 + u * (8.0 - 3.0 * u));
  const double H4 = u3 * (-4.0 + u * (7.0 - 3.0 * u)), H2 = u2 * (0.5 + u * (-1.5 + u * (1.5 - 0.5 * u)));
  const double H5 = u3 * (0.5 + u * (-1.0 + 0.5 * u));
  const double w = 1.0 - u;
  const double G3 = 30.0 * (u2 * (w * w)), G1 = 1.0 + u2 * (-18.0 + u * (32.0 - 15.0 * u)), G4 = u2 * (-12.0 + u * (28.0 - 15.0 * u));
  const double G2 = u * (1.0 + u * (-4.5 + u * (6.0 - 2.5 * u))), G5 = u2 * (1.5 + u * (-4.0 + 2.5 * u));
  const double F3 = u * (60.0 + u * (-180.0 + 120.0 * u)), F1 = u * (-36.0 + u * (96.0 - 60.0 * u)), F4 = u * (-24.0 + u * (84.0 - 60.0 * u));
  const double F2 = 1.0 + u * (-9.0 + u * (18.0 - 10.0 * u)), F5 = u * (3.0 + u * (-12.0 + 10.0 * u));
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double qa = q0[j], qb = q0[N + j], da = d0[j], db = d0[N + j], ea = e0[j], eb = e0[N + j];
    const double D = qb - qa;
    const double p1 = h * mp_two_products(H1, da, H4, db), p2 = (h * h) * mp_two_products(H2, ea, H5, eb);
    const double p = qa + (__builtin_fma(H3, D, p1) + p2);
    q[j] = u == 0.0 ? qa : p;
    const double v1 = mp_two_products(G1, da, G4, db), v2 = h * mp_two_products(G2, ea, G5, eb);
    dq[j] = __builtin_fma(nm1 * G3, D, v1) + v2;
    const double a1 = nm1 * mp_two_products(F1, da, F4, db), a2 = mp_two_products(F2, ea, F5, eb);
    ddq[j] = __builtin_fma((nm1 * nm1) * F3, D, a1) + a2;
  }
}

// Row k of path b, H the path's head.  A path without samples: NaN in everything.
template <int N, int SOURCE, int TAU, typename MT>
MP_HD void mp_ts_row(const MT& M, const MpCall<double>& C, const MpSampleIn& I, long b, const MpSampleHead& H, long k, MpSampleRow<N>& o) {
  if (H.count == 0) {
    const double nan = mp_tp_nan();
    o.s = nan; o.sd = nan; o.sdd = nan;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      o.q[j] = nan; o.qd[j] = nan; o.qdd[j] = nan;
      if (TAU != MP_TS_NO_TAU) o.tau[j] = nan;
    }
    return;
  }
  const double* t = I.t + b * I.grid;
  const double* x = I.x + b * I.grid;
  const double tk = (double)k * I.dt;
  const double* points = SOURCE == MP_TS_CURVE ? I.points + b * (long)I.w_in * N : nullptr;
  const int m = SOURCE == MP_TS_CURVE ? I.bcount[b] : 0;
  if (!(tk < H.T)) {  // the hold row: the path's end point at rest
    o.s = 1.0; o.sd = 0.0; o.sdd = 0.0;
    const double* end = SOURCE == MP_TS_CURVE ? points + (long)(m - 1) * N : I.q + (b * I.grid + (I.grid - 1)) * N;
#pragma unroll
    for (int j = 0; j < N; ++j) { o.q[j] = end[j]; o.qd[j] = 0.0; o.qdd[j] = 0.0; }
  } else {
    int lo = 0, hi = I.grid - 2;
    while (lo < hi) {  // the largest i in 0..grid-2 with t[i] <= tk
      const int mid = (lo + hi + 1) >> 1;
      if (t[mid] <= tk) lo = mid;
      else hi = mid - 1;
    }
    const int i = lo;
    const double nm1 = (double)(I.grid - 1), D = 1.0 / nm1, two_d = 2.0 / nm1;
    const double xi = x[i], del = tk - t[i], r = mp_sqrt(xi), ub = (x[i + 1] - xi) / two_d;
    const double sig = mp_min(mp_max((r + 0.5 * ub * del) * del, 0.0), D);
    const double s = (double)i / nm1 + sig, sd = mp_max(r + ub * del, 0.0);
    o.s = s; o.sd = sd; o.sdd = ub;
    double d1[N], d2[N];
    if (SOURCE == MP_TS_CURVE) {
      mp_blend_sample_at<N>(m, I.length[b], points, I.cut + b * (long)I.w_in, I.knot + b * (long)I.w_in, s, o.q, d1, d2);
    } else {
      const long at = (b * I.grid + i) * N;
      mp_ts_hermite<N>(I.q + at, I.dq + at, I.ddq + at, mp_min(sig * nm1, 1.0), nm1, o.q, d1, d2);
    }
    const double x_ = sd * sd;
#pragma unroll
    for (int j = 0; j < N; ++j) { o.qd[j] = d1[j] * sd; o.qdd[j] = mp_two_products(d2[j], x_, d1[j], ub); }
  }
  if (TAU != MP_TS_NO_TAU) {
    MpJointState<double, N> js;
    mp_joint_state<double, N>(M, o.q, js);
    const double tn[3] = {C.F1n[0], C.F1n[1], C.F1n[2]}, tf[3] = {C.F1f[0], C.F1f[1], C.F1f[2]};
    mp_tp_rnea<N, true, TAU == MP_TS_TAU_FTIP>(M, C.a0, tn, tf, js, o.qd, o.qdd, o.tau);
  }
}

// One path on the host, for the CPU twin: its head, then its M rows into the arrays of O (whole arrays; row b * M + k).
template <int N, int SOURCE, int TAU, typename MT>
void mp_ts_path_cpu(const MT& M, const MpCall<double>& C, const MpSampleIn& I, const MpSampleOut& O, long b) {
  const MpSampleHead H = mp_ts_head<SOURCE>(I, b, mp_ts_scan<SOURCE>(I, N, b, 0, 1));
  if (O.status) O.status[b] = H.status;
  if (O.count) O.count[b] = H.count;
  if (O.needed) O.needed[b] = H.needed;
  if (!(O.s || O.sd || O.sdd || O.pos || O.vel || O.acc || O.tau)) return;
  for (long k = 0; k < I.M; ++k) {
    MpSampleRow<N> o;
    mp_ts_row<N, SOURCE, TAU>(M, C, I, b, H, k, o);
    const long r = b * I.M + k;
    if (O.s) O.s[r] = o.s;
    if (O.sd) O.sd[r] = o.sd;
    if (O.sdd) O.sdd[r] = o.sdd;
    for (int j = 0; j < N; ++j) {
      if (O.pos) O.pos[r * N + j] = o.q[j];
      if (O.vel) O.vel[r * N + j] = o.qd[j];
      if (O.acc) O.acc[r * N + j] = o.qdd[j];
      if (TAU != MP_TS_NO_TAU && O.tau) O.tau[r * N + j] = o.tau[j];
    }
  }
}
