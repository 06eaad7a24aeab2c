// C2 corner blending of piecewise-linear joint-space paths over the sphere collision model, one problem per call (float64,
// 1..MP_MAX_DOF joints).  Header-only like mp_shortcut.h: the HIP kernels k_path_blend / k_path_blend_sample (mp_kernels.hip) and the
// CPU twin (mp_cpu.cpp) instantiate the same templates.  The contract - screen, compaction, segments, the attempts of a corner, the
// parameter sigma, the grid, the outputs - is stated once, in include/manipula_hip.h (mp_path_blend_*); this is how it is computed.
//
// A problem is a small state machine around the evaluation of mp_collision.h, in the style of mp_goal.h.  mp_blend_begin screens the
// problem, compacts its rows into `points`, looks for a reversal and sets the first corner up; one mp_blend_trip then makes exactly
// one collision evaluation of the running attempt and books what it decides: the next attempt at half the cut, the next corner, or
// the end of the problem.  The state is the corner itself - its point and the unit directions of the two segments that meet there,
// 3 n doubles - and a cursor into the problem's own input rows, from which the next corner is read: there is no workspace.  `cut`
// and `knot` are written as the corners are proven, the padding (or the NaN rows of a problem that has no curve) when it ends.
//
// The curve variant of the edge check: mp_blend_curve_begin makes the speed bounds L[ka][kb] of mp_col_edge_begin with the curve's
// |dq_j/du| <= v_j in the place of |D_j| and the hull's reach in the place of the end points'; mp_blend_curve_iterate is
// mp_col_edge_iterate on q(u).  mp_collision_edge_eval is used as it is.
//
// mp_blend_sample is one grid point of a finished problem, read back from `points`, `cut`, `knot`: the body of k_path_blend_sample.
#pragma once

#include "mp_collision.h"

constexpr int MP_BL_DONE = 0, MP_BL_STRAIGHT = 1, MP_BL_SKIPPED = 2, MP_BL_POINT = 3, MP_BL_BLOCKED = 4, MP_BL_REVERSAL = 5,
              MP_BL_INVALID = -1;  // = MP_BLEND_*
constexpr int MP_BL_MAX_WAYPOINTS = 65536, MP_BL_MAX_GRID = 65536, MP_BL_MAX_HALVINGS = 32;
#define MP_BL_REVERSAL_DOT (-1.0 + 1e-9)

struct MpBlendParams {
  MpColEdgeParams edge;
  double blend;
  int max_halvings, w_in, grid, pad;  // w_in: the rows of an input path; grid: the grid points N
};

// the per-problem outputs of the work-queue kernel, any of them null (the grid's q, dq, ddq are sampled from them afterwards)
struct MpBlendOut {
  int *status, *corner, *count;
  double* points;    // (B, w_in, n)
  double *cut, *knot;  // (B, w_in)
  double* length;
  int *halvings, *evaluations;
  double* clearance;
};
// the outputs a problem writes while it runs: its rows of `points`, `cut`, `knot`, any of them null
struct MpBlendRows {
  double* points;
  double* cut;
  double* knot;
};
MP_HD MpBlendRows mp_blend_rows(const MpBlendOut& O, long row, int w_in, int n) {
  return {O.points ? O.points + row * (long)w_in * n : nullptr, O.cut ? O.cut + row * (long)w_in : nullptr,
          O.knot ? O.knot + row * (long)w_in : nullptr};
}

constexpr int MP_BL_IDLE = 0, MP_BL_RUN = 1, MP_BL_FINISHED = 2;

template <int N>
struct MpBlendState {
  double r[N], uin[N], uout[N];  // the corner r_k and the unit directions of segments k and k + 1
  double lin, lout;              // their lengths
  double d;                      // the cut of the running attempt
  double u;                      // its parameter
  double cut_prev, knot_prev;    // cut[k - 1], knot[k - 1]
  double clearance, length;
  int phase, status, corner;
  int k, m;                      // the running corner, the points of the compacted path
  int inext;                     // the input row that holds r_{k+1}
  int attempts, steps;           // of the running corner / attempt
  int halvings, evals;
};

// D = to - from, l = sqrt(sum_j D_j^2) with j ascending, u = D / l: every unit direction of the problem is made here
template <int N>
MP_HD void mp_blend_segment(const double (&from)[N], const double (&to)[N], double (&u)[N], double& l) {
  double D[N], d2 = 0.0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    D[j] = to[j] - from[j];
    d2 += D[j] * D[j];
  }
  l = mp_sqrt(d2);
#pragma unroll
  for (int j = 0; j < N; ++j) u[j] = D[j] / l;
}

template <int N>
MP_HD void mp_blend_row(const double* rows, int w, double (&x)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) x[j] = rows[(long)w * N + j];
}

template <int N>
MP_HD bool mp_blend_differs(const double (&a)[N], const double (&b)[N]) {
  bool d = false;
#pragma unroll
  for (int j = 0; j < N; ++j) d = d || a[j] != b[j];
  return d;
}

// the first row after `w` that differs from `last` (there is one: the caller knows the compacted path goes on), copied into x
template <int N>
MP_HD int mp_blend_next(const double* rows, int count_in, int w, const double (&last)[N], double (&x)[N]) {
  for (++w; w < count_in; ++w) {
    mp_blend_row<N>(rows, w, x);
    if (mp_blend_differs<N>(x, last)) return w;
  }
  return count_in - 1;
}

// q(u) = r - d uin (1 - u)^4 (1 + 1.5 u) + d uout u^4 (2.5 - 1.5 u)
template <int N>
MP_HD void mp_blend_curve_point(const double (&r)[N], const double (&uin)[N], const double (&uout)[N], double d, double u, double (&q)[N]) {
  const double w = 1.0 - u;
  const double w2 = w * w, u2 = u * u;
  const double A = d * ((w2 * w2) * (1.0 + 1.5 * u)), B = d * ((u2 * u2) * (2.5 - 1.5 * u));
#pragma unroll
  for (int j = 0; j < N; ++j) q[j] = (r[j] - A * uin[j]) + B * uout[j];
}

// The speed bounds of the blend of cut d at the state's corner: mp_col_edge_begin's sums with v_j = 2.5 d max(|uin_j|, |uout_j|) in
// the place of |D_j| and reach_j = max(|a_j|, |r_j|, |b_j|), a = r - d uin, b = r + d uout; the attempt starts at u = 0.
template <int N, typename MT, typename SP, typename BOUNDS>
MP_HD void mp_blend_curve_begin(const MT& M, const SP& sph, MpBlendState<N>& S, BOUNDS& L) {
  double v[N], reach[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    v[j] = 2.5 * S.d * mp_max(mp_abs(S.uin[j]), mp_abs(S.uout[j]));
    const double a = S.r[j] - S.d * S.uin[j], b = S.r[j] + S.d * S.uout[j];
    reach[j] = mp_max(mp_max(mp_abs(a), mp_abs(S.r[j])), mp_abs(b));
  }
#pragma unroll
  for (int kb = 1; kb <= N; ++kb) {
    double e = 0.0, acc = 0.0;
#pragma unroll
    for (int j = kb; j >= 1; --j) {
      const bool rev = mp_joint_of(M, j - 1).rev != 0.0;
      const double w = rev ? sph->rho[j - 1][kb] + e : 1.0;
      acc += v[j - 1] * w;
      L.put(mp_col_bound_index(j - 1, kb), acc);
      if (!rev) e += reach[j - 1];
    }
  }
  S.u = 0.0;
  S.steps = 0;
}

// One evaluation at S.u.  Returns 0 while the attempt is running, otherwise 1 + MP_COL_EDGE_FREE / _BLOCKED / _UNDECIDED.
template <int N, typename MT, typename TB, typename PARK, typename BOUNDS>
MP_HD int mp_blend_curve_iterate(const MT& M, const TB& tb, const MpColEdgeParams& P, MpBlendState<N>& S, PARK& park, const BOUNDS& L) {
  double q[N];
  mp_blend_curve_point<N>(S.r, S.uin, S.uout, S.d, S.u, q);
  MpColEdgeEval ev;
  mp_collision_edge_eval<N>(M, tb, q, P.margin, park, L, ev);
  S.steps += 1;
  S.evals += 1;
  const double d = ev.dist_world <= ev.dist_self ? ev.dist_world : ev.dist_self;
  if (d < S.clearance) S.clearance = d;
  if (d - P.margin <= P.tol) return 1 + MP_COL_EDGE_BLOCKED;
  if (S.u + ev.tau >= 1.0) return 1 + MP_COL_EDGE_FREE;
  if (S.steps >= P.max_steps) return 1 + MP_COL_EDGE_UNDECIDED;
  S.u += ev.tau;
  return 0;
}

// The problem has ended.  A curve (DONE / STRAIGHT / POINT): the padding of cut (0) and knot (the length) and their first entries;
// otherwise NaN in every row of points, cut and knot, a NaN length and clearance and m = 0.
template <int N>
MP_HD void mp_blend_finish(const MpBlendParams& P, MpBlendState<N>& S, int status, const MpBlendRows& o) {
  S.status = status;
  S.phase = MP_BL_FINISHED;
  const bool curve = status == MP_BL_DONE || status == MP_BL_STRAIGHT || status == MP_BL_POINT;
  const double nan = __builtin_nan("");
  if (curve) {
    if (o.cut != nullptr) {
      o.cut[0] = 0.0;
      for (int w = S.m - 1; w < P.w_in; ++w) o.cut[w] = 0.0;
    }
    if (o.knot != nullptr) {
      o.knot[0] = 0.0;
      for (int w = S.m - 1; w < P.w_in; ++w) o.knot[w] = S.length;
    }
  } else {
    S.m = 0;
    S.length = nan;
    S.clearance = nan;
    for (int w = 0; w < P.w_in; ++w) {
      if (o.cut != nullptr) o.cut[w] = nan;
      if (o.knot != nullptr) o.knot[w] = nan;
      if (o.points != nullptr) {
#pragma unroll
        for (int j = 0; j < N; ++j) o.points[(long)w * N + j] = nan;
      }
    }
  }
}

// the first attempt of the state's corner
template <int N, typename MT, typename SP, typename BOUNDS>
MP_HD void mp_blend_corner_begin(const MT& M, const SP& sph, const MpBlendParams& P, MpBlendState<N>& S, BOUNDS& L) {
  S.d = mp_min(mp_min(P.blend, S.lin / 2), S.lout / 2);
  S.attempts = 0;
  mp_blend_curve_begin<N>(M, sph, S, L);
}

// A new problem: screened, compacted into o.points (padded by repeating the last point), searched for a reversal; then its first
// corner is set up.  rows = the problem's w_in input rows.
template <int N, typename MT, typename SP, typename BOUNDS>
MP_HD void mp_blend_begin(const MT& M, const SP& sph, const MpBlendParams& P, const double* rows, int count_in, MpBlendState<N>& S,
                          BOUNDS& L, const MpBlendRows& o) {
  S.corner = -1;
  S.k = 0; S.m = 0; S.inext = 0; S.attempts = 0; S.steps = 0; S.halvings = 0; S.evals = 0;
  S.cut_prev = 0.0; S.knot_prev = 0.0; S.length = 0.0; S.d = 0.0; S.u = 0.0; S.lin = 0.0; S.lout = 0.0;
  S.clearance = __builtin_huge_val();
  if (count_in < 2) {
    mp_blend_finish<N>(P, S, MP_BL_SKIPPED, o);
    return;
  }
  if (count_in > P.w_in) {
    mp_blend_finish<N>(P, S, MP_BL_INVALID, o);
    return;
  }
  MpBad<double> bad;
  for (int w = 0; w < count_in; ++w) {
    double x[N];
    mp_blend_row<N>(rows, w, x);
    bad.add(x);
  }
  if (bad.any()) {
    mp_blend_finish<N>(P, S, MP_BL_INVALID, o);
    return;
  }
  // compaction; the unit directions of the last two segments follow it, so that every corner's dot product is seen once
  double last[N], ua[N], ub[N];
  mp_blend_row<N>(rows, 0, last);
#pragma unroll
  for (int j = 0; j < N; ++j) { ua[j] = 0.0; ub[j] = 0.0; }
  int m = 1, reversal = -1, second = 0;
  double l1 = 0.0;
  if (o.points != nullptr) {
#pragma unroll
    for (int j = 0; j < N; ++j) o.points[j] = last[j];
  }
  for (int w = 1; w < count_in; ++w) {
    double x[N];
    mp_blend_row<N>(rows, w, x);
    if (!mp_blend_differs<N>(x, last)) continue;
    if (o.points != nullptr) {
#pragma unroll
      for (int j = 0; j < N; ++j) o.points[(long)m * N + j] = x[j];
    }
    double l;
    mp_blend_segment<N>(last, x, ub, l);
    if (m == 1) { second = w; l1 = l; }
    if (m >= 2 && reversal < 0) {
      double dot = 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) dot += ua[j] * ub[j];
      if (dot < MP_BL_REVERSAL_DOT) reversal = m - 1;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) { last[j] = x[j]; ua[j] = ub[j]; }
    m += 1;
  }
  S.m = m;
  if (o.points != nullptr) {
    for (int w = m; w < P.w_in; ++w) {
#pragma unroll
      for (int j = 0; j < N; ++j) o.points[(long)w * N + j] = last[j];
    }
  }
  if (m == 1) {
    mp_blend_finish<N>(P, S, MP_BL_POINT, o);
    return;
  }
  if (m == 2) {
    S.length = l1;
    mp_blend_finish<N>(P, S, MP_BL_STRAIGHT, o);
    return;
  }
  if (reversal >= 0) {
    S.corner = reversal;
    mp_blend_finish<N>(P, S, MP_BL_REVERSAL, o);
    return;
  }
  // corner 1: r_0, r_1 = the row `second`, r_2 = the next row that differs
  double r0[N], r2[N];
  mp_blend_row<N>(rows, 0, r0);
  mp_blend_row<N>(rows, second, S.r);
  mp_blend_segment<N>(r0, S.r, S.uin, S.lin);
  S.inext = mp_blend_next<N>(rows, count_in, second, S.r, r2);
  mp_blend_segment<N>(S.r, r2, S.uout, S.lout);
  S.k = 1;
  S.phase = MP_BL_RUN;
  mp_blend_corner_begin<N>(M, sph, P, S, L);
}

// One trip: one evaluation of the running attempt and what follows from its decision.  Returns 1 when the problem has ended
// (S.status, S.corner, S.m, S.length, S.halvings, S.evals, S.clearance are its outputs, its rows are written), 0 while it is running
// - and for an IDLE state.
template <int N, typename MT, typename TB, typename PARK, typename BOUNDS>
MP_HD int mp_blend_trip(const MT& M, const TB& tb, const MpBlendParams& P, const double* rows, int count_in, MpBlendState<N>& S,
                        PARK& park, BOUNDS& L, const MpBlendRows& o) {
  if (S.phase == MP_BL_RUN) {
    const int done = mp_blend_curve_iterate<N>(M, tb, P.edge, S, park, L);
    if (done - 1 == MP_COL_EDGE_FREE) {
      // knot[k] = knot[k-1] + 2.5 cut[k-1] + (l_k - cut[k-1] - cut[k])
      const double knot = (S.knot_prev + 2.5 * S.cut_prev) + ((S.lin - S.cut_prev) - S.d);
      if (o.cut != nullptr) o.cut[S.k] = S.d;
      if (o.knot != nullptr) o.knot[S.k] = knot;
      S.cut_prev = S.d;
      S.knot_prev = knot;
      if (S.k == S.m - 2) {  // the last corner: knot[m-1] is the length
        S.length = (knot + 2.5 * S.d) + (S.lout - S.d);
        mp_blend_finish<N>(P, S, MP_BL_DONE, o);
      } else {
        double r2[N];
        mp_blend_row<N>(rows, S.inext, S.r);
#pragma unroll
        for (int j = 0; j < N; ++j) S.uin[j] = S.uout[j];
        S.lin = S.lout;
        S.inext = mp_blend_next<N>(rows, count_in, S.inext, S.r, r2);
        mp_blend_segment<N>(S.r, r2, S.uout, S.lout);
        S.k += 1;
        mp_blend_corner_begin<N>(M, tb.sph, P, S, L);
      }
    } else if (done != 0) {  // a failed attempt
      S.halvings += 1;
      S.attempts += 1;
      if (S.attempts > P.max_halvings) {
        S.corner = S.k;
        mp_blend_finish<N>(P, S, MP_BL_BLOCKED, o);
      } else {
        S.d = S.d / 2;
        mp_blend_curve_begin<N>(M, tb.sph, S, L);
      }
    }
  }
  return S.phase == MP_BL_FINISHED ? 1 : 0;
}

// the row a finished problem reports beside what it wrote while it ran, stored by the kernel and the twin alike
template <int N>
MP_HD void mp_blend_store(const MpBlendOut& O, long row, const MpBlendState<N>& S) {
  if (O.status) O.status[row] = S.status;
  if (O.corner) O.corner[row] = S.corner;
  if (O.count) O.count[row] = S.m;
  if (O.length) O.length[row] = S.length;
  if (O.halvings) O.halvings[row] = S.halvings;
  if (O.evaluations) O.evaluations[row] = S.evals;
  if (O.clearance) O.clearance[row] = S.clearance;
}

// Problem b over plain host rows, for the CPU twin: S is left as the last trip left it.  rows: its input rows; o: its rows of points /
// cut / knot, any of them null.
template <int N, typename MT, typename TB>
void mp_blend_cpu(const MT& M, const TB& tb, const MpBlendParams& P, const double* rows, int count_in, long b, const MpBlendRows& o,
                  const MpBlendOut& O, MpBlendState<N>& S) {
  MpColParkLocal park;
  MpColBoundsLocal<N> L;
  S.phase = MP_BL_IDLE;
  mp_blend_begin<N>(M, tb.sph, P, rows, count_in, S, L, o);
  while (!mp_blend_trip<N>(M, tb, P, rows, count_in, S, park, L, o)) {}
  mp_blend_store<N>(O, b, S);
}

// Grid point i of a finished problem: q, dq/ds, d2q/ds2 at s_i = i / (grid - 1).  points / cut / knot: the problem's rows.
template <int N>
MP_HD void mp_blend_sample(int status, int m, double length, const double* points, const double* cut, const double* knot, int i, int grid,
                           double (&q)[N], double (&dq)[N], double (&ddq)[N]) {
  const bool curve = status == MP_BL_DONE || status == MP_BL_STRAIGHT || status == MP_BL_POINT;
  if (!curve || m < 1) {
#pragma unroll
    for (int j = 0; j < N; ++j) { q[j] = __builtin_nan(""); dq[j] = q[j]; ddq[j] = q[j]; }
    return;
  }
#pragma unroll
  for (int j = 0; j < N; ++j) ddq[j] = 0.0;
  if (m == 1) {
    mp_blend_row<N>(points, 0, q);
#pragma unroll
    for (int j = 0; j < N; ++j) dq[j] = 0.0;
    return;
  }
  const double sigma = ((double)i / (double)(grid - 1)) * length;
  int k;
  if (i == 0) {
    k = 0;
  } else if (i == grid - 1) {
    k = m - 2;
  } else {
    int lo = 0, hi = m - 2;
    while (lo < hi) {  // the largest k in 0..m-2 with knot[k] <= sigma
      const int mid = (lo + hi + 1) >> 1;
      if (knot[mid] <= sigma) lo = mid;
      else hi = mid - 1;
    }
    k = lo;
  }
  double rk[N], rn[N], un[N], ln;
  mp_blend_row<N>(points, k, rk);
  mp_blend_row<N>(points, k + 1, rn);
  mp_blend_segment<N>(rk, rn, un, ln);  // u_{k+1}
  if (i == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) { q[j] = rk[j]; dq[j] = length * un[j]; }
    return;
  }
  if (i == grid - 1) {
#pragma unroll
    for (int j = 0; j < N; ++j) { q[j] = rn[j]; dq[j] = length * un[j]; }
    return;
  }
  const double ck = cut[k], at = sigma - knot[k];
  if (k >= 1 && at < 2.5 * ck) {
    double rp[N], up[N], lp;
    mp_blend_row<N>(points, k - 1, rp);
    mp_blend_segment<N>(rp, rk, up, lp);  // u_k
    const double u = at / (2.5 * ck), w = 1.0 - u;
    mp_blend_curve_point<N>(rk, up, un, ck, u, q);
    const double fa = (w * w * w) * (1.0 + 3.0 * u), fb = (u * u * u) * (4.0 - 3.0 * u);
    const double g = (length * length) * 4.8 * (u * w);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      dq[j] = length * (up[j] * fa + un[j] * fb);
      ddq[j] = g * (u * un[j] - w * up[j]) / ck;
    }
  } else {
    const double t = ((ck + sigma) - knot[k]) - 2.5 * ck;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      q[j] = rk[j] + t * un[j];
      dq[j] = length * un[j];
    }
  }
}

// a b + c d with the rounding pinned: one product, then one fused multiply-add.  Left as a sum of two products the compiler fuses
// either of them, as the code around the sum suggests, and the kernel variants of the trajectory sampler (with and without the
// torques) must round the geometry alike.
MP_HD double mp_two_products(double a, double b, double c, double d) { return __builtin_fma(a, b, c * d); }

// The same curve at a real parameter s in [0, 1] (sigma = s * length) of a problem that has one (m >= 1): the formulas of
// mp_blend_sample, step 6 of the contract, with s in the place of i / (grid - 1).  s <= 0 and s >= 1 are the end points themselves,
// bit for bit.  For the trajectory sampler (mp_sample.h); mp_blend_sample is not touched.  Sums of two products go through mp_two_products.
template <int N>
MP_HD void mp_blend_sample_at(int m, double length, const double* points, const double* cut, const double* knot, double s, double (&q)[N],
                              double (&dq)[N], double (&ddq)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) ddq[j] = 0.0;
  if (m == 1) {
    mp_blend_row<N>(points, 0, q);
#pragma unroll
    for (int j = 0; j < N; ++j) dq[j] = 0.0;
    return;
  }
  const bool first = !(s > 0.0), last = !first && s >= 1.0;
  const double sigma = s * length;
  int k;
  if (first) {
    k = 0;
  } else if (last) {
    k = m - 2;
  } else {
    int lo = 0, hi = m - 2;
    while (lo < hi) {  // the largest k in 0..m-2 with knot[k] <= sigma
      const int mid = (lo + hi + 1) >> 1;
      if (knot[mid] <= sigma) lo = mid;
      else hi = mid - 1;
    }
    k = lo;
  }
  double rk[N], rn[N], un[N], ln;
  mp_blend_row<N>(points, k, rk);
  mp_blend_row<N>(points, k + 1, rn);
  mp_blend_segment<N>(rk, rn, un, ln);  // u_{k+1}
  if (first || last) {
#pragma unroll
    for (int j = 0; j < N; ++j) { q[j] = first ? rk[j] : rn[j]; dq[j] = length * un[j]; }
    return;
  }
  const double ck = cut[k], at = sigma - knot[k];
  if (k >= 1 && at < 2.5 * ck) {
    double rp[N], up[N], lp;
    mp_blend_row<N>(points, k - 1, rp);
    mp_blend_segment<N>(rp, rk, up, lp);  // u_k
    const double u = at / (2.5 * ck), w = 1.0 - u;
    mp_blend_curve_point<N>(rk, up, un, ck, u, q);
    const double fa = (w * w * w) * (1.0 + 3.0 * u), fb = (u * u * u) * (4.0 - 3.0 * u);
    const double g = (length * length) * 4.8 * (u * w);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      dq[j] = length * mp_two_products(up[j], fa, un[j], fb);
      ddq[j] = g * mp_two_products(u, un[j], -w, up[j]) / ck;
    }
  } else {
    const double t = ((ck + sigma) - knot[k]) - 2.5 * ck;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      q[j] = rk[j] + t * un[j];
      dq[j] = length * un[j];
    }
  }
}
