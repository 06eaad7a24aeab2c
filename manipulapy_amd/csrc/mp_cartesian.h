// Cartesian straight-line paths, tracked in joint space and proven free over the sphere collision model (float64, 3..MP_MAX_DOF
// joints).  Header-only like mp_blend.h: the HIP kernels k_cart_track / k_cart_span / k_cart_reduce (mp_kernels.hip) and the CPU twin
// (mp_cpu.cpp) instantiate the same templates.  The contract - the line, the tracking and its four decisions, the spans and their
// proof, the deviation, the outputs - is stated once, in include/manipula_hip.h (mp_cartesian_path_*); this is how it is computed.
//
// Three steps, each a function of the problem's (or the span's) content alone:
//   mp_cart_track   one problem, grid point by grid point: predictor, damped Newton steps on the hybrid Jacobian (the step of
//                   mp_goal.h without its clamp), then the undamped minimum-norm dq/ds and d2q/ds2 of the accepted point (the
//                   factorisation and pivot rule of mp_opspace.h, Jdot qd from mp_opspace_kin in the hybrid frame).  The rows go out
//                   as they are accepted; the head (tracking status, reached, iterations, pose error) goes to the workspace.
//   mp_cart_span_*  one span of a fully tracked problem: the quintic Hermite interpolant of rows i and i + 1 is a quintic Bezier
//                   curve, whose control polygon bounds |dq_j/du| and |q_j(u)|; those go into the sums of mp_blend_curve_begin, and
//                   the advance is mp_blend_curve_iterate's with mp_ts_hermite as the point evaluator - the curve the trajectory
//                   sampler executes.  begin also measures the curve's midpoint against the line.  A span's record goes to the
//                   workspace.
//   mp_cart_reduce  one problem: its spans' records, walked in order, into status / span / t / clearance / deviations / evaluations.
// Independent spans get a lane each; nothing a problem reports depends on which lane served which span.
//
// TASK rows: MR = 6 (FULL: angular rows first, as mp_ik_error and the Jacobian order them) or 3 (POSITION: the linear rows).
#pragma once

#include "mp_collision.h"
#include "mp_ik.h"
#include "mp_opspace.h"
#include "mp_sample.h"

constexpr int MP_CP_DONE = 0, MP_CP_STALLED = 1, MP_CP_SINGULAR = 2, MP_CP_LIMIT = 3, MP_CP_JUMP = 4, MP_CP_BLOCKED = 5,
              MP_CP_UNDECIDED = 6, MP_CP_INVALID = -1;  // = MP_CARTESIAN_*
constexpr int MP_CP_SPAN_SKIPPED = -1;                  // a span of a problem that was not tracked to its end (else MP_COL_EDGE_*)
constexpr int MP_CP_FULL = 0, MP_CP_POSITION = 1;       // = MP_TASK_* ; the `task` of mp_opspace_kin
constexpr int MP_CP_MAX_GRID = 65536, MP_CP_MAX_ITERS = 65536;
#define MP_CP_HALF_TURN (3.14159265358979323846 - 1e-6)

struct MpCartParams {
  double lo[MP_MAX_DOF], hi[MP_MAX_DOF];
  double eomg, ev, damping, max_joint_step;
  MpColEdgeParams edge;  // margin, tol, max_steps
  int grid, task, max_iters, pad;
};

// The workspace of one call: the heads of B problems and the records of E = B (grid - 1) spans, as arrays (the doubles first).
struct MpCartWork {
  double *pose_error;                 // (B)
  double *t, *clearance, *dpos, *drot;  // (E)
  int *track, *reached, *iterations;  // (B)
  int *sstatus, *sevals;              // (E)
};
MP_HD size_t mp_cart_work_bytes(long B, long grid) {
  const size_t b = (size_t)B, e = (size_t)B * (size_t)(grid - 1);
  return ((8 * (b + 4 * e) + 4 * (3 * b + 2 * e)) + 15) & ~(size_t)15;
}
MP_HD MpCartWork mp_cart_work(void* base, long B, long grid) {
  const size_t b = (size_t)B, e = (size_t)B * (size_t)(grid - 1);
  double* d = static_cast<double*>(base);
  int* i = reinterpret_cast<int*>(d + b + 4 * e);
  return {d, d + b, d + b + e, d + b + 2 * e, d + b + 3 * e, i, i + b, i + 2 * b, i + 3 * b, i + 3 * b + e};
}

// the per-problem outputs of a call, any of them null
struct MpCartOut {
  int *status, *reached, *span;
  double *t, *clearance, *deviation_pos, *deviation_rot, *pose_error;
  int *iterations, *evaluations;
  int* span_status;        // (B, grid - 1)
  double* span_clearance;  // (B, grid - 1)
};

// The line's pose at s: R(s) = exp([omega] s) R_start, p(s) = p_start + s v; Ts = the start pose (0..11 read), V = [omega; v].
// POSITION keeps R_start: its rotation is never compared.
template <int MR>
MP_HD void mp_cart_target(const double (&Ts)[16], const double (&V)[6], double s, double (&Td)[16]) {
  Td[3] = Ts[3] + s * V[3]; Td[7] = Ts[7] + s * V[4]; Td[11] = Ts[11] + s * V[5];
  Td[12] = 0.0; Td[13] = 0.0; Td[14] = 0.0; Td[15] = 1.0;
  double E[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  if (MR == 6) {
    const double a = mp_sqrt(V[0] * V[0] + V[1] * V[1] + V[2] * V[2]);
    if (a > 0.0) {
      const double kx = V[0] / a, ky = V[1] / a, kz = V[2] / a, th = a * s;
      const double sn = sin(th), c1 = 1.0 - cos(th);
      E[0] = 1.0 - c1 * (ky * ky + kz * kz); E[1] = c1 * (kx * ky) - sn * kz;     E[2] = c1 * (kx * kz) + sn * ky;
      E[3] = c1 * (kx * ky) + sn * kz;     E[4] = 1.0 - c1 * (kx * kx + kz * kz); E[5] = c1 * (ky * kz) - sn * kx;
      E[6] = c1 * (kx * kz) - sn * ky;     E[7] = c1 * (ky * kz) + sn * kx;     E[8] = 1.0 - c1 * (kx * kx + ky * ky);
    }
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) Td[4 * r + c] = E[3 * r] * Ts[c] + E[3 * r + 1] * Ts[4 + c] + E[3 * r + 2] * Ts[8 + c];
}

// J (the space Jacobian of mp_fk_jac at a pose whose origin is p, 6 x N) -> the task's rows of the hybrid Jacobian (MR x N):
// v_i + w_i x p, under the angular rows when the task keeps them
template <int N, int MR>
MP_HD void mp_cart_hybrid(const double (&Tc)[16], const double (&J)[6 * N], double (&Jh)[MR * N]) {
  const double px = Tc[3], py = Tc[7], pz = Tc[11];
  constexpr int LIN = MR - 3;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double wx = J[i], wy = J[N + i], wz = J[2 * N + i];
    if (MR == 6) { Jh[i] = wx; Jh[N + i] = wy; Jh[2 * N + i] = wz; }
    Jh[(LIN + 0) * N + i] = J[3 * N + i] + (wy * pz - wz * py);
    Jh[(LIN + 1) * N + i] = J[4 * N + i] + (wz * px - wx * pz);
    Jh[(LIN + 2) * N + i] = J[5 * N + i] + (wx * py - wy * px);
  }
}

// the lower triangle of Jh Jh^T + lam 1
template <int N, int MR>
MP_HD void mp_cart_gram(const double (&Jh)[MR * N], double lam, double (&A)[MR][MR]) {
#pragma unroll
  for (int r = 0; r < MR; ++r) {
#pragma unroll
    for (int c = 0; c <= r; ++c) {
      double s = (r == c) ? lam : 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) s += Jh[r * N + j] * Jh[c * N + j];
      A[r][c] = s;
    }
#pragma unroll
    for (int c = r + 1; c < MR; ++c) A[r][c] = 0.0;  // (never read)
  }
}
template <int N, int MR>
MP_HD void mp_cart_back(const double (&Jh)[MR * N], const double (&y)[MR], double sign, double (&d)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < MR; ++r) s += Jh[r * N + j] * y[r];
    d[j] = sign * s;
  }
}
// the task's rows of the 6-vector [angular; linear]
template <int MR>
MP_HD void mp_cart_rows(const double (&V)[6], double (&y)[MR]) {
#pragma unroll
  for (int r = 0; r < MR; ++r) y[r] = V[(6 - MR) + r];
}

// The derivatives of an accepted point: dq = Jh^T (Jh Jh^T)^-1 V and ddq = -Jh^T (Jh Jh^T)^-1 (Jhdot dq), undamped.  Tc, J: the pose
// and space Jacobian at q.  Returns whether every pivot passed the rule of mp_opspace.h.
template <int N, int MR, typename MT>
MP_HD bool mp_cart_derivatives(const MT& M, const double (&q)[N], const double (&Tc)[16], const double (&J)[6 * N], const double (&V)[6],
                               double (&dq)[N], double (&ddq)[N]) {
  double Jh[MR * N], A[MR][MR], dg[MR], y[MR];
  mp_cart_hybrid<N, MR>(Tc, J, Jh);
  mp_cart_gram<N, MR>(Jh, 0.0, A);
  const bool ok = mp_os_chol<MR>(A, dg, MP_OS_PIVOT_EPS);
  mp_cart_rows<MR>(V, y);
  mp_os_fwd<MR>(A, y);
  mp_os_back<MR>(A, y);
  mp_cart_back<N, MR>(Jh, y, 1.0, dq);
  MpJointState<double, N> js;
  mp_joint_state<double, N>(M, q, js);
  double TT[16], J2[6 * N], jd[6];
  mp_opspace_kin<N>(M, 2, MR == 6 ? MP_CP_FULL : MP_CP_POSITION, js, dq, TT, J2, jd);  // the task's rows first
#pragma unroll
  for (int r = 0; r < MR; ++r) y[r] = jd[r];
  mp_os_fwd<MR>(A, y);
  mp_os_back<MR>(A, y);
  mp_cart_back<N, MR>(Jh, y, -1.0, ddq);
  return ok;
}

struct MpCartHead {
  double pose_error;
  int status, reached, iterations;  // status: DONE = tracked to the end, else the failing decision
};

// One problem's tracking.  q0p (n), Tgp (16, 0..11 read); qo / dqo / ddqo: the problem's grid rows, written as they are accepted and
// NaN from `reached` on.
template <int N, int MR, typename MT>
MP_HD void mp_cart_track(const MT& M, const MpCartParams& P, const double* __restrict__ q0p, const double* __restrict__ Tgp,
                         double* __restrict__ qo, double* __restrict__ dqo, double* __restrict__ ddqo, MpCartHead& H) {
  double q[N], Tg[16];
#pragma unroll
  for (int j = 0; j < N; ++j) q[j] = q0p[j];
#pragma unroll
  for (int k = 0; k < 12; ++k) Tg[k] = Tgp[k];
  Tg[12] = 0.0; Tg[13] = 0.0; Tg[14] = 0.0; Tg[15] = 1.0;
  MpBad<double> bad;
  bad.add(q);
#pragma unroll
  for (int k = 0; k < 12; ++k) bad.add(Tg[k]);
  H.status = MP_CP_DONE; H.reached = 0; H.iterations = 0; H.pose_error = 0.0;
  double Ts[16], J[6 * N], V[6], dq[N], ddq[N];
  if (bad.any()) {
    H.status = MP_CP_INVALID;
  } else {
    double rot, tr;
    MpIkUnrolled<N>::template fk<true>(M, q, Ts, J);
    mp_ik_error(Ts, Tg, V, rot, tr);
    bool in = true;
#pragma unroll
    for (int j = 0; j < N; ++j) in = in && q[j] >= P.lo[j] && q[j] <= P.hi[j];
    if (MR == 6 && rot >= MP_CP_HALF_TURN) H.status = MP_CP_INVALID;
    else if (!in) H.status = MP_CP_LIMIT;
    else if (!mp_cart_derivatives<N, MR>(M, q, Ts, J, V, dq, ddq)) H.status = MP_CP_SINGULAR;
  }
  const double nm1 = (double)(P.grid - 1), h = 1.0 / nm1;
  if (H.status == MP_CP_DONE) {
#pragma unroll
    for (int j = 0; j < N; ++j) { qo[j] = q[j]; dqo[j] = dq[j]; ddqo[j] = ddq[j]; }
    H.reached = 1;
    for (int i = 1; i < P.grid; ++i) {
      double qn[N], Td[16], Tc[16], e[6], rot = 0.0, tr = 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) qn[j] = q[j] + h * dq[j];
      mp_cart_target<MR>(Ts, V, (double)i / nm1, Td);
      int status = MP_CP_DONE;
      for (int k = 0;; ++k) {
        MpIkUnrolled<N>::template fk<true>(M, qn, Tc, J);
        mp_ik_error(Tc, Td, e, rot, tr);
        if ((MR == 3 || rot < P.eomg) && tr < P.ev) break;
        if (k >= P.max_iters) { status = MP_CP_STALLED; break; }
        double Jh[MR * N], A[MR][MR], y[MR], d[N];
        mp_cart_hybrid<N, MR>(Tc, J, Jh);
        mp_cart_gram<N, MR>(Jh, P.damping * P.damping, A);
        mp_cart_rows<MR>(e, y);
        mp_spd_solve<double, MR>(A, y);
        mp_cart_back<N, MR>(Jh, y, 1.0, d);
#pragma unroll
        for (int j = 0; j < N; ++j) qn[j] += d[j];
        H.iterations += 1;
      }
      if (status == MP_CP_DONE) {
        bool in = true;
        double jump = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          in = in && qn[j] >= P.lo[j] && qn[j] <= P.hi[j];
          jump = mp_max(jump, mp_abs(qn[j] - q[j]));
        }
        if (!in) status = MP_CP_LIMIT;
        else if (jump > P.max_joint_step) status = MP_CP_JUMP;
        else if (!mp_cart_derivatives<N, MR>(M, qn, Tc, J, V, dq, ddq)) status = MP_CP_SINGULAR;
      }
      if (status != MP_CP_DONE) { H.status = status; break; }
      const long at = (long)i * N;
#pragma unroll
      for (int j = 0; j < N; ++j) { q[j] = qn[j]; qo[at + j] = qn[j]; dqo[at + j] = dq[j]; ddqo[at + j] = ddq[j]; }
      H.reached = i + 1;
      const double err = MR == 6 ? mp_max(rot, tr) : tr;
      H.pose_error = mp_max(H.pose_error, err);
    }
  }
  const double nan = __builtin_nan("");
  for (long i = H.reached; i < P.grid; ++i) {
#pragma unroll
    for (int j = 0; j < N; ++j) { qo[i * N + j] = nan; dqo[i * N + j] = nan; ddqo[i * N + j] = nan; }
  }
  if (H.status == MP_CP_INVALID) H.pose_error = nan;
}

MP_HD void mp_cart_head_store(const MpCartWork& W, long b, const MpCartHead& H) {
  W.track[b] = H.status; W.reached[b] = H.reached; W.iterations[b] = H.iterations; W.pose_error[b] = H.pose_error;
}

struct MpCartSpan {
  double u, clearance, dpos, drot;
  int steps, status;
};

// A new span: rows i, i + 1 of the problem's grid at q0 / d0 / e0 (2 n doubles each), `first` = the problem's row 0 (the start
// configuration the line is rebuilt from), Tgp = its goal, smid = (i + 1/2) / (grid - 1).  The control polygon P0..P5 per joint gives
// v_j = 5 max |P_{k+1} - P_k| and reach_j = max |P_k|, which enter the sums of mp_blend_curve_begin; the midpoint of the curve is
// measured against the line.
template <int N, int MR, typename MT, typename SP, typename BOUNDS>
MP_HD void mp_cart_span_begin(const MT& M, const SP& sph, const double* __restrict__ q0, const double* __restrict__ d0,
                              const double* __restrict__ e0, const double* __restrict__ first, const double* __restrict__ Tgp, double nm1,
                              double smid, MpCartSpan& S, BOUNDS& L) {
  const double h = 1.0 / nm1;
  double v[N], reach[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double qa = q0[j], qb = q0[N + j], da = d0[j], db = d0[N + j], ea = e0[j], eb = e0[N + j];
    const double p0 = qa, p1 = qa + h * da / 5.0, p2 = (qa + 2.0 * h * da / 5.0) + (h * h) * ea / 20.0;
    const double p5 = qb, p4 = qb - h * db / 5.0, p3 = (qb - 2.0 * h * db / 5.0) + (h * h) * eb / 20.0;
    const double s01 = mp_abs(p1 - p0), s12 = mp_abs(p2 - p1), s23 = mp_abs(p3 - p2), s34 = mp_abs(p4 - p3), s45 = mp_abs(p5 - p4);
    v[j] = 5.0 * mp_max(mp_max(mp_max(s01, s12), mp_max(s23, s34)), s45);
    reach[j] = mp_max(mp_max(mp_max(mp_abs(p0), mp_abs(p1)), mp_max(mp_abs(p2), mp_abs(p3))), mp_max(mp_abs(p4), mp_abs(p5)));
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
  S.u = 0.0; S.steps = 0; S.status = 0;
  S.clearance = __builtin_huge_val();
  // the deviation: FK of the curve's midpoint against the line's pose at smid
  double qs[N], qm[N], dm[N], em[N], Tg[16], Ts[16], Tm[16], Td[16], J[6 * N], V[6], e[6], rot, tr;
#pragma unroll
  for (int j = 0; j < N; ++j) qs[j] = first[j];
#pragma unroll
  for (int k = 0; k < 12; ++k) Tg[k] = Tgp[k];
  Tg[12] = 0.0; Tg[13] = 0.0; Tg[14] = 0.0; Tg[15] = 1.0;
  MpIkUnrolled<N>::template fk<false>(M, qs, Ts, J);
  mp_ik_error(Ts, Tg, V, rot, tr);
  mp_cart_target<MR>(Ts, V, smid, Td);
  mp_ts_hermite<N>(q0, d0, e0, 0.5, nm1, qm, dm, em);
  MpIkUnrolled<N>::template fk<false>(M, qm, Tm, J);
  mp_ik_error(Tm, Td, e, rot, tr);
  S.dpos = tr;
  S.drot = MR == 6 ? rot : 0.0;
}

// One evaluation at S.u: the iteration and the three decisions of mp_blend_curve_iterate on the Hermite interpolant.  Returns 0 while
// the span is running, otherwise 1 + MP_COL_EDGE_FREE / _BLOCKED / _UNDECIDED (S.u is then the reported t; FREE: 1).
template <int N, typename MT, typename TB, typename PARK, typename BOUNDS>
MP_HD int mp_cart_span_iterate(const MT& M, const TB& tb, const MpColEdgeParams& P, const double* __restrict__ q0,
                               const double* __restrict__ d0, const double* __restrict__ e0, double nm1, MpCartSpan& S, PARK& park,
                               const BOUNDS& L) {
  double q[N], dq[N], ddq[N];
  mp_ts_hermite<N>(q0, d0, e0, S.u, nm1, q, dq, ddq);
  MpColEdgeEval ev;
  mp_collision_edge_eval<N>(M, tb, q, P.margin, park, L, ev);
  S.steps += 1;
  const double d = ev.dist_world <= ev.dist_self ? ev.dist_world : ev.dist_self;
  if (d < S.clearance) S.clearance = d;
  if (d - P.margin <= P.tol) return 1 + MP_COL_EDGE_BLOCKED;
  if (S.u + ev.tau >= 1.0) { S.u = 1.0; return 1 + MP_COL_EDGE_FREE; }
  if (S.steps >= P.max_steps) return 1 + MP_COL_EDGE_UNDECIDED;
  S.u += ev.tau;
  return 0;
}

MP_HD void mp_cart_span_store(const MpCartWork& W, long e, const MpCartSpan& S) {
  W.sstatus[e] = S.status; W.sevals[e] = S.steps;
  W.t[e] = S.u; W.clearance[e] = S.clearance; W.dpos[e] = S.dpos; W.drot[e] = S.drot;
}
MP_HD void mp_cart_span_skip(const MpCartWork& W, long e) {
  const double nan = __builtin_nan("");
  W.sstatus[e] = MP_CP_SPAN_SKIPPED; W.sevals[e] = 0;
  W.t[e] = nan; W.clearance[e] = nan; W.dpos[e] = nan; W.drot[e] = nan;
}

// Problem b from its head and its spans' records, walked in order.  Fully tracked: DONE if every span is FREE, else what the first
// span that is not says, `span` = that span and t where its advance stopped; clearance = the smallest and the deviations = the
// largest over all spans, evaluations = their sum.  Otherwise the tracking's status, span -1 and NaN.
MP_HD void mp_cart_reduce(const MpCartWork& W, long b, int grid, const MpCartOut& O) {
  const int track = W.track[b];
  const long e0 = b * (long)(grid - 1);
  const double nan = __builtin_nan("");
  int status = track, span = -1, evals = 0;
  double t = nan, clearance = nan, dpos = nan, drot = nan;
  if (track == MP_CP_DONE) {
    t = 1.0; clearance = __builtin_huge_val(); dpos = 0.0; drot = 0.0;
    for (int i = 0; i < grid - 1; ++i) {
      const int st = W.sstatus[e0 + i];
      if (span < 0 && st != MP_COL_EDGE_FREE) {
        span = i;
        status = st == MP_COL_EDGE_BLOCKED ? MP_CP_BLOCKED : MP_CP_UNDECIDED;
        t = W.t[e0 + i];
      }
      evals += W.sevals[e0 + i];
      clearance = mp_min(clearance, W.clearance[e0 + i]);
      dpos = mp_max(dpos, W.dpos[e0 + i]);
      drot = mp_max(drot, W.drot[e0 + i]);
    }
  }
  if (O.status) O.status[b] = status;
  if (O.reached) O.reached[b] = W.reached[b];
  if (O.span) O.span[b] = span;
  if (O.t) O.t[b] = t;
  if (O.clearance) O.clearance[b] = clearance;
  if (O.deviation_pos) O.deviation_pos[b] = dpos;
  if (O.deviation_rot) O.deviation_rot[b] = drot;
  if (O.pose_error) O.pose_error[b] = W.pose_error[b];
  if (O.iterations) O.iterations[b] = W.iterations[b];
  if (O.evaluations) O.evaluations[b] = evals;
  for (int i = 0; i < grid - 1; ++i) {
    if (O.span_status) O.span_status[e0 + i] = W.sstatus[e0 + i];
    if (O.span_clearance) O.span_clearance[e0 + i] = W.clearance[e0 + i];
  }
}

// One problem on the host, for the CPU twin: tracking, its spans one after the other, the reduction.  q / dq / ddq: whole arrays.
template <int N, int MR, typename MT, typename TB>
void mp_cart_problem_cpu(const MT& M, const TB& tb, const MpCartParams& P, const double* q_start, const double* T_goal, long b,
                         const MpCartWork& W, double* q, double* dq, double* ddq, const MpCartOut& O) {
  const long at = b * (long)P.grid * N;
  MpCartHead H;
  mp_cart_track<N, MR>(M, P, q_start + b * N, T_goal + 16 * b, q + at, dq + at, ddq + at, H);
  mp_cart_head_store(W, b, H);
  const double nm1 = (double)(P.grid - 1);
  for (int i = 0; i < P.grid - 1; ++i) {
    const long e = b * (long)(P.grid - 1) + i;
    if (H.status != MP_CP_DONE) {
      mp_cart_span_skip(W, e);
      continue;
    }
    MpColParkLocal park;
    MpColBoundsLocal<N> L;
    MpCartSpan S;
    const long r = at + (long)i * N;
    mp_cart_span_begin<N, MR>(M, tb.sph, q + r, dq + r, ddq + r, q + at, T_goal + 16 * b, nm1, ((double)i + 0.5) / nm1, S, L);
    int done;
    while (!(done = mp_cart_span_iterate<N>(M, tb, P.edge, q + r, dq + r, ddq + r, nm1, S, park, L))) {}
    S.status = done - 1;
    mp_cart_span_store(W, e, S);
  }
  mp_cart_reduce(W, b, P.grid, O);
}
