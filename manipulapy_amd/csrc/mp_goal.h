// Collision-free goal configurations for pose goals over the sphere collision model, one problem per call (float64, 1..MP_MAX_DOF
// joints).  Header-only like mp_rrt.h: the HIP kernel k_goal_ik (mp_kernels.hip) and the CPU twin (mp_cpu.cpp) instantiate the same
// templates.  The contract - the random numbers, the attempts, the step on the hybrid Jacobian, the zero-edge decision, the outputs -
// is stated once, in include/manipula_hip.h (mp_goal_ik_*); this is how it is computed.
//
// A problem is a small state machine in the style of mp_rrt_begin / mp_rrt_trip, so that a lane can interleave "take the next
// problem" with "advance the current one".  One mp_goal_trip does at most one pose evaluation (mp_fk_jac + mp_ik_error) of a problem
// that is iterating, with the damped step that follows it or the start of the next attempt; and, if any lane of the wave has just
// converged (wave_any; the identity on the host), the one collision evaluation of such a lane: mp_col_edge_begin(theta, theta) and one
// mp_col_edge_iterate - a zero edge has no motion, so its single evaluation decides FREE or BLOCKED, and it is the decision the
// planner makes for its q_goal.  The target pose is not part of the state: its 12 entries are re-read from memory on every trip, as
// mp_ik_iterate does.  The seed configuration is read once, by mp_goal_begin, which clamps it into the box and hashes it into the key
// the later attempts draw their start points with; the key is the only thing kept of it.
//
// The state keeps two configurations, the running attempt's theta and the answer so far (`best`: the converged attempt of the
// largest clearance; on FOUND the free one), with the pose error, clearance and witness of the latter.  No workspace.
#pragma once

#include "mp_ik.h"
#include "mp_rrt.h"

constexpr int MP_GIK_FOUND = 0, MP_GIK_IN_COLLISION = 1, MP_GIK_UNREACHED = 2, MP_GIK_INVALID = -1;  // = MP_GOAL_*
constexpr int MP_GOAL_MAX_ATTEMPTS = 65536;

struct MpGoalParams {
  double lo[MP_MAX_DOF], hi[MP_MAX_DOF];  // the box: joint limits of the steps and the range of the restarts
  double eomg, ev, damping, step_cap;
  MpColEdgeParams edge;  // margin, tol; max_steps = 1 (a zero edge is decided by its first evaluation)
  unsigned seed;
  int max_iters, max_attempts;
};
// the per-problem outputs of a call, any of them null
struct MpGoalOut {
  int* status;
  double* q;           // (B, n)
  int *attempts, *iterations, *converged;
  double* pose_error;  // (B, 2)
  double* clearance;
  int* witness;        // (B, 3)
};

constexpr int MP_GOAL_IDLE = 0, MP_GOAL_RUN = 1, MP_GOAL_FINISHED = 2;

template <int N>
struct MpGoalState {
  double theta[N], best[N];   // the running attempt; the answer so far (FINISHED: q)
  unsigned long long key;     // the problem's hash
  double rot, tr, clearance;  // of `best`
  int phase, k, attempt;      // k: the steps of the running attempt
  int iterations, converged, status, witness[3];
};

// FNV-1a over the bit patterns of T_goal[0..12) then q_seed[0..n) (the constants of mp_rrt_key)
template <int N>
MP_HD unsigned long long mp_goal_key(const double (&Tg)[12], const double (&q0)[N]) {
  unsigned long long h = 0xCBF29CE484222325ull;
#pragma unroll
  for (int k = 0; k < 12; ++k) h = (h ^ __builtin_bit_cast(unsigned long long, Tg[k])) * 0x100000001B3ull;
#pragma unroll
  for (int j = 0; j < N; ++j) h = (h ^ __builtin_bit_cast(unsigned long long, q0[j])) * 0x100000001B3ull;
  return h;
}

// the problem has ended; UNREACHED and INVALID have no answer: NaN and -1
template <int N>
MP_HD void mp_goal_finish(MpGoalState<N>& S, int status) {
  S.status = status;
  S.phase = MP_GOAL_FINISHED;
  if (status == MP_GIK_UNREACHED || status == MP_GIK_INVALID) {
    const double nan = __builtin_nan("");
#pragma unroll
    for (int j = 0; j < N; ++j) S.best[j] = nan;
    S.rot = nan; S.tr = nan; S.clearance = nan;
    S.witness[0] = -1; S.witness[1] = -1; S.witness[2] = -1;
  }
}

// the running attempt is over without a free answer: the next one's start point, or the end of the problem
template <int N>
MP_HD void mp_goal_next(const MpGoalParams& P, MpGoalState<N>& S) {
  const int a = S.attempt + 1;
  if (a >= P.max_attempts) {
    mp_goal_finish<N>(S, S.converged > 0 ? MP_GIK_IN_COLLISION : MP_GIK_UNREACHED);
    return;
  }
  S.attempt = a;
  S.k = 0;
#pragma unroll
  for (int j = 0; j < N; ++j) S.theta[j] = P.lo[j] + mp_rrt_uniform(P.seed, S.key, a, j) * (P.hi[j] - P.lo[j]);
}

// A new problem.  Tgp = its 16 doubles (0..11 read), q0p = its seed configuration (n).
template <int N>
MP_HD void mp_goal_begin(const MpGoalParams& P, const double* __restrict__ Tgp, const double* __restrict__ q0p, MpGoalState<N>& S) {
  double Tg[12], q0[N];
#pragma unroll
  for (int k = 0; k < 12; ++k) Tg[k] = Tgp[k];
#pragma unroll
  for (int j = 0; j < N; ++j) q0[j] = q0p[j];
  MpBad<double> bad;
  bad.add(Tg);
  bad.add(q0);
  S.key = mp_goal_key<N>(Tg, q0);
  S.rot = 0.0; S.tr = 0.0;
  S.clearance = -__builtin_huge_val();  // no answer yet: the first converged attempt is strictly better
  S.k = 0; S.attempt = 0; S.iterations = 0; S.converged = 0;
  S.witness[0] = -1; S.witness[1] = -1; S.witness[2] = -1;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    S.theta[j] = q0[j] < P.lo[j] ? P.lo[j] : (q0[j] > P.hi[j] ? P.hi[j] : q0[j]);
    S.best[j] = 0.0;
  }
  if (bad.any()) {
    S.attempt = -1;  // no attempt started
    mp_goal_finish<N>(S, MP_GIK_INVALID);
    return;
  }
  S.phase = MP_GOAL_RUN;
}

// The damped Newton step on the hybrid Jacobian.  J: the space Jacobian of mp_fk_jac at theta (6 x N, rows 0..2 angular); it is
// turned into J_h in place: column i of rows 3..5 becomes v_i + w_i x p_c.  Only the lower triangle of A = J_h J_h^T + damping^2 1
// is formed - mp_spd_solve reads no other entry.
template <int N>
MP_HD void mp_goal_step(const MpGoalParams& P, MpGoalState<N>& S, const double (&Tc)[16], double (&J)[6 * N], double (&e)[6]) {
  const double px = Tc[3], py = Tc[7], pz = Tc[11];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double wx = J[i], wy = J[N + i], wz = J[2 * N + i];
    J[3 * N + i] += wy * pz - wz * py;
    J[4 * N + i] += wz * px - wx * pz;
    J[5 * N + i] += wx * py - wy * px;
  }
  const double lam = P.damping * P.damping;
  double A[6][6];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int c = 0; c <= r; ++c) {
      double s = (r == c) ? lam : 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) s += J[r * N + j] * J[c * N + j];
      A[r][c] = s;
    }
#pragma unroll
    for (int c = r + 1; c < 6; ++c) A[r][c] = 0.0;  // (never read)
  }
  mp_spd_solve<double, 6>(A, e);
  double d[N], nd = 0.0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) s += J[r * N + j] * e[r];
    d[j] = s;
    nd += s * s;
  }
  nd = mp_sqrt(nd);
  const double scale = nd > P.step_cap ? P.step_cap / nd : 1.0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double t = S.theta[j] + d[j] * scale;
    S.theta[j] = t < P.lo[j] ? P.lo[j] : (t > P.hi[j] ? P.hi[j] : t);
  }
  S.k += 1;
  S.iterations += 1;
}

// One trip.  Returns 1 when the problem has ended (S.status, S.best, S.attempt + 1, S.iterations, S.converged, S.rot, S.tr,
// S.clearance and S.witness are its outputs), 0 while it is running - and for an IDLE state, which only takes part in the wave-wide
// step.  W: the wave-wide questions (MpWaveOpsSerial on the host).
template <int N, typename MT, typename TB, typename WAVE, typename PARK, typename BOUNDS>
MP_HD int mp_goal_trip(const MT& M, const TB& tb, const MpGoalParams& P, MpGoalState<N>& S, const WAVE& W, PARK& park, BOUNDS& L,
                       const double* __restrict__ Tgp) {
  bool check = false;
  double rot = 0.0, tr = 0.0;
  if (S.phase == MP_GOAL_RUN) {
    double Td[16];
#pragma unroll
    for (int k = 0; k < 12; ++k) Td[k] = Tgp[k];  // the last row of a pose is never read
    Td[12] = 0.0; Td[13] = 0.0; Td[14] = 0.0; Td[15] = 1.0;
    double Tc[16], J[6 * N], e[6];
    MpIkUnrolled<N>::template fk<true>(M, S.theta, Tc, J);
    mp_ik_error(Tc, Td, e, rot, tr);
    if (rot < P.eomg && tr < P.ev) check = true;                    // converged: the collision evaluation below
    else if (S.k >= P.max_iters) mp_goal_next<N>(P, S);             // the attempt has failed
    else mp_goal_step<N>(P, S, Tc, J, e);
  }
  if (W.wave_any(check)) {
    if (check) {
      MpColEdgeState<N> E;
      mp_col_edge_begin<N>(M, tb.sph, S.theta, S.theta, E, L);
      const int done = mp_col_edge_iterate<N>(M, tb, P.edge, E, park, L);  // a zero edge: FREE or BLOCKED at once
      S.converged += 1;
      const bool free = done - 1 == MP_COL_EDGE_FREE;
      if (free || E.clearance > S.clearance) {  // of equal clearances the first stays
#pragma unroll
        for (int j = 0; j < N; ++j) S.best[j] = S.theta[j];
        S.rot = rot; S.tr = tr; S.clearance = E.clearance;
        S.witness[0] = E.witness[0]; S.witness[1] = E.witness[1]; S.witness[2] = E.witness[2];
      }
      if (free) mp_goal_finish<N>(S, MP_GIK_FOUND);
      else mp_goal_next<N>(P, S);
    }
  }
  return S.phase == MP_GOAL_FINISHED ? 1 : 0;
}

// The row a finished problem reports, stored by the kernel and the twin alike.  q leaves as n plain stores: the twin's rows are not
// 16-byte aligned, so the kernels' vector store (RunIO) is not for both.
template <int N>
MP_HD void mp_goal_store(const MpGoalOut& O, long row, const MpGoalState<N>& S) {
  if (O.status) O.status[row] = S.status;
  if (O.q) {
#pragma unroll
    for (int j = 0; j < N; ++j) O.q[row * N + j] = S.best[j];
  }
  if (O.attempts) O.attempts[row] = S.attempt + 1;
  if (O.iterations) O.iterations[row] = S.iterations;
  if (O.converged) O.converged[row] = S.converged;
  if (O.pose_error) { O.pose_error[2 * row] = S.rot; O.pose_error[2 * row + 1] = S.tr; }
  if (O.clearance) O.clearance[row] = S.clearance;
  if (O.witness) {
#pragma unroll
    for (int k = 0; k < 3; ++k) O.witness[3 * row + k] = S.witness[k];
  }
}

// One problem of the C entry over plain host rows, for the CPU twin.
template <int N, typename MT, typename TB>
void mp_goal_cpu(const MT& M, const TB& tb, const MpGoalParams& P, const double* T_goal, const double* q_seed, long b,
                 const MpGoalOut& O) {
  MpColParkLocal park;
  MpColBoundsLocal<N> L;
  const MpWaveOpsSerial W{};
  MpGoalState<N> S;
  mp_goal_begin<N>(P, T_goal + 16 * b, q_seed + b * N, S);
  while (!mp_goal_trip<N>(M, tb, P, S, W, park, L, T_goal + 16 * b)) {}
  mp_goal_store<N>(O, b, S);
}
