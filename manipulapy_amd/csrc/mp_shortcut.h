// Randomised shortcutting of piecewise-linear joint-space paths over the sphere collision model, one problem per call (float64,
// 1..MP_MAX_DOF joints).  Header-only like mp_rrt.h: the HIP kernel k_path_shortcut (mp_kernels.hip) and the CPU twin (mp_cpu.cpp)
// instantiate the same templates.  The contract - lengths, random numbers, locate, the procedure, the outputs - is stated once, in
// include/manipula_hip.h (mp_path_shortcut_*); this is how it is computed.
//
// A problem is a small state machine around the edge check of mp_collision.h, in the style of mp_rrt_begin / mp_rrt_trip.  One
// mp_shortcut_trip does the selection work the problem is waiting for - book the finished edge (splice, recompute the lengths), the
// head of the loop, the two draws, both locates, the gain and room tests, mp_col_edge_begin - and then exactly one
// mp_col_edge_iterate.  Iterations that need no edge are consumed inside the trip until an edge is begun or the problem ends.
//
// Path storage goes through an accessor (PATH): waypoints get / put (waypoint, joint), cumulative lengths len / set_len (waypoint),
// and the two wave-wide questions of the kernel, wave_max and wave_any, which are the identity on the host.  The working path
// belongs to the lane (the thread), not to the problem: a new problem copies its rows in, the finished one writes its row out.  The
// locate scan is called by EVERY lane of the wave on every pass - with a count of 0 by the lanes that are not searching - and loops
// to the wave's largest count under a per-lane predicate: in the kernel's [waypoint][lane] layout the wave then reads whole 512-byte
// lines.  The state carries the running edge and the two segment indices; the two new waypoints of an accepted shortcut are the
// end points of the motion the edge check has proven, qa and qa + dq, so there is no second copy of a configuration.
#pragma once

#include "mp_rrt.h"

constexpr int MP_SC_DONE = 0, MP_SC_STRAIGHT = 1, MP_SC_SKIPPED = 2, MP_SC_INVALID = -1;  // = MP_SHORTCUT_*
constexpr int MP_SC_MAX_WAYPOINTS = 65536;

struct MpShortcutParams {
  MpColEdgeParams edge;
  double min_gain;
  unsigned seed;
  int max_iters, max_waypoints, w_in;  // w_in: the rows of an input path
};
// the per-problem outputs of a call, any of them null
struct MpShortcutOut {
  int *status, *count;
  double* waypoints;  // (B, max_waypoints, n): written while the problem runs (mp_shortcut_begin, mp_shortcut_trip)
  double *length_in, *length_out;
  int *iterations, *accepted, *skipped_full, *evaluations;
};

// the twin's path: waypoints [waypoint][dim], lengths [waypoint]
struct MpShortcutPathLocal : MpWaveOpsSerial {
  double* pts;
  double* cum;
  int n;
  MP_HD double get(int w, int j) const { return pts[(long)w * n + j]; }
  MP_HD void put(int w, int j, double x) { pts[(long)w * n + j] = x; }
  MP_HD double len(int w) const { return cum[w]; }
  MP_HD void set_len(int w, double x) { cum[w] = x; }
};

constexpr int MP_SC_IDLE = 0, MP_SC_EDGE = 1, MP_SC_TOP = 2, MP_SC_SCAN = 3, MP_SC_FINISHED = 4;

template <int N>
struct MpShortcutState {
  MpColEdgeState<N> E;     // the running edge a -> b
  unsigned long long key;  // the problem's hash
  double lam_in;           // the input path's length
  int phase, done;
  int k, m, i, j;          // iteration, the waypoints of the working path, the segments of a and b
  int accepted, skipped_full, evals, status;
};

// c_0 = 0, c_w = c_{w-1} + |p_w - p_{w-1}|, the sum over j ascending
template <int N, typename PATH>
MP_HD void mp_shortcut_lengths(PATH& T, int m) {
  double c = 0.0;
  T.set_len(0, 0.0);
  for (int w = 1; w < m; ++w) {
    double d2 = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const double diff = T.get(w, j) - T.get(w - 1, j);
      d2 += diff * diff;
    }
    c += mp_sqrt(d2);
    T.set_len(w, c);
  }
}

// Both locates in one scan of the lengths: i (j) is the smallest index in 0..m-2 with sa (sb) < c_{i+1}, m - 2 if there is none
// (s = u Lambda with u < 1 stays below Lambda = c_{m-1}, so that needs Lambda = 0); ca / cb are c_i, c_{i+1} of the segments.
// Every lane calls it (m = 0: not searching); the loop runs to the wave's largest m.
template <typename PATH>
MP_HD void mp_shortcut_locate(const PATH& T, int m, double sa, double sb, int& i, int& j, double (&ca)[2], double (&cb)[2]) {
  const int limit = T.wave_max(m);
  i = m - 2;
  j = m - 2;
  ca[0] = 0.0; ca[1] = 0.0; cb[0] = 0.0; cb[1] = 0.0;
  bool fa = false, fb = false;
  double prev = 0.0;
  for (int w = 1; w < limit; ++w) {
    if (w < m) {
      const double c = T.len(w);
      if (!fa && sa < c) { fa = true; i = w - 1; ca[0] = prev; ca[1] = c; }
      if (!fb && sb < c) { fb = true; j = w - 1; cb[0] = prev; cb[1] = c; }
      prev = c;
    }
  }
  if (m >= 2 && !(fa && fb)) {  // the last segment, as the contract says
    const double c0 = T.len(m - 2), c1 = T.len(m - 1);
    if (!fa) { ca[0] = c0; ca[1] = c1; }
    if (!fb) { cb[0] = c0; cb[1] = c1; }
  }
}

// the point at arc length s of segment i = [c0, c1)
template <int N, typename PATH>
MP_HD void mp_shortcut_point(const PATH& T, int i, double s, double c0, double c1, double (&x)[N]) {
  const double lam = (s - c0) / (c1 - c0);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double p = T.get(i, j);
    x[j] = p + lam * (T.get(i + 1, j) - p);
  }
}

// The problem has ended: its status and, for DONE / STRAIGHT, its row - the working path padded by repeating the last waypoint;
// NaN rows otherwise.  wp = the problem's output rows, or null.
template <int N, typename PATH>
MP_HD void mp_shortcut_finish(const MpShortcutParams& P, MpShortcutState<N>& S, const PATH& T, int status, double* wp) {
  S.status = status;
  S.phase = MP_SC_FINISHED;
  const bool path = status == MP_SC_DONE || status == MP_SC_STRAIGHT;
  if (!path) S.m = 0;
  if (wp != nullptr) {
    for (int w = 0; w < P.max_waypoints; ++w) {
      const int from = w < S.m ? w : S.m - 1;
#pragma unroll
      for (int j = 0; j < N; ++j) wp[(long)w * N + j] = path ? T.get(from, j) : __builtin_nan("");
    }
  }
}

// A new problem: its rows are copied into the lane's path and checked, the lengths and the key are made.  rows = the problem's
// w_in input rows, wp = its output rows or null.
template <int N, typename PATH>
MP_HD void mp_shortcut_begin(const MpShortcutParams& P, const double* rows, int count_in, MpShortcutState<N>& S, PATH& T, double* wp) {
  S.key = 0;
  S.lam_in = __builtin_nan("");
  S.done = 0;
  S.k = 0; S.m = 0; S.i = 0; S.j = 0; S.accepted = 0; S.skipped_full = 0; S.evals = 0;
  if (count_in < 2) {
    mp_shortcut_finish<N>(P, S, T, MP_SC_SKIPPED, wp);
    return;
  }
  if (count_in > P.w_in || count_in > P.max_waypoints) {
    mp_shortcut_finish<N>(P, S, T, MP_SC_INVALID, wp);
    return;
  }
  MpBad<double> bad;
  double first[N], last[N];
#pragma unroll
  for (int j = 0; j < N; ++j) { first[j] = 0.0; last[j] = 0.0; }
  for (int w = 0; w < count_in; ++w) {
    double x[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      x[j] = rows[(long)w * N + j];
      T.put(w, j, x[j]);
      if (w == 0) first[j] = x[j];
      last[j] = x[j];
    }
    bad.add(x);
  }
  if (bad.any()) {
    mp_shortcut_finish<N>(P, S, T, MP_SC_INVALID, wp);
    return;
  }
  S.m = count_in;
  S.key = mp_rrt_key<N>(first, last);
  mp_shortcut_lengths<N>(T, S.m);
  S.lam_in = T.len(S.m - 1);
  S.phase = MP_SC_TOP;
}

// The accepted shortcut between segments i < j: p_0 .. p_i, a, a + D, p_{j+1} .. p_{m-1}, in place.  a = qa and a + D = qa + dq
// are the end points of the motion q(t) = qa + t dq that the edge check has proven (D = b - a as mp_col_edge_begin rounded it:
// a + D is b to within an ulp); one addition, so the value does not depend on how the compiler contracts anything.
template <int N, typename PATH>
MP_HD void mp_shortcut_splice(MpShortcutState<N>& S, PATH& T) {
  const int i = S.i, j = S.j, m = S.m;
  const int shift = i - j + 2;  // of the tail p_{j+1} ..: +1, 0 or negative
  if (shift > 0) {
    for (int w = m - 1; w > j; --w) {
#pragma unroll
      for (int d = 0; d < N; ++d) T.put(w + 1, d, T.get(w, d));
    }
  } else if (shift < 0) {
    for (int w = j + 1; w < m; ++w) {
#pragma unroll
      for (int d = 0; d < N; ++d) T.put(w + shift, d, T.get(w, d));
    }
  }
#pragma unroll
  for (int d = 0; d < N; ++d) {
    T.put(i + 1, d, S.E.qa[d]);
    T.put(i + 2, d, S.E.qa[d] + S.E.dq[d]);
  }
  S.m = m + shift;
  mp_shortcut_lengths<N>(T, S.m);
}

// One trip.  Returns 1 when the problem has ended (S.status, S.m, S.k, S.accepted, S.skipped_full, S.evals, S.lam_in and the
// path's last length are its outputs, its row is written), 0 while it is running - and for an IDLE state, which only takes part in
// the wave-wide steps.
template <int N, typename MT, typename TB, typename PATH, typename PARK, typename BOUNDS>
MP_HD int mp_shortcut_trip(const MT& M, const TB& tb, const MpShortcutParams& P, MpShortcutState<N>& S, PATH& T, PARK& park, BOUNDS& L,
                           double* wp) {
  for (;;) {
    int scan = 0;
    double sa = 0.0, sb = 0.0;
    if (S.done != 0) {  // the running edge has ended
      const bool free = S.done - 1 == MP_COL_EDGE_FREE && !S.E.bad;
      S.done = 0;
      S.evals += S.E.steps;
      if (free) {
        mp_shortcut_splice<N>(S, T);
        S.accepted += 1;
      }
      S.k += 1;
      S.phase = MP_SC_TOP;
    }
    if (S.phase == MP_SC_TOP) {  // the head of the loop
      if (S.m == 2 && (S.k < P.max_iters || S.k == 0)) {
        mp_shortcut_finish<N>(P, S, T, MP_SC_STRAIGHT, wp);
      } else if (S.k >= P.max_iters) {
        mp_shortcut_finish<N>(P, S, T, MP_SC_DONE, wp);
      } else {
        const double lam = T.len(S.m - 1);
        const double s0 = mp_rrt_uniform(P.seed, S.key, S.k, 0) * lam, s1 = mp_rrt_uniform(P.seed, S.key, S.k, 1) * lam;
        sa = s0 <= s1 ? s0 : s1;
        sb = s0 <= s1 ? s1 : s0;
        scan = S.m;
        S.phase = MP_SC_SCAN;
      }
    }
    int i, j;
    double ca[2], cb[2];
    mp_shortcut_locate(T, scan, sa, sb, i, j, ca, cb);
    if (S.phase == MP_SC_SCAN) {
      bool edge = false;
      if (i != j) {
        double a[N], b[N];
        mp_shortcut_point<N>(T, i, sa, ca[0], ca[1], a);
        mp_shortcut_point<N>(T, j, sb, cb[0], cb[1], b);
        double d2 = 0.0;
#pragma unroll
        for (int d = 0; d < N; ++d) {
          const double diff = b[d] - a[d];
          d2 += diff * diff;
        }
        const double gain = (sb - sa) - mp_sqrt(d2);
        if (gain > P.min_gain) {
          if (S.m - (j - i) + 2 > P.max_waypoints) {
            S.skipped_full += 1;
          } else {
            mp_col_edge_begin<N>(M, tb.sph, a, b, S.E, L);
            S.i = i; S.j = j;
            edge = true;
          }
        }
      }
      if (edge) {
        S.phase = MP_SC_EDGE;
      } else {
        S.k += 1;
        S.phase = MP_SC_TOP;
      }
    }
    if (!T.wave_any(S.phase == MP_SC_TOP)) break;  // bounded by max_iters: every pass ends a problem, begins an edge or raises k
  }
  if (S.phase == MP_SC_EDGE) {
    S.done = mp_col_edge_iterate<N>(M, tb, P.edge, S.E, park, L);
    return 0;
  }
  return S.phase == MP_SC_FINISHED ? 1 : 0;
}

// the row a finished problem reports, stored by the kernel and the twin alike; T: its working path, which holds the output's length
template <int N, typename PATH>
MP_HD void mp_shortcut_store(const MpShortcutOut& O, long row, const MpShortcutState<N>& S, const PATH& T) {
  if (O.status) O.status[row] = S.status;
  if (O.count) O.count[row] = S.m;
  if (O.length_in) O.length_in[row] = S.lam_in;
  if (O.length_out) O.length_out[row] = S.m > 0 ? T.len(S.m - 1) : __builtin_nan("");
  if (O.iterations) O.iterations[row] = S.k;
  if (O.accepted) O.accepted[row] = S.accepted;
  if (O.skipped_full) O.skipped_full[row] = S.skipped_full;
  if (O.evaluations) O.evaluations[row] = S.evals;
}

// One problem of the C entry over plain host rows, for the CPU twin.  `pts` / `cum`: max_waypoints n / max_waypoints doubles of the
// calling thread.
template <int N, typename MT, typename TB>
void mp_shortcut_cpu(const MT& M, const TB& tb, const MpShortcutParams& P, const double* waypoints_in, const int* count_in, long b,
                     double* pts, double* cum, const MpShortcutOut& O) {
  MpColParkLocal park;
  MpColBoundsLocal<N> L;
  MpShortcutPathLocal T{{}, pts, cum, N};
  MpShortcutState<N> S;
  double* wp = O.waypoints ? O.waypoints + b * (long)P.max_waypoints * N : nullptr;
  mp_shortcut_begin<N>(P, waypoints_in + b * (long)P.w_in * N, count_in[b], S, T, wp);
  while (!mp_shortcut_trip<N>(M, tb, P, S, T, park, L, wp)) {}
  mp_shortcut_store<N>(O, b, S, T);
}
