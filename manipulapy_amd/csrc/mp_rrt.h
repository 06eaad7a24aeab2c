// Bidirectional RRT-Connect over the sphere collision model, one problem per call (float64, 1..MP_MAX_DOF joints).  Header-only like
// mp_collision.h: the HIP kernel k_rrt_connect (mp_kernels.hip) and the CPU twin (mp_cpu.cpp) instantiate the same templates.  The
// contract - random numbers, nearest, the partial node, the procedure, the outputs - is stated once, in include/manipula_hip.h
// (mp_rrt_connect_*); this is how it is computed.
//
// A problem is a small state machine around the edge check of mp_collision.h, in the style of mp_ik_begin / mp_ik_iterate, so that a
// lane can interleave "take the next problem" with "advance the current one".  S.phase names the edge that is running (START / GOAL:
// the two end-point checks, EXTEND, CONNECT) and S.done is what its last mp_col_edge_iterate returned.  One mp_rrt_trip does the
// selection work the problem is waiting for - book the finished edge (append, partial node), the head of the loop, the sample, the
// nearest search, mp_col_edge_begin, the path - and then exactly one mp_col_edge_iterate.
//
// Tree storage goes through an accessor (TREE): nodes get / put (tree, node, joint), parents parent / set_parent (tree, node), and
// the two wave-wide questions of the kernel, wave_max and wave_any, which are the identity on the host.  The nearest search is
// called by EVERY lane of the wave on every trip - with a count of 0 by the lanes that are not searching - and loops to the wave's
// largest count under a per-lane predicate: in the kernel's [tree][node][dim][lane] layout the wave then reads whole 512-byte lines.
// The target of an extension is written to the tree's next free slot BEFORE its edge runs (the slot exists: the head of the loop
// has checked both counts) and is kept by raising the count, so the state carries no second configuration.
#pragma once

#include "mp_collision.h"

constexpr int MP_RRT_SOLVED = 0, MP_RRT_EXHAUSTED = 1, MP_RRT_TREE_FULL = 2, MP_RRT_START_BLOCKED = 3, MP_RRT_GOAL_BLOCKED = 4,
              MP_RRT_PATH_TOO_LONG = 5, MP_RRT_INVALID = -1;  // = MP_PLAN_*
constexpr int MP_RRT_MAX_NODES = 65536;

struct MpRrtParams {
  double lo[MP_MAX_DOF], hi[MP_MAX_DOF];  // the sampling box
  double step, min_advance;
  MpColEdgeParams edge;
  unsigned seed;
  int max_iters, max_nodes, max_waypoints;
};
// the per-problem outputs of a call, any of them null
struct MpRrtOut {
  int *status, *count;
  double* waypoints;  // (B, max_waypoints, n): written while the problem runs (mp_rrt_begin, mp_rrt_trip)
  int* iterations;
  int* nodes;         // (B, 2)
  int* evaluations;
};

// the twin's trees: nodes [tree][node][dim], parents [tree][node]
struct MpRrtTreeLocal : MpWaveOpsSerial {
  double* nodes;
  int* parents;
  int max_nodes, n;
  MP_HD double get(int tree, int v, int j) const { return nodes[((long)tree * max_nodes + v) * n + j]; }
  MP_HD void put(int tree, int v, int j, double x) { nodes[((long)tree * max_nodes + v) * n + j] = x; }
  MP_HD int parent(int tree, int v) const { return parents[(long)tree * max_nodes + v]; }
  MP_HD void set_parent(int tree, int v, int p) { parents[(long)tree * max_nodes + v] = p; }
};

constexpr int MP_RRT_IDLE = 0, MP_RRT_START = 1, MP_RRT_GOAL = 2, MP_RRT_EXTEND = 3, MP_RRT_CONNECT = 4, MP_RRT_TOP = 5,
              MP_RRT_WANT_CONNECT = 6, MP_RRT_SCAN_EXTEND = 7, MP_RRT_SCAN_CONNECT = 8, MP_RRT_FINISHED = 9;

template <int N>
struct MpRrtState {
  MpColEdgeState<N> E;     // the running edge
  unsigned long long key;  // the problem's hash
  double ell;              // the running edge's joint-space length
  int phase, done;
  int k, a, cnt0, cnt1;    // iteration, the active tree, the node counts
  int from, fresh;         // the node the running edge starts at (i / i2); the node the extension appended (new)
  int evals, status, count;
};

// FNV-1a over the bit patterns of q_start then q_goal (the constants of mp_ik_key)
template <int N>
MP_HD unsigned long long mp_rrt_key(const double (&qs)[N], const double (&qg)[N]) {
  unsigned long long h = 0xCBF29CE484222325ull;
#pragma unroll
  for (int j = 0; j < N; ++j) h = (h ^ __builtin_bit_cast(unsigned long long, qs[j])) * 0x100000001B3ull;
#pragma unroll
  for (int j = 0; j < N; ++j) h = (h ^ __builtin_bit_cast(unsigned long long, qg[j])) * 0x100000001B3ull;
  return h;
}

// u(k, j) in [0, 1): one splitmix64 draw (the finaliser of mp_ik_normal)
MP_HD double mp_rrt_uniform(unsigned seed, unsigned long long key, int k, int j) {
  unsigned long long x = (unsigned long long)seed * 0x9E3779B97F4A7C15ull + key * 0xBF58476D1CE4E5B9ull +
                         ((unsigned long long)k * 64ull + (unsigned long long)j) * 0x94D049BB133111EBull;
  x += 0x9E3779B97F4A7C15ull;
  unsigned long long z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// the node of `tree` nearest q among its first `count`: sum over j ascending, of equal d2 the lowest index.  Every lane calls it
// (count = 0: not searching); the loop runs to the wave's largest count.
template <int N, typename TREE>
MP_HD void mp_rrt_nearest(const TREE& T, int tree, int count, const double (&q)[N], int& best, double& best_d2) {
  const int limit = T.wave_max(count);
  best = 0;
  best_d2 = __builtin_huge_val();
  for (int v = 0; v < limit; ++v) {
    if (v < count) {
      double d2 = 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const double diff = T.get(tree, v, j) - q[j];
        d2 += diff * diff;
      }
      if (d2 < best_d2) { best_d2 = d2; best = v; }
    }
  }
}

// the problem has ended: its status and count, and NaN in its waypoints unless the path has been written
template <int N>
MP_HD void mp_rrt_finish(const MpRrtParams& P, MpRrtState<N>& S, int status, int count, double* wp) {
  S.status = status;
  S.count = count;
  S.phase = MP_RRT_FINISHED;
  if (wp != nullptr && status != MP_RRT_SOLVED) {
    const long total = (long)P.max_waypoints * N;
    for (long i = 0; i < total; ++i) wp[i] = __builtin_nan("");
  }
}

// SOLVED: root0 .. p0 of tree 0, then p1 .. root1 of tree 1, padded by repeating the last waypoint
template <int N, typename TREE>
MP_HD void mp_rrt_path(const MpRrtParams& P, MpRrtState<N>& S, const TREE& T, int p0, int p1, double* wp) {
  int d0 = 0, d1 = 0;
  for (int v = T.parent(0, p0); v >= 0; v = T.parent(0, v)) ++d0;
  for (int v = T.parent(1, p1); v >= 0; v = T.parent(1, v)) ++d1;
  const int count = d0 + d1 + 2;
  if (count > P.max_waypoints) {
    mp_rrt_finish<N>(P, S, MP_RRT_PATH_TOO_LONG, count, wp);
    return;
  }
  if (wp != nullptr) {
    int at = d0;
    for (int v = p0; v >= 0; v = T.parent(0, v), --at) {
#pragma unroll
      for (int j = 0; j < N; ++j) wp[(long)at * N + j] = T.get(0, v, j);
    }
    at = d0 + 1;
    for (int v = p1; v >= 0; v = T.parent(1, v), ++at) {
#pragma unroll
      for (int j = 0; j < N; ++j) wp[(long)at * N + j] = T.get(1, v, j);
    }
    for (; at < P.max_waypoints; ++at) {  // (the last waypoint is root1)
#pragma unroll
      for (int j = 0; j < N; ++j) wp[(long)at * N + j] = T.get(1, 0, j);
    }
  }
  mp_rrt_finish<N>(P, S, MP_RRT_SOLVED, count, wp);
}

// A new problem: a non-finite end point ends it at once; otherwise the roots are placed (a lane's workspace is reused by resetting
// the counts only) and the check of q_start is begun.  wp = the problem's waypoint rows, or null.
template <int N, typename MT, typename TB, typename TREE, typename BOUNDS>
MP_HD void mp_rrt_begin(const MT& M, const TB& tb, const MpRrtParams& P, const double (&qs)[N], const double (&qg)[N], MpRrtState<N>& S,
                        TREE& T, BOUNDS& L, double* wp) {
  MpBad<double> bad;
  bad.add(qs);
  bad.add(qg);
  S.key = mp_rrt_key<N>(qs, qg);
  S.ell = 0.0;
  S.done = 0;
  S.k = 0; S.a = 0; S.cnt0 = 0; S.cnt1 = 0; S.from = 0; S.fresh = 0; S.evals = 0;
  if (bad.any()) {
    mp_rrt_finish<N>(P, S, MP_RRT_INVALID, 0, wp);
    return;
  }
#pragma unroll
  for (int j = 0; j < N; ++j) { T.put(0, 0, j, qs[j]); T.put(1, 0, j, qg[j]); }
  T.set_parent(0, 0, -1);
  T.set_parent(1, 0, -1);
  S.cnt0 = 1; S.cnt1 = 1;
  mp_col_edge_begin<N>(M, tb.sph, qs, qs, S.E, L);
  S.phase = MP_RRT_START;
}

// One trip.  Returns 1 when the problem has ended (S.status, S.count, S.k, S.cnt0 / S.cnt1 and S.evals are its outputs, its
// waypoints are written), 0 while it is running - and for an IDLE state, which only takes part in the wave-wide steps.
template <int N, typename MT, typename TB, typename TREE, typename PARK, typename BOUNDS>
MP_HD int mp_rrt_trip(const MT& M, const TB& tb, const MpRrtParams& P, MpRrtState<N>& S, TREE& T, PARK& park, BOUNDS& L, double* wp) {
  for (;;) {
    int scan_tree = 0, scan_count = 0;
    double q[N];
#pragma unroll
    for (int j = 0; j < N; ++j) q[j] = 0.0;
    if (S.done != 0) {  // the running edge has ended
      const bool free = S.done - 1 == MP_COL_EDGE_FREE;
      S.done = 0;
      S.evals += S.E.steps;
      if (S.phase == MP_RRT_START) {
        if (!free) {
          mp_rrt_finish<N>(P, S, MP_RRT_START_BLOCKED, 0, wp);
        } else {
          double g[N];
#pragma unroll
          for (int j = 0; j < N; ++j) g[j] = T.get(1, 0, j);
          mp_col_edge_begin<N>(M, tb.sph, g, g, S.E, L);
          S.phase = MP_RRT_GOAL;
        }
      } else if (S.phase == MP_RRT_GOAL) {
        if (!free) mp_rrt_finish<N>(P, S, MP_RRT_GOAL_BLOCKED, 0, wp);
        else S.phase = MP_RRT_TOP;
      } else if (S.phase == MP_RRT_CONNECT && free) {
        mp_rrt_path<N>(P, S, T, S.a == 0 ? S.fresh : S.from, S.a == 0 ? S.from : S.fresh, wp);
      } else {  // an extension, or a connection that stopped short
        const int tr = S.phase == MP_RRT_EXTEND ? S.a : 1 - S.a;  // the tree the edge grows
        const int at = tr ? S.cnt1 : S.cnt0;
        bool appended = free;  // (EXTEND: the target is in the slot already)
        if (!free) {
          const double half = 0.5 * S.E.t;  // [0, t) is proven
          if (half * S.ell >= P.min_advance) {
#pragma unroll
            for (int j = 0; j < N; ++j) T.put(tr, at, j, S.E.qa[j] + half * S.E.dq[j]);
            appended = true;
          }
        }
        if (appended) {
          T.set_parent(tr, at, S.from);
          S.cnt0 += tr ? 0 : 1;
          S.cnt1 += tr ? 1 : 0;
        }
        if (S.phase == MP_RRT_EXTEND && appended) {
          S.fresh = at;
          S.phase = MP_RRT_WANT_CONNECT;
        } else {  // trapped, or the connection's turn is over
          S.k += 1;
          S.a ^= 1;
          S.phase = MP_RRT_TOP;
        }
      }
    }
    if (S.phase == MP_RRT_TOP) {  // the head of the loop
      if (S.k >= 1 && S.k >= P.max_iters) {
        mp_rrt_finish<N>(P, S, MP_RRT_EXHAUSTED, 0, wp);
      } else if (S.cnt0 == P.max_nodes || S.cnt1 == P.max_nodes) {
        mp_rrt_finish<N>(P, S, MP_RRT_TREE_FULL, 0, wp);
      } else if (S.k == 0) {  // the direct motion first: new = the root
        S.fresh = 0;
        S.phase = MP_RRT_WANT_CONNECT;
      } else {
#pragma unroll
        for (int j = 0; j < N; ++j) q[j] = P.lo[j] + mp_rrt_uniform(P.seed, S.key, S.k, j) * (P.hi[j] - P.lo[j]);
        scan_tree = S.a;
        scan_count = S.a ? S.cnt1 : S.cnt0;
        S.phase = MP_RRT_SCAN_EXTEND;
      }
    }
    if (S.phase == MP_RRT_WANT_CONNECT) {
#pragma unroll
      for (int j = 0; j < N; ++j) q[j] = T.get(S.a, S.fresh, j);
      scan_tree = 1 - S.a;
      scan_count = S.a ? S.cnt0 : S.cnt1;
      S.phase = MP_RRT_SCAN_CONNECT;
    }
    int best;
    double d2;
    mp_rrt_nearest<N>(T, scan_tree, scan_count, q, best, d2);
    if (S.phase == MP_RRT_SCAN_EXTEND) {
      const double d = mp_sqrt(d2);
      if (d == 0.0) {  // trapped on the spot
        S.k += 1;
        S.a ^= 1;
        S.phase = MP_RRT_TOP;
      } else {
        const bool whole = d <= P.step;
        const double s = P.step / d;
        const int at = S.a ? S.cnt1 : S.cnt0;
        double x[N], target[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
          x[j] = T.get(S.a, best, j);
          target[j] = whole ? q[j] : x[j] + s * (q[j] - x[j]);
          T.put(S.a, at, j, target[j]);
        }
        S.ell = whole ? d : P.step;
        S.from = best;
        mp_col_edge_begin<N>(M, tb.sph, x, target, S.E, L);
        S.phase = MP_RRT_EXTEND;
      }
    } else if (S.phase == MP_RRT_SCAN_CONNECT) {
      double y[N];
#pragma unroll
      for (int j = 0; j < N; ++j) y[j] = T.get(1 - S.a, best, j);
      S.ell = mp_sqrt(d2);
      S.from = best;
      mp_col_edge_begin<N>(M, tb.sph, y, q, S.E, L);
      S.phase = MP_RRT_CONNECT;
    }
    if (!T.wave_any(S.phase == MP_RRT_TOP)) break;  // (only after d = 0)
  }
  if (S.phase >= MP_RRT_START && S.phase <= MP_RRT_CONNECT) {
    S.done = mp_col_edge_iterate<N>(M, tb, P.edge, S.E, park, L);
    return 0;
  }
  return S.phase == MP_RRT_FINISHED ? 1 : 0;
}

// the row a finished problem reports, stored by the kernel and the twin alike
template <int N>
MP_HD void mp_rrt_store(const MpRrtOut& O, long row, const MpRrtState<N>& S) {
  if (O.status) O.status[row] = S.status;
  if (O.count) O.count[row] = S.count;
  if (O.iterations) O.iterations[row] = S.k;
  if (O.nodes) { O.nodes[2 * row] = S.cnt0; O.nodes[2 * row + 1] = S.cnt1; }
  if (O.evaluations) O.evaluations[row] = S.evals;
}

// One problem of the C entry over plain host rows, for the CPU twin.  `nodes` / `parents`: 2 max_nodes n doubles / 2 max_nodes ints
// of the calling thread.
template <int N, typename MT, typename TB>
void mp_rrt_cpu(const MT& M, const TB& tb, const MpRrtParams& P, const double* q_start, const double* q_goal, long b, double* nodes,
                int* parents, const MpRrtOut& O) {
  double qs[N], qg[N];
  for (int j = 0; j < N; ++j) { qs[j] = q_start[b * N + j]; qg[j] = q_goal[b * N + j]; }
  MpColParkLocal park;
  MpColBoundsLocal<N> L;
  MpRrtTreeLocal T{{}, nodes, parents, P.max_nodes, N};
  MpRrtState<N> S;
  double* wp = O.waypoints ? O.waypoints + b * (long)P.max_waypoints * N : nullptr;
  mp_rrt_begin<N>(M, tb, P, qs, qg, S, T, L, wp);
  while (!mp_rrt_trip<N>(M, tb, P, S, T, park, L, wp)) {}
  mp_rrt_store<N>(O, b, S);
}
