// Stand-alone check of the RRT-Connect CPU twin under AddressSanitizer / UBSan (host code only, no GPU, no Python):
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=float-cast-overflow -fno-sanitize-recover=undefined -pthread \
//       -Imanipulapy_amd/csrc tools/rrt_sanitize_main.cpp manipulapy_amd/csrc/mp_cpu.cpp manipulapy_amd/csrc/mp_model_compile.cpp \
//       -o rrt_sanitize
// Exits 0 and prints "ok" when every call behaved as the header says.  (float-cast-overflow is left out for the reason given in
// collision_sanitize_main.cpp.)  The trees are the smallest the entry takes (max_nodes 2 .. 24) so that the sanitizer sees the
// slots at both ends of them, and the waypoint rows are as short as 2.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/manipula_hip.h"
#include "../manipulapy_amd/csrc/mp_handles.h"
#include "../manipulapy_amd/csrc/mp_model_compile.h"

static char g_msg[512];
int mp_set_error(int code, const char* msg) { std::snprintf(g_msg, sizeof g_msg, "%s", msg); return code; }

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, g_msg); ++fails; } } while (0)

int main() {
  // a 3-joint chain: z, y, prismatic x (the chain of collision_edges_sanitize_main.cpp)
  const int n = 3;
  double S[6 * n] = {0, 0, 0,   0, 1, 0,   1, 0, 0,   0, -0.3, 1,   0, 0, 0,   0, 0.3, 0};  // (6, n) row-major
  double Mcom[n * 16], G[n * 36], Mee[16];
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < 16; ++k) Mcom[16 * i + k] = (k % 5 == 0) ? 1.0 : 0.0;
    Mcom[16 * i + 3] = 0.2 * (i + 1);
    for (int k = 0; k < 36; ++k) G[36 * i + k] = (k % 7 == 0) ? 1.0 : 0.0;
  }
  for (int k = 0; k < 16; ++k) Mee[k] = (k % 5 == 0) ? 1.0 : 0.0;
  Mee[3] = 0.8;
  mp_model* model = new mp_model;
  char msg[400] = "";
  std::memset(model->pmap, 0, sizeof model->pmap);
  EXPECT(mp_compile_model(n, S, Mcom, G, Mee, nullptr, nullptr, &model->d, msg, sizeof msg, model->pmap) == 0);
  model->uid = 1;

  // four spheres along the arm, none on the base, no pairs; three obstacles around it
  int32_t link[4] = {1, 2, 3, 3};
  double centre[12] = {0.1, 0, 0.3,   0.3, 0, 0.3,   0.55, 0, 0.3,   0.75, 0, 0.3}, radius[4] = {0.05, 0.05, 0.04, 0.04};
  mp_collision* h = nullptr;
  EXPECT(mp_collision_create(model, 4, link, centre, radius, 0, nullptr, &h) == MP_OK);
  int32_t kind[3] = {MP_OBSTACLE_SPHERE, MP_OBSTACLE_CAPSULE, MP_OBSTACLE_BOX};
  double prm[3 * 16] = {};
  double* p = prm;
  p[0] = 0.5; p[1] = 0.45; p[2] = 0.3; p[3] = 0.15; p += 16;
  p[0] = -0.5; p[1] = 0.3; p[2] = 0.0; p[3] = -0.5; p[4] = 0.3; p[5] = 0.8; p[6] = 0.06; p += 16;
  p[0] = 0.3; p[1] = -0.6; p[2] = 0.3; p[3] = 1; p[7] = 1; p[11] = 1; p[12] = 0.1; p[13] = 0.1; p[14] = 0.4;
  EXPECT(mp_collision_pack_world("main", 3, kind, prm, &h->world) == MP_OK && h->world.size() == 3);

  // 67 problems (the last slice of a thread is short): starts and goals on both sides of the obstacles, a NaN and an inf row
  const int B = 67;
  const double lo[n] = {-2.5, -0.6, -0.2}, hi[n] = {2.5, 0.6, 0.2};
  std::vector<double> qs(B * n), qg(B * n);
  for (int b = 0; b < B; ++b) {
    qs[b * n] = -2.4 + 0.07 * b; qs[b * n + 1] = 0.05 * ((b * 3) % 11) - 0.25; qs[b * n + 2] = 0.01 * (b % 9) - 0.04;
    qg[b * n] = 2.4 - 0.05 * ((b * 5) % 67); qg[b * n + 1] = 0.04 * ((b * 7) % 13) - 0.24; qg[b * n + 2] = 0.02 * (b % 5) - 0.04;
  }
  qs[17 * n + 1] = NAN;
  qg[40 * n + 2] = INFINITY;
  const double margin = 0.01, tol = 1e-3;
  int seen_total[7] = {0, 0, 0, 0, 0, 0, 0};
  const int sizes[5][3] = {{24, 12, 60}, {2, 2, 40}, {24, 2, 60}, {8, 3, 25}, {24, 30, 0}};  // max_nodes, max_waypoints, max_iters
  for (int run = 0; run < 10; ++run) {
    const int threads = run % 2 ? 4 : 1;
    const int max_nodes = sizes[run / 2][0], W = sizes[run / 2][1], iters = sizes[run / 2][2];
    std::vector<int32_t> st(B, -7), cnt(B, -7), it(B, -7), nd(2 * B, -7), ev(B, -7), st2(B, -7);
    std::vector<double> wp((size_t)B * W * n, -7.0);
    EXPECT(mp_rrt_connect_cpu_f64(model, h, qs.data(), qg.data(), B, lo, hi, 5u, 0.8, 0.1, iters, max_nodes, W, margin, tol, 16,
                                  st.data(), cnt.data(), wp.data(), it.data(), nd.data(), ev.data(), threads) == MP_OK);
    int seen[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < B; ++b) {
      const double* w = &wp[(size_t)b * W * n];
      if (b == 17 || b == 40) {
        EXPECT(st[b] == MP_PLAN_INVALID && cnt[b] == 0 && it[b] == 0 && nd[2 * b] == 0 && nd[2 * b + 1] == 0 && ev[b] == 0 && std::isnan(w[0]));
        continue;
      }
      EXPECT(st[b] >= 0 && st[b] <= 5 && it[b] >= 0 && it[b] <= (iters > 1 ? iters : 1) && ev[b] >= 1);
      EXPECT(nd[2 * b] >= 1 && nd[2 * b] <= max_nodes && nd[2 * b + 1] >= 1 && nd[2 * b + 1] <= max_nodes);
      seen[st[b]] += 1;
      if (st[b] == MP_PLAN_SOLVED) {
        EXPECT(cnt[b] >= 2 && cnt[b] <= W);
        for (int j = 0; j < n; ++j) EXPECT(w[j] == qs[b * n + j] && w[(size_t)(cnt[b] - 1) * n + j] == qg[b * n + j] && w[(size_t)(W - 1) * n + j] == qg[b * n + j]);
        for (int k = 0; k < W * n; ++k) EXPECT(std::isfinite(w[k]));
      } else {
        EXPECT(std::isnan(w[0]) && std::isnan(w[W * n - 1]));
        EXPECT(st[b] == MP_PLAN_PATH_TOO_LONG ? cnt[b] > W : cnt[b] == 0);
      }
      if (st[b] == MP_PLAN_TREE_FULL) EXPECT(nd[2 * b] == max_nodes || nd[2 * b + 1] == max_nodes);
    }
    std::printf("max_nodes %d, max_waypoints %d, max_iters %d, threads %d: %d solved, %d exhausted, %d full, %d + %d blocked, %d too long\n",
                max_nodes, W, iters, threads, seen[0], seen[1], seen[2], seen[3], seen[4], seen[5]);
    for (int k = 0; k < 6; ++k) seen_total[k] += seen[k];
    // a subset of the outputs gives the same statuses
    EXPECT(mp_rrt_connect_cpu_f64(model, h, qs.data(), qg.data(), B, lo, hi, 5u, 0.8, 0.1, iters, max_nodes, W, margin, tol, 16,
                                  st2.data(), nullptr, nullptr, nullptr, nullptr, nullptr, threads) == MP_OK);
    for (int b = 0; b < B; ++b) EXPECT(st2[b] == st[b]);
  }
  EXPECT(seen_total[MP_PLAN_SOLVED] > 0 && seen_total[MP_PLAN_TREE_FULL] > 0 && seen_total[MP_PLAN_EXHAUSTED] > 0 &&
         seen_total[MP_PLAN_PATH_TOO_LONG] > 0);
  // a degenerate box (every sample the same point) and min_advance 0
  {
    std::vector<int32_t> st(B);
    const double mid[n] = {0.3, 0.1, 0.0};
    EXPECT(mp_rrt_connect_cpu_f64(model, h, qs.data(), qg.data(), B, mid, mid, 1u, 0.8, 0.0, 20, 8, 4, margin, tol, 16, st.data(), nullptr,
                                  nullptr, nullptr, nullptr, nullptr, 2) == MP_OK);
  }
  // invalid parameters
  std::vector<int32_t> st(B);
  const double bad_hi[n] = {2.5, -0.7, 0.2}, open_hi[n] = {2.5, INFINITY, 0.2};
#define CALL(LO, HI, STEP, ADV, ITERS, NODES, W, MARGIN, TOL, STEPS, OUT) \
  mp_rrt_connect_cpu_f64(model, h, qs.data(), qg.data(), B, LO, HI, 1u, STEP, ADV, ITERS, NODES, W, MARGIN, TOL, STEPS, OUT, nullptr, nullptr, nullptr, nullptr, nullptr, 1)
  EXPECT(CALL(lo, bad_hi, 0.8, 0.1, 10, 8, 4, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, open_hi, 0.8, 0.1, 10, 8, 4, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(nullptr, hi, 0.8, 0.1, 10, 8, 4, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, hi, 0.0, 0.1, 10, 8, 4, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, hi, 0.8, -0.1, 10, 8, 4, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, hi, 0.8, 0.1, -1, 8, 4, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, hi, 0.8, 0.1, 10, 1, 4, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, hi, 0.8, 0.1, 10, 65537, 4, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, hi, 0.8, 0.1, 10, 8, 1, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, hi, 0.8, 0.1, 10, 8, 4, NAN, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, hi, 0.8, 0.1, 10, 8, 4, margin, 0.0, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, hi, 0.8, 0.1, 10, 8, 4, margin, tol, 0, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, hi, 0.8, 0.1, 10, 8, 4, margin, tol, 16, nullptr) == MP_ERR_INVALID);
  EXPECT(mp_rrt_connect_cpu_f64(model, h, qs.data(), qg.data(), 0, lo, hi, 1u, 0.8, 0.1, 10, 8, 4, margin, tol, 16, nullptr, nullptr, nullptr,
                                nullptr, nullptr, nullptr, 1) == MP_OK);
  EXPECT(mp_rrt_connect_workspace_bytes(3, 8, 2) == 2 * 64 * 2 * 8 * 28 && mp_rrt_connect_workspace_bytes(9, 8, 2) == -MP_ERR_UNSUPPORTED &&
         mp_rrt_connect_workspace_bytes(3, 1, 2) == -MP_ERR_INVALID && mp_rrt_connect_workspace_bytes(3, 8, 0) == -MP_ERR_INVALID);
  mp_collision_destroy(h);
  delete model;
  std::printf(fails ? "%d checks failed\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
