// Stand-alone check of the Cartesian-path CPU twin under AddressSanitizer / UBSan (host code only, no GPU, no Python):
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=float-cast-overflow -fno-sanitize-recover=undefined -pthread \
//       -Imanipulapy_amd/csrc tools/cartesian_sanitize_main.cpp manipulapy_amd/csrc/mp_cpu.cpp manipulapy_amd/csrc/mp_model_compile.cpp \
//       -o cartesian_sanitize
// Exits 0 and prints "ok" when every call behaved as the header says.  (float-cast-overflow is left out for the reason given in
// collision_sanitize_main.cpp.)  Every array is exactly as large as the header says and the grid as small as 2 points, so that the
// sanitizer sees the slots at both ends of the grid arrays, of the span arrays and of the twin's own workspace.
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
  // the 3-joint chain and the world of blend_sanitize_main.cpp: z, y, prismatic x; the position task
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

  // 67 lines: the tool starts on a circle about z and moves by a vector that turns with the problem, so that some lines pass the
  // sphere and the box.  Problem 17 has a NaN in q_start, 18 in T_goal, 40 starts outside the box, 41 has its goal 10 m away, 42 its
  // goal at its start.
  const int B = 67;
  const double margin = 0.01, tol = 1e-3;
  const double lo[3] = {-3.0, -1.2, -0.3}, hi[3] = {3.0, 1.2, 0.3};
  int seen[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // by status, INVALID last
  const int grids[5] = {2, 3, 5, 9, 33};
  for (int run = 0; run < 10; ++run) {
    const int threads = run % 2 ? 4 : 1, N = grids[run / 2], steps = run / 2 == 3 ? 2 : 16;
    std::vector<double> q0((size_t)B * n), Tg((size_t)B * 16, 0.0);
    for (int b = 0; b < B; ++b) {
      double* q = &q0[(size_t)b * n];
      q[0] = -2.4 + 0.07 * b; q[1] = 0.04 * ((b * 3) % 11) - 0.2; q[2] = 0.01 * (b % 9) - 0.04;
      // the start pose of this chain: Rz(q0) Ry(q1), the tool at Rz Ry (0.8 + q2 along x, offset of the y joint at z = 0.3)
      const double c0 = std::cos(q[0]), s0 = std::sin(q[0]), c1 = std::cos(q[1]), s1 = std::sin(q[1]);
      const double r = 0.8 + q[2], px = c1 * r, pz = 0.3 - s1 * r + 0.0;
      double* T = &Tg[(size_t)b * 16];
      T[0] = c0 * c1; T[1] = -s0; T[2] = c0 * s1; T[4] = s0 * c1; T[5] = c0; T[6] = s0 * s1; T[8] = -s1; T[10] = c1; T[15] = 1.0;
      const double a = 0.37 * b;
      T[3] = c0 * px + 0.12 * std::cos(a); T[7] = s0 * px + 0.12 * std::sin(a); T[11] = pz + 0.03 * std::sin(2 * a);
    }
    q0[(size_t)17 * n + 1] = NAN;
    Tg[(size_t)18 * 16 + 7] = NAN;
    for (int j = 0; j < n; ++j) q0[(size_t)40 * n + j] = hi[j] + 0.5;
    Tg[(size_t)41 * 16 + 3] += 10.0;
    std::vector<int32_t> st(B, -7), re(B, -7), sp(B, -7), it(B, -7), ev(B, -7), st2(B, -7), ss((size_t)B * (N - 1), -7);
    std::vector<double> t(B, -7.0), cl(t), dp(t), dr(t), pe(t), sc((size_t)B * (N - 1), -7.0);
    std::vector<double> q((size_t)B * N * n, -7.0), dq(q), ddq(q), q2(q);
    EXPECT(mp_cartesian_path_cpu_f64(model, h, q0.data(), Tg.data(), B, lo, hi, N, MP_TASK_POSITION, 1e-6, 1e-8, 0.01, 20, 0.5, margin, tol,
                                     steps, st.data(), re.data(), sp.data(), t.data(), cl.data(), dp.data(), dr.data(), pe.data(), it.data(),
                                     ev.data(), q.data(), dq.data(), ddq.data(), ss.data(), sc.data(), threads) == MP_OK);
    int here[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < B; ++b) {
      const double* g = &q[(size_t)b * N * n];
      EXPECT(st[b] >= -1 && st[b] <= 6 && re[b] >= 0 && re[b] <= N && it[b] >= 0 && ev[b] >= 0);
      here[st[b] < 0 ? 7 : st[b]] += 1;
      if (b == 17 || b == 18) EXPECT(st[b] == MP_CARTESIAN_INVALID && re[b] == 0 && std::isnan(pe[b]));
      if (b == 40) EXPECT(st[b] == MP_CARTESIAN_LIMIT && re[b] == 0);
      if (b == 41) EXPECT(st[b] == MP_CARTESIAN_LIMIT && re[b] == 1);  // (the prismatic joint reaches it, far outside the box)
      const bool tracked = st[b] == MP_CARTESIAN_DONE || st[b] == MP_CARTESIAN_BLOCKED || st[b] == MP_CARTESIAN_UNDECIDED;
      EXPECT(tracked == (re[b] == N));
      EXPECT((st[b] == MP_CARTESIAN_BLOCKED || st[b] == MP_CARTESIAN_UNDECIDED) == (sp[b] >= 0));
      for (int i = 0; i < N; ++i)
        for (int j = 0; j < n; ++j) {
          const size_t at = ((size_t)b * N + i) * n + j;
          EXPECT((i < re[b]) == std::isfinite(q[at]) && (i < re[b]) == std::isfinite(dq[at]) && (i < re[b]) == std::isfinite(ddq[at]));
        }
      if (re[b] > 0)
        for (int j = 0; j < n; ++j) EXPECT(g[j] == q0[(size_t)b * n + j]);
      for (int i = 0; i < N - 1; ++i) {
        const size_t e = (size_t)b * (N - 1) + i;
        EXPECT(tracked ? (ss[e] >= 0 && ss[e] <= 2 && std::isfinite(sc[e])) : (ss[e] == -1 && std::isnan(sc[e])));
      }
      if (tracked) EXPECT(std::isfinite(t[b]) && std::isfinite(cl[b]) && dp[b] >= 0.0 && dr[b] == 0.0 && ev[b] >= N - 1);
      else EXPECT(std::isnan(t[b]) && std::isnan(cl[b]) && std::isnan(dp[b]) && ev[b] == 0 && sp[b] == -1);
      if (st[b] == MP_CARTESIAN_DONE) EXPECT(t[b] == 1.0 && cl[b] > margin);
    }
    std::printf("N %d, max_steps %d, threads %d: %d done, %d stalled, %d singular, %d limit, %d jump, %d blocked, %d undecided, %d invalid\n", N,
                steps, threads, here[0], here[1], here[2], here[3], here[4], here[5], here[6], here[7]);
    for (int k = 0; k < 8; ++k) seen[k] += here[k];
    // subsets of the outputs - the status without the grid, the grid alone - give the same values
    EXPECT(mp_cartesian_path_cpu_f64(model, h, q0.data(), Tg.data(), B, lo, hi, N, MP_TASK_POSITION, 1e-6, 1e-8, 0.01, 20, 0.5, margin, tol,
                                     steps, st2.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                     nullptr, nullptr, nullptr, nullptr, threads) == MP_OK);
    EXPECT(mp_cartesian_path_cpu_f64(model, h, q0.data(), Tg.data(), B, lo, hi, N, MP_TASK_POSITION, 1e-6, 1e-8, 0.01, 20, 0.5, margin, tol,
                                     steps, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, q2.data(),
                                     nullptr, nullptr, nullptr, nullptr, threads) == MP_OK);
    for (int b = 0; b < B; ++b) EXPECT(st2[b] == st[b]);
    EXPECT(std::memcmp(q.data(), q2.data(), q.size() * sizeof(double)) == 0);
  }
  EXPECT(seen[0] > 0 && seen[3] > 0 && seen[4] > 0 && seen[5] > 0 && seen[6] > 0 && seen[7] > 0);
  // invalid parameters
  std::vector<double> q0((size_t)B * n, 0.0), Tg((size_t)B * 16, 0.0);
  std::vector<int32_t> st(B);
#define CALL(N, TASK, EOMG, EV, DAMP, ITERS, JUMP, MARGIN, TOL, STEPS, OUT)                                                              \
  mp_cartesian_path_cpu_f64(model, h, q0.data(), Tg.data(), B, lo, hi, N, TASK, EOMG, EV, DAMP, ITERS, JUMP, MARGIN, TOL, STEPS, OUT, nullptr, \
                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,    \
                            nullptr, 1)
  EXPECT(CALL(3, 1, 1e-6, 1e-6, 0.01, 20, 0.5, margin, tol, 16, st.data()) == MP_OK);
  EXPECT(CALL(1, 1, 1e-6, 1e-6, 0.01, 20, 0.5, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(65537, 1, 1e-6, 1e-6, 0.01, 20, 0.5, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(3, 2, 1e-6, 1e-6, 0.01, 20, 0.5, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(3, 0, 1e-6, 1e-6, 0.01, 20, 0.5, margin, tol, 16, st.data()) == MP_ERR_UNSUPPORTED);
  EXPECT(CALL(3, 1, 0.0, 1e-6, 0.01, 20, 0.5, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(3, 1, 1e-6, NAN, 0.01, 20, 0.5, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(3, 1, 1e-6, 1e-6, 0.0, 20, 0.5, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(3, 1, 1e-6, 1e-6, 0.01, -1, 0.5, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(3, 1, 1e-6, 1e-6, 0.01, 20, 0.0, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(3, 1, 1e-6, 1e-6, 0.01, 20, 0.5, NAN, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(3, 1, 1e-6, 1e-6, 0.01, 20, 0.5, margin, 0.0, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(3, 1, 1e-6, 1e-6, 0.01, 20, 0.5, margin, tol, 0, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(3, 1, 1e-6, 1e-6, 0.01, 20, 0.5, margin, tol, 16, nullptr) == MP_ERR_INVALID);
  EXPECT(mp_cartesian_path_workspace_bytes(B, 1) == -MP_ERR_INVALID && mp_cartesian_path_workspace_bytes(B, 17) > 0);
  mp_collision_destroy(h);
  delete model;
  std::printf(fails ? "%d checks failed\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
