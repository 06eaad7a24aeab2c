// Stand-alone check of the goal-configuration CPU twin under AddressSanitizer / UBSan (host code only, no GPU, no Python):
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=float-cast-overflow -fno-sanitize-recover=undefined -pthread \
//       -Imanipulapy_amd/csrc tools/goal_sanitize_main.cpp manipulapy_amd/csrc/mp_cpu.cpp manipulapy_amd/csrc/mp_model_compile.cpp \
//       -o goal_sanitize
// Exits 0 and prints "ok" when every call behaved as the header says.  (float-cast-overflow is left out for the reason given in
// collision_sanitize_main.cpp.)  The batch sizes end a thread's slice short, every output is followed by a canary, and the runs go
// down to max_iters = 0 and max_attempts = 1, so that the sanitizer sees the first and the last row of every output array.
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
  // the 3-joint chain and the world of rrt_sanitize_main.cpp: z, y, prismatic x
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

  // B poses: the forward kinematics of configurations swept through the box, seeds swept the other way.  Problem 5 has a NaN in
  // its pose, 9 an infinity in its seed, 11 is out of reach, 13 is seeded with its own solution, 15 from outside the box; the last
  // row of every pose is NaN (it is never read).
  const double lo[n] = {-2.5, -1.2, -0.3}, hi[n] = {2.5, 1.2, 0.3};
  const double margin = 0.01, tol = 1e-3, CANARY = -7.0;
  int seen_total[4] = {0, 0, 0, 0};
  const int shapes[5][3] = {{67, 30, 4}, {67, 0, 1}, {1, 30, 2}, {64, 5, 3}, {65, 30, 1}};  // B, max_iters, max_attempts
  for (int run = 0; run < 10; ++run) {
    const int threads = run % 2 ? 4 : 1;
    const int B = shapes[run / 2][0], iters = shapes[run / 2][1], attempts = shapes[run / 2][2];
    std::vector<double> Tg((size_t)B * 16), q0((size_t)B * n), qt((size_t)B * n);
    for (int b = 0; b < B; ++b) {
      for (int j = 0; j < n; ++j) {
        const double s = ((b * (3 + 2 * j)) % 17) / 16.0, r = ((b * (5 + j)) % 13) / 12.0;
        qt[(size_t)b * n + j] = lo[j] + s * (hi[j] - lo[j]);
        q0[(size_t)b * n + j] = hi[j] - r * (hi[j] - lo[j]);
      }
      double theta[n], Tc[16], J[6 * n];
      for (int j = 0; j < n; ++j) theta[j] = qt[(size_t)b * n + j];
      MpIkUnrolled<n>::fk<false>(model->d, theta, Tc, J);
      for (int k = 0; k < 12; ++k) Tg[(size_t)b * 16 + k] = Tc[k];
      for (int k = 12; k < 16; ++k) Tg[(size_t)b * 16 + k] = NAN;
    }
    if (B > 15) {
      Tg[5 * 16 + 6] = NAN;
      q0[9 * n + 2] = INFINITY;
      Tg[11 * 16 + 3] += 10.0;
      for (int j = 0; j < n; ++j) { q0[13 * n + j] = qt[13 * n + j]; q0[15 * n + j] = hi[j] + 0.5; }
    }
    std::vector<int32_t> st(B + 1, -7), att(B + 1, -7), it(B + 1, -7), cv(B + 1, -7), wit(3 * B + 1, -7), st2(B + 1, -7);
    std::vector<double> q((size_t)B * n + 1, CANARY), pe(2 * B + 1, CANARY), cl(B + 1, CANARY);
    EXPECT(mp_goal_ik_cpu_f64(model, h, Tg.data(), q0.data(), B, lo, hi, 5u, 1e-6, 1e-6, 0.02, 0.5, iters, attempts, margin, tol, st.data(),
                              q.data(), att.data(), it.data(), cv.data(), pe.data(), cl.data(), wit.data(), threads) == MP_OK);
    EXPECT(st[B] == -7 && att[B] == -7 && it[B] == -7 && cv[B] == -7 && wit[3 * B] == -7 && q[(size_t)B * n] == CANARY &&
           pe[2 * B] == CANARY && cl[B] == CANARY);
    int seen[4] = {0, 0, 0, 0};
    for (int b = 0; b < B; ++b) {
      const bool bad = B > 15 && (b == 5 || b == 9);
      if (bad || st[b] == MP_GOAL_UNREACHED) {
        EXPECT(st[b] == (bad ? MP_GOAL_INVALID : MP_GOAL_UNREACHED));
        EXPECT(std::isnan(q[(size_t)b * n]) && std::isnan(q[(size_t)b * n + n - 1]) && std::isnan(pe[2 * b]) && std::isnan(pe[2 * b + 1]) &&
               std::isnan(cl[b]) && wit[3 * b] == -1 && wit[3 * b + 2] == -1 && cv[b] == 0);
        EXPECT(bad ? (att[b] == 0 && it[b] == 0) : (att[b] == attempts && it[b] == attempts * iters));
        seen[bad ? 3 : 2] += 1;
        continue;
      }
      EXPECT(st[b] == MP_GOAL_FOUND || st[b] == MP_GOAL_IN_COLLISION);
      EXPECT(att[b] >= 1 && att[b] <= attempts && it[b] >= 0 && it[b] <= attempts * iters && cv[b] >= 1 && cv[b] <= att[b]);
      EXPECT((st[b] == MP_GOAL_FOUND) == (cl[b] - margin > tol) && (st[b] == MP_GOAL_FOUND || att[b] == attempts));
      EXPECT(pe[2 * b] < 1e-6 && pe[2 * b + 1] < 1e-6 && pe[2 * b] >= 0.0 && wit[3 * b] >= 0 && wit[3 * b] <= 1);
      for (int j = 0; j < n; ++j) EXPECT(q[(size_t)b * n + j] >= lo[j] && q[(size_t)b * n + j] <= hi[j]);
      seen[st[b]] += 1;
    }
    if (B > 15) {
      EXPECT(st[11] == MP_GOAL_UNREACHED);
      EXPECT(it[13] == 0 && att[13] == 1 && cv[13] == 1);
      for (int j = 0; j < n; ++j) EXPECT(q[13 * n + j] == qt[13 * n + j]);
    }
    std::printf("B %d, max_iters %d, max_attempts %d, threads %d: %d found, %d in collision, %d unreached, %d invalid\n", B, iters, attempts,
                threads, seen[0], seen[1], seen[2], seen[3]);
    for (int k = 0; k < 4; ++k) seen_total[k] += seen[k];
    // a subset of the outputs gives the same statuses
    EXPECT(mp_goal_ik_cpu_f64(model, h, Tg.data(), q0.data(), B, lo, hi, 5u, 1e-6, 1e-6, 0.02, 0.5, iters, attempts, margin, tol, st2.data(),
                              nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, threads) == MP_OK);
    for (int b = 0; b <= B; ++b) EXPECT(st2[b] == st[b]);
  }
  EXPECT(seen_total[0] > 0 && seen_total[1] > 0 && seen_total[2] > 0 && seen_total[3] > 0);
  // invalid parameters
  const int B = 4;
  std::vector<double> Tg((size_t)B * 16, 0.0), q0((size_t)B * n, 0.0);
  std::vector<int32_t> st(B);
  const double nolo[n] = {-2.5, 1.3, -0.3};
#define CALL(LO, EOMG, EV, DAMP, CAP, ITERS, ATT, MARGIN, TOL, OUT) \
  mp_goal_ik_cpu_f64(model, h, Tg.data(), q0.data(), B, LO, hi, 1u, EOMG, EV, DAMP, CAP, ITERS, ATT, MARGIN, TOL, OUT, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1)
  EXPECT(CALL(lo, 1e-6, 1e-6, 0.02, 0.5, 10, 2, margin, tol, st.data()) == MP_OK);
  EXPECT(CALL(nolo, 1e-6, 1e-6, 0.02, 0.5, 10, 2, margin, tol, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(nullptr, 1e-6, 1e-6, 0.02, 0.5, 10, 2, margin, tol, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, 0.0, 1e-6, 0.02, 0.5, 10, 2, margin, tol, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, 1e-6, NAN, 0.02, 0.5, 10, 2, margin, tol, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, 1e-6, 1e-6, 0.0, 0.5, 10, 2, margin, tol, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, 1e-6, 1e-6, 0.02, INFINITY, 10, 2, margin, tol, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, 1e-6, 1e-6, 0.02, 0.5, -1, 2, margin, tol, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, 1e-6, 1e-6, 0.02, 0.5, 10, 0, margin, tol, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, 1e-6, 1e-6, 0.02, 0.5, 10, 65537, margin, tol, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, 1e-6, 1e-6, 0.02, 0.5, 10, 2, NAN, tol, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, 1e-6, 1e-6, 0.02, 0.5, 10, 2, margin, 0.0, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(lo, 1e-6, 1e-6, 0.02, 0.5, 10, 2, margin, tol, nullptr) == MP_ERR_INVALID);
  EXPECT(mp_goal_ik_cpu_f64(model, h, nullptr, nullptr, 0, lo, hi, 1u, 1e-6, 1e-6, 0.02, 0.5, 10, 2, margin, tol, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr, nullptr, nullptr, 1) == MP_OK);
  mp_collision_destroy(h);
  delete model;
  std::printf(fails ? "%d checks failed\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
