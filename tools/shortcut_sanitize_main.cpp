// Stand-alone check of the path-shortcutting CPU twin under AddressSanitizer / UBSan (host code only, no GPU, no Python):
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=float-cast-overflow -fno-sanitize-recover=undefined -pthread \
//       -Imanipulapy_amd/csrc tools/shortcut_sanitize_main.cpp manipulapy_amd/csrc/mp_cpu.cpp manipulapy_amd/csrc/mp_model_compile.cpp \
//       -o shortcut_sanitize
// Exits 0 and prints "ok" when every call behaved as the header says.  (float-cast-overflow is left out for the reason given in
// collision_sanitize_main.cpp.)  The paths are as short as 2 and 3 waypoints and the output rows as few as the input's count and 2,
// so that the sanitizer sees the slots at both ends of the working path when a shortcut adds a waypoint, removes some or has no room.
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

  // 67 zigzag paths of `count` waypoints in W_in rows (the last slice of a thread is short); the rows past the count are NaN, so a
  // read past it shows.  Problem 17 has a NaN inside its count, 40 a count of 1, 41 of 0, 42 a count above W_in, 50 a repeated point.
  const int B = 67;
  const double margin = 0.01, tol = 1e-3;
  int seen_total[4] = {0, 0, 0, 0};
  long accepted_total = 0, full_total = 0;
  const int shapes[6][4] = {{2, 2, 2, 30}, {3, 3, 3, 30}, {3, 3, 2, 30}, {5, 8, 5, 60}, {12, 12, 16, 80}, {7, 9, 9, 0}};  // count, W_in, W, max_iters
  for (int run = 0; run < 12; ++run) {
    const int threads = run % 2 ? 4 : 1;
    const int count = shapes[run / 2][0], Win = shapes[run / 2][1], W = shapes[run / 2][2], iters = shapes[run / 2][3];
    std::vector<double> in((size_t)B * Win * n, NAN);
    std::vector<int32_t> cin(B, count);
    for (int b = 0; b < B; ++b)
      for (int w = 0; w < count; ++w) {
        double* q = &in[((size_t)b * Win + w) * n];
        const double s = count > 1 ? (double)w / (count - 1) : 0.0;
        q[0] = -2.4 + 0.03 * b + s * (4.6 - 0.05 * ((b * 5) % 67)) + (w % 2 ? 0.25 : 0.0);
        q[1] = 0.05 * ((b * 3) % 11) - 0.25 + (w % 2 ? 0.2 : -0.1) * (w > 0 && w < count - 1);
        q[2] = 0.01 * (b % 9) - 0.04 + (w % 3 == 1 ? 0.05 : 0.0);
      }
    in[((size_t)17 * Win + (count > 2 ? 1 : 0)) * n + 1] = NAN;
    cin[40] = 1; cin[41] = 0; cin[42] = Win + 1;
    if (count >= 3) std::memcpy(&in[((size_t)50 * Win + 1) * n], &in[((size_t)50 * Win + 2) * n], n * sizeof(double));
    std::vector<int32_t> st(B, -7), cnt(B, -7), it(B, -7), acc(B, -7), full(B, -7), ev(B, -7), st2(B, -7);
    std::vector<double> wp((size_t)B * W * n, -7.0), li(B, -7.0), lo(B, -7.0);
    EXPECT(mp_path_shortcut_cpu_f64(model, h, in.data(), cin.data(), B, Win, 5u, iters, 1e-4, W, margin, tol, 16, st.data(), cnt.data(),
                                    wp.data(), li.data(), lo.data(), it.data(), acc.data(), full.data(), ev.data(), threads) == MP_OK);
    int seen[4] = {0, 0, 0, 0};
    for (int b = 0; b < B; ++b) {
      const double* w = &wp[(size_t)b * W * n];
      const bool off = b == 17 || b == 40 || b == 41 || b == 42 || count > W;
      if (off) {
        EXPECT(st[b] == ((b == 40 || b == 41) ? MP_SHORTCUT_SKIPPED : MP_SHORTCUT_INVALID));
        EXPECT(cnt[b] == 0 && it[b] == 0 && acc[b] == 0 && full[b] == 0 && ev[b] == 0 && std::isnan(w[0]) && std::isnan(w[W * n - 1]) &&
               std::isnan(li[b]) && std::isnan(lo[b]));
        seen[st[b] == MP_SHORTCUT_SKIPPED ? 2 : 3] += 1;
        continue;
      }
      EXPECT(st[b] == MP_SHORTCUT_DONE || st[b] == MP_SHORTCUT_STRAIGHT);
      EXPECT((st[b] == MP_SHORTCUT_STRAIGHT) == (cnt[b] == 2 && (it[b] < iters || it[b] == 0)));
      EXPECT(cnt[b] >= 2 && cnt[b] <= W && it[b] >= 0 && it[b] <= iters && acc[b] >= 0 && full[b] >= 0 && ev[b] >= 0);
      EXPECT(lo[b] <= li[b] && (acc[b] == 0 || lo[b] < li[b]));
      const double* first = &in[(size_t)b * Win * n];
      const double* last = &in[((size_t)b * Win + count - 1) * n];
      for (int j = 0; j < n; ++j)
        EXPECT(w[j] == first[j] && w[(size_t)(cnt[b] - 1) * n + j] == last[j] && w[(size_t)(W - 1) * n + j] == last[j]);
      for (int k = 0; k < W * n; ++k) EXPECT(std::isfinite(w[k]));
      seen[st[b]] += 1;
      accepted_total += acc[b];
      full_total += full[b];
    }
    std::printf("count %d, W_in %d, max_waypoints %d, max_iters %d, threads %d: %d done, %d straight, %d skipped, %d invalid\n", count, Win,
                W, iters, threads, seen[0], seen[1], seen[2], seen[3]);
    for (int k = 0; k < 4; ++k) seen_total[k] += seen[k];
    // a subset of the outputs gives the same statuses
    EXPECT(mp_path_shortcut_cpu_f64(model, h, in.data(), cin.data(), B, Win, 5u, iters, 1e-4, W, margin, tol, 16, st2.data(), nullptr,
                                    nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, threads) == MP_OK);
    for (int b = 0; b < B; ++b) EXPECT(st2[b] == st[b]);
  }
  std::printf("%ld accepted, %ld skipped for room\n", accepted_total, full_total);
  EXPECT(seen_total[0] > 0 && seen_total[1] > 0 && seen_total[2] > 0 && seen_total[3] > 0 && accepted_total > 0 && full_total > 0);
  // invalid parameters
  std::vector<double> in((size_t)B * 4 * n, 0.0);
  std::vector<int32_t> cin(B, 4), st(B);
#define CALL(WIN, ITERS, GAIN, W, MARGIN, TOL, STEPS, OUT) \
  mp_path_shortcut_cpu_f64(model, h, in.data(), cin.data(), B, WIN, 1u, ITERS, GAIN, W, MARGIN, TOL, STEPS, OUT, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1)
  EXPECT(CALL(4, 10, 0.0, 4, margin, tol, 16, st.data()) == MP_OK);
  EXPECT(CALL(0, 10, 0.0, 4, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, -1, 0.0, 4, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 10, -1.0, 4, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 10, NAN, 4, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 10, 0.0, 1, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 10, 0.0, 65537, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 10, 0.0, 4, NAN, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 10, 0.0, 4, margin, 0.0, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 10, 0.0, 4, margin, tol, 0, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 10, 0.0, 4, margin, tol, 16, nullptr) == MP_ERR_INVALID);
  EXPECT(mp_path_shortcut_cpu_f64(model, h, in.data(), cin.data(), 0, 4, 1u, 10, 0.0, 4, margin, tol, 16, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, nullptr, 1) == MP_OK);
  EXPECT(mp_path_shortcut_workspace_bytes(3, 8, 2) == 2 * 64 * 8 * 32 && mp_path_shortcut_workspace_bytes(9, 8, 2) == -MP_ERR_UNSUPPORTED &&
         mp_path_shortcut_workspace_bytes(3, 1, 2) == -MP_ERR_INVALID && mp_path_shortcut_workspace_bytes(3, 8, 0) == -MP_ERR_INVALID);
  mp_collision_destroy(h);
  delete model;
  std::printf(fails ? "%d checks failed\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
