// Stand-alone check of the corner-blending CPU twin under AddressSanitizer / UBSan (host code only, no GPU, no Python):
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=float-cast-overflow -fno-sanitize-recover=undefined -pthread \
//       -Imanipulapy_amd/csrc tools/blend_sanitize_main.cpp manipulapy_amd/csrc/mp_cpu.cpp manipulapy_amd/csrc/mp_model_compile.cpp \
//       -o blend_sanitize
// Exits 0 and prints "ok" when every call behaved as the header says.  (float-cast-overflow is left out for the reason given in
// collision_sanitize_main.cpp.)  Every array is exactly as large as the header says, the input rows as few as the path's count and
// the grid as small as 3 points, so that the sanitizer sees the slots at both ends of points, cut, knot and of the grid arrays.
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
  // the 3-joint chain and the world of shortcut_sanitize_main.cpp: z, y, prismatic x
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

  // 67 zigzag paths of `count` waypoints in W_in rows; the rows past the count are NaN, so a read past it shows.  Problem 17 has a NaN
  // inside its count, 40 a count of 1, 41 of 0, 42 a count above W_in, 50 a repeated point, 51 all points equal, 52 doubles back.
  const int B = 67;
  const double margin = 0.01, tol = 1e-3;
  int seen[7] = {0, 0, 0, 0, 0, 0, 0};  // by status, INVALID last
  long halvings_total = 0;
  const int shapes[5][4] = {{2, 2, 3, 0}, {3, 3, 3, 2}, {3, 5, 4, 0}, {6, 6, 9, 6}, {12, 16, 33, 3}};  // count, W_in, N, max_halvings
  for (int run = 0; run < 10; ++run) {
    const int threads = run % 2 ? 4 : 1;
    const int count = shapes[run / 2][0], Win = shapes[run / 2][1], N = shapes[run / 2][2], halv = shapes[run / 2][3];
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
    if (count >= 3) {
      std::memcpy(&in[((size_t)50 * Win + 1) * n], &in[((size_t)50 * Win + 2) * n], n * sizeof(double));
      std::memcpy(&in[((size_t)52 * Win + 2) * n], &in[((size_t)52 * Win + 0) * n], n * sizeof(double));
      for (int j = 0; j < n; ++j) in[((size_t)52 * Win + 1) * n + j] = in[(size_t)52 * Win * n + j] + (j == 0 ? 0.25 : 0.0);
    }
    for (int w = 1; w < count; ++w) std::memcpy(&in[((size_t)51 * Win + w) * n], &in[(size_t)51 * Win * n], n * sizeof(double));
    std::vector<int32_t> st(B, -7), co(B, -7), cnt(B, -7), hv(B, -7), ev(B, -7), st2(B, -7);
    std::vector<double> pts((size_t)B * Win * n, -7.0), cut((size_t)B * Win, -7.0), knot((size_t)B * Win, -7.0), len(B, -7.0), cl(B, -7.0);
    std::vector<double> q((size_t)B * N * n, -7.0), dq(q), ddq(q), q2(q);
    EXPECT(mp_path_blend_cpu_f64(model, h, in.data(), cin.data(), B, Win, N, 0.3, halv, margin, tol, 16, st.data(), co.data(), cnt.data(),
                                 pts.data(), cut.data(), knot.data(), len.data(), hv.data(), ev.data(), cl.data(), q.data(), dq.data(),
                                 ddq.data(), threads) == MP_OK);
    int here[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < B; ++b) {
      const bool curve = st[b] == MP_BLEND_DONE || st[b] == MP_BLEND_STRAIGHT || st[b] == MP_BLEND_POINT;
      const double* g = &q[(size_t)b * N * n];
      EXPECT(st[b] >= -1 && st[b] <= 5 && hv[b] >= 0 && ev[b] >= 0);
      here[st[b] < 0 ? 6 : st[b]] += 1;
      halvings_total += hv[b];
      if (b == 17 || b == 42) EXPECT(st[b] == MP_BLEND_INVALID);
      if (b == 40 || b == 41) EXPECT(st[b] == MP_BLEND_SKIPPED);
      if (b == 51) EXPECT(st[b] == MP_BLEND_POINT && cnt[b] == 1 && len[b] == 0.0);
      if (b == 52 && count >= 3) EXPECT(st[b] == MP_BLEND_REVERSAL && co[b] == 1 && ev[b] == 0);
      if (b == 50 && count >= 3 && curve) EXPECT(cnt[b] == count - 1);
      EXPECT((st[b] == MP_BLEND_BLOCKED || st[b] == MP_BLEND_REVERSAL) == (co[b] >= 1));
      if (!curve) {
        EXPECT(cnt[b] == 0 && std::isnan(len[b]) && std::isnan(cl[b]) && std::isnan(g[0]) && std::isnan(g[N * n - 1]) &&
               std::isnan(pts[(size_t)b * Win * n]) && std::isnan(pts[(size_t)(b + 1) * Win * n - 1]) &&
               std::isnan(cut[(size_t)b * Win]) && std::isnan(knot[(size_t)(b + 1) * Win - 1]));
        continue;
      }
      const int m = cnt[b];
      EXPECT(m >= 1 && m <= cin[b] && len[b] >= 0.0 && cut[(size_t)b * Win] == 0.0 && knot[(size_t)b * Win] == 0.0 &&
             knot[(size_t)(b + 1) * Win - 1] == len[b] && cut[(size_t)(b + 1) * Win - 1] == 0.0);
      const double* first = &in[(size_t)b * Win * n];
      const double* last = &in[((size_t)b * Win + cin[b] - 1) * n];
      for (int j = 0; j < n; ++j) EXPECT(g[j] == first[j] && g[(size_t)(N - 1) * n + j] == last[j] && pts[(size_t)(b + 1) * Win * n - n + j] == last[j]);
      for (int k = 0; k < N * n; ++k) EXPECT(std::isfinite(g[k]) && std::isfinite(dq[(size_t)b * N * n + k]) && std::isfinite(ddq[(size_t)b * N * n + k]));
    }
    std::printf("count %d, W_in %d, N %d, max_halvings %d, threads %d: %d done, %d straight, %d skipped, %d point, %d blocked, %d reversal, "
                "%d invalid\n", count, Win, N, halv, threads, here[0], here[1], here[2], here[3], here[4], here[5], here[6]);
    for (int k = 0; k < 7; ++k) seen[k] += here[k];
    // subsets of the outputs - the grid without its tables among them - give the same values
    EXPECT(mp_path_blend_cpu_f64(model, h, in.data(), cin.data(), B, Win, N, 0.3, halv, margin, tol, 16, st2.data(), nullptr, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, threads) == MP_OK);
    EXPECT(mp_path_blend_cpu_f64(model, h, in.data(), cin.data(), B, Win, N, 0.3, halv, margin, tol, 16, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, q2.data(), nullptr, nullptr, threads) == MP_OK);
    for (int b = 0; b < B; ++b) EXPECT(st2[b] == st[b]);
    EXPECT(std::memcmp(q.data(), q2.data(), q.size() * sizeof(double)) == 0);
  }
  std::printf("%ld failed attempts\n", halvings_total);
  for (int k = 0; k < 7; ++k) EXPECT(seen[k] > 0);
  EXPECT(halvings_total > 0);
  // invalid parameters
  std::vector<double> in((size_t)B * 4 * n, 0.0);
  std::vector<int32_t> cin(B, 4), st(B);
#define CALL(WIN, N, BLEND, HALV, MARGIN, TOL, STEPS, OUT) \
  mp_path_blend_cpu_f64(model, h, in.data(), cin.data(), B, WIN, N, BLEND, HALV, MARGIN, TOL, STEPS, OUT, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1)
  EXPECT(CALL(4, 3, 0.5, 6, margin, tol, 16, st.data()) == MP_OK);
  EXPECT(CALL(0, 3, 0.5, 6, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(65537, 3, 0.5, 6, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 2, 0.5, 6, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 65537, 0.5, 6, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 3, 0.0, 6, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 3, NAN, 6, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 3, 0.5, -1, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 3, 0.5, 33, margin, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 3, 0.5, 6, NAN, tol, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 3, 0.5, 6, margin, 0.0, 16, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 3, 0.5, 6, margin, tol, 0, st.data()) == MP_ERR_INVALID);
  EXPECT(CALL(4, 3, 0.5, 6, margin, tol, 16, nullptr) == MP_ERR_INVALID);
  mp_collision_destroy(h);
  delete model;
  std::printf(fails ? "%d checks failed\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
