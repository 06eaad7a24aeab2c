// Stand-alone check of the collision tables' validation and of the CPU twin under AddressSanitizer / UBSan (host code only, no GPU, no
// Python):
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=float-cast-overflow -fno-sanitize-recover=undefined -pthread \
//       -Imanipulapy_amd/csrc tools/collision_sanitize_main.cpp manipulapy_amd/csrc/mp_cpu.cpp manipulapy_amd/csrc/mp_model_compile.cpp -o collision_sanitize
// Exits 0 and prints "ok" when every call behaved as the header says.  (float-cast-overflow is left out: mp_sincos of mp_core.h takes
// the quadrant of a NaN angle through an int cast on the poisoned rows - every kernel's shared routine, whose result is NaN either way.)
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
  // a 3-joint chain: z, y, prismatic x
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

  // S = 64 in an order that is not sorted by link, every pair two links apart
  std::vector<int32_t> link(64), pairs;
  std::vector<double> centre(64 * 3), radius(64);
  for (int s = 0; s < 64; ++s) {
    link[s] = (s * 7) % 4;
    for (int k = 0; k < 3; ++k) centre[3 * s + k] = 0.01 * ((s * (k + 3)) % 60) - 0.3;
    radius[s] = 0.02 + 0.001 * s;
  }
  for (int a = 0; a < 64; ++a)
    for (int b = 0; b < 64; ++b)
      if (link[a] + 2 <= link[b]) { pairs.push_back(a); pairs.push_back(b); }
  mp_collision* h = nullptr;
  EXPECT(mp_collision_create(model, 64, link.data(), centre.data(), radius.data(), (int)pairs.size() / 2, pairs.data(), &h) == MP_OK);
  // invalid tables: no handle comes back
  mp_collision* bad = nullptr;
  EXPECT(mp_collision_create(model, 65, link.data(), centre.data(), radius.data(), 0, nullptr, &bad) == MP_ERR_INVALID && !bad);
  EXPECT(mp_collision_create(model, 0, link.data(), centre.data(), radius.data(), 0, nullptr, &bad) == MP_ERR_INVALID && !bad);
  { auto l = link; l[5] = 4; EXPECT(mp_collision_create(model, 64, l.data(), centre.data(), radius.data(), 0, nullptr, &bad) == MP_ERR_INVALID); }
  { auto r = radius; r[9] = 0.0; EXPECT(mp_collision_create(model, 64, link.data(), centre.data(), r.data(), 0, nullptr, &bad) == MP_ERR_INVALID); }
  { int32_t p[2] = {3, 64}; EXPECT(mp_collision_create(model, 64, link.data(), centre.data(), radius.data(), 1, p, &bad) == MP_ERR_INVALID); }
  { int32_t p[2] = {3, 3}; EXPECT(mp_collision_create(model, 64, link.data(), centre.data(), radius.data(), 1, p, &bad) == MP_ERR_INVALID); }

  // the world: one of each kind, then the invalid ones (which leave it in place)
  std::vector<MpColObstacle> w;
  int32_t kind[4] = {MP_OBSTACLE_SPHERE, MP_OBSTACLE_CAPSULE, MP_OBSTACLE_BOX, MP_OBSTACLE_CAPSULE};
  double prm[4 * 16] = {};
  double* p = prm;
  p[0] = 0.3; p[1] = 0.1; p[2] = 0.2; p[3] = 0.15; p += 16;
  p[0] = -0.2; p[1] = 0.1; p[2] = 0.0; p[3] = 0.2; p[4] = 0.3; p[5] = 0.4; p[6] = 0.05; p += 16;
  p[0] = 0.1; p[1] = -0.3; p[2] = 0.3; p[3] = 1; p[7] = 1; p[11] = 1; p[12] = 0.1; p[13] = 0.2; p[14] = 0.3; p += 16;
  p[0] = p[3] = 0.5; p[1] = p[4] = 0.5; p[2] = p[5] = 0.5; p[6] = 0.1;  // degenerate capsule
  EXPECT(mp_collision_pack_world("main", 4, kind, prm, &w) == MP_OK && w.size() == 4);
  { int32_t k2[1] = {7}; EXPECT(mp_collision_pack_world("main", 1, k2, prm, &w) == MP_ERR_INVALID && w.size() == 4); }
  { double q2[16]; std::memcpy(q2, prm + 32, sizeof q2); q2[4] = 1e-8; int32_t k2[1] = {MP_OBSTACLE_BOX};
    EXPECT(mp_collision_pack_world("main", 1, k2, q2, &w) == MP_ERR_INVALID); }
  { double q2[16] = {}; q2[1] = NAN; int32_t k2[1] = {MP_OBSTACLE_SPHERE}; EXPECT(mp_collision_pack_world("main", 1, k2, q2, &w) == MP_ERR_INVALID); }
  h->world = w;

  // the twin: 131 rows (the last slice of a thread is short), a NaN row, every output, then the distances alone, one thread and four
  const int rows = 131;
  std::vector<double> q(rows * n), dw(rows), ds(rows), cost(rows), gdw(rows * n), gds(rows * n), grad(rows * n), dw2(rows);
  std::vector<int32_t> aw(2 * rows), as(2 * rows);
  for (int r = 0; r < rows; ++r)
    for (int j = 0; j < n; ++j) q[r * n + j] = 0.05 * ((r * (j + 2)) % 50) - 1.2;
  q[17 * n + 1] = NAN;
  for (int threads : {1, 4}) {
    EXPECT(mp_collision_cpu_f64(model, h, q.data(), rows, 0.1, 0.1, dw.data(), aw.data(), ds.data(), as.data(), gdw.data(), gds.data(),
                                cost.data(), grad.data(), threads) == MP_OK);
    EXPECT(std::isnan(dw[17]) && std::isnan(grad[17 * n]) && aw[34] == -1 && as[35] == -1);
    EXPECT(std::isfinite(dw[16]) && std::isfinite(ds[18]) && aw[0] >= 0 && aw[0] < 64 && aw[1] >= 0 && aw[1] < 4);
    EXPECT(mp_collision_cpu_f64(model, h, q.data(), rows, 0.1, 0.1, dw2.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr, threads) == MP_OK);
    for (int r = 0; r < rows; ++r) EXPECT(r == 17 || dw2[r] == dw[r]);
  }
  EXPECT(mp_collision_cpu_f64(model, h, q.data(), rows, 0.0, 0.1, dw.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1) ==
         MP_ERR_INVALID);
  // no world, no pairs, one sphere on the base
  mp_collision* one = nullptr;
  int32_t l0[1] = {0};
  EXPECT(mp_collision_create(model, 1, l0, centre.data(), radius.data(), 0, nullptr, &one) == MP_OK);
  EXPECT(mp_collision_cpu_f64(model, one, q.data(), rows, 0.1, 0.1, dw.data(), aw.data(), ds.data(), as.data(), gdw.data(), gds.data(),
                              cost.data(), grad.data(), 2) == MP_OK);
  EXPECT(std::isinf(dw[0]) && std::isinf(ds[0]) && cost[0] == 0.0 && aw[0] == -1);
  mp_collision_destroy(one);
  mp_collision_destroy(h);
  delete model;
  std::printf(fails ? "%d checks failed\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
