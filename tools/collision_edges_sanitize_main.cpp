// Stand-alone check of the edge check's motion-bound tables and of its CPU twin under AddressSanitizer / UBSan (host code only, no GPU,
// no Python):
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=float-cast-overflow -fno-sanitize-recover=undefined -pthread \
//       -Imanipulapy_amd/csrc tools/collision_edges_sanitize_main.cpp manipulapy_amd/csrc/mp_cpu.cpp manipulapy_amd/csrc/mp_model_compile.cpp \
//       -o collision_edges_sanitize
// Exits 0 and prints "ok" when every call behaved as the header says.  (float-cast-overflow is left out for the reason given in
// collision_sanitize_main.cpp.)
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
  // a 3-joint chain: z, y, prismatic x (the chain of collision_sanitize_main.cpp)
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

  // S = 64 (the largest park) in an order that is not sorted by link, every pair two links apart
  std::vector<int32_t> link(64), pairs;
  std::vector<double> centre(64 * 3), radius(64);
  for (int s = 0; s < 64; ++s) {
    link[s] = (s * 7) % 4;
    for (int k = 0; k < 3; ++k) centre[3 * s + k] = 0.01 * ((s * (k + 3)) % 60) - 0.3;
    radius[s] = 0.02 + 0.0002 * s;
  }
  for (int a = 0; a < 64; ++a)
    for (int b = 0; b < 64; ++b)
      if (link[a] + 2 <= link[b]) { pairs.push_back(a); pairs.push_back(b); }
  mp_collision* h = nullptr;
  EXPECT(mp_collision_create(model, 64, link.data(), centre.data(), radius.data(), (int)pairs.size() / 2, pairs.data(), &h) == MP_OK);

  // the bound table: (n, n + 1), zero below the diagonal and for the prismatic joint 3, positive for the revolute joints
  double rho[n * (n + 1)];
  for (double& v : rho) v = -1.0;
  EXPECT(mp_collision_motion_bounds(h, rho) == MP_OK);
  EXPECT(mp_collision_motion_bounds(nullptr, rho) == MP_ERR_INVALID && mp_collision_motion_bounds(h, nullptr) == MP_ERR_INVALID);
  for (int j = 0; j < n; ++j)
    for (int k = 0; k <= n; ++k) {
      const double v = rho[j * (n + 1) + k];
      if (k < j + 1 || j == 2) EXPECT(v == 0.0);
      else EXPECT(v > 0.0 && std::isfinite(v));
    }
  EXPECT(rho[0 * 4 + 2] >= rho[1 * 4 + 2]);  // the polyline to joint 1 runs through the anchor of joint 2

  int32_t kind[3] = {MP_OBSTACLE_SPHERE, MP_OBSTACLE_CAPSULE, MP_OBSTACLE_BOX};
  double prm[3 * 16] = {};
  double* p = prm;
  p[0] = 0.9; p[1] = 0.1; p[2] = 0.2; p[3] = 0.15; p += 16;
  p[0] = -0.7; p[1] = 0.6; p[2] = 0.0; p[3] = -0.6; p[4] = 0.9; p[5] = 0.4; p[6] = 0.05; p += 16;
  p[0] = 0.1; p[1] = -1.0; p[2] = 0.3; p[3] = 1; p[7] = 1; p[11] = 1; p[12] = 0.1; p[13] = 0.2; p[14] = 0.3;
  EXPECT(mp_collision_pack_world("main", 3, kind, prm, &h->world) == MP_OK && h->world.size() == 3);

  // the twin: 133 edges (the last slice of a thread is short) of every kind - zero edges, short and long ones, a NaN and an inf
  // end point - every output, then subsets, one thread and four
  const int E = 133;
  std::vector<double> qa(E * n), qb(E * n), t(E), cl(E), t2(E);
  std::vector<int32_t> st(E), sp(E), wi(3 * E), st2(E);
  for (int e = 0; e < E; ++e)
    for (int j = 0; j < n; ++j) {
      qa[e * n + j] = 0.05 * ((e * (j + 2)) % 50) - 1.2;
      qb[e * n + j] = qa[e * n + j] + (e % 5) * 0.4 * (((e + j) % 3) - 1);
    }
  qa[17 * n + 1] = NAN;
  qb[40 * n + 2] = INFINITY;
  const double tol = 1e-3;
  double margin = 0.0;
  int total[3] = {0, 0, 0};
  // the crowded model overlaps at home: negative margins leave free edges
  for (int run = 0; run < 6; ++run) {
    const int threads = run % 2 ? 4 : 1;
    margin = run < 2 ? -0.5 : (run < 4 ? -0.2 : -0.1);
    EXPECT(mp_collision_edges_cpu_f64(model, h, qa.data(), qb.data(), E, margin, tol, 64, st.data(), t.data(), sp.data(), cl.data(), wi.data(),
                                      threads) == MP_OK);
    EXPECT(st[17] == MP_EDGE_INVALID && std::isnan(t[17]) && std::isnan(cl[17]) && sp[17] == 0 && wi[3 * 17] == -1);
    EXPECT(st[40] == MP_EDGE_INVALID && sp[40] == 0 && wi[3 * 40 + 2] == -1);
    int seen[3] = {0, 0, 0};
    for (int e = 0; e < E; ++e) {
      if (e == 17 || e == 40) continue;
      EXPECT(st[e] >= 0 && st[e] <= 2 && sp[e] >= 1 && sp[e] <= 64 && t[e] >= 0.0 && t[e] <= 1.0 && std::isfinite(cl[e]));
      EXPECT((wi[3 * e] == 0 && wi[3 * e + 2] < 3) || (wi[3 * e] == 1 && wi[3 * e + 2] < 64));
      EXPECT(wi[3 * e + 1] >= 0 && wi[3 * e + 1] < 64);
      if (e % 5 == 0) EXPECT(sp[e] == 1 && (t[e] == 0.0 || t[e] == 1.0));  // a zero edge
      seen[st[e]] += 1;
    }
    std::printf("margin %g, threads %d: %d free, %d blocked, %d undecided\n", margin, threads, seen[0], seen[1], seen[2]);
    EXPECT(seen[0] + seen[1] + seen[2] == E - 2);
    for (int k = 0; k < 3; ++k) total[k] += seen[k];
    EXPECT(mp_collision_edges_cpu_f64(model, h, qa.data(), qb.data(), E, margin, tol, 64, st2.data(), t2.data(), nullptr, nullptr, nullptr,
                                      threads) == MP_OK);
    for (int e = 0; e < E; ++e) EXPECT(st2[e] == st[e] && (e == 17 || e == 40 || t2[e] == t[e]));
  }
  EXPECT(total[MP_EDGE_FREE] > 0 && total[MP_EDGE_BLOCKED] > 0);
  // one evaluation an edge: whatever is not decided at t = 0 is UNDECIDED there
  EXPECT(mp_collision_edges_cpu_f64(model, h, qa.data(), qb.data(), E, margin, tol, 1, st.data(), t.data(), sp.data(), nullptr, nullptr, 2) == MP_OK);
  for (int e = 0; e < E; ++e) EXPECT(e == 17 || e == 40 || (sp[e] == 1 && (st[e] != MP_EDGE_UNDECIDED || t[e] == 0.0)));
  // invalid parameters
  EXPECT(mp_collision_edges_cpu_f64(model, h, qa.data(), qb.data(), E, NAN, tol, 8, st.data(), nullptr, nullptr, nullptr, nullptr, 1) == MP_ERR_INVALID);
  EXPECT(mp_collision_edges_cpu_f64(model, h, qa.data(), qb.data(), E, 0.0, 0.0, 8, st.data(), nullptr, nullptr, nullptr, nullptr, 1) == MP_ERR_INVALID);
  EXPECT(mp_collision_edges_cpu_f64(model, h, qa.data(), qb.data(), E, 0.0, tol, 0, st.data(), nullptr, nullptr, nullptr, nullptr, 1) == MP_ERR_INVALID);
  EXPECT(mp_collision_edges_cpu_f64(model, h, qa.data(), qb.data(), E, 0.0, tol, 65537, st.data(), nullptr, nullptr, nullptr, nullptr, 1) == MP_ERR_INVALID);
  EXPECT(mp_collision_edges_cpu_f64(model, h, qa.data(), qb.data(), E, 0.0, tol, 8, nullptr, nullptr, nullptr, nullptr, nullptr, 1) == MP_ERR_INVALID);
  EXPECT(mp_collision_edges_cpu_f64(model, h, qa.data(), qb.data(), 0, 0.0, tol, 8, nullptr, nullptr, nullptr, nullptr, nullptr, 1) == MP_OK);
  // no world, no pairs, one sphere on the base: FREE in one step, +inf clearance, no witness
  mp_collision* one = nullptr;
  int32_t l0[1] = {0};
  EXPECT(mp_collision_create(model, 1, l0, centre.data(), radius.data(), 0, nullptr, &one) == MP_OK);
  EXPECT(mp_collision_edges_cpu_f64(model, one, qa.data(), qb.data(), E, 0.02, tol, 8, st.data(), t.data(), sp.data(), cl.data(), wi.data(), 2) == MP_OK);
  EXPECT(st[0] == MP_EDGE_FREE && t[3] == 1.0 && sp[4] == 1 && std::isinf(cl[5]) && wi[18] == -1 && st[17] == MP_EDGE_INVALID);
  mp_collision_destroy(one);
  mp_collision_destroy(h);
  delete model;
  std::printf(fails ? "%d checks failed\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
