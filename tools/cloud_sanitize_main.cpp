// Stand-alone check of the point-cloud world under AddressSanitizer / UBSan (host code only, no GPU, no Python): the grid builder,
// the validation and the CPU twin's query on the recipe of tests/cloud_cases.py (497 points: a table top, a post, 60 loose points).
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=float-cast-overflow -fno-sanitize-recover=undefined -pthread \
//       -Imanipulapy_amd/csrc tools/cloud_sanitize_main.cpp manipulapy_amd/csrc/mp_cpu.cpp manipulapy_amd/csrc/mp_cloud_build.cpp \
//       manipulapy_amd/csrc/mp_model_compile.cpp -o cloud_sanitize
// Exits 0 and prints "ok" when every call behaved as the header says.  (float-cast-overflow: see tools/collision_sanitize_main.cpp.)
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

static unsigned long long lcg = 12345;
static double uniform(double lo, double hi) {
  lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
  return lo + (hi - lo) * (double)(lcg >> 11) / 9007199254740992.0;
}

// brute force over all points: the value, the index (M where truncated)
static void brute(const std::vector<double>& pts, double r_c, double d_max, const double p[3], double& sd, int& who) {
  const int M = (int)pts.size() / 3;
  double best = HUGE_VAL;
  int bi = -1;
  for (int i = 0; i < M; ++i) {
    const double dx = p[0] - pts[3 * i], dy = p[1] - pts[3 * i + 1], dz = p[2] - pts[3 * i + 2];
    const double d2 = dx * dx + dy * dy + dz * dz;
    if (d2 < best) { best = d2; bi = i; }
  }
  const double m = std::sqrt(best) - r_c;
  if (m <= d_max) { sd = m; who = bi; } else { sd = d_max; who = M; }
}

int main() {
  const double pitch = 0.04, r_c = pitch * std::sqrt(3.0) / 2.0, d_max = 0.2;
  std::vector<double> pts;
  for (int a = 0; a < 16; ++a)
    for (int b = 0; b < 26; ++b) { pts.push_back(0.25 + pitch * a); pts.push_back(-0.5 + pitch * b); pts.push_back(0.1); }
  for (int k = 0; k < 21; ++k) { pts.push_back(0.5); pts.push_back(0.3); pts.push_back(0.1 + pitch * k); }
  for (int k = 0; k < 60; ++k) { pts.push_back(uniform(-0.9, 0.9)); pts.push_back(uniform(-0.9, 0.9)); pts.push_back(uniform(0.0, 1.2)); }
  const int M = (int)pts.size() / 3;
  EXPECT(M == 497);

  // the builder at the default cell and at a quarter of it; the validation (which leaves the image alone)
  std::vector<MpCloudPoint> coarse, fine, keep;
  EXPECT(mp_cloud_build("main", M, pts.data(), r_c, d_max, 0.0, &coarse) == MP_OK && !coarse.empty());
  EXPECT(mp_cloud_build("main", M, pts.data(), r_c, d_max, (d_max + r_c) / 4, &fine) == MP_OK && fine.size() > coarse.size());
  const MpColCloud* hc = reinterpret_cast<const MpColCloud*>(coarse.data());
  const MpColCloud* hf = reinterpret_cast<const MpColCloud*>(fine.data());
  EXPECT(hc->M == M && hc->R == 1 && hf->R == 4 && hc->cells == hc->dim[0] * hc->dim[1] * hc->dim[2]);
  EXPECT(hf->pts_off + (size_t)M * sizeof(MpCloudPoint) == fine.size() * sizeof(MpCloudPoint));
  {
    const int* start = reinterpret_cast<const int*>(fine.data() + 4);
    bool mono = start[0] == 0 && start[hf->cells] == M;
    for (int c = 0; c < hf->cells; ++c) mono = mono && start[c] <= start[c + 1];
    EXPECT(mono);
  }
  keep = coarse;
  { auto p = pts; p[3 * 17 + 1] = NAN; EXPECT(mp_cloud_build("main", M, p.data(), r_c, d_max, 0.0, &coarse) == MP_ERR_INVALID); }
  { auto p = pts; p[3 * 400 + 2] = HUGE_VAL; EXPECT(mp_cloud_build("main", M, p.data(), r_c, d_max, 0.0, &coarse) == MP_ERR_INVALID); }
  EXPECT(mp_cloud_build("main", M, pts.data(), -0.01, d_max, 0.0, &coarse) == MP_ERR_INVALID);
  EXPECT(mp_cloud_build("main", M, pts.data(), NAN, d_max, 0.0, &coarse) == MP_ERR_INVALID);
  EXPECT(mp_cloud_build("main", M, pts.data(), r_c, 0.0, 0.0, &coarse) == MP_ERR_INVALID);
  EXPECT(mp_cloud_build("main", M, pts.data(), r_c, HUGE_VAL, 0.0, &coarse) == MP_ERR_INVALID);
  EXPECT(mp_cloud_build("main", M, pts.data(), r_c, d_max, (d_max + r_c) / 4.001, &coarse) == MP_ERR_INVALID);
  EXPECT(mp_cloud_build("main", M, pts.data(), r_c, d_max, HUGE_VAL, &coarse) == MP_ERR_INVALID);
  EXPECT(mp_cloud_build("main", (1 << 24) + 1, pts.data(), r_c, d_max, 0.0, &coarse) == MP_ERR_INVALID && std::strstr(g_msg, "2^24"));
  EXPECT(mp_cloud_build("main", -1, pts.data(), r_c, d_max, 0.0, &coarse) == MP_ERR_INVALID);
  EXPECT(mp_cloud_build("main", M, nullptr, r_c, d_max, 0.0, &coarse) == MP_ERR_INVALID);
  { double far[6] = {0, 0, 0, 1000, 1000, 1000};
    EXPECT(mp_cloud_build("main", 2, far, 0.01, 0.04, 0.0, &coarse) == MP_ERR_INVALID && std::strstr(g_msg, "raise cell")); }
  EXPECT(coarse.size() == keep.size() && std::memcmp(coarse.data(), keep.data(), keep.size() * sizeof(MpCloudPoint)) == 0);
  { std::vector<MpCloudPoint> none = keep; EXPECT(mp_cloud_build("main", 0, nullptr, 0.0, 1.0, 0.0, &none) == MP_OK && none.empty()); }

  // the query against brute force: inside the box, far outside on every side, on the points themselves; both grids bit for bit
  for (int k = 0; k < 4000; ++k) {
    double p[3] = {uniform(-1.2, 1.2), uniform(-1.2, 1.2), uniform(-0.3, 1.5)};
    if (k % 7 == 0) p[k % 3] += (k % 2 ? 50.0 : -50.0);
    if (k % 11 == 0) { const int i = k % M; p[0] = pts[3 * i]; p[1] = pts[3 * i + 1]; p[2] = pts[3 * i + 2]; }
    double sd, nx, ny, nz, sd2, mx, my, mz, want;
    int who, who2, wi;
    mp_cloud_distance<MpCloudPtrHost>(hc, p[0], p[1], p[2], MP_COL_TINY, sd, nx, ny, nz, who);
    mp_cloud_distance<MpCloudPtrHost>(hf, p[0], p[1], p[2], MP_COL_TINY, sd2, mx, my, mz, who2);
    brute(pts, r_c, d_max, p, want, wi);
    EXPECT(sd == want && who == wi);
    EXPECT(sd2 == sd && who2 == who && mx == nx && my == ny && mz == nz);
    const double len = std::sqrt(nx * nx + ny * ny + nz * nz);
    if (who == M) EXPECT(sd == d_max && len == 0.0);
    else if (k % 11 == 0) EXPECT(sd == -r_c && len == 0.0);  // on a point: n = 0
    else EXPECT(std::fabs(len - 1.0) < 1e-12);
  }
  { double sd, nx, ny, nz; int who;  // a NaN query runs through the clamp and touches nothing it should not
    mp_cloud_distance<MpCloudPtrHost>(hf, NAN, 0.0, HUGE_VAL, MP_COL_TINY, sd, nx, ny, nz, who);
    EXPECT(who == M && sd == d_max); }
  // M = 1, r_c = 0, the query on the point
  { double one[3] = {0.1, 0.2, 0.3}; std::vector<MpCloudPoint> img; double sd, nx, ny, nz; int who;
    EXPECT(mp_cloud_build("main", 1, one, 0.0, 0.5, 0.0, &img) == MP_OK);
    mp_cloud_distance<MpCloudPtrHost>(reinterpret_cast<const MpColCloud*>(img.data()), 0.1, 0.2, 0.3, MP_COL_TINY, sd, nx, ny, nz, who);
    EXPECT(sd == 0.0 && who == 0 && nx == 0.0 && ny == 0.0 && nz == 0.0); }

  // the twin through a handle: a 3-joint chain (z, y, prismatic x), spheres on every link, the cloud with and without primitives
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
  std::vector<int32_t> link(40);
  std::vector<double> centre(40 * 3), radius(40);
  for (int s = 0; s < 40; ++s) {
    link[s] = (s * 7) % 4;
    centre[3 * s] = 0.02 * s; centre[3 * s + 1] = 0.01 * ((s * 5) % 20) - 0.1; centre[3 * s + 2] = 0.15 + 0.01 * ((s * 3) % 30);
    radius[s] = 0.03 + 0.001 * s;
  }
  mp_collision* h = nullptr;
  EXPECT(mp_collision_create(model, 40, link.data(), centre.data(), radius.data(), 0, nullptr, &h) == MP_OK);
  const int rows = 131;
  std::vector<double> q(rows * n), dw(rows), dw0(rows), cost(rows), gdw(rows * n), grad(rows * n);
  std::vector<int32_t> aw(2 * rows), st(rows), wit(3 * rows);
  for (int r = 0; r < rows; ++r)
    for (int j = 0; j < n; ++j) q[r * n + j] = 0.05 * ((r * (j + 2)) % 50) - 1.2;
  q[17 * n + 1] = NAN;
  EXPECT(mp_collision_cpu_f64(model, h, q.data(), rows, 0.1, 0.1, dw0.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2) == MP_OK);
  EXPECT(std::isinf(dw0[0]));
  h->cloud = fine;
  int64_t im = 0; double ir = 0, id = 0, ic = 0; int32_t dims[3];
  EXPECT(mp_collision_cloud_info(h, &im, &ir, &id, &ic, dims) == MP_OK && im == M && ir == r_c && id == d_max && dims[0] == hf->dim[0]);
  for (int threads : {1, 4}) {
    EXPECT(mp_collision_cpu_f64(model, h, q.data(), rows, 0.1, 0.1, dw.data(), aw.data(), nullptr, nullptr, gdw.data(), nullptr, cost.data(),
                                grad.data(), threads) == MP_OK);
    EXPECT(std::isnan(dw[17]) && aw[34] == -1 && std::isfinite(dw[16]) && dw[16] <= d_max && aw[33] >= 0 && aw[33] <= M);
  }
  int32_t kind[1] = {MP_OBSTACLE_SPHERE};
  double prm[16] = {0.3, 0.1, 0.2, 0.15};
  EXPECT(mp_collision_pack_world("main", 1, kind, prm, &h->world) == MP_OK);
  EXPECT(mp_collision_cpu_f64(model, h, q.data(), rows, 0.1, 0.1, dw.data(), aw.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1) == MP_OK);
  EXPECT(aw[1] >= 0 && aw[1] <= 1 + M);
  std::vector<double> qb(q);
  for (int r = 0; r < rows; ++r) qb[r * n] += 0.4;
  EXPECT(mp_collision_edges_cpu_f64(model, h, q.data(), qb.data(), rows, 0.02, 1e-3, 512, st.data(), nullptr, nullptr, nullptr, wit.data(), 3) == MP_OK);
  EXPECT(st[17] == MP_EDGE_INVALID && st[16] >= 0);
  h->cloud.clear();
  h->world.clear();
  EXPECT(mp_collision_cpu_f64(model, h, q.data(), rows, 0.1, 0.1, dw.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2) == MP_OK);
  for (int r = 0; r < rows; ++r) EXPECT(r == 17 || dw[r] == dw0[r]);
  mp_collision_destroy(h);
  delete model;
  std::printf(fails ? "%d checks failed\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
