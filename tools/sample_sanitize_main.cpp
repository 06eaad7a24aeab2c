// Stand-alone check of the trajectory sampler's CPU twin under AddressSanitizer / UBSan (host code only, no GPU, no Python):
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=float-cast-overflow -fno-sanitize-recover=undefined -pthread \
//       -Imanipulapy_amd/csrc tools/sample_sanitize_main.cpp manipulapy_amd/csrc/mp_cpu.cpp manipulapy_amd/csrc/mp_model_compile.cpp \
//       -o sample_sanitize
// Exits 0 and prints "ok" when every call behaved as the header says.  (float-cast-overflow is left out for the reason given in
// collision_sanitize_main.cpp.)  Every array is exactly as large as the header says: N = 3 and 33 grid points, M = 1, 2 and 40 rows,
// both sources, so that the sanitizer sees the slots at both ends of every table and of every output.  The paths are timed by the
// parameterisation's own twin and, in the curve source, blended by the blender's.
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

static const int n = 3, B = 9;
static int seen[5] = {0, 0, 0, 0, 0};  // by status, INVALID last

// rows 3.. of t / x are replaced: 3 NaN (no timing), 4 an interior stop, 5 a decreasing t, 7 T = dt / 2, 8 T = 8 dt exactly (6 is the
// grid source's NaN in q, the curve source's path without a curve); returns dt
static double plant(std::vector<double>& t, std::vector<double>& x, int N) {
  double Tmax = 0.0;
  for (int b = 0; b < 3; ++b) Tmax = std::fmax(Tmax, t[(size_t)b * N + N - 1]);
  const double dt = std::exp2(std::round(std::log2(Tmax / 39.0)));
  for (int b = 3; b < B; ++b)
    for (int i = 0; i < N; ++i) { t[(size_t)b * N + i] = t[i]; x[(size_t)b * N + i] = x[i]; }
  for (int i = 0; i < N; ++i) { t[(size_t)3 * N + i] = NAN; x[(size_t)3 * N + i] = NAN; }
  for (int i = N / 2; i < N; ++i) t[(size_t)4 * N + i] = INFINITY;
  x[(size_t)4 * N + N / 2] = 0.0;
  std::swap(t[(size_t)5 * N + 1], t[(size_t)5 * N + 2]);
  const double T = t[N - 1], to[2] = {dt / 2, 8 * dt};
  for (int k = 0; k < 2; ++k) {
    const double c = to[k] / T;
    for (int i = 0; i < N; ++i) { t[(size_t)(7 + k) * N + i] = t[i] * c; x[(size_t)(7 + k) * N + i] = x[i] / (c * c); }
    t[(size_t)(7 + k) * N + N - 1] = to[k];
  }
  return dt;
}

// every M and thread count on one source; `end`: the paths' end points (B, n)
static void sample_all(const mp_model* model, const char* what, int N, double dt, const std::vector<double>& t, const std::vector<double>& x,
                       const double* q, const double* dq, const double* ddq, const int32_t* bst, const int32_t* bcnt, const double* pts,
                       const double* cut, const double* knot, const double* len, int Win, const std::vector<double>& end) {
  const double F[6] = {0.1, 0.0, -0.2, 1.0, 2.0, -1.0};
  const int Ms[3] = {1, 2, 40};
  for (int mi = 0; mi < 3; ++mi)
    for (int threads = 1; threads <= 4; threads += 3) {
      const int M = Ms[mi];
      std::vector<int32_t> st(B, -7), cnt(B, -7), need(B, -7), st2(B, -7);
      std::vector<double> s((size_t)B * M, -7.0), sd(s), sdd(s);
      std::vector<double> pos((size_t)B * M * n, -7.0), vel(pos), acc(pos), tau(pos), pos2(pos), tau2(pos), tauF(pos);
#define SAMPLE(FTIP, ST, CNT, NEED, S, SD, SDD, POS, VEL, ACC, TAU)                                                                      \
  mp_trajectory_sample_cpu_f64(model, t.data(), x.data(), B, N, q, dq, ddq, bst, bcnt, pts, cut, knot, len, Win, dt, M, nullptr, FTIP, ST, \
                               CNT, NEED, S, SD, SDD, POS, VEL, ACC, TAU, threads)
      EXPECT(SAMPLE(nullptr, st.data(), cnt.data(), need.data(), s.data(), sd.data(), sdd.data(), pos.data(), vel.data(), acc.data(),
                    tau.data()) == MP_OK);
      int here[5] = {0, 0, 0, 0, 0};
      for (int b = 0; b < B; ++b) {
        EXPECT(st[b] >= -1 && st[b] <= 3);
        here[st[b] < 0 ? 4 : st[b]] += 1;
        const bool live = st[b] == MP_SAMPLE_OK || st[b] == MP_SAMPLE_TRUNCATED;
        const double* p = &pos[(size_t)b * M * n];
        if (b == 3) EXPECT(st[b] == MP_SAMPLE_UNTIMED);
        if (b == 4) EXPECT(st[b] == MP_SAMPLE_STOPS);
        if (b == 5) EXPECT(st[b] == MP_SAMPLE_INVALID);
        if (b == 6) EXPECT(!live);
        if (b == 7) EXPECT(live && need[b] == 2);
        if (b == 8) EXPECT(live && need[b] == 9);
        if (!live) {
          EXPECT(cnt[b] == 0 && need[b] == 0 && std::isnan(p[0]) && std::isnan(p[M * n - 1]) && std::isnan(s[(size_t)b * M]) &&
                 std::isnan(tau[(size_t)(b + 1) * M * n - 1]) && std::isnan(sdd[(size_t)(b + 1) * M - 1]));
          continue;
        }
        EXPECT(need[b] >= 1 && cnt[b] == (need[b] < M ? need[b] : M) && (st[b] == MP_SAMPLE_TRUNCATED) == (need[b] > M));
        EXPECT(s[(size_t)b * M] == 0.0);
        for (int k = 0; k < M; ++k) {
          const double sk = s[(size_t)b * M + k];
          EXPECT(sk >= 0.0 && sk <= 1.0 && (k == 0 || sk >= s[(size_t)b * M + k - 1]) && sd[(size_t)b * M + k] >= 0.0);
          for (int j = 0; j < n; ++j) {
            const size_t at = ((size_t)b * M + k) * n + j;
            EXPECT(std::isfinite(pos[at]) && std::isfinite(vel[at]) && std::isfinite(acc[at]) && std::isfinite(tau[at]));
            if (k >= cnt[b] - 1 && st[b] == MP_SAMPLE_OK) EXPECT(pos[at] == end[(size_t)b * n + j] && vel[at] == 0.0 && acc[at] == 0.0 && sk == 1.0);
          }
        }
      }
      std::printf("%s, N %d, M %d, threads %d: %d ok, %d truncated, %d stops, %d untimed, %d invalid\n", what, N, M, threads, here[0], here[1],
                  here[2], here[3], here[4]);
      for (int k = 0; k < 5; ++k) seen[k] += here[k];
      // subsets of the outputs give the same values; a wrench changes the torques only
      EXPECT(SAMPLE(nullptr, st2.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == MP_OK);
      EXPECT(SAMPLE(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, pos2.data(), nullptr, nullptr, nullptr) == MP_OK);
      EXPECT(SAMPLE(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, tau2.data()) == MP_OK);
      EXPECT(SAMPLE(F, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, tauF.data()) == MP_OK);
      for (int b = 0; b < B; ++b) EXPECT(st2[b] == st[b]);
      EXPECT(std::memcmp(pos.data(), pos2.data(), pos.size() * sizeof(double)) == 0);
      EXPECT(std::memcmp(tau.data(), tau2.data(), tau.size() * sizeof(double)) == 0);
      EXPECT(std::memcmp(tau.data(), tauF.data(), tau.size() * sizeof(double)) != 0);
#undef SAMPLE
    }
}

int main() {
  // the 3-joint chain and the world of blend_sanitize_main.cpp: z, y, prismatic x
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
  EXPECT(mp_collision_create(model, 4, link, centre, radius, 0, nullptr, &h) == MP_OK);   // an empty world: nothing blocks a blend

  const double vlim[n] = {1.0, 1.0, 0.5}, alim[n] = {2.0, 2.0, 1.0};
  const int grids[2] = {3, 33};
  for (int gi = 0; gi < 2; ++gi) {
    const int N = grids[gi];
    const size_t rows = (size_t)B * N;
    std::vector<double> zero(B, 0.0), K(rows * 2), u(rows), dur(B);
    std::vector<int32_t> tst(B);
    // ---- the grid source: q(s) = q0 + s D + A sin^2(pi s)
    {
      std::vector<double> q(rows * n), dq(q), ddq(q), t(rows), x(rows), end((size_t)B * n);
      for (int b = 0; b < B; ++b)
        for (int i = 0; i < N; ++i)
          for (int j = 0; j < n; ++j) {
            const int p = b < 3 ? b : 0;
            const double s = (double)i / (N - 1), q0 = -0.4 + 0.1 * p + 0.05 * j, D = 0.8 - 0.3 * j + 0.1 * p, A = 0.1 * (j - 1);
            const size_t at = ((size_t)b * N + i) * n + j;
            q[at] = q0 + s * D + A * std::sin(M_PI * s) * std::sin(M_PI * s);
            dq[at] = D + A * M_PI * std::sin(2 * M_PI * s);
            ddq[at] = A * 2 * M_PI * M_PI * std::cos(2 * M_PI * s);
            if (i == N - 1) end[(size_t)b * n + j] = q[at];
          }
      EXPECT(mp_toppra_cpu_f64(model, q.data(), dq.data(), ddq.data(), vlim, nullptr, alim, zero.data(), zero.data(), B, N, nullptr, nullptr,
                               K.data(), x.data(), u.data(), t.data(), dur.data(), tst.data(), nullptr, nullptr, nullptr, 1) == MP_OK);
      for (int b = 0; b < B; ++b) EXPECT(tst[b] == 0 && std::isfinite(dur[b]));
      const double dt = plant(t, x, N);
      q[((size_t)6 * N + 1) * n + 2] = NAN;
      sample_all(model, "grid", N, dt, t, x, q.data(), dq.data(), ddq.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, end);
    }
    // ---- the curve source: zigzags of 4 waypoints in W_in = 4 rows (path 6: a count of 1, no curve), blended, timed on the blend's grid
    {
      const int Win = 4;
      std::vector<double> in((size_t)B * Win * n), end((size_t)B * n);
      std::vector<int32_t> cin(B, Win), bst(B), bcnt(B);
      for (int b = 0; b < B; ++b)
        for (int w = 0; w < Win; ++w) {
          double* p = &in[((size_t)b * Win + w) * n];
          const int pth = b < 3 ? b : 0;
          p[0] = -0.5 + 0.1 * pth + 0.4 * w;
          p[1] = 0.1 * pth + (w % 2 ? 0.3 : -0.1);
          p[2] = 0.02 * w;
          if (w == Win - 1) std::memcpy(&end[(size_t)b * n], p, n * sizeof(double));
        }
      cin[6] = 1;
      std::vector<double> pts((size_t)B * Win * n), cut((size_t)B * Win), knot(cut), len(B), q(rows * n), dq(q), ddq(q), t(rows), x(rows);
      EXPECT(mp_path_blend_cpu_f64(model, h, in.data(), cin.data(), B, Win, N, 0.2, 2, 0.0, 1e-3, 16, bst.data(), nullptr, bcnt.data(), pts.data(),
                                   cut.data(), knot.data(), len.data(), nullptr, nullptr, nullptr, q.data(), dq.data(), ddq.data(), 1) == MP_OK);
      for (int b = 0; b < B; ++b) EXPECT(b == 6 ? bst[b] == MP_BLEND_SKIPPED : bst[b] == MP_BLEND_DONE);
      for (size_t k = 0; k < (size_t)N * n; ++k) { q[(size_t)6 * N * n + k] = q[k]; dq[(size_t)6 * N * n + k] = dq[k]; ddq[(size_t)6 * N * n + k] = ddq[k]; }
      EXPECT(mp_toppra_cpu_f64(model, q.data(), dq.data(), ddq.data(), vlim, nullptr, alim, zero.data(), zero.data(), B, N, nullptr, nullptr,
                               K.data(), x.data(), u.data(), t.data(), dur.data(), tst.data(), nullptr, nullptr, nullptr, 1) == MP_OK);
      for (int b = 0; b < B; ++b) EXPECT(tst[b] == 0);
      if (std::isfinite(dur[0]) && std::isfinite(dur[1]) && std::isfinite(dur[2])) {
        const double dt = plant(t, x, N);
        sample_all(model, "curve", N, dt, t, x, nullptr, nullptr, nullptr, bst.data(), bcnt.data(), pts.data(), cut.data(), knot.data(),
                   len.data(), Win, end);
      } else {
        std::printf("curve, N %d: the coarse grid's timing has an interior stop; the source is covered by the other grid\n", N);
      }
    }
  }
  for (int k = 0; k < 5; ++k) EXPECT(seen[k] > 0);
  // refused parameters and pointer groups
  {
    const int N = 3, M = 2;
    std::vector<double> t = {0.0, 0.5, 1.0}, x = {0.0, 4.0, 0.0}, q(N * n, 0.1), tab(4 * n, 0.0), len(1, 0.0);
    std::vector<int32_t> st(1), bst(1, 0), bcnt(1, 1);
    const double* Q = q.data();
    const double* Tb = tab.data();
    const double* Z = nullptr;
    const int32_t* ZI = nullptr;
    auto CALL = [&](int64_t BB, int64_t NN, const double* q0, const double* q1, const double* q2, const int32_t* s0, const int32_t* s1,
                    const double* p0, const double* p1, const double* p2, const double* p3, int64_t win, double dt, int64_t MM,
                    int32_t* out) {
      return mp_trajectory_sample_cpu_f64(model, t.data(), x.data(), BB, NN, q0, q1, q2, s0, s1, p0, p1, p2, p3, win, dt, MM, nullptr,
                                          nullptr, out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1);
    };
    EXPECT(CALL(1, N, Q, Q, Q, ZI, ZI, Z, Z, Z, Z, 0, 0.25, M, st.data()) == MP_OK && st[0] == MP_SAMPLE_TRUNCATED);
    EXPECT(CALL(1, N, Z, Z, Z, bst.data(), bcnt.data(), Tb, Tb, Tb, len.data(), 4, 0.25, M, st.data()) == MP_OK);
    EXPECT(CALL(0, N, Q, Q, Q, ZI, ZI, Z, Z, Z, Z, 0, 0.25, M, st.data()) == MP_OK);
    EXPECT(CALL(-1, N, Q, Q, Q, ZI, ZI, Z, Z, Z, Z, 0, 0.25, M, st.data()) == MP_ERR_INVALID);
    EXPECT(CALL(1, 2, Q, Q, Q, ZI, ZI, Z, Z, Z, Z, 0, 0.25, M, st.data()) == MP_ERR_INVALID);
    EXPECT(CALL(1, N, Q, Q, Q, ZI, ZI, Z, Z, Z, Z, 0, 0.0, M, st.data()) == MP_ERR_INVALID);
    EXPECT(CALL(1, N, Q, Q, Q, ZI, ZI, Z, Z, Z, Z, 0, -1.0, M, st.data()) == MP_ERR_INVALID);
    EXPECT(CALL(1, N, Q, Q, Q, ZI, ZI, Z, Z, Z, Z, 0, NAN, M, st.data()) == MP_ERR_INVALID);
    EXPECT(CALL(1, N, Q, Q, Q, ZI, ZI, Z, Z, Z, Z, 0, INFINITY, M, st.data()) == MP_ERR_INVALID);
    EXPECT(CALL(1, N, Q, Q, Q, ZI, ZI, Z, Z, Z, Z, 0, 0.25, 0, st.data()) == MP_ERR_INVALID);
    EXPECT(CALL(1, N, Q, Q, Q, ZI, ZI, Z, Z, Z, Z, 0, 0.25, (int64_t)1 << 31, st.data()) == MP_ERR_INVALID);
    EXPECT(CALL((int64_t)1 << 58, N, Q, Q, Q, ZI, ZI, Z, Z, Z, Z, 0, 0.25, M, st.data()) == MP_ERR_INVALID);
    EXPECT(CALL(1, N, Q, Z, Q, ZI, ZI, Z, Z, Z, Z, 0, 0.25, M, st.data()) == MP_ERR_INVALID);
    EXPECT(CALL(1, N, Z, Z, Z, ZI, ZI, Z, Z, Z, Z, 0, 0.25, M, st.data()) == MP_ERR_INVALID);
    EXPECT(CALL(1, N, Q, Q, Q, bst.data(), bcnt.data(), Tb, Tb, Tb, len.data(), 4, 0.25, M, st.data()) == MP_ERR_INVALID);
    EXPECT(CALL(1, N, Z, Z, Z, bst.data(), ZI, Tb, Tb, Tb, len.data(), 4, 0.25, M, st.data()) == MP_ERR_INVALID);
    EXPECT(CALL(1, N, Z, Z, Z, bst.data(), bcnt.data(), Tb, Tb, Tb, len.data(), 0, 0.25, M, st.data()) == MP_ERR_INVALID);
    EXPECT(CALL(1, N, Z, Z, Z, bst.data(), bcnt.data(), Tb, Tb, Tb, len.data(), 65537, 0.25, M, st.data()) == MP_ERR_INVALID);
    EXPECT(CALL(1, N, Q, Q, Q, ZI, ZI, Z, Z, Z, Z, 0, 0.25, M, nullptr) == MP_ERR_INVALID);
    EXPECT(mp_trajectory_sample_cpu_f64(model, nullptr, x.data(), 1, N, Q, Q, Q, ZI, ZI, Z, Z, Z, Z, 0, 0.25, M, nullptr, nullptr, st.data(), nullptr, nullptr,
                                        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1) == MP_ERR_INVALID);
    EXPECT(mp_trajectory_sample_cpu_f64(nullptr, t.data(), x.data(), 1, N, Q, Q, Q, ZI, ZI, Z, Z, Z, Z, 0, 0.25, M, nullptr, nullptr, st.data(), nullptr,
                                        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1) == MP_ERR_INVALID);
  }
  mp_collision_destroy(h);
  delete model;
  std::printf(fails ? "%d checks failed\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
