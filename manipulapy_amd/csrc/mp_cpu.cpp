// CPU twins of the hot-path entry points (include/manipula_hip.h, "*_cpu"): the SAME per-row templates the HIP
// kernels instantiate (mp_core.h), compiled for the host and run over the rows by a small std::thread pool.
// They are what the kernel registry's cpu_launchers call when the reference's own routing rule sends an operation to
// the CPU (NumPy backend active, or use_cuda=False): reference cuda_kernels/registry.py:85-89 picks
// `gpu_launcher if _cuda_routing_enabled() else cpu_launcher`.  They are NOT a fallback of the GPU path - a failing
// or missing GPU under the "hip" backend raises - and they are the product's own analytic recursion, not the test
// suite's restatement of the reference's 1 + 2n mass-matrix algorithm.  No HIP call is made here.
#include <sched.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/manipula_hip.h"
#include "mp_core.h"
#include "mp_deriv.h"
#include "mp_adjoint.h"
#include "mp_kin_vjp.h"
#include "mp_opspace.h"
#include "mp_dyn.h"
#include "mp_ik.h"
#include "mp_handles.h"
#include "mp_model_compile.h"
#include "mp_regressor.h"
#include "mp_rollout_vjp.h"
#include "mp_ilqr.h"
#include "mp_toppra.h"
#include "mp_collision.h"

namespace {
// Threads a launcher takes when the caller names none: every core this process may run on (its affinity mask) - but a container is
// often SHOWN more cores than it is granted time on (the MI355X boxes of this project: 256 visible, a cgroup quota of 16 CPUs), and
// one thread per visible core then loses to a fraction of them (the CPU baseline of bench.py: 256 threads 0.27 M rows/s, 64: 0.68): at
// most four threads per CPU of a cgroup quota (v2 cpu.max, v1 cfs_quota_us / cfs_period_us).
int default_threads() {
  static const int n = [] {
    int have = 0;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) have = CPU_COUNT(&set);
    if (have <= 0) have = (int)std::thread::hardware_concurrency();
    if (have <= 0) have = 1;
    double quota = 0;
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
      char q[32];
      long period = 0;
      if (std::fscanf(f, "%31s %ld", q, &period) == 2 && std::strcmp(q, "max") != 0 && period > 0) quota = std::atof(q) / (double)period;
      std::fclose(f);
    } else {
      long q = 0, period = 0;
      if (FILE* a = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (std::fscanf(a, "%ld", &q) != 1) q = 0; std::fclose(a); }
      if (FILE* b = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (std::fscanf(b, "%ld", &period) != 1) period = 0; std::fclose(b); }
      if (q > 0 && period > 0) quota = (double)q / (double)period;
    }
    if (quota > 0) have = std::min(have, std::max(1, (int)std::ceil(4.0 * quota)));
    return have;
  }();
  return n;
}
int thread_count(int64_t items, int64_t grain, int nthreads) {
  int want = nthreads;
  if (want <= 0) {
    if (const char* e = getenv("MANIPULAPY_CPU_THREADS")) want = atoi(e);
    if (want <= 0) want = default_threads();
  }
  const int64_t by_work = (items + grain - 1) / grain;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, by_work));
}

// fn(lo, hi) over [0, items) in contiguous slices, one per thread; small inputs stay on the calling thread.  A thread that
// cannot be started (std::system_error under a pid / thread limit) must not cross the C ABI as an exception: its slice, and
// every later one, runs on the calling thread instead, and the threads already started are joined either way.
template <class F>
int parallel_for(int64_t items, int64_t grain, int nthreads, F fn) {
  const int T = thread_count(items, grain, nthreads);
  if (T <= 1) { fn((int64_t)0, items); return 1; }
  std::vector<std::thread> pool;
  pool.reserve(T - 1);
  const int64_t per = (items + T - 1) / T;
  int started = 1;
  for (int t = 1; t < T; ++t) {
    const int64_t lo = std::min(items, t * per), hi = std::min(items, lo + per);
    if (lo >= hi) continue;
    bool spawned = false;
    try {
      pool.emplace_back([=] { fn(lo, hi); });
      spawned = true;
      ++started;
    } catch (...) {
    }
    if (!spawned) fn(lo, hi);
  }
  fn((int64_t)0, std::min(items, per));
  for (auto& th : pool) th.join();
  return started;
}

template <typename T>
MpCall<T> make_call(const mp_model* m, const double* g, const double* Ftip) {
  MpCall<double> cd;
  if (m->big) mp_make_call(m->bd, g ? g : kG, Ftip, &cd);
  else mp_make_call(m->d, g ? g : kG, Ftip, &cd);
  MpCall<T> c;
  mp_call_cast(cd, &c);
  // the float64 model for the re-evaluated float32 rows (mp_core.h, mp_rnea_row / mp_dyn.h, mp_dyn_row_id_f64)
  c.cold_model = m->big ? (const void*)&m->bd : (const void*)&m->d;
  return c;
}

#define MP_CPU_DISPATCH(n, ...)                                  \
  switch (n) {                                                   \
    case 1: { constexpr int N = 1; __VA_ARGS__; } break;         \
    case 2: { constexpr int N = 2; __VA_ARGS__; } break;         \
    case 3: { constexpr int N = 3; __VA_ARGS__; } break;         \
    case 4: { constexpr int N = 4; __VA_ARGS__; } break;         \
    case 5: { constexpr int N = 5; __VA_ARGS__; } break;         \
    case 6: { constexpr int N = 6; __VA_ARGS__; } break;         \
    case 7: { constexpr int N = 7; __VA_ARGS__; } break;         \
    case 8: { constexpr int N = 8; __VA_ARGS__; } break;         \
    default: return mp_fail(MP_ERR_INVALID, "dof outside 1..8 (larger models take the looped path before this dispatch)"); \
  }

// ---- one row of FK / Jacobian / inverse dynamics: the body of k_fk_jac_id / k_id on the host
template <typename T, int N, bool F>
void rows_fk_jac_id(const MpModel<T>& M, const MpCall<T>& C, const T* q, const T* qd, const T* qdd, T* Tout, T* Jout, T* tau,
                    int64_t lo, int64_t hi) {
  for (int64_t r = lo; r < hi; ++r) {
    T a[N];
    for (int j = 0; j < N; ++j) a[j] = q[r * N + j];
    MpJointState<T, N> js;
    mp_joint_state<T, N>(M, a, js);
    MpBad<T> bad;
    bad.add(a);
    if (Tout || Jout) {
      T TT[16], JJ[6 * N];
      mp_fk_jac<T, N, true>(M, js, TT, JJ);
      mp_poison_if(bad.any(), TT);
      mp_poison_if(bad.any(), JJ);
      if (Tout) std::memcpy(Tout + r * 16, TT, sizeof TT);
      if (Jout) std::memcpy(Jout + r * 6 * N, JJ, sizeof JJ);
    }
    if (tau) {
      T b[N], c[N], t[N];
      for (int j = 0; j < N; ++j) { b[j] = qd[r * N + j]; c[j] = qdd[r * N + j]; }
      mp_rnea_row<T, N, F>(M, C, js, a, b, c, t);
      for (int j = 0; j < N; ++j) t[j] = mp_clip(t[j], M.taumin[j], M.taumax[j]);
      bad.add(b); bad.add(c);
      mp_poison_if(bad.any(), t);
      std::memcpy(tau + r * N, t, sizeof t);
    }
  }
}

template <typename T>
int fk_jac_id_cpu(const char* fn, const mp_model* model, const T* q, const T* qd, const T* qdd, int64_t rows, const double* g,
                  const double* Ftip, T* Tout, T* Jout, T* tau, int nthreads) {
  REQUIRE(model, "null model");
  REQUIRE(rows >= 0, "negative row count");
  if (rows == 0) return MP_OK;
  REQUIRE(q && (Tout || Jout || tau) && (!tau || (qd && qdd)), "%s", fn);
  const MpModel<T>& M = pick<T>(model);
  const MpCall<T> C = make_call<T>(model, g, Ftip);
  const bool ftip = any_nonzero(Ftip);
  if (model->big) {  // 9..32 joints: the looped rows of csrc/mp_dyn.h
    const MpBigModel<T>& MB = pick_big<T>(model);
    parallel_for(rows, 128, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t r = lo; r < hi; ++r) {
        if (ftip) mp_dyn_row_fk_jac_id<MP_BIG_DOF, T, true>(MB, C, q, qd, qdd, Tout, Jout, tau, (long)r);
        else mp_dyn_row_fk_jac_id<MP_BIG_DOF, T, false>(MB, C, q, qd, qdd, Tout, Jout, tau, (long)r);
      }
    });
    return MP_OK;
  }
  MP_CPU_DISPATCH(M.n, {
    parallel_for(rows, 256, nthreads, [&](int64_t lo, int64_t hi) {
      if (ftip) rows_fk_jac_id<T, N, true>(M, C, q, qd, qdd, Tout, Jout, tau, lo, hi);
      else rows_fk_jac_id<T, N, false>(M, C, q, qd, qdd, Tout, Jout, tau, lo, hi);
    });
  })
  return MP_OK;
}

// ---- mass matrix / forward dynamics per row
template <typename T, int N>
void rows_mass_matrix(const MpModel<T>& M, const T* q, T* out, int64_t lo, int64_t hi) {
  for (int64_t r = lo; r < hi; ++r) {
    T a[N];
    for (int j = 0; j < N; ++j) a[j] = q[r * N + j];
    MpJointState<T, N> js;
    mp_joint_state<T, N>(M, a, js);
    T Mq[N][N];
    mp_mass_matrix_crba<T, N>(M, js, Mq);
    MpBad<T> bad;
    bad.add(a);
    for (int i = 0; i < N; ++i) {
      mp_poison_if(bad.any(), Mq[i]);
      std::memcpy(out + (r * N + i) * N, Mq[i], sizeof Mq[i]);
    }
  }
}

template <typename T, int N, bool F>
void rows_forward_dynamics(const MpModel<T>& M, const MpCall<T>& C, const T* q, const T* qd, const T* tau, T* qdd, int64_t lo,
                           int64_t hi) {
  const T tn[3] = {C.F1n[0], C.F1n[1], C.F1n[2]}, tf[3] = {C.F1f[0], C.F1f[1], C.F1f[2]};
  for (int64_t r = lo; r < hi; ++r) {
    T a[N], b[N], t[N], o[N];
    for (int j = 0; j < N; ++j) { a[j] = q[r * N + j]; b[j] = qd[r * N + j]; t[j] = tau[r * N + j]; }
    mp_forward_dynamics<T, N, F>(M, C.a0, tn, tf, a, b, t, o);
    MpBad<T> bad;
    bad.add(a); bad.add(b); bad.add(t);
    mp_poison_if(bad.any(), o);
    std::memcpy(qdd + r * N, o, sizeof o);
  }
}

// ---- forward_dynamics_trajectory: the body of k_fd_traj for trajectories [lo, hi)
template <typename T, int N, bool F>
void rollouts(const MpModel<T>& M, const MpCall<T>& C, const T* theta0, const T* dtheta0, const T* taumat, const T* Ftipmat,
              int64_t Nt, T h, int intRes, float* pos, float* vel, float* acc, int64_t lo, int64_t hi) {
  const float nanf_ = __builtin_bit_cast(float, 0x7fc00000u);
  for (int64_t b = lo; b < hi; ++b) {
    T q[N], qd[N];
    for (int j = 0; j < N; ++j) { q[j] = theta0[b * N + j]; qd[j] = dtheta0[b * N + j]; }
    MpBad<T> bad;
    bad.add(q); bad.add(qd);
    for (int64_t i = 0; i < Nt; ++i) {
      T last[N];
      for (int j = 0; j < N; ++j) last[j] = T(0);
      if (i > 0) {
        T tau[N], tn[3] = {T(0), T(0), T(0)}, tf[3] = {T(0), T(0), T(0)};
        for (int j = 0; j < N; ++j) tau[j] = taumat[(b * Nt + i) * N + j];
        bad.add(tau);
        if (F) {
          T W[6];
          for (int k = 0; k < 6; ++k) W[k] = Ftipmat[(b * Nt + i) * 6 + k];
          bad.add(W);
          mp_wrench_to_frame1(M, W, tn, tf);
        }
        for (int k = 0; k < intRes; ++k) {
          mp_forward_dynamics<T, N, F>(M, C.a0, tn, tf, q, qd, tau, last);
          for (int j = 0; j < N; ++j) {
            qd[j] = qd[j] + last[j] * h;
            q[j] = mp_clip(q[j] + qd[j] * h, M.qmin[j], M.qmax[j]);
          }
        }
        bad.add(qd);
      }
      const bool poison = i > 0 && bad.any();
      for (int j = 0; j < N; ++j) {
        const int64_t o = (b * Nt + i) * N + j;
        pos[o] = poison ? nanf_ : (float)q[j];
        vel[o] = poison ? nanf_ : (float)qd[j];
        acc[o] = poison ? nanf_ : (float)last[j];
      }
    }
  }
}

template <typename T>
int fd_trajectory_cpu(const mp_model* model, const T* theta0, const T* dtheta0, const T* taumat, const T* Ftipmat, int64_t B,
                      int64_t Nt, const double* g, double dt, int intRes, float* pos, float* vel, float* acc, int nthreads) {
  REQUIRE(model, "null model");
  REQUIRE(B >= 0 && Nt >= 0, "negative trajectory / step count");
  if (B == 0 || Nt == 0) return MP_OK;
  REQUIRE(intRes >= 1, "intRes must be >= 1");
  REQUIRE(theta0 && dtheta0 && taumat && pos && vel && acc, "null pointer");
  const MpModel<T>& M = pick<T>(model);
  const MpCall<T> C = make_call<T>(model, g, nullptr);
  const T h = (T)(dt / intRes);
  if (model->big) {
    const MpBigModel<T>& MB = pick_big<T>(model);
    parallel_for(B, 1, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t b = lo; b < hi; ++b) {
        if (Ftipmat) mp_dyn_rollout<MP_BIG_DOF, T, true>(MB, C, theta0, dtheta0, taumat, Ftipmat, (long)b, (long)B, (long)Nt, h, intRes, pos, vel, acc, false);
        else mp_dyn_rollout<MP_BIG_DOF, T, false>(MB, C, theta0, dtheta0, taumat, Ftipmat, (long)b, (long)B, (long)Nt, h, intRes, pos, vel, acc, false);
      }
    });
    return MP_OK;
  }
  MP_CPU_DISPATCH(M.n, {
    parallel_for(B, 1, nthreads, [&](int64_t lo, int64_t hi) {
      if (Ftipmat) rollouts<T, N, true>(M, C, theta0, dtheta0, taumat, Ftipmat, Nt, h, intRes, pos, vel, acc, lo, hi);
      else rollouts<T, N, false>(M, C, theta0, dtheta0, taumat, Ftipmat, Nt, h, intRes, pos, vel, acc, lo, hi);
    });
  })
  return MP_OK;
}
}  // namespace

// ---- the argument checks that the twins below share with the entries of a context (mp_handles.h); the sphere-model families'
// stand further down, beside their twins
int mp_opspace_check(const char* fn, int frame, int task, double damping, int64_t rows) {
  REQUIRE(frame >= 0 && frame <= 2, "%s: frame must be 0 (space), 1 (body) or 2 (hybrid), got %d", fn, frame);
  REQUIRE(task >= 0 && task <= 2, "%s: task must be 0 (full), 1 (linear) or 2 (angular), got %d", fn, task);
  REQUIRE(std::isfinite(damping) && damping >= 0.0, "%s: damping must be finite and >= 0", fn);
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  return MP_OK;
}
int mp_kin_vjp_check(const char* fn, int frame, int64_t rows) {
  REQUIRE(frame == 0 || frame == 1, "%s: frame must be 0 (space) or 1 (body), got %d", fn, frame);
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  return MP_OK;
}
int mp_regressor_check(const char* fn, int64_t rows) {
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  return MP_OK;
}
int mp_ilqr_weights_check(const char* fn, int n, const double* wq, const double* wr, const double* wf) {
  REQUIRE(wq && wr && wf, "%s: null weight vector", fn);
  for (int j = 0; j < 2 * n; ++j) REQUIRE(std::isfinite(wq[j]) && std::isfinite(wf[j]) && std::isfinite(wr[j / 2]), "%s: non-finite weight", fn);
  return MP_OK;
}
int mp_toppra_vmax_check(const char* fn, int n, const double* vlim, MpToppraVmax* out) {
  REQUIRE(vlim, "%s: null velocity limits", fn);
  std::memset(out, 0, sizeof *out);
  for (int j = 0; j < n; ++j) {
    REQUIRE(std::isfinite(vlim[j]) && vlim[j] > 0.0, "%s: velocity limits must be finite and positive", fn);
    out->v[j] = vlim[j];
  }
  return MP_OK;
}
int mp_toppra_limits_check(const char* fn, int n, const double* tlim, const double* alim, MpToppraLimits* out) {
  std::memset(out, 0, sizeof *out);
  for (int j = 0; j < n; ++j) {
    out->tau_lo[j] = tlim ? tlim[2 * j] : -INFINITY;
    out->tau_hi[j] = tlim ? tlim[2 * j + 1] : INFINITY;
    out->amax[j] = alim ? alim[j] : INFINITY;
    REQUIRE(!std::isnan(out->tau_lo[j]) && !std::isnan(out->tau_hi[j]) && out->tau_lo[j] <= out->tau_hi[j],
            "%s: torque limits must be ordered pairs (lo <= hi, either may be infinite)", fn);
    REQUIRE(out->amax[j] > 0.0, "%s: acceleration limits must be positive", fn);
  }
  return MP_OK;
}

extern "C" {

int mp_cpu_threads(int64_t items) { return thread_count(items, 1, 0); }

int mp_id_trajectory_cpu_f32(const mp_model* model, const float* q, const float* qd, const float* qdd, int64_t rows,
                             const double* g, const double* Ftip, float* tau, int nthreads) {
  REQUIRE(rows <= 0 || tau, "mp_id_trajectory_cpu_f32: null tau");
  return fk_jac_id_cpu<float>("mp_id_trajectory_cpu_f32: null pointer", model, q, qd, qdd, rows, g, Ftip, nullptr, nullptr, tau, nthreads);
}
int mp_id_trajectory_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* qdd, int64_t rows,
                             const double* g, const double* Ftip, double* tau, int nthreads) {
  REQUIRE(rows <= 0 || tau, "mp_id_trajectory_cpu_f64: null tau");
  return fk_jac_id_cpu<double>("mp_id_trajectory_cpu_f64: null pointer", model, q, qd, qdd, rows, g, Ftip, nullptr, nullptr, tau, nthreads);
}
// which rows the float32 inverse-dynamics kernels evaluate in float64 (mp_core.h, mp_id_row_is_hard): 1 per such row
int mp_id_row_precision_cpu_f32(const mp_model* model, const float* q, const float* qd, const float* qdd, int64_t rows,
                                const double* g, const double* Ftip, uint8_t* in_f64, int nthreads) {
  REQUIRE(model, "mp_id_row_precision_cpu_f32: null model");
  REQUIRE(rows >= 0, "mp_id_row_precision_cpu_f32: negative row count");
  if (rows == 0) return MP_OK;
  REQUIRE(q && qd && qdd && in_f64, "mp_id_row_precision_cpu_f32: null pointer");
  const MpModel<float>& M = model->f;
  const MpCall<float> C = make_call<float>(model, g, Ftip);
  const bool ftip = any_nonzero(Ftip);
  if (model->big) {  // 9..32 joints: the same verdict from the looped recursion (mp_dyn.h)
    const MpBigModel<float>& MB = model->bf;
    const int n = MB.n;
    parallel_for(rows, 128, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t r = lo; r < hi; ++r) {
        float t[MP_BIG_DOF], scale = 0.0f;
        MpDynState<float, MP_BIG_DOF> js;
        mp_dyn_joint_state<float>(MB, n, q + r * n, js);
        if (ftip) mp_dyn_rnea<float, true>(MB, n, C.a0, C.F1n, C.F1f, js, qd + r * n, qdd + r * n, t, &scale);
        else mp_dyn_rnea<float, false>(MB, n, C.a0, C.F1n, C.F1f, js, qd + r * n, qdd + r * n, t, &scale);
        in_f64[r] = mp_dyn_row_is_hard(t, n, scale) ? 1 : 0;
      }
    });
    return MP_OK;
  }
  MP_CPU_DISPATCH(M.n, {
    parallel_for(rows, 256, nthreads, [&](int64_t lo, int64_t hi) {
      const float tn[3] = {C.F1n[0], C.F1n[1], C.F1n[2]}, tf[3] = {C.F1f[0], C.F1f[1], C.F1f[2]};
      for (int64_t r = lo; r < hi; ++r) {
        float a[N], b[N], c[N], t[N];
        for (int j = 0; j < N; ++j) { a[j] = q[r * N + j]; b[j] = qd[r * N + j]; c[j] = qdd[r * N + j]; }
        MpJointState<float, N> js;
        mp_joint_state<float, N>(M, a, js);
        MpRowScale<float, N> sc;
        if (ftip) mp_rnea_impl<float, N, true>(M, C.a0, tn, tf, js, b, c, t, sc);
        else mp_rnea_impl<float, N, false>(M, C.a0, tn, tf, js, b, c, t, sc);
        in_f64[r] = mp_id_row_is_hard<N>(t, sc.scale(M.lscale)) ? 1 : 0;
      }
    });
  })
  return MP_OK;
}
int mp_fk_jac_id_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* qdd, int64_t rows,
                         const double* g, const double* Ftip, double* T, double* J, double* tau, int nthreads) {
  return fk_jac_id_cpu<double>("mp_fk_jac_id_cpu_f64: null pointer / no output / tau without qd, qdd", model, q, qd, qdd, rows, g,
                               Ftip, T, J, tau, nthreads);
}

int mp_mass_matrix_cpu_f64(const mp_model* model, const double* q, int64_t rows, double* Mout, int nthreads) {
  REQUIRE(model, "mp_mass_matrix_cpu_f64: null model");
  REQUIRE(rows >= 0, "mp_mass_matrix_cpu_f64: negative row count");
  if (rows == 0) return MP_OK;
  REQUIRE(q && Mout, "mp_mass_matrix_cpu_f64: null pointer");
  const MpModel<double>& M = model->d;
  if (model->big) {
    parallel_for(rows, 128, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t r = lo; r < hi; ++r) mp_dyn_row_mass_matrix<MP_BIG_DOF, double>(model->bd, q, Mout, (long)r);
    });
    return MP_OK;
  }
  MP_CPU_DISPATCH(M.n, { parallel_for(rows, 256, nthreads, [&](int64_t lo, int64_t hi) { rows_mass_matrix<double, N>(M, q, Mout, lo, hi); }); })
  return MP_OK;
}

int mp_forward_dynamics_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* tau, int64_t rows,
                                const double* g, const double* Ftip, double* qdd, int nthreads) {
  REQUIRE(model, "mp_forward_dynamics_cpu_f64: null model");
  REQUIRE(rows >= 0, "mp_forward_dynamics_cpu_f64: negative row count");
  if (rows == 0) return MP_OK;
  REQUIRE(q && qd && tau && qdd, "mp_forward_dynamics_cpu_f64: null pointer");
  const MpModel<double>& M = model->d;
  const MpCall<double> C = make_call<double>(model, g, Ftip);
  const bool ftip = any_nonzero(Ftip);
  if (model->big) {
    parallel_for(rows, 64, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t r = lo; r < hi; ++r) {
        if (ftip) mp_dyn_row_forward_dynamics<MP_BIG_DOF, double, true>(model->bd, C, q, qd, tau, qdd, (long)r);
        else mp_dyn_row_forward_dynamics<MP_BIG_DOF, double, false>(model->bd, C, q, qd, tau, qdd, (long)r);
      }
    });
    return MP_OK;
  }
  MP_CPU_DISPATCH(M.n, {
    parallel_for(rows, 128, nthreads, [&](int64_t lo, int64_t hi) {
      if (ftip) rows_forward_dynamics<double, N, true>(M, C, q, qd, tau, qdd, lo, hi);
      else rows_forward_dynamics<double, N, false>(M, C, q, qd, tau, qdd, lo, hi);
    });
  })
  return MP_OK;
}

// analytical derivatives (mp_deriv.h): the kernels' per-row code over host rows
static int deriv_cpu(const char* fn, bool fd, const mp_model* model, const double* q, const double* qd, const double* x, int64_t rows,
                     const double* g, const double* Ftip, double* y, double* dq, double* dqd, double* mat, int nthreads) {
  if (int rc = mp_small_model(fn, model)) return rc;
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  if (rows == 0) return MP_OK;
  REQUIRE(q && qd && x && dq && dqd, "%s: null pointer", fn);
  const MpModel<double>& M = model->d;
  const MpCall<double> C = make_call<double>(model, g, Ftip);
  const bool ftip = any_nonzero(Ftip);
  MP_CPU_DISPATCH(M.n, {
    parallel_for(rows, 64, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t r = lo; r < hi; ++r) {
        if (fd) {
          if (ftip) mp_fd_deriv_row<N, true>(M, C, q, qd, x, y, dq, dqd, mat, (long)r);
          else mp_fd_deriv_row<N, false>(M, C, q, qd, x, y, dq, dqd, mat, (long)r);
        } else {
          if (ftip) mp_id_deriv_row<N, true>(M, C, q, qd, x, y, dq, dqd, mat, (long)r);
          else mp_id_deriv_row<N, false>(M, C, q, qd, x, y, dq, dqd, mat, (long)r);
        }
      }
    });
  })
  return MP_OK;
}
int mp_id_derivatives_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* qdd, int64_t rows,
                              const double* g, const double* Ftip, double* tau, double* dtau_dq, double* dtau_dqd, double* M,
                              int nthreads) {
  return deriv_cpu("mp_id_derivatives_cpu_f64", false, model, q, qd, qdd, rows, g, Ftip, tau, dtau_dq, dtau_dqd, M, nthreads);
}
int mp_fd_derivatives_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* tau, int64_t rows,
                              const double* g, const double* Ftip, double* qdd, double* dqdd_dq, double* dqdd_dqd, double* Minv,
                              int nthreads) {
  return deriv_cpu("mp_fd_derivatives_cpu_f64", true, model, q, qd, tau, rows, g, Ftip, qdd, dqdd_dq, dqdd_dqd, Minv, nthreads);
}
// vector-Jacobian products (mp_adjoint.h): the kernels' per-row code over host rows.  x = qdd (ID) / tau (FD), cot = the cotangent;
// ID: o1 = gq, o2 = gqd, o3 = gqdd (may be null), y unused;  FD: y = qdd (may be null), o1 = gq, o2 = gqd, o3 = gtau (may be null)
static int vjp_cpu(const char* fn, bool fd, const mp_model* model, const double* q, const double* qd, const double* x, const double* cot,
                   int64_t rows, const double* g, const double* Ftip, double* y, double* o1, double* o2, double* o3, int nthreads) {
  if (int rc = mp_small_model(fn, model)) return rc;
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  if (rows == 0) return MP_OK;
  REQUIRE(q && qd && x && cot && o1 && o2, "%s: null pointer", fn);
  const MpModel<double>& M = model->d;
  const MpCall<double> C = make_call<double>(model, g, Ftip);
  const bool ftip = any_nonzero(Ftip);
  MP_CPU_DISPATCH(M.n, {
    parallel_for(rows, 128, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t r = lo; r < hi; ++r) {
        if (fd) {
          if (ftip) mp_fd_vjp_row<N, true>(M, C, q, qd, x, cot, y, o1, o2, o3, (long)r);
          else mp_fd_vjp_row<N, false>(M, C, q, qd, x, cot, y, o1, o2, o3, (long)r);
        } else {
          if (ftip) mp_id_vjp_row<N, true>(M, C, q, qd, x, cot, o1, o2, o3, (long)r);
          else mp_id_vjp_row<N, false>(M, C, q, qd, x, cot, o1, o2, o3, (long)r);
        }
      }
    });
  })
  return MP_OK;
}
int mp_id_vjp_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* qdd, const double* gtau, int64_t rows,
                      const double* g, const double* Ftip, double* gq, double* gqd, double* gqdd, int nthreads) {
  return vjp_cpu("mp_id_vjp_cpu_f64", false, model, q, qd, qdd, gtau, rows, g, Ftip, nullptr, gq, gqd, gqdd, nthreads);
}
int mp_fd_vjp_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* tau, const double* gqdd, int64_t rows,
                      const double* g, const double* Ftip, double* qdd, double* gq, double* gqd, double* gtau, int nthreads) {
  return vjp_cpu("mp_fd_vjp_cpu_f64", true, model, q, qd, tau, gqdd, rows, g, Ftip, qdd, gq, gqd, gtau, nthreads);
}
// reverse mode through FK + Jacobian (mp_kin_vjp.h): the kernel's per-row code over host rows; frame 0 = space, 1 = body
int mp_fk_jac_vjp_cpu_f64(const mp_model* model, int frame, const double* q, const double* gT, const double* gJ, int64_t rows,
                          double* T, double* J, double* gq, int nthreads) {
  const char* fn = "mp_fk_jac_vjp_cpu_f64";
  if (int rc = mp_small_model(fn, model)) return rc;
  if (int rc = mp_kin_vjp_check(fn, frame, rows)) return rc;
  if (rows == 0) return MP_OK;
  REQUIRE(q, "%s: null pointer", fn);
  REQUIRE(T || J || gq, "%s: at least one output is required", fn);
  const MpModel<double>& M = model->d;
  MP_CPU_DISPATCH(M.n, {
    parallel_for(rows, 256, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t r = lo; r < hi; ++r) {
        if (frame == 0) mp_fk_jac_vjp_row<double, N, 0>(M, q, gT, gJ, T, J, gq, (long)r);
        else mp_fk_jac_vjp_row<double, N, 1>(M, q, gT, gJ, T, J, gq, (long)r);
      }
    });
  })
  return MP_OK;
}
// operational-space dynamics and task-space torque (mp_opspace.h): the kernels' per-row code over host rows
int mp_opspace_cpu_f64(const mp_model* model, int frame, int task, double damping, const double* q, const double* qd, int64_t rows,
                       const double* g, double* T, double* J, double* Jdqd, double* Lambda, double* Jbar, double* mu, double* p,
                       int nthreads) {
  const char* fn = "mp_opspace_cpu_f64";
  if (int rc = mp_small_model(fn, model)) return rc;
  if (int rc = mp_opspace_check(fn, frame, task, damping, rows)) return rc;
  if (rows == 0) return MP_OK;
  REQUIRE(q && qd, "%s: null pointer", fn);
  REQUIRE(T || J || Jdqd || Lambda || Jbar || mu || p, "%s: at least one output is required", fn);
  const MpModel<double>& M = model->d;
  const MpCall<double> C = make_call<double>(model, g, nullptr);
  const double lam2 = damping * damping;
  MP_CPU_DISPATCH(M.n, {
    parallel_for(rows, 64, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t r = lo; r < hi; ++r) mp_opspace_cpu_row<N>(M, C, frame, task, lam2, q, qd, T, J, Jdqd, Lambda, Jbar, mu, p, (long)r);
    });
  })
  return MP_OK;
}
int mp_opspace_torque_cpu_f64(const mp_model* model, int frame, int task, double damping, const double* q, const double* qd,
                              const double* acc, const double* tau0, int64_t rows, const double* g, double* tau, int nthreads) {
  const char* fn = "mp_opspace_torque_cpu_f64";
  if (int rc = mp_small_model(fn, model)) return rc;
  if (int rc = mp_opspace_check(fn, frame, task, damping, rows)) return rc;
  if (rows == 0) return MP_OK;
  REQUIRE(q && qd && acc && tau, "%s: null pointer", fn);
  const MpModel<double>& M = model->d;
  const MpCall<double> C = make_call<double>(model, g, nullptr);
  const double lam2 = damping * damping;
  MP_CPU_DISPATCH(M.n, {
    parallel_for(rows, 64, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t r = lo; r < hi; ++r) mp_opspace_torque_cpu_row<N>(M, C, frame, task, lam2, q, qd, acc, tau0, tau, (long)r);
    });
  })
  return MP_OK;
}
// dynamics regressor (mp_regressor.h): the kernels' per-row code over host rows
int mp_id_regressor_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* qdd, int64_t rows, const double* g,
                            const double* Ftip, double* Y, double* tau_ext, int nthreads) {
  const char* fn = "mp_id_regressor_cpu_f64";
  if (int rc = mp_small_model(fn, model)) return rc;
  if (int rc = mp_regressor_check(fn, rows)) return rc;
  if (rows == 0) return MP_OK;
  REQUIRE(q && qd && qdd && Y, "%s: null pointer", fn);
  const MpModel<double>& M = model->d;
  const MpCall<double> C = make_call<double>(model, g, Ftip);
  const bool ftip = any_nonzero(Ftip);
  MP_CPU_DISPATCH(M.n, {
    parallel_for(rows, 64, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t r = lo; r < hi; ++r) {
        if (ftip) mp_id_regressor_row<N, true>(M, model->pmap, C, q, qd, qdd, Y, tau_ext, (long)r);
        else mp_id_regressor_row<N, false>(M, model->pmap, C, q, qd, qdd, Y, tau_ext, (long)r);
      }
    });
  })
  return MP_OK;
}
// Normal equations: the rows are cut into a number of chunks fixed by the row count alone (never by the thread count); each chunk
// sums its rows in order, then the chunks are added in order - repeat calls are bit-identical.  Only A's upper triangle is summed
// and then mirrored.
int mp_id_regressor_normal_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* qdd, const double* rhs,
                                   int64_t rows, const double* g, const double* Ftip, double* A, double* b, double* rr, int nthreads) {
  const char* fn = "mp_id_regressor_normal_cpu_f64";
  if (int rc = mp_small_model(fn, model)) return rc;
  if (int rc = mp_regressor_check(fn, rows)) return rc;
  REQUIRE(b && rr && (rows == 0 || (q && qd && qdd && rhs)), "%s: null pointer", fn);
  const MpModel<double>& M = model->d;
  const int W = MP_REG_P * M.n;
  const int64_t chunks = std::min<int64_t>(256, (rows + 63) / 64), per = chunks ? (rows + chunks - 1) / chunks : 0;
  const size_t stride = (size_t)W * W + W + 1;
  std::vector<double> part((size_t)chunks * stride, 0.0);
  const MpCall<double> C = make_call<double>(model, g, Ftip);
  const bool ftip = any_nonzero(Ftip);
  const bool with_a = A != nullptr;
  MP_CPU_DISPATCH(M.n, {
    parallel_for(chunks, 1, nthreads, [&](int64_t lo, int64_t hi) {
      constexpr int WN = MP_REG_P * N;
      double y[N][WN], res[N];
      auto put = [&](int j, int col, double v) { y[j][col] = v; };
      auto rs = [&](int j, double v) { res[j] = v; };
      for (int64_t ch = lo; ch < hi; ++ch) {
        double* P = part.data() + (size_t)ch * stride;
        for (int64_t r = ch * per; r < std::min(rows, (ch + 1) * per); ++r) {
          if (ftip) mp_id_regressor_normal_part<N, true, 1>(M, model->pmap, C, q, qd, qdd, rhs, (long)r, 0, put, rs);
          else mp_id_regressor_normal_part<N, false, 1>(M, model->pmap, C, q, qd, qdd, rhs, (long)r, 0, put, rs);
          for (int j = 0; j < N; ++j) {
            if (with_a)
              for (int a = 0; a < WN; ++a)
                for (int c = a; c < WN; ++c) P[a * WN + c] += y[j][a] * y[j][c];
            for (int a = 0; a < WN; ++a) P[WN * WN + a] += y[j][a] * res[j];
            P[WN * WN + WN] += res[j] * res[j];
          }
        }
      }
    });
  })
  for (size_t e = 0; e < stride; ++e) {
    double v = 0.0;
    for (int64_t ch = 0; ch < chunks; ++ch) v += part[(size_t)ch * stride + e];
    const size_t ww = (size_t)W * W;
    if (e < ww) {
      const size_t i = e / W, j = e % W;
      if (with_a && i <= j) { A[e] = v; A[j * W + i] = v; }
    } else if (e < ww + W) b[e - ww] = v;
    else rr[0] = v;
  }
  return MP_OK;
}
// reverse mode through the roll-out (mp_rollout_vjp.h): the kernel's per-trajectory code over batch-major host arrays, each thread
// with its own workspace of (N + intRes) 2n doubles
int mp_fd_trajectory_vjp_cpu_f64(const mp_model* model, const double* theta0, const double* dtheta0, const double* taumat,
                                 const double* Ftipmat, int64_t B, int64_t Nt, const double* g, double dt, int intRes, const double* gpos,
                                 const double* gvel, const double* gacc, double* gtheta0, double* gdtheta0, double* gtaumat,
                                 int nthreads) {
  const char* fn = "mp_fd_trajectory_vjp_cpu_f64";
  if (int rc = mp_small_model(fn, model)) return rc;
  REQUIRE(B >= 0 && Nt >= 0, "%s: negative B or N", fn);
  REQUIRE(intRes >= 1, "%s: intRes must be >= 1 (got %d)", fn, intRes);
  if (B == 0 || Nt == 0) return MP_OK;
  REQUIRE(theta0 && dtheta0 && taumat && gtheta0 && gdtheta0 && gtaumat, "%s: null pointer", fn);
  const MpModel<double>& M = model->d;
  const MpCall<double> C = make_call<double>(model, g, nullptr);
  const double h = dt / intRes;
  MP_CPU_DISPATCH(M.n, {
    parallel_for(B, 1, nthreads, [&](int64_t lo, int64_t hi) {
      std::vector<double> work((size_t)(Nt + intRes) * 2 * N);
      double *ck = work.data(), *sub = ck + (size_t)Nt * 2 * N;
      for (int64_t b = lo; b < hi; ++b) {
        const int64_t o = b * Nt * N, s = b * N;  // (B, N, n) row 0 / (B, n) row of trajectory b
        const double* F = Ftipmat ? Ftipmat + b * Nt * 6 : nullptr;
        const double *gp = gpos ? gpos + o : nullptr, *gv = gvel ? gvel + o : nullptr, *ga = gacc ? gacc + o : nullptr;
        if (F) mp_fd_traj_vjp<N, true>(M, C, theta0 + s, dtheta0 + s, taumat + o, F, 1, (long)Nt, h, intRes, gp, gv, ga, ck, 1, sub, 1,
                                       gtheta0 + s, gdtheta0 + s, gtaumat + o);
        else mp_fd_traj_vjp<N, false>(M, C, theta0 + s, dtheta0 + s, taumat + o, nullptr, 1, (long)Nt, h, intRes, gp, gv, ga, ck, 1, sub, 1,
                                      gtheta0 + s, gdtheta0 + s, gtaumat + o);
      }
    });
  })
  return MP_OK;
}
// batched iLQR (mp_ilqr.h): the kernels' per-trajectory code over batch-major host arrays.  The backward twin forms the derivative
// blocks of its trajectory itself (mp_fd_deriv_row over rows (pos[0:N-1], vel[0:N-1], tau[1:N])), each thread with its own workspace.
static int ilqr_cpu_check(const char* fn, const mp_model* model, int64_t B, int64_t Nt, const double* wq, const double* wr,
                          const double* wf) {
  if (int rc = mp_small_model(fn, model)) return rc;
  REQUIRE(B >= 0, "%s: negative B", fn);
  REQUIRE(Nt >= 2, "%s: N must be >= 2 (got %lld)", fn, (long long)Nt);
  return mp_ilqr_weights_check(fn, model->d.n, wq, wr, wf);
}
int mp_ilqr_backward_cpu_f64(const mp_model* model, const double* pos, const double* vel, const double* taumat, const double* xref,
                             const double* wq, const double* wr, const double* wf, const double* reg, int64_t B, int64_t Nt,
                             const double* g, double dt, double* K, double* k, double* dV, int32_t* status, int nthreads) {
  const char* fn = "mp_ilqr_backward_cpu_f64";
  if (int rc = ilqr_cpu_check(fn, model, B, Nt, wq, wr, wf)) return rc;
  if (B == 0) return MP_OK;
  REQUIRE(pos && vel && taumat && xref && reg && K && k && dV && status, "%s: null pointer", fn);
  const MpModel<double>& M = model->d;
  const MpCall<double> C = make_call<double>(model, g, nullptr);
  // MANIPULAPY_ILQR_CPU_FORM=coop (read at every call): the cooperative form of the device kernel, lane by lane, instead of the
  // one-lane-per-trajectory form - for tests of that form without a GPU
  const char* form = getenv("MANIPULAPY_ILQR_CPU_FORM");
  const bool coop = form && std::strcmp(form, "coop") == 0;
  MP_CPU_DISPATCH(M.n, {
    parallel_for(B, 1, nthreads, [&](int64_t lo, int64_t hi) {
      const size_t blk = (size_t)(Nt - 1) * N * N;
      std::vector<double> buf(3 * blk + (size_t)mp_ilqr_work_doubles(N));
      double *dq = buf.data(), *dqd = dq + blk, *mi = dqd + blk, *work = mi + blk;
      for (int64_t b = lo; b < hi; ++b) {
        const int64_t o = b * Nt * N;
        for (int64_t r = 0; r + 1 < Nt; ++r)
          mp_fd_deriv_row<N, false>(M, C, pos + o, vel + o, taumat + o + N, nullptr, dq, dqd, mi, (long)r);
        int st = 0;
        if (coop) {   // the device's cooperative form, its 16 lanes run in turn phase by phase
          const MpIlqrArgs A{pos + o, vel + o, taumat + o, 1, (long)Nt, dt, dq, dqd, mi, 1, xref + 2 * o, 1, wq, wr, wf, reg[b],
                             K + 2 * o * N, k + o, 1, dV + 2 * b, &st, true};
          mp_ilqr_backward_coop_host<N>(M, A);
        } else {
          mp_ilqr_backward<N>(M, pos + o, vel + o, taumat + o, 1, (long)Nt, dt, dq, dqd, mi, 1, xref + 2 * o, 1, wq, wr, wf, reg[b], work, 1,
                              K + 2 * o * N, k + o, 1, dV + 2 * b, &st);
        }
        status[b] = st;
      }
    });
  })
  return MP_OK;
}
int mp_ilqr_rollout_cpu_f64(const mp_model* model, const double* theta0, const double* dtheta0, const double* taumat, const double* pos,
                            const double* vel, const double* K, const double* k, const double* alpha, const double* xref,
                            const double* wq, const double* wr, const double* wf, int64_t A, int64_t B, int64_t Nt, const double* g,
                            double dt, double* cost, double* opos, double* ovel, double* otau, int nthreads) {
  const char* fn = "mp_ilqr_rollout_cpu_f64";
  if (int rc = ilqr_cpu_check(fn, model, B, Nt, wq, wr, wf)) return rc;
  REQUIRE(A >= 0, "%s: negative A", fn);
  if (A == 0 || B == 0) return MP_OK;
  REQUIRE(theta0 && dtheta0 && taumat && alpha && xref && cost, "%s: null pointer", fn);
  REQUIRE((K != nullptr) == (k != nullptr) && (!K || (pos && vel)),
          "%s: K and k must both be given, with the nominal pos and vel, or both be null", fn);
  REQUIRE((opos != nullptr) == (ovel != nullptr) && (opos != nullptr) == (otau != nullptr),
          "%s: the three row outputs must all be given or all be null", fn);
  const MpModel<double>& M = model->d;
  const MpCall<double> C = make_call<double>(model, g, nullptr);
  MP_CPU_DISPATCH(M.n, {
    parallel_for(A * B, 1, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t l = lo; l < hi; ++l) {
        const int64_t b = l % B, o = b * Nt * N, lo_ = l * Nt * N;
        mp_ilqr_rollout<N>(M, C, theta0 + b * N, dtheta0 + b * N, taumat + o, K ? pos + o : nullptr, K ? vel + o : nullptr, 1,
                           K ? K + 2 * o * N : nullptr, K ? k + o : nullptr, 1, alpha[l], xref + 2 * o, 1, wq, wr, wf, (long)Nt, dt,
                           cost + l, opos ? opos + lo_ : nullptr, opos ? ovel + lo_ : nullptr, opos ? otau + lo_ : nullptr, 1);
      }
    });
  })
  return MP_OK;
}
// time-optimal path parameterisation (mp_toppra.h): the kernels' per-row and per-path code over batch-major host arrays
int mp_path_dynamics_cpu_f64(const mp_model* model, const double* q, const double* dq, const double* ddq, int64_t rows,
                             const double* velocity_limits, const double* g, const double* Ftip, double* a, double* b, double* c,
                             double* xbar, int nthreads) {
  const char* fn = "mp_path_dynamics_cpu_f64";
  if (int rc = mp_small_model(fn, model)) return rc;
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  MpToppraVmax V;
  if (int rc = mp_toppra_vmax_check(fn, model->d.n, velocity_limits, &V)) return rc;
  if (rows == 0) return MP_OK;
  REQUIRE(q && dq && ddq && a && b && c && xbar, "%s: null pointer", fn);
  const MpModel<double>& M = model->d;
  const MpCall<double> C = make_call<double>(model, g, Ftip);
  const bool ftip = any_nonzero(Ftip);
  MP_CPU_DISPATCH(M.n, {
    parallel_for(rows, 256, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t r = lo; r < hi; ++r) {
        if (ftip) mp_path_coeffs_row<N, true>(M, C, V, q, dq, ddq, a, b, c, xbar, (long)r);
        else mp_path_coeffs_row<N, false>(M, C, V, q, dq, ddq, a, b, c, xbar, (long)r);
      }
    });
  })
  return MP_OK;
}
// the sweep alone on given coefficients (batch-major (B, N, n) / (B, N)); qd / qdd / tau all or none
int mp_toppra_sweep_cpu_f64(int n, const double* a, const double* b, const double* c, const double* xbar, const double* dq,
                            const double* ddq, const double* torque_limits, const double* acceleration_limits, const double* sd_start,
                            const double* sd_end, int64_t B, int64_t Nt, double* K, double* x, double* u, double* t, double* duration,
                            int32_t* status, double* qd, double* qdd, double* tau, int nthreads) {
  const char* fn = "mp_toppra_sweep_cpu_f64";
  if (n < 1 || n > MP_MAX_DOF) return mp_fail(MP_ERR_UNSUPPORTED, "%s: n must be 1..%d", fn, MP_MAX_DOF);
  REQUIRE(B >= 0, "%s: negative B", fn);
  REQUIRE(Nt >= 3, "%s: N must be >= 3 (got %lld)", fn, (long long)Nt);
  MpToppraLimits L;
  if (int rc = mp_toppra_limits_check(fn, n, torque_limits, acceleration_limits, &L)) return rc;
  if (B == 0) return MP_OK;
  REQUIRE(a && b && c && xbar && sd_start && sd_end && K && x && u && t && duration && status, "%s: null pointer", fn);
  REQUIRE((qd != nullptr) == (qdd != nullptr) && (qd != nullptr) == (tau != nullptr),
          "%s: the three row outputs must all be given or all be null", fn);
  REQUIRE(!(acceleration_limits || tau) || (dq && ddq), "%s: acceleration limits and the row outputs need the path derivatives dq and ddq", fn);
  const bool acc = acceleration_limits != nullptr;
  MP_CPU_DISPATCH(n, {
    parallel_for(B, 1, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t p = lo; p < hi; ++p) {
        const int64_t o = p * Nt * N, s = p * Nt;
        int st = 0;
        if (acc)
          mp_toppra_sweep<N, true>(L, a + o, b + o, c + o, xbar + s, dq + o, ddq + o, 1, (long)Nt, sd_start[p], sd_end[p], K + 2 * s, x + s,
                                   u + s, t + s, duration + p, &st, tau ? qd + o : nullptr, tau ? qdd + o : nullptr, tau ? tau + o : nullptr);
        else
          mp_toppra_sweep<N, false>(L, a + o, b + o, c + o, xbar + s, dq ? dq + o : nullptr, ddq ? ddq + o : nullptr, 1, (long)Nt,
                                    sd_start[p], sd_end[p], K + 2 * s, x + s, u + s, t + s, duration + p, &st, tau ? qd + o : nullptr,
                                    tau ? qdd + o : nullptr, tau ? tau + o : nullptr);
        status[p] = st;
      }
    });
  })
  return MP_OK;
}
int mp_toppra_cpu_f64(const mp_model* model, const double* q, const double* dq, const double* ddq, const double* velocity_limits,
                      const double* torque_limits, const double* acceleration_limits, const double* sd_start, const double* sd_end,
                      int64_t B, int64_t Nt, const double* g, const double* Ftip, double* K, double* x, double* u, double* t,
                      double* duration, int32_t* status, double* qd, double* qdd, double* tau, int nthreads) {
  const char* fn = "mp_toppra_cpu_f64";
  if (int rc = mp_small_model(fn, model)) return rc;
  REQUIRE(B >= 0, "%s: negative B", fn);
  REQUIRE(Nt >= 3, "%s: N must be >= 3 (got %lld)", fn, (long long)Nt);
  const int n = model->d.n;
  std::vector<double> co;
  try {
    co.resize((size_t)B * Nt * (3 * n + 1));
  } catch (...) {
    return mp_fail(MP_ERR_INVALID, "%s: out of memory for the coefficients", fn);
  }
  const size_t blk = (size_t)B * Nt * n;
  double *a = co.data(), *b = a + blk, *c = b + blk, *xb = c + blk;
  if (int rc = mp_path_dynamics_cpu_f64(model, q, dq, ddq, B * Nt, velocity_limits, g, Ftip, a, b, c, xb, nthreads)) return rc;
  return mp_toppra_sweep_cpu_f64(n, a, b, c, xb, dq, ddq, torque_limits, acceleration_limits, sd_start, sd_end, B, Nt, K, x, u, t, duration,
                                 status, qd, qdd, tau, nthreads);
}
int mp_fd_trajectory_cpu_f32(const mp_model* model, const float* theta0, const float* dtheta0, const float* taumat,
                             const float* Ftipmat, int64_t B, int64_t N, const double* g, double dt, int intRes, float* pos,
                             float* vel, float* acc, int nthreads) {
  return fd_trajectory_cpu<float>(model, theta0, dtheta0, taumat, Ftipmat, B, N, g, dt, intRes, pos, vel, acc, nthreads);
}
int mp_fd_trajectory_cpu_f64(const mp_model* model, const double* theta0, const double* dtheta0, const double* taumat,
                             const double* Ftipmat, int64_t B, int64_t N, const double* g, double dt, int intRes, float* pos,
                             float* vel, float* acc, int nthreads) {
  return fd_trajectory_cpu<double>(model, theta0, dtheta0, taumat, Ftipmat, B, N, g, dt, intRes, pos, vel, acc, nthreads);
}

int mp_inverse_kinematics_cpu_f64(const mp_model* model, const double* T_desired, const double* theta0, int64_t B,
                                  const double* joint_limits, double eomg, double ev, int max_iterations, double damping,
                                  double step_cap, double weight_orientation, double weight_position, int adaptive_tuning,
                                  int backtracking, uint32_t seed, double* theta, int32_t* success, int32_t* iterations,
                                  int32_t* restarts, int nthreads) {
  const char* fn = "mp_inverse_kinematics_cpu_f64";
  REQUIRE(model, "%s: null model", fn);
  REQUIRE(B >= 0, "%s: negative problem count", fn);
  if (B == 0) return MP_OK;
  REQUIRE(T_desired && theta0 && theta && success && iterations && restarts, "%s: null pointer", fn);
  REQUIRE(max_iterations >= 1, "%s: max_iterations must be at least 1", fn);
  auto pack = [&](auto* P) {  // (the twin's words for crossed limits name no joint)
    const int rc = mp_ik_pack(fn, model->d.n, joint_limits, eomg, ev, max_iterations, damping, step_cap, weight_orientation, weight_position,
                              adaptive_tuning, backtracking, seed, P);
    return rc < 0 ? mp_fail(MP_ERR_INVALID, "%s: a joint has its lower limit above its upper limit", fn) : rc;
  };
  if (model->big) {  // 9..32 joints: the body of k_dyn_ik (run-time-n kinematics of csrc/mp_dyn.h under the same iteration)
    MpIkBigParams PB;
    if (int rc = pack(&PB)) return rc;
    const MpBigModel<double>& MB = model->bd;
    const int n = MB.n;
    auto rows_of = [&](auto cap_tag) {   // per-problem arrays of 16 entries for 9..16 joints, 32 beyond (as the kernels: MP_DISPATCH_CAP)
      constexpr int CAP = decltype(cap_tag)::value;
      parallel_for(B, 1, nthreads, [&](int64_t lo, int64_t hi) {
        for (int64_t row = lo; row < hi; ++row) {
          MpIkState<CAP> S;
          for (int j = 0; j < CAP; ++j) S.theta[j] = j < n ? theta0[row * n + j] : 0.0;
          mp_ik_begin(S, PB);
          int done = 0;
          while (!(done = mp_ik_iterate<CAP, MpIkLooped<CAP>>(MB, PB, S, T_desired + row * 16, theta0 + row * n))) {}
          for (int j = 0; j < n; ++j) theta[row * n + j] = S.theta[j];
          success[row] = done == 2 ? 1 : 0;
          iterations[row] = S.k + 1;
          restarts[row] = S.restarts;
        }
      });
    };
    if (n <= MP_MID_DOF) rows_of(std::integral_constant<int, MP_MID_DOF>{});
    else rows_of(std::integral_constant<int, MP_BIG_DOF>{});
    return MP_OK;
  }
  MpIkParams P;
  if (int rc = pack(&P)) return rc;
  const MpModel<double>& M = model->d;
  // the body of k_ik (csrc/mp_kernels.hip) per problem: begin, iterate until the iteration reports done
  MP_CPU_DISPATCH(M.n, {
    parallel_for(B, 1, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t row = lo; row < hi; ++row) {
        MpIkState<N> S;
        for (int j = 0; j < N; ++j) S.theta[j] = theta0[row * N + j];
        mp_ik_begin(S, P);
        int done = 0;
        while (!(done = mp_ik_iterate<N>(M, P, S, T_desired + row * 16, theta0 + row * N))) {}
        for (int j = 0; j < N; ++j) theta[row * N + j] = S.theta[j];
        success[row] = done == 2 ? 1 : 0;
        iterations[row] = S.k + 1;
        restarts[row] = S.restarts;
      }
    });
  })
  return MP_OK;
}

int mp_pd_regulation_cpu_f64(const mp_model* model, const double* theta0, const double* theta_des, const double* Kp, const double* Kd,
                             int64_t K, const double* g, double dt, int steps, double* errors, int32_t* count, int nthreads) {
  REQUIRE(model, "mp_pd_regulation_cpu_f64: null model");
  REQUIRE(K >= 0 && steps >= 0, "mp_pd_regulation_cpu_f64: negative run or step count");
  if (K == 0) return MP_OK;
  REQUIRE(theta0 && theta_des && Kp && Kd && count && (errors || steps == 0), "mp_pd_regulation_cpu_f64: null pointer");
  const MpCall<double> C = make_call<double>(model, g, nullptr);
  const int n = model->d.n;
  if (model->big) {  // the body of k_dyn_pd_regulation
    parallel_for(K, 1, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t k = lo; k < hi; ++k)
        count[k] = mp_dyn_pd_regulation_run<MP_BIG_DOF, double>(model->bd, C.a0, theta0 + k * n, theta_des + k * n, Kp[k], Kd[k], dt, steps,
                                                    errors + k * steps);
    });
    return MP_OK;
  }
  const MpModel<double>& M = model->d;
  MP_CPU_DISPATCH(M.n, {  // the body of k_pd_regulation
    parallel_for(K, 1, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t k = lo; k < hi; ++k) {
        double a[N], d[N];
        for (int j = 0; j < N; ++j) { a[j] = theta0[k * N + j]; d[j] = theta_des[k * N + j]; }
        count[k] = mp_pd_regulation_run<double, N>(M, C.a0, a, d, Kp[k], Kd[k], dt, steps, errors + k * steps);
      }
    });
  })
  return MP_OK;
}

int mp_cartesian_trajectory_cpu_f32(const double* Xstart, const double* Xend, int64_t B, int64_t N, double Tf, int method,
                                    float* pos, float* vel, float* acc, float* orient, int nthreads) {
  REQUIRE(B >= 0 && N >= 0, "mp_cartesian_trajectory_cpu_f32: negative count");
  if (B == 0 || N == 0) return MP_OK;
  REQUIRE(N >= 2, "mp_cartesian_trajectory_cpu_f32: N must be >= 2");
  REQUIRE(Xstart && Xend && pos && vel && acc && orient, "mp_cartesian_trajectory_cpu_f32: null pointer");
  parallel_for(B * N, 512, nthreads, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      const int64_t b = r / N, i = r - b * N;
      double A[16], E[16];
      std::memcpy(A, Xstart + b * 16, sizeof A);
      std::memcpy(E, Xend + b * 16, sizeof E);
      float p[3], v[3], a[3], o[9];
      mp_cartesian_point(A, E, (long)i, (long)N, Tf, method, p, v, a, o);
      std::memcpy(pos + r * 3, p, sizeof p); std::memcpy(vel + r * 3, v, sizeof v); std::memcpy(acc + r * 3, a, sizeof a);
      std::memcpy(orient + r * 9, o, sizeof o);
    }
  });
  return MP_OK;
}

// ---- sphere-model collision (mp_collision.h): the tables' checks, the handle, and the kernel's per-row code over host rows
int mp_collision_create(const mp_model* model, int S, const int32_t* link, const double* centre, const double* radius, int P,
                        const int32_t* pairs, mp_collision** out) {
  const char* fn = "mp_collision_create";
  REQUIRE(out, "%s: null output", fn);
  *out = nullptr;
  if (int rc = mp_small_model(fn, model)) return rc;
  REQUIRE(S >= 1 && S <= MP_COL_MAX_SPHERES, "%s: %d spheres, outside 1..64", fn, S);
  REQUIRE(P >= 0, "%s: negative pair count", fn);
  REQUIRE(link && centre && radius && (P == 0 || pairs), "%s: null table", fn);
  const MpModel<double>& M = model->d;
  const int n = M.n;
  for (int s = 0; s < S; ++s) {
    REQUIRE(link[s] >= 0 && link[s] <= n, "%s: sphere %d: link outside 0..n", fn, s);
    REQUIRE(radius[s] > 0.0 && std::isfinite(radius[s]), "%s: sphere %d: radius %g is not positive and finite", fn, s, radius[s]);
    for (int k = 0; k < 3; ++k) REQUIRE(std::isfinite(centre[3 * s + k]), "%s: sphere %d: non-finite centre", fn, s);
  }
  for (int k = 0; k < P; ++k) {
    const int a = pairs[2 * k], b = pairs[2 * k + 1];
    REQUIRE(a >= 0 && a < S && b >= 0 && b < S, "%s: pair %d: sphere index outside 0..S-1", fn, k);
    REQUIRE(a != b, "%s: pair %d: a sphere paired with itself", fn, k);
  }
  mp_collision* h = new (std::nothrow) mp_collision;
  REQUIRE(h, "%s: out of host memory", fn);
  h->n = n;
  // the link frames at the home configuration
  double R[MP_MAX_DOF][9], p[MP_MAX_DOF][3];
  switch (n) {
#define MP_COL_HOME(NN)                                                              \
    case NN: {                                                                       \
      double z[NN] = {}, Rn[NN][9], pn[NN][3];                                       \
      mp_col_link_frames<NN>(M, z, Rn, pn);                                          \
      std::memcpy(R, Rn, sizeof Rn); std::memcpy(p, pn, sizeof pn);                  \
    } break;
    MP_COL_HOME(1) MP_COL_HOME(2) MP_COL_HOME(3) MP_COL_HOME(4) MP_COL_HOME(5) MP_COL_HOME(6) MP_COL_HOME(7) MP_COL_HOME(8)
#undef MP_COL_HOME
    default: delete h; return mp_fail(MP_ERR_INVALID, "%s: dof outside 1..8", fn);
  }
  MpColSpheres& T = h->sph;
  std::memset(&T, 0, sizeof T);
  T.S = S; T.P = P;
  int at = 0, where[MP_COL_MAX_SPHERES];  // caller index -> sorted index
  for (int k = 0; k <= MP_MAX_DOF; ++k) {   // a stable sort by link
    T.first[k] = at;
    for (int s = 0; s < S; ++s) {
      if (link[s] != k) continue;
      T.caller[at] = s; T.link[at] = k; T.radius[at] = radius[s];
      const double* c = centre + 3 * s;
      if (k == 0) {
        T.local[at][0] = c[0]; T.local[at][1] = c[1]; T.local[at][2] = c[2];
      } else {  // R_k(0)^T (c - p_k(0))
        const double* Rk = R[k - 1];
        const double dx = c[0] - p[k - 1][0], dy = c[1] - p[k - 1][1], dz = c[2] - p[k - 1][2];
        for (int a = 0; a < 3; ++a) T.local[at][a] = Rk[a] * dx + Rk[3 + a] * dy + Rk[6 + a] * dz;
      }
      where[s] = at++;
    }
  }
  T.first[MP_MAX_DOF + 1] = at;
  // The motion bounds of the edge check.  Anchor A_j of a revolute joint: the point of its axis nearest the origin at home (the axis
  // is the z line of link frame j).  r_j(c) for a centre c on link k: the polyline c -> A_i1 -> ... -> A_j through the anchors of the
  // revolute joints j < i <= k in descending order - a rotation about axis i keeps the distance to a point of that axis, so the
  // polyline's length bounds |c(q) - A_j(q)| at every q that moves no prismatic joint between them.
  double A[MP_MAX_DOF][3];
  bool rev[MP_MAX_DOF];
  for (int j = 0; j < n; ++j) {
    const double w[3] = {R[j][2], R[j][5], R[j][8]};
    const double along = w[0] * p[j][0] + w[1] * p[j][1] + w[2] * p[j][2];
    for (int a = 0; a < 3; ++a) A[j][a] = p[j][a] - along * w[a];
    rev[j] = M.j[j].rev != 0.0;
  }
  for (int s = 0; s < S; ++s) {
    const int k = link[s];
    double at3[3] = {centre[3 * s], centre[3 * s + 1], centre[3 * s + 2]}, len = 0.0;
    for (int j = k; j >= 1; --j) {  // joint j (1-based) walks down from the sphere's link
      if (!rev[j - 1]) continue;
      const double dx = at3[0] - A[j - 1][0], dy = at3[1] - A[j - 1][1], dz = at3[2] - A[j - 1][2];
      len += std::sqrt(dx * dx + dy * dy + dz * dz);
      for (int a = 0; a < 3; ++a) at3[a] = A[j - 1][a];
      if (len > T.rho[j - 1][k]) T.rho[j - 1][k] = len;
    }
  }
  h->pairs.resize((size_t)P);
  for (int k = 0; k < P; ++k) { h->pairs[(size_t)k].a = where[pairs[2 * k]]; h->pairs[(size_t)k].b = where[pairs[2 * k + 1]]; }
  *out = h;
  return MP_OK;
}

int mp_collision_destroy(mp_collision* h) {
  if (!h) return MP_OK;
  if (h->release) h->release(h);
  delete h;
  return MP_OK;
}

}  // extern "C"

int mp_collision_pack_world(const char* fn, int O, const int32_t* kind, const double* params, std::vector<MpColObstacle>* out) {
  REQUIRE(O >= 0, "%s: negative obstacle count", fn);
  REQUIRE(O == 0 || (kind && params), "%s: null obstacle table", fn);
  std::vector<MpColObstacle> w((size_t)O);
  for (int o = 0; o < O; ++o) {
    const double* p = params + 16 * (size_t)o;
    const int used = kind[o] == MP_OBSTACLE_SPHERE ? 4 : kind[o] == MP_OBSTACLE_CAPSULE ? 7 : kind[o] == MP_OBSTACLE_BOX ? 15 : 0;
    REQUIRE(used, "%s: obstacle %d: unknown kind", fn, o);
    for (int k = 0; k < used; ++k) REQUIRE(std::isfinite(p[k]), "%s: obstacle %d: non-finite parameter", fn, o);
    REQUIRE(kind[o] != MP_OBSTACLE_SPHERE || !(p[3] < 0.0), "%s: obstacle %d: negative radius", fn, o);
    REQUIRE(kind[o] != MP_OBSTACLE_CAPSULE || !(p[6] < 0.0), "%s: obstacle %d: negative radius", fn, o);
    if (kind[o] == MP_OBSTACLE_BOX) {
      for (int k = 12; k < 15; ++k) REQUIRE(!(p[k] < 0.0), "%s: obstacle %d: negative half-extent", fn, o);
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
          double dot = 0.0;
          for (int k = 0; k < 3; ++k) dot += p[3 + 3 * k + a] * p[3 + 3 * k + b];
          REQUIRE(!(std::fabs(dot - (a == b ? 1.0 : 0.0)) > 1e-9), "%s: obstacle %d: box rotation is not orthonormal to 1e-9", fn, o);
        }
    }
    MpColObstacle& ob = w[(size_t)o];
    std::memset(&ob, 0, sizeof ob);
    std::memcpy(ob.p, p, (size_t)used * sizeof(double));
    ob.kind = kind[o];
  }
  out->swap(w);
  return MP_OK;
}

// ---- what the four twins below share: the first checks, and the handle's host tables as the per-row code reads them
static int col_twin_enter(const char* fn, const mp_model* model, const mp_collision* h) {
  REQUIRE(model && h, "%s: null model or collision handle", fn);
  REQUIRE_SMALL(fn);
  REQUIRE(h->n == model->d.n, "%s: the collision handle was made for a model of %d joints", fn, h->n);
  return MP_OK;
}
static int col_joint_count(const char* fn, int n) {  // the n of the two workspace sizes
  REQUIRE(n >= 1, "%s: joint count %d below 1", fn, n);
  return n > MP_MAX_DOF ? mp_too_many_joints(fn, n) : MP_OK;
}
// (the twins always carry the cloud's query: a null address in the header skips it, and the arithmetic of the rest is the same)
typedef MpColTables<const MpColSpheres*, const MpColPair*, const MpColWorld*, const MpColObstacle*, MpCloudPtrHost> MpColTablesHost;
static MpColTablesHost col_host_tables(const mp_collision* h, MpColWorld& hdr) {  // hdr: the caller's, the tables point at it
  hdr = {(int)h->world.size(), 0, h->cloud.empty() ? nullptr : reinterpret_cast<const MpColCloud*>(h->cloud.data())};
  return {&h->sph, h->pairs.data(), &hdr, h->world.data()};
}

extern "C" {

int mp_collision_cpu_f64(const mp_model* model, const mp_collision* h, const double* q, int64_t rows, double eps_world, double eps_self,
                         double* dist_world, int32_t* arg_world, double* dist_self, int32_t* arg_self, double* grad_dist_world,
                         double* grad_dist_self, double* cost, double* grad, int nthreads) {
  const char* fn = "mp_collision_cpu_f64";
  if (int rc = col_twin_enter(fn, model, h)) return rc;
  REQUIRE(eps_world > 0.0 && eps_self > 0.0 && std::isfinite(eps_world) && std::isfinite(eps_self),
          "%s: eps_world and eps_self must be positive and finite", fn);
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  if (rows == 0) return MP_OK;
  REQUIRE(q, "%s: null pointer", fn);
  const MpColOut O = {dist_world, arg_world, dist_self, arg_self, grad_dist_world, grad_dist_self, cost, grad};
  REQUIRE(mp_out_any(O), "%s: at least one output is required", fn);
  const MpModel<double>& M = model->d;
  MpColWorld hdr;
  const MpColTablesHost tb = col_host_tables(h, hdr);
  const bool want_grad = grad_dist_world || grad_dist_self || grad;
  MP_CPU_DISPATCH(M.n, {
    parallel_for(rows, 64, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t r = lo; r < hi; ++r) {
        if (want_grad) mp_collision_cpu_row<N, true>(M, tb, q, eps_world, eps_self, (long)r, O);
        else mp_collision_cpu_row<N, false>(M, tb, q, eps_world, eps_self, (long)r, O);
      }
    });
  })
  return MP_OK;
}

}  // extern "C"

// ---- continuous collision checking of joint-space edges (mp_collision.h, mp_collision_edge_*)
int mp_collision_edges_check(const char* fn, double margin, double tol, int max_steps) {
  REQUIRE(std::isfinite(margin), "%s: margin must be finite", fn);
  REQUIRE(tol > 0.0 && std::isfinite(tol), "%s: tol must be positive and finite", fn);
  REQUIRE(max_steps >= 1 && max_steps <= MP_COL_EDGE_MAX_STEPS, "%s: max_steps %d outside 1..65536", fn, max_steps);
  return MP_OK;
}

extern "C" {

int mp_collision_motion_bounds(const mp_collision* h, double* rho) {
  const char* fn = "mp_collision_motion_bounds";
  REQUIRE(h && rho, "%s: null pointer", fn);
  for (int j = 0; j < h->n; ++j)
    for (int k = 0; k <= h->n; ++k) rho[j * (h->n + 1) + k] = h->sph.rho[j][k];
  return MP_OK;
}

int mp_collision_edges_cpu_f64(const mp_model* model, const mp_collision* h, const double* q_from, const double* q_to, int64_t edges,
                               double margin, double tol, int max_steps, int32_t* status, double* t, int32_t* steps, double* clearance,
                               int32_t* witness, int nthreads) {
  const char* fn = "mp_collision_edges_cpu_f64";
  if (int rc = col_twin_enter(fn, model, h)) return rc;
  if (int rc = mp_collision_edges_check(fn, margin, tol, max_steps)) return rc;
  REQUIRE(edges >= 0, "%s: negative edge count", fn);
  if (edges == 0) return MP_OK;
  REQUIRE(q_from && q_to, "%s: null pointer", fn);
  const MpColEdgeOut O = {status, t, steps, clearance, witness};
  REQUIRE(mp_out_any(O), "%s: at least one output is required", fn);
  const MpModel<double>& M = model->d;
  MpColWorld hdr;
  const MpColTablesHost tb = col_host_tables(h, hdr);
  const MpColEdgeParams P = {margin, tol, max_steps, 0};
  MP_CPU_DISPATCH(M.n, {
    parallel_for(edges, 16, nthreads, [&](int64_t lo, int64_t hi) {
      for (int64_t e = lo; e < hi; ++e) mp_collision_edge_cpu<N>(M, tb, q_from, q_to, P, (long)e, O);
    });
  })
  return MP_OK;
}

}  // extern "C"

// ---- batched RRT-Connect over the sphere model (mp_rrt.h)
int mp_rrt_connect_check(const char* fn, int n, const double* lo, const double* hi, uint32_t seed, double step, double min_advance,
                         int max_iters, int max_nodes, int max_waypoints, double margin, double tol, int max_steps, MpRrtParams* out) {
  if (int rc = mp_collision_edges_check(fn, margin, tol, max_steps)) return rc;
  REQUIRE(lo && hi, "%s: null sampling box", fn);
  MpRrtParams P;
  std::memset(&P, 0, sizeof P);
  for (int j = 0; j < n; ++j) {
    REQUIRE(std::isfinite(lo[j]) && std::isfinite(hi[j]) && lo[j] <= hi[j], "%s: joint %d: the sampling box must be finite with lo <= hi", fn, j);
    P.lo[j] = lo[j];
    P.hi[j] = hi[j];
  }
  REQUIRE(step > 0.0 && std::isfinite(step), "%s: step must be positive and finite", fn);
  REQUIRE(min_advance >= 0.0 && std::isfinite(min_advance), "%s: min_advance must be non-negative and finite", fn);
  REQUIRE(max_iters >= 0, "%s: negative max_iters", fn);
  REQUIRE(max_nodes >= 2 && max_nodes <= MP_RRT_MAX_NODES, "%s: max_nodes %d outside 2..65536", fn, max_nodes);
  REQUIRE(max_waypoints >= 2, "%s: max_waypoints %d below 2", fn, max_waypoints);
  P.step = step; P.min_advance = min_advance;
  P.edge = {margin, tol, max_steps, 0};
  P.seed = seed; P.max_iters = max_iters; P.max_nodes = max_nodes; P.max_waypoints = max_waypoints;
  *out = P;
  return MP_OK;
}

extern "C" {

int64_t mp_rrt_connect_workspace_bytes(int n, int max_nodes, int blocks) {
  const char* fn = "mp_rrt_connect_workspace_bytes";
  if (int rc = col_joint_count(fn, n)) return -(int64_t)rc;
  if (max_nodes < 2 || max_nodes > MP_RRT_MAX_NODES) return -(int64_t)mp_fail(MP_ERR_INVALID, "%s: max_nodes %d outside 2..65536", fn, max_nodes);
  if (blocks < 1) return -(int64_t)mp_fail(MP_ERR_INVALID, "%s: block count %d below 1", fn, blocks);
  return (int64_t)blocks * 64 * 2 * (int64_t)max_nodes * (8 * (int64_t)n + 4);
}

int mp_rrt_connect_cpu_f64(const mp_model* model, const mp_collision* h, const double* q_start, const double* q_goal, int64_t B,
                           const double* lo, const double* hi, uint32_t seed, double step, double min_advance, int max_iters,
                           int max_nodes, int max_waypoints, double margin, double tol, int max_steps, int32_t* status, int32_t* count,
                           double* waypoints, int32_t* iterations, int32_t* nodes, int32_t* evaluations, int nthreads) {
  const char* fn = "mp_rrt_connect_cpu_f64";
  if (int rc = col_twin_enter(fn, model, h)) return rc;
  MpRrtParams P;
  if (int rc = mp_rrt_connect_check(fn, model->d.n, lo, hi, seed, step, min_advance, max_iters, max_nodes, max_waypoints, margin, tol,
                                    max_steps, &P))
    return rc;
  REQUIRE(B >= 0, "%s: negative problem count", fn);
  if (B == 0) return MP_OK;
  REQUIRE(q_start && q_goal, "%s: null pointer", fn);
  const MpRrtOut O = {status, count, waypoints, iterations, nodes, evaluations};
  REQUIRE(mp_out_any(O), "%s: at least one output is required", fn);
  const MpModel<double>& M = model->d;
  MpColWorld hdr;
  const MpColTablesHost tb = col_host_tables(h, hdr);
  MP_CPU_DISPATCH(M.n, {
    parallel_for(B, 1, nthreads, [&](int64_t b0, int64_t b1) {
      std::vector<double> tree((size_t)2 * (size_t)max_nodes * N);  // the thread's trees, reused like a lane's
      std::vector<int> parents((size_t)2 * (size_t)max_nodes);
      for (int64_t b = b0; b < b1; ++b) mp_rrt_cpu<N>(M, tb, P, q_start, q_goal, (long)b, tree.data(), parents.data(), O);
    });
  })
  return MP_OK;
}

}  // extern "C"

// ---- batched path shortcutting over the sphere model (mp_shortcut.h)
int mp_path_shortcut_check(const char* fn, int64_t w_in, uint32_t seed, int max_iters, double min_gain, int max_waypoints, double margin,
                           double tol, int max_steps, MpShortcutParams* out) {
  if (int rc = mp_collision_edges_check(fn, margin, tol, max_steps)) return rc;
  REQUIRE(w_in >= 1 && w_in <= MP_SC_MAX_WAYPOINTS, "%s: %lld input rows a path, outside 1..65536", fn, (long long)w_in);
  REQUIRE(max_iters >= 0, "%s: negative max_iters", fn);
  REQUIRE(min_gain >= 0.0 && std::isfinite(min_gain), "%s: min_gain must be non-negative and finite", fn);
  REQUIRE(max_waypoints >= 2 && max_waypoints <= MP_SC_MAX_WAYPOINTS, "%s: max_waypoints %d outside 2..65536", fn, max_waypoints);
  MpShortcutParams P;
  std::memset(&P, 0, sizeof P);
  P.edge = {margin, tol, max_steps, 0};
  P.min_gain = min_gain;
  P.seed = seed; P.max_iters = max_iters; P.max_waypoints = max_waypoints; P.w_in = (int)w_in;
  *out = P;
  return MP_OK;
}

extern "C" {

int64_t mp_path_shortcut_workspace_bytes(int n, int max_waypoints, int blocks) {
  const char* fn = "mp_path_shortcut_workspace_bytes";
  if (int rc = col_joint_count(fn, n)) return -(int64_t)rc;
  if (max_waypoints < 2 || max_waypoints > MP_SC_MAX_WAYPOINTS)
    return -(int64_t)mp_fail(MP_ERR_INVALID, "%s: max_waypoints %d outside 2..65536", fn, max_waypoints);
  if (blocks < 1) return -(int64_t)mp_fail(MP_ERR_INVALID, "%s: block count %d below 1", fn, blocks);
  return (int64_t)blocks * 64 * (int64_t)max_waypoints * (8 * (int64_t)n + 8);
}

int mp_path_shortcut_cpu_f64(const mp_model* model, const mp_collision* h, const double* waypoints_in, const int32_t* count_in, int64_t B,
                             int64_t W_in, uint32_t seed, int max_iters, double min_gain, int max_waypoints, double margin, double tol,
                             int max_steps, int32_t* status, int32_t* count, double* waypoints, double* length_in, double* length_out,
                             int32_t* iterations, int32_t* accepted, int32_t* skipped_full, int32_t* evaluations, int nthreads) {
  const char* fn = "mp_path_shortcut_cpu_f64";
  if (int rc = col_twin_enter(fn, model, h)) return rc;
  MpShortcutParams P;
  if (int rc = mp_path_shortcut_check(fn, W_in, seed, max_iters, min_gain, max_waypoints, margin, tol, max_steps, &P)) return rc;
  REQUIRE(B >= 0, "%s: negative problem count", fn);
  if (B == 0) return MP_OK;
  REQUIRE(waypoints_in && count_in, "%s: null pointer", fn);
  const MpShortcutOut O = {status, count, waypoints, length_in, length_out, iterations, accepted, skipped_full, evaluations};
  REQUIRE(mp_out_any(O), "%s: at least one output is required", fn);
  const MpModel<double>& M = model->d;
  MpColWorld hdr;
  const MpColTablesHost tb = col_host_tables(h, hdr);
  MP_CPU_DISPATCH(M.n, {
    parallel_for(B, 1, nthreads, [&](int64_t b0, int64_t b1) {
      std::vector<double> pts((size_t)max_waypoints * N), cum((size_t)max_waypoints);  // the thread's path, reused like a lane's
      for (int64_t b = b0; b < b1; ++b) mp_shortcut_cpu<N>(M, tb, P, waypoints_in, count_in, (long)b, pts.data(), cum.data(), O);
    });
  })
  return MP_OK;
}

}  // extern "C"

// ---- goal configurations for pose goals over the sphere model (mp_goal.h)
int mp_goal_ik_check(const char* fn, int n, const double* lo, const double* hi, uint32_t seed, double eomg, double ev, double damping,
                     double step_cap, int max_iters, int max_attempts, double margin, double tol, MpGoalParams* out) {
  if (int rc = mp_collision_edges_check(fn, margin, tol, 1)) return rc;
  REQUIRE(lo && hi, "%s: null joint box", fn);
  MpGoalParams P;
  std::memset(&P, 0, sizeof P);
  for (int j = 0; j < n; ++j) {
    REQUIRE(std::isfinite(lo[j]) && std::isfinite(hi[j]) && lo[j] <= hi[j], "%s: joint %d: the box must be finite with lo <= hi", fn, j);
    P.lo[j] = lo[j];
    P.hi[j] = hi[j];
  }
  REQUIRE(eomg > 0.0 && std::isfinite(eomg) && ev > 0.0 && std::isfinite(ev), "%s: eomg and ev must be positive and finite", fn);
  REQUIRE(damping > 0.0 && std::isfinite(damping), "%s: damping must be positive and finite", fn);
  REQUIRE(step_cap > 0.0 && std::isfinite(step_cap), "%s: step_cap must be positive and finite", fn);
  REQUIRE(max_iters >= 0, "%s: negative max_iters", fn);
  REQUIRE(max_attempts >= 1 && max_attempts <= MP_GOAL_MAX_ATTEMPTS, "%s: max_attempts %d outside 1..65536", fn, max_attempts);
  P.eomg = eomg; P.ev = ev; P.damping = damping; P.step_cap = step_cap;
  P.edge = {margin, tol, 1, 0};
  P.seed = seed; P.max_iters = max_iters; P.max_attempts = max_attempts;
  *out = P;
  return MP_OK;
}

extern "C" {

int mp_goal_ik_cpu_f64(const mp_model* model, const mp_collision* h, const double* T_goal, const double* q_seed, int64_t B,
                       const double* lo, const double* hi, uint32_t seed, double eomg, double ev, double damping, double step_cap,
                       int max_iters, int max_attempts, double margin, double tol, int32_t* status, double* q, int32_t* attempts,
                       int32_t* iterations, int32_t* converged, double* pose_error, double* clearance, int32_t* witness, int nthreads) {
  const char* fn = "mp_goal_ik_cpu_f64";
  if (int rc = col_twin_enter(fn, model, h)) return rc;
  MpGoalParams P;
  if (int rc = mp_goal_ik_check(fn, model->d.n, lo, hi, seed, eomg, ev, damping, step_cap, max_iters, max_attempts, margin, tol, &P))
    return rc;
  REQUIRE(B >= 0, "%s: negative problem count", fn);
  if (B == 0) return MP_OK;
  REQUIRE(T_goal && q_seed, "%s: null pointer", fn);
  const MpGoalOut O = {status, q, attempts, iterations, converged, pose_error, clearance, witness};
  REQUIRE(mp_out_any(O), "%s: at least one output is required", fn);
  const MpModel<double>& M = model->d;
  MpColWorld hdr;
  const MpColTablesHost tb = col_host_tables(h, hdr);
  MP_CPU_DISPATCH(M.n, {
    parallel_for(B, 1, nthreads, [&](int64_t b0, int64_t b1) {
      for (int64_t b = b0; b < b1; ++b) mp_goal_cpu<N>(M, tb, P, T_goal, q_seed, (long)b, O);
    });
  })
  return MP_OK;
}

}  // extern "C"

// ---- C2 corner blending of waypoint paths over the sphere model (mp_blend.h)
int mp_path_blend_check(const char* fn, int64_t w_in, int64_t grid, double blend, int max_halvings, double margin, double tol,
                        int max_steps, MpBlendParams* out) {
  if (int rc = mp_collision_edges_check(fn, margin, tol, max_steps)) return rc;
  REQUIRE(w_in >= 1 && w_in <= MP_BL_MAX_WAYPOINTS, "%s: %lld input rows a path, outside 1..65536", fn, (long long)w_in);
  REQUIRE(grid >= 3 && grid <= MP_BL_MAX_GRID, "%s: %lld grid points, outside 3..65536", fn, (long long)grid);
  REQUIRE(blend > 0.0 && std::isfinite(blend), "%s: blend must be positive and finite", fn);
  REQUIRE(max_halvings >= 0 && max_halvings <= MP_BL_MAX_HALVINGS, "%s: max_halvings %d outside 0..32", fn, max_halvings);
  MpBlendParams P;
  std::memset(&P, 0, sizeof P);
  P.edge = {margin, tol, max_steps, 0};
  P.blend = blend;
  P.max_halvings = max_halvings; P.w_in = (int)w_in; P.grid = (int)grid;
  *out = P;
  return MP_OK;
}

extern "C" {

int mp_path_blend_cpu_f64(const mp_model* model, const mp_collision* h, const double* waypoints_in, const int32_t* count_in, int64_t B,
                          int64_t W_in, int64_t N_grid, double blend, int max_halvings, double margin, double tol, int max_steps,
                          int32_t* status, int32_t* corner, int32_t* count, double* points, double* cut, double* knot, double* length,
                          int32_t* halvings, int32_t* evaluations, double* clearance, double* q, double* dq, double* ddq, int nthreads) {
  const char* fn = "mp_path_blend_cpu_f64";
  if (int rc = col_twin_enter(fn, model, h)) return rc;
  MpBlendParams P;
  if (int rc = mp_path_blend_check(fn, W_in, N_grid, blend, max_halvings, margin, tol, max_steps, &P)) return rc;
  REQUIRE(B >= 0, "%s: negative problem count", fn);
  if (B == 0) return MP_OK;
  REQUIRE(waypoints_in && count_in, "%s: null pointer", fn);
  const MpBlendOut O = {status, corner, count, points, cut, knot, length, halvings, evaluations, clearance};
  const bool grid = q || dq || ddq;
  REQUIRE(mp_out_any(O) || grid, "%s: at least one output is required", fn);
  const MpModel<double>& M = model->d;
  MpColWorld hdr;
  const MpColTablesHost tb = col_host_tables(h, hdr);
  MP_CPU_DISPATCH(M.n, {
    parallel_for(B, 1, nthreads, [&](int64_t b0, int64_t b1) {
      // the tables the grid reads back, where the caller did not ask for them: the thread's own, reused like a lane's registers
      std::vector<double> own_points(grid && !points ? (size_t)W_in * N : 0), own_cut(grid && !cut ? (size_t)W_in : 0),
          own_knot(grid && !knot ? (size_t)W_in : 0);
      for (int64_t b = b0; b < b1; ++b) {
        MpBlendRows o = mp_blend_rows(O, (long)b, P.w_in, N);
        if (grid && !points) o.points = own_points.data();
        if (grid && !cut) o.cut = own_cut.data();
        if (grid && !knot) o.knot = own_knot.data();
        MpBlendState<N> S;
        mp_blend_cpu<N>(M, tb, P, waypoints_in + b * W_in * N, count_in[b], (long)b, o, O, S);
        if (!grid) continue;
        for (int i = 0; i < P.grid; ++i) {
          double x[N], dx[N], ddx[N];
          mp_blend_sample<N>(S.status, S.m, S.length, o.points, o.cut, o.knot, i, P.grid, x, dx, ddx);
          const int64_t at = (b * P.grid + i) * N;
          for (int j = 0; j < N; ++j) {
            if (q) q[at + j] = x[j];
            if (dq) dq[at + j] = dx[j];
            if (ddq) ddq[at + j] = ddx[j];
          }
        }
      }
    });
  })
  return MP_OK;
}

}  // extern "C"

// ---- Cartesian straight-line paths over the sphere model (mp_cartesian.h)
int mp_cartesian_path_check(const char* fn, int n, int64_t B, const double* lo, const double* hi, int64_t grid, int task, double eomg,
                            double ev, double damping, int max_iters, double max_joint_step, double margin, double tol, int max_steps,
                            MpCartParams* out) {
  if (int rc = mp_collision_edges_check(fn, margin, tol, max_steps)) return rc;
  REQUIRE(task == MP_CP_FULL || task == MP_CP_POSITION, "%s: task %d is neither MP_TASK_FULL (0) nor MP_TASK_POSITION (1)", fn, task);
  const int rows = task == MP_CP_FULL ? 6 : 3;
  if (n < rows)
    return mp_fail(MP_ERR_UNSUPPORTED, "%s: a task of %d rows needs at least %d joints (this model has %d)", fn, rows, rows, n);
  REQUIRE(B >= 0, "%s: negative problem count", fn);
  REQUIRE(grid >= 2 && grid <= MP_CP_MAX_GRID, "%s: %lld grid points, outside 2..65536", fn, (long long)grid);
  REQUIRE(B == 0 || grid <= ((int64_t)1 << 56) / B / n, "%s: %lld problems of %lld grid points are not addressable", fn, (long long)B,
          (long long)grid);
  REQUIRE(lo && hi, "%s: null joint box", fn);
  MpCartParams P;
  std::memset(&P, 0, sizeof P);
  for (int j = 0; j < n; ++j) {
    REQUIRE(std::isfinite(lo[j]) && std::isfinite(hi[j]) && lo[j] <= hi[j], "%s: joint %d: the box must be finite with lo <= hi", fn, j);
    P.lo[j] = lo[j];
    P.hi[j] = hi[j];
  }
  REQUIRE(eomg > 0.0 && std::isfinite(eomg) && ev > 0.0 && std::isfinite(ev), "%s: eomg and ev must be positive and finite", fn);
  REQUIRE(damping > 0.0 && std::isfinite(damping), "%s: damping must be positive and finite", fn);
  REQUIRE(max_joint_step > 0.0 && std::isfinite(max_joint_step), "%s: max_joint_step must be positive and finite", fn);
  REQUIRE(max_iters >= 0 && max_iters <= MP_CP_MAX_ITERS, "%s: max_iters %d outside 0..65536", fn, max_iters);
  P.eomg = eomg; P.ev = ev; P.damping = damping; P.max_joint_step = max_joint_step;
  P.edge = {margin, tol, max_steps, 0};
  P.grid = (int)grid; P.task = task; P.max_iters = max_iters;
  *out = P;
  return MP_OK;
}

// the twin's instance for a chain of N joints and a task of MR rows; none where the chain is too short (the check has refused it)
template <int N, int MR, bool FITS = (N >= MR)>
struct CartesianTwin {
  template <typename... A> static void run(A&&... a) { mp_cart_problem_cpu<N, MR>(a...); }
};
template <int N, int MR>
struct CartesianTwin<N, MR, false> {
  template <typename... A> static void run(A&&...) {}
};

extern "C" {

int64_t mp_cartesian_path_workspace_bytes(int64_t B, int64_t N) {
  if (B < 0 || N < 2 || N > MP_CP_MAX_GRID || (B > 0 && N > ((int64_t)1 << 56) / B)) {
    mp_fail(MP_ERR_INVALID, "mp_cartesian_path_workspace_bytes: %lld problems of %lld grid points (N in 2..65536)", (long long)B, (long long)N);
    return -MP_ERR_INVALID;
  }
  return (int64_t)mp_cart_work_bytes((long)B, (long)N);
}

int mp_cartesian_path_cpu_f64(const mp_model* model, const mp_collision* h, const double* q_start, const double* T_goal, int64_t B,
                              const double* lo, const double* hi, int64_t N_grid, int task, double eomg, double ev, double damping,
                              int max_iters, double max_joint_step, double margin, double tol, int max_steps, int32_t* status,
                              int32_t* reached, int32_t* span, double* t, double* clearance, double* deviation_pos,
                              double* deviation_rot, double* pose_error, int32_t* iterations, int32_t* evaluations, double* q, double* dq,
                              double* ddq, int32_t* span_status, double* span_clearance, int nthreads) {
  const char* fn = "mp_cartesian_path_cpu_f64";
  if (int rc = col_twin_enter(fn, model, h)) return rc;
  MpCartParams P;
  if (int rc = mp_cartesian_path_check(fn, model->d.n, B, lo, hi, N_grid, task, eomg, ev, damping, max_iters, max_joint_step, margin, tol,
                                       max_steps, &P))
    return rc;
  if (B == 0) return MP_OK;
  REQUIRE(q_start && T_goal, "%s: null pointer", fn);
  const MpCartOut O = {status, reached, span, t, clearance, deviation_pos, deviation_rot, pose_error, iterations, evaluations, span_status,
                       span_clearance};
  REQUIRE(mp_out_any(O) || q || dq || ddq, "%s: at least one output is required", fn);
  const MpModel<double>& M = model->d;
  MpColWorld hdr;
  const MpColTablesHost tb = col_host_tables(h, hdr);
  MP_CPU_DISPATCH(M.n, {
    parallel_for(B, 1, nthreads, [&](int64_t b0, int64_t b1) {
      // One problem at a time: its workspace and the grid arrays the caller did not ask for are the thread's own, addressed as
      // problem 0 of a batch of one - so are the outputs, through pointers moved to the problem.
      const size_t rows = (size_t)P.grid * N;
      std::vector<char> work(mp_cart_work_bytes(1, P.grid) + 16);
      std::vector<double> own_q(q ? 0 : rows), own_dq(dq ? 0 : rows), own_ddq(ddq ? 0 : rows);
      void* base = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(work.data()) + 15) & ~(uintptr_t)15);
      const MpCartWork W = mp_cart_work(base, 1, P.grid);
      for (int64_t b = b0; b < b1; ++b) {
        const int64_t e = b * (P.grid - 1);
        const MpCartOut Ob = {O.status ? O.status + b : nullptr, O.reached ? O.reached + b : nullptr, O.span ? O.span + b : nullptr,
                              O.t ? O.t + b : nullptr, O.clearance ? O.clearance + b : nullptr,
                              O.deviation_pos ? O.deviation_pos + b : nullptr, O.deviation_rot ? O.deviation_rot + b : nullptr,
                              O.pose_error ? O.pose_error + b : nullptr, O.iterations ? O.iterations + b : nullptr,
                              O.evaluations ? O.evaluations + b : nullptr, O.span_status ? O.span_status + e : nullptr,
                              O.span_clearance ? O.span_clearance + e : nullptr};
        double* qb = q ? q + b * rows : own_q.data();
        double* dqb = dq ? dq + b * rows : own_dq.data();
        double* ddqb = ddq ? ddq + b * rows : own_ddq.data();
        if (P.task == MP_CP_FULL) CartesianTwin<N, 6>::run(M, tb, P, q_start + b * N, T_goal + 16 * b, 0L, W, qb, dqb, ddqb, Ob);
        else CartesianTwin<N, 3>::run(M, tb, P, q_start + b * N, T_goal + 16 * b, 0L, W, qb, dqb, ddqb, Ob);
      }
    });
  })
  return MP_OK;
}

}  // extern "C"

// ---- fixed-rate sampling of timed paths (mp_sample.h)
int mp_trajectory_sample_check(const char* fn, int64_t B, int64_t grid, int64_t w_in, double dt, int64_t M, int n, int grid_given,
                               int curve_given, MpSampleIn* out) {
  REQUIRE(B >= 0, "%s: negative path count", fn);
  REQUIRE(grid >= 3 && grid <= 2147483647LL, "%s: %lld grid points, outside 3..2^31-1", fn, (long long)grid);
  REQUIRE(dt > 0.0 && std::isfinite(dt), "%s: dt must be positive and finite", fn);
  REQUIRE(M >= 1 && M <= 2147483647LL, "%s: %lld sample rows a path, outside 1..2^31-1", fn, (long long)M);
  const int64_t cap = (int64_t)1 << 60;
  REQUIRE(B == 0 || (M <= cap / B / n && grid <= cap / B / n), "%s: %lld paths of %lld rows and %lld grid points are not addressable", fn,
          (long long)B, (long long)M, (long long)grid);
  REQUIRE(grid_given == 0 || grid_given == 3, "%s: the grid source needs q, dq and ddq, all three", fn);
  REQUIRE(curve_given == 0 || curve_given == 6, "%s: the curve source needs status, count, points, cut, knot and length, all six", fn);
  REQUIRE((grid_given != 0) != (curve_given != 0), "%s: exactly one source of the geometry must be given, the grid or the curve", fn);
  REQUIRE(curve_given == 0 || (w_in >= 1 && w_in <= MP_BL_MAX_WAYPOINTS), "%s: %lld rows a path in the curve's tables, outside 1..65536", fn,
          (long long)w_in);
  MpSampleIn I;
  std::memset(&I, 0, sizeof I);
  I.dt = dt;
  I.B = (long)B; I.M = (int)M; I.grid = (int)grid; I.w_in = curve_given ? (int)w_in : 0;
  *out = I;
  return MP_OK;
}

extern "C" {

int mp_trajectory_sample_cpu_f64(const mp_model* model, const double* t, const double* x, int64_t B, int64_t N_grid, const double* q,
                                 const double* dq, const double* ddq, const int32_t* blend_status, const int32_t* blend_count,
                                 const double* points, const double* cut, const double* knot, const double* length, int64_t W_in, double dt,
                                 int64_t M_rows, const double* g, const double* Ftip, int32_t* status, int32_t* count, int32_t* needed,
                                 double* s, double* sd, double* sdd, double* positions, double* velocities, double* accelerations,
                                 double* torques, int nthreads) {
  const char* fn = "mp_trajectory_sample_cpu_f64";
  if (int rc = mp_small_model(fn, model)) return rc;
  MpSampleIn I;
  if (int rc = mp_trajectory_sample_check(fn, B, N_grid, W_in, dt, M_rows, model->d.n, (q != nullptr) + (dq != nullptr) + (ddq != nullptr),
                                          (blend_status != nullptr) + (blend_count != nullptr) + (points != nullptr) + (cut != nullptr) +
                                              (knot != nullptr) + (length != nullptr), &I))
    return rc;
  if (B == 0) return MP_OK;
  REQUIRE(t && x, "%s: null pointer", fn);
  const MpSampleOut O = {status, count, needed, s, sd, sdd, positions, velocities, accelerations, torques};
  REQUIRE(mp_out_any(O), "%s: at least one output is required", fn);
  I.t = t; I.x = x; I.q = q; I.dq = dq; I.ddq = ddq;
  I.bstatus = blend_status; I.bcount = blend_count; I.points = points; I.cut = cut; I.knot = knot; I.length = length;
  const MpModel<double>& M = model->d;
  const MpCall<double> C = make_call<double>(model, g, Ftip);
  const int tau = !torques ? MP_TS_NO_TAU : (any_nonzero(Ftip) ? MP_TS_TAU_FTIP : MP_TS_TAU);
  const bool curve = points != nullptr;
  MP_CPU_DISPATCH(M.n, {
    parallel_for(B, 1, nthreads, [&](int64_t b0, int64_t b1) {
      for (int64_t b = b0; b < b1; ++b) {
        if (curve) {
          if (tau == MP_TS_NO_TAU) mp_ts_path_cpu<N, MP_TS_CURVE, MP_TS_NO_TAU>(M, C, I, O, (long)b);
          else if (tau == MP_TS_TAU) mp_ts_path_cpu<N, MP_TS_CURVE, MP_TS_TAU>(M, C, I, O, (long)b);
          else mp_ts_path_cpu<N, MP_TS_CURVE, MP_TS_TAU_FTIP>(M, C, I, O, (long)b);
        } else {
          if (tau == MP_TS_NO_TAU) mp_ts_path_cpu<N, MP_TS_GRID, MP_TS_NO_TAU>(M, C, I, O, (long)b);
          else if (tau == MP_TS_TAU) mp_ts_path_cpu<N, MP_TS_GRID, MP_TS_TAU>(M, C, I, O, (long)b);
          else mp_ts_path_cpu<N, MP_TS_GRID, MP_TS_TAU_FTIP>(M, C, I, O, (long)b);
        }
      }
    });
  })
  return MP_OK;
}

}  // extern "C"
