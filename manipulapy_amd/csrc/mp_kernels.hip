// HIP kernels for gfx950 (MI355X): one thread per (trajectory, timestep) row.
//
// Layout in HBM: exactly the reference's API arrays — q / qd / qdd / tau are (rows, n) row-major
// ("array of rows"), T is (rows, 4, 4), J is (rows, 6, n), start/end are (B, n).  A wavefront's 64
// rows are one contiguous 64*n*sizeof(T) span per array, read/written with the widest vector access
// the row size allows (16 / 8 / 4 bytes per lane).  The robot model and the per-call constants are
// kernel ARGUMENTS (kernarg segment -> scalar loads -> SGPR operands): zero per-thread traffic.
// No MFMA: there is no dense contraction on this path (BASELINE.json north_star).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "mp_bodies.h"
#include "mp_deriv.h"
#include "mp_adjoint.h"
#include "mp_kin_vjp.h"
#include "mp_opspace.h"
#include "mp_dyn.h"
#include "mp_ik.h"
#include "mp_kernels.h"
#include "mp_regressor.h"
#include "mp_rollout_vjp.h"
#include "mp_ilqr.h"
#include "mp_toppra.h"
#include "mp_collision.h"
#include "mp_rrt.h"
#include "mp_shortcut.h"
#include "mp_goal.h"
#include "mp_blend.h"
#include "mp_cartesian.h"
#include "mp_sample.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPkMinWaves = 2;  // waves per SIMD asked for by the packed (two rows per lane) fused kernel: register cap = 512 / 2

// ------------------------------------------------------------------------------------- probe
__global__ void k_selftest(int* out) { out[threadIdx.x] = (int)threadIdx.x; }

// ------------------------------------------------------------------------- inverse dynamics
template <typename T, int N, bool HAS_FTIP>
__global__ __launch_bounds__(kBlock) void k_id(const MpModel<T> M, const MpCall<T> C, const T* __restrict__ q,
                                               const T* __restrict__ qd, const T* __restrict__ qdd,
                                               T* __restrict__ tau, long rows) {
  MP_COLD_BUFFER(N, kBlock, sizeof(T));
  const long r = (long)blockIdx.x * kBlock + threadIdx.x;
  if (r >= rows) return;
  mp_body_id<T, N, HAS_FTIP>(M, C, q, qd, qdd, tau, r, MP_COLD_PTR);
}

// The same with the model read through a pointer to device memory (scalar loads, K$-resident) instead of the kernel-argument
// struct: the joints' constants are then loaded joint by joint where the recursion uses them (mp_joint_of, mp_core.h), not all
// 185 dwords at the top of the kernel - which overflows the SGPR file into VGPR lanes (60 v_writelane / v_readlane of 1203
// instructions at n = 6) and keeps the wave count down.
// (five waves per SIMD asked for without a tip wrench, four with one: the float64 re-evaluation loop behind the float32 pass raised
// the unconstrained allocation from 85 to 106 VGPRs; held to 96 / 128 neither pass touches scratch)
// Round 5: the kernel's first L.blocks workgroups carry the float64 pass of an earlier launch of the same model (mp_body_id_lead, as
// the robot-specialised kernels do); the float64 path spills under this kernel's register cap - in those workgroups only.
// Round 6: ALLREV = the model holds revolute joints only (the launcher looks): the float32 rows read it as an MpModelRev, whose
// `rev` the recursion folds to 1 (csrc/mp_model.h) - 13 VALU instructions per joint fewer, no branch.
template <typename T, int N, bool HAS_FTIP, bool ALLREV = false>
__global__ __launch_bounds__(kBlock, HAS_FTIP ? 4 : 5) void k_id_dm(const MpModel<T>* __restrict__ Mdev, const MpCall<T> C, const T* __restrict__ q,
                                                  const T* __restrict__ qd, const T* __restrict__ qdd, T* __restrict__ tau, long rows,
                                                  const MpLead L) {
  MP_COLD_BUFFER(N, kBlock, sizeof(T));
  typedef const __attribute__((address_space(4))) MpModel<T> MC;
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (sizeof(T) == 4) {
    if (blockIdx.x < L.blocks) {
      mp_body_id_lead<N, HAS_FTIP>(*(MpModelConstD*)L.C.cold_model, *(MC*)Mdev, L);
      return;
    }
  }
#endif
  const long r = (long)(blockIdx.x - L.blocks) * kBlock + threadIdx.x;
  if (r >= rows) return;
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (ALLREV && sizeof(T) == 4) {
    mp_body_id<T, N, HAS_FTIP>(*(MpModelRevConstF*)Mdev, C, q, qd, qdd, tau, r, MP_COLD_PTR);
    return;
  }
#endif
  mp_body_id<T, N, HAS_FTIP>(*(MC*)Mdev, C, q, qd, qdd, tau, r, MP_COLD_PTR);
}

// The float64 pass over the rows k_id_dm handed over (mp_body_id_hard, csrc/mp_bodies.h): both models through device pointers.
template <int N, bool HAS_FTIP>
__global__ __launch_bounds__(64) void k_id_hard(const MpModel<float>* __restrict__ Mdev, const MpCall<float> C, const float* __restrict__ q,
                                                const float* __restrict__ qd, const float* __restrict__ qdd, float* __restrict__ tau, unsigned rows) {
#if defined(__HIP_DEVICE_COMPILE__)
  mp_body_id_hard<N, HAS_FTIP>(*(MpModelConstD*)C.cold_model, *(MpModelConstF*)Mdev, C,
                               [&](long r, float (&x)[N], float (&y)[N], float (&z)[N]) {
                                 RunIO<float, N>::load(q, r, x); RunIO<float, N>::load(qd, r, y); RunIO<float, N>::load(qdd, r, z);
                               }, tau, rows);
#endif
}

// ... up to four launches' lists in one kernel (blockIdx.y picks the launch), as the specialised programs' pass: a pass costs ~5 us of
// launch and latency however few rows it holds (round 5: the generic passes ran one kernel each until then)
template <int N, bool HAS_FTIP>
__global__ __launch_bounds__(64) void k_id_hard_batch(const MpModel<float>* __restrict__ Mdev, const MpHardBatch B) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int e = blockIdx.y;
  const float* __restrict__ q = B.q[e]; const float* __restrict__ qd = B.qd[e]; const float* __restrict__ qdd = B.qdd[e];
  mp_body_id_hard<N, HAS_FTIP>(*(MpModelConstD*)B.C[e].cold_model, *(MpModelConstF*)Mdev, B.C[e],
                               [&](long r, float (&x)[N], float (&y)[N], float (&z)[N]) {
                                 RunIO<float, N>::load(q, r, x); RunIO<float, N>::load(qd, r, y); RunIO<float, N>::load(qdd, r, z);
                               }, B.tau[e], B.rows[e]);
#endif
}

// the same pass for rows the fused generic kernel handed over: a row's inputs are generated again from start / end / the time table
template <int N, bool HAS_FTIP>
__global__ __launch_bounds__(64) void k_traj_id_hard(const MpModel<float>* __restrict__ Mdev, const MpCall<float> C, const float* __restrict__ start,
                                                     const float* __restrict__ end, unsigned Nt, const double* __restrict__ tab,
                                                     float* __restrict__ tau, unsigned rows) {
#if defined(__HIP_DEVICE_COMPILE__)
  MpModelConstF& M = *(MpModelConstF*)Mdev;
  mp_body_id_hard<N, HAS_FTIP>(*(MpModelConstD*)C.cold_model, M, C,
                               [&](long r, float (&x)[N], float (&y)[N], float (&z)[N]) {
                                 const unsigned b = (unsigned)r / Nt, t = (unsigned)r - b * Nt;
                                 float a[N], e[N];
                                 RunIO<float, N>::load(start, (long)b, a);
                                 RunIO<float, N>::load(end, (long)b, e);
                                 const double u0 = tab[3 * t], u1 = tab[3 * t + 1], u2 = tab[3 * t + 2];
#pragma unroll
                                 for (int j = 0; j < N; ++j) {
                                   const double d = (double)(e[j] - a[j]);
                                   x[j] = mp_clip((float)(u0 * d + (double)a[j]), M.qmin[j], M.qmax[j]);
                                   y[j] = (float)(u1 * d);
                                   z[j] = (float)(u2 * d);
                                 }
                               }, tau, rows);
#endif
}

// -------------------------------------------------------------- trajectory generation pieces
template <int N>
__global__ __launch_bounds__(kBlock) void k_batch_traj(const MpModel<float> M, const float* __restrict__ start,
                                                       const float* __restrict__ end, long B, long Nt, double Tf,
                                                       int method, float* __restrict__ pos, float* __restrict__ vel,
                                                       float* __restrict__ acc) {
  // A pure write kernel: a full wave's 64 consecutive rows of each output leave as whole lines, non-temporal, through LDS
  // (MpRowStage, csrc/mp_bodies.h); the last, partial wave stores per lane.  (Non-temporal PER-LANE stores of these 24-byte rows
  // halve the rate: 0.053 -> 0.096 ms.)
  using ST = MpRowStage<float, N>;
  __shared__ __attribute__((aligned(16))) char lds[kBlock / 64][3 * ST::SPAN];
  const long total = B * Nt;
  const long r = (long)blockIdx.x * kBlock + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  const long row0 = mp_wave_uniform(r - lane);   // (every lane is still active here: the flush addresses form on the scalar unit)
  if (row0 >= total) return;
  const bool full = row0 + 64 <= total;  // wave-uniform
  if (r >= total) return;                // (only in the partial wave)
  const long b = r / Nt, t = r - b * Nt;
  float p[N], v[N], a[N];
  traj_row<N>(M, start, end, b, t, Nt, Tf, method, p, v, a);
  if (full) {
    char* w = lds[threadIdx.x >> 6];
    ST::row_out(w, lane, p);
    ST::row_out(w + ST::SPAN, lane, v);
    ST::row_out(w + 2 * ST::SPAN, lane, a);
    ST::sync();
    ST::flush(pos, row0, lane, w);
    ST::flush(vel, row0, lane, w + ST::SPAN);
    ST::flush(acc, row0, lane, w + 2 * ST::SPAN);
  } else {
    RunIO<float, N>::store(pos, r, p);
    RunIO<float, N>::store(vel, r, v);
    RunIO<float, N>::store(acc, r, a);
  }
}

// (Generic float32 forms removed in round 6, each slower than what is left - the one-row kernel k_id_dm for given rows, the table-driven
// packed kernel k_traj_id_pk_tab for generated ones: k_id<float> / k_id_pk with the model in the kernel arguments (c2 0.126 / 0.119 ms
// against 0.100), k_traj_id / k_traj_id_pk with the time scaling per row (0.0577 against 0.0525 specialised); profiles/HISTORY.md.)

// per-call table of the time scaling, three doubles per timestep: exactly traj_row's arithmetic, once per timestep
// instead of once per row
__global__ __launch_bounds__(kBlock) void k_time_table(double* __restrict__ tab, long Nt, double Tf, int method) {
  const long t = (long)blockIdx.x * kBlock + threadIdx.x;
  if (t >= Nt) return;
  const double tt = (double)t * (Tf / (double)(Nt - 1));
  double s, sd, sdd;
  mp_time_scaling(method, tt / Tf, Tf, s, sd, sdd);
  tab[3 * t] = s; tab[3 * t + 1] = sd; tab[3 * t + 2] = sdd;
}

template <int N, bool HAS_FTIP>
__global__ __launch_bounds__(kBlock, kPkMinWaves) void k_traj_id_pk_tab(const MpModel<float> M, const MpCall<float> C,
                                                              const float* __restrict__ start, const float* __restrict__ end,
                                                              long Nt, unsigned bpt, const double* __restrict__ tab,
                                                              float* __restrict__ tau) {
  MP_COLD_BUFFER(N, kBlock, 4);
  long b, t0, t1;
  bool valid1;
  if (!mp_traj_pair(blockIdx.x, threadIdx.x, kBlock, bpt, Nt, b, t0, t1, valid1)) return;
  mp_body_traj_id_pk_tab<N, HAS_FTIP>(M, C, start, end, b, t0, t1, valid1, Nt, tab, tau, MP_COLD_PTR);
}

// ------------------------------------------------------------- FK + space Jacobian + ID fused
// one wave per block: the per-wave LDS staging slice (9 KiB) then never limits residency (a 256-thread block needs
// 36 KiB, i.e. at most 4 blocks = 16 waves per CU, and blocks drain unevenly: 1.7 waves per SIMD measured)
constexpr int kFkBlock = 64;

template <typename T, int N, bool HAS_FTIP>
__global__ __launch_bounds__(kFkBlock) void k_fk_jac_id(const MpModel<T> M, const MpCall<T> C, const T* __restrict__ q,
                                                      const T* __restrict__ qd, const T* __restrict__ qdd,
                                                      T* __restrict__ Tout, T* __restrict__ Jout,
                                                      T* __restrict__ tau, long rows) {
  __shared__ __attribute__((aligned(16))) char lds[(kFkBlock / 64) * MP_WAVE_LDS_BYTES];  // one staging slice per wave
  const long r = (long)blockIdx.x * kFkBlock + threadIdx.x;
  mp_body_fk_jac_id<T, N, HAS_FTIP>(M, C, q, qd, qdd, Tout, Jout, tau, r, rows, lds + (threadIdx.x >> 6) * MP_WAVE_LDS_BYTES);
}

// ------------------------------------------------------------- mass matrix / forward dynamics
// one wave per block; the N x N rows leave through the wave-cooperative coalesced store (see mp_bodies.h)
template <typename T, int N>
__global__ __launch_bounds__(kFkBlock) void k_mass_matrix(const MpModel<T> M, const T* __restrict__ q, T* __restrict__ Mout,
                                                          long rows) {
  __shared__ __attribute__((aligned(16))) char lds[MP_WAVE_LDS_BYTES];
  const int lane = (int)threadIdx.x;
  const long row0 = (long)blockIdx.x * kFkBlock;
  if (row0 >= rows) return;
  const long left = rows - row0;
  const int nvalid = left < 64 ? (int)left : 64;
  const long r = lane < nvalid ? row0 + lane : rows - 1;  // out-of-range lanes recompute the last row, store nothing
  T a[N];
  RunIO<T, N>::load(q, r, a);
  MpJointState<T, N> js;
  mp_joint_state<T, N>(M, a, js);
  T Mq[N][N];
  mp_mass_matrix_crba<T, N>(M, js, Mq);
  T flat[N * N];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) flat[i * N + j] = Mq[i][j];
  MpBad<T> bad;
  bad.add(a);
  mp_poison_if(bad.any(), flat);
  mp_wave_store_auto<T, N * N>(Mout, row0, lane, nvalid, flat, lds);
}

// qdd = forward_dynamics(q, qd, tau, g, Ftip) per row; Ftip is one wrench for every row (per-call constant)
template <typename T, int N, bool HAS_FTIP>
__global__ __launch_bounds__(kBlock) void k_forward_dynamics(const MpModel<T> M, const MpCall<T> C, const T* __restrict__ q,
                                                             const T* __restrict__ qd, const T* __restrict__ tau,
                                                             T* __restrict__ qdd, long rows) {
  const long r = (long)blockIdx.x * kBlock + threadIdx.x;
  if (r >= rows) return;
  mp_body_fd<T, N, HAS_FTIP>(M, C, q, qd, tau, qdd, r);
}

// ------------------------------------------------------- derivatives of inverse / forward dynamics (float64, mp_deriv.h)
// 64-lane blocks: the per-row state (~20 doubles a link kept for the sweeps) takes most of a lane's registers, and a small block
// lets the scheduler place the few waves a SIMD then holds anywhere
constexpr int kDerivBlock = 64;
template <int N, bool HAS_FTIP>
__global__ __launch_bounds__(kDerivBlock) void k_id_deriv(const MpModel<double> M, const MpCall<double> C, const double* __restrict__ q,
                                                          const double* __restrict__ qd, const double* __restrict__ qdd,
                                                          double* __restrict__ tau, double* __restrict__ dq, double* __restrict__ dqd,
                                                          double* __restrict__ Mout, long rows) {
  const long r = (long)blockIdx.x * kDerivBlock + threadIdx.x;
  if (r >= rows) return;
  mp_id_deriv_row<N, HAS_FTIP>(M, C, q, qd, qdd, tau, dq, dqd, Mout, r);
}
template <int N, bool HAS_FTIP>
__global__ __launch_bounds__(kDerivBlock) void k_fd_deriv(const MpModel<double> M, const MpCall<double> C, const double* __restrict__ q,
                                                          const double* __restrict__ qd, const double* __restrict__ tau,
                                                          double* __restrict__ qdd, double* __restrict__ dq, double* __restrict__ dqd,
                                                          double* __restrict__ Minv, long rows) {
  const long r = (long)blockIdx.x * kDerivBlock + threadIdx.x;
  if (r >= rows) return;
  mp_fd_deriv_row<N, HAS_FTIP>(M, C, q, qd, tau, qdd, dq, dqd, Minv, r);
}

// vector-Jacobian products by reverse mode (mp_adjoint.h): one lane per row, the block size of the derivative kernels
template <int N, bool HAS_FTIP>
__global__ __launch_bounds__(kDerivBlock) void k_id_vjp(const MpModel<double> M, const MpCall<double> C, const double* __restrict__ q,
                                                        const double* __restrict__ qd, const double* __restrict__ qdd,
                                                        const double* __restrict__ gtau, double* __restrict__ gq, double* __restrict__ gqd,
                                                        double* __restrict__ gqdd, long rows) {
  const long r = (long)blockIdx.x * kDerivBlock + threadIdx.x;
  if (r >= rows) return;
  mp_id_vjp_row<N, HAS_FTIP>(M, C, q, qd, qdd, gtau, gq, gqd, gqdd, r);
}
template <int N, bool HAS_FTIP>
__global__ __launch_bounds__(kDerivBlock) void k_fd_vjp(const MpModel<double> M, const MpCall<double> C, const double* __restrict__ q,
                                                        const double* __restrict__ qd, const double* __restrict__ tau,
                                                        const double* __restrict__ gqdd, double* __restrict__ qdd, double* __restrict__ gq,
                                                        double* __restrict__ gqd, double* __restrict__ gtau, long rows) {
  const long r = (long)blockIdx.x * kDerivBlock + threadIdx.x;
  if (r >= rows) return;
  mp_fd_vjp_row<N, HAS_FTIP>(M, C, q, qd, tau, gqdd, qdd, gq, gqd, gtau, r);
}

// ------------------------------------------------------- reverse mode through FK + Jacobian (float64, mp_kin_vjp.h)
// The mirror of mp_wave_store_flat for loads.  A lane that reads its own long cotangent row (gJ: 288 B at n = 6, 384 B at n = 8)
// issues loads whose lanes are a row apart: every instruction touches 64 lines (mp_bodies.h measured that pattern at 4.0 against
// 5.4 TB/s on stores).  Here a FULL wave reads its 64 consecutive rows as flat 16-byte chunks, non-temporal, so that one load
// instruction covers a contiguous kilobyte, and stages them 16 rows at a time in its LDS slice (mp_wave_store_flat's pitch: an odd
// number of chunks, conflict-free for the row reads), where the 16 lanes that own the rows pick them up.  The next pass's chunks are
// requested before the current pass is staged.
template <typename T, int COUNT>
__device__ __forceinline__ void mp_wave_load_flat(const T* __restrict__ gbase, long row0, int lane, T (&v)[COUNT],
                                                  char* __restrict__ lds) {
  constexpr int ROWB = COUNT * (int)sizeof(T), CH = ROWB / 16, ROWS = 16, TOTAL = ROWS * CH, NJ = (TOTAL + 63) / 64;
  static_assert(ROWB % 16 == 0, "rows of whole 16-byte chunks");
  constexpr int PITCH = (CH % 2 == 1) ? ROWB : ((ROWB + 127) / 128) * 128 + 16;
  static_assert(ROWS * PITCH <= MP_WAVE_LDS_BYTES, "wave staging slice too small");
  const mp_u4* g = reinterpret_cast<const mp_u4*>(gbase + row0 * COUNT);
  mp_u4 buf[2][NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (j * 64 + lane < TOTAL) buf[0][j] = mp_stream_load(g + j * 64 + lane);
#pragma unroll
  for (int pass = 0; pass < 64 / ROWS; ++pass) {
    if (pass + 1 < 64 / ROWS) {
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (j * 64 + lane < TOTAL) buf[(pass + 1) & 1][j] = mp_stream_load(g + (pass + 1) * TOTAL + j * 64 + lane);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int f = j * 64 + lane;  // flat chunk index inside this pass's 16 rows
      if (f < TOTAL) {
        const int row = f / CH, col = f - row * CH;
        *reinterpret_cast<mp_u4*>(lds + row * PITCH + col * 16) = buf[pass & 1][j];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if ((lane >> 4) == pass) {
      const T* src = reinterpret_cast<const T*>(lds + (lane & (ROWS - 1)) * PITCH);
#pragma unroll
      for (int e = 0; e < COUNT; ++e) v[e] = src[e];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// One lane per row, one wave per block (kFkBlock: the wave's LDS slice).  q moves as whole lines (MpRowStage), the cotangents through
// mp_wave_load_flat, T / J / g leave through the wave-cooperative stores; the last, partial wave reads per lane.  The cotangents are
// read only when gq is requested; a null cotangent is zero.  The pose cotangent is reduced to its 6-vector before gJ is read, so the
// 6N Jacobian columns and the 6N cotangents are the registers the sweep holds.
template <int N, int FRAME>
__global__ __launch_bounds__(kFkBlock) void k_fk_jac_vjp(const MpModel<double> M, const double* __restrict__ q,
                                                         const double* __restrict__ gT, const double* __restrict__ gJ,
                                                         double* __restrict__ Tout, double* __restrict__ Jout, double* __restrict__ gq,
                                                         long rows) {
  using ST = MpRowStage<double, N>;
  static_assert(ST::SPAN <= MP_WAVE_LDS_BYTES, "one array's 64 rows fit the wave's staging slice");
  __shared__ __attribute__((aligned(16))) char lds[MP_WAVE_LDS_BYTES];
  const int lane = (int)threadIdx.x;
  const long row0 = (long)blockIdx.x * kFkBlock;
  if (row0 >= rows) return;
  const long left = rows - row0;
  const int nvalid = left < 64 ? (int)left : 64;
  const bool full = nvalid == 64;
  const long rr = lane < nvalid ? row0 + lane : rows - 1;  // out-of-range lanes recompute the last row, store nothing
  double a[N];
  if (full) {
    mp_u4 bq[ST::NJ];
    ST::fetch(q, row0, lane, bq);
    ST::stage(bq, lane, lds);
    ST::sync();
    ST::row_in(lds, lane, a);
    ST::sync();
  } else {
    RunIO<double, N>::load(q, rr, a);
  }
  MpBad<double> bad;
  bad.add(a);
  double TT[16], JJ[6 * N], g[N];
  mp_kin_primal<double, N, FRAME>(M, a, TT, JJ);
  if (gq != nullptr) {
    double w[6];
    {
      double ct[16];
      if (gT == nullptr) {
#pragma unroll
        for (int k = 0; k < 16; ++k) ct[k] = 0.0;
      } else if (full) {
        mp_wave_load_flat<double, 16>(gT, row0, lane, ct, lds);
      } else {
        RunIO<double, 16>::load(gT, rr, ct);
      }
      bad.add(ct);
      mp_kin_pose_cotangent<double, FRAME>(TT, ct, w);
    }
    double cj[6 * N];
    if (gJ == nullptr) {
#pragma unroll
      for (int k = 0; k < 6 * N; ++k) cj[k] = 0.0;
    } else if (full) {
      mp_wave_load_flat<double, 6 * N>(gJ, row0, lane, cj, lds);
    } else {
      RunIO<double, 6 * N>::load(gJ, rr, cj);
    }
    bad.add(cj);
    mp_kin_sweep<double, N, FRAME>(JJ, w, cj, g);
  }
  const bool poison = bad.any();
  if (Tout != nullptr) {
    mp_poison_if(poison, TT);
    mp_wave_store_auto<double, 16>(Tout, row0, lane, nvalid, TT, lds);
  }
  if (Jout != nullptr) {
    mp_poison_if(poison, JJ);
    mp_wave_store_auto<double, 6 * N>(Jout, row0, lane, nvalid, JJ, lds);
  }
  if (gq != nullptr) {
    mp_poison_if(poison, g);
    mp_wave_store_auto<double, N>(gq, row0, lane, nvalid, g, lds);
  }
}

// ------------------------------------------------------- sphere-model collision distances, cost and gradients (float64, mp_collision.h)
// One lane per row, one wave per block.  q moves as whole lines (MpRowStage) and is the only per-row read; the sphere, pair and obstacle
// tables are read through constant-address-space pointers, so every lane of the wave visits the same sphere, obstacle and pair in step
// and the tables cost scalar loads only.  The world centres are parked in dynamic LDS as [sphere][xyz][lane] (24 S bytes a lane, sized
// by the launcher from the model's S) for the pair loop; the wave's static slice stages q and the row outputs.  The n-wide outputs
// leave through the wave-cooperative stores, the one- and two-value ones as one coalesced store a lane.
typedef const __attribute__((address_space(4))) MpColSpheres MpColSpheresConst;
typedef const __attribute__((address_space(4))) MpColPair MpColPairConst;
typedef const __attribute__((address_space(4))) MpColWorld MpColWorldConst;
typedef const __attribute__((address_space(4))) MpColObstacle MpColObstacleConst;
// The point cloud (mp_cloud.h): the header wave-uniform through the constant address space, cells and records per lane through the
// global one.  CLOUD = false gives the tables without the query: every sphere-model kernel has both instances, and the launcher takes
// the one without for a handle that has no cloud (MpColDevice::cloud), so such a launch runs the code it ran before there were clouds.
struct MpCloudPtrDevice {
  typedef const __attribute__((address_space(4))) MpColCloud* Header;
  typedef const __attribute__((address_space(1))) int* Cells;
  typedef const __attribute__((address_space(1))) MpCloudPoint* Points;
};
template <bool CLOUD> struct MpColTablesConstOf {
  typedef MpColTables<MpColSpheresConst*, MpColPairConst*, MpColWorldConst*, MpColObstacleConst*> type;
};
template <> struct MpColTablesConstOf<true> {
  typedef MpColTables<MpColSpheresConst*, MpColPairConst*, MpColWorldConst*, MpColObstacleConst*, MpCloudPtrDevice> type;
};
template <bool CLOUD>
__device__ __forceinline__ typename MpColTablesConstOf<CLOUD>::type mp_col_tables_const(const MpColSpheres* sph, const MpColPair* pairs,
                                                                                        const MpColWorld* world) {
  return {(MpColSpheresConst*)sph, (MpColPairConst*)pairs, (MpColWorldConst*)world, (MpColObstacleConst*)(world + 1)};
}
// The scaffold of the one-wave work-queue kernels on the sphere model (k_collision_edges, k_rrt_connect, k_path_shortcut, k_goal_ik, k_path_blend; DESIGN
// §4.10).  Their dynamic LDS, sized by mp_col_queue_lds_bytes (mp_collision.h): the park of S centres, then the edge's n (n + 1) / 2
// speed bounds [entry][lane] - per lane, but read at wave-uniform link numbers.  Each lane reads and writes only its own column of
// both, so no barrier is needed.
struct MpColQueueLanes {
  MpColParkLanes park;
  MpColBoundsLanes L;
};
__device__ __forceinline__ MpColQueueLanes mp_col_queue_lanes(double* lds, int lane, int S) {
  return {{lds + lane}, {lds + mp_col_queue_bounds_offset(S) + lane}};
}
// the wave-wide steps of the state machines of mp_rrt.h and mp_shortcut.h over the 64 lanes (the twins': MpWaveOpsSerial)
struct MpWaveOpsLanes {
  __device__ __forceinline__ int wave_max(int v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int w = __shfl_xor(v, o);
      v = w > v ? w : v;
    }
    return v;
  }
  __device__ __forceinline__ bool wave_any(bool b) const { return __any(b ? 1 : 0) != 0; }
};

template <int N, bool WANT_GRAD, bool CLOUD>
__global__ __launch_bounds__(64) void k_collision(const MpModel<double> M, const MpColSpheres* __restrict__ sph,
                                                  const MpColPair* __restrict__ pairs, const MpColWorld* __restrict__ world,
                                                  const double* __restrict__ q, long rows, double eps_world, double eps_self,
                                                  const MpColOut O) {
  using ST = MpRowStage<double, N>;
  static_assert(ST::SPAN <= MP_WAVE_LDS_BYTES, "one array's 64 rows fit the wave's staging slice");
  __shared__ __attribute__((aligned(16))) char lds[MP_WAVE_LDS_BYTES];
  extern __shared__ __attribute__((aligned(16))) double mp_col_park[];
  const int lane = (int)threadIdx.x;
  const long row0 = (long)blockIdx.x * 64;
  if (row0 >= rows) return;
  const long left = rows - row0;
  const int nvalid = left < 64 ? (int)left : 64;
  const long rr = lane < nvalid ? row0 + lane : rows - 1;  // out-of-range lanes recompute the last row, store nothing
  double a[N];
  if (nvalid == 64) {
    mp_u4 bq[ST::NJ];
    ST::fetch(q, row0, lane, bq);
    ST::stage(bq, lane, lds);
    ST::sync();
    ST::row_in(lds, lane, a);
    ST::sync();
  } else {
    RunIO<double, N>::load(q, rr, a);
  }
  MpBad<double> bad;
  bad.add(a);
  const auto tb = mp_col_tables_const<CLOUD>(sph, pairs, world);
  MpColParkLanes park{mp_col_park + lane};
  MpColRow<N> o;
  mp_collision_row<N, WANT_GRAD>(M, tb, a, eps_world, eps_self, park, o);
  mp_collision_poison<N, WANT_GRAD>(bad.any(), o);
  if (lane < nvalid) {
    if (O.dist_world != nullptr) O.dist_world[rr] = o.dist_world;
    if (O.dist_self != nullptr) O.dist_self[rr] = o.dist_self;
    if (O.cost != nullptr) O.cost[rr] = o.cost;
    if (O.arg_world != nullptr) *reinterpret_cast<int2*>(O.arg_world + 2 * rr) = make_int2(o.arg_world[0], o.arg_world[1]);
    if (O.arg_self != nullptr) *reinterpret_cast<int2*>(O.arg_self + 2 * rr) = make_int2(o.arg_self[0], o.arg_self[1]);
  }
  if constexpr (WANT_GRAD) {
    if (O.grad_dist_world != nullptr) mp_wave_store_auto<double, N>(O.grad_dist_world, row0, lane, nvalid, o.grad_dist_world, lds);
    if (O.grad_dist_self != nullptr) mp_wave_store_auto<double, N>(O.grad_dist_self, row0, lane, nvalid, o.grad_dist_self, lds);
    if (O.grad != nullptr) mp_wave_store_auto<double, N>(O.grad, row0, lane, nvalid, o.grad, lds);
  }
}

// ------------------------------------------------------- continuous collision checking of joint-space edges (float64, mp_collision.h)
// One wave per block (the park is [sphere][xyz][lane]), tables through constant-address-space pointers as in k_collision.  Work queue
// as in k_ik: a lane without an edge takes the next index from the device counter, every trip of the loop evaluates ONE configuration
// of the lane's own edge, and a finished lane writes its row and fetches another - iteration counts run from 1 to a few hundred between
// neighbouring edges.  The loop ends because the counter only grows and every edge ends within max_steps.  Dynamic LDS: the park and
// the speed bounds (mp_col_queue_lanes).  The 2 n inputs of an edge are plain per-lane loads.
template <int N, bool CLOUD>
__global__ __launch_bounds__(64) void k_collision_edges(const MpModel<double> M, const MpColSpheres* __restrict__ sph,
                                                        const MpColPair* __restrict__ pairs, const MpColWorld* __restrict__ world,
                                                        const double* __restrict__ q_from, const double* __restrict__ q_to, long edges,
                                                        const MpColEdgeParams P, const MpColEdgeOut O,
                                                        unsigned long long* __restrict__ next) {
  extern __shared__ __attribute__((aligned(16))) double mp_col_edge_lds[];
  const int lane = (int)threadIdx.x;
  const auto tb = mp_col_tables_const<CLOUD>(sph, pairs, world);
  MpColQueueLanes Q = mp_col_queue_lanes(mp_col_edge_lds, lane, tb.sph->S);
  MpColEdgeState<N> S;
  bool have = false;
  long row = 0;
  for (;;) {
    if (!have) {
      row = (long)atomicAdd(next, 1ull);
      if (row >= edges) break;
      double a[N], b[N];
      RunIO<double, N>::load(q_from, row, a);
      RunIO<double, N>::load(q_to, row, b);
      mp_col_edge_begin<N>(M, tb.sph, a, b, S, Q.L);
      have = true;
    }
    if (const int done = mp_col_edge_iterate<N>(M, tb, P, S, Q.park, Q.L)) {
      mp_col_edge_store<N>(O, row, S, done);
      have = false;
    }
  }
}

// ------------------------------------------------------- batched RRT-Connect over the sphere model (float64, mp_rrt.h)
// One wave per block and a work queue as in k_collision_edges: a lane without a problem takes the next index from the device counter,
// every trip of the loop does the selection work the lane's problem is waiting for and evaluates ONE configuration of its running
// edge, and a finished lane writes its row and fetches another.  Dynamic LDS: the park and the speed bounds (mp_col_queue_lanes).
// The trees live in the caller's workspace and belong to the resident lane, not to the problem: per block the
// nodes [tree][node][dim][lane] (doubles), then the parents [tree][node][lane] (int32); a new problem resets the lane's counts
// only.  Each lane reads and writes only its own column, in program order, so no barrier or fence is needed.  The nearest search
// (mp_rrt_nearest) is entered by all 64 lanes on every trip and runs to the wave's largest count, so the wave reads whole 512-byte
// lines; the loop of the kernel ends for the whole wave at once, when no lane holds a problem and the queue is empty.
struct MpRrtTreeLanes : MpWaveOpsLanes {
  double* nodes;  // already offset by the block and the lane
  int* parents;
  int max_nodes, n;
  __device__ __forceinline__ double get(int tree, int v, int j) const { return nodes[(((long)tree * max_nodes + v) * n + j) * 64]; }
  __device__ __forceinline__ void put(int tree, int v, int j, double x) { nodes[(((long)tree * max_nodes + v) * n + j) * 64] = x; }
  __device__ __forceinline__ int parent(int tree, int v) const { return parents[((long)tree * max_nodes + v) * 64]; }
  __device__ __forceinline__ void set_parent(int tree, int v, int p) { parents[((long)tree * max_nodes + v) * 64] = p; }
};

template <int N, bool CLOUD>
__global__ __launch_bounds__(64) void k_rrt_connect(const MpModel<double> M, const MpColSpheres* __restrict__ sph,
                                                    const MpColPair* __restrict__ pairs, const MpColWorld* __restrict__ world,
                                                    const double* __restrict__ q_start, const double* __restrict__ q_goal, long problems,
                                                    const MpRrtParams P, const MpRrtOut O, double* __restrict__ workspace,
                                                    unsigned long long* __restrict__ next) {
  extern __shared__ __attribute__((aligned(16))) double mp_rrt_lds[];
  const int lane = (int)threadIdx.x;
  const auto tb = mp_col_tables_const<CLOUD>(sph, pairs, world);
  MpColQueueLanes Q = mp_col_queue_lanes(mp_rrt_lds, lane, tb.sph->S);
  const size_t node_words = (size_t)2 * (size_t)P.max_nodes * N * 64;                  // doubles a block
  const size_t block_words = node_words + (size_t)P.max_nodes * 64;                   // + 2 max_nodes 64 int32
  double* const mine = workspace + (size_t)blockIdx.x * block_words;
  MpRrtTreeLanes T{{}, mine + lane, reinterpret_cast<int*>(mine + node_words) + lane, P.max_nodes, N};
  MpRrtState<N> S;
  S.phase = MP_RRT_IDLE;
  S.done = 0;
  bool have = false, dry = false;
  long row = 0;
  for (;;) {
    if (!have && !dry) {
      row = (long)atomicAdd(next, 1ull);
      if (row >= problems) {
        dry = true;
      } else {
        double a[N], b[N];
        RunIO<double, N>::load(q_start, row, a);
        RunIO<double, N>::load(q_goal, row, b);
        mp_rrt_begin<N>(M, tb, P, a, b, S, T, Q.L, O.waypoints != nullptr ? O.waypoints + row * (long)P.max_waypoints * N : nullptr);
        have = true;
      }
    }
    if (!T.wave_any(have)) break;
    double* wp = (have && O.waypoints != nullptr) ? O.waypoints + row * (long)P.max_waypoints * N : nullptr;
    if (mp_rrt_trip<N>(M, tb, P, S, T, Q.park, Q.L, wp)) {
      mp_rrt_store<N>(O, row, S);
      have = false;
      S.phase = MP_RRT_IDLE;
    }
  }
}

// ------------------------------------------------------- batched path shortcutting over the sphere model (float64, mp_shortcut.h)
// One wave per block and the work queue of k_collision_edges / k_rrt_connect: a lane without a problem takes the next index from the
// device counter, every trip of the loop does the selection work the lane's problem is waiting for and evaluates ONE configuration
// of its running edge, and a finished lane writes its row and fetches another.  Dynamic LDS: the park and the speed bounds
// (mp_col_queue_lanes).  The working path lives in the caller's workspace and belongs to the resident lane, not to the
// problem: per block the waypoints [waypoint][dim][lane] (doubles), then the cumulative lengths [waypoint][lane]; a lane that takes
// a new problem copies its count_in rows in.  Each lane reads and writes only its own column, in program order, so no barrier or
// fence is needed.  The locate scan (mp_shortcut_locate) is entered by all 64 lanes on every pass and runs to the wave's largest m,
// so the wave reads whole 512-byte lines; the splice and the recomputation of the lengths after an accepted shortcut are per lane.
// The loop of the kernel ends for the whole wave at once, when no lane holds a problem and the queue is empty.
struct MpShortcutPathLanes : MpWaveOpsLanes {
  double* pts;  // already offset by the block and the lane
  double* cum;
  int n;
  __device__ __forceinline__ double get(int w, int j) const { return pts[((long)w * n + j) * 64]; }
  __device__ __forceinline__ void put(int w, int j, double x) { pts[((long)w * n + j) * 64] = x; }
  __device__ __forceinline__ double len(int w) const { return cum[(long)w * 64]; }
  __device__ __forceinline__ void set_len(int w, double x) { cum[(long)w * 64] = x; }
};

template <int N, bool CLOUD>
__global__ __launch_bounds__(64) void k_path_shortcut(const MpModel<double> M, const MpColSpheres* __restrict__ sph,
                                                      const MpColPair* __restrict__ pairs, const MpColWorld* __restrict__ world,
                                                      const double* __restrict__ waypoints_in, const int* __restrict__ count_in,
                                                      long problems, const MpShortcutParams P, const MpShortcutOut O,
                                                      double* __restrict__ workspace, unsigned long long* __restrict__ next) {
  extern __shared__ __attribute__((aligned(16))) double mp_shortcut_lds[];
  const int lane = (int)threadIdx.x;
  const auto tb = mp_col_tables_const<CLOUD>(sph, pairs, world);
  MpColQueueLanes Q = mp_col_queue_lanes(mp_shortcut_lds, lane, tb.sph->S);
  const size_t point_words = (size_t)P.max_waypoints * N * 64;           // doubles a block
  const size_t block_words = point_words + (size_t)P.max_waypoints * 64;  // + the lengths
  double* const mine = workspace + (size_t)blockIdx.x * block_words;
  MpShortcutPathLanes T{{}, mine + lane, mine + point_words + lane, N};
  MpShortcutState<N> S;
  S.phase = MP_SC_IDLE;
  S.done = 0;
  S.m = 0;
  bool have = false, dry = false;
  long row = 0;
  for (;;) {
    if (!have && !dry) {
      row = (long)atomicAdd(next, 1ull);
      if (row >= problems) {
        dry = true;
      } else {
        mp_shortcut_begin<N>(P, waypoints_in + row * (long)P.w_in * N, count_in[row], S, T,
                             O.waypoints != nullptr ? O.waypoints + row * (long)P.max_waypoints * N : nullptr);
        have = true;
      }
    }
    if (!T.wave_any(have)) break;
    double* wp = (have && O.waypoints != nullptr) ? O.waypoints + row * (long)P.max_waypoints * N : nullptr;
    if (mp_shortcut_trip<N>(M, tb, P, S, T, Q.park, Q.L, wp)) {
      mp_shortcut_store<N>(O, row, S, T);
      have = false;
      S.phase = MP_SC_IDLE;
      S.m = 0;
    }
  }
}

// ------------------------------------------------------- goal configurations for pose goals over the sphere model (float64, mp_goal.h)
// One wave per block and the work queue of k_collision_edges / k_rrt_connect: a lane without a problem takes the next index from the
// device counter, every trip of the loop does at most one pose evaluation with its step for a lane that is iterating and - only if
// some lane of the wave has just converged - the one collision evaluation of such a lane, and a finished lane writes its row and
// fetches another.  Dynamic LDS: the park and the speed bounds (mp_col_queue_lanes), which only the collision evaluation touches.
// All of a problem's state is in registers: no workspace.  The loop of the kernel ends for the whole wave at once, when no lane holds
// a problem and the queue is empty; it ends because the counter only grows and every problem ends within
// max_attempts (max_iters + 2) trips.
template <int N, bool CLOUD>
__global__ __launch_bounds__(64) void k_goal_ik(const MpModel<double> M, const MpColSpheres* __restrict__ sph,
                                                const MpColPair* __restrict__ pairs, const MpColWorld* __restrict__ world,
                                                const double* __restrict__ T_goal, const double* __restrict__ q_seed, long problems,
                                                const MpGoalParams P, const MpGoalOut O, unsigned long long* __restrict__ next) {
  extern __shared__ __attribute__((aligned(16))) double mp_goal_lds[];
  const int lane = (int)threadIdx.x;
  const auto tb = mp_col_tables_const<CLOUD>(sph, pairs, world);
  MpColQueueLanes Q = mp_col_queue_lanes(mp_goal_lds, lane, tb.sph->S);
  const MpWaveOpsLanes W{};
  MpGoalState<N> S;
  S.phase = MP_GOAL_IDLE;
  bool have = false, dry = false;
  long row = 0;
  for (;;) {
    if (!have && !dry) {
      row = (long)atomicAdd(next, 1ull);
      if (row >= problems) {
        dry = true;
      } else {
        mp_goal_begin<N>(P, T_goal + 16 * row, q_seed + row * N, S);
        have = true;
      }
    }
    if (!W.wave_any(have)) break;
    if (mp_goal_trip<N>(M, tb, P, S, W, Q.park, Q.L, T_goal + 16 * (have ? row : 0))) {
      mp_goal_store<N>(O, row, S);
      have = false;
      S.phase = MP_GOAL_IDLE;
    }
  }
}

// ------------------------------------------------------- C2 corner blending of waypoint paths (float64, mp_blend.h)
// One wave per block and the work queue of k_collision_edges / k_goal_ik: a lane without a problem takes the next index from the
// device counter and screens, compacts and sets it up (mp_blend_begin), every trip of the loop makes ONE collision evaluation of the
// lane's running attempt, and a finished lane writes its row and fetches another.  Dynamic LDS: the park and the speed bounds
// (mp_col_queue_lanes).  A problem's state is its corner, in registers; the next corner is read from the lane's own input rows: no
// workspace.  The loop of the kernel ends for the whole wave at once, when no lane holds a problem and the queue is empty; it ends
// because the counter only grows and every problem ends within (count_in - 2) (max_halvings + 1) max_steps trips.
template <int N, bool CLOUD>
__global__ __launch_bounds__(64) void k_path_blend(const MpModel<double> M, const MpColSpheres* __restrict__ sph,
                                                   const MpColPair* __restrict__ pairs, const MpColWorld* __restrict__ world,
                                                   const double* __restrict__ waypoints_in, const int* __restrict__ count_in,
                                                   long problems, const MpBlendParams P, const MpBlendOut O,
                                                   unsigned long long* __restrict__ next) {
  extern __shared__ __attribute__((aligned(16))) double mp_blend_lds[];
  const int lane = (int)threadIdx.x;
  const auto tb = mp_col_tables_const<CLOUD>(sph, pairs, world);
  MpColQueueLanes Q = mp_col_queue_lanes(mp_blend_lds, lane, tb.sph->S);
  const MpWaveOpsLanes W{};
  MpBlendState<N> S;
  S.phase = MP_BL_IDLE;
  bool have = false, dry = false;
  long row = 0;
  int cin = 0;
  MpBlendRows o = {nullptr, nullptr, nullptr};
  for (;;) {
    if (!have && !dry) {
      row = (long)atomicAdd(next, 1ull);
      if (row >= problems) {
        dry = true;
        row = 0;
      } else {
        cin = count_in[row];
        o = mp_blend_rows(O, row, P.w_in, N);
        mp_blend_begin<N>(M, tb.sph, P, waypoints_in + row * (long)P.w_in * N, cin, S, Q.L, o);
        have = true;
      }
    }
    if (!W.wave_any(have)) break;
    if (mp_blend_trip<N>(M, tb, P, waypoints_in + row * (long)P.w_in * N, cin, S, Q.park, Q.L, o)) {
      mp_blend_store<N>(O, row, S);
      have = false;
      S.phase = MP_BL_IDLE;
    }
  }
}

// The grid of the blended curves: one lane a grid point over problems x grid rows, one wave per block.  A lane finds its piece by a
// binary search of the problem's knots, evaluates the closed forms (mp_blend_sample) and the wave stores its 64 rows of q, dq/ds,
// d2q/ds2 as whole lines (mp_wave_store_auto): 24 n bytes a row written, a few table entries read.  The lanes of the last, partial
// wave that have no row recompute the last one and store nothing.
template <int N>
__global__ __launch_bounds__(64) void k_path_blend_sample(long problems, int grid, int w_in, const int* __restrict__ status,
                                                          const int* __restrict__ count, const double* __restrict__ points,
                                                          const double* __restrict__ cut, const double* __restrict__ knot,
                                                          const double* __restrict__ length, double* __restrict__ q,
                                                          double* __restrict__ dq, double* __restrict__ ddq) {
  __shared__ __attribute__((aligned(16))) char lds[MP_WAVE_LDS_BYTES];
  const int lane = (int)threadIdx.x;
  const long rows = problems * grid;
  const long row0 = (long)blockIdx.x * 64;
  if (row0 >= rows) return;
  const long left = rows - row0;
  const int nvalid = left < 64 ? (int)left : 64;
  const long rr = lane < nvalid ? row0 + lane : rows - 1;
  const long b = rr / grid;
  const int i = (int)(rr - b * grid);
  double x[N], dx[N], ddx[N];
  mp_blend_sample<N>(status[b], count[b], length[b], points + b * (long)w_in * N, cut + b * (long)w_in, knot + b * (long)w_in, i, grid, x, dx,
                     ddx);
  if (q != nullptr) mp_wave_store_auto<double, N>(q, row0, lane, nvalid, x, lds);
  if (dq != nullptr) mp_wave_store_auto<double, N>(dq, row0, lane, nvalid, dx, lds);
  if (ddq != nullptr) mp_wave_store_auto<double, N>(ddq, row0, lane, nvalid, ddx, lds);
}

// ------------------------------------------------------- Cartesian straight-line paths, proven free (float64, mp_cartesian.h)
// Tracking: one lane per problem, sequential over its grid, a plain grid and no LDS - a problem's state (q, dq, the line's V and start
// pose) is in registers, the targets are recomputed from s.  A lane stores its own rows as it accepts them (RunIO-style plain per-lane
// stores, as k_goal_ik stores its q) and its head into the workspace.
template <int N, int MR>
__global__ __launch_bounds__(64) void k_cart_track(const MpModel<double> M, const MpCartParams P, const double* __restrict__ q_start,
                                                   const double* __restrict__ T_goal, long problems, const MpCartWork W,
                                                   double* __restrict__ q, double* __restrict__ dq, double* __restrict__ ddq) {
  const long b = (long)blockIdx.x * 64 + (long)threadIdx.x;
  if (b >= problems) return;
  const long at = b * (long)P.grid * N;
  MpCartHead H;
  mp_cart_track<N, MR>(M, P, q_start + b * N, T_goal + 16 * b, q + at, dq + at, ddq + at, H);
  mp_cart_head_store(W, b, H);
}

// The spans: one wave per block and the work queue of k_collision_edges over problems x (grid - 1) spans, ONE LANE PER SPAN - the
// spans of a problem are independent once its rows stand, so they spread over the lanes instead of being walked by the problem's
// own.  A lane without a span takes the next index from the device counter; the span of a problem that was not tracked to its end is
// recorded SKIPPED at once; otherwise mp_cart_span_begin (bounds, midpoint deviation) and then one collision evaluation a trip.  The
// span's two grid rows are re-read from memory every trip (mp_ts_hermite reads them in place): the state in registers is u, the
// clearance and two counters.  Dynamic LDS: the park and the speed bounds (mp_col_queue_lanes).  No wave-wide step: a lane leaves when
// the queue is dry.  The loop ends because the counter only grows and every span ends within max_steps trips.
template <int N, int MR, bool CLOUD>
__global__ __launch_bounds__(64) void k_cart_span(const MpModel<double> M, const MpColSpheres* __restrict__ sph,
                                                  const MpColPair* __restrict__ pairs, const MpColWorld* __restrict__ world,
                                                  const MpCartParams P, const double* __restrict__ T_goal, long problems,
                                                  const MpCartWork W, const double* __restrict__ q, const double* __restrict__ dq,
                                                  const double* __restrict__ ddq, unsigned long long* __restrict__ next) {
  extern __shared__ __attribute__((aligned(16))) double mp_cart_lds[];
  const int lane = (int)threadIdx.x;
  const auto tb = mp_col_tables_const<CLOUD>(sph, pairs, world);
  MpColQueueLanes Q = mp_col_queue_lanes(mp_cart_lds, lane, tb.sph->S);
  const long per = (long)(P.grid - 1), spans = problems * per;
  const double nm1 = (double)(P.grid - 1);
  MpCartSpan S;
  bool have = false;
  long e = 0, r = 0;
  for (;;) {
    if (!have) {
      e = (long)atomicAdd(next, 1ull);
      if (e >= spans) break;
      const long b = e / per;
      const int i = (int)(e - b * per);
      if (W.track[b] != MP_CP_DONE) {
        mp_cart_span_skip(W, e);
        continue;
      }
      const long at = b * (long)P.grid * N;
      r = at + (long)i * N;
      mp_cart_span_begin<N, MR>(M, tb.sph, q + r, dq + r, ddq + r, q + at, T_goal + 16 * b, nm1, ((double)i + 0.5) / nm1, S, Q.L);
      have = true;
    }
    if (const int done = mp_cart_span_iterate<N>(M, tb, P.edge, q + r, dq + r, ddq + r, nm1, S, Q.park, Q.L)) {
      S.status = done - 1;
      mp_cart_span_store(W, e, S);
      have = false;
    }
  }
}

// The reduction: one lane per problem walks its spans' records in order (mp_cart_reduce) - what a problem reports is a function of
// the records, whichever lanes wrote them.
__global__ __launch_bounds__(64) void k_cart_reduce(long problems, int grid, const MpCartWork W, const MpCartOut O) {
  const long b = (long)blockIdx.x * 64 + (long)threadIdx.x;
  if (b >= problems) return;
  mp_cart_reduce(W, b, grid, O);
}

// ------------------------------------------------------- fixed-rate sampling of timed paths (float64, mp_sample.h)
// One lane a (path, sample) row over B x M rows, one wave per block, a block takes the tiles of 64 rows blockIdx.x, + gridDim.x, ...
// The 64 rows of a tile belong to paths bf..bl; the wave screens each of them once, its lanes sharing the scan of the path's tables
// (flags OR-ed over the wave: the same bits as the twin's walk), and a lane keeps the flags of its own path.  Neighbouring lanes are
// neighbouring samples of one path: their searches of the time stamps and their reads of the interval's rows hit the same lines.  The
// rows go out as whole lines (mp_wave_store_auto), s / sd / sdd per lane (a tile's 64 values are one run), status / count / needed
// by the lane that holds a path's row 0.  The lanes of the last, partial tile that have no row recompute the last one and store nothing.
template <int N, int SOURCE, int TAU>
__global__ __launch_bounds__(64) void k_traj_sample(const MpModel<double> M, const MpCall<double> C, const MpSampleIn I, const MpSampleOut O,
                                                    long tiles) {
  __shared__ __attribute__((aligned(16))) char lds[MP_WAVE_LDS_BYTES];
  const int lane = (int)threadIdx.x;
  const long rows = I.B * I.M;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long row0 = tile * 64, left = rows - row0;
    const int nvalid = left < 64 ? (int)left : 64;
    const long rr = lane < nvalid ? row0 + lane : rows - 1;
    const long b = rr / I.M, k = rr - b * I.M;
    const long bf = row0 / I.M, bl = (row0 + nvalid - 1) / I.M;
    int flags = 0;
    for (long p = bf; p <= bl; ++p) {
      const int f = mp_ts_scan<SOURCE>(I, N, p, lane, 64);
      const int all = (__any(f & MP_TS_F_NAN) ? MP_TS_F_NAN : 0) | (__any(f & MP_TS_F_STOP) ? MP_TS_F_STOP : 0) |
                      (__any(f & MP_TS_F_BAD) ? MP_TS_F_BAD : 0);
      if (p == b) flags = all;
    }
    const MpSampleHead H = mp_ts_head<SOURCE>(I, b, flags);
    MpSampleRow<N> o;
    mp_ts_row<N, SOURCE, TAU>(M, C, I, b, H, k, o);
    if (k == 0 && lane < nvalid) {
      if (O.status != nullptr) O.status[b] = H.status;
      if (O.count != nullptr) O.count[b] = H.count;
      if (O.needed != nullptr) O.needed[b] = H.needed;
    }
    if (lane < nvalid) {
      if (O.s != nullptr) O.s[rr] = o.s;
      if (O.sd != nullptr) O.sd[rr] = o.sd;
      if (O.sdd != nullptr) O.sdd[rr] = o.sdd;
    }
    if (O.pos != nullptr) mp_wave_store_auto<double, N>(O.pos, row0, lane, nvalid, o.q, lds);
    if (O.vel != nullptr) mp_wave_store_auto<double, N>(O.vel, row0, lane, nvalid, o.qd, lds);
    if (O.acc != nullptr) mp_wave_store_auto<double, N>(O.acc, row0, lane, nvalid, o.qdd, lds);
    if (TAU != MP_TS_NO_TAU) mp_wave_store_auto<double, N>(O.tau, row0, lane, nvalid, o.tau, lds);
  }
}

// ------------------------------------------------------- operational-space dynamics and torque (float64, mp_opspace.h)
// One lane per row, one wave per block.  A full wave moves its 64 rows of q / qd as whole lines (MpRowStage, two regions of the
// wave's slice); the last, partial wave reads per lane and its out-of-range lanes recompute the last row and store nothing.
template <int N>
__device__ __forceinline__ void mp_os_rows_in(const double* __restrict__ q, const double* __restrict__ qd, long row0, long rr, int lane,
                                              bool full, double (&a)[N], double (&b)[N], char* __restrict__ lds) {
  using ST = MpRowStage<double, N>;
  static_assert(2 * ST::SPAN <= MP_WAVE_LDS_BYTES, "two arrays' 64 rows fit the wave's staging slice");
  if (full) {
    mp_u4 bq[ST::NJ], bd[ST::NJ];
    ST::fetch(q, row0, lane, bq);
    ST::fetch(qd, row0, lane, bd);
    ST::stage(bq, lane, lds);
    ST::stage(bd, lane, lds + ST::SPAN);
    ST::sync();
    ST::row_in(lds, lane, a);
    ST::row_in(lds + ST::SPAN, lane, b);
    ST::sync();
  } else {
    RunIO<double, N>::load(q, rr, a);
    RunIO<double, N>::load(qd, rr, b);
  }
}
// one more (rows, COUNT) input array, the same way
template <int COUNT>
__device__ __forceinline__ void mp_os_row_in(const double* __restrict__ x, long row0, long rr, int lane, bool full, double (&v)[COUNT],
                                             char* __restrict__ lds) {
  using ST = MpRowStage<double, COUNT>;
  if (full) {
    mp_u4 bx[ST::NJ];
    ST::fetch(x, row0, lane, bx);
    ST::stage(bx, lane, lds);
    ST::sync();
    ST::row_in(lds, lane, v);
    ST::sync();
  } else {
    RunIO<double, COUNT>::load(x, rr, v);
  }
}

// the wave-cooperative stores of k_fk_jac_vjp as mp_opspace_row's output functor: every lane of the wave calls it
struct MpOsWaveOut {
  long row0;
  int lane, nvalid;
  char* lds;
  template <int COUNT>
  __device__ __forceinline__ void operator()(double* __restrict__ base, const double (&v)[COUNT]) const {
    mp_wave_store_auto<double, COUNT>(base, row0, lane, nvalid, v, lds);
  }
};

// T, J, Jdot qd, Lambda, Jbar, mu, p of every row: frame / task / the null outputs are wave-uniform branches of one instance per N
template <int N>
__global__ __launch_bounds__(kDerivBlock) void k_opspace(const MpModel<double> M, const MpCall<double> C, int frame, int task, double lam2,
                                                         const double* __restrict__ q, const double* __restrict__ qd,
                                                         double* __restrict__ Tout, double* __restrict__ Jout, double* __restrict__ Jdqd,
                                                         double* __restrict__ Lam, double* __restrict__ Jbar, double* __restrict__ mu,
                                                         double* __restrict__ p, long rows) {
  __shared__ __attribute__((aligned(16))) char lds[MP_WAVE_LDS_BYTES];
  const int lane = (int)threadIdx.x;
  const long row0 = (long)blockIdx.x * kDerivBlock;
  if (row0 >= rows) return;
  const long left = rows - row0;
  const int nvalid = left < 64 ? (int)left : 64;
  const long rr = lane < nvalid ? row0 + lane : rows - 1;
  double a[N], b[N];
  mp_os_rows_in<N>(q, qd, row0, rr, lane, nvalid == 64, a, b, lds);
  MpBad<double> bad;
  bad.add(a); bad.add(b);
  const MpOsWaveOut out{row0, lane, nvalid, lds};
  mp_opspace_row<N>(M, C, frame, task, lam2, a, b, bad.any(), out, Tout, Jout, Jdqd, Lam, Jbar, mu, p);
}

// The hot path: q, qd, the task acceleration (rows, m) and tau0 (rows, n; may be null) in, tau (rows, n) out - nothing wider than a
// row of n values touches memory.
template <int N>
__global__ __launch_bounds__(kDerivBlock) void k_opspace_torque(const MpModel<double> M, const MpCall<double> C, int frame, int task,
                                                                double lam2, const double* __restrict__ q, const double* __restrict__ qd,
                                                                const double* __restrict__ acc, const double* __restrict__ tau0,
                                                                double* __restrict__ tau, long rows) {
  using ST = MpRowStage<double, N>;
  __shared__ __attribute__((aligned(16))) char lds[MP_WAVE_LDS_BYTES];
  const int lane = (int)threadIdx.x;
  const long row0 = (long)blockIdx.x * kDerivBlock;
  if (row0 >= rows) return;
  const long left = rows - row0;
  const int nvalid = left < 64 ? (int)left : 64;
  const bool full = nvalid == 64;
  const long rr = lane < nvalid ? row0 + lane : rows - 1;
  double a[N], b[N], x[6], t0[N], t[N];
  mp_os_rows_in<N>(q, qd, row0, rr, lane, full, a, b, lds);
  if (task == 0) {
    mp_os_row_in<6>(acc, row0, rr, lane, full, x, lds);
  } else {
    double x3[3];
    mp_os_row_in<3>(acc, row0, rr, lane, full, x3, lds);
    x[0] = x3[0]; x[1] = x3[1]; x[2] = x3[2]; x[3] = 0.0; x[4] = 0.0; x[5] = 0.0;
  }
  if (tau0 != nullptr) {
    mp_os_row_in<N>(tau0, row0, rr, lane, full, t0, lds);
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k) t0[k] = 0.0;
  }
  MpBad<double> bad;
  bad.add(a); bad.add(b); bad.add(x); bad.add(t0);
  mp_opspace_torque_row<N>(M, C, frame, task, lam2, a, b, x, t0, bad.any(), t);
  if (full) {
    ST::row_out(lds, lane, t);
    ST::sync();
    ST::flush(tau, row0, lane, lds);
  } else if (lane < nvalid) {
    RunIO<double, N>::store(tau, rr, t);
  }
}

// reverse mode through the roll-out (mp_rollout_vjp.h): one lane = one trajectory on the time-major layout, so that the 64 lanes of a
// wave read and write neighbouring rows at every step; the workspace is time-major too (row i of trajectory b at (i B + b) 2n)
template <int N, bool HAS_FTIP>
__global__ __launch_bounds__(kDerivBlock) void k_fd_traj_vjp(const MpModel<double> M, const MpCall<double> C, const double* __restrict__ th0,
                                                             const double* __restrict__ dth0, const double* __restrict__ taumat,
                                                             const double* __restrict__ Fm, long B, long Nt, double h, int intRes,
                                                             const double* __restrict__ gp, const double* __restrict__ gv,
                                                             const double* __restrict__ ga, double* __restrict__ work,
                                                             double* __restrict__ gth0, double* __restrict__ gdth0, double* __restrict__ gtau) {
  const long b = (long)blockIdx.x * kDerivBlock + threadIdx.x;
  if (b >= B) return;
  const long o = b * N;
  double* ck = work + b * (2 * N);
  double* sub = work + B * Nt * (2 * N) + b * (2 * N);
  mp_fd_traj_vjp<N, HAS_FTIP>(M, C, th0 + o, dth0 + o, taumat + o, HAS_FTIP ? Fm + b * 6 : nullptr, B, Nt, h, intRes, gp ? gp + o : nullptr,
                              gv ? gv + o : nullptr, ga ? ga + o : nullptr, ck, B, sub, B, gth0 + o, gdth0 + o, gtau + o);
}

// batched iLQR (mp_ilqr.h), one lane = one trajectory on the time-major layout like k_fd_traj_vjp.  The 2n x 2n value matrix and its
// products live in `work` (element e of trajectory b at e B + b: a wave's lanes touch one run of doubles).  K / k rows: time-major
// (N, B, *) or, kbm = 1, batch-major (B, N, *), which is what the host form hands back.
template <int N>
__global__ __launch_bounds__(kDerivBlock) void k_ilqr_backward(const MpModel<double> M, const MpIlqrWeights Wt, const double* __restrict__ pos,
                                                               const double* __restrict__ vel, const double* __restrict__ tau,
                                                               const double* __restrict__ dq, const double* __restrict__ dqd,
                                                               const double* __restrict__ Minv, const double* __restrict__ xref,
                                                               const double* __restrict__ reg, long B, long Nt, double h, int kbm,
                                                               double* __restrict__ work, double* __restrict__ K, double* __restrict__ k,
                                                               double* __restrict__ dV, int* __restrict__ status) {
  const long b = (long)blockIdx.x * kDerivBlock + threadIdx.x;
  if (b >= B) return;
  const long o = b * N, kb = kbm ? b * Nt : b, ks = kbm ? 1 : B;
  mp_ilqr_backward<N>(M, pos + o, vel + o, tau + o, B, Nt, h, dq + b * (N * N), dqd + b * (N * N), Minv + b * (N * N), B, xref + b * (2 * N),
                      B, Wt.wq, Wt.wr, Wt.wf, reg[b], work + b, B, K + kb * (2 * N * N), k + kb * N, ks, dV + b * 2, status + b);
}

// The cooperative form (mp_ilqr.h): 16 lanes a trajectory, four trajectories a wave, one wave a workgroup.  S, R / G, Qux, K, Quu and the
// step's blocks sit in LDS (7.3 KB a trajectory at n = 8); nothing but the inputs, K and k touches global memory.  A group past the end
// of the batch runs trajectory B - 1 along (the barriers need every lane) and stores nothing.
template <int N>
__global__ __launch_bounds__(64) void k_ilqr_backward_coop(const MpModel<double> M, const MpIlqrWeights Wt, const double* __restrict__ pos,
                                                           const double* __restrict__ vel, const double* __restrict__ tau,
                                                           const double* __restrict__ dq, const double* __restrict__ dqd,
                                                           const double* __restrict__ Minv, const double* __restrict__ xref,
                                                           const double* __restrict__ reg, long B, long Nt, double h, int kbm,
                                                           double* __restrict__ K, double* __restrict__ k, double* __restrict__ dV,
                                                           int* __restrict__ status) {
  __shared__ MpIlqrShared<N> shared[4];
  const int grp = (int)threadIdx.x >> 4, lane = (int)threadIdx.x & 15;
  long b = (long)blockIdx.x * 4 + grp;
  const bool act = b < B;
  if (!act) b = B - 1;
  const long o = b * N, kb = kbm ? b * Nt : b, ks = kbm ? 1 : B;
  const MpIlqrArgs A{pos + o, vel + o, tau + o, B, Nt, h, dq + b * (N * N), dqd + b * (N * N), Minv + b * (N * N), B, xref + b * (2 * N), B,
                     Wt.wq, Wt.wr, Wt.wf, reg[b], K + kb * (2 * N * N), k + kb * N, ks, dV + b * 2, status + b, act};
  MpIlqrShared<N>& sh = shared[grp];
  MpIlqrLane<N> L;
  mp_ilqr_coop_phase<N>(MP_ILQR_PH_INIT, 0, M, A, sh, L, lane);
  __syncthreads();
  for (long i = Nt - 1; i >= 1; --i) {
    mp_ilqr_coop_phase<N>(0, i, M, A, sh, L, lane); __syncthreads();
    mp_ilqr_coop_phase<N>(1, i, M, A, sh, L, lane); __syncthreads();
    mp_ilqr_coop_phase<N>(2, i, M, A, sh, L, lane); __syncthreads();
    mp_ilqr_coop_phase<N>(3, i, M, A, sh, L, lane); __syncthreads();
    mp_ilqr_coop_phase<N>(4, i, M, A, sh, L, lane); __syncthreads();
    mp_ilqr_coop_phase<N>(5, i, M, A, sh, L, lane); __syncthreads();
  }
  mp_ilqr_coop_phase<N>(MP_ILQR_PH_FLAG, 0, M, A, sh, L, lane);
  __syncthreads();
  mp_ilqr_coop_phase<N>(MP_ILQR_PH_FINAL, 0, M, A, sh, L, lane);
}

// one lane per (candidate a, trajectory b): lane l = a B + b reads trajectory b's nominal and gains and writes column l of the outputs
template <int N>
__global__ __launch_bounds__(kDerivBlock) void k_ilqr_rollout(const MpModel<double> M, const MpCall<double> C, const MpIlqrWeights Wt,
                                                              const double* __restrict__ th0, const double* __restrict__ dth0,
                                                              const double* __restrict__ tau, const double* __restrict__ pos,
                                                              const double* __restrict__ vel, const double* __restrict__ K,
                                                              const double* __restrict__ k, const double* __restrict__ alpha,
                                                              const double* __restrict__ xref, long A, long B, long Nt, double h, int kbm,
                                                              double* __restrict__ cost, double* __restrict__ opos,
                                                              double* __restrict__ ovel, double* __restrict__ otau) {
  const long l = (long)blockIdx.x * kDerivBlock + threadIdx.x;
  if (l >= A * B) return;
  const long b = l % B, o = b * N, kb = kbm ? b * Nt : b, ks = kbm ? 1 : B;
  mp_ilqr_rollout<N>(M, C, th0 + o, dth0 + o, tau + o, K ? pos + o : nullptr, K ? vel + o : nullptr, B, K ? K + kb * (2 * N * N) : nullptr,
                     K ? k + kb * N : nullptr, ks, alpha[l], xref + b * (2 * N), B, Wt.wq, Wt.wr, Wt.wf, Nt, h, cost + l,
                     opos ? opos + l * N : nullptr, opos ? ovel + l * N : nullptr, opos ? otau + l * N : nullptr, A * B);
}

// ------------------------------------------------------- time-optimal path parameterisation (float64, mp_toppra.h)
// The path-dynamics coefficients: one lane per grid row, like k_id_deriv; reads 3 n doubles a row, writes 3 n + 1
template <int N, bool HAS_FTIP>
__global__ __launch_bounds__(kDerivBlock) void k_path_coeffs(const MpModel<double> M, const MpCall<double> C, const MpToppraVmax V,
                                                             const double* __restrict__ q, const double* __restrict__ dq,
                                                             const double* __restrict__ ddq, double* __restrict__ a, double* __restrict__ b,
                                                             double* __restrict__ c, double* __restrict__ xbar, long rows) {
  const long r = (long)blockIdx.x * kDerivBlock + threadIdx.x;
  if (r >= rows) return;
  mp_path_coeffs_row<N, HAS_FTIP>(M, C, V, q, dq, ddq, a, b, c, xbar, r);
}

// The sweep: one lane per path on the time-major layout like k_fd_traj_vjp, so a wave's lanes read one run of doubles a row.  A
// sequential chain of Nt - 1 small LPs and Nt - 1 forward steps per lane: latency-bound, not bandwidth-bound.  K is written by the
// backward pass and read back by the same lane in the forward pass (no __restrict__ on it).
template <int N, bool ACC>
__global__ __launch_bounds__(kDerivBlock) void k_toppra_sweep(const MpToppraLimits lim, const double* __restrict__ a,
                                                              const double* __restrict__ b, const double* __restrict__ c,
                                                              const double* __restrict__ xbar, const double* __restrict__ dq,
                                                              const double* __restrict__ ddq, const double* __restrict__ sd_start,
                                                              const double* __restrict__ sd_end, long B, long Nt, double* K,
                                                              double* __restrict__ x, double* __restrict__ u, double* __restrict__ t,
                                                              double* __restrict__ dur, int* __restrict__ status, double* __restrict__ oqd,
                                                              double* __restrict__ oqdd, double* __restrict__ otau) {
  const long p = (long)blockIdx.x * kDerivBlock + threadIdx.x;
  if (p >= B) return;
  const long o = p * N;
  mp_toppra_sweep<N, ACC>(lim, a + o, b + o, c + o, xbar + p, dq ? dq + o : nullptr, ddq ? ddq + o : nullptr, B, Nt, sd_start[p], sd_end[p],
                          K + 2 * p, x + p, u + p, t + p, dur + p, status + p, otau ? oqd + o : nullptr, otau ? oqdd + o : nullptr,
                          otau ? otau + o : nullptr);
}

// The epilogue as a launch of its own: one lane per row, reads 5 n + 2 doubles, writes 3 n
template <int N>
__global__ __launch_bounds__(kDerivBlock) void k_path_rows(const double* __restrict__ a, const double* __restrict__ b,
                                                           const double* __restrict__ c, const double* __restrict__ dq,
                                                           const double* __restrict__ ddq, const double* __restrict__ x,
                                                           const double* __restrict__ u, double* __restrict__ oqd, double* __restrict__ oqdd,
                                                           double* __restrict__ otau, long rows) {
  const long r = (long)blockIdx.x * kDerivBlock + threadIdx.x;
  if (r >= rows) return;
  mp_path_rows_row<N>(a, b, c, dq, ddq, x[r], u[r], oqd, oqdd, otau, r);
}

// ------------------------------------------------------- dynamics regressor (float64, mp_regressor.h)
// One lane per row, like k_id_deriv: write-bound (10 n^2 doubles a row)
template <int N, bool HAS_FTIP>
__global__ __launch_bounds__(kDerivBlock) void k_id_regressor(const MpModel<double> M, const double* __restrict__ Dmap,
                                                              const MpCall<double> C, const double* __restrict__ q,
                                                              const double* __restrict__ qd, const double* __restrict__ qdd,
                                                              double* __restrict__ Y, double* __restrict__ tau_ext, long rows) {
  const long r = (long)blockIdx.x * kDerivBlock + threadIdx.x;
  if (r >= rows) return;
  mp_id_regressor_row<N, HAS_FTIP>(M, Dmap, C, q, qd, qdd, Y, tau_ext, r);
}

// Normal equations, fused: one wave a workgroup, a fixed grid striding over tiles of T = 64 / LANES rows.  Per tile, LANES lanes
// build each row's Y (its n rows of 10n) and its residual rhs - tau_ext into LDS; then lane L < 55 adds the tile's n T rows of Y
// into its n x n register block (bi, bj), bi <= bj, of the upper triangle of A (10 blocks a side, whatever n), every lane one or
// two entries of b, lane 63 the squared residuals.  The wave's partials go to `work` once at the end; nothing reaches memory per row.
template <int N, bool HAS_FTIP, bool WITH_A>
__global__ __launch_bounds__(64) void k_id_regressor_normal(const MpModel<double> M, const double* __restrict__ Dmap,
                                                            const MpCall<double> C, const double* __restrict__ q,
                                                            const double* __restrict__ qd, const double* __restrict__ qdd,
                                                            const double* __restrict__ rhs, long rows, double* __restrict__ work) {
  constexpr int LANES = kRegNormalLanes, T = 64 / LANES, W = MP_REG_P * N, R = T * N;
  static_assert(MP_REG_P % LANES == 0, "lanes per row must divide the 10 parameters");
  __shared__ double Ys[R * W];
  __shared__ double Rs[R];
  const int L = threadIdx.x;
  const int t = L / LANES, sub = L % LANES;
  int bi = 0, rem = L < 55 ? L : 0;  // (bi, bj) = the L-th upper block in row order
  while (rem >= 10 - bi) { rem -= 10 - bi; ++bi; }
  const int bj = bi + rem;
  double acc[N][N];
#pragma unroll
  for (int x = 0; x < N; ++x)
#pragma unroll
    for (int y = 0; y < N; ++y) acc[x][y] = 0.0;
  double ab0 = 0.0, ab1 = 0.0, arr = 0.0;
  const long tiles = (rows + T - 1) / T;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long r = tile * T + t;
    if (t < T) {
      double* yrow = Ys + t * N * W;
      if (r < rows) {
        mp_id_regressor_normal_part<N, HAS_FTIP, LANES>(
            M, Dmap, C, q, qd, qdd, rhs, r, sub, [&](int j, int col, double v) { yrow[j * W + col] = v; },
            [&](int j, double v) { Rs[t * N + j] = v; });
      } else {  // past the last row: zeros
        for (int e = sub; e < N * W; e += LANES) yrow[e] = 0.0;
        if (sub == 0)
          for (int j = 0; j < N; ++j) Rs[t * N + j] = 0.0;
      }
    }
    __syncthreads();
    for (int row = 0; row < R; ++row) {
      const double* y = Ys + row * W;
      const double res = Rs[row];
      if (WITH_A) {
        double u[N], v[N];
#pragma unroll
        for (int x = 0; x < N; ++x) { u[x] = y[bi * N + x]; v[x] = y[bj * N + x]; }
#pragma unroll
        for (int x = 0; x < N; ++x)
#pragma unroll
          for (int z = 0; z < N; ++z) acc[x][z] += u[x] * v[z];
      }
      if (L < W) ab0 += y[L] * res;
      if (L + 64 < W) ab1 += y[L + 64] * res;
      if (L == 63) arr += res * res;
    }
    __syncthreads();
  }
  double* out = work + (long)blockIdx.x * mp_reg_normal_stride(N);
  if (WITH_A && L < 55) {
#pragma unroll
    for (int x = 0; x < N; ++x)
#pragma unroll
      for (int z = 0; z < N; ++z) out[(bi * N + x) * W + bj * N + z] = acc[x][z];
  }
  if (L < W) out[W * W + L] = ab0;
  if (L + 64 < W) out[W * W + L + 64] = ab1;
  if (L == 63) out[W * W + W] = arr;
}
// The partials added in workgroup order (four interleaved sums, then combined: a fixed order, so repeat calls are bit-identical).
// A entry (i, j) is read from the upper block that holds (i, j) or (j, i): A comes out exactly symmetric.
template <int N>
__global__ __launch_bounds__(256) void k_id_regressor_normal_reduce(const double* __restrict__ work, int groups, bool with_a,
                                                                    double* __restrict__ A, double* __restrict__ b,
                                                                    double* __restrict__ rr) {
  constexpr int W = MP_REG_P * N;
  const int e = (int)(blockIdx.x * 256 + threadIdx.x);
  const int first = with_a ? 0 : W * W;
  if (first + e >= W * W + W + 1) return;
  const int o = first + e;
  int src = o;
  if (o < W * W) {
    const int i = o / W, j = o % W;
    src = (i / N <= j / N) ? o : j * W + i;
  }
  const long stride = mp_reg_normal_stride(N);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int g = 0;
  for (; g + 3 < groups; g += 4) {
    s0 += work[(long)g * stride + src];
    s1 += work[(long)(g + 1) * stride + src];
    s2 += work[(long)(g + 2) * stride + src];
    s3 += work[(long)(g + 3) * stride + src];
  }
  for (; g < groups; ++g) s0 += work[(long)g * stride + src];
  const double v = (s0 + s1) + (s2 + s3);
  if (o < W * W) A[o] = v;
  else if (o < W * W + W) b[o - W * W] = v;
  else rr[0] = v;
}

// one wave per block: the roll-out's LDS tile is per wave and nothing is shared between waves
constexpr int kFdBlock = 64;
template <typename T, int N, bool HAS_FTIP>
__global__ __launch_bounds__(kFdBlock, (sizeof(T) == 4 ? 2 : 1)) void k_fd_traj(const MpModel<T> M, const MpCall<T> C, const T* __restrict__ theta0,
                                                      const T* __restrict__ dtheta0, const T* __restrict__ taumat,
                                                      const T* __restrict__ Ftipmat, long B, long Nt, T h, int intRes,
                                                      float* __restrict__ pos, float* __restrict__ vel, float* __restrict__ acc) {
  __shared__ unsigned lds[MpFdTile<T, N, HAS_FTIP>::DWORDS];
  const long b = (long)blockIdx.x * kFdBlock + threadIdx.x;  // lanes past the batch stay (wave-cooperative stores)
  mp_body_fd_traj<T, N, HAS_FTIP>(M, C, theta0, dtheta0, taumat, Ftipmat, b, B, Nt, h, intRes, pos, vel, acc, lds, (int)threadIdx.x);
}

// the roll-out on the time-major device layout (mp_body_fd_traj_tm): no LDS, 64-thread blocks so that the 2048 waves of a
// 131072-trajectory shard spread evenly over the 1024 SIMDs
template <typename T, int N, bool HAS_FTIP>
__global__ __launch_bounds__(kFdBlock, 2) void k_fd_traj_tm(const MpModel<T> M, const MpCall<T> C, const T* __restrict__ theta0,
                                                            const T* __restrict__ dtheta0, const T* __restrict__ taumat,
                                                            const T* __restrict__ Ftipmat, long B, long Nt, T h, int intRes,
                                                            float* __restrict__ pos, float* __restrict__ vel, float* __restrict__ acc) {
  const long b0 = (long)blockIdx.x * kFdBlock;  // one wave per block: its first trajectory is wave-uniform
  if (b0 + threadIdx.x >= B) return;
  mp_body_fd_traj_tm<T, N, HAS_FTIP>(M, C, theta0, dtheta0, taumat, Ftipmat, b0, (int)threadIdx.x, B, Nt, h, intRes, pos, vel, acc);
}

// (outer, inner, W dwords) -> (inner, outer, W dwords), see mp_body_transpose_rows
__global__ __launch_bounds__(kBlock) void k_transpose_rows(const unsigned* __restrict__ src, unsigned* __restrict__ dst, long outer,
                                                           long inner, int W) {
  extern __shared__ unsigned tr_lds[];
  const int TI = mp_tr_ti(W);
  const unsigned gx = (unsigned)((inner + TI - 1) / TI);  // tiles along `inner`; the grid is one-dimensional
  const unsigned ty = blockIdx.x / gx, tx = blockIdx.x - ty * gx;
  mp_body_transpose_rows(src, dst, outer, inner, W, (long)ty * MP_TR_TO, (long)tx * TI, tr_lds, (int)threadIdx.x, kBlock);
}

// ------------------------------------------------------------------- Cartesian straight-line path
// one lane per (pose pair b, timestep i); outputs float32 (B,N,3) x3 and (B,N,3,3).
// `bpt` blocks of 256 timesteps per pose pair: the pair's rotation logarithm (acos, the half-turn branches) is worked
// out once per block by lane 0 and broadcast through LDS together with the start rotation and the end points, so a lane
// neither reloads two 4x4 poses nor repeats the logarithm, and there is no row -> (pair, timestep) division
__global__ __launch_bounds__(kBlock) void k_cartesian_traj(const double* __restrict__ Xstart, const double* __restrict__ Xend,
                                                           long Nt, unsigned bpt, double Tf, int method, float* __restrict__ pos,
                                                           float* __restrict__ vel, float* __restrict__ acc,
                                                           float* __restrict__ ori) {
  __shared__ double sh[18];  // w (3), Rs (9), ps (3), pe (3)
  const unsigned bb = blockIdx.x / bpt;
  const long b = bb, i = (long)(blockIdx.x - bb * bpt) * kBlock + threadIdx.x;
  if (threadIdx.x == 0) {
    double Xs[16], Xe[16], w[3];
    RunIO<double, 16>::load(Xstart, b, Xs);
    RunIO<double, 16>::load(Xend, b, Xe);
    mp_cartesian_prepare(Xs, Xe, w);
    sh[0] = w[0]; sh[1] = w[1]; sh[2] = w[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) sh[3 + 3 * r + c] = Xs[4 * r + c];
      sh[12 + r] = Xs[4 * r + 3];
      sh[15 + r] = Xe[4 * r + 3];
    }
  }
  __syncthreads();
  if (i >= Nt) return;
  double w[3], Rs[9], ps[3], pe[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { w[k] = sh[k]; ps[k] = sh[12 + k]; pe[k] = sh[15 + k]; }
#pragma unroll
  for (int k = 0; k < 9; ++k) Rs[k] = sh[3 + k];
  float p[3], v[3], a[3], o[9];
  mp_cartesian_eval(Rs, ps, pe, w, i, Nt, Tf, method, p, v, a, o);
  const long r = b * Nt + i;
#pragma unroll
  for (int k = 0; k < 3; ++k) { pos[r * 3 + k] = p[k]; vel[r * 3 + k] = v[k]; acc[r * 3 + k] = a[k]; }
#pragma unroll
  for (int k = 0; k < 9; ++k) ori[r * 9 + k] = o[k];
}

// ------------------------------------------------------------------- fused potential field
// Per point: U = 1/2 |p - goal|^2 + sum_obs 1/2 (1/d - 1/d0)^2 over obstacles with 0 < d < d0, and its gradient
// (reference cuda_kernels/field_kernels.py:20-104 / :113-161, float32).  One lane per point; the obstacle index is
// wave-uniform, so obstacle coordinates arrive through scalar loads.
__global__ __launch_bounds__(kBlock) void k_potential_field(const float* __restrict__ pos, float gx, float gy, float gz,
                                                            const float* __restrict__ obs, long P, long O, float inv_d0,
                                                            float d0sq, float* __restrict__ pot, float* __restrict__ grad) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= P) return;
  const float px = pos[3 * i], py = pos[3 * i + 1], pz = pos[3 * i + 2];
  float dx = px - gx, dy = py - gy, dz = pz - gz;
  float U = 0.5f * (dx * dx + dy * dy + dz * dz);
  float Gx = dx, Gy = dy, Gz = dz;
  for (long o = 0; o < O; ++o) {
    const float ox = px - obs[3 * o], oy = py - obs[3 * o + 1], oz = pz - obs[3 * o + 2];
    const float d2 = ox * ox + oy * oy + oz * oz;
    if (d2 > 0.0f && d2 < d0sq) {
      const float inv = __builtin_amdgcn_rsqf(d2);  // v_rsq_f32, 1 ulp: the divide-after-sqrt sequence it replaces is ~15 instructions of ~40
      const float t = inv - inv_d0;
      U += 0.5f * t * t;
      const float f = -t * inv * inv * inv;
      Gx += f * ox; Gy += f * oy; Gz += f * oz;
    }
  }
  pot[i] = U;
  grad[3 * i] = Gx; grad[3 * i + 1] = Gy; grad[3 * i + 2] = Gz;
}

// ------------------------------------------------------------------- batched inverse kinematics
// Work queue: a lane that finishes its pose target takes the next unsolved one from a global counter instead of idling
// until the slowest problem of its wave is done (iteration counts vary from a handful to max_iterations; with one
// fixed problem per lane nearly every wave contains a straggler).  Every trip of the loop either fetches a problem or
// advances one by a single iteration, so the lanes of a wave keep executing the same code on different problems.
// Exit: the counter passes B for every lane eventually (it only grows), so every wave drains.  float64 throughout: the
// reference's default tolerances are 1e-6 rad / 1e-6 m.
template <int N>
__global__ __launch_bounds__(kBlock) void k_ik(const MpModel<double> M, const MpIkParams P, const double* __restrict__ Tdes,
                                               const double* __restrict__ theta0, long B, double* __restrict__ theta,
                                               int* __restrict__ success, int* __restrict__ iterations,
                                               int* __restrict__ restarts, unsigned long long* __restrict__ next) {
  MpIkState<N> S;
  bool have = false;
  long row = 0;
  for (;;) {
    if (!have) {
      row = (long)atomicAdd(next, 1ull);
      if (row >= B) break;
      RunIO<double, N>::load(theta0, row, S.theta);
      mp_ik_begin(S, P);
      have = true;
    }
    if (const int done = mp_ik_iterate<N>(M, P, S, Tdes + row * 16, theta0 + row * N)) {
      RunIO<double, N>::store(theta, row, S.theta);
      success[row] = done == 2 ? 1 : 0;
      iterations[row] = S.k + 1;
      restarts[row] = S.restarts;
      have = false;
    }
  }
}

// ------------------------------------------------------------------- 9..32 joints: run-time-n kernels (csrc/mp_dyn.h)
// One lane per row (or per trajectory), the model read through a pointer to device memory, per-joint state in indexed
// arrays.  Plain per-lane accesses: these kernels exist so that every robot the reference can evaluate computes here too.
// CAP = the capacity of those arrays (MP_MID_DOF or MP_BIG_DOF; the launchers pick it from the joint count).
template <typename T> using MpBigConst = const __attribute__((address_space(4))) MpBigModel<T>;

template <int CAP, typename T, bool HAS_FTIP>
__global__ __launch_bounds__(kBlock) void k_dyn_fk_jac_id(const MpBigModel<T>* __restrict__ Mdev, const MpCall<T> C,
                                                          const T* __restrict__ q, const T* __restrict__ qd, const T* __restrict__ qdd,
                                                          T* __restrict__ Tout, T* __restrict__ Jout, T* __restrict__ tau, long rows) {
  const long r = (long)blockIdx.x * kBlock + threadIdx.x;
  if (r >= rows) return;
  mp_dyn_row_fk_jac_id<CAP, T, HAS_FTIP>(*(MpBigConst<T>*)Mdev, C, q, qd, qdd, Tout, Jout, tau, r);
}
template <int CAP, typename T>
__global__ __launch_bounds__(kBlock) void k_dyn_mass_matrix(const MpBigModel<T>* __restrict__ Mdev, const T* __restrict__ q,
                                                            T* __restrict__ Mout, long rows) {
  const long r = (long)blockIdx.x * kBlock + threadIdx.x;
  if (r >= rows) return;
  mp_dyn_row_mass_matrix<CAP, T>(*(MpBigConst<T>*)Mdev, q, Mout, r);
}
template <int CAP, typename T, bool HAS_FTIP>
__global__ __launch_bounds__(kBlock) void k_dyn_forward_dynamics(const MpBigModel<T>* __restrict__ Mdev, const MpCall<T> C,
                                                                 const T* __restrict__ q, const T* __restrict__ qd,
                                                                 const T* __restrict__ tau, T* __restrict__ qdd, long rows) {
  const long r = (long)blockIdx.x * kBlock + threadIdx.x;
  if (r >= rows) return;
  mp_dyn_row_forward_dynamics<CAP, T, HAS_FTIP>(*(MpBigConst<T>*)Mdev, C, q, qd, tau, qdd, r);
}
template <int CAP, typename T, bool HAS_FTIP>
__global__ __launch_bounds__(64) void k_dyn_fd_traj(const MpBigModel<T>* __restrict__ Mdev, const MpCall<T> C,
                                                    const T* __restrict__ theta0, const T* __restrict__ dtheta0,
                                                    const T* __restrict__ taumat, const T* __restrict__ Ftipmat, long B, long Nt, T h,
                                                    int intRes, float* __restrict__ pos, float* __restrict__ vel,
                                                    float* __restrict__ acc, int time_major) {
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  mp_dyn_rollout<CAP, T, HAS_FTIP>(*(MpBigConst<T>*)Mdev, C, theta0, dtheta0, taumat, Ftipmat, b, B, Nt, h, intRes, pos, vel, acc,
                              time_major != 0);
}
template <int CAP, bool HAS_FTIP>
__global__ __launch_bounds__(kBlock) void k_dyn_traj(const MpBigModel<float>* __restrict__ Mdev, const MpCall<float> C,
                                                     const float* __restrict__ start, const float* __restrict__ end, long B, long Nt,
                                                     double Tf, int method, float* __restrict__ pos, float* __restrict__ vel,
                                                     float* __restrict__ acc, float* __restrict__ tau) {
  const long r = (long)blockIdx.x * kBlock + threadIdx.x;
  if (r >= B * Nt) return;
  const long b = r / Nt;
  mp_dyn_row_traj<CAP, HAS_FTIP>(*(MpBigConst<float>*)Mdev, C, start, end, b, r - b * Nt, Nt, Tf, method, pos, vel, acc, tau);
}

// ---------------------------------------------------------------------------------- launching
constexpr int kWave = 64;  // the block of the kernels declared __launch_bounds__(64): one wave

// The one grid rule: the blocks for `items` at `per_block` lanes or rows a block, rounded up (`y`: the grid's second dimension).
// A grid holds at most 2^31 - 1 blocks along x; beyond that `ok` is false and launch() refuses.
struct MpGrid { unsigned x, y; bool ok; };
constexpr long kMaxGrid = 0x7fffffffL;
constexpr long mp_blocks(long items, long per_block) { return items > 0 ? (items - 1) / per_block + 1 : 0; }
constexpr MpGrid mp_grid(long items, long per_block, long y = 1) {
  return {(unsigned)mp_blocks(items, per_block), (unsigned)y, mp_blocks(items, per_block) <= kMaxGrid};
}
// ... and a grid of a x b blocks along x (blocks per trajectory x trajectories, tiles x tiles): the product is checked
constexpr MpGrid mp_grid2(long a, long b) {
  return a < 0 || b < 0 || a > kMaxGrid || b > kMaxGrid ? MpGrid{0, 1, false} : mp_grid(a * b, 1);
}
static_assert(mp_grid(0, 64).x == 0 && mp_grid(0, 64).ok && mp_grid(1, 64).x == 1 && mp_grid(64, 64).x == 1 && mp_grid(65, 64).x == 2 &&
              mp_grid(256, 256).x == 1 && mp_grid(257, 256).x == 2 && mp_grid(65, 64).y == 1 && mp_grid(65, 64).ok, "rounds up");
static_assert(mp_grid(kMaxGrid * 64, 64).ok && mp_grid(kMaxGrid * 64, 64).x == 0x7fffffffu && !mp_grid(kMaxGrid * 64 + 1, 64).ok &&
              mp_grid(kMaxGrid * 256, 256).ok && !mp_grid(kMaxGrid * 256 + 1, 256).ok, "2^31 - 1 blocks are the most");
static_assert(mp_grid2(3, 5).x == 15 && mp_grid2(3, 5).ok && mp_grid2(0, 5).x == 0 && mp_grid2(kMaxGrid, 1).ok && !mp_grid2(kMaxGrid, 2).ok &&
              mp_grid2(46340, 46340).ok && !mp_grid2(46341, 46341).ok && !mp_grid2(kMaxGrid + 1, 1).ok, "the product is what is bounded");

// The one launch - the only place that spells it.  Typed on the kernel's own parameters P..., the arguments bound as const P& outside
// template deduction: they convert to the kernel's types here exactly as at a launch written out (bool -> int, long -> unsigned, a
// const T* const -> const T* __restrict__), a by-value struct such as the model is bound, not copied a second time, and a list that
// does not fit does not compile.  No runtime query, no allocation.
template <typename P> struct MpArg { typedef P type; };  // (keeps the arguments out of template deduction)
template <typename... P>
hipError_t launch(void (*kernel)(P...), MpGrid grid, int block, size_t lds, hipStream_t s, const typename MpArg<P>::type&... args) {
  if (!grid.ok) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3(grid.x, grid.y), dim3(block), lds, s, args...);
  return hipGetLastError();
}

// A launcher names its kernel's arguments ONCE: MP_DISPATCH_N / MP_DISPATCH_CAP bind the run-time joint count to the constant N / CAP,
// MP_FLAG binds a run-time bool to a constexpr bool NAME, and each expands its body once per value - so the body,
// `return launch(k_x<N, NAME>, grid, block, lds, s, <arguments>)`, is written one time whatever the number of instances.  MP_FLAG nests.
#define MP_FLAG(flag, NAME, ...)                      \
  if (flag) { constexpr bool NAME = true; __VA_ARGS__; } \
  else { constexpr bool NAME = false; __VA_ARGS__; }
#define MP_DISPATCH_N(n, ...)                                   \
  switch (n) {                                                  \
    case 1: { constexpr int N = 1; __VA_ARGS__; } break;        \
    case 2: { constexpr int N = 2; __VA_ARGS__; } break;        \
    case 3: { constexpr int N = 3; __VA_ARGS__; } break;        \
    case 4: { constexpr int N = 4; __VA_ARGS__; } break;        \
    case 5: { constexpr int N = 5; __VA_ARGS__; } break;        \
    case 6: { constexpr int N = 6; __VA_ARGS__; } break;        \
    case 7: { constexpr int N = 7; __VA_ARGS__; } break;        \
    case 8: { constexpr int N = 8; __VA_ARGS__; } break;        \
    default: return hipErrorInvalidValue;                       \
  }
// the looped kernels' array capacity for a model of n joints
#define MP_DISPATCH_CAP(n, ...)                                                       \
  if ((n) <= MP_MID_DOF) { constexpr int CAP = MP_MID_DOF; __VA_ARGS__; }             \
  else if ((n) <= MP_BIG_DOF) { constexpr int CAP = MP_BIG_DOF; __VA_ARGS__; }        \
  else return hipErrorInvalidValue;

}  // namespace

// streaming probes for the roofline: dst = a (one read per write) or dst = a + b + c (the 3 : 1 byte mix of the ID kernels)
typedef float mp_f4v __attribute__((ext_vector_type(4)));
template <int READS, bool NT>
__global__ __launch_bounds__(256) void k_stream(const mp_f4v* __restrict__ a, const mp_f4v* __restrict__ b, const mp_f4v* __restrict__ c,
                                                mp_f4v* __restrict__ d, long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  mp_f4v v = NT ? __builtin_nontemporal_load(a + i) : a[i];
  if (READS == 3) v = v + (NT ? __builtin_nontemporal_load(b + i) : b[i]) + (NT ? __builtin_nontemporal_load(c + i) : c[i]);
  if (NT) __builtin_nontemporal_store(v, d + i);
  else d[i] = v;
}
hipError_t mpk_stream(hipStream_t s, int reads, bool nontemporal, const void* a, const void* b, const void* c, void* d, long n4) {
  MP_FLAG(reads == 3, THREE, MP_FLAG(nontemporal, NT, return launch(k_stream<THREE ? 3 : 1, NT>, mp_grid(n4, kBlock), kBlock, 0, s,
      (const mp_f4v*)a, (const mp_f4v*)b, (const mp_f4v*)c, (mp_f4v*)d, n4)))
}

// the same with any byte mix: every lane reads R 16-byte chunks (one from each of R arrays laid back to back in `a`) and writes W
// (into W arrays back to back in `d`) - c3's kernel writes three bytes for every one it reads, the roll-out reads two for three
template <int R, int W, bool NT>
__global__ __launch_bounds__(256) void k_stream_mix(const mp_f4v* __restrict__ a, mp_f4v* __restrict__ d, long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  mp_f4v v = {1.f, 2.f, 3.f, 4.f};
#pragma unroll
  for (int r = 0; r < R; ++r) v = v + (NT ? __builtin_nontemporal_load(a + r * n4 + i) : a[r * n4 + i]);
#pragma unroll
  for (int w = 0; w < W; ++w) {
    if (NT) __builtin_nontemporal_store(v, d + w * n4 + i);
    else d[w * n4 + i] = v;
  }
}
hipError_t mpk_stream_mix(hipStream_t s, int reads, int writes, bool nontemporal, const void* a, void* d, long n4) {
  // (the mixes that exist: what is particular here is this list)
#define MP_MIX(R, W)              \
  if (reads == R && writes == W) { \
    MP_FLAG(nontemporal, NT, return launch(k_stream_mix<R, W, NT>, mp_grid(n4, kBlock), kBlock, 0, s, (const mp_f4v*)a, (mp_f4v*)d, n4)) \
  }
  MP_MIX(0, 1) MP_MIX(1, 1) MP_MIX(3, 1) MP_MIX(1, 3) MP_MIX(2, 3) MP_MIX(1, 2) MP_MIX(2, 1)
  MP_MIX(9, 1) MP_MIX(10, 1)   // the read-heavy mixes of k_fk_jac_vjp (q + gT + gJ in, gq out: 9.7 : 1 at n = 6, 9 : 1 at n = 8)
#undef MP_MIX
  return hipErrorInvalidValue;
}

// Shader-clock sampler for the measurement harness (MI355X_MICROARCH.md, "DVFS give-back" (6): the in-kernel clock is
// delta s_memtime / delta s_memrealtime x 100 MHz).  One wave per block; lane 0 stamps both counters, naps `naps` x s_sleep 127
// (64 x 127 cycles each) and stamps again, `samples` times - strictly bounded, nothing to wait for.  It is launched on a stream of its
// own BESIDE the kernels whose clock is asked for and costs them one wave slot per block; out[block][sample] = {memtime, realtime}.
__global__ __launch_bounds__(64) void k_clock_sampler(unsigned long long* __restrict__ out, unsigned samples, unsigned naps) {
  if (threadIdx.x != 0) return;
  unsigned long long* o = out + (size_t)blockIdx.x * samples * 2;
  for (unsigned i = 0; i < samples; ++i) {
    o[2 * i] = __builtin_amdgcn_s_memtime();
    o[2 * i + 1] = __builtin_amdgcn_s_memrealtime();
    for (unsigned k = 0; k < naps; ++k) __builtin_amdgcn_s_sleep(127);
  }
}
hipError_t mpk_clock_sampler(hipStream_t s, unsigned long long* out, unsigned blocks, unsigned samples, unsigned naps) {
  return launch(k_clock_sampler, mp_grid(blocks, 1), kWave, 0, s, out, samples, naps);
}

hipError_t mpk_selftest(hipStream_t s, int* d_out) { return launch(k_selftest, mp_grid(1, 1), kWave, 0, s, d_out); }

// one row per lane, model through a device pointer (k_id_dm)
hipError_t mpk_id_dm(hipStream_t s, const MpModel<float>* d_model, int n, const MpCall<float>& C, bool ftip, const float* q,
                     const float* qd, const float* qdd, float* tau, long rows, const MpLead& L, bool all_revolute) {
  if (rows <= 0) return hipSuccess;
  const MpGrid grid = mp_grid(rows + (long)L.blocks * kBlock, kBlock);  // the lead's blocks, then the rows' (ceil(rows / kBlock) + L.blocks)
  MP_DISPATCH_N(n, MP_FLAG(all_revolute, REV, MP_FLAG(ftip, F,
      return launch(k_id_dm<float, N, F, REV>, grid, kBlock, 0, s, d_model, C, q, qd, qdd, tau, rows, L))))
}

hipError_t mpk_id_hard(hipStream_t s, const MpModel<float>* d_model, int n, const MpCall<float>& C, bool ftip, const float* q,
                       const float* qd, const float* qdd, float* tau, unsigned rows, unsigned blocks) {
  if (blocks == 0 || !C.hard_rows || !C.cold_model) return hipSuccess;
  MP_DISPATCH_N(n, MP_FLAG(ftip, F, return launch(k_id_hard<N, F>, mp_grid(blocks, 1), kWave, 0, s, d_model, C, q, qd, qdd, tau, rows)))
}

hipError_t mpk_id_hard_batch(hipStream_t s, const MpModel<float>* d_model, int n, bool ftip, const MpHardBatch& B, int entries, unsigned blocks) {
  if (blocks == 0 || entries <= 0) return hipSuccess;
  MP_DISPATCH_N(n, MP_FLAG(ftip, F, return launch(k_id_hard_batch<N, F>, mp_grid(blocks, 1, entries), kWave, 0, s, d_model, B)))
}

template <>
hipError_t mpk_id<double>(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, bool ftip, const double* q,
                          const double* qd, const double* qdd, double* tau, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, MP_FLAG(ftip, F, return launch(k_id<double, N, F>, mp_grid(rows, kBlock), kBlock, 0, s, M, C, q, qd, qdd, tau, rows)))
}

hipError_t mpk_batch_traj(hipStream_t s, const MpModel<float>& M, const float* start, const float* end, long B,
                          long Nt, double Tf, int method, float* pos, float* vel, float* acc) {
  const long rows = B * Nt;
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, return launch(k_batch_traj<N>, mp_grid(rows, kBlock), kBlock, 0, s, M, start, end, B, Nt, Tf, method, pos, vel, acc))
}

hipError_t mpk_time_table(hipStream_t s, double* tab, long Nt, double Tf, int method) {
  if (Nt <= 0) return hipSuccess;
  return launch(k_time_table, mp_grid(Nt, kBlock), kBlock, 0, s, tab, Nt, Tf, method);
}

// blocks per trajectory of the table-driven fused kernels (block = 256 lanes, ceil(Nt / 2) lanes per trajectory)
unsigned mpk_traj_blocks_per_trajectory(long Nt) { return mp_grid((Nt + 1) / 2, kBlock).x; }

hipError_t mpk_traj_id_tab(hipStream_t s, const MpModel<float>& M, const MpCall<float>& C, bool ftip, const float* start,
                           const float* end, long B, long Nt, const double* tab, float* tau) {
  if (B <= 0 || Nt <= 0) return hipSuccess;
  const unsigned bpt = mpk_traj_blocks_per_trajectory(Nt);
  MP_DISPATCH_N(M.n, MP_FLAG(ftip, F,
      return launch(k_traj_id_pk_tab<N, F>, mp_grid2(B, bpt), kBlock, 0, s, M, C, start, end, Nt, bpt, tab, tau)))
}

hipError_t mpk_traj_id_hard(hipStream_t s, const MpModel<float>* d_model, int n, const MpCall<float>& C, bool ftip, const float* start,
                            const float* end, unsigned Nt, const double* tab, float* tau, unsigned rows, unsigned blocks) {
  if (blocks == 0 || !C.hard_rows || !C.cold_model) return hipSuccess;
  MP_DISPATCH_N(n, MP_FLAG(ftip, F,
      return launch(k_traj_id_hard<N, F>, mp_grid(blocks, 1), kWave, 0, s, d_model, C, start, end, Nt, tab, tau, rows)))
}

template <typename T>
hipError_t mpk_fk_jac_id(hipStream_t s, const MpModel<T>& M, const MpCall<T>& C, bool ftip, const T* q, const T* qd,
                         const T* qdd, T* Tout, T* Jout, T* tau, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, MP_FLAG(ftip, F,
      return launch(k_fk_jac_id<T, N, F>, mp_grid(rows, kFkBlock), kFkBlock, 0, s, M, C, q, qd, qdd, Tout, Jout, tau, rows)))
}
template hipError_t mpk_fk_jac_id<float>(hipStream_t, const MpModel<float>&, const MpCall<float>&, bool, const float*,
                                         const float*, const float*, float*, float*, float*, long);
template hipError_t mpk_fk_jac_id<double>(hipStream_t, const MpModel<double>&, const MpCall<double>&, bool,
                                          const double*, const double*, const double*, double*, double*, double*, long);

template <typename T>
hipError_t mpk_mass_matrix(hipStream_t s, const MpModel<T>& M, const T* q, T* Mout, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, return launch(k_mass_matrix<T, N>, mp_grid(rows, kFkBlock), kFkBlock, 0, s, M, q, Mout, rows))
}
template hipError_t mpk_mass_matrix<float>(hipStream_t, const MpModel<float>&, const float*, float*, long);
template hipError_t mpk_mass_matrix<double>(hipStream_t, const MpModel<double>&, const double*, double*, long);

template <typename T>
hipError_t mpk_forward_dynamics(hipStream_t s, const MpModel<T>& M, const MpCall<T>& C, bool ftip, const T* q, const T* qd,
                                const T* tau, T* qdd, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, MP_FLAG(ftip, F,
      return launch(k_forward_dynamics<T, N, F>, mp_grid(rows, kBlock), kBlock, 0, s, M, C, q, qd, tau, qdd, rows)))
}
template hipError_t mpk_forward_dynamics<float>(hipStream_t, const MpModel<float>&, const MpCall<float>&, bool, const float*,
                                                const float*, const float*, float*, long);
template hipError_t mpk_forward_dynamics<double>(hipStream_t, const MpModel<double>&, const MpCall<double>&, bool,
                                                 const double*, const double*, const double*, double*, long);

hipError_t mpk_id_deriv(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, bool ftip, const double* q, const double* qd,
                        const double* qdd, double* tau, double* dq, double* dqd, double* Mout, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, MP_FLAG(ftip, F,
      return launch(k_id_deriv<N, F>, mp_grid(rows, kDerivBlock), kDerivBlock, 0, s, M, C, q, qd, qdd, tau, dq, dqd, Mout, rows)))
}
hipError_t mpk_fd_deriv(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, bool ftip, const double* q, const double* qd,
                        const double* tau, double* qdd, double* dq, double* dqd, double* Minv, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, MP_FLAG(ftip, F,
      return launch(k_fd_deriv<N, F>, mp_grid(rows, kDerivBlock), kDerivBlock, 0, s, M, C, q, qd, tau, qdd, dq, dqd, Minv, rows)))
}

hipError_t mpk_id_vjp(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, bool ftip, const double* q, const double* qd,
                      const double* qdd, const double* gtau, double* gq, double* gqd, double* gqdd, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, MP_FLAG(ftip, F,
      return launch(k_id_vjp<N, F>, mp_grid(rows, kDerivBlock), kDerivBlock, 0, s, M, C, q, qd, qdd, gtau, gq, gqd, gqdd, rows)))
}
hipError_t mpk_fd_vjp(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, bool ftip, const double* q, const double* qd,
                      const double* tau, const double* gqdd, double* qdd, double* gq, double* gqd, double* gtau, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, MP_FLAG(ftip, F,
      return launch(k_fd_vjp<N, F>, mp_grid(rows, kDerivBlock), kDerivBlock, 0, s, M, C, q, qd, tau, gqdd, qdd, gq, gqd, gtau, rows)))
}

hipError_t mpk_fk_jac_vjp(hipStream_t s, const MpModel<double>& M, int frame, const double* q, const double* gT, const double* gJ,
                         double* Tout, double* Jout, double* gq, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, MP_FLAG(frame != 0, BODY,
      return launch(k_fk_jac_vjp<N, BODY ? 1 : 0>, mp_grid(rows, kFkBlock), kFkBlock, 0, s, M, q, gT, gJ, Tout, Jout, gq, rows)))
}

// dynamic LDS: the park of S world centres for 64 lanes; beyond the default limit the function's own limit is raised first
hipError_t mpk_collision(hipStream_t s, const MpModel<double>& M, const MpColDevice& D, const double* q, long rows, double eps_world,
                         double eps_self, const MpColOut& O) {
  if (rows <= 0) return hipSuccess;
  if (D.S < 1 || D.S > MP_COL_MAX_SPHERES) return hipErrorInvalidValue;
  const unsigned park = (unsigned)D.S * 3u * kWave * (unsigned)sizeof(double);
  const bool want_grad = O.grad_dist_world != nullptr || O.grad_dist_self != nullptr || O.grad != nullptr;
  MP_DISPATCH_N(M.n, MP_FLAG(want_grad, WG, MP_FLAG(D.cloud, CLOUD, {
    if (park + MP_WAVE_LDS_BYTES > 64u * 1024u) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_collision<N, WG, CLOUD>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)park);
      if (e != hipSuccess) return e;
    }
    return launch(k_collision<N, WG, CLOUD>, mp_grid(rows, kWave), kWave, park, s, M, D.sph, D.pairs, D.world, q, rows, eps_world,
                  eps_self, O);
  })))
}

// The launch plan of a one-wave work-queue kernel on the sphere model: its dynamic LDS (beyond the default limit the kernel's own
// limit is raised first) and the blocks of it the device keeps resident.  The only runtime queries of these kernels; the launchers
// below are handed what the caller made of the plan.
template <typename K>
static hipError_t queue_plan(K kernel, int n, int S, int compute_units, MpQueuePlan* plan) {
  const unsigned lds = mp_col_queue_lds_bytes(n, S);
  const void* fn = reinterpret_cast<const void*>(kernel);
  if (lds > 64u * 1024u) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  int per_cu = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kWave, lds);
  if (e != hipSuccess) return e;
  *plan = {lds, (long)(per_cu > 0 ? per_cu : 1) * (compute_units > 0 ? compute_units : 256)};
  return hipSuccess;
}

hipError_t mpk_queue_plan(MpQueueKernel kernel, int n, int S, bool cloud, int compute_units, MpQueuePlan* plan) {
  if (S < 1 || S > MP_COL_MAX_SPHERES) return hipErrorInvalidValue;
  MP_DISPATCH_N(n, MP_FLAG(cloud, CLOUD, {
    switch (kernel) {
      case MP_QUEUE_EDGES: return queue_plan(&k_collision_edges<N, CLOUD>, N, S, compute_units, plan);
      case MP_QUEUE_RRT: return queue_plan(&k_rrt_connect<N, CLOUD>, N, S, compute_units, plan);
      case MP_QUEUE_SHORTCUT: return queue_plan(&k_path_shortcut<N, CLOUD>, N, S, compute_units, plan);
      case MP_QUEUE_GOAL: return queue_plan(&k_goal_ik<N, CLOUD>, N, S, compute_units, plan);
      case MP_QUEUE_BLEND: return queue_plan(&k_path_blend<N, CLOUD>, N, S, compute_units, plan);
    }
  }))
  return hipErrorInvalidValue;
}

// The five queue launches: `blocks` is the grid the caller has settled on (the plan's resident blocks, the count, its cap and the
// workspace), `lds` the plan's dynamic LDS.  They zero the queue counter on the stream and launch; no runtime query.
static hipError_t queue_reset(hipStream_t s, const MpColDevice& D, long blocks) {
  if (D.S < 1 || D.S > MP_COL_MAX_SPHERES || blocks < 1) return hipErrorInvalidValue;
  return hipMemsetAsync(D.counter, 0, sizeof(unsigned long long), s);
}

hipError_t mpk_collision_edges(hipStream_t s, const MpModel<double>& M, const MpColDevice& D, const double* q_from, const double* q_to,
                               long edges, const MpColEdgeParams& P, const MpColEdgeOut& O, long blocks, unsigned lds) {
  if (edges <= 0) return hipSuccess;
  const hipError_t e = queue_reset(s, D, blocks);
  if (e != hipSuccess) return e;
  MP_DISPATCH_N(M.n, MP_FLAG(D.cloud, CLOUD,
      return launch(k_collision_edges<N, CLOUD>, mp_grid(blocks, 1), kWave, lds, s, M, D.sph, D.pairs, D.world, q_from, q_to, edges, P,
                    O, D.counter)))
}

hipError_t mpk_rrt_connect(hipStream_t s, const MpModel<double>& M, const MpColDevice& D, const double* q_start, const double* q_goal,
                           long problems, const MpRrtParams& P, const MpRrtOut& O, double* workspace, long blocks, unsigned lds) {
  if (problems <= 0) return hipSuccess;
  const hipError_t e = queue_reset(s, D, blocks);
  if (e != hipSuccess) return e;
  MP_DISPATCH_N(M.n, MP_FLAG(D.cloud, CLOUD,
      return launch(k_rrt_connect<N, CLOUD>, mp_grid(blocks, 1), kWave, lds, s, M, D.sph, D.pairs, D.world, q_start, q_goal, problems, P,
                    O, workspace, D.counter)))
}

hipError_t mpk_path_shortcut(hipStream_t s, const MpModel<double>& M, const MpColDevice& D, const double* waypoints_in, const int* count_in,
                             long problems, const MpShortcutParams& P, const MpShortcutOut& O, double* workspace, long blocks,
                             unsigned lds) {
  if (problems <= 0) return hipSuccess;
  const hipError_t e = queue_reset(s, D, blocks);
  if (e != hipSuccess) return e;
  MP_DISPATCH_N(M.n, MP_FLAG(D.cloud, CLOUD,
      return launch(k_path_shortcut<N, CLOUD>, mp_grid(blocks, 1), kWave, lds, s, M, D.sph, D.pairs, D.world, waypoints_in, count_in,
                    problems, P, O, workspace, D.counter)))
}

hipError_t mpk_goal_ik(hipStream_t s, const MpModel<double>& M, const MpColDevice& D, const double* T_goal, const double* q_seed,
                       long problems, const MpGoalParams& P, const MpGoalOut& O, long blocks, unsigned lds) {
  if (problems <= 0) return hipSuccess;
  const hipError_t e = queue_reset(s, D, blocks);
  if (e != hipSuccess) return e;
  MP_DISPATCH_N(M.n, MP_FLAG(D.cloud, CLOUD,
      return launch(k_goal_ik<N, CLOUD>, mp_grid(blocks, 1), kWave, lds, s, M, D.sph, D.pairs, D.world, T_goal, q_seed, problems, P,
                    O, D.counter)))
}

hipError_t mpk_path_blend(hipStream_t s, const MpModel<double>& M, const MpColDevice& D, const double* waypoints_in, const int* count_in,
                          long problems, const MpBlendParams& P, const MpBlendOut& O, long blocks, unsigned lds) {
  if (problems <= 0) return hipSuccess;
  const hipError_t e = queue_reset(s, D, blocks);
  if (e != hipSuccess) return e;
  MP_DISPATCH_N(M.n, MP_FLAG(D.cloud, CLOUD,
      return launch(k_path_blend<N, CLOUD>, mp_grid(blocks, 1), kWave, lds, s, M, D.sph, D.pairs, D.world, waypoints_in, count_in,
                    problems, P, O, D.counter)))
}

hipError_t mpk_path_blend_sample(hipStream_t s, int n, long problems, const MpBlendParams& P, const int* status, const int* count,
                                 const double* points, const double* cut, const double* knot, const double* length, double* q, double* dq,
                                 double* ddq) {
  if (problems <= 0) return hipSuccess;
  MP_DISPATCH_N(n, return launch(k_path_blend_sample<N>, mp_grid(problems * P.grid, kWave), kWave, 0, s, problems, P.grid, P.w_in, status,
                                 count, points, cut, knot, length, q, dq, ddq))
}

// Cartesian paths: the joint count and the task's rows bound to constants - POSITION (3 rows) from 3 joints, FULL (6 rows) from 6.
// The body is written once, as a generic lambda over the two constants.
template <int V> struct MpConst { static constexpr int value = V; };
template <typename F>
static hipError_t cart_dispatch(int n, int task, F f) {
  const bool pos = task == MP_CP_POSITION;
  switch (n) {
    case 3: return pos ? f(MpConst<3>{}, MpConst<3>{}) : hipErrorInvalidValue;
    case 4: return pos ? f(MpConst<4>{}, MpConst<3>{}) : hipErrorInvalidValue;
    case 5: return pos ? f(MpConst<5>{}, MpConst<3>{}) : hipErrorInvalidValue;
    case 6: return pos ? f(MpConst<6>{}, MpConst<3>{}) : f(MpConst<6>{}, MpConst<6>{});
    case 7: return pos ? f(MpConst<7>{}, MpConst<3>{}) : f(MpConst<7>{}, MpConst<6>{});
    case 8: return pos ? f(MpConst<8>{}, MpConst<3>{}) : f(MpConst<8>{}, MpConst<6>{});
    default: return hipErrorInvalidValue;
  }
}

hipError_t mpk_cart_plan(int n, int task, int S, bool cloud, int compute_units, MpQueuePlan* plan) {
  if (S < 1 || S > MP_COL_MAX_SPHERES) return hipErrorInvalidValue;
  return cart_dispatch(n, task, [&](auto cn, auto cm) {
    MP_FLAG(cloud, CLOUD, return queue_plan(&k_cart_span<decltype(cn)::value, decltype(cm)::value, CLOUD>, decltype(cn)::value, S,
                                            compute_units, plan))
  });
}

// Tracking, the spans on the work queue (`blocks` and `lds` from mpk_cart_plan, the queue head zeroed on the stream first), the
// reduction: three launches on one stream, no runtime query.
hipError_t mpk_cartesian_path(hipStream_t s, const MpModel<double>& M, const MpColDevice& D, const MpCartParams& P, const double* q_start,
                              const double* T_goal, long problems, const MpCartWork& W, double* q, double* dq, double* ddq,
                              const MpCartOut& O, long blocks, unsigned lds) {
  if (problems <= 0) return hipSuccess;
  hipError_t e = queue_reset(s, D, blocks);
  if (e != hipSuccess) return e;
  e = cart_dispatch(M.n, P.task, [&](auto cn, auto cm) {
    constexpr int N = decltype(cn)::value, MR = decltype(cm)::value;
    const hipError_t t = launch(k_cart_track<N, MR>, mp_grid(problems, kWave), kWave, 0, s, M, P, q_start, T_goal, problems, W, q, dq, ddq);
    if (t != hipSuccess) return t;
    MP_FLAG(D.cloud, CLOUD,
        return launch(k_cart_span<N, MR, CLOUD>, mp_grid(blocks, 1), kWave, lds, s, M, D.sph, D.pairs, D.world, P, T_goal, problems, W, q,
                      dq, ddq, D.counter))
  });
  if (e != hipSuccess) return e;
  return launch(k_cart_reduce, mp_grid(problems, kWave), kWave, 0, s, problems, P.grid, W, O);
}

// `ftip`: the call's wrench is not zero.  The grid: the tiles of 64 rows, clamped to what a grid holds and to the caller's cap - the
// kernel strides over the tiles.  The torque variant: none without O.tau, else with or without the wrench (three instances, not four).
hipError_t mpk_traj_sample(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, bool ftip, bool curve, const MpSampleIn& I,
                           const MpSampleOut& O, long max_blocks) {
  if (I.B <= 0) return hipSuccess;
  const long tiles = (I.B * I.M + kWave - 1) / kWave;
  long blocks = tiles < kMaxGrid ? tiles : kMaxGrid;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
  MP_DISPATCH_N(M.n, MP_FLAG(curve, CURVE, MP_FLAG(O.tau != nullptr, WITH_TAU, MP_FLAG(ftip, F, {
    constexpr int TAU = !WITH_TAU ? MP_TS_NO_TAU : F ? MP_TS_TAU_FTIP : MP_TS_TAU;
    return launch(k_traj_sample<N, CURVE ? MP_TS_CURVE : MP_TS_GRID, TAU>, mp_grid(blocks, 1), kWave, 0, s, M, C, I, O, tiles);
  }))))
}

hipError_t mpk_opspace(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, int frame, int task, double lam2, const double* q,
                       const double* qd, double* Tout, double* Jout, double* Jdqd, double* Lam, double* Jbar, double* mu, double* p,
                       long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, return launch(k_opspace<N>, mp_grid(rows, kDerivBlock), kDerivBlock, 0, s, M, C, frame, task, lam2, q, qd, Tout, Jout,
                                   Jdqd, Lam, Jbar, mu, p, rows))
}

hipError_t mpk_opspace_torque(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, int frame, int task, double lam2,
                              const double* q, const double* qd, const double* acc, const double* tau0, double* tau, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, return launch(k_opspace_torque<N>, mp_grid(rows, kDerivBlock), kDerivBlock, 0, s, M, C, frame, task, lam2, q, qd, acc,
                                   tau0, tau, rows))
}

hipError_t mpk_fd_traj_vjp(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, const double* theta0, const double* dtheta0,
                           const double* taumat, const double* Ftipmat, long B, long Nt, double h, int intRes, const double* gp,
                           const double* gv, const double* ga, double* work, double* gth0, double* gdth0, double* gtau) {
  if (B <= 0 || Nt <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, MP_FLAG(Ftipmat != nullptr, F,
      return launch(k_fd_traj_vjp<N, F>, mp_grid(B, kDerivBlock), kDerivBlock, 0, s, M, C, theta0, dtheta0, taumat, Ftipmat, B, Nt, h, intRes,
                    gp, gv, ga, work, gth0, gdth0, gtau)))
}

hipError_t mpk_ilqr_backward(hipStream_t s, const MpModel<double>& M, const MpIlqrWeights& Wt, const double* pos, const double* vel,
                             const double* tau, const double* dq, const double* dqd, const double* Minv, const double* xref,
                             const double* reg, long B, long Nt, double h, bool k_batch_major, double* work, double* K, double* k,
                             double* dV, int* status) {
  if (B <= 0 || Nt <= 0) return hipSuccess;
  if (!work) {   // no workspace: the cooperative form, kWave / MP_ILQR_LANES trajectories a block
    MP_DISPATCH_N(M.n, return launch(k_ilqr_backward_coop<N>, mp_grid(B, kWave / MP_ILQR_LANES), kWave, 0, s, M, Wt, pos, vel, tau, dq, dqd,
                                     Minv, xref, reg, B, Nt, h, k_batch_major, K, k, dV, status))
  }
  MP_DISPATCH_N(M.n, return launch(k_ilqr_backward<N>, mp_grid(B, kDerivBlock), kDerivBlock, 0, s, M, Wt, pos, vel, tau, dq, dqd, Minv, xref,
                                   reg, B, Nt, h, k_batch_major, work, K, k, dV, status))
}
hipError_t mpk_ilqr_rollout(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, const MpIlqrWeights& Wt, const double* th0,
                            const double* dth0, const double* tau, const double* pos, const double* vel, const double* K, const double* k,
                            const double* alpha, const double* xref, long A, long B, long Nt, double h, bool k_batch_major, double* cost,
                            double* opos, double* ovel, double* otau) {
  if (A <= 0 || B <= 0 || Nt <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, return launch(k_ilqr_rollout<N>, mp_grid(A * B, kDerivBlock), kDerivBlock, 0, s, M, C, Wt, th0, dth0, tau, pos, vel, K, k,
                                   alpha, xref, A, B, Nt, h, k_batch_major, cost, opos, ovel, otau))
}

hipError_t mpk_path_coeffs(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, bool ftip, const MpToppraVmax& V,
                           const double* q, const double* dq, const double* ddq, double* a, double* b, double* c, double* xbar, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, MP_FLAG(ftip, F,
      return launch(k_path_coeffs<N, F>, mp_grid(rows, kDerivBlock), kDerivBlock, 0, s, M, C, V, q, dq, ddq, a, b, c, xbar, rows)))
}
hipError_t mpk_toppra_sweep(hipStream_t s, int n, const MpToppraLimits& lim, bool acc, const double* a, const double* b, const double* c,
                            const double* xbar, const double* dq, const double* ddq, const double* sd_start, const double* sd_end, long B,
                            long Nt, double* K, double* x, double* u, double* t, double* dur, int* status, double* oqd, double* oqdd,
                            double* otau) {
  if (B <= 0) return hipSuccess;
  if (Nt < 3) return hipErrorInvalidValue;
  MP_DISPATCH_N(n, MP_FLAG(acc, ACC,
      return launch(k_toppra_sweep<N, ACC>, mp_grid(B, kDerivBlock), kDerivBlock, 0, s, lim, a, b, c, xbar, dq, ddq, sd_start, sd_end, B, Nt,
                    K, x, u, t, dur, status, oqd, oqdd, otau)))
}
hipError_t mpk_path_rows(hipStream_t s, int n, const double* a, const double* b, const double* c, const double* dq, const double* ddq,
                         const double* x, const double* u, double* oqd, double* oqdd, double* otau, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_N(n, return launch(k_path_rows<N>, mp_grid(rows, kDerivBlock), kDerivBlock, 0, s, a, b, c, dq, ddq, x, u, oqd, oqdd, otau, rows))
}

hipError_t mpk_id_regressor(hipStream_t s, const MpModel<double>& M, const double* Dmap, const MpCall<double>& C, bool ftip,
                            const double* q, const double* qd, const double* qdd, double* Y, double* tau_ext, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, MP_FLAG(ftip, F,
      return launch(k_id_regressor<N, F>, mp_grid(rows, kDerivBlock), kDerivBlock, 0, s, M, Dmap, C, q, qd, qdd, Y, tau_ext, rows)))
}
hipError_t mpk_id_regressor_normal(hipStream_t s, const MpModel<double>& M, const double* Dmap, const MpCall<double>& C, bool ftip,
                                   const double* q, const double* qd, const double* qdd, const double* rhs, long rows, double* work,
                                   double* A, double* b, double* rr) {
  if (rows <= 0) return hipSuccess;
  const long groups = mp_reg_normal_groups(rows);
  const bool with_a = A != nullptr;
  MP_DISPATCH_N(M.n, MP_FLAG(ftip, F, MP_FLAG(with_a, WITH_A, {
    const hipError_t e = launch(k_id_regressor_normal<N, F, WITH_A>, mp_grid(groups, 1), kWave, 0, s, M, Dmap, C, q, qd, qdd, rhs, rows, work);
    if (e != hipSuccess) return e;
    constexpr int W = MP_REG_P * N, outs = (WITH_A ? W * W : 0) + W + 1;
    return launch(k_id_regressor_normal_reduce<N>, mp_grid(outs, kBlock), kBlock, 0, s, work, groups, with_a, A, b, rr);
  })))
}

template <typename T>
hipError_t mpk_fd_traj(hipStream_t s, const MpModel<T>& M, const MpCall<T>& C, const T* theta0, const T* dtheta0,
                       const T* taumat, const T* Ftipmat, long B, long Nt, T h, int intRes, float* pos, float* vel, float* acc) {
  if (B <= 0 || Nt <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, MP_FLAG(Ftipmat != nullptr, F,
      return launch(k_fd_traj<T, N, F>, mp_grid(B, kFdBlock), kFdBlock, 0, s, M, C, theta0, dtheta0, taumat, Ftipmat, B, Nt, h, intRes, pos, vel,
                    acc)))
}
template hipError_t mpk_fd_traj<float>(hipStream_t, const MpModel<float>&, const MpCall<float>&, const float*, const float*,
                                       const float*, const float*, long, long, float, int, float*, float*, float*);
template hipError_t mpk_fd_traj<double>(hipStream_t, const MpModel<double>&, const MpCall<double>&, const double*,
                                        const double*, const double*, const double*, long, long, double, int, float*, float*,
                                        float*);

template <typename T>
hipError_t mpk_fd_traj_tm(hipStream_t s, const MpModel<T>& M, const MpCall<T>& C, const T* theta0, const T* dtheta0,
                          const T* taumat, const T* Ftipmat, long B, long Nt, T h, int intRes, float* pos, float* vel, float* acc) {
  if (B <= 0 || Nt <= 0) return hipSuccess;
  MP_DISPATCH_N(M.n, MP_FLAG(Ftipmat != nullptr, F,
      return launch(k_fd_traj_tm<T, N, F>, mp_grid(B, kFdBlock), kFdBlock, 0, s, M, C, theta0, dtheta0, taumat, Ftipmat, B, Nt, h, intRes, pos,
                    vel, acc)))
}
template hipError_t mpk_fd_traj_tm<float>(hipStream_t, const MpModel<float>&, const MpCall<float>&, const float*, const float*,
                                          const float*, const float*, long, long, float, int, float*, float*, float*);
template hipError_t mpk_fd_traj_tm<double>(hipStream_t, const MpModel<double>&, const MpCall<double>&, const double*,
                                           const double*, const double*, const double*, long, long, double, int, float*, float*,
                                           float*);

// ---- launchers of the run-time-n kernels (d_model: MpBigModel<T> resident in device memory)
template <typename T>
hipError_t mpk_dyn_fk_jac_id(hipStream_t s, int n, const MpBigModel<T>* d_model, const MpCall<T>& C, bool ftip, const T* q, const T* qd,
                             const T* qdd, T* Tout, T* Jout, T* tau, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_CAP(n, MP_FLAG(ftip, F,
      return launch(k_dyn_fk_jac_id<CAP, T, F>, mp_grid(rows, kBlock), kBlock, 0, s, d_model, C, q, qd, qdd, Tout, Jout, tau, rows)))
}
template hipError_t mpk_dyn_fk_jac_id<float>(hipStream_t, int, const MpBigModel<float>*, const MpCall<float>&, bool, const float*,
                                             const float*, const float*, float*, float*, float*, long);
template hipError_t mpk_dyn_fk_jac_id<double>(hipStream_t, int, const MpBigModel<double>*, const MpCall<double>&, bool, const double*,
                                              const double*, const double*, double*, double*, double*, long);
template <typename T>
hipError_t mpk_dyn_mass_matrix(hipStream_t s, int n, const MpBigModel<T>* d_model, const T* q, T* Mout, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_CAP(n, return launch(k_dyn_mass_matrix<CAP, T>, mp_grid(rows, kBlock), kBlock, 0, s, d_model, q, Mout, rows))
}
template hipError_t mpk_dyn_mass_matrix<float>(hipStream_t, int, const MpBigModel<float>*, const float*, float*, long);
template hipError_t mpk_dyn_mass_matrix<double>(hipStream_t, int, const MpBigModel<double>*, const double*, double*, long);
template <typename T>
hipError_t mpk_dyn_forward_dynamics(hipStream_t s, int n, const MpBigModel<T>* d_model, const MpCall<T>& C, bool ftip, const T* q,
                                    const T* qd, const T* tau, T* qdd, long rows) {
  if (rows <= 0) return hipSuccess;
  MP_DISPATCH_CAP(n, MP_FLAG(ftip, F,
      return launch(k_dyn_forward_dynamics<CAP, T, F>, mp_grid(rows, kBlock), kBlock, 0, s, d_model, C, q, qd, tau, qdd, rows)))
}
template hipError_t mpk_dyn_forward_dynamics<float>(hipStream_t, int, const MpBigModel<float>*, const MpCall<float>&, bool, const float*,
                                                    const float*, const float*, float*, long);
template hipError_t mpk_dyn_forward_dynamics<double>(hipStream_t, int, const MpBigModel<double>*, const MpCall<double>&, bool,
                                                     const double*, const double*, const double*, double*, long);
template <typename T>
hipError_t mpk_dyn_fd_traj(hipStream_t s, int n, const MpBigModel<T>* d_model, const MpCall<T>& C, const T* theta0, const T* dtheta0,
                           const T* taumat, const T* Ftipmat, long B, long Nt, T h, int intRes, float* pos, float* vel, float* acc,
                           bool time_major) {
  if (B <= 0 || Nt <= 0) return hipSuccess;
  MP_DISPATCH_CAP(n, MP_FLAG(Ftipmat != nullptr, F,
      return launch(k_dyn_fd_traj<CAP, T, F>, mp_grid(B, kWave), kWave, 0, s, d_model, C, theta0, dtheta0, taumat, Ftipmat, B, Nt, h, intRes, pos,
                    vel, acc, time_major)))
}
template hipError_t mpk_dyn_fd_traj<float>(hipStream_t, int, const MpBigModel<float>*, const MpCall<float>&, const float*, const float*,
                                           const float*, const float*, long, long, float, int, float*, float*, float*, bool);
template hipError_t mpk_dyn_fd_traj<double>(hipStream_t, int, const MpBigModel<double>*, const MpCall<double>&, const double*,
                                            const double*, const double*, const double*, long, long, double, int, float*, float*, float*,
                                            bool);
hipError_t mpk_dyn_traj(hipStream_t s, int n, const MpBigModel<float>* d_model, const MpCall<float>& C, bool ftip, const float* start,
                        const float* end, long B, long Nt, double Tf, int method, float* pos, float* vel, float* acc, float* tau) {
  if (B <= 0 || Nt <= 0) return hipSuccess;
  MP_DISPATCH_CAP(n, MP_FLAG(ftip, F,
      return launch(k_dyn_traj<CAP, F>, mp_grid(B * Nt, kBlock), kBlock, 0, s, d_model, C, start, end, B, Nt, Tf, method, pos, vel, acc, tau)))
}

hipError_t mpk_transpose_rows(hipStream_t s, const void* src, void* dst, long outer, long inner, int row_dwords) {
  if (outer <= 0 || inner <= 0 || row_dwords <= 0) return hipSuccess;
  const int TI = mp_tr_ti(row_dwords);
  const size_t lds = (size_t)MP_TR_TO * (TI * row_dwords + 1) * sizeof(unsigned);
  return launch(k_transpose_rows, mp_grid2(mp_blocks(inner, TI), mp_blocks(outer, MP_TR_TO)), kBlock, lds, s, (const unsigned*)src,
                (unsigned*)dst, outer, inner, row_dwords);
}

// K closed-loop regulation runs (mp_pd_regulation_run), one lane each: rows of theta0 / des (K, n), gains per run, errors (K, steps)
template <int N>
__global__ __launch_bounds__(64) void k_pd_regulation(const MpModel<double> M, const MpCall<double> C, const double* __restrict__ theta0,
                                                      const double* __restrict__ des, const double* __restrict__ Kp,
                                                      const double* __restrict__ Kd, long K, double dt, int steps,
                                                      double* __restrict__ err, int* __restrict__ count) {
  const long k = (long)blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  double a[N], d[N];
  RunIO<double, N>::load(theta0, k, a);
  RunIO<double, N>::load(des, k, d);
  count[k] = mp_pd_regulation_run<double, N>(M, C.a0, a, d, Kp[k], Kd[k], dt, steps, err + k * steps);
}
template <int CAP>
__global__ __launch_bounds__(64) void k_dyn_pd_regulation(const MpBigModel<double>* __restrict__ Mdev, const MpCall<double> C,
                                                          const double* __restrict__ theta0, const double* __restrict__ des,
                                                          const double* __restrict__ Kp, const double* __restrict__ Kd, long K, double dt,
                                                          int steps, double* __restrict__ err, int* __restrict__ count) {
  const long k = (long)blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  MpBigConst<double>& M = *(MpBigConst<double>*)Mdev;
  count[k] = mp_dyn_pd_regulation_run<CAP, double>(M, C.a0, theta0 + k * M.n, des + k * M.n, Kp[k], Kd[k], dt, steps, err + k * steps);
}

// inverse kinematics with a run-time joint count: the work queue of k_ik, the looped kinematics of mp_dyn.h.  CAP: the capacity of
// the per-problem arrays (16 for the reference's 9- and 10-joint Jaco arms, 32 beyond: MP_DISPATCH_CAP, as the dynamics kernels)
template <int CAP>
__global__ __launch_bounds__(kBlock) void k_dyn_ik(const MpBigModel<double>* __restrict__ Mdev, const MpIkParamsT<CAP> P,
                                                   const double* __restrict__ Tdes, const double* __restrict__ theta0, long B,
                                                   double* __restrict__ theta, int* __restrict__ success, int* __restrict__ iterations,
                                                   int* __restrict__ restarts, unsigned long long* __restrict__ next) {
  MpBigConst<double>& M = *(MpBigConst<double>*)Mdev;
  const int n = M.n;
  MpIkState<CAP> S;
  bool have = false;
  long row = 0;
  for (;;) {  // exit: the counter only grows, so every lane sees row >= B eventually
    if (!have) {
      row = (long)atomicAdd(next, 1ull);
      if (row >= B) break;
      for (int j = 0; j < CAP; ++j) S.theta[j] = j < n ? theta0[row * n + j] : 0.0;
      mp_ik_begin(S, P);
      have = true;
    }
    if (const int done = mp_ik_iterate<CAP, MpIkLooped<CAP>>(M, P, S, Tdes + row * 16, theta0 + row * n)) {
      for (int j = 0; j < n; ++j) theta[row * n + j] = S.theta[j];
      success[row] = done == 2 ? 1 : 0;
      iterations[row] = S.k + 1;
      restarts[row] = S.restarts;
      have = false;
    }
  }
}
hipError_t mpk_cartesian_traj(hipStream_t s, const double* Xstart, const double* Xend, long B, long Nt, double Tf, int method,
                              float* pos, float* vel, float* acc, float* ori) {
  if (B <= 0 || Nt <= 0) return hipSuccess;
  const unsigned bpt = mp_grid(Nt, kBlock).x;
  return launch(k_cartesian_traj, mp_grid2(B, bpt), kBlock, 0, s, Xstart, Xend, Nt, bpt, Tf, method, pos, vel, acc, ori);
}

// the grid of the IK work queues: resident lanes only (two 256-thread blocks per CU; fp64 IK needs > 128 VGPRs): the queue feeds them
static MpGrid ik_grid(long B, int compute_units) {
  const long want = mp_blocks(B, kBlock), cap = 2L * (compute_units > 0 ? compute_units : 256);
  return mp_grid(want < cap ? want : cap, 1);
}

hipError_t mpk_ik(hipStream_t s, const MpModel<double>& M, const MpIkParams& P, const double* Tdes, const double* theta0, long B,
                  double* theta, int* success, int* iterations, int* restarts, unsigned long long* queue_counter, int compute_units) {
  if (B <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(queue_counter, 0, sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  MP_DISPATCH_N(M.n, return launch(k_ik<N>, ik_grid(B, compute_units), kBlock, 0, s, M, P, Tdes, theta0, B, theta, success, iterations,
                                   restarts, queue_counter))
}

hipError_t mpk_pd_regulation(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, const double* theta0, const double* des,
                             const double* Kp, const double* Kd, long K, double dt, int steps, double* err, int* count) {
  if (K <= 0) return hipSuccess;  // (steps == 0 still launches: every run reports a count of 0)
  MP_DISPATCH_N(M.n, return launch(k_pd_regulation<N>, mp_grid(K, kWave), kWave, 0, s, M, C, theta0, des, Kp, Kd, K, dt, steps, err, count))
}
hipError_t mpk_dyn_pd_regulation(hipStream_t s, int n, const MpBigModel<double>* d_model, const MpCall<double>& C, const double* theta0,
                                 const double* des, const double* Kp, const double* Kd, long K, double dt, int steps, double* err, int* count) {
  if (K <= 0) return hipSuccess;  // (steps == 0 still launches: every run reports a count of 0)
  MP_DISPATCH_CAP(n, return launch(k_dyn_pd_regulation<CAP>, mp_grid(K, kWave), kWave, 0, s, d_model, C, theta0, des, Kp, Kd, K, dt, steps, err,
                                   count))
}

template <int CAP>
static MpIkParamsT<CAP> ik_params_for(const MpIkBigParams& P) {
  MpIkParamsT<CAP> Q;
  Q.eomg = P.eomg; Q.ev = P.ev; Q.damping = P.damping; Q.step_cap = P.step_cap; Q.w_o = P.w_o; Q.w_p = P.w_p;
  Q.max_iterations = P.max_iterations; Q.seed = P.seed; Q.adaptive_tuning = P.adaptive_tuning; Q.backtracking = P.backtracking;
  for (int j = 0; j < CAP; ++j) { Q.lo[j] = P.lo[j]; Q.hi[j] = P.hi[j]; }
  return Q;
}
hipError_t mpk_dyn_ik(hipStream_t s, int n, const MpBigModel<double>* d_model, const MpIkBigParams& P, const double* Tdes, const double* theta0,
                      long B, double* theta, int* success, int* iterations, int* restarts, unsigned long long* queue_counter,
                      int compute_units) {
  if (B <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(queue_counter, 0, sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  MP_DISPATCH_CAP(n, return launch(k_dyn_ik<CAP>, ik_grid(B, compute_units), kBlock, 0, s, d_model, ik_params_for<CAP>(P), Tdes, theta0, B,
                                   theta, success, iterations, restarts, queue_counter))
}

hipError_t mpk_potential_field(hipStream_t s, const float* pos, const float* goal3_host, const float* obs, long P, long O,
                               float influence, float* pot, float* grad) {
  if (P <= 0) return hipSuccess;
  const float inv = influence > 0.0f ? (float)(1.0 / (double)influence) : 0.0f;
  return launch(k_potential_field, mp_grid(P, kBlock), kBlock, 0, s, pos, goal3_host[0], goal3_host[1], goal3_host[2], obs, P, O, inv,
                influence * influence, pot, grad);
}
