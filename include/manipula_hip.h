/* manipula_hip.h — C ABI of libmanipula_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary for the batched trajectory + rigid-body-dynamics hot path of
 * boelnasr/ManipulaPy v1.4.1.  The reference has no FFI: its "GPU side" is a set of Python
 * launchers behind a kernel registry (ManipulaPy/cuda_kernels/registry.py:46-89, :828-867) and
 * mixin methods that launch Numba kernels directly (planning/trajectory_dynamics.py:248-260,
 * :524-539; planning/trajectory.py:643).  Each entry point below is what such a launcher binds
 * (through ctypes); the reference interface it replaces is cited per function.
 *
 * Conventions
 *   - every function returns int: 0 = MP_OK, otherwise an MP_ERR_* code; mp_last_error() returns
 *     the thread-local message of the last failure on the calling thread.  There is NO CPU fallback
 *     anywhere behind this ABI: without a usable GPU the compute calls that take an mp_ctx fail with MP_ERR_HIP
 *     (the *_cpu twins at the end are separate entry points a caller selects explicitly).
 *   - arrays are C-contiguous (row-major), exactly the shapes the reference's Python API uses;
 *     "d_" parameters are device pointers obtained from mp_malloc (16-byte aligned), "h_" or
 *     unprefixed pointers are host memory owned by the caller.
 *   - kernels are enqueued on the context's compute stream and return immediately; the *_host
 *     variants copy in, launch, copy out and synchronise before returning.
 *   - a context is bound to one device; one context per process per GPU (one process per GPU for
 *     multi-GPU jobs, see mp_comm_*).  Calls on one context must not race from several threads.
 */
#ifndef MANIPULA_HIP_H
#define MANIPULA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MP_OK 0
#define MP_ERR_INVALID 1      /* bad argument (null pointer, shape, alignment, dof mismatch) */
#define MP_ERR_HIP 2          /* HIP runtime failure (no device, launch error, out of memory) */
#define MP_ERR_MODEL 3        /* robot tables rejected by the model compiler */
#define MP_ERR_UNSUPPORTED 4  /* valid request this build does not implement */
#define MP_ERR_COMM 5         /* RCCL failure */

#define MP_MAX_DOF 8      /* joints of the fully unrolled / run-time-specialisable kernels */
#define MP_BIG_DOF 32     /* joints mp_model_create accepts: 9..32 run looped run-time-n kernels (csrc/mp_dyn.h; every operation
                             incl. inverse kinematics; run-time specialisation is MP_ERR_UNSUPPORTED) */
#define MP_UNIQUE_ID_BYTES 128

typedef struct mp_ctx mp_ctx;     /* device context: device id, streams, device-buffer pool */
typedef struct mp_model mp_model; /* compiled robot model (host object; reaches the kernels by value or as a device copy) */
typedef struct mp_event mp_event; /* HIP event on the context's compute stream */
typedef struct mp_graph mp_graph; /* instantiated HIP graph captured from the context's compute stream */
typedef struct mp_comm mp_comm;   /* RCCL communicator (one rank per process) */

/* ---- library / device ----------------------------------------------------------------------- */
int mp_version(void);                 /* ABI version, currently 1 */
const char* mp_last_error(void);      /* message of the last error on this thread ("" if none) */
/* Number of visible HIP devices; 0 with MP_OK when the runtime loads but finds none.
 * Replaces the reference's CUDA probe, cuda_kernels/_runtime.py:32-73 / registry.py:92-137. */
int mp_device_count(int* count);
int mp_ctx_create(int device_id, mp_ctx** out);
int mp_ctx_destroy(mp_ctx* ctx);
int mp_ctx_synchronize(mp_ctx* ctx);  /* waits for every stream of the context */
/* The context's compute stream as a hipStream_t (returned through a void*: no HIP header is needed to include this file), for a
 * caller that orders its own HIP work - a copy, a kernel of its own - behind the library's launches.  Stream order is the whole
 * contract: every device-pointer entry point returns with everything its result needs enqueued on this stream.  (Before this call
 * the float64 pass of a float32 inverse-dynamics launch on pool arrays may stay parked - note at mp_id_trajectory_f32; the call runs
 * what is parked and switches parking OFF for the rest of the context's life: mp_malloc returns plain device pointers, so a caller
 * that holds the stream can read pool memory with its own copies and kernels.)  The reference has no streams of its
 * own to expose (its launchers return finished host arrays, cuda_kernels/trajectory_kernels.py:1043-1081). */
int mp_ctx_get_stream(mp_ctx* ctx, void** hip_stream);
/* Stream order with a caller's stream (a hipStream_t through a void*; NULL = the device's null stream) WITHOUT handing the compute
 * stream out, so parking is left as it is (unlike mp_ctx_get_stream): each records a HIP event on one stream and makes the other
 * wait for it.  _wait_for_stream: the compute stream waits for what is enqueued on hip_stream so far; _stream_wait_for_ctx:
 * hip_stream waits for what is enqueued on the compute stream so far (parked passes are run first).  A framework that hands device
 * tensors to the device-pointer entry points joins both ways around them (manipulapy_amd/autograd.py). */
int mp_ctx_wait_for_stream(mp_ctx* ctx, void* hip_stream);
int mp_ctx_stream_wait_for_ctx(mp_ctx* ctx, void* hip_stream);
/* name, CU count, total HBM bytes — replaces get_gpu_properties(), cuda_kernels/registry.py:335-356 */
int mp_ctx_properties(mp_ctx* ctx, char* name, size_t name_len, int* compute_units, uint64_t* hbm_bytes);
/* Launch a 1-block probe kernel that writes its lane ids and check the result on the host.
 * Replaces the reference's device self-test kernel, cuda_kernels/_runtime.py:127-138. */
int mp_selftest(mp_ctx* ctx);
/* Device-copy microbenchmark for the roofline ("confirm the peak with a device-copy microbenchmark in the same
 * run"): `reps` launches of dst = a (reads = 1) or dst = a + b + c (reads = 3, the 3 : 1 byte mix of the inverse-dynamics
 * kernels) over arrays of bytes_per_array bytes, 16 bytes per lane; *gb_per_s = (reads + 1) * bytes * reps / elapsed.
 * reads = 11 / 13: the same two kernels with non-temporal loads and stores (what the whole-line row movers use).
 * Nothing in the reference corresponds to it. */
int mp_stream_bandwidth(mp_ctx* ctx, size_t bytes_per_array, int reads, int reps, double* gb_per_s);
/* The same probe for any of the byte mixes the kernels have (reads : writes = 0:1, 1:1, 2:1, 3:1, 1:2, 1:3, 2:3): every lane
 * reads one 16-byte chunk from each of `reads` arrays and writes one to each of `writes` arrays of bytes_per_array bytes, plain
 * or non-temporal; *gb_per_s = (reads + writes) * bytes * reps / elapsed.  bench.py runs it with a configuration's own mix and
 * size right before its timed region: roofline.frac_of_probe says how much of what THIS box streams the kernel reaches. */
int mp_stream_bandwidth_mix(mp_ctx* ctx, size_t bytes_per_array, int reads, int writes, int nontemporal, int reps, double* gb_per_s);

/* The shader clock the GPU holds WHILE the caller's launches run (measurement plumbing, nothing in the reference corresponds to it):
 * _begin starts a bounded sampler on a stream of its own (8 one-wave blocks stamping s_memtime / s_memrealtime over about
 * duration_ms, 0 < duration_ms <= 2000), the caller launches what it wants measured, _end waits for the sampler and returns
 * *clock_hz = median over the blocks of delta s_memtime / delta s_memrealtime x 100 MHz and, optionally, the time the stamps span.
 * bench.py reports it as `clock_hz` beside every configuration's kernel time (the package's power controller runs the same code
 * object at 1.7 - 2.5 GHz depending on the kernel's mix and the box). */
int mp_clock_sample_begin(mp_ctx* ctx, double duration_ms);
int mp_clock_sample_end(mp_ctx* ctx, double* clock_hz, double* sampled_ms);

/* Profiling (replaces the reference's profile_start / profile_stop hooks, planning/trajectory_planning.py:295-296, and
 * the timing part of its performance_stats): while on, every device-pointer entry point (and so every *_host one)
 * brackets what it enqueues with a timed HIP event pair on the compute stream and an roctx range named after the
 * entry point (visible to rocprofv3 --marker-trace).  mp_ctx_profile waits for the pairs recorded since the last
 * read and returns the accumulated kernel milliseconds, the number of timed calls and the last call's milliseconds
 * (any output may be NULL); reset != 0 zeroes the accumulators afterwards.  Off by default; not active while a launch
 * graph is being captured. */
int mp_ctx_set_profiling(mp_ctx* ctx, int on);
int mp_ctx_profile(mp_ctx* ctx, double* kernel_ms_total, int64_t* timed_calls, double* kernel_ms_last, int reset);

/* ---- device memory (pooled per context; replaces _GlobalCudaMemoryPool, cuda_kernels/memory.py:55-118,
 *      and the pinned-H2D helper _h2d_pinned, cuda_kernels/memory.py:12-50) ----------------------- */
int mp_malloc(mp_ctx* ctx, size_t bytes, void** d_ptr);
int mp_free(mp_ctx* ctx, void* d_ptr);            /* returns the buffer to the pool */
int mp_pool_trim(mp_ctx* ctx);                    /* releases pooled buffers back to the driver */
int mp_memcpy_h2d(mp_ctx* ctx, void* d_dst, const void* h_src, size_t bytes); /* synchronous */
int mp_memcpy_d2h(mp_ctx* ctx, void* h_dst, const void* d_src, size_t bytes); /* synchronous */
int mp_memset(mp_ctx* ctx, void* d_dst, int value, size_t bytes);
/* page-locked host buffers (the reference's pinned staging, cuda_kernels/memory.py:12-50, handed to the caller): the
 * *_host_* entry points below accept any host pointer; on buffers from mp_host_alloc the upload, the kernels and
 * the download of a large call overlap chunk by chunk (pageable memory is staged by the runtime and serialises).
 * When a *_host_* entry point returns an error, no transfer to or from the caller's arrays is pending any more, and
 * the contents of its output arrays are unspecified. */
int mp_host_alloc(mp_ctx* ctx, size_t bytes, void** h_ptr);
int mp_host_free(mp_ctx* ctx, void* h_ptr); /* ctx may be NULL: the buffer outlives the context that allocated it */

/* ---- timing on the compute stream ------------------------------------------------------------ */
int mp_event_create(mp_ctx* ctx, mp_event** out);
int mp_event_destroy(mp_event* ev);
int mp_event_record(mp_ctx* ctx, mp_event* ev);   /* on the stream the kernels are launched on */
int mp_event_elapsed_ms(mp_event* start, mp_event* stop, float* ms); /* synchronises on `stop` */

/* ---- launch graphs ----------------------------------------------------------------------------
 * Every device-pointer entry point below only enqueues kernels on the context's compute stream, so a sequence of
 * them can be captured once and replayed with a single submission (hipGraph): between mp_graph_begin and
 * mp_graph_end the calls are recorded instead of executed.  Replaying re-runs the same kernels on the same
 * device pointers with the same per-call constants; the caller refreshes the buffers' contents in between.
 * (The reference has no counterpart: its launchers pay one Numba dispatch per kernel, cuda_kernels/registry.py:828-867.)
 * Not capturable: the *_host_* entry points, mp_malloc / mp_free, mp_model_specialize, mp_comm_*. */
int mp_graph_begin(mp_ctx* ctx);
int mp_graph_end(mp_ctx* ctx, mp_graph** out);
int mp_graph_launch(mp_ctx* ctx, mp_graph* graph);   /* asynchronous, on the compute stream */
int mp_graph_destroy(mp_graph* graph);

/* ---- robot model ------------------------------------------------------------------------------
 * Inputs are the reference's constant tables (urdf/core.py:670-769; ManipulatorDynamics ctor,
 * dynamics/manipulator_dynamics.py:43-86), float64 row-major:
 *   S (6,n) space screws [w;v]; Mcom n x (4,4) = Mlist_per_link; G n x (6,6) = Glist;
 *   M_ee (4,4) = M_list; joint_limits (n,2) or NULL (= unbounded); torque_limits (n,2) or NULL
 *   (= +-inf, planning/trajectory_planning.py:219-223).  Limits are rounded to float32 as the
 *   planner stores them (:218).  No device is needed: the model is host data.  1 <= n <= MP_BIG_DOF (the reference's
 *   algorithms loop over any n, dynamics/mass_matrix.py:62-96; its database goes up to 10 actuated joints). */
int mp_model_create(int n, const double* S, const double* Mcom, const double* G, const double* M_ee,
                    const double* joint_limits, const double* torque_limits, mp_model** out);
/* Also releases what every live context holds for the model (specialised code object, device-resident copies); while a
 * launch graph captured on a context is alive, or a capture is open, they are retired instead and released with the last
 * graph / the context (a graph keeps kernel nodes and device addresses of the models it captured, no reference). */
int mp_model_destroy(mp_model* model);
int mp_model_dof(const mp_model* model, int* n);
/* Compiled per-joint parameters, 16 doubles per joint (see csrc/mp_model.h): for inspection/tests. */
int mp_model_params(const mp_model* model, double* out /* n*16 */);
/* The whole compiled model as the kernels receive it (struct MpModel<float|double>, csrc/mp_model.h):
 * *bytes = its size; out may be NULL to query the size.  Used by the kernel specialiser and by tests. */
int mp_model_blob(const mp_model* model, int use_f64, void* out, size_t* bytes);
/* End-effector pose through the compiled chain on the HOST in float64 (model self-check helper). */
int mp_model_fk_host(const mp_model* model, const double* q /* n */, double* T /* 16 */);

/* ---- run-time specialisation (new; csrc/mp_jit.cpp) -------------------------------------------------
 * Compile the float32 kernels with THIS robot's constants baked in (hiprtc, gfx950; on-disk cache in
 * MANIPULAPY_HIP_CACHE or <library dir>/jit_cache) and load them on the context's device.  Afterwards
 * mp_id_trajectory_f32 / mp_traj_id_fused_f32 / mp_fd_trajectory_f32 (+ their *_host forms) use them for
 * this (context, model) pair; every other entry point keeps using the generic kernels.  Idempotent.
 * MANIPULAPY_HIP_SPECIALIZE=0 makes the launchers ignore specialised kernels (A/B measurements). */
int mp_model_specialize(mp_ctx* ctx, const mp_model* model);
int mp_model_is_specialized(mp_ctx* ctx, const mp_model* model, int* yes);
/* Generate + compile only (needs hiprtc, no GPU): size of the two code objects together and whether both came from the cache. */
int mp_model_specialize_compile(const mp_model* model, size_t* code_bytes, int* from_cache);
/* The two generated translation units (NUL-terminated; the second - the one-row-per-lane float32 inverse dynamics, compiled with
 * another scheduling strategy - behind a "// ==== second program" line).  *len = required size incl. NUL; buf may be NULL. */
int mp_model_specialize_source(const mp_model* model, char* buf, size_t* len);

/* ---- hot path, device pointers ----------------------------------------------------------------
 * g: (3,) gravity vector or NULL (= [0,0,-9.81], planning/trajectory_dynamics.py:54);
 * Ftip: (6,) SPACE-frame wrench [m;f] or NULL (= 0) (dynamics/id_fd.py:41-47). */

/* pos/vel/acc (B,N,n) float32 for B start/end pairs (B,n): time scaling of
 * planning/trajectory.py:15-75 + clip of positions to the joint limits (:311-313, :479-481).
 * Replaces batch_trajectory_kernel, cuda_kernels/trajectory_kernels.py:763-831, and its launcher
 * optimized_batch_trajectory_generation (:1204-1290); B = 1 is joint_trajectory (registry launchers
 * "trajectory.*", cuda_kernels/registry.py:828-867).  method: 3 cubic, 5 quintic, else zeros. */
int mp_batch_trajectory_f32(mp_ctx* ctx, const mp_model* model, const float* d_start, const float* d_end,
                            int64_t B, int64_t N, double Tf, int method, float* d_pos, float* d_vel, float* d_acc);

/* tau (rows,n) = clip(inverse_dynamics(q, qd, qdd, g, Ftip), torque_limits) for `rows` independent
 * (trajectory, timestep) rows.  Replaces _inverse_dynamics_gpu / inverse_dynamics_kernel
 * (planning/trajectory_dynamics.py:92-306, cuda_kernels/trajectory_kernels.py:521-602) with the
 * arithmetic of _inverse_dynamics_cpu (:308-380) -> dynamics/id_fd.py:16-48.
 *
 * float32 rows, adaptive precision.  The float32 kernels hand the few rows per thousand whose torques are a small difference of
 * large terms (csrc/mp_core.h, MpRowScale / mp_id_row_is_hard) to a float64 pass behind them, so that EVERY row holds the
 * float32 parity bound.  When the call returns:
 *   - arrays the CALLER allocated (hipMalloc, a framework tensor - anything not from mp_malloc): kernel and pass are both
 *     enqueued on the compute stream.  Whatever the caller enqueues there next - or a wait on that stream - sees the complete
 *     torques; the arrays may be freed or reused as soon as the stream has passed the call, like after any asynchronous launch.
 *   - arrays from this context's pool (mp_malloc), all four of them: the pass may stay PARKED - to ride with the next launch of the
 *     same robot-specialised kernel on other arrays (that launch's first workgroups work it off), or to run together with the
 *     passes of up to three more launches.  It runs before anything can see the difference: every other entry point of the context
 *     (mp_memcpy_*, mp_ctx_synchronize, mp_event_record, mp_ctx_get_stream, the *_host calls, the communicator ...), a launch
 *     whose arrays overlap the parked one's, a fifth launch, mp_ctx_destroy.  Without the compute stream (mp_ctx_get_stream) pool
 *     memory is only reachable through those; once the stream has been handed out, nothing is parked any more (as for caller-owned arrays).
 * The same holds for mp_traj_id_fused_f32 (start / end / tau). */
int mp_id_trajectory_f32(mp_ctx* ctx, const mp_model* model, const float* d_q, const float* d_qd,
                         const float* d_qdd, int64_t rows, const double* g, const double* Ftip, float* d_tau);
int mp_id_trajectory_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd,
                         const double* d_qdd, int64_t rows, const double* g, const double* Ftip, double* d_tau);

/* joint_trajectory -> inverse_dynamics_trajectory fused: tau (B,N,n) straight from (B,n) start/end
 * pairs; the intermediate positions (clipped) / velocities / accelerations are rounded to float32
 * exactly as the two-call pipeline would store them, but never touch HBM. */
int mp_traj_id_fused_f32(mp_ctx* ctx, const mp_model* model, const float* d_start, const float* d_end,
                         int64_t B, int64_t N, double Tf, int method, const double* g, const double* Ftip,
                         float* d_tau);

/* Per row: T (4,4) = forward_kinematics(q,"space") (kinematics/fk.py:59-70), J (6,n) =
 * jacobian(q,"space") (kinematics/jacobian.py:62-73), tau as above.  Any of d_T / d_J / d_tau may
 * be NULL to skip that output (d_qd/d_qdd may then be NULL too). */
int mp_fk_jac_id_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd,
                     const double* d_qdd, int64_t rows, const double* g, const double* Ftip, double* d_T,
                     double* d_J, double* d_tau);
int mp_fk_jac_id_f32(mp_ctx* ctx, const mp_model* model, const float* d_q, const float* d_qd,
                     const float* d_qdd, int64_t rows, const double* g, const double* Ftip, float* d_T,
                     float* d_J, float* d_tau);

/* M (rows,n,n) = mass_matrix(q) per row (dynamics/mass_matrix.py:16-99), symmetrised like the reference. */
int mp_mass_matrix_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, int64_t rows, double* d_M);
int mp_mass_matrix_f32(mp_ctx* ctx, const mp_model* model, const float* d_q, int64_t rows, float* d_M);

/* qdd (rows,n) = forward_dynamics(q, qd, tau, g, Ftip) per row = solve(M, tau - c - g - Js^T Ftip)
 * (dynamics/id_fd.py:50-83); one g / Ftip for all rows. */
int mp_forward_dynamics_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd,
                            const double* d_tau, int64_t rows, const double* g, const double* Ftip, double* d_qdd);
/* float32 (float32 model, bias recursion, CRBA and Cholesky; no float64 re-evaluation).  Accuracy, per row, against the float64
 * solution of the same float32 inputs (tests/test_gpu_row_dynamics.py, tests/test_row_dynamics_host.py):
 *   backward, any chain:  max|M qdd - (tau - bias)| <= 1e-5 (max|M| max|qdd| + max|tau| + max|bias|);
 *   forward, well-conditioned arms (the suite's UR5 / xArm6 / iiwa14 / Panda, cond(M) up to ~3e4):
 *                         max|qdd - qdd_ref| <= 1e-4 max|qdd_ref|.
 * The forward error grows with cond(M): on a badly conditioned chain it is not bounded by the second rule.  A row with a NaN or
 * inf in q, qd or tau comes back NaN; the other rows are unaffected. */
int mp_forward_dynamics_f32(mp_ctx* ctx, const mp_model* model, const float* d_q, const float* d_qd,
                            const float* d_tau, int64_t rows, const double* g, const double* Ftip, float* d_qdd);

/* Analytical first derivatives (float64, models of 1..8 joints - MP_ERR_UNSUPPORTED above that).  No counterpart in this ABI's
 * reference interface: the reference differentiates its torch / JAX backends with autograd (README "Differentiable");
 * these are the same Jacobians, computed per row by forward-mode tangents through the Newton-Euler recursion (csrc/mp_deriv.h).
 * Every (rows,n,n) output holds [row][i][j] = d out_i / d in_j; outputs marked "may be NULL" are skipped when NULL.  A row with a
 * non-finite input comes back NaN in every output of that row only.  Derivatives are those of the unclipped torque.
 *   inverse dynamics at (q, qd, qdd):  tau (rows,n, may be NULL), dtau_dq, dtau_dqd (rows,n,n), M = dtau_dqdd (rows,n,n, may be NULL)
 *   forward dynamics at (q, qd, tau):  qdd (rows,n, may be NULL), dqdd_dq = -M^-1 dtau_dq, dqdd_dqd = -M^-1 dtau_dqd (rows,n,n),
 *                                      Minv = dqdd_dtau (rows,n,n, may be NULL)
 * The device forms are asynchronous (no synchronisation: they may be captured into a launch graph). */
int mp_id_derivatives_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_qdd,
                          int64_t rows, const double* g, const double* Ftip, double* d_tau, double* d_dtau_dq, double* d_dtau_dqd,
                          double* d_M);
int mp_fd_derivatives_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_tau,
                          int64_t rows, const double* g, const double* Ftip, double* d_qdd, double* d_dqdd_dq, double* d_dqdd_dqd,
                          double* d_Minv);
/* Vector-Jacobian products of the same two functions (float64, models of 1..8 joints - MP_ERR_UNSUPPORTED above that), by reverse
 * mode through the Newton-Euler recursion (csrc/mp_adjoint.h): O(n) per row, no Jacobian formed.  All arrays (rows,n).
 *   inverse dynamics at (q, qd, qdd), cotangent gtau:  gq = dtau_dq^T gtau, gqd = dtau_dqd^T gtau, gqdd = M gtau (may be NULL)
 *   forward dynamics at (q, qd, tau), cotangent gqdd:  qdd (may be NULL), gtau = M^-1 gqdd (may be NULL), gq = dqdd_dq^T gqdd,
 *                                                      gqd = dqdd_dqd^T gqdd
 * Derivatives of the unclipped torque; a row with a non-finite input or cotangent comes back NaN in every output of that row only.
 * The device forms are asynchronous (no synchronisation, no allocation: they may be captured into a launch graph); the _host forms
 * take their device memory from the context's pool; the _cpu twins are listed with the others below. */
int mp_id_vjp_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_qdd, const double* d_gtau,
                  int64_t rows, const double* g, const double* Ftip, double* d_gq, double* d_gqd, double* d_gqdd);
int mp_fd_vjp_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_tau, const double* d_gqdd,
                  int64_t rows, const double* g, const double* Ftip, double* d_qdd, double* d_gq, double* d_gqd, double* d_gtau);

/* Vector-Jacobian products of forward kinematics and the Jacobian (float64, models of 1..8 joints - MP_ERR_UNSUPPORTED above that), by
 * reverse mode through the compiled chain (csrc/mp_kin_vjp.h): O(n) per row, no 4x4xn or 6xnxn tensor formed.
 *   frame 0 = space, 1 = body (anything else is refused).  q (rows,n); cotangents gT (rows,4,4) and gJ (rows,6,n), either may be NULL
 *   (= 0); outputs T (rows,4,4), J (rows,6,n, in `frame`) and gq = d<gT, T> / dq + d<gJ, J> / dq (rows,n), each may be NULL, at least
 *   one required.  The cotangents are read only for gq; the bottom row of gT does not contribute.  With no cotangents this is FK plus
 *   the Jacobian in either frame.
 * A row with a non-finite q or cotangent comes back NaN in every output of that row only.  The device form is asynchronous (no
 * synchronisation, no allocation: it may be captured into a launch graph); the _host form takes its device memory from the context's
 * pool; the _cpu twin is listed with the others below. */
int mp_fk_jac_vjp_f64(mp_ctx* ctx, const mp_model* model, int frame, const double* d_q, const double* d_gT, const double* d_gJ,
                      int64_t rows, double* d_T, double* d_J, double* d_gq);

/* Operational-space (task-space) dynamics and task-space computed torque (float64, models of 1..8 joints - MP_ERR_UNSUPPORTED above
 * that; csrc/mp_opspace.h).  Twists are [w; v].  frame 0 = space, 1 = body, 2 = hybrid (J_h = blkdiag(R, R) J_b, R the rotation of
 * T = FK(q): angular velocity and tool-origin velocity, both in space axes); task 0 = full (m = 6 rows), 1 = linear (rows 3..5, m = 3),
 * 2 = angular (rows 0..2, m = 3); anything else is refused, as is a negative or non-finite damping.  With J the selected m x n block,
 * c(q, qd) the velocity-product torques, g(q) the gravity torques (g = NULL: (0, 0, -9.81)) and lambda = damping:
 *   A = J M^-1 J^T + lambda^2 1 (m x m)    Lambda = A^-1    Jbar = M^-1 J^T Lambda (n x m, the dynamically consistent inverse)
 *   mu = Lambda (J M^-1 c - Jdot qd)       p = Lambda J M^-1 g
 *   tau(a*, tau0) = J^T (Lambda a* + mu + p) + (1 - J^T Jbar^T) tau0
 * so that, with lambda = 0, forward dynamics of tau gives J qdd + Jdot qd = a* whatever the null-space torque tau0 is.  No tip wrench
 * enters: a wrench F at the tool is the caller's J^T F added to tau.  A is formed through the Cholesky factor of M (W = L^-1 J^T,
 * A = W^T W + lambda^2 1) and factored by Cholesky itself; M^-1 is never formed.
 *   mp_opspace_f64: q, qd (rows,n) -> T (rows,4,4), J (rows,m,n), Jdqd = Jdot qd (rows,m), Lambda (rows,m,m), Jbar (rows,n,m),
 *     mu (rows,m), p (rows,m); every output may be NULL, at least one is required.
 *   mp_opspace_torque_f64: q, qd (rows,n), acc = a* (rows,m), tau0 (rows,n) or NULL (= 0) -> tau (rows,n); nothing wider than a row of
 *     n values is read or written.
 * A pivot d_j of the Cholesky factorisation of A that is not positive makes the Lambda-dependent outputs of that row NaN (Lambda, Jbar,
 * mu, p, tau); T, J and Jdqd of the row stay valid.  "Positive" is judged against rounding: d_j > 2^-46 A_jj (64 eps, what the
 * subtracted products and W leave in d_j; a matrix that fails has cond(A) above 1e13).  The converse is not promised: rounding can
 * lift the pivot of a singular A over the threshold, so with damping = 0 a singular or nearly singular pose (cond(A) > 1e13) gives
 * either NaN or finite values of the size of 1 / (eps |A|) - check cond(A) or use a damping where that matters.  A damping too small
 * to lift a pivot over the threshold (lambda^2 <= 2^-46 A_jj, lambda below about 1e-7 for A_jj of order 1) changes nothing: choose
 * one that matters at the scale of A.  One case is decided without factorising: a task with more rows than the chain has joints
 * (m > n) has rank(A) <= n < m at every pose, and with damping = 0 every row is NaN in Lambda, Jbar, mu, p and tau (T, J and Jdqd
 * stay valid).  A row with a non-finite input comes back NaN in every output of that row only.
 * rows = 0 is a no-op.  The device forms are asynchronous (no synchronisation, no allocation: they may be captured into a launch graph);
 * the _host forms take their device memory from the context's pool; the _cpu twins are listed with the others below. */
int mp_opspace_f64(mp_ctx* ctx, const mp_model* model, int frame, int task, double damping, const double* d_q, const double* d_qd,
                   int64_t rows, const double* g, double* d_T, double* d_J, double* d_Jdqd, double* d_Lambda, double* d_Jbar, double* d_mu,
                   double* d_p);
int mp_opspace_torque_f64(mp_ctx* ctx, const mp_model* model, int frame, int task, double damping, const double* d_q, const double* d_qd,
                          const double* d_acc, const double* d_tau0, int64_t rows, const double* g, double* d_tau);

/* forward_dynamics_trajectory for B independent trajectories (planning/trajectory_dynamics.py:382-423,
 * :580-708; replaces forward_dynamics_kernel, cuda_kernels/trajectory_kernels.py:604-705): semi-implicit
 * Euler, intRes sub-steps of dt/intRes, positions clipped to the joint limits after every sub-step, row 0 =
 * initial state.  theta0/dtheta0 (B,n), taumat (B,N,n), Ftipmat (B,N,6) or NULL (= no wrench); the state is
 * integrated in the input precision, pos/vel/acc (B,N,n) are float32 as the reference stores them. */
int mp_fd_trajectory_f32(mp_ctx* ctx, const mp_model* model, const float* d_theta0, const float* d_dtheta0,
                         const float* d_taumat, const float* d_Ftipmat, int64_t B, int64_t N, const double* g,
                         double dt, int intRes, float* d_pos, float* d_vel, float* d_acc);
int mp_fd_trajectory_f64(mp_ctx* ctx, const mp_model* model, const double* d_theta0, const double* d_dtheta0,
                         const double* d_taumat, const double* d_Ftipmat, int64_t B, int64_t N, const double* g,
                         double dt, int intRes, float* d_pos, float* d_vel, float* d_acc);

/* The same roll-out on the TIME-MAJOR device layout: d_taumat (N,B,n), d_Ftipmat (N,B,6) or NULL, d_pos / d_vel / d_acc
 * (N,B,n); d_theta0 / d_dtheta0 stay (B,n).  The reference integrates ONE trajectory (planning/trajectory_dynamics.py:
 * 382-423, :580-708); the batch axis is this library's extension, and with time outermost the trajectories of a wavefront
 * are neighbours in memory at every step (whole cache lines per step instead of 4-step LDS tiles): the faster form for
 * callers that keep their histories on the device.  Results are element for element those of mp_fd_trajectory_*. */
int mp_fd_trajectory_tm_f32(mp_ctx* ctx, const mp_model* model, const float* d_theta0, const float* d_dtheta0,
                            const float* d_taumat, const float* d_Ftipmat, int64_t B, int64_t N, const double* g,
                            double dt, int intRes, float* d_pos, float* d_vel, float* d_acc);
int mp_fd_trajectory_tm_f64(mp_ctx* ctx, const mp_model* model, const double* d_theta0, const double* d_dtheta0,
                            const double* d_taumat, const double* d_Ftipmat, int64_t B, int64_t N, const double* g,
                            double dt, int intRes, float* d_pos, float* d_vel, float* d_acc);
/* Inverse-dynamics regressor and the normal equations of inertial-parameter identification (float64, models of 1..8 joints -
 * MP_ERR_UNSUPPORTED above that; csrc/mp_regressor.h).  No counterpart in this ABI's reference interface.  Inverse dynamics is
 * linear in the ten inertial parameters of every link:  tau = Y(q, qd, qdd, g) pi + tau_ext(q, Ftip),  pi = n x [m, hx, hy, hz,
 * Ixx, Ixy, Ixz, Iyy, Iyz, Izz] in link i's CoM frame at the home pose (Mlist_per_link[i]), h = m c, I about that frame's origin;
 * tau_ext is the tip wrench's share.  Torques are the unclipped ones.
 *   regressor:        Y (rows, n, 10n) as [row][j][10 k + c] (zero for k < j), tau_ext (rows, n, may be NULL).  A row with a
 *                     non-finite input comes back NaN in its row of Y and tau_ext.
 *   normal equations: A = sum Y^T Y (10n, 10n, full and symmetric; may be NULL: then only b and rr), b = sum Y^T (rhs - tau_ext)
 *                     (10n), rr = sum |rhs - tau_ext|^2 (1), over all rows, Y never stored.  With A = NULL, Ftip = NULL and rhs a
 *                     cotangent of tau, b is the parameter vector-Jacobian product.  A non-finite input in any row (rhs included)
 *                     makes A, b and rr NaN; rows = 0 gives zeros.  A fixed grid, per-workgroup partials added in a fixed order
 *                     and no floating-point atomics: repeat calls are bit-identical.
 * The device forms are asynchronous (no synchronisation, no allocation: they may be captured into a launch graph); d_work holds
 * mp_id_regressor_normal_workspace_bytes(model, rows) (the byte count, or minus an MP_ERR_* code).  The host forms take their
 * device memory from the context's pool. */
int mp_id_regressor_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_qdd, int64_t rows,
                        const double* g, const double* Ftip, double* d_Y, double* d_tau_ext);
int64_t mp_id_regressor_normal_workspace_bytes(const mp_model* model, int64_t rows);
int mp_id_regressor_normal_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_qdd,
                               const double* d_rhs, int64_t rows, const double* g, const double* Ftip, void* d_work, double* d_A,
                               double* d_b, double* d_rr);
/* Gradients of forward_dynamics_trajectory (float64, models of 1..8 joints - MP_ERR_UNSUPPORTED above that; intRes >= 1): the
 * vector-Jacobian product of the roll-out above, by a reverse pass through its sub-steps (csrc/mp_rollout_vjp.h).  No counterpart in
 * this ABI's reference interface, whose torch backend differentiates the roll-out with autograd.  Given the cotangents gpos / gvel /
 * gacc of the three (N, n) row arrays (each may be NULL = zero) it returns dL/dtheta0, dL/ddtheta0 (B,n) and dL/dtaumat (N rows,
 * row 0 always zero).  The clip's gradient is torch.clamp's (inclusive limits); derivatives are those of the unclipped torque, the
 * float32 cast of the rows counts as the identity, and g / Ftipmat are constants.  A trajectory whose inputs or forward state turn
 * non-finite gets NaN in all of its gradients.
 *   _tm_f64:   device pointers, time-major taumat / Ftipmat / gpos / gvel / gacc / gtaumat (N,B,*); d_work holds
 *              mp_fd_trajectory_vjp_workspace_bytes(model, B, N, intRes) = (B N + B intRes) 2n doubles.  Asynchronous (no
 *              synchronisation, no allocation: it may be captured into a launch graph).
 *   _host_f64: batch-major host arrays (B,N,*); converted on the device, workspace from the context's pool, the batch cut into
 *              chunks of whole trajectories whose workspace stays under MANIPULAPY_HIP_VJP_WORK_BYTES (default 1 GiB).
 *   _cpu_f64:  the CPU twin on batch-major host arrays.
 * mp_fd_trajectory_vjp_workspace_bytes returns the byte count, or minus an MP_ERR_* code. */
int64_t mp_fd_trajectory_vjp_workspace_bytes(const mp_model* model, int64_t B, int64_t N, int intRes);
int mp_fd_trajectory_vjp_tm_f64(mp_ctx* ctx, const mp_model* model, const double* d_theta0, const double* d_dtheta0,
                                const double* d_taumat, const double* d_Ftipmat, int64_t B, int64_t N, const double* g, double dt,
                                int intRes, const double* d_gpos, const double* d_gvel, const double* d_gacc, void* d_work,
                                double* d_gtheta0, double* d_gdtheta0, double* d_gtaumat);
/* Batched iLQR about a roll-out (float64, models of 1..8 joints - MP_ERR_UNSUPPORTED above that; intRes = 1, gravity per call, no tip
 * wrench; N >= 2, else MP_ERR_INVALID): the Riccati backward pass and the closed-loop roll-out (csrc/mp_ilqr.h).  No counterpart in this
 * ABI's reference interface.  Indexing is the roll-out's: rows i = 0..N-1, row 0 the given state, torque row i >= 1 drives step i
 * (torque row 0 is unused), h = dt:
 *     a = FD(q_{i-1}, qd_{i-1}, u_i; g),  qd_i = qd_{i-1} + h a,  w = q_{i-1} + h qd_i,  q_i = clip(w, qmin, qmax),
 *     m = [qmin <= w <= qmax]  (inclusive, as the roll-out's gradient)
 * State x = (q, qd).  With Aq = da/dq, Av = da/dqd, Mi = M^-1 - the three blocks of mp_fd_derivatives_f64 at (q_{i-1}, qd_{i-1}, u_i) -
 *     A_i = [[m (1 + h^2 Aq), m h (1 + h Av)], [h Aq, 1 + h Av]],    B_i = [[m h^2 Mi], [h Mi]]      (m scales rows)
 * Cost per trajectory, diagonal weights shared by the batch (host vectors wq, wf of 2n and wr of n entries), e = x - xref, xref per
 * trajectory (N rows of 2n):
 *     J = 1/2 sum_{i=1}^{N-1} u_i^T wr u_i + 1/2 sum_{i=1}^{N-2} e_i^T wq e_i + 1/2 e_{N-1}^T wf e_{N-1}
 * Backward pass, i = N-1 .. 1, from S = diag(wf), s = wf e_{N-1}:
 *     Qx = A^T s,  Qu = wr u_i + B^T s,  Qxx = A^T S A,  Quu = diag(wr) + B^T S B,  Qux = B^T S A
 *     K_i = -(Quu + reg 1)^-1 Qux,  k_i = -(Quu + reg 1)^-1 Qu  (Cholesky),  dV1 += k_i^T Qu,  dV2 += 1/2 k_i^T Quu k_i
 *     s <- Qx + K^T Quu k + K^T Qu + Qux^T k,  S <- Qxx + K^T Quu K + K^T Qux + Qux^T K  (the unregularised Quu; S kept symmetric)
 *     if i - 1 >= 1:  s += wq e_{i-1},  S += diag(wq)
 * reg (B) is per trajectory.  Outputs: K (N rows of n x 2n, row 0 zero), k (N rows of n, row 0 zero), dV (B,2) = (dV1, dV2), status (B)
 * int32: 0 fine; i > 0 the factor of Quu + reg 1 met a pivot at or below 2^-46 of its diagonal term first at step i - that trajectory
 * gets K = 0, k = 0, dV = 0; -1 a non-finite input - that trajectory's K, k (rows 1..N-1) and dV are NaN.
 * Roll-out: A B lanes, lane (a, b) runs trajectory b with u_i = tau_i + alpha[a,b] k_i + K_i (x_{i-1} - xbar_{i-1}) about the nominal
 * (pos, vel) with the roll-out's own step arithmetic; cost (A,B) = J; opos / ovel / otau (all three or none) receive the float64 states
 * and the applied torques (row 0 = theta0, dtheta0, torque row 0).  K and k may both be NULL (open loop: pos / vel are not read).  A
 * trajectory with a non-finite input or state gets a NaN cost and NaN rows.
 *   _tm_f64:   device pointers on the time-major layout: pos / vel / taumat (N,B,n), xref (N,B,2n), K (N,B,n,2n), k (N,B,n), opos /
 *              ovel / otau (N,A B,n); the blocks are those of the (N-1) B rows (pos[0:N-1], vel[0:N-1], taumat[1:N]) - contiguous
 *              slices, so mp_fd_derivatives_f64 produces them as they are (with B n odd the torque slice starts 8 bytes off the
 *              16-byte boundary that entry asks for: copy it first - mp_transpose_rows with outer = 1 is a device copy).  The kernel
 *              runs 16 lanes a trajectory with the value matrix in LDS and needs no workspace:
 *              mp_ilqr_backward_workspace_bytes(model, B, N) is 0 and d_work may be NULL.  (MANIPULAPY_HIP_ILQR_BACKWARD=lane, read at
 *              every call, selects the one-lane-per-trajectory kernel kept for A/B measurements; the byte count is then 12 n^2 B
 *              doubles and d_work is required.)  Asynchronous (no synchronisation, no allocation: may be captured into a launch graph).
 *   _host_f64: batch-major host arrays (B,N,*), K (B,N,n,2n), opos / ovel / otau (A,B,N,n); converted on the device, memory from the
 *              context's pool.  The backward form runs the derivative launch itself.
 *   _cpu_f64:  the CPU twins of the host forms.
 * mp_ilqr_backward_workspace_bytes returns the byte count, or minus an MP_ERR_* code. */
int64_t mp_ilqr_backward_workspace_bytes(const mp_model* model, int64_t B, int64_t N);
int mp_ilqr_backward_tm_f64(mp_ctx* ctx, const mp_model* model, const double* d_pos, const double* d_vel, const double* d_taumat,
                            const double* d_dqdd_dq, const double* d_dqdd_dqd, const double* d_Minv, const double* d_xref,
                            const double* wq, const double* wr, const double* wf, const double* d_reg, int64_t B, int64_t N, double dt,
                            void* d_work, double* d_K, double* d_k, double* d_dV, int32_t* d_status);
int mp_ilqr_rollout_tm_f64(mp_ctx* ctx, const mp_model* model, const double* d_theta0, const double* d_dtheta0, const double* d_taumat,
                           const double* d_pos, const double* d_vel, const double* d_K, const double* d_k, const double* d_alpha,
                           const double* d_xref, const double* wq, const double* wr, const double* wf, int64_t A, int64_t B, int64_t N,
                           const double* g, double dt, double* d_cost, double* d_opos, double* d_ovel, double* d_otau);
/* Batched time-optimal path parameterisation under torque, acceleration and velocity limits (float64, models of 1..8 joints -
 * MP_ERR_UNSUPPORTED above that; csrc/mp_toppra.h).  The method is TOPP by reachability analysis (TOPP-RA).  No counterpart in this
 * ABI's reference interface.
 * Path grid: s_i = i / (N - 1), i = 0..N-1, D = 1 / (N - 1), N >= 3 (else MP_ERR_INVALID).  The caller gives q, q' = dq/ds, q'' = d2q/ds2
 * at the grid points.  With qd = q' sd and qdd = q' sdd + q'' sd^2 the torque is tau = a sdd + b sd^2 + c,
 *     a = M(q) q',    b = M(q) q'' + C(q, q') q'  (the velocity-quadratic forces at "velocity" q'),    c = g(q) + Js^T Ftip.
 * mp_path_dynamics_f64 takes the three vectors from recursions over the row's link frames that share its joint state - (velocity 0,
 * acceleration q', no gravity), (velocity q', acceleration q'', no gravity), (everything 0, base acceleration -g, the wrench) - never
 * from a difference of inverse-dynamics results, and writes xbar_i = min_j (vmax_j / |q'_ij|)^2 over the joints with q'_ij != 0
 * (+inf when there is none).  A row with a non-finite input gets NaN in a, b, c and xbar.
 * Constraints at grid point i on (u, x) = (sdd_i, sd_i^2), each a row p u + q x + r <= 0:
 *     torque        tau_lo <= a u + b x + c <= tau_hi         (2n rows; an infinite bound is an absent row, it enters no arithmetic)
 *     acceleration  -a_max <= q' u + q'' x <= a_max           (2n rows, optional)
 *     speed         0 <= x <= xbar_i
 *     transition    K_{i+1,lo} <= x + 2 D u <= K_{i+1,hi}     (x_{i+1} = x_i + 2 D u_i)
 * Backward pass, i = N-2 .. 0 from K_{N-1} = [sd_end^2, sd_end^2]:  K_i = [min x, max x] over that polygon - two linear programmes in
 * two variables.  For fixed x the feasible u is [alpha(x), beta(x)] (alpha the largest of the lines with p < 0, beta the smallest of
 * those with p > 0, rows with p = 0 bound x directly); beta - alpha is concave and piecewise linear; from x = xbar_i (max) or 0 (min)
 * the two active lines are evaluated and x jumps to their intersection until beta >= alpha - a Newton step on a concave function,
 * monotone from outside the feasible interval, finitely many pieces.  A tangent that does not lead back: the set is empty.
 * Forward pass, i = 0 .. N-2 from x_0 = sd_start^2:  u_i = beta(x_i) (the greatest admissible acceleration),
 *     x_{i+1} = clip(x_i + 2 D u_i, K_{i+1}),    u_{N-1} := u_{N-2}  (the constraints of the last point are not imposed).
 * Time: t_0 = 0, t_{i+1} = t_i + 2 D / (sqrt x_i + sqrt x_{i+1}) (+inf through an interior stop, which is not an error), duration = t_{N-1}.
 * Rows: qd_i = q'_i sqrt x_i,  qdd_i = q'_i u_i + q''_i x_i,  tau_i = a_i u_i + b_i x_i + c_i.
 * status (B) int32: 0 fine; i + 1 (1..N-1) the controllable set is first empty, going backward, at grid point i; -2 sd_end^2 > xbar_{N-1},
 * or sd_start^2 outside K_0; -1 a non-finite input or a grid row whose q' is all zero (non-finite a, b, c or xbar in the _tm form).
 * Order of the tests: -1, the end speed, i + 1, the start speed.  With status != 0 that path's x, u, t, duration and rows are NaN and
 * its K is NaN from the failing point down (all of K for -1 and for the end speed, none of it for the start speed); other paths are
 * untouched.
 * Limits are host vectors: velocity_limits (n) finite and positive; torque_limits (n, 2) = (lo, hi) pairs, either may be infinite,
 * NULL = none; acceleration_limits (n) positive, NULL = none.  sd_start / sd_end (B) are per path.  g[3] and Ftip[6] per call, both
 * nullable, as for the inverse-dynamics entries.
 *   mp_path_dynamics_f64: device rows of q, q', q'' in any layout -> a, b, c (rows, n), xbar (rows).  Asynchronous.
 *   mp_toppra_tm_f64:     device pointers on the time-major layout: a / b / c / dq / ddq (N,B,n), xbar (N,B) -> K (N,B,2), x / u / t
 *                         (N,B), duration (B), status (B), qd / qdd / tau (N,B,n) (all three or none).  dq / ddq may be NULL without
 *                         acceleration limits and row outputs.  Asynchronous, allocates nothing, may be captured into a launch graph.
 *   mp_toppra_host_f64:   batch-major host arrays q / dq / ddq (B,N,n) -> K (B,N,2), x / u / t (B,N), duration, status (B), qd / qdd /
 *                         tau (B,N,n) (all three or none); converted on the device with mp_transpose_rows, memory from the context's pool.
 *   mp_path_dynamics_cpu_f64 / mp_toppra_cpu_f64: the CPU twins of mp_path_dynamics_f64 (host rows) and mp_toppra_host_f64;
 *   mp_toppra_sweep_cpu_f64: the sweep alone on given batch-major coefficients. */
int mp_path_dynamics_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_dq, const double* d_ddq, int64_t rows,
                         const double* velocity_limits, const double* g, const double* Ftip, double* d_a, double* d_b, double* d_c,
                         double* d_xbar);
int mp_toppra_tm_f64(mp_ctx* ctx, const mp_model* model, const double* d_a, const double* d_b, const double* d_c, const double* d_xbar,
                     const double* d_dq, const double* d_ddq, const double* torque_limits, const double* acceleration_limits,
                     const double* d_sd_start, const double* d_sd_end, int64_t B, int64_t N, double* d_K, double* d_x, double* d_u,
                     double* d_t, double* d_duration, int32_t* d_status, double* d_qd, double* d_qdd, double* d_tau);
/* d_dst (inner, outer, row_bytes) <- d_src (outer, inner, row_bytes): converts between the batch-major API arrays
 * (B,N,n) and the time-major layout (N,B,n), either way.  row_bytes: a multiple of 4, at most 256 (32 float64 joints). */
int mp_transpose_rows(mp_ctx* ctx, const void* d_src, int64_t outer, int64_t inner, int64_t row_bytes, void* d_dst);

/* cartesian_trajectory for B pose pairs (planning/trajectory.py:504-594, :676-737; replaces
 * cartesian_trajectory_kernel, cuda_kernels/trajectory_kernels.py:707-759, and the host-side orientation loop):
 * Xstart / Xend (B,4,4) float64; pos / vel / acc (B,N,3) and orientations (B,N,3,3) float32.  N >= 2. */
int mp_cartesian_trajectory_f32(mp_ctx* ctx, const double* d_Xstart, const double* d_Xend, int64_t B, int64_t N, double Tf,
                                int method, float* d_pos, float* d_vel, float* d_acc, float* d_orient);

/* Fused potential field ("potential_field.fused", cuda_kernels/field_kernels.py:20-104, registry.py:870-897):
 * potential (P,) and gradient (P,3) at positions (P,3) for one goal (3, host) and obstacles (O,3), float32. */
int mp_potential_field_f32(mp_ctx* ctx, const float* d_positions, const float* goal, const float* d_obstacles, int64_t P,
                           int64_t O, float influence_distance, float* d_potential, float* d_gradient);

/* Batched inverse kinematics: B independent pose targets (B,4,4) from initial guesses (B,n), float64.  One lane runs
 * the reference's damped-least-squares iteration (kinematics/ik.py:39-311; adaptive_tuning / backtracking select its two options, default off: no adaptive tuning, no
 * backtracking unless asked for) for one target: geometric error, damped step through a 6x6 Cholesky (== the reference's damped
 * pseudo-inverse), step cap, joint-limit projection (joint_limits: host (n,2), +-inf = open, NULL = all open), best
 * solution tracking, stagnation restart (counter-hashed noise seeded by `seed`; the reference draws from NumPy's
 * global stream).  iterations follows the reference's count (k + 1, or max_iterations + 1 when exhausted). */
int mp_inverse_kinematics_f64(mp_ctx* ctx, const mp_model* model, const double* d_T_desired, const double* d_theta0, int64_t B,
                              const double* joint_limits, double eomg, double ev, int max_iterations, double damping,
                              double step_cap, double weight_orientation, double weight_position, int adaptive_tuning, int backtracking,
                              uint32_t seed,
                              double* d_theta, int32_t* d_success, int32_t* d_iterations, int32_t* d_restarts);

/* ---- hot path, host pointers (what a Python gpu_launcher calls): H2D, launch, D2H, synchronise - */
int mp_batch_trajectory_host_f32(mp_ctx* ctx, const mp_model* model, const float* start, const float* end,
                                 int64_t B, int64_t N, double Tf, int method, float* pos, float* vel, float* acc);
int mp_id_trajectory_host_f32(mp_ctx* ctx, const mp_model* model, const float* q, const float* qd,
                              const float* qdd, int64_t rows, const double* g, const double* Ftip, float* tau);
int mp_id_trajectory_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd,
                              const double* qdd, int64_t rows, const double* g, const double* Ftip, double* tau);
int mp_traj_id_fused_host_f32(mp_ctx* ctx, const mp_model* model, const float* start, const float* end,
                              int64_t B, int64_t N, double Tf, int method, const double* g, const double* Ftip,
                              float* tau);
int mp_fk_jac_id_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd,
                          const double* qdd, int64_t rows, const double* g, const double* Ftip, double* T,
                          double* J, double* tau);

int mp_mass_matrix_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, int64_t rows, double* M);
int mp_id_regressor_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd, const double* qdd, int64_t rows,
                             const double* g, const double* Ftip, double* Y, double* tau_ext);
int mp_id_regressor_normal_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd, const double* qdd,
                                    const double* rhs, int64_t rows, const double* g, const double* Ftip, double* A, double* b,
                                    double* rr);
int mp_fd_trajectory_vjp_host_f64(mp_ctx* ctx, const mp_model* model, const double* theta0, const double* dtheta0,
                                  const double* taumat, const double* Ftipmat, int64_t B, int64_t N, const double* g, double dt,
                                  int intRes, const double* gpos, const double* gvel, const double* gacc, double* gtheta0,
                                  double* gdtheta0, double* gtaumat);
int mp_ilqr_backward_host_f64(mp_ctx* ctx, const mp_model* model, const double* pos, const double* vel, const double* taumat,
                              const double* xref, const double* wq, const double* wr, const double* wf, const double* reg, int64_t B,
                              int64_t N, const double* g, double dt, double* K, double* k, double* dV, int32_t* status);
int mp_ilqr_rollout_host_f64(mp_ctx* ctx, const mp_model* model, const double* theta0, const double* dtheta0, const double* taumat,
                             const double* pos, const double* vel, const double* K, const double* k, const double* alpha,
                             const double* xref, const double* wq, const double* wr, const double* wf, int64_t A, int64_t B, int64_t N,
                             const double* g, double dt, double* cost, double* opos, double* ovel, double* otau);
int mp_toppra_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* dq, const double* ddq,
                       const double* velocity_limits, const double* torque_limits, const double* acceleration_limits,
                       const double* sd_start, const double* sd_end, int64_t B, int64_t N, const double* g, const double* Ftip, double* K,
                       double* x, double* u, double* t, double* duration, int32_t* status, double* qd, double* qdd, double* tau);
int mp_forward_dynamics_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd,
                                 const double* tau, int64_t rows, const double* g, const double* Ftip, double* qdd);
int mp_id_derivatives_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd, const double* qdd,
                               int64_t rows, const double* g, const double* Ftip, double* tau, double* dtau_dq, double* dtau_dqd,
                               double* M);
int mp_fd_derivatives_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd, const double* tau,
                               int64_t rows, const double* g, const double* Ftip, double* qdd, double* dqdd_dq, double* dqdd_dqd,
                               double* Minv);
int mp_id_vjp_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd, const double* qdd, const double* gtau,
                       int64_t rows, const double* g, const double* Ftip, double* gq, double* gqd, double* gqdd);
int mp_fd_vjp_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd, const double* tau, const double* gqdd,
                       int64_t rows, const double* g, const double* Ftip, double* qdd, double* gq, double* gqd, double* gtau);
int mp_fk_jac_vjp_host_f64(mp_ctx* ctx, const mp_model* model, int frame, const double* q, const double* gT, const double* gJ,
                           int64_t rows, double* T, double* J, double* gq);
int mp_opspace_host_f64(mp_ctx* ctx, const mp_model* model, int frame, int task, double damping, const double* q, const double* qd,
                        int64_t rows, const double* g, double* T, double* J, double* Jdqd, double* Lambda, double* Jbar, double* mu,
                        double* p);
int mp_opspace_torque_host_f64(mp_ctx* ctx, const mp_model* model, int frame, int task, double damping, const double* q, const double* qd,
                               const double* acc, const double* tau0, int64_t rows, const double* g, double* tau);
int mp_fd_trajectory_host_f32(mp_ctx* ctx, const mp_model* model, const float* theta0, const float* dtheta0,
                              const float* taumat, const float* Ftipmat, int64_t B, int64_t N, const double* g,
                              double dt, int intRes, float* pos, float* vel, float* acc);
int mp_fd_trajectory_host_f64(mp_ctx* ctx, const mp_model* model, const double* theta0, const double* dtheta0,
                              const double* taumat, const double* Ftipmat, int64_t B, int64_t N, const double* g,
                              double dt, int intRes, float* pos, float* vel, float* acc);

int mp_cartesian_trajectory_host_f32(mp_ctx* ctx, const double* Xstart, const double* Xend, int64_t B, int64_t N, double Tf,
                                     int method, float* pos, float* vel, float* acc, float* orient);

int mp_potential_field_host_f32(mp_ctx* ctx, const float* positions, const float* goal, const float* obstacles, int64_t P,
                                int64_t O, float influence_distance, float* potential, float* gradient);

int mp_inverse_kinematics_host_f64(mp_ctx* ctx, const mp_model* model, const double* T_desired, const double* theta0, int64_t B,
                                   const double* joint_limits, double eomg, double ev, int max_iterations, double damping,
                                   double step_cap, double weight_orientation, double weight_position, int adaptive_tuning, int backtracking,
                              uint32_t seed,
                                   double* theta, int32_t* success, int32_t* iterations, int32_t* restarts);

/* K closed-loop regulation runs under joint-space PD torque, one lane each, float64 - the simulations the reference's
 * Ziegler-Nichols gain sweep runs one gain after the other (control/metrics.py:315-355: tau = Kp (des - theta) - Kd omega,
 * alpha = M^-1 (tau - c - g), omega += alpha dt, theta += omega dt, error = |theta - des|, stop after a step > 10 whose
 * error exceeds 1e10).  Host arrays: theta0 / theta_des (K,n), Kp / Kd (K); errors (K,steps) - entries past a run's
 * count are left untouched - and count (K) come back.  g: 3 doubles or NULL (0,0,-9.81). */
int mp_pd_regulation_host_f64(mp_ctx* ctx, const mp_model* model, const double* theta0, const double* theta_des, const double* Kp,
                              const double* Kd, int64_t K, const double* g, double dt, int steps, double* errors, int32_t* count);

/* ---- CPU twins (csrc/mp_cpu.cpp): what the kernel registry's cpu_launcher of each operation calls ----------------
 * The reference routes every registered operation through `gpu_launcher if _cuda_routing_enabled() else cpu_launcher`
 * (cuda_kernels/registry.py:85-89) and its planner mixins pick _*_cpu when _should_use_gpu is false
 * (planning/trajectory_dynamics.py:84-90, :414-423); its CPU launchers are NumPy code (dynamics/id_fd.py:16-83,
 * kinematics/fk.py:39-86, kinematics/jacobian.py:39-93, dynamics/mass_matrix.py:16-99,
 * planning/trajectory_dynamics.py:308-380, :580-708, planning/trajectory.py:676-737).  These entry points evaluate the
 * same per-row templates the HIP kernels instantiate, on host arrays, over `nthreads` host threads (0 = all cores, or
 * MANIPULAPY_CPU_THREADS).  No context and no GPU are involved; they are selected by the routing rule (NumPy backend
 * active / use_cuda=False), never as a fallback of a failing GPU call.  Same argument meaning as the *_host forms. */
int mp_cpu_threads(int64_t items); /* threads a call over `items` rows would use */
int mp_id_trajectory_cpu_f32(const mp_model* model, const float* q, const float* qd, const float* qdd, int64_t rows,
                             const double* g, const double* Ftip, float* tau, int nthreads);
int mp_id_trajectory_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* qdd, int64_t rows,
                             const double* g, const double* Ftip, double* tau, int nthreads);
/* Diagnostic: in_f64[r] = 1 where the float32 inverse-dynamics kernels (and mp_id_trajectory_cpu_f32) evaluate row r in float64 -
 * the rows whose joint wrenches exceed 16 x their largest torque, where a float32 recursion cannot hold the parity bound
 * 1e-4 |ref| + 5e-6 max|row| (csrc/mp_core.h, mp_rnea_row).  No counterpart in the reference, whose path is float64 throughout
 * (planning/trajectory_dynamics.py:308-380). */
int mp_id_row_precision_cpu_f32(const mp_model* model, const float* q, const float* qd, const float* qdd, int64_t rows,
                                const double* g, const double* Ftip, uint8_t* in_f64, int nthreads);
int mp_fk_jac_id_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* qdd, int64_t rows,
                         const double* g, const double* Ftip, double* T, double* J, double* tau, int nthreads);
int mp_mass_matrix_cpu_f64(const mp_model* model, const double* q, int64_t rows, double* M, int nthreads);
int mp_forward_dynamics_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* tau, int64_t rows,
                                const double* g, const double* Ftip, double* qdd, int nthreads);
int mp_id_derivatives_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* qdd, int64_t rows,
                              const double* g, const double* Ftip, double* tau, double* dtau_dq, double* dtau_dqd, double* M,
                              int nthreads);
int mp_fd_derivatives_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* tau, int64_t rows,
                              const double* g, const double* Ftip, double* qdd, double* dqdd_dq, double* dqdd_dqd, double* Minv,
                              int nthreads);
int mp_id_vjp_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* qdd, const double* gtau, int64_t rows,
                      const double* g, const double* Ftip, double* gq, double* gqd, double* gqdd, int nthreads);
int mp_fd_vjp_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* tau, const double* gqdd, int64_t rows,
                      const double* g, const double* Ftip, double* qdd, double* gq, double* gqd, double* gtau, int nthreads);
int mp_fk_jac_vjp_cpu_f64(const mp_model* model, int frame, const double* q, const double* gT, const double* gJ, int64_t rows,
                          double* T, double* J, double* gq, int nthreads);
int mp_opspace_cpu_f64(const mp_model* model, int frame, int task, double damping, const double* q, const double* qd, int64_t rows,
                       const double* g, double* T, double* J, double* Jdqd, double* Lambda, double* Jbar, double* mu, double* p,
                       int nthreads);
int mp_opspace_torque_cpu_f64(const mp_model* model, int frame, int task, double damping, const double* q, const double* qd,
                              const double* acc, const double* tau0, int64_t rows, const double* g, double* tau, int nthreads);
int mp_fd_trajectory_cpu_f32(const mp_model* model, const float* theta0, const float* dtheta0, const float* taumat,
                             const float* Ftipmat, int64_t B, int64_t N, const double* g, double dt, int intRes, float* pos,
                             float* vel, float* acc, int nthreads);
int mp_id_regressor_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* qdd, int64_t rows, const double* g,
                            const double* Ftip, double* Y, double* tau_ext, int nthreads);
int mp_id_regressor_normal_cpu_f64(const mp_model* model, const double* q, const double* qd, const double* qdd, const double* rhs,
                                   int64_t rows, const double* g, const double* Ftip, double* A, double* b, double* rr, int nthreads);
int mp_ilqr_backward_cpu_f64(const mp_model* model, const double* pos, const double* vel, const double* taumat, const double* xref,
                             const double* wq, const double* wr, const double* wf, const double* reg, int64_t B, int64_t N,
                             const double* g, double dt, double* K, double* k, double* dV, int32_t* status, int nthreads);
int mp_ilqr_rollout_cpu_f64(const mp_model* model, const double* theta0, const double* dtheta0, const double* taumat, const double* pos,
                            const double* vel, const double* K, const double* k, const double* alpha, const double* xref,
                            const double* wq, const double* wr, const double* wf, int64_t A, int64_t B, int64_t N, const double* g,
                            double dt, double* cost, double* opos, double* ovel, double* otau, int nthreads);
int mp_path_dynamics_cpu_f64(const mp_model* model, const double* q, const double* dq, const double* ddq, int64_t rows,
                             const double* velocity_limits, const double* g, const double* Ftip, double* a, double* b, double* c,
                             double* xbar, int nthreads);
int mp_toppra_sweep_cpu_f64(int n, const double* a, const double* b, const double* c, const double* xbar, const double* dq,
                            const double* ddq, const double* torque_limits, const double* acceleration_limits, const double* sd_start,
                            const double* sd_end, int64_t B, int64_t N, double* K, double* x, double* u, double* t, double* duration,
                            int32_t* status, double* qd, double* qdd, double* tau, int nthreads);
int mp_toppra_cpu_f64(const mp_model* model, const double* q, const double* dq, const double* ddq, const double* velocity_limits,
                      const double* torque_limits, const double* acceleration_limits, const double* sd_start, const double* sd_end,
                      int64_t B, int64_t N, const double* g, const double* Ftip, double* K, double* x, double* u, double* t,
                      double* duration, int32_t* status, double* qd, double* qdd, double* tau, int nthreads);
int mp_fd_trajectory_vjp_cpu_f64(const mp_model* model, const double* theta0, const double* dtheta0, const double* taumat,
                                 const double* Ftipmat, int64_t B, int64_t N, const double* g, double dt, int intRes, const double* gpos,
                                 const double* gvel, const double* gacc, double* gtheta0, double* gdtheta0, double* gtaumat,
                                 int nthreads);
int mp_fd_trajectory_cpu_f64(const mp_model* model, const double* theta0, const double* dtheta0, const double* taumat,
                             const double* Ftipmat, int64_t B, int64_t N, const double* g, double dt, int intRes, float* pos,
                             float* vel, float* acc, int nthreads);
/* Batched inverse kinematics on the host: the iteration of mp_inverse_kinematics_f64 (reference kinematics/ik.py:39-311), one
 * problem after the other per thread; same arguments and results as mp_inverse_kinematics_host_f64. */
int mp_inverse_kinematics_cpu_f64(const mp_model* model, const double* T_desired, const double* theta0, int64_t B,
                                  const double* joint_limits, double eomg, double ev, int max_iterations, double damping,
                                  double step_cap, double weight_orientation, double weight_position, int adaptive_tuning,
                                  int backtracking, uint32_t seed, double* theta, int32_t* success, int32_t* iterations,
                                  int32_t* restarts, int nthreads);
int mp_cartesian_trajectory_cpu_f32(const double* Xstart, const double* Xend, int64_t B, int64_t N, double Tf, int method,
                                    float* pos, float* vel, float* acc, float* orient, int nthreads);
int mp_pd_regulation_cpu_f64(const mp_model* model, const double* theta0, const double* theta_des, const double* Kp, const double* Kd,
                             int64_t K, const double* g, double dt, int steps, double* errors, int32_t* count, int nthreads);

/* ---- sphere-model collision distances, cost and gradients (float64, models of 1..8 joints - MP_ERR_UNSUPPORTED above that;
 * csrc/mp_collision.h).  No counterpart in this ABI's reference interface, whose collision checker has no geometry.
 * Robot spheres: S of them (1..64), each with a link index k in 0..n (0 = the fixed base; link k moves with joints 1..k), a radius > 0
 *   and a centre c given in the SPACE frame at the home configuration q = 0: its world centre at q is prod_{j<=k} exp([S_j] q_j) c.
 *   mp_collision_create turns the centres into link-local coordinates of the compiled frames and sorts the spheres by link; every
 *   index it reports is the caller's.  Self pairs: P >= 0 pairs (a, b) of caller indices, a != b.
 * World obstacles: O >= 0 rows of a kind and 16 doubles (unused ones are ignored), kept in device memory with their count:
 *     MP_OBSTACLE_SPHERE   c[3], r                      sd(p) = |p - c| - r
 *     MP_OBSTACLE_CAPSULE  p0[3], p1[3], r              sd(p) = |p - closest point of the segment| - r;  p0 = p1 is a sphere
 *     MP_OBSTACLE_BOX      c[3], R[9] row-major, h[3]   columns of R = the box axes in the world, l = R^T (p - c), q_i = |l_i| - h_i:
 *                          outside (some q_i > 0) sd = |max(q, 0)|, direction R (sign(l_i) max(q_i, 0)) / sd; otherwise sd = max_i q_i <= 0
 *                          with the direction R (sign(l_i) e_i) of the nearest face i, ties to the lowest axis; sign(0) = +
 *   sd is negative inside; the direction n is the outward unit vector d sd / d p; it is 0 where its length would be below 1e-300
 *   (coincident centres, a point on a capsule's axis or segment).  r and h may be 0, not negative.
 * Per row (every output may be NULL; the host forms need at least one):
 *     dist_world (rows)        min over (sphere s on a link >= 1, obstacle o) of d_so = sd_o(p_s) - r_s; +inf if there is none
 *     arg_world (rows,2) int32 that (sphere, obstacle), or (-1, -1); of equal minima the first in (link, caller index), then obstacle order
 *     dist_self (rows)         min over the pairs of d_ab = |p_a - p_b| - r_a - r_b; +inf without pairs;  arg_self (rows,2) = (a, b) of
 *                              the first such pair, or (-1, -1)
 *     grad_dist_world, grad_dist_self (rows,n)   d dist / d q = n^T J_p(q) at the witness (for a pair, of p_a minus of p_b, n the
 *                              direction from b to a), zero columns beyond the witness's link; zeros without a witness
 *     cost (rows)              sum_{s on a link >= 1, o} phi(d_so; eps_world) + sum_pairs phi(d_ab; eps_self), the CHOMP hinge
 *                              phi = -d + eps/2 (d < 0), (d - eps)^2 / (2 eps) (0 <= d < eps), 0 beyond: C1; eps_* > 0 and finite
 *     grad (rows,n)            d cost / d q.  With F = phi'(d) n (+F on a, -F on b for a pair) and the space-frame wrench of link k
 *                              W_k = [sum p x F; sum F]:  grad_j = J_s,j . sum_{k >= j} W_k, one sweep from the tip
 *   The base's spheres (link 0) meet the world in no output: they are constants of q; they take part in the pairs.
 *   A row with a non-finite q has NaN in every float output and -1 in the indices; other rows are untouched.
 * mp_collision_create validates and copies the tables: S outside 1..64, a link outside 0..n, a radius that is not positive and finite,
 *   a non-finite centre, a pair index outside 0..S-1 or a == b are MP_ERR_INVALID with a message.  The handle belongs to the model's
 *   joint count, not to a context; mp_collision_destroy releases it and its device tables (no launch that uses it may be in flight).
 * mp_collision_set_world(ctx, h, O, kind, params): kind (O) int32, params (O,16) host arrays.  An unknown kind, a non-finite or negative
 *   parameter that the kind uses, or a box R with |R^T R - 1| > 1e-9 is MP_ERR_INVALID and leaves the previous world in place.  The
 *   table is copied to the context's device behind the launches already on its compute stream and the call returns when the copy is
 *   done; launches made afterwards - replays of a graph captured earlier included, as long as O does not outgrow the table's capacity
 *   (it grows in steps of 64 obstacles; a replaced table stays allocated until the handle is destroyed) - see the new world.  The robot's
 *   tables are not rebuilt.  ctx = NULL sets the world of the _cpu twin only; a handle that no call has given a world has O = 0.  Not
 *   allowed during a capture.
 * Point cloud (csrc/mp_cloud.h): M points x_i with one common radius r_c >= 0 and a truncation distance d_max > 0.  It counts as ONE
 *   obstacle, appended after the O primitives, for every entry that takes the handle (the edge check and the planners included):
 *     sd_cloud(p) = min( d_max , min_i |p - x_i| - r_c )
 *   the exact signed distance to the union of the M balls, cut off at d_max.  It is >= -r_c and 1-Lipschitz, so it never overstates the
 *   true distance and conservative advancement stays sound with it; far from the cloud a step is limited by d_max, the knob.
 *   The direction n is the unit vector from the nearest point to p; it is 0 where the value is the truncated one or the two coincide
 *   (length below 1e-300).  Witness: the obstacle member of arg_world (and of the edge check's witness) is O + i for the caller's point
 *   i, O + M where the cloud's value is the truncated one; -1 keeps meaning that there is no candidate at all.  Of equal minima the first
 *   in (link, caller sphere index), then obstacle order stays: the cloud's points come after the primitives in the caller's index order
 *   (of equally near points the lowest index, whatever the grid stores or visits), the truncated value last (|p - x_i| - r_c = d_max is
 *   point i; a point within an ulp or so of that distance may be reported either way - the value is d_max in both cases).  Cost: ONE hinge term per (sphere on a link >= 1, cloud), phi(sd_cloud(p_s) - r_s; eps_world), not one per point, with the
 *   gradient phi' n (zero where truncated); it is the exact cost of the union of balls whenever d_max >= eps_world + max_s r_s.  Edge
 *   check: the cloud's d enters its link's smallest distance and the witness exactly as a primitive's does.  The base's spheres do not
 *   meet the cloud.
 * mp_collision_set_cloud(ctx, h, M, points, radius, d_max, cell): points (M,3) host array; M = 0 removes the cloud; cell <= 0 selects
 *   the default d_max + radius.  The points are sorted into a uniform grid of edge `cell` over their bounding box (float64 positions,
 *   the caller's index beside each); a query visits the (2 R + 1)^3 cells around p, R = ceil((d_max + radius) / cell), which must be
 *   1..4.  A non-finite point, a negative or non-finite radius, d_max not positive and finite, R outside 1..4, M above 2^24 or a grid of
 *   more than 2^22 cells ("raise cell") is MP_ERR_INVALID with a message and leaves the previous cloud in place.  Otherwise as
 *   mp_collision_set_world: the image is copied behind the launches already on the compute stream, the call returns when the copy is
 *   done, a replaced device buffer stays allocated until the handle is destroyed, ctx = NULL sets the _cpu twin's copy only, not allowed
 *   during a capture; the two calls never disturb each other.  Launches on a handle with a cloud run kernel instances of their own
 *   (without one, the code is what it was before clouds existed): a graph captured while a cloud was set sees every later cloud when
 *   replayed, one captured without a cloud keeps running without.
 * mp_collision_cloud_info(h, &M, &radius, &d_max, &cell, dims): the cloud's count (0: none), parameters and grid dimensions (3 int32);
 *   any output may be NULL.
 * mp_collision_f64: d_q (rows,n) device rows, 16-byte aligned like every output.  Asynchronous, no synchronisation; it allocates nothing
 *   once the handle is resident on the context (its first mp_collision_set_world, mp_collision_f64 or _host_f64 there makes it so),
 *   and may then be captured into a launch graph.  mp_collision_host_f64: host arrays, device memory from the context's pool.
 *   mp_collision_cpu_f64: the kernel's per-row code on the host, no context. */
#define MP_OBSTACLE_SPHERE 0
#define MP_OBSTACLE_CAPSULE 1
#define MP_OBSTACLE_BOX 2
#define MP_COLLISION_MAX_SPHERES 64
typedef struct mp_collision mp_collision;
int mp_collision_create(const mp_model* model, int S, const int32_t* link, const double* centre, const double* radius, int P,
                        const int32_t* pairs, mp_collision** out);
int mp_collision_destroy(mp_collision* h);
int mp_collision_set_world(mp_ctx* ctx, mp_collision* h, int O, const int32_t* kind, const double* params);
int mp_collision_set_cloud(mp_ctx* ctx, mp_collision* h, int64_t M, const double* points, double radius, double d_max, double cell);
int mp_collision_cloud_info(const mp_collision* h, int64_t* M, double* radius, double* d_max, double* cell, int32_t* dims);
int mp_collision_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_q, int64_t rows, double eps_world,
                     double eps_self, double* d_dist_world, int32_t* d_arg_world, double* d_dist_self, int32_t* d_arg_self,
                     double* d_grad_dist_world, double* d_grad_dist_self, double* d_cost, double* d_grad);
int mp_collision_host_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* q, int64_t rows, double eps_world,
                          double eps_self, double* dist_world, int32_t* arg_world, double* dist_self, int32_t* arg_self,
                          double* grad_dist_world, double* grad_dist_self, double* cost, double* grad);
int mp_collision_cpu_f64(const mp_model* model, const mp_collision* h, const double* q, int64_t rows, double eps_world, double eps_self,
                         double* dist_world, int32_t* arg_world, double* dist_self, int32_t* arg_self, double* grad_dist_world,
                         double* grad_dist_self, double* cost, double* grad, int nthreads);

/* ---- continuous collision checking of joint-space edges by conservative advancement (float64, models of 1..8 joints -
 * MP_ERR_UNSUPPORTED above that; csrc/mp_collision.h).  Is the straight motion from q_a to q_b free under the sphere model above, and
 * if not, where does it stop?  The answer is a proof over the whole interval, not a sample.
 * Edge e: q(t) = q_a + t D, D = q_b - q_a, t in [0, 1].  Candidates are those of mp_collision_f64: (sphere on a link >= 1, obstacle)
 *   with d_so, and the self pairs with d_ab.  The clearance of a candidate is c = d - margin.
 * Motion bounds, fixed at mp_collision_create (joints are 1-based; link k moves with joints 1..k):
 *   anchor A_j of a revolute joint = the point of its axis nearest the origin at home, w_j x v_j of its unit screw (w_j, v_j);
 *   r_j(c), for a sphere centre c on link k and a revolute joint j <= k = the length of the polyline c -> A_i1 -> A_i2 -> ... -> A_j
 *     through the anchors of the revolute joints i with j < i <= k in descending order (a rotation about axis i keeps the distance
 *     to a point of that axis, so this bounds the distance from c to axis j in every configuration);
 *   rho[j][k] = max of r_j(c) over the spheres of link k; 0 if the link has none, if k < j, or if joint j is prismatic.
 *   mp_collision_motion_bounds(h, rho) copies the table: rho (n, n + 1) row-major, row j - 1, column k = 0..n.
 * Per edge: a prismatic joint i between them (j < i <= k) lengthens the polyline by at most |q_i|:
 *     e[j][k] = sum over the prismatic i, j < i <= k, of max(|q_a,i|, |q_b,i|)
 *   The speed of link kb relative to link ka (0 <= ka < kb <= n) per unit t is at most
 *     L[ka][kb] = sum_{j = ka+1..kb} |D_j| w_j,   w_j = rho[j][kb] + e[j][kb] (revolute j),  1 (prismatic j)
 *   A world candidate on link k uses L[0][k]; a pair on links ka < kb uses L[ka][kb] (their distance is frame-invariant: only the
 *   joints between them count); a pair on one link uses 0.  All three obstacle kinds' sd are 1-Lipschitz, so every candidate
 *   satisfies d(t') >= d(t) - L (t' - t).
 * Iteration: t_0 = 0.  At t_i every candidate is evaluated: c_i = min c, tau_i = min c / L over the candidates (L = 0 contributes
 *   +inf); `steps` counts the evaluations.  c_i <= tol: BLOCKED, t = t_i.  Otherwise t_i + tau_i >= 1: FREE, t = 1 (the last
 *   interval, end point included, is proven without evaluating it).  Otherwise t_{i+1} = t_i + tau_i.  After max_steps evaluations
 *   without a decision: UNDECIDED, t = the last t_i - proven: clearance > margin on [0, t).
 * Per edge (every output may be NULL; the host forms need at least one):
 *     status (edges) int32     MP_EDGE_FREE 0, MP_EDGE_BLOCKED 1, MP_EDGE_UNDECIDED 2, MP_EDGE_INVALID -1
 *     t (edges), steps (edges) int32
 *     clearance (edges)        the smallest min(dist_world, dist_self) over the evaluated configurations; +inf without candidates
 *     witness (edges,3) int32  (0 world | 1 self, i, j) of that value, in the caller's indices: (0, sphere, obstacle) or (1, a, b).
 *                              Ties within world or within self resolve as arg_world / arg_self above; a world and a self candidate
 *                              of equal clearance: world; equal minima across evaluated configurations: the first evaluated.
 *                              (-1, -1, -1) without candidates
 *   A non-finite q_a or q_b gives MP_EDGE_INVALID with NaN in t and clearance, 0 steps and a -1 witness; other edges are untouched.
 *   D = 0 gives one step: FREE or BLOCKED at 0.  No obstacles and no pairs: FREE in one step.
 *   margin must be finite, tol positive and finite, max_steps in 1..65536: anything else is MP_ERR_INVALID with a message.
 * mp_collision_edges_f64: d_q_from, d_q_to (edges,n) device rows, 16-byte aligned like every output.  One launch: the edges are
 *   handed to the resident lanes through a queue (iteration counts differ widely between neighbouring edges), so the order in which
 *   they are processed is not the order of the arrays; every edge's outputs depend on that edge alone.  max_blocks > 0 caps the grid
 *   (0: as many one-wave blocks as the device keeps resident, at most ceil(edges / 64)).  Asynchronous, no synchronisation; it
 *   allocates nothing once the handle is resident on the context and may then be captured into a launch graph (the queue head's reset
 *   is part of it).  mp_collision_edges_host_f64: host arrays, device memory from the context's pool.
 *   mp_collision_edges_cpu_f64: the kernel's per-edge code on the host, no context. */
#define MP_EDGE_FREE 0
#define MP_EDGE_BLOCKED 1
#define MP_EDGE_UNDECIDED 2
#define MP_EDGE_INVALID (-1)
int mp_collision_motion_bounds(const mp_collision* h, double* rho);
int mp_collision_edges_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_q_from, const double* d_q_to, int64_t edges,
                           double margin, double tol, int max_steps, int max_blocks, int32_t* d_status, double* d_t, int32_t* d_steps,
                           double* d_clearance, int32_t* d_witness);
int mp_collision_edges_host_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* q_from, const double* q_to, int64_t edges,
                                double margin, double tol, int max_steps, int32_t* status, double* t, int32_t* steps, double* clearance,
                                int32_t* witness);
int mp_collision_edges_cpu_f64(const mp_model* model, const mp_collision* h, const double* q_from, const double* q_to, int64_t edges,
                               double margin, double tol, int max_steps, int32_t* status, double* t, int32_t* steps, double* clearance,
                               int32_t* witness, int nthreads);

/* ---- batched RRT-Connect over the sphere model above (float64, models of 1..8 joints - MP_ERR_UNSUPPORTED above that;
 * csrc/mp_rrt.h).  Bidirectional RRT-Connect (Kuffner and LaValle) for B independent problems in one world: every tree edge is proven
 * free over its whole length by the conservative advancement of mp_collision_edges_*, with the launch's margin, tol and max_steps.
 * The kernel, the CPU twin and the tests' NumPy oracle implement exactly the contract below.
 * Per problem: q_start, q_goal (n).  Per launch: the sampling box lo, hi (n each, HOST arrays, finite, lo <= hi), seed (uint32),
 *   step > 0, min_advance >= 0 (both finite), max_iters >= 0, max_nodes in 2..65536 (per tree), max_waypoints >= 2, and margin, tol,
 *   max_steps as for the edges.  Anything else is MP_ERR_INVALID with a message.
 * Random numbers: key = the FNV-1a hash (offset 0xCBF29CE484222325, prime 0x100000001B3) over the 64-bit patterns of
 *   q_start[0..n) then q_goal[0..n).  u(k, j): x = seed * 0x9E3779B97F4A7C15 + key * 0xBF58476D1CE4E5B9 +
 *   (k * 64 + j) * 0x94D049BB133111EB (64-bit, wrapping); x += 0x9E3779B97F4A7C15; z = x; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *   z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^= z >> 31; u = (z >> 11) * 2^-53.  q_rand_j(k) = lo_j + u(k, j) (hi_j - lo_j).
 *   A problem's result depends on its own content and the seed only - not on its row, its lane or the launch.
 * Trees: T[0] is rooted at q_start, T[1] at q_goal; a tree holds nodes (n doubles) and a parent index each (root: -1).
 *   nearest(T, q): the node with the smallest d2 = sum_j (x_j - q_j)^2, summed over j ascending; of equal d2 the lowest index.
 *     d = sqrt(d2).
 *   edge(a -> b): one edge check of the section above, D = b - a: status, t, steps.
 *   Partial node: after an edge from node i that is not FREE (BLOCKED or UNDECIDED at t: [0, t) is proven), with l the edge's
 *     joint-space length as given below: if (t / 2) l >= min_advance, a + (t / 2) D is appended with parent i; otherwise nothing.
 * Procedure:
 *   A non-finite q_start or q_goal: INVALID, nothing is evaluated.
 *   edge(q_start -> q_start) not FREE: START_BLOCKED.  Then edge(q_goal -> q_goal) not FREE: GOAL_BLOCKED.
 *   a = 0, k = 0; loop:
 *     if k >= 1 and k >= max_iters: EXHAUSTED (the direct attempt at k = 0 is always made, so max_iters = 0 behaves as 1).
 *     if either tree holds max_nodes nodes: TREE_FULL.
 *     EXTEND (k >= 1; at k = 0 it is skipped and new = the root of T[a]: the direct motion between start and goal comes first):
 *       i, d = nearest(T[a], q_rand(k)).  d == 0: trapped.  Otherwise the target is q_rand itself if d <= step, else
 *       x_i + (step / d) (q_rand - x_i); l = min(d, step).  edge(x_i -> target): FREE appends the target with parent i, otherwise the
 *       partial-node rule applies.  Nothing appended: trapped - k += 1, a ^= 1, continue.  new = the appended node.
 *     CONNECT: i2, d = nearest(T[1 - a], x_new), l = d.  edge(y_i2 -> x_new) over its whole length: FREE is SOLVED, otherwise the
 *       partial-node rule applies to T[1 - a].
 *     k += 1, a ^= 1.
 *   SOLVED: the path is root0 .. new, i2 .. root1 (a = 0) or root0 .. i2, new .. root1 (a = 1).  More than max_waypoints points:
 *     PATH_TOO_LONG, and count is the number needed.
 * Per problem (every output may be NULL; at least one is needed):
 *     status (B) int32                   MP_PLAN_SOLVED 0, _EXHAUSTED 1, _TREE_FULL 2, _START_BLOCKED 3, _GOAL_BLOCKED 4,
 *                                        _PATH_TOO_LONG 5, _INVALID -1
 *     count (B) int32                    the waypoints of the path (SOLVED), the number needed (PATH_TOO_LONG), 0 otherwise
 *     waypoints (B, max_waypoints, n)    the path, padded by repeating the last waypoint (the array can go straight into a check of
 *                                        its segments: a repeated point is a zero edge); NaN rows unless SOLVED
 *     iterations (B) int32               k at the end
 *     nodes (B, 2) int32                 the sizes of T[0], T[1] at the end (1, 1 for START_ / GOAL_BLOCKED; 0, 0 for INVALID)
 *     evaluations (B) int32              the configurations evaluated, the two end-point checks included (0 for INVALID)
 * mp_rrt_connect_f64: d_q_start, d_q_goal (B,n) device rows, 16-byte aligned like every output and the workspace.  One launch: a
 *   lane serves one problem at a time and takes problems from a queue, so the launch lasts as long as its slowest problem - max_iters
 *   is the latency knob.  The trees live in d_workspace and belong to the resident lane: mp_rrt_connect_workspace_bytes(n, max_nodes,
 *   blocks) = blocks x 64 lanes x 2 max_nodes (8 n + 4) bytes (or minus an MP_ERR_* code).  The grid is the smallest of the one-wave
 *   blocks the device keeps resident, ceil(B / 64), max_blocks (if positive) and the blocks the workspace holds; room for less than
 *   one block is MP_ERR_INVALID.  Asynchronous; it allocates nothing once the handle is resident on the context and may then be
 *   captured into a launch graph.  Launches that share a collision handle share its queue head: they are serialised by the handle's
 *   lock and the compute stream.  mp_rrt_connect_host_f64: host arrays, device memory and workspace from the context's pool.
 *   mp_rrt_connect_cpu_f64: the kernel's per-problem code on the host, no context. */
#define MP_PLAN_SOLVED 0
#define MP_PLAN_EXHAUSTED 1
#define MP_PLAN_TREE_FULL 2
#define MP_PLAN_START_BLOCKED 3
#define MP_PLAN_GOAL_BLOCKED 4
#define MP_PLAN_PATH_TOO_LONG 5
#define MP_PLAN_INVALID (-1)
int64_t mp_rrt_connect_workspace_bytes(int n, int max_nodes, int blocks);
int mp_rrt_connect_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_q_start, const double* d_q_goal, int64_t B,
                       const double* lo, const double* hi, uint32_t seed, double step, double min_advance, int max_iters, int max_nodes,
                       int max_waypoints, double margin, double tol, int max_steps, void* d_workspace, size_t workspace_bytes,
                       int max_blocks, int32_t* d_status, int32_t* d_count, double* d_waypoints, int32_t* d_iterations, int32_t* d_nodes,
                       int32_t* d_evaluations);
int mp_rrt_connect_host_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* q_start, const double* q_goal, int64_t B,
                            const double* lo, const double* hi, uint32_t seed, double step, double min_advance, int max_iters,
                            int max_nodes, int max_waypoints, double margin, double tol, int max_steps, int32_t* status, int32_t* count,
                            double* waypoints, int32_t* iterations, int32_t* nodes, int32_t* evaluations);
int mp_rrt_connect_cpu_f64(const mp_model* model, const mp_collision* h, const double* q_start, const double* q_goal, int64_t B,
                           const double* lo, const double* hi, uint32_t seed, double step, double min_advance, int max_iters,
                           int max_nodes, int max_waypoints, double margin, double tol, int max_steps, int32_t* status, int32_t* count,
                           double* waypoints, int32_t* iterations, int32_t* nodes, int32_t* evaluations, int nthreads);

/* ---- batched path shortcutting over the sphere model above (float64, models of 1..8 joints - MP_ERR_UNSUPPORTED above that;
 * csrc/mp_shortcut.h).  Randomised shortcutting (Geraerts and Overmars; Hauser and Ng-Thow-Hing) of B piecewise-linear joint-space
 * paths in one world: two points are drawn on the path by arc length, the straight motion between them is proven free by the
 * conservative advancement of mp_collision_edges_*, with the launch's margin, tol and max_steps, and if it is free it replaces the
 * piece of path between them.  The kernel, the CPU twin and the tests' NumPy oracle implement exactly the contract below.
 * Per problem: waypoints_in (W_in, n) and count_in.  The first count_in rows are the path p_0 .. p_{m-1}; the rest is ignored, so a
 *   planner's padded `waypoints` and its `count` go straight in.  Per launch: W_in in 1..65536, seed (uint32), max_iters >= 0,
 *   min_gain >= 0 and finite, max_waypoints in 2..65536 (the output rows W), and margin, tol, max_steps as for the edges.  Anything
 *   else is MP_ERR_INVALID with a message.
 * Start of a problem: count_in < 2: SKIPPED (a planner row that was not SOLVED has count 0).  count_in > W_in, count_in >
 *   max_waypoints, or a non-finite value in the first count_in rows: INVALID.  Neither evaluates anything; both return NaN rows,
 *   count 0, NaN lengths and 0 in the counters.
 * Lengths: c_0 = 0, c_{i+1} = c_i + sqrt(sum_j (p_{i+1,j} - p_{i,j})^2), summed over j ascending; Lambda = c_{m-1}.  The table is
 *   recomputed from scratch, by this same formula, after every accepted shortcut.
 * Random numbers: key = the hash of mp_rrt_connect_* over p_0 then p_{m-1} of the INPUT path; u(k, j) as there, j = 0, 1.  A
 *   problem's result depends on its own content and the seed only - not on its row, its lane or the launch.
 * locate(s): i = the smallest index in 0..m-2 with s < c_{i+1}, m - 2 if there is none (a zero-length segment is never chosen);
 *   lambda = (s - c_i) / (c_{i+1} - c_i); the point is p_i + lambda (p_{i+1} - p_i).
 * Procedure, for k = 0, 1, ..:
 *     m == 2 and (k < max_iters or k == 0): stop, STRAIGHT - a path of two waypoints is STRAIGHT before anything is drawn, whatever
 *       max_iters is, and a path that becomes one ends at the head of the next iteration, if there is one.
 *     k == max_iters: stop, DONE.
 *     s_a = u(k, 0) Lambda, s_b = u(k, 1) Lambda, swapped so that s_a <= s_b; (i, a) = locate(s_a), (j, b) = locate(s_b).
 *     i == j: nothing to gain, next k.
 *     d = sqrt(sum_j (b_j - a_j)^2), gain = (s_b - s_a) - d.  gain <= min_gain: next k, with no edge check.
 *     m' = m - (j - i) + 2.  m' > max_waypoints: skipped_full += 1, next k.
 *     edge(a -> b), one edge check of the section above, D = b - a: FREE: the path becomes p_0 .. p_i, a, a + D, p_{j+1} .. p_{m-1}
 *       (a + D, the end of the motion a + t D that the check has proven, is b to within an ulp), m = m', the lengths are recomputed,
 *       accepted += 1.  BLOCKED or UNDECIDED: nothing changes.  Next k.
 * What is proven: every segment the procedure creates is proven FREE; pieces of input segments are kept as they are, so the output is
 *   as free as the input.  THE INPUT IS NOT CHECKED: validate it (mp_collision_edges_* over its segments, batch_validate_path in
 *   Python) if it does not come from mp_rrt_connect_* under the same margin.  The output starts at p_0 and ends at p_{m-1} of the
 *   input bit for bit.
 * Per problem (every output may be NULL; at least one is needed):
 *     status (B) int32                   MP_SHORTCUT_DONE 0, _STRAIGHT 1, _SKIPPED 2, _INVALID -1
 *     count (B) int32                    the waypoints of the output path (0 for SKIPPED and INVALID)
 *     waypoints (B, max_waypoints, n)    the path, padded by repeating the last waypoint as the planner pads; must not overlap
 *                                        waypoints_in
 *     length_in, length_out (B)          Lambda of the input path and of the output path
 *     iterations (B) int32               k at the end
 *     accepted, skipped_full (B) int32
 *     evaluations (B) int32              the configurations evaluated
 * mp_path_shortcut_f64: d_waypoints_in (B,W_in,n), d_count_in (B) int32 device arrays, 16-byte aligned like every output and the
 *   workspace.  One launch: a lane serves one problem at a time and takes problems from a queue.  The working paths live in
 *   d_workspace and belong to the resident lane: mp_path_shortcut_workspace_bytes(n, max_waypoints, blocks) = blocks x 64 lanes x
 *   max_waypoints (8 n + 8) bytes (or minus an MP_ERR_* code).  The grid is the smallest of the one-wave blocks the device keeps
 *   resident, ceil(B / 64), max_blocks (if positive) and the blocks the workspace holds; room for less than one block is
 *   MP_ERR_INVALID.  Asynchronous; it allocates nothing once the handle is resident on the context and may then be captured into a
 *   launch graph (the queue head's reset is part of it).  Launches that share a collision handle share its queue head: they are
 *   serialised by the handle's lock and the compute stream.  mp_path_shortcut_host_f64: host arrays, device memory and workspace
 *   from the context's pool.  mp_path_shortcut_cpu_f64: the kernel's per-problem code on the host, no context. */
#define MP_SHORTCUT_DONE 0
#define MP_SHORTCUT_STRAIGHT 1
#define MP_SHORTCUT_SKIPPED 2
#define MP_SHORTCUT_INVALID (-1)
int64_t mp_path_shortcut_workspace_bytes(int n, int max_waypoints, int blocks);
int mp_path_shortcut_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_waypoints_in, const int32_t* d_count_in,
                         int64_t B, int64_t W_in, uint32_t seed, int max_iters, double min_gain, int max_waypoints, double margin,
                         double tol, int max_steps, void* d_workspace, size_t workspace_bytes, int max_blocks, int32_t* d_status,
                         int32_t* d_count, double* d_waypoints, double* d_length_in, double* d_length_out, int32_t* d_iterations,
                         int32_t* d_accepted, int32_t* d_skipped_full, int32_t* d_evaluations);
int mp_path_shortcut_host_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* waypoints_in, const int32_t* count_in,
                              int64_t B, int64_t W_in, uint32_t seed, int max_iters, double min_gain, int max_waypoints, double margin,
                              double tol, int max_steps, int32_t* status, int32_t* count, double* waypoints, double* length_in,
                              double* length_out, int32_t* iterations, int32_t* accepted, int32_t* skipped_full, int32_t* evaluations);
int mp_path_shortcut_cpu_f64(const mp_model* model, const mp_collision* h, const double* waypoints_in, const int32_t* count_in, int64_t B,
                             int64_t W_in, uint32_t seed, int max_iters, double min_gain, int max_waypoints, double margin, double tol,
                             int max_steps, int32_t* status, int32_t* count, double* waypoints, double* length_in, double* length_out,
                             int32_t* iterations, int32_t* accepted, int32_t* skipped_full, int32_t* evaluations, int nthreads);

/* ---- collision-free goal configurations for pose goals over the sphere model above (float64, models of 1..8 joints -
 * MP_ERR_UNSUPPORTED above that; generic kernels only, no run-time specialisation; csrc/mp_goal.h).  For B independent end-effector
 * poses in one world: a joint configuration inside a box that reaches the pose and that the planner accepts as a goal.  Damped
 * Newton attempts from the caller's seed and then from random points of the box; every attempt that reaches the pose gets the
 * zero-edge decision mp_rrt_connect_* makes for its q_goal, and the first FREE one is the answer.  This is not
 * mp_inverse_kinematics_*: no best-point restarts, no adaptive damping, and the step is taken on the hybrid Jacobian.  The kernel,
 * the CPU twin and the tests' NumPy oracle implement exactly the contract below.
 * Per problem: T_goal, 16 doubles row-major of which only entries 0..11 are read (as mp_inverse_kinematics_* reads a pose), and
 *   q_seed (n).  Per launch: the box lo, hi (n each, HOST arrays, finite, lo <= hi), seed (uint32), eomg, ev, damping, step_cap (all
 *   finite and > 0), max_iters >= 0, max_attempts in 1..65536, and margin, tol with the meaning they have for the edges.  Anything
 *   else is MP_ERR_INVALID with a message.
 * Random numbers: u(k, j) of mp_rrt_connect_*, with key = the FNV-1a hash (the same offset and prime) over the 64-bit patterns of
 *   T_goal[0..12) then q_seed[0..n), and k the attempt number.  A problem's result depends on its own content and the seed only -
 *   not on its row, its lane or the launch.
 * Procedure:
 *   A non-finite value among T_goal[0..12) or q_seed: INVALID, nothing is evaluated.
 *   For attempt a = 0 .. max_attempts - 1:
 *     theta_j = clamp(q_seed_j, lo_j, hi_j) for a = 0; theta_j = lo_j + u(a, j) (hi_j - lo_j) for a >= 1.
 *     For k = 0 .. max_iters:
 *       T_c and the space Jacobian J_s at theta (the FK and Jacobian of mp_fk_jac_id_*); e = [angular error in space axes;
 *         p_goal - p_c], rot = the rotation angle and tr = |p_goal - p_c|, exactly as mp_inverse_kinematics_* measures them.
 *       rot < eomg and tr < ev: the attempt has converged; leave the loop.
 *       k == max_iters: the attempt has failed; leave the loop.
 *       Otherwise one damped Newton step on the HYBRID Jacobian J_h, the proper pair of e: rows 0..2 are those of J_s, column i of
 *         rows 3..5 is v_i + w_i x p_c (p_c the translation of T_c).  A = J_h J_h^T + damping^2 1 (each entry summed over the joints
 *         ascending, the diagonal starting from damping^2), y = A^-1 e by Cholesky, d = J_h^T y; if |d| > step_cap then
 *         d <- d (step_cap / |d|); theta_j <- clamp(theta_j + d_j, lo_j, hi_j); iterations += 1.
 *     A converged attempt: converged += 1, and ONE evaluation of the zero edge theta -> theta by the edge check of the section
 *       above with the launch's margin and tol (a zero edge is FREE or BLOCKED at its first evaluation).  FREE: FOUND, q = theta,
 *       stop.  Otherwise, if its clearance is strictly larger than the best so far (or it is the first), theta becomes the best.
 *   After the last attempt: a best exists: IN_COLLISION, q = best.  Otherwise UNREACHED.
 * Per problem (every output may be NULL; at least one is needed; a bad row leaves the others untouched):
 *     status (B) int32                   MP_GOAL_FOUND 0, _IN_COLLISION 1, _UNREACHED 2, _INVALID -1
 *     q (B, n)                           the configuration; NaN for UNREACHED and INVALID
 *     attempts (B) int32                 attempts started (0 for INVALID)
 *     iterations (B) int32               steps taken, all attempts together
 *     converged (B) int32                attempts that reached the pose
 *     pose_error (B, 2)                  rot, tr at q; NaN without one
 *     clearance (B), witness (B, 3)      at q, as the zero edge reports them; NaN and -1 without one
 *   q goes straight into mp_rrt_connect_* as q_goal: under the same margin and tol a FOUND row is never GOAL_BLOCKED there (it is
 *   the same decision on the same configuration), an IN_COLLISION row is GOAL_BLOCKED, UNREACHED and INVALID rows are MP_PLAN_INVALID.
 * mp_goal_ik_f64: d_T_goal (B,16), d_q_seed (B,n) device rows, 16-byte aligned like every output.  One launch: a lane serves one
 *   problem at a time and takes problems from a queue; a trip of the wave is one pose evaluation with its step and, only when a lane
 *   has just converged, one collision evaluation.  No workspace: a problem's state lives in registers.  The grid is the smallest of
 *   the one-wave blocks the device keeps resident, ceil(B / 64) and max_blocks (if positive).  Asynchronous; it allocates nothing once
 *   the handle is resident on the context and may then be captured into a launch graph (the queue head's reset is part of it).
 *   Launches that share a collision handle share its queue head: they are serialised by the handle's lock and the compute stream.
 *   mp_goal_ik_host_f64: host arrays, device memory from the context's pool.  mp_goal_ik_cpu_f64: the kernel's per-problem code on
 *   the host, no context. */
#define MP_GOAL_FOUND 0
#define MP_GOAL_IN_COLLISION 1
#define MP_GOAL_UNREACHED 2
#define MP_GOAL_INVALID (-1)
int mp_goal_ik_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_T_goal, const double* d_q_seed, int64_t B,
                   const double* lo, const double* hi, uint32_t seed, double eomg, double ev, double damping, double step_cap,
                   int max_iters, int max_attempts, double margin, double tol, int max_blocks, int32_t* d_status, double* d_q,
                   int32_t* d_attempts, int32_t* d_iterations, int32_t* d_converged, double* d_pose_error, double* d_clearance,
                   int32_t* d_witness);
int mp_goal_ik_host_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* T_goal, const double* q_seed, int64_t B,
                        const double* lo, const double* hi, uint32_t seed, double eomg, double ev, double damping, double step_cap,
                        int max_iters, int max_attempts, double margin, double tol, int32_t* status, double* q, int32_t* attempts,
                        int32_t* iterations, int32_t* converged, double* pose_error, double* clearance, int32_t* witness);
int mp_goal_ik_cpu_f64(const mp_model* model, const mp_collision* h, const double* T_goal, const double* q_seed, int64_t B,
                       const double* lo, const double* hi, uint32_t seed, double eomg, double ev, double damping, double step_cap,
                       int max_iters, int max_attempts, double margin, double tol, int32_t* status, double* q, int32_t* attempts,
                       int32_t* iterations, int32_t* converged, double* pose_error, double* clearance, int32_t* witness, int nthreads);

/* ---- batched C2 corner blending of waypoint paths over the sphere model above (float64, models of 1..8 joints - MP_ERR_UNSUPPORTED
 * above that; generic kernels only, no run-time specialisation; csrc/mp_blend.h).  For B piecewise-linear joint-space paths in one
 * world: every interior corner is replaced by a quintic blend that is proven free by the conservative advancement of
 * mp_collision_edges_*, and the resulting twice-differentiable curve is sampled on the uniform grid s_i = i / (N - 1) as q, dq/ds,
 * d2q/ds2 - what mp_toppra_* reads.  No random numbers.  The kernels, the CPU twin and the tests' NumPy oracle implement exactly the
 * contract below; every sum is taken in the order written, j ascending.
 * Per problem: waypoints_in (W_in, n) and count_in, exactly as mp_path_shortcut_* reads them.  Per launch: W_in in 1..65536, N in
 *   3..65536, blend > 0 and finite (the largest cut distance, in the joint-space norm of the shortcutter's lengths), max_halvings in
 *   0..32, and margin, tol, max_steps as for the edges.  Anything else is MP_ERR_INVALID with a message.
 * 1 Screen: count_in < 2: SKIPPED.  count_in > W_in, or a non-finite value in the first count_in rows: INVALID.
 * 2 Compact: r_0 = p_0; p_i is kept iff some component differs, compared as doubles, from the last kept point: m points.
 *   m == 1: POINT - q = r_0 on the whole grid, dq = ddq = 0, length 0.
 * 3 Segments: for i = 1..m-1, D_i = r_i - r_{i-1}, l_i = sqrt(sum_j D_ij^2), u_i = D_i / l_i.  m == 2: STRAIGHT.  Corners are
 *   k = 1..m-2 with u_in = u_k, u_out = u_{k+1}.  The first k with sum_j u_in,j u_out,j < -1 + 1e-9: REVERSAL, corner = k, nothing is
 *   evaluated (a path that doubles back has no C2 blend of non-zero speed).
 * 4 Corners, in ascending order: d = min(blend, l_k / 2, l_{k+1} / 2); up to max_halvings + 1 attempts; an attempt that is not FREE
 *   halves d and adds 1 to `halvings`.  The first FREE attempt sets cut[k] = d.  None: BLOCKED, corner = k, the problem stops.
 *   An attempt is the iteration of mp_collision_edges_* over u in [0, 1], u_0 = 0, on the curve
 *       q(u) = r_k - d u_in (1 - u)^4 (1 + 1.5 u) + d u_out u^4 (2.5 - 1.5 u)
 *   - the quintic Bezier on a, (a + r) / 2, r, r, (r + b) / 2, b with a = r_k - d u_in, b = r_k + d u_out, whose second derivative
 *   vanishes at both ends - with the speed bounds L[ka][kb] of the edges, in which |D_j| is replaced by v_j = 2.5 d max(|u_in,j|,
 *   |u_out,j|) and the reach max(|q_a,j|, |q_b,j|) of a prismatic joint by max(|a_j|, |r_k,j|, |b_j|): both bound the whole curve
 *   (the hodograph's control differences are (r - a) / 2 twice, 0, (b - r) / 2 twice, and the curve lies in the hull of a, r, b).
 *   The decisions are the edge's: c <= tol: BLOCKED; otherwise u + tau >= 1: FREE; max_steps evaluations of one attempt without a
 *   decision: a failed attempt.  The linear pieces are pieces of input segments and ARE NOT CHECKED, as in mp_path_shortcut_*.
 * 5 Parameter sigma: unit speed on linear pieces, and a blend of cut d takes 2.5 d of it (so that dq/dsigma is continuous).  With
 *   cut[0] = cut[m-1] = 0: knot[0] = 0, knot[k] = (knot[k-1] + 2.5 cut[k-1]) + ((l_k - cut[k-1]) - cut[k]) for k = 1..m-1;
 *   knot[m-1] = Sigma, the length.
 * 6 Grid: sigma = (i / (N - 1)) Sigma.  i = 0: r_0, Sigma u_1, 0.  i = N - 1: r_{m-1}, Sigma u_{m-1}, 0.  Otherwise k = the
 *   largest index in 0..m-2 with knot[k] <= sigma.  If k >= 1 and sigma - knot[k] < 2.5 cut[k]: blend k at u = (sigma - knot[k]) /
 *   (2.5 cut[k]): q(u) as above with d = cut[k], dq/ds = Sigma [u_in (1 - u)^3 (1 + 3 u) + u_out u^3 (4 - 3 u)], d2q/ds2 = Sigma^2
 *   4.8 u (1 - u) [u u_out - (1 - u) u_in] / cut[k].  Else the linear piece of segment k + 1: q = r_k + (((cut[k] + sigma) -
 *   knot[k]) - 2.5 cut[k]) u_{k+1}, dq/ds = Sigma u_{k+1}, d2q/ds2 = 0.  All three are continuous across a knot.
 * Per problem (every output may be NULL; at least one is needed):
 *     status (B) int32                   MP_BLEND_DONE 0, _STRAIGHT 1, _SKIPPED 2, _POINT 3, _BLOCKED 4, _REVERSAL 5, _INVALID -1
 *     corner (B) int32                   the first offending corner of the compacted path (BLOCKED, REVERSAL), else -1
 *     count (B) int32                    m
 *     points (B, W_in, n)                the compacted points, padded by repeating the last
 *     cut (B, W_in), knot (B, W_in)      padded with 0 and with Sigma
 *     length (B)                         Sigma
 *     halvings, evaluations (B) int32    failed attempts, configurations evaluated
 *     clearance (B)                      the smallest min(dist_world, dist_self) met in the attempts, +inf without any
 *     q, dq, ddq (B, N, n)               the grid, batch-major
 *   A problem that is not DONE, STRAIGHT or POINT has NaN in every real output and 0 in count; status, corner and the two counters
 *   stay meaningful.  A problem's result depends on its own content only.  points and the grid arrays must not overlap waypoints_in.
 * mp_path_blend_f64: device arrays, 16-byte aligned.  Two launches on the compute stream: the corners - a lane serves one problem at a
 *   time and takes problems from a queue, one collision evaluation a trip, no workspace (a lane reads its own input rows) - and,
 *   if any of q, dq, ddq is given, the grid, one lane a grid point.  The grid reads status, count, points, cut, knot and length
 *   back: all six are then required.  max_blocks > 0 caps the first grid.  Asynchronous; it allocates nothing once the handle is
 *   resident on the context and may then be captured into a launch graph (the queue head's reset is part of it).  Launches that share
 *   a collision handle share its queue head: they are serialised by the handle's lock and the compute stream.
 *   mp_path_blend_host_f64: host arrays, device memory from the context's pool.  mp_path_blend_cpu_f64: the kernels' per-problem and
 *   per-grid-point code on the host, no context. */
#define MP_BLEND_DONE 0
#define MP_BLEND_STRAIGHT 1
#define MP_BLEND_SKIPPED 2
#define MP_BLEND_POINT 3
#define MP_BLEND_BLOCKED 4
#define MP_BLEND_REVERSAL 5
#define MP_BLEND_INVALID (-1)
int mp_path_blend_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_waypoints_in, const int32_t* d_count_in,
                      int64_t B, int64_t W_in, int64_t N, double blend, int max_halvings, double margin, double tol, int max_steps,
                      int max_blocks, int32_t* d_status, int32_t* d_corner, int32_t* d_count, double* d_points, double* d_cut,
                      double* d_knot, double* d_length, int32_t* d_halvings, int32_t* d_evaluations, double* d_clearance, double* d_q,
                      double* d_dq, double* d_ddq);
int mp_path_blend_host_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* waypoints_in, const int32_t* count_in,
                           int64_t B, int64_t W_in, int64_t N, double blend, int max_halvings, double margin, double tol, int max_steps,
                           int32_t* status, int32_t* corner, int32_t* count, double* points, double* cut, double* knot, double* length,
                           int32_t* halvings, int32_t* evaluations, double* clearance, double* q, double* dq, double* ddq);
int mp_path_blend_cpu_f64(const mp_model* model, const mp_collision* h, const double* waypoints_in, const int32_t* count_in, int64_t B,
                          int64_t W_in, int64_t N, double blend, int max_halvings, double margin, double tol, int max_steps,
                          int32_t* status, int32_t* corner, int32_t* count, double* points, double* cut, double* knot, double* length,
                          int32_t* halvings, int32_t* evaluations, double* clearance, double* q, double* dq, double* ddq, int nthreads);

/* ---- batched fixed-rate sampling of time-optimal trajectories (float64, models of 1..8 joints - MP_ERR_UNSUPPORTED above that;
 * generic kernels only, no run-time specialisation; csrc/mp_sample.h).  B timed paths in, B trajectories out whose row k is the
 * time k dt: s, sd, sdd, q, qd, qdd and the full inverse dynamics of the row, on at most M rows a path.  The kernel, the CPU twin
 * and the tests' NumPy oracle implement exactly the contract below.
 * Per path: t (B, N) and x = sd^2 (B, N), batch-major, as mp_toppra_* returns them (t, x) on the grid s_i = i / (N - 1),
 *   D = 1 / (N - 1).  Per launch: N in 3..2^31-1, dt > 0 and finite, M in 1..2^31-1, B M n and B N n below 2^60.  Anything else is
 *   MP_ERR_INVALID with a message.
 * The geometry comes from one of two sources, chosen by which group of pointers is given (both groups, neither, or a group that is
 *   given in part: MP_ERR_INVALID):
 *   grid:  q, dq, ddq (B, N, n), the arrays the parameterisation read.  Between grid points i and i + 1 the path is the quintic
 *     Hermite interpolant in s - the one quintic that matches q, q' and q'' at both ends; it is C2 across grid points and exact for
 *     a path that is a polynomial of degree <= 5 in s on the interval.  At the left end of an interval it is q_i bit for bit.
 *   curve: blend_status, blend_count (B) int32, points (B, W_in, n), cut, knot (B, W_in), length (B): the tables of
 *     mp_path_blend_* (W_in in 1..65536).  The path is that contract's closed-form curve, evaluated at the real parameter
 *     sigma = s Sigma by the formulas of its step 6 with s in the place of i / (N - 1); s <= 0 and s >= 1 are r_0 and r_{m-1} bit for
 *     bit.  The samples lie on the curve whose blends were proven free, not on an interpolant of its grid.
 * 1 Screen, in this order.  NaN anywhere in the path's t or x (a parameterisation status != 0), or (curve) a blend status other than
 *   DONE, STRAIGHT, POINT or a count outside 1..W_in: UNTIMED.  +inf in t (the interior stop the parameterisation allows): STOPS.
 *   t_0 != 0, a t_{i+1} < t_i, a negative or infinite x, (grid) a non-finite value in q, dq, ddq, (curve) a non-finite length, or
 *   T / dt >= 2^31 - 2 (the count would not fit): INVALID.  Such a path has NaN in every real output and 0 in count and needed.
 * 2 T = t_{N-1}.  k_end = the smallest integer k >= 0 with (double)k * dt >= T, computed as k = ceil(T / dt); if k > 0 and
 *   (double)(k - 1) * dt >= T then k - 1, else if (double)k * dt < T then k + 1: a function of the IEEE products alone.
 *   needed = k_end + 1, count = min(needed, M), status OK, or TRUNCATED when needed > M.  needed is always reported.
 * 3 Row k < M, tau_k = (double)k * dt.  tau_k >= T: the HOLD row - s = 1, sd = sdd = 0, q = the path's end point (q_{N-1} / r_{m-1},
 *   bit for bit), qd = qdd = 0: the robot at rest at the end, whatever sd_end the parameterisation was given (a path timed to
 *   arrive with speed still stops here: a controller that runs past the last sample must find a configuration it can hold).
 *   Rows count..M-1 of an OK path are hold rows, as the planner pads a path by repeating its goal.  Otherwise the MOVING row:
 *   i = the largest index in 0..N-2 with t_i <= tau_k (binary search), delta = tau_k - t_i, r = sqrt(x_i),
 *   ubar = (x_{i+1} - x_i) / (2 D), sigma = clamp((r + 0.5 ubar delta) delta, 0, D), s = i / (N - 1) + sigma,
 *   sd = max(r + ubar delta, 0), sdd = ubar; then qd = q'(s) sd, qdd = q'(s) ubar + q''(s) sd^2.  ubar comes from the two x values
 *   and not from the stored u: the forward pass clips x_{i+1}, and only ubar reproduces the stored time stamps
 *   (r + ubar (t_{i+1} - t_i) = sqrt(x_{i+1})).
 * 4 torques = the inverse dynamics of the row at (q, qd, qdd) with the call's g and Ftip (either may be NULL: -9.81 z, no wrench):
 *   one Newton-Euler recursion over the link frames from the row's own sin / cos - not an interpolation of the grid's torques, so
 *   that a limit missed between grid points shows.  Without torques the recursion is not compiled in.
 * Per path (every output may be NULL; at least one is needed):
 *     status (B) int32                   MP_SAMPLE_OK 0, _TRUNCATED 1, _STOPS 2, _UNTIMED 3, _INVALID -1
 *     count, needed (B) int32
 *     s, sd, sdd (B, M)
 *     positions, velocities, accelerations, torques (B, M, n), batch-major
 *   A path's result depends on its own content only.  No output may overlap an input.
 * mp_trajectory_sample_f64: device arrays, 16-byte aligned.  One launch on the compute stream, one lane a row, a path's screen shared
 *   by the lanes of a wave; max_blocks > 0 caps the grid.  Models of 7 and 8 joints, where the fused recursion was measured slower:
 *   the torques come from a second launch, the inverse-dynamics kernel over the rows just written (same contract: the inverse
 *   dynamics of the row).  Asynchronous; allocates nothing and may be captured into a launch graph - except a call for the torques of
 *   a 7- or 8-joint model without all of positions, velocities and accelerations, which takes the missing rows from the context's
 *   pool for the length of the call and is refused inside a capture.
 *   mp_trajectory_sample_host_f64: host arrays, device memory from the context's pool.  mp_trajectory_sample_cpu_f64: the kernel's
 *   per-path and per-row code on the host, no context. */
#define MP_SAMPLE_OK 0
#define MP_SAMPLE_TRUNCATED 1
#define MP_SAMPLE_STOPS 2
#define MP_SAMPLE_UNTIMED 3
#define MP_SAMPLE_INVALID (-1)
int mp_trajectory_sample_f64(mp_ctx* ctx, const mp_model* model, const double* d_t, const double* d_x, int64_t B, int64_t N, const double* d_q,
                             const double* d_dq, const double* d_ddq, const int32_t* d_blend_status, const int32_t* d_blend_count,
                             const double* d_points, const double* d_cut, const double* d_knot, const double* d_length, int64_t W_in,
                             double dt, int64_t M, const double* g, const double* Ftip, int max_blocks, int32_t* d_status,
                             int32_t* d_count, int32_t* d_needed, double* d_s, double* d_sd, double* d_sdd, double* d_positions,
                             double* d_velocities, double* d_accelerations, double* d_torques);
int mp_trajectory_sample_host_f64(mp_ctx* ctx, const mp_model* model, const double* t, const double* x, int64_t B, int64_t N, const double* q,
                                  const double* dq, const double* ddq, const int32_t* blend_status, const int32_t* blend_count,
                                  const double* points, const double* cut, const double* knot, const double* length, int64_t W_in,
                                  double dt, int64_t M, const double* g, const double* Ftip, int32_t* status, int32_t* count,
                                  int32_t* needed, double* s, double* sd, double* sdd, double* positions, double* velocities,
                                  double* accelerations, double* torques);
int mp_trajectory_sample_cpu_f64(const mp_model* model, const double* t, const double* x, int64_t B, int64_t N, const double* q,
                                 const double* dq, const double* ddq, const int32_t* blend_status, const int32_t* blend_count,
                                 const double* points, const double* cut, const double* knot, const double* length, int64_t W_in, double dt,
                                 int64_t M, const double* g, const double* Ftip, int32_t* status, int32_t* count, int32_t* needed,
                                 double* s, double* sd, double* sdd, double* positions, double* velocities, double* accelerations,
                                 double* torques, int nthreads);

/* ---- batched Cartesian straight-line paths over the sphere model above, proven free (float64, models of 3..8 joints; generic
 * kernels only, no run-time specialisation; csrc/mp_cartesian.h).  For B independent problems: from a start configuration the tool
 * travels on a straight line to a goal pose; the joint-space curve that does it comes back as the (q, dq/ds, d2q/ds2) grid that
 * mp_toppra_* reads, and conservative advancement proves the curve the trajectory sampler executes collision-free.  The kernels,
 * the CPU twin and the tests' NumPy oracle implement exactly the contract below.
 * Per problem: q_start (n), T_goal (16, row-major; the last row is not read).  Per launch: the box lo, hi (n, finite, lo <= hi),
 *   the grid size N in 2..65536, task MP_TASK_FULL (6 rows: needs n >= 6) or MP_TASK_POSITION (3 rows, orientation free: needs
 *   n >= 3) - fewer joints than rows is MP_ERR_UNSUPPORTED, as is n > 8 - eomg, ev, damping, max_joint_step positive and finite,
 *   max_iters in 0..65536, and margin, tol, max_steps as for the edges.  Anything else is MP_ERR_INVALID with a message.
 * 1 The line.  T_start = FK(q_start).  V = [omega; v] = the error vector of the goal step (mp_goal_ik_*) between T_start and T_goal:
 *   the rotation vector of R_start^T R_goal in space axes and p_goal - p_start.  The target at s_i = i / (N - 1) is
 *   R(s) = exp([omega] s) R_start (Rodrigues with angle |omega| s about omega / |omega|; the identity when |omega| = 0),
 *   p(s) = p_start + s v.  POSITION uses p(s) and v alone.  A non-finite value in q_start or T_goal, or (FULL) a rotation angle of
 *   R_start^T R_goal at or above pi - 1e-6 (no unique geodesic): INVALID.
 * 2 Tracking, grid point by grid point; J_h = the task's rows of the hybrid Jacobian (angular rows first), h = 1 / (N - 1).
 *   Row 0 is q_start bit for bit, with no Newton step.  Point i >= 1 starts from the predictor q_{i-1} + h dq_{i-1} and makes at most
 *   max_iters steps q <- q + J_h^T (J_h J_h^T + damping^2 1)^-1 e, e = the same error vector between FK(q) and the target, not clamped
 *   into the box; it has converged when rot < eomg && tr < ev (POSITION: tr < ev), tested before every step.  At every accepted
 *   point, row 0 included: dq = J_h^T (J_h J_h^T)^-1 V and ddq = -J_h^T (J_h J_h^T)^-1 (Jdot_h dq), undamped and minimum-norm, so
 *   that J_h dq = V along the whole line.  The first failing decision ends the problem, in this order at each point:
 *     not converged after max_iters steps                                  STALLED
 *     the converged q outside [lo, hi]                                     LIMIT (at index 0 when q_start itself is outside)
 *     max_j |q_i - q_{i-1}| > max_joint_step                               JUMP (a branch flip near a singularity)
 *     a pivot d of the Cholesky factor of J_h J_h^T with d <= 2^-46 A_jj   SINGULAR
 *   reached = the number of accepted grid points; rows reached..N-1 of q, dq, ddq are NaN.
 * 3 Proof.  The curve is the quintic Hermite interpolant of the grid rows, the one mp_trajectory_sample_* evaluates for a grid
 *   source, through the same function.  Span i (s_i..s_{i+1}, u in [0, 1]) is the quintic Bezier curve on
 *     P0 = q_i, P1 = P0 + h dq_i / 5, P2 = P0 + 2 h dq_i / 5 + h^2 ddq_i / 20,
 *     P5 = q_{i+1}, P4 = P5 - h dq_{i+1} / 5, P3 = P5 - 2 h dq_{i+1} / 5 + h^2 ddq_{i+1} / 20,
 *   so |dq_j/du| <= 5 max_k |P_{k+1,j} - P_{k,j}| and |q_j(u)| <= max_k |P_{k,j}|.  These take the places of the blend's speed and
 *   reach in the sums of mp_path_blend_*; the advance from u = 0, its three decisions (BLOCKED: d - margin <= tol; FREE:
 *   u + tau >= 1; UNDECIDED: max_steps evaluations) and their order are that contract's.  Every span of a fully tracked problem is
 *   checked on its own.  The problem is DONE if all its spans are FREE, else BLOCKED or UNDECIDED as the FIRST span that is not
 *   free says; span = that span, t = the u at which its advance stopped.  DONE: span -1, t 1.
 * 4 Deviation.  Each span evaluates the curve at u = 1/2, takes its FK and compares it with the line's pose at (i + 1/2) / (N - 1):
 *   deviation_pos / deviation_rot = the largest position distance / rotation angle (POSITION: 0) over the problem's spans.
 * Per problem (every output may be NULL, at least one is needed; the device form needs q, dq and ddq, which its span launch reads):
 *     status (B) int32                   MP_CARTESIAN_DONE 0, _STALLED 1, _SINGULAR 2, _LIMIT 3, _JUMP 4, _BLOCKED 5, _UNDECIDED 6,
 *                                        _INVALID -1
 *     reached, span (B) int32
 *     t, clearance (B)                   clearance: the smallest distance any evaluation of any span saw
 *     deviation_pos, deviation_rot (B)
 *     pose_error (B)                     the largest converged error over the grid points 1..reached-1: max(rot, tr), POSITION: tr
 *     iterations, evaluations (B) int32  Newton steps; collision evaluations over all spans
 *     q, dq, ddq (B, N, n)               the grid, batch-major
 *     span_status (B, N - 1) int32       MP_EDGE_FREE / _BLOCKED / _UNDECIDED, -1 for the spans of a problem not tracked to its end
 *     span_clearance (B, N - 1)
 *   A problem that was not tracked to its end has span -1, NaN in t, clearance and the deviations and 0 evaluations; INVALID also has
 *   a NaN pose_error.  No random numbers; a problem's result depends on its own content only.  No output may overlap an input.
 * mp_cartesian_path_f64: device arrays, 16-byte aligned.  Three launches on the compute stream: the tracking, one lane a problem;
 *   the spans, one lane a span, taken from a queue, one collision evaluation a trip; the reduction, one lane a problem.  The spans'
 *   records pass through d_workspace, mp_cartesian_path_workspace_bytes(B, N) bytes (or minus an MP_ERR_* code); max_blocks > 0 caps
 *   the grid of the span launch.  Asynchronous; it allocates nothing once the handle is resident on the context and may then be
 *   captured into a launch graph (the queue head's reset is part of it).  Launches that share a collision handle share its queue
 *   head: they are serialised by the handle's lock and the compute stream.
 *   mp_cartesian_path_host_f64: host arrays, device memory (workspace and unrequested grid arrays included) from the context's pool.
 *   mp_cartesian_path_cpu_f64: the kernels' per-problem and per-span code on the host, no context. */
#define MP_CARTESIAN_DONE 0
#define MP_CARTESIAN_STALLED 1
#define MP_CARTESIAN_SINGULAR 2
#define MP_CARTESIAN_LIMIT 3
#define MP_CARTESIAN_JUMP 4
#define MP_CARTESIAN_BLOCKED 5
#define MP_CARTESIAN_UNDECIDED 6
#define MP_CARTESIAN_INVALID (-1)
#define MP_TASK_FULL 0
#define MP_TASK_POSITION 1
int64_t mp_cartesian_path_workspace_bytes(int64_t B, int64_t N);
int mp_cartesian_path_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_q_start, const double* d_T_goal, int64_t B,
                          const double* lo, const double* hi, int64_t N, int task, double eomg, double ev, double damping, int max_iters,
                          double max_joint_step, double margin, double tol, int max_steps, void* d_workspace, size_t workspace_bytes,
                          int max_blocks, int32_t* d_status, int32_t* d_reached, int32_t* d_span, double* d_t, double* d_clearance,
                          double* d_deviation_pos, double* d_deviation_rot, double* d_pose_error, int32_t* d_iterations,
                          int32_t* d_evaluations, double* d_q, double* d_dq, double* d_ddq, int32_t* d_span_status,
                          double* d_span_clearance);
int mp_cartesian_path_host_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* q_start, const double* T_goal, int64_t B,
                               const double* lo, const double* hi, int64_t N, int task, double eomg, double ev, double damping,
                               int max_iters, double max_joint_step, double margin, double tol, int max_steps, int32_t* status,
                               int32_t* reached, int32_t* span, double* t, double* clearance, double* deviation_pos,
                               double* deviation_rot, double* pose_error, int32_t* iterations, int32_t* evaluations, double* q, double* dq,
                               double* ddq, int32_t* span_status, double* span_clearance);
int mp_cartesian_path_cpu_f64(const mp_model* model, const mp_collision* h, const double* q_start, const double* T_goal, int64_t B,
                              const double* lo, const double* hi, int64_t N, int task, double eomg, double ev, double damping,
                              int max_iters, double max_joint_step, double margin, double tol, int max_steps, int32_t* status,
                              int32_t* reached, int32_t* span, double* t, double* clearance, double* deviation_pos,
                              double* deviation_rot, double* pose_error, int32_t* iterations, int32_t* evaluations, double* q, double* dq,
                              double* ddq, int32_t* span_status, double* span_clearance, int nthreads);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI (new; the reference is single-device) ------
 * Trajectory batches are sharded over ranks with no exchange during compute; the only collective is
 * the all-gather that reassembles the torque history.  Rank 0 creates the id, the launcher
 * broadcasts its 128 bytes out of band (bench.py uses the torch.distributed gloo store). */
int mp_comm_unique_id(uint8_t id[MP_UNIQUE_ID_BYTES]);
int mp_comm_create(mp_ctx* ctx, const uint8_t id[MP_UNIQUE_ID_BYTES], int nranks, int rank, mp_comm** out);
int mp_comm_destroy(mp_comm* comm);
/* d_recv (nranks * bytes_per_rank) <- every rank's d_send (bytes_per_rank); enqueued on the compute
 * stream after the kernels already queued there. */
int mp_comm_allgather(mp_comm* comm, const void* d_send, void* d_recv, size_t bytes_per_rank);
/* Uneven shards (B % nranks != 0; sharding.shard_range gives the first B % nranks ranks one trajectory more): rank r
 * contributes bytes_of_rank[r] bytes and d_recv receives the shards back to back in rank order.  Grouped ncclSend / ncclRecv
 * per peer on the compute stream (ncclAllGather needs equal counts).  Every rank passes the same nranks-entry array. */
int mp_comm_allgatherv(mp_comm* comm, const void* d_send, void* d_recv, const size_t* bytes_of_rank);
/* The same reassembly, overlapped with compute.  d_all holds nranks slots of bytes_per_rank; a rank writes ITS slot
 * chunk by chunk with ordinary launches on the compute stream (output pointer = slot + offset) and, after the launches
 * of a chunk, calls mp_comm_exchange_chunk: the bytes [offset, offset + nbytes) of its slot go to every peer, every
 * peer's same range arrives in that peer's slot (one ncclSend + ncclRecv per peer in a group: xGMI is point to point),
 * on the communicator's own stream, ordered behind the compute stream's tail - so the kernels of the next chunk run
 * beside the exchange.  Every rank must issue the same sequence of chunks.  mp_comm_join makes the compute stream
 * wait for all exchanges issued so far (call it before anything reads d_all). */
int mp_comm_exchange_chunk(mp_comm* comm, void* d_all, size_t bytes_per_rank, size_t offset, size_t nbytes);
/* mp_comm_exchange_chunk for uneven shards: rank r's slot starts slot_offset[r] bytes into d_all, and this chunk is
 * [chunk_offset[r], chunk_offset[r] + chunk_bytes[r]) of it; nranks entries each, the same arrays on every rank. */
int mp_comm_exchange_chunk_v(mp_comm* comm, void* d_all, const size_t* slot_offset, const size_t* chunk_offset,
                             const size_t* chunk_bytes);
/* Buffer lifetime: mp_free hands a buffer back to the pool immediately, and the pool orders reuse with respect to the
 * context's COMPUTE stream only.  A buffer a communicator is still reading or writing on its own stream (after
 * mp_comm_exchange_chunk) must therefore not be freed before mp_comm_join (mp_comm_allgather runs on the compute
 * stream and needs no join). */
int mp_comm_join(mp_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* MANIPULA_HIP_H */
