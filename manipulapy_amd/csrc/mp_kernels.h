// Launcher prototypes (defined in mp_kernels.hip); every launch is asynchronous on `s`.
#pragma once
#include <hip/hip_runtime_api.h>

#include "mp_model.h"

hipError_t mpk_selftest(hipStream_t s, int* d_out /* 64 ints */);
hipError_t mpk_stream(hipStream_t s, int reads, bool nontemporal, const void* a, const void* b, const void* c, void* d, long n4);
hipError_t mpk_stream_mix(hipStream_t s, int reads, int writes, bool nontemporal, const void* a, void* d, long n4);
hipError_t mpk_clock_sampler(hipStream_t s, unsigned long long* out, unsigned blocks, unsigned samples, unsigned naps);

template <typename T>   // (float64 only: float32 rows take mpk_id_dm)
hipError_t mpk_id(hipStream_t s, const MpModel<T>& M, const MpCall<T>& C, bool ftip, const T* q, const T* qd,
                  const T* qdd, T* tau, long rows);

// float32, one row per lane, the model read through a pointer to a device-resident copy (scalar loads joint by joint)
// all_revolute: every joint of the model is revolute (rev == 1) - the kernel instance that folds the revolute / prismatic blend
hipError_t mpk_id_dm(hipStream_t s, const MpModel<float>* d_model, int n, const MpCall<float>& C, bool ftip, const float* q,
                     const float* qd, const float* qdd, float* tau, long rows, const MpLead& L, bool all_revolute);

// the float64 pass over the rows the kernel above handed over (C.hard_rows / hard_ctrl), `blocks` blocks of 64 lanes
hipError_t mpk_id_hard(hipStream_t s, const MpModel<float>* d_model, int n, const MpCall<float>& C, bool ftip, const float* q,
                       const float* qd, const float* qdd, float* tau, unsigned rows, unsigned blocks);
hipError_t mpk_id_hard_batch(hipStream_t s, const MpModel<float>* d_model, int n, bool ftip, const MpHardBatch& B, int entries, unsigned blocks);

hipError_t mpk_batch_traj(hipStream_t s, const MpModel<float>& M, const float* start, const float* end, long B,
                          long Nt, double Tf, int method, float* pos, float* vel, float* acc);

template <typename T>
hipError_t mpk_fk_jac_id(hipStream_t s, const MpModel<T>& M, const MpCall<T>& C, bool ftip, const T* q, const T* qd,
                         const T* qdd, T* Tout, T* Jout, T* tau, long rows);

template <typename T>
hipError_t mpk_mass_matrix(hipStream_t s, const MpModel<T>& M, const T* q, T* Mout, long rows);
template <typename T>
hipError_t mpk_forward_dynamics(hipStream_t s, const MpModel<T>& M, const MpCall<T>& C, bool ftip, const T* q, const T* qd,
                                const T* tau, T* qdd, long rows);
// analytical derivatives (csrc/mp_deriv.h), float64, 1..MP_MAX_DOF joints; tau / Mout and qdd / Minv may be null
hipError_t mpk_id_deriv(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, bool ftip, const double* q, const double* qd,
                        const double* qdd, double* tau, double* dq, double* dqd, double* Mout, long rows);
hipError_t mpk_fd_deriv(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, bool ftip, const double* q, const double* qd,
                        const double* tau, double* qdd, double* dq, double* dqd, double* Minv, long rows);
// vector-Jacobian products by reverse mode (csrc/mp_adjoint.h), float64, 1..MP_MAX_DOF joints; gqdd, qdd and gtau (outputs) may be null
hipError_t mpk_id_vjp(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, bool ftip, const double* q, const double* qd,
                      const double* qdd, const double* gtau, double* gq, double* gqd, double* gqdd, long rows);
hipError_t mpk_fd_vjp(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, bool ftip, const double* q, const double* qd,
                      const double* tau, const double* gqdd, double* qdd, double* gq, double* gqd, double* gtau, long rows);
// reverse mode through FK + Jacobian (csrc/mp_kin_vjp.h), float64, 1..MP_MAX_DOF joints; frame 0 = space, 1 = body; gT / gJ (inputs)
// and Tout / Jout / gq (outputs) may be null
hipError_t mpk_fk_jac_vjp(hipStream_t s, const MpModel<double>& M, int frame, const double* q, const double* gT, const double* gJ,
                         double* Tout, double* Jout, double* gq, long rows);
// operational-space dynamics and task-space torque (csrc/mp_opspace.h), float64, 1..MP_MAX_DOF joints; frame 0 = space, 1 = body,
// 2 = hybrid; task 0 = full, 1 = linear, 2 = angular; lam2 = damping^2; every output of mpk_opspace and tau0 may be null
hipError_t mpk_opspace(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, int frame, int task, double lam2, const double* q,
                       const double* qd, double* Tout, double* Jout, double* Jdqd, double* Lam, double* Jbar, double* mu, double* p,
                       long rows);
hipError_t mpk_opspace_torque(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, int frame, int task, double lam2,
                              const double* q, const double* qd, const double* acc, const double* tau0, double* tau, long rows);
// reverse mode through the roll-out (csrc/mp_rollout_vjp.h) on the time-major layout: taumat / Ftipmat / gp / gv / ga / gtau (Nt, B, *),
// theta0 / dtheta0 / gth0 / gdth0 (B, n); Ftipmat and the cotangents may be null; `work` holds (B Nt + B intRes) 2n doubles
// dynamics regressor (csrc/mp_regressor.h), float64, 1..MP_MAX_DOF joints; Dmap = the model's n x 100 inertial-parameter map in
// device memory.  Y (rows, n, 10n); tau_ext may be null.
hipError_t mpk_id_regressor(hipStream_t s, const MpModel<double>& M, const double* Dmap, const MpCall<double>& C, bool ftip,
                            const double* q, const double* qd, const double* qdd, double* Y, double* tau_ext, long rows);
// Normal equations of the regressor without Y in memory: a fixed grid of mp_reg_normal_groups(rows) workgroups, each over tiles of
// mp_reg_normal_tile() rows, leaves its partial sums (mp_reg_normal_stride(n) doubles) in `work`; a second kernel adds them in
// workgroup order.  A (10n, 10n, may be null), b (10n), rr (1).  rows >= 1.
constexpr int kRegNormalLanes = 5;       // lanes that build one row (a divisor of 10: each builds 10 / lanes columns of every block)
constexpr int kRegNormalMaxGroups = 1024;
constexpr int mp_reg_normal_tile() { return 64 / kRegNormalLanes; }
inline long mp_reg_normal_groups(long rows) {
  const long tiles = (rows + mp_reg_normal_tile() - 1) / mp_reg_normal_tile();
  return tiles < kRegNormalMaxGroups ? (tiles > 0 ? tiles : 1) : kRegNormalMaxGroups;
}
constexpr long mp_reg_normal_stride(int n) { return ((100L * n * n + 10L * n + 1) + 1) & ~1L; }
hipError_t mpk_id_regressor_normal(hipStream_t s, const MpModel<double>& M, const double* Dmap, const MpCall<double>& C, bool ftip,
                                   const double* q, const double* qd, const double* qdd, const double* rhs, long rows, double* work,
                                   double* A, double* b, double* rr);
hipError_t mpk_fd_traj_vjp(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, const double* theta0, const double* dtheta0,
                           const double* taumat, const double* Ftipmat, long B, long Nt, double h, int intRes, const double* gp,
                           const double* gv, const double* ga, double* work, double* gth0, double* gdth0, double* gtau);
// batched iLQR (csrc/mp_ilqr.h) on the time-major layout, float64, 1..MP_MAX_DOF joints: pos / vel / tau (Nt, B, n), the derivative
// blocks of the (Nt - 1) B rows (pos[0:Nt-1], vel[0:Nt-1], tau[1:Nt]), xref (Nt, B, 2n), reg (B).  work == nullptr: the cooperative
// kernel (16 lanes a trajectory, LDS); otherwise the one-lane-per-trajectory kernel, `work` holding B mp_ilqr_work_doubles(n) doubles.  K (Nt, B, n, 2n) / k (Nt, B, n), or (B, Nt, ...) with k_batch_major.  The roll-out runs A B lanes: alpha / cost (A, B),
// opos / ovel / otau (Nt, A B, n) or all null; K and k may both be null (open loop).
struct MpIlqrWeights {
  double wq[2 * MP_MAX_DOF], wr[MP_MAX_DOF], wf[2 * MP_MAX_DOF];
};
hipError_t mpk_ilqr_backward(hipStream_t s, const MpModel<double>& M, const MpIlqrWeights& Wt, const double* pos, const double* vel,
                             const double* tau, const double* dq, const double* dqd, const double* Minv, const double* xref,
                             const double* reg, long B, long Nt, double h, bool k_batch_major, double* work, double* K, double* k,
                             double* dV, int* status);
hipError_t mpk_ilqr_rollout(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, const MpIlqrWeights& Wt, const double* th0,
                            const double* dth0, const double* tau, const double* pos, const double* vel, const double* K, const double* k,
                            const double* alpha, const double* xref, long A, long B, long Nt, double h, bool k_batch_major, double* cost,
                            double* opos, double* ovel, double* otau);
// time-optimal path parameterisation (csrc/mp_toppra.h), float64, 1..MP_MAX_DOF joints.  mpk_path_coeffs: one lane per row of q / q' / q''
// in any layout -> a, b, c (rows, n), xbar (rows).  mpk_toppra_sweep: one lane per path on the time-major layout, coefficients (Nt, B, n),
// xbar (Nt, B), sd_start / sd_end (B) -> K (Nt, B, 2), x / u / t (Nt, B), dur (B), status (B); dq / ddq are read when `acc` or when the
// three row outputs oqd / oqdd / otau (Nt, B, n) are given (the epilogue fused into the forward pass).  mpk_path_rows: the epilogue as a
// launch of its own, one lane per row.
struct MpToppraLimits;
struct MpToppraVmax;
hipError_t mpk_path_coeffs(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, bool ftip, const MpToppraVmax& V,
                           const double* q, const double* dq, const double* ddq, double* a, double* b, double* c, double* xbar, long rows);
hipError_t mpk_toppra_sweep(hipStream_t s, int n, const MpToppraLimits& lim, bool acc, const double* a, const double* b, const double* c,
                            const double* xbar, const double* dq, const double* ddq, const double* sd_start, const double* sd_end, long B,
                            long Nt, double* K, double* x, double* u, double* t, double* dur, int* status, double* oqd, double* oqdd,
                            double* otau);
hipError_t mpk_path_rows(hipStream_t s, int n, const double* a, const double* b, const double* c, const double* dq, const double* ddq,
                         const double* x, const double* u, double* oqd, double* oqdd, double* otau, long rows);
// Ftipmat == nullptr: no tip wrench.  h = dt / intRes.  Outputs are float32 (B, Nt, n).
template <typename T>
hipError_t mpk_fd_traj(hipStream_t s, const MpModel<T>& M, const MpCall<T>& C, const T* theta0, const T* dtheta0,
                       const T* taumat, const T* Ftipmat, long B, long Nt, T h, int intRes, float* pos, float* vel, float* acc);

// the same roll-out on the TIME-MAJOR device layout: taumat (Nt, B, n), Ftipmat (Nt, B, 6), pos / vel / acc (Nt, B, n)
template <typename T>
hipError_t mpk_fd_traj_tm(hipStream_t s, const MpModel<T>& M, const MpCall<T>& C, const T* theta0, const T* dtheta0,
                          const T* taumat, const T* Ftipmat, long B, long Nt, T h, int intRes, float* pos, float* vel, float* acc);
// (outer, inner, row_dwords x 4 bytes) -> (inner, outer, row_dwords x 4 bytes)
hipError_t mpk_transpose_rows(hipStream_t s, const void* src, void* dst, long outer, long inner, int row_dwords);

// ---- 9..32 joints (csrc/mp_dyn.h): run-time-n kernels, the model (MpBigModel<T>) resident in device memory; n = its joint count
// (picks the kernels' per-row array capacity, MP_MID_DOF or MP_BIG_DOF)
template <typename T>
hipError_t mpk_dyn_fk_jac_id(hipStream_t s, int n, const MpBigModel<T>* d_model, const MpCall<T>& C, bool ftip, const T* q, const T* qd,
                             const T* qdd, T* Tout, T* Jout, T* tau, long rows);
template <typename T>
hipError_t mpk_dyn_mass_matrix(hipStream_t s, int n, const MpBigModel<T>* d_model, const T* q, T* Mout, long rows);
template <typename T>
hipError_t mpk_dyn_forward_dynamics(hipStream_t s, int n, const MpBigModel<T>* d_model, const MpCall<T>& C, bool ftip, const T* q, const T* qd,
                                    const T* tau, T* qdd, long rows);
template <typename T>
hipError_t mpk_dyn_fd_traj(hipStream_t s, int n, const MpBigModel<T>* d_model, const MpCall<T>& C, const T* theta0, const T* dtheta0,
                           const T* taumat, const T* Ftipmat, long B, long Nt, T h, int intRes, float* pos, float* vel, float* acc,
                           bool time_major);
// pos / vel / acc (all three or none) and / or tau of the time-scaled trajectories
hipError_t mpk_dyn_traj(hipStream_t s, int n, const MpBigModel<float>* d_model, const MpCall<float>& C, bool ftip, const float* start,
                        const float* end, long B, long Nt, double Tf, int method, float* pos, float* vel, float* acc, float* tau);

// Cartesian straight-line trajectories between B pose pairs (4x4 row-major float64): float32 (B,Nt,3) x3, (B,Nt,3,3)
hipError_t mpk_cartesian_traj(hipStream_t s, const double* Xstart, const double* Xend, long B, long Nt, double Tf, int method,
                              float* pos, float* vel, float* acc, float* ori);

// Fused attractive + repulsive potential and gradient at P points against O obstacles (float32); goal on the host.
hipError_t mpk_potential_field(hipStream_t s, const float* pos, const float* goal3_host, const float* obs, long P, long O,
                               float influence, float* pot, float* grad);

// B damped-least-squares inverse-kinematics problems (csrc/mp_ik.h): Tdes (B,4,4), theta0 / theta (B,n) float64
template <int CAP> struct MpIkParamsT;
typedef MpIkParamsT<MP_MAX_DOF> MpIkParams;
typedef MpIkParamsT<MP_BIG_DOF> MpIkBigParams;
// queue_counter: 8 bytes of device memory owned by the caller (zeroed here on the stream before the launch)
hipError_t mpk_ik(hipStream_t s, const MpModel<double>& M, const MpIkParams& P, const double* Tdes, const double* theta0, long B,
                  double* theta, int* success, int* iterations, int* restarts, unsigned long long* queue_counter, int compute_units);
// K closed-loop PD regulation runs (csrc/mp_core.h mp_pd_regulation_run): theta0 / des (K,n), Kp / Kd (K), err (K,steps), count (K)
hipError_t mpk_pd_regulation(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, const double* theta0, const double* des,
                             const double* Kp, const double* Kd, long K, double dt, int steps, double* err, int* count);
hipError_t mpk_dyn_pd_regulation(hipStream_t s, int n, const MpBigModel<double>* d_model, const MpCall<double>& C, const double* theta0,
                                 const double* des, const double* Kp, const double* Kd, long K, double dt, int steps, double* err, int* count);
// the same for 9..32 joints (run-time joint count, the model resident in device memory)
hipError_t mpk_dyn_ik(hipStream_t s, int n, const MpBigModel<double>* d_model, const MpIkBigParams& P, const double* Tdes, const double* theta0,
                      long B, double* theta, int* success, int* iterations, int* restarts, unsigned long long* queue_counter,
                      int compute_units);

// table-driven fused generation + ID (float32): `tab` = 3 doubles per timestep written by mpk_time_table for the same
// (Nt, Tf, method); one lane takes timesteps t and t + ceil(Nt / 2) of one trajectory
hipError_t mpk_time_table(hipStream_t s, double* tab, long Nt, double Tf, int method);
unsigned mpk_traj_blocks_per_trajectory(long Nt);
// the float64 pass over the rows the fused generic kernel handed over (inputs regenerated)
hipError_t mpk_traj_id_hard(hipStream_t s, const MpModel<float>* d_model, int n, const MpCall<float>& C, bool ftip, const float* start,
                            const float* end, unsigned Nt, const double* tab, float* tau, unsigned rows, unsigned blocks);
hipError_t mpk_traj_id_tab(hipStream_t s, const MpModel<float>& M, const MpCall<float>& C, bool ftip, const float* start,
                           const float* end, long B, long Nt, const double* tab, float* tau);

// sphere-model collision distances, cost and gradients (csrc/mp_collision.h), float64, 1..MP_MAX_DOF joints; D.S sizes the dynamic
// LDS; O: the outputs, any of them null (the gradient instance is taken when one of its three gradient arrays is given)
struct MpColSpheres;
struct MpColPair;
struct MpColWorld;
struct MpColOut;
struct MpColDevice {  // a collision handle's tables on one device, and the 8-byte head of the work queue beside them
  int S;
  const MpColSpheres* sph;
  const MpColPair* pairs;
  const MpColWorld* world;
  unsigned long long* counter;
  bool cloud;  // the handle has a point cloud (csrc/mp_cloud.h): the launchers take the kernels' instance that queries it
};
hipError_t mpk_collision(hipStream_t s, const MpModel<double>& M, const MpColDevice& D, const double* q, long rows, double eps_world,
                         double eps_self, const MpColOut& O);
// The one-wave work-queue kernels on the sphere model: continuous collision checking of joint-space edges (csrc/mp_collision.h),
// batched RRT-Connect (csrc/mp_rrt.h, the trees in `workspace`: blocks x 64 x 2 max_nodes (8 n + 4) bytes), batched path
// shortcutting (csrc/mp_shortcut.h, the working paths in `workspace`: blocks x 64 x max_waypoints (8 n + 8) bytes) and goal
// configurations for pose goals (csrc/mp_goal.h, no workspace: one pose or collision evaluation a trip).  A work queue
// over the edges / problems, one evaluated configuration a trip.  mpk_queue_plan gives a kernel's dynamic LDS and the blocks of it the
// device keeps resident (occupancy x compute_units); the caller settles the grid (`blocks`) from that, the count, its cap and the
// workspace, and hands grid and LDS to the launch, which zeroes D.counter on the stream first and makes no runtime query.  Each
// family's outputs travel as one struct of pointers (Mp*Out, beside its Mp*Params), any of them null, from the entry to the kernel.
enum MpQueueKernel { MP_QUEUE_EDGES, MP_QUEUE_RRT, MP_QUEUE_SHORTCUT, MP_QUEUE_GOAL, MP_QUEUE_BLEND };
struct MpQueuePlan {
  unsigned lds;
  long resident;
};
hipError_t mpk_queue_plan(MpQueueKernel kernel, int n, int S, bool cloud, int compute_units, MpQueuePlan* plan);
struct MpColEdgeParams;
struct MpColEdgeOut;
hipError_t mpk_collision_edges(hipStream_t s, const MpModel<double>& M, const MpColDevice& D, const double* q_from, const double* q_to,
                               long edges, const MpColEdgeParams& P, const MpColEdgeOut& O, long blocks, unsigned lds);
struct MpRrtParams;
struct MpRrtOut;
hipError_t mpk_rrt_connect(hipStream_t s, const MpModel<double>& M, const MpColDevice& D, const double* q_start, const double* q_goal,
                           long problems, const MpRrtParams& P, const MpRrtOut& O, double* workspace, long blocks, unsigned lds);
struct MpShortcutParams;
struct MpShortcutOut;
hipError_t mpk_path_shortcut(hipStream_t s, const MpModel<double>& M, const MpColDevice& D, const double* waypoints_in, const int* count_in,
                             long problems, const MpShortcutParams& P, const MpShortcutOut& O, double* workspace, long blocks,
                             unsigned lds);
struct MpGoalParams;
struct MpGoalOut;
hipError_t mpk_goal_ik(hipStream_t s, const MpModel<double>& M, const MpColDevice& D, const double* T_goal, const double* q_seed,
                       long problems, const MpGoalParams& P, const MpGoalOut& O, long blocks, unsigned lds);
// C2 corner blending of waypoint paths (csrc/mp_blend.h): the corners on the work queue (no workspace: one collision evaluation a
// trip, a lane reads its own input rows), then mpk_path_blend_sample, one lane a grid point over problems x P.grid rows, which reads
// O's status, count, points, cut, knot and length back (q, dq, ddq: any may be null).
struct MpBlendParams;
struct MpBlendOut;
hipError_t mpk_path_blend(hipStream_t s, const MpModel<double>& M, const MpColDevice& D, const double* waypoints_in, const int* count_in,
                          long problems, const MpBlendParams& P, const MpBlendOut& O, long blocks, unsigned lds);
hipError_t mpk_path_blend_sample(hipStream_t s, int n, long problems, const MpBlendParams& P, const int* status, const int* count,
                                 const double* points, const double* cut, const double* knot, const double* length, double* q, double* dq,
                                 double* ddq);
// Cartesian straight-line paths (csrc/mp_cartesian.h): k_cart_track, one lane a problem; k_cart_span, the work queue over problems x
// (P.grid - 1) spans, one lane a span (its plan from mpk_cart_plan: the instance depends on the task's rows too); k_cart_reduce, one
// lane a problem.  W: the call's workspace (mp_cart_work); q, dq, ddq are required, the outputs of O may be null.
struct MpCartParams;
struct MpCartWork;
struct MpCartOut;
hipError_t mpk_cart_plan(int n, int task, int S, bool cloud, int compute_units, MpQueuePlan* plan);
hipError_t mpk_cartesian_path(hipStream_t s, const MpModel<double>& M, const MpColDevice& D, const MpCartParams& P, const double* q_start,
                              const double* T_goal, long problems, const MpCartWork& W, double* q, double* dq, double* ddq,
                              const MpCartOut& O, long blocks, unsigned lds);
// fixed-rate sampling of timed paths (csrc/mp_sample.h): one lane a (path, sample) row over I.B x I.M rows, the tiles of 64 rows
// spread over at most `max_blocks` blocks (0: one block a tile).  curve: the geometry is the blend's tables, else the grid arrays.
struct MpSampleIn;
struct MpSampleOut;
hipError_t mpk_traj_sample(hipStream_t s, const MpModel<double>& M, const MpCall<double>& C, bool ftip, bool curve, const MpSampleIn& I,
                           const MpSampleOut& O, long max_blocks);
