// What the translation units that implement the C ABI share (mp_capi.cpp: the entries of a context; mp_cpu.cpp: their CPU twins):
// the handle layouts, the one way to refuse a call (mp_fail / REQUIRE), the pointer checks of an output struct (mp_out_any,
// mp_out_aligned16), the model gate, and per family the check of an entry's arguments (mp_*_check, defined in mp_cpu.cpp) that all
// three entries of an operation call.  DESIGN.md, section 3, has the rules.
#pragma once
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/manipula_hip.h"
#include "mp_collision.h"
#include "mp_rrt.h"
#include "mp_shortcut.h"
#include "mp_goal.h"
#include "mp_blend.h"
#include "mp_sample.h"
#include "mp_cartesian.h"
#include "mp_ik.h"
#include "mp_toppra.h"
#include "mp_model.h"

// ---- refusing a call: the message of mp_last_error, formatted; REQUIRE(cond, fmt, ...) returns MP_ERR_INVALID unless cond holds
int mp_set_error(int code, const char* msg);  // thread-local message of mp_last_error (mp_capi.cpp; C++ linkage)
__attribute__((format(printf, 2, 3))) inline int mp_fail(int code, const char* fmt, ...) {
  char msg[512];  // the size of the message mp_last_error keeps
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(msg, sizeof msg, fmt, ap);
  va_end(ap);
  return mp_set_error(code, msg);
}
#define REQUIRE(cond, ...)                                        \
  do {                                                            \
    if (!(cond)) return mp_fail(MP_ERR_INVALID, __VA_ARGS__);     \
  } while (0)

// ---- the pointer checks of an output struct (MpColOut ... MpSampleOut: pointers only, any of them null), seen as its array of pointers
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
template <typename Out>
std::array<const void*, sizeof(Out) / sizeof(void*)> mp_out_pointers(const Out& O) {
  static_assert(std::is_standard_layout<Out>::value && sizeof(Out) % sizeof(void*) == 0, "an output struct is a whole number of pointers");
  std::array<const void*, sizeof(Out) / sizeof(void*)> p;
  std::memcpy(p.data(), &O, sizeof O);
  return p;
}
template <typename Out>
bool mp_out_any(const Out& O) {  // is any output asked for
  for (const void* p : mp_out_pointers(O))
    if (p) return true;
  return false;
}
template <typename Out>
bool mp_out_aligned16(const Out& O) {  // (a null pointer is aligned)
  for (const void* p : mp_out_pointers(O))
    if (!aligned16(p)) return false;
  return true;
}

struct mp_model {
  MpModel<double> d;   // n <= MP_MAX_DOF: the unrolled kernels take these by value.  d.n is ALWAYS the joint count.
  MpModel<float> f;
  bool big = false;    // MP_MAX_DOF < n <= MP_BIG_DOF: only bd / bf hold the joints; the looped kernels (csrc/mp_dyn.h) read them
  MpBigModel<double> bd;
  MpBigModel<float> bf;
  double pmap[MP_MAX_DOF * 100];  // n <= MP_MAX_DOF: per link the 10 x 10 inertial-parameter map D (mp_inertial_map, mp_regressor.h)
  uint64_t uid;  // never reused, so a context's device copies cannot alias a destroyed model
};

// ---- the model gate of the entries that exist for the unrolled kernels only.  `n`: the joint count refused
inline int mp_too_many_joints(const char* fn, int n) {
  return mp_fail(MP_ERR_UNSUPPORTED, "%s: not available for models with more than %d joints (this one has %d)", fn, MP_MAX_DOF, n);
}
#define REQUIRE_SMALL(fn)                                              \
  do {                                                                 \
    if (model->big) return mp_too_many_joints(fn, model->d.n);         \
  } while (0)
// the twins' form: a model, and a small one (the entries of a context word the null case with their context)
inline int mp_small_model(const char* fn, const mp_model* model) {
  REQUIRE(model, "%s: null model", fn);
  REQUIRE_SMALL(fn);
  return MP_OK;
}

const double kG[3] = {0.0, 0.0, -9.81};  // reference planning/trajectory_dynamics.py:54
inline bool any_nonzero(const double* F) {
  if (!F) return false;
  for (int k = 0; k < 6; ++k)
    if (F[k] != 0.0) return true;
  return false;
}
template <typename T> const MpModel<T>& pick(const mp_model* m);
template <> inline const MpModel<float>& pick<float>(const mp_model* m) { return m->f; }
template <> inline const MpModel<double>& pick<double>(const mp_model* m) { return m->d; }
template <typename T> const MpBigModel<T>& pick_big(const mp_model* m);
template <> inline const MpBigModel<float>& pick_big<float>(const mp_model* m) { return m->bf; }
template <> inline const MpBigModel<double>& pick_big<double>(const mp_model* m) { return m->bd; }

// ---- per family the check of an entry's arguments: 0, or an MP_ERR_* code with the message set, `fn` the entry's name in front
// (mp_cpu.cpp).  A check packs the kernel's parameter struct where this header can see it.
// operational space: frame 0..2, task 0..2, damping finite and >= 0, rows >= 0
int mp_opspace_check(const char* fn, int frame, int task, double damping, int64_t rows);
// kinematics VJP: frame 0 or 1, rows >= 0
int mp_kin_vjp_check(const char* fn, int frame, int64_t rows);
// the regressor and its normal form: rows >= 0
int mp_regressor_check(const char* fn, int64_t rows);
// iLQR: three weight vectors (2n, n, 2n), finite.  (MpIlqrWeights is declared with the launchers, which the twins do not see: the
// entries of a context pack it themselves)
int mp_ilqr_weights_check(const char* fn, int n, const double* wq, const double* wr, const double* wf);
// TOPP-RA: the velocity limits (n, finite and positive) and the torque (n, 2) / acceleration (n) limits, either may be null (none)
int mp_toppra_vmax_check(const char* fn, int n, const double* vlim, MpToppraVmax* out);
int mp_toppra_limits_check(const char* fn, int n, const double* tlim, const double* alim, MpToppraLimits* out);
// inverse kinematics: the tolerances, then the settings packed into MpIkParams / MpIkBigParams.  0; MP_ERR_INVALID with the message
// set; or -(1 + j) with no message for a joint j whose lower limit lies above its upper one, which the twin and the entries of a
// context word differently
template <int CAP>
int mp_ik_pack(const char* fn, int n, const double* joint_limits, double eomg, double ev, int max_iterations, double damping,
               double step_cap, double w_o, double w_p, int adaptive, int backtracking, uint32_t seed, MpIkParamsT<CAP>* P) {
  REQUIRE(eomg > 0 && ev > 0 && damping >= 0 && step_cap > 0, "%s: eomg, ev, step_cap must be positive and damping non-negative", fn);
  P->eomg = eomg; P->ev = ev; P->damping = damping; P->step_cap = step_cap; P->w_o = w_o; P->w_p = w_p;
  P->max_iterations = max_iterations; P->seed = seed;
  P->adaptive_tuning = adaptive ? 1 : 0; P->backtracking = backtracking ? 1 : 0;
  for (int j = 0; j < CAP; ++j) {
    P->lo[j] = (j < n && joint_limits) ? joint_limits[2 * j] : -HUGE_VAL;
    P->hi[j] = (j < n && joint_limits) ? joint_limits[2 * j + 1] : HUGE_VAL;
    if (P->lo[j] > P->hi[j]) return -(1 + j);
  }
  return MP_OK;
}

// Sphere collision model (mp_collision.h): the host tables, and per context that has used it the device copies.  The device side is
// mp_capi.cpp's: it registers `release` when it makes the first copy, mp_collision_destroy (mp_cpu.cpp) calls it.
struct mp_collision {
  int n = 0;                          // joint count of the model it was made for
  MpColSpheres sph;
  std::vector<MpColPair> pairs;
  std::vector<MpColObstacle> world;   // the _cpu twin's world (and the last one set on any context)
  std::vector<MpCloudPoint> cloud;    // the point cloud's image (mp_cloud.h: header, cell starts, records), empty: none; as `world`
  struct Resident {
    int device = -1;
    void* sph = nullptr;              // MpColSpheres, then the pairs
    void* world = nullptr;            // MpColWorld, then `cap` obstacles
    void* cloud = nullptr;            // the cloud's image, null: none (the world table's header holds this address)
    int cap = 0;
    void* counter = nullptr;          // the 8-byte work-queue head of k_collision_edges
    std::vector<void*> retired;       // outgrown world tables that captured graphs may still read
  };
  std::map<uint64_t, Resident> resident;  // by context uid
  std::mutex mu;
  void (*release)(mp_collision*) = nullptr;
};
// checks an obstacle table and packs it; 0 or an MP_ERR_* code with the message set (mp_cpu.cpp)
int mp_collision_pack_world(const char* fn, int O, const int32_t* kind, const double* params, std::vector<MpColObstacle>* out);
// checks a point cloud and builds its image with a counting sort; M = 0 gives the empty image (no cloud); cell <= 0: the default,
// d_max + radius; 0, or MP_ERR_INVALID with the message set and `image` untouched (mp_cloud_build.cpp)
int mp_cloud_build(const char* fn, int64_t M, const double* points, double radius, double d_max, double cell,
                   std::vector<MpCloudPoint>* image);
// the edge check's parameters: margin finite, tol positive and finite, max_steps in 1..65536; 0 or MP_ERR_INVALID (mp_cpu.cpp)
int mp_collision_edges_check(const char* fn, double margin, double tol, int max_steps);
// the planner's parameters (the edge check's among them), packed into `out`; 0, or MP_ERR_INVALID with the message set (mp_cpu.cpp)
int mp_rrt_connect_check(const char* fn, int n, const double* lo, const double* hi, uint32_t seed, double step, double min_advance,
                         int max_iters, int max_nodes, int max_waypoints, double margin, double tol, int max_steps, MpRrtParams* out);
// the shortcutter's parameters (the edge check's among them), packed into `out`; 0, or MP_ERR_INVALID with the message set (mp_cpu.cpp)
int mp_path_shortcut_check(const char* fn, int64_t w_in, uint32_t seed, int max_iters, double min_gain, int max_waypoints, double margin,
                           double tol, int max_steps, MpShortcutParams* out);
// the goal-configuration parameters (margin and tol of the edge check among them), packed into `out`; 0, or MP_ERR_INVALID with the
// message set (mp_cpu.cpp)
int mp_goal_ik_check(const char* fn, int n, const double* lo, const double* hi, uint32_t seed, double eomg, double ev, double damping,
                     double step_cap, int max_iters, int max_attempts, double margin, double tol, MpGoalParams* out);
// the corner blender's parameters (the edge check's among them), packed into `out`; 0, or MP_ERR_INVALID with the message set
// (mp_cpu.cpp)
int mp_path_blend_check(const char* fn, int64_t w_in, int64_t grid, double blend, int max_halvings, double margin, double tol,
                        int max_steps, MpBlendParams* out);
// the Cartesian path's parameters (the edge check's among them), packed into `out`; 0, MP_ERR_UNSUPPORTED for a chain with fewer
// joints than the task has rows, or MP_ERR_INVALID, with the message set (mp_cpu.cpp)
int mp_cartesian_path_check(const char* fn, int n, int64_t B, const double* lo, const double* hi, int64_t grid, int task, double eomg,
                            double ev, double damping, int max_iters, double max_joint_step, double margin, double tol, int max_steps,
                            MpCartParams* out);
// the trajectory sampler's arguments, packed into `out` (the pointers are the caller's to fill in): the source is chosen by which group of
// pointers is given - grid_given of the 3 grid arrays, curve_given of the 6 blend tables; 0, or MP_ERR_INVALID with the message set
// (mp_cpu.cpp)
int mp_trajectory_sample_check(const char* fn, int64_t B, int64_t grid, int64_t w_in, double dt, int64_t M, int n, int grid_given,
                               int curve_given, MpSampleIn* out);
