// Handle layouts shared by the translation units that implement the C ABI (mp_capi.cpp, mp_cpu.cpp).
#pragma once
#include <cstdint>
#include <map>
#include <mutex>
#include <vector>

#include "mp_collision.h"
#include "mp_rrt.h"
#include "mp_shortcut.h"
#include "mp_goal.h"
#include "mp_model.h"

struct mp_model {
  MpModel<double> d;   // n <= MP_MAX_DOF: the unrolled kernels take these by value.  d.n is ALWAYS the joint count.
  MpModel<float> f;
  bool big = false;    // MP_MAX_DOF < n <= MP_BIG_DOF: only bd / bf hold the joints; the looped kernels (csrc/mp_dyn.h) read them
  MpBigModel<double> bd;
  MpBigModel<float> bf;
  double pmap[MP_MAX_DOF * 100];  // n <= MP_MAX_DOF: per link the 10 x 10 inertial-parameter map D (mp_inertial_map, mp_regressor.h)
  uint64_t uid;  // never reused, so a context's device copies cannot alias a destroyed model
};

// Sphere collision model (mp_collision.h): the host tables, and per context that has used it the device copies.  The device side is
// mp_capi.cpp's: it registers `release` when it makes the first copy, mp_collision_destroy (mp_cpu.cpp) calls it.
struct mp_collision {
  int n = 0;                          // joint count of the model it was made for
  MpColSpheres sph;
  std::vector<MpColPair> pairs;
  std::vector<MpColObstacle> world;   // the _cpu twin's world (and the last one set on any context)
  struct Resident {
    int device = -1;
    void* sph = nullptr;              // MpColSpheres, then the pairs
    void* world = nullptr;            // MpColWorld, then `cap` obstacles
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

int mp_set_error(int code, const char* msg);  // thread-local message of mp_last_error (mp_capi.cpp; C++ linkage)
