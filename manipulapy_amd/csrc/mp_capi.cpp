// C ABI of libmanipula_hip.so — see include/manipula_hip.h for the contract.
// Host-only translation unit (no device code): context / streams / pooled device memory / events,
// model handles, argument validation and the host-pointer convenience wrappers.
#include <hip/hip_runtime_api.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <set>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/manipula_hip.h"
#include "mp_jit.h"
#include "mp_ik.h"
#include "mp_ilqr.h"
#include "mp_toppra.h"
#include "mp_kernels.h"
#include "mp_model_compile.h"
#include "mp_handles.h"

// ------------------------------------------------------------------------------------- objects
struct MpSpec {  // run-time specialised kernels of one model on one device
  hipModule_t mod = nullptr;
  hipModule_t mod_ilp = nullptr;  // second program (mp_jit part 1): id_s / id_co, compiled with the max-ILP scheduling strategy
  hipFunction_t traj_id_pk[2] = {nullptr, nullptr}, fd_traj[2] = {nullptr, nullptr};
  hipFunction_t id_d[2] = {nullptr, nullptr}, fk_jac_id_d[2] = {nullptr, nullptr};
  hipFunction_t ik = nullptr;
  hipFunction_t fd_s[2] = {nullptr, nullptr}, fd_d[2] = {nullptr, nullptr};  // forward dynamics per row, float32 / float64
  hipFunction_t id_s[2] = {nullptr, nullptr};                                  // inverse dynamics, float32, one row per lane
  hipFunction_t fd_traj_tm[2] = {nullptr, nullptr};                            // the roll-out on the time-major device layout
  hipFunction_t id_co[2] = {nullptr, nullptr};   // id_s with whole-line non-temporal row movement through LDS (full waves only)
  hipFunction_t id_hard[2] = {nullptr, nullptr}, traj_id_hard[2] = {nullptr, nullptr};  // the float64 pass over handed-over rows
};
struct mp_ctx {
  int device = -1;
  hipStream_t compute = nullptr;
  hipStream_t copy = nullptr;      // host -> device leg of the chunked host-buffer pipeline
  hipStream_t copy_out = nullptr;  // device -> host leg
  hipStream_t aux = nullptr;       // the shader-clock sampler's stream (mp_clock_sample_begin; created on first use)
  unsigned long long* clock_buf = nullptr;  // its stamps
  bool clock_sampling = false;
  std::map<size_t, std::vector<void*>> free_by_size;  // pool: exact-size free lists
  std::map<void*, size_t> live;                        // every buffer handed out -> its size
  std::map<uint64_t, void*> dev_models;                // model uid -> float32 model resident on this device
  std::map<uint64_t, void*> dev_big[2];                // model uid -> MpBigModel<float> [0] / <double> [1] resident on this device
  std::map<uint64_t, MpSpec> specs;                    // model uid -> specialised kernels (mp_model_specialize)
  int compute_units = 0;
  uint64_t uid = 0;                                    // never reused (graphs identify their context by it, not by address)
  bool capturing = false;                              // between mp_graph_begin and mp_graph_end
  bool stream_exported = false;                        // mp_ctx_get_stream has handed the compute stream out: no pass stays parked any more
  void* queue_counter = nullptr;                       // 8-byte work-queue head of the IK kernel (lazily allocated)
  // The float64 pass over the ill-conditioned rows of a float32 inverse-dynamics launch (attach_hard_list / hard_defer /
  // hard_flush).  The pass costs ~5 us of launch + memory latency however few rows it holds - 8 % of c2's kernel - so it is NOT
  // launched behind every float32 kernel: a launch parks it (`busy`), and parked passes are run, up to four in ONE kernel, before
  // anything that could see the difference - any other entry point, a float32 launch whose arrays overlap theirs, a fifth launch.
  struct HardSlot {
    unsigned* rows = nullptr;     // row indices
    unsigned* ctrl = nullptr;     // two counters used alternately: the pass zeroes the one the list's NEXT user counts in
    unsigned cap = 0, uses = 0;
    bool busy = false;
    bool orphan = false;          // attached to a launch whose pass never followed (a failed launch): its counters are reset on reuse
    unsigned long long seq = 0;   // launch order
    hipFunction_t fn = nullptr;   // the specialised pass of its model, or null: the generic one (k_id_hard_batch) on ...
    const MpModel<float>* gen_dm = nullptr;  // ... this device copy of the model,
    int gen_n = 0;                           // ... this joint count
    bool gen_ftip = false;                   // ... and with / without a tip wrench
    MpCall<float> C;
    const float *q = nullptr, *qd = nullptr, *qdd = nullptr;
    float* tau = nullptr;
    unsigned nrows = 0;
    unsigned nt = 0;              // generated rows (the fused kernels): timesteps per trajectory, q / qd = start / end points, qdd = the time table
    size_t bytes = 0;             // of the torque array
    size_t bytes_in = 0;          // of each input array the caller owns (q, qd, qdd; start, end)
  };
  static constexpr int kHardSlots = MP_HARD_BATCH;
  // The slots of one owner: the context's own (launches on the stream), or those of a launch graph being captured - a graph keeps
  // its lists for its lifetime, its passes are nodes of the graph, and its counters are zeroed by a node ahead of their first user.
  struct HardPool {
    HardSlot slot[kHardSlots];
    unsigned long long seq = 0;
    std::vector<void*> retired;  // lists outgrown during a capture: earlier nodes of the graph still point at them
  };
  HardPool own_pool;
  HardPool* hp = &own_pool;      // the pool launches attach to: own_pool, or the open capture's
  double* time_tab = nullptr;                          // per-timestep time-scaling table of the fused kernels
  long tab_cap = 0, tab_Nt = -1;                       // its capacity in timesteps / the call it currently holds
  double tab_Tf = 0;
  int tab_method = 0;
  bool tab_volatile = false;                           // a launch graph holds a table kernel: never trust the cache again
  std::vector<void*> retired_tabs;                     // outgrown tables that captured graphs may still reference
  int live_graphs = 0;                                 // launch graphs captured on this context and not yet destroyed
  std::vector<hipModule_t> retired_mods;               // code objects / device models of destroyed models that a live graph (or
  std::vector<void*> retired_bufs;                     //   an open capture) may still reference: released with the last graph
  std::recursive_mutex mu;                             // serialises the entry points of this context (CTX_ENTER)
  // profiling (mp_ctx_set_profiling): every device-pointer entry point brackets its launches with a timed HIP event pair
  // on the compute stream and an roctx range; the pairs are resolved when the figures are read (mp_ctx_profile)
  bool profiling = false;
  struct Pending { hipEvent_t a, b; };
  std::vector<Pending> prof_pending;
  double prof_total_ms = 0, prof_last_ms = 0;
  long long prof_launches = 0;
};
struct mp_event {
  hipEvent_t ev = nullptr;
  int device = -1;
};

struct mp_graph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  int device = -1;
  mp_ctx* ctx = nullptr;  // the context it was captured on (only dereferenced while that context is still registered ...
  uint64_t ctx_uid = 0;   // ... under the SAME never-reused id: a later context may be allocated at the same address)
  mp_ctx::HardPool* pool = nullptr;  // row lists + counters of the float64 passes captured in it
};

namespace {
thread_local char g_err[512] = "";  // what mp_set_error keeps for mp_last_error; every refusal goes through mp_fail (mp_handles.h)

int hip_err(hipError_t e, const char* what) {
  return mp_fail(MP_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
#define HIP_TRY(expr)                                   \
  do {                                                  \
    hipError_t e_ = (expr);                             \
    if (e_ != hipSuccess) return hip_err(e_, #expr);    \
  } while (0)

int bind(mp_ctx* ctx) {
  HIP_TRY(hipSetDevice(ctx->device));
  return MP_OK;
}
// Every entry point that touches a context starts with CTX_ENTER: it serialises the callers of one context (the pool,
// the specialisation table and the capture flag are plain containers; ctypes releases the GIL during a call, so
// Python threads sharing a planner do arrive concurrently - the reference runs its planners from several threads in
// tests/test_trajectory_planning.py:1375) and binds the calling thread to the context's device.  Recursive: the
// host-buffer entry points call the device-pointer ones.
// ... and runs the float64 passes that float32 inverse-dynamics launches have parked (hard_flush): whatever the entry point
// enqueues next may read the torques they write.  The float32 inverse-dynamics entry points, whose point it is NOT to run one
// pass per launch, enter with CTX_ENTER_NOJOIN and flush only when their arrays overlap a parked pass's.
int hard_flush(mp_ctx* ctx);
int hard_park_or_run(mp_ctx* ctx, const void* a, const void* b, const void* c, const void* out, size_t bytes_out, size_t bytes_in);
#define CTX_ENTER_NOJOIN(ctx)                                  \
  std::lock_guard<std::recursive_mutex> ctx_lock_((ctx)->mu);  \
  if (int rc_enter_ = bind(ctx)) return rc_enter_
#define CTX_ENTER(ctx)                                         \
  CTX_ENTER_NOJOIN(ctx);                                       \
  if (int rc_join_ = hard_flush(ctx)) return rc_join_
// every live context, so that mp_model_destroy can drop the per-context state of a model (specialised code object,
// device-resident copy) instead of leaving it to mp_ctx_destroy
std::mutex g_ctxs_mu;
std::set<mp_ctx*> g_ctxs;

// roctx ranges (rocprofv3 --marker-trace shows them): libroctx64 is dlopen'd on first use only, absent = no ranges
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    for (const char* name : {"libroctx64.so.4", "libroctx64.so", "/opt/rocm/lib/libroctx64.so"}) {
      if (void* h = dlopen(name, RTLD_NOW | RTLD_LOCAL)) {
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (push && pop) return;
        push = nullptr; pop = nullptr;
      }
    }
  }
};
const Roctx& roctx() { static const Roctx r; return r; }

// Scope of one device-pointer entry point when the context profiles: an roctx range named after the entry point and a
// timed HIP event pair around whatever it enqueues on the compute stream (the replacement of the reference's
// profile_start / CUDA profiler hooks, planning/trajectory_planning.py:295-296, cuda_kernels/_runtime.py).
struct KernelScope {
  mp_ctx* ctx;
  hipEvent_t a = nullptr, b = nullptr;
  bool ranged = false;
  KernelScope(mp_ctx* c, const char* name) : ctx(c) {
    if (!c->profiling || c->capturing) return;
    if (roctx().push) { roctx().push(name); ranged = true; }
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess || hipEventRecord(a, c->compute) != hipSuccess) {
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
      a = b = nullptr;
    }
  }
  ~KernelScope() {
    if (a && b) {
      if (hipEventRecord(b, ctx->compute) == hipSuccess) ctx->prof_pending.push_back({a, b});
      else { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
      // Nobody may ever read the figures (profiling is a flag of the shared context; other users of it never call
      // mp_ctx_profile): pairs that have completed are folded into the totals here, oldest first, once a few are pending,
      // so a long-lived process holds a bounded number of events.
      if (ctx->prof_pending.size() > 32) {
        size_t done = 0;
        while (done < ctx->prof_pending.size() && hipEventQuery(ctx->prof_pending[done].b) == hipSuccess) {
          float ms = 0.f;
          if (hipEventElapsedTime(&ms, ctx->prof_pending[done].a, ctx->prof_pending[done].b) == hipSuccess) {
            ctx->prof_total_ms += ms; ctx->prof_last_ms = ms; ctx->prof_launches += 1;
          }
          (void)hipEventDestroy(ctx->prof_pending[done].a);
          (void)hipEventDestroy(ctx->prof_pending[done].b);
          ++done;
        }
        (void)hipGetLastError();  // hipErrorNotReady of the first unfinished pair is not an error
        ctx->prof_pending.erase(ctx->prof_pending.begin(), ctx->prof_pending.begin() + (long)done);
      }
    }
    if (ranged) roctx().pop();
  }
};
#define PROFILE_SCOPE(ctx, name) KernelScope kernel_scope_((ctx), (name))

template <typename T>
void make_call(const mp_model* m, const double* g, const double* Ftip, MpCall<T>* c) {
  MpCall<double> cd;
  if (m->big) mp_make_call(m->bd, g ? g : kG, Ftip, &cd);
  else mp_make_call(m->d, g ? g : kG, Ftip, &cd);
  mp_call_cast(cd, c);
}

// RAII device scratch from the pool: the *_host entry points take theirs through HostCall, the self-checks directly
struct Scratch {
  mp_ctx* ctx;
  std::vector<void*> bufs;
  explicit Scratch(mp_ctx* c) : ctx(c) {}
  ~Scratch() { for (void* p : bufs) mp_free(ctx, p); }
  int get(size_t bytes, void** p) {
    int rc = mp_malloc(ctx, bytes ? bytes : 16, p);
    if (rc == MP_OK) bufs.push_back(*p);
    return rc;
  }
};
// rows per chunk of the host-buffer pipeline (MANIPULAPY_HIP_HOST_CHUNK_ROWS, default 512 Ki rows), rounded up to a
// multiple of 4: every chunk then starts on a 16-byte boundary for any row size (4 rows x n x 4 bytes), which the
// device-pointer entry points require, and only the last chunk can end on an odd row
int64_t host_chunk_rows() {
  static const int64_t rows = [] {
    const char* e = getenv("MANIPULAPY_HIP_HOST_CHUNK_ROWS");
    long long v = e ? atoll(e) : 0;
    if (v <= 0) v = 512 * 1024;
    return (int64_t)((v + 3) & ~3LL);
  }();
  return rows;
}
// true when `p` is page-locked host memory the device can DMA directly (mp_host_alloc, hipHostMalloc, hipHostRegister)
bool is_pinned_host(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // an ordinary pageable pointer is reported as an error: clear it
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

// events of one pipelined call, destroyed on every exit path
struct EventList {
  std::vector<hipEvent_t> evs;
  ~EventList() { for (hipEvent_t e : evs) (void)hipEventDestroy(e); }
  int make(hipEvent_t* out) {
    hipError_t he = hipEventCreateWithFlags(out, hipEventDisableTiming);
    if (he != hipSuccess) return hip_err(he, "hipEventCreate");
    evs.push_back(*out);
    return MP_OK;
  }
};
#define H2D(dst, src, bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->compute))
#define D2H(dst, src, bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->compute))


// MANIPULAPY_HIP_SPECIALIZE=0: ignore specialised kernels (A/B measurements)
bool specialize_enabled() {
  static const bool on = [] { const char* e = getenv("MANIPULAPY_HIP_SPECIALIZE"); return !(e && e[0] == '0'); }();
  return on;
}
const MpSpec* find_spec(mp_ctx* ctx, const mp_model* model) {
  if (!specialize_enabled()) return nullptr;
  auto it = ctx->specs.find(model->uid);
  return it == ctx->specs.end() ? nullptr : &it->second;
}
int launch_spec(mp_ctx* ctx, hipFunction_t fn, long threads, void** args, unsigned block = 256) {
  const unsigned grid = (unsigned)((threads + block - 1) / block);
  HIP_TRY(hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, 0, ctx->compute, args, nullptr));
  return MP_OK;
}

// While a capture is open on this thread (hipStreamCaptureModeThreadLocal) an allocation or a blocking copy is refused; the few
// that belong to a captured launch (its row list, a model's device copy on first use) run under the relaxed mode - they execute
// at once, outside the graph.
struct RelaxedCapture {
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  bool on;
  explicit RelaxedCapture(bool capturing) : on(capturing) { if (on) (void)hipThreadExchangeStreamCaptureMode(&mode); }
  ~RelaxedCapture() { if (on) (void)hipThreadExchangeStreamCaptureMode(&mode); }
};
// true when [p, p + bytes) lies inside one allocation of this context's pool (mp_malloc): memory the library owns, which no
// caller can read, free or hand to another allocator behind the library's back
bool pool_owned(mp_ctx* ctx, const void* p, size_t bytes) {
  if (!p) return true;
  auto it = ctx->live.upper_bound(const_cast<void*>(p));
  if (it == ctx->live.begin()) return false;
  --it;
  const char* base = (const char*)it->first;
  return (const char*)p >= base && (const char*)p + bytes <= base + it->second;
}
// float32 model resident in device memory (read by the *_dm kernels with scalar loads), followed in the same buffer by the
// float64 model (read by the float64 re-evaluation of ill-conditioned float32 rows in the generic kernels, MpCall::cold_model)
constexpr size_t kDevModelD = (sizeof(MpModel<float>) + 255) & ~(size_t)255;  // offset of the float64 copy
// ... and then the inertial-parameter map of the regressor (mp_model::pmap, csrc/mp_regressor.h)
constexpr size_t kDevModelMap = (kDevModelD + sizeof(MpModel<double>) + 255) & ~(size_t)255;
constexpr size_t kDevModelBytes = kDevModelMap + sizeof(mp_model::pmap);
int device_model(mp_ctx* ctx, const mp_model* model, const MpModel<float>** out) {
  auto it = ctx->dev_models.find(model->uid);
  if (it == ctx->dev_models.end()) {
    void* d = nullptr;
    if (ctx->capturing) {
      // first use inside a capture: the copy is made at once, outside the graph - on the context's upload stream (not capturing;
      // a blocking hipMemcpy would tie the legacy stream to the capturing one and is refused) and waited for, so the replays'
      // kernels - and the eager launches after the capture - find it
      RelaxedCapture relaxed(true);
      const size_t bytes = (kDevModelBytes + 255) & ~size_t(255);
      HIP_TRY(hipMalloc(&d, bytes));
      ctx->live[d] = bytes;
      hipError_t he = hipMemcpyAsync(d, &model->f, sizeof(MpModel<float>), hipMemcpyHostToDevice, ctx->copy);
      if (he == hipSuccess) he = hipMemcpyAsync((char*)d + kDevModelD, &model->d, sizeof(MpModel<double>), hipMemcpyHostToDevice, ctx->copy);
      if (he == hipSuccess) he = hipMemcpyAsync((char*)d + kDevModelMap, model->pmap, sizeof model->pmap, hipMemcpyHostToDevice, ctx->copy);
      if (he == hipSuccess) he = hipStreamSynchronize(ctx->copy);
      if (he != hipSuccess) { ctx->free_by_size[bytes].push_back(d); return hip_err(he, "device copy of the model (first use inside a capture)"); }
    } else {
      if (int rc = mp_malloc(ctx, kDevModelBytes, &d)) return rc;
      // (on the compute stream and waited for: the first kernel that reads the copy follows on that stream, and the streams are
      // non-blocking - nothing orders them with a copy on the null stream)
      HIP_TRY(hipMemcpyAsync(d, &model->f, sizeof(MpModel<float>), hipMemcpyHostToDevice, ctx->compute));
      HIP_TRY(hipMemcpyAsync((char*)d + kDevModelD, &model->d, sizeof(MpModel<double>), hipMemcpyHostToDevice, ctx->compute));
      HIP_TRY(hipMemcpyAsync((char*)d + kDevModelMap, model->pmap, sizeof model->pmap, hipMemcpyHostToDevice, ctx->compute));
      HIP_TRY(hipStreamSynchronize(ctx->compute));
    }
    it = ctx->dev_models.emplace(model->uid, d).first;
  }
  *out = static_cast<const MpModel<float>*>(it->second);
  return MP_OK;
}
// a float32 call's constants + where its kernels find the float64 model.  Generic kernels only (the specialised programs carry
// the literal); `generic_kernel`: the launch goes to a generic kernel even if the model is specialised (an entry that has no
// specialised float32 program, mp_fk_jac_id_f32) - without the float64 model its ill-conditioned rows would be re-evaluated
// with the float32 model's constants and differ from the same rows of the unspecialised model.
void make_call_f32(mp_ctx* ctx, const mp_model* model, const double* g, const double* Ftip, MpCall<float>* c, bool generic_kernel = false) {
  make_call<float>(model, g, Ftip, c);
  if (model->big || (!generic_kernel && find_spec(ctx, model))) return;
  auto it = ctx->dev_models.find(model->uid);
  if (it == ctx->dev_models.end()) {
    const MpModel<float>* dm = nullptr;
    if (device_model(ctx, model, &dm) != MP_OK) return;
    it = ctx->dev_models.find(model->uid);
  }
  if (it != ctx->dev_models.end()) c->cold_model = (const char*)it->second + kDevModelD;
}
// The list a float32 inverse-dynamics launch of `rows` rows leaves its ill-conditioned rows in for the float64 pass
// (csrc/mp_bodies.h, mp_push_hard_rows / mp_body_id_hard): room for one row in eight, at least 65 536 (c2-distributed rows flag 0.5 - 1.5 %; a list that
// overflows makes the pass evaluate every row of the launch).  Returns the slot (c carries its pointers), or null = no list, the
// kernels re-evaluate in place: more than 2^32 rows, or the switch.  A launch that is being CAPTURED takes its list from the
// capture's own pool (mp_graph_begin): the graph owns it, the pass is a node of the graph.
mp_ctx::HardSlot* attach_hard_list(mp_ctx* ctx, long rows, MpCall<float>* c) {
  // MANIPULAPY_HIP_HARD_PASS=0: no list - the path a launch of 2^32 rows or a failed list allocation takes (tested that way)
  static const bool on = !(getenv("MANIPULAPY_HIP_HARD_PASS") && getenv("MANIPULAPY_HIP_HARD_PASS")[0] == '0');
  if (!on || rows >= 0xffffffffL) return nullptr;
  mp_ctx::HardPool* pool = ctx->hp;
  mp_ctx::HardSlot* hs = nullptr;
  for (auto& cand : pool->slot)
    if (!cand.busy) { hs = &cand; break; }
  if (!hs) {  // all parked: run them (one kernel), then take the first
    if (hard_flush(ctx) != MP_OK) return nullptr;
    hs = &pool->slot[0];
  }
  const unsigned need = (unsigned)std::min<long>(std::max<long>(rows / 8, 1L << 16), 1L << 28);
  if (hs->cap < need) {
    RelaxedCapture relaxed(ctx->capturing);
    if (!ctx->capturing && hipStreamSynchronize(ctx->compute) != hipSuccess) return nullptr;
    // EVERY free slot of the pool gets its counters and a list of this size now, not only the one this launch takes: a slot's first
    // use in the middle of a run of launches put a stream synchronisation and two allocations between two 65 us kernels (round 5's
    // "cold" c2 figure, 0.08 - 0.12 ms against 0.065 sustained: profiles/r06_cold_before_windows.json - the kernels themselves
    // ran at their sustained duration).  A parked slot keeps its list (its pass reads it) and grows when it is next taken.
    // (zeroed ON the compute stream: a plain hipMemset of device memory is not ordered with a kernel launched on another,
    // non-blocking stream right behind it - a kernel that met the allocation's old bytes as its counter took the list for full and
    // re-evaluated in place, correct but not bit-equal to the pass: seen once, as 27 elements of a 240 000-element comparison.
    // In a capture this is the node that zeroes the graph's counters ahead of their first user, on every replay.)
    auto grow = [&](mp_ctx::HardSlot* s) -> bool {
      if (!s->ctrl && (hipMalloc((void**)&s->ctrl, 2 * sizeof(unsigned)) != hipSuccess ||
                       hipMemsetAsync(s->ctrl, 0, 2 * sizeof(unsigned), ctx->compute) != hipSuccess)) {
        s->ctrl = nullptr;
        return false;
      }
      if (s->rows && ctx->capturing) pool->retired.push_back(s->rows);  // earlier nodes of the graph still write it
      else if (s->rows) (void)hipFree(s->rows);
      s->rows = nullptr; s->cap = 0;
      if (hipMalloc((void**)&s->rows, (size_t)need * sizeof(unsigned)) != hipSuccess) { s->rows = nullptr; return false; }
      s->cap = need;
      return true;
    };
    if (!grow(hs)) return nullptr;
    for (auto& other : pool->slot)
      if (&other != hs && !other.busy && other.cap < need && !grow(&other)) break;  // (a slot left small grows when it is taken)
  }
  if (hs->orphan && hipMemsetAsync(hs->ctrl, 0, 2 * sizeof(unsigned), ctx->compute) != hipSuccess) return nullptr;
  hs->orphan = true;  // until its pass is parked (hard_defer) or launched (hard_passed)
  const unsigned turn = hs->uses++ & 1u;
  c->hard_rows = hs->rows; c->hard_ctrl = hs->ctrl + turn; c->hard_next = hs->ctrl + (turn ^ 1u); c->hard_cap = hs->cap;
  c->hard_row_base = 0;
  return hs;
}
void free_hard_pool(mp_ctx::HardPool* pool) {
  for (auto& hs : pool->slot) {
    if (hs.rows) (void)hipFree(hs.rows);
    if (hs.ctrl) (void)hipFree(hs.ctrl);
    hs.rows = nullptr; hs.ctrl = nullptr; hs.cap = 0; hs.busy = false; hs.gen_dm = nullptr;
  }
  for (void* p : pool->retired) (void)hipFree(p);
  pool->retired.clear();
}
unsigned hard_pass_blocks(long rows) {
  return (unsigned)std::min<long>((rows / 8 + 63) / 64 + 1, 1024L);
}
// the pass of the list's launch has been enqueued directly (the fused paths); returns rc for tail calls
inline int hard_passed(mp_ctx::HardSlot* hs, int rc) {
  if (rc == MP_OK) hs->orphan = false;
  return rc;
}
// park the pass of the launch just enqueued
void hard_defer(mp_ctx* ctx, mp_ctx::HardSlot* hs, hipFunction_t fn, const MpModel<float>* gen_dm, bool gen_ftip, const MpCall<float>& C,
                const float* q, const float* qd, const float* qdd, float* tau, long rows, int n) {
  hs->busy = true; hs->orphan = false; hs->seq = ++ctx->hp->seq; hs->fn = fn; hs->gen_dm = gen_dm; hs->gen_n = n; hs->gen_ftip = gen_ftip;
  hs->C = C; hs->C.hard_row_base = 0;
  hs->q = q; hs->qd = qd; hs->qdd = qdd; hs->tau = tau; hs->nrows = (unsigned)rows; hs->bytes = (size_t)rows * (size_t)n * sizeof(float);
  hs->bytes_in = hs->bytes; hs->nt = 0;
}
// ... of a fused launch: its rows are generated from B start / end points and the context's time table, which therefore must
// not be rewritten while the pass is parked (mp_traj_id_fused_f32 runs the parked passes before it touches the table)
void hard_defer_generated(mp_ctx* ctx, mp_ctx::HardSlot* hs, hipFunction_t fn, const MpCall<float>& C, const float* start, const float* end,
                          const double* tab, float* tau, long rows, int n, long B, unsigned nt) {
  hard_defer(ctx, hs, fn, nullptr, false, C, start, end, (const float*)tab, tau, rows, n);
  hs->bytes_in = (size_t)B * (size_t)n * sizeof(float); hs->nt = nt;
}
// What becomes of the pass just parked.  It STAYS parked only when every array of its launch lies in this context's pool: such
// memory is read, freed and reused through the library alone, and every entry point runs the parked passes first.  Arrays the
// caller allocated itself (hipMalloc, a framework tensor) may be read with the caller's own HIP calls on the compute stream, or
// handed back to another allocator, without the library hearing of it - their pass is enqueued at once, so that the entry point
// returns with the complete result stream-ordered behind it, as the reference's launchers return finished arrays
// (cuda_kernels/trajectory_kernels.py:1043-1081).
int hard_park_or_run(mp_ctx* ctx, const void* a, const void* b, const void* c, const void* out, size_t bytes_out, size_t bytes_in) {
  // ... and once the caller holds the compute stream (mp_ctx_get_stream) it can read pool memory too - mp_malloc returns a plain device
  // pointer - with a copy or a kernel of its own on that stream, behind the library's back: from then on nothing stays parked
  if (!ctx->stream_exported && pool_owned(ctx, a, bytes_in) && pool_owned(ctx, b, bytes_in) && pool_owned(ctx, c, bytes_in) && pool_owned(ctx, out, bytes_out))
    return MP_OK;
  return hard_flush(ctx);
}
// run every parked pass on the compute stream, in launch order; passes of one specialised program share a kernel launch
int hard_flush(mp_ctx* ctx) {
  mp_ctx::HardSlot* order[mp_ctx::kHardSlots];
  int k = 0;
  for (auto& hs : ctx->hp->slot)
    if (hs.busy) order[k++] = &hs;
  if (k == 0) return MP_OK;
  std::sort(order, order + k, [](const mp_ctx::HardSlot* a, const mp_ctx::HardSlot* b) { return a->seq < b->seq; });
  int rc = MP_OK;
  for (int i = 0; i < k;) {
    mp_ctx::HardSlot* h = order[i];
    MpHardBatch B;
    std::memset(&B, 0, sizeof B);
    mp_ctx::HardSlot* ent[MP_HARD_BATCH];
    int m = 0;
    unsigned blocks = 1;
    // passes of one program - a specialised one (fn), or the generic kernel of one (device model, joint count, wrench) - share a launch
    auto same = [&](const mp_ctx::HardSlot* o) {
      return o->fn == h->fn && (h->fn || (o->gen_dm == h->gen_dm && o->gen_n == h->gen_n && o->gen_ftip == h->gen_ftip));
    };
    while (i < k && same(order[i]) && m < MP_HARD_BATCH) {
      mp_ctx::HardSlot* e = order[i++];
      B.C[m] = e->C; B.q[m] = e->q; B.qd[m] = e->qd; B.qdd[m] = e->qdd; B.tau[m] = e->tau; B.rows[m] = e->nrows; B.nt[m] = e->nt;
      blocks = std::max(blocks, hard_pass_blocks((long)e->nrows));
      e->busy = false;
      ent[m++] = e;
    }
    if (rc == MP_OK) {
      void* args[] = {&B};
      hipError_t he = h->fn ? hipModuleLaunchKernel(h->fn, blocks, (unsigned)m, 1, 64, 1, 1, 0, ctx->compute, args, nullptr)
                            : mpk_id_hard_batch(ctx->compute, h->gen_dm, h->gen_n, h->gen_ftip, B, m, blocks);
      if (he != hipSuccess) rc = hip_err(he, "float64 pass of the ill-conditioned float32 rows");
    }
    for (int j = 0; j < m; ++j) ent[j]->orphan = rc != MP_OK;  // a pass that did not run leaves its list's counters as they are
  }
  return rc;
}
// a float32 launch about to be enqueued on [lo, lo + bytes) arrays: parked passes run first if they read or write what it writes, or
// write what it reads
int hard_flush_if_overlapping(mp_ctx* ctx, const void* const* lo, const size_t* bytes, int k) {
  for (auto& hs : ctx->hp->slot) {
    if (!hs.busy) continue;
    const char* mine[4] = {(const char*)hs.q, (const char*)hs.qd, hs.nt ? nullptr : (const char*)hs.qdd, (const char*)hs.tau};
    const size_t size[4] = {hs.bytes_in, hs.bytes_in, hs.bytes_in, hs.bytes};
    for (int i = 0; i < k; ++i) {  // lo[k - 1] is the array the launch WRITES, the others it reads: two reads do not conflict
      const char* a = (const char*)lo[i];
      if (!a) continue;
      for (int j = i == k - 1 ? 0 : 3; j < 4; ++j)
        if (mine[j] && a < mine[j] + size[j] && mine[j] < a + bytes[i]) return hard_flush(ctx);
    }
  }
  return MP_OK;
}
// A parked float64 pass rides with the next float32 launch of its program (the launch's first workgroups work it off) instead of
// waiting for a kernel of its own: both specialised kernels host the path - the fused one (two waves per SIMD by design: the float64
// recursion's registers are free) and the given-rows one (held to its five waves: the carried path spills to scratch, csrc/mp_jit.cpp)
// - and so does the generic k_id_dm.  (A/B against passes as kernels of their own: profiles/r05_ab_e.txt, r05_ab_g.txt.)
// the parked pass (given rows, specialised program `fn`) a launch may carry: the oldest; `self` is the launch's own slot
mp_ctx::HardSlot* pick_rider(mp_ctx* ctx, hipFunction_t fn, const mp_ctx::HardSlot* self, bool generated = false) {
  mp_ctx::HardSlot* best = nullptr;
  for (auto& hs : ctx->hp->slot)
    if (hs.busy && &hs != self && hs.fn == fn && fn && (hs.nt != 0) == generated && (!best || hs.seq < best->seq)) best = &hs;
  return best;
}
template <typename T>
void make_call_ctx(mp_ctx* ctx, const mp_model* model, const double* g, const double* Ftip, MpCall<T>* c, bool generic_kernel = false);
template <>
void make_call_ctx<float>(mp_ctx* ctx, const mp_model* model, const double* g, const double* Ftip, MpCall<float>* c, bool generic_kernel) {
  make_call_f32(ctx, model, g, Ftip, c, generic_kernel);
}
template <> void make_call_ctx<double>(mp_ctx*, const mp_model* model, const double* g, const double* Ftip, MpCall<double>* c, bool) {
  make_call<double>(model, g, Ftip, c);
}

// MpBigModel<T> of a 9..32-joint model resident in device memory (read by the looped k_dyn_* kernels through scalar loads)
template <typename T>
int device_big_model(mp_ctx* ctx, const mp_model* model, const MpBigModel<T>** out) {
  auto& table = ctx->dev_big[sizeof(T) == 8 ? 1 : 0];
  auto it = table.find(model->uid);
  if (it == table.end()) {
    REQUIRE(!ctx->capturing, "a model with more than %d joints is uploaded on first use: call once before capturing a launch graph", MP_MAX_DOF);
    void* d = nullptr;
    if (int rc = mp_malloc(ctx, sizeof(MpBigModel<T>), &d)) return rc;
    HIP_TRY(hipMemcpyAsync(d, &pick_big<T>(model), sizeof(MpBigModel<T>), hipMemcpyHostToDevice, ctx->compute));  // (as device_model)
    HIP_TRY(hipStreamSynchronize(ctx->compute));
    it = table.emplace(model->uid, d).first;
  }
  *out = static_cast<const MpBigModel<T>*>(it->second);
  return MP_OK;
}
// float32 calls on a 9..32-joint model: where the kernels find the float64 model for their ill-conditioned rows (mp_dyn.h,
// mp_dyn_row_id_f64); float64 calls need nothing
int big_cold_model(mp_ctx* ctx, const mp_model* model, MpCall<float>* c) {
  const MpBigModel<double>* dd = nullptr;
  if (int rc = device_big_model<double>(ctx, model, &dd)) return rc;
  c->cold_model = dd;
  return MP_OK;
}
int big_cold_model(mp_ctx*, const mp_model*, MpCall<double>*) { return MP_OK; }

template <typename T>
int launch_big_fk_jac_id(mp_ctx* ctx, const mp_model* model, const MpCall<T>& c, bool ftip, const T* q, const T* qd, const T* qdd, T* Tout,
                         T* Jout, T* tau, long rows) {
  const MpBigModel<T>* dm = nullptr;
  if (int rc = device_big_model<T>(ctx, model, &dm)) return rc;
  MpCall<T> cc = c;
  if (int rc = big_cold_model(ctx, model, &cc)) return rc;
  HIP_TRY(mpk_dyn_fk_jac_id<T>(ctx->compute, model->d.n, dm, cc, ftip, q, qd, qdd, Tout, Jout, tau, rows));
  return MP_OK;
}

int launch_id(mp_ctx* ctx, const mp_model* model, const MpCall<double>& c, bool ftip, const double* q, const double* qd,
              const double* qdd, double* tau, long rows) {
  if (model->big) return launch_big_fk_jac_id<double>(ctx, model, c, ftip, q, qd, qdd, nullptr, nullptr, tau, rows);
  if (const MpSpec* sp = find_spec(ctx, model)) {
    MpCall<double> cc = c;
    void* args[] = {&cc, &q, &qd, &qdd, &tau, &rows};
    return launch_spec(ctx, sp->id_d[ftip ? 1 : 0], rows, args);
  }
  HIP_TRY(mpk_id<double>(ctx->compute, model->d, c, ftip, q, qd, qdd, tau, rows));
  return MP_OK;
}
int launch_id(mp_ctx* ctx, const mp_model* model, const MpCall<float>& c, bool ftip, const float* q, const float* qd,
              const float* qdd, float* tau, long rows) {
  if (model->big) return launch_big_fk_jac_id<float>(ctx, model, c, ftip, q, qd, qdd, nullptr, nullptr, tau, rows);
  if (const MpSpec* sp = find_spec(ctx, model)) {
    // one row per lane in scalar arithmetic (a wave64 v_fma_f32 holds its SIMD for 2 cycles, a packed one for 4: the two-rows-per-lane
    // form measured 5 - 7.5 % slower and was removed in round 6)
    MpCall<float> cc = c;
    // ill-conditioned rows go to a float64 pass of their own behind the float32 kernels (see attach_hard_list)
    mp_ctx::HardSlot* hs = attach_hard_list(ctx, rows, &cc);
    auto hard_pass = [&]() -> int {
      if (!hs) return MP_OK;
      hard_defer(ctx, hs, sp->id_hard[ftip ? 1 : 0], nullptr, false, cc, q, qd, qdd, tau, rows, model->d.n);
      return hard_park_or_run(ctx, q, qd, qdd, tau, (size_t)rows * (size_t)model->d.n * sizeof(float), (size_t)rows * (size_t)model->d.n * sizeof(float));
    };
    long done = 0;
    if (rows >= 64) {  // whole waves: rows moved as whole lines, non-temporal (mp_body_id_co)
      long rows64 = rows & ~63L;
      // One float64 pass that is still parked - an earlier launch's of the same program, none of whose arrays this launch
      // touches (the others were run by hard_flush_if_overlapping on the way in) - rides with this launch: its first workgroups
      // work the list off beside the float32 rows (mp_body_id_lead) instead of a kernel of its own doing so later.
      MpLead lead;
      std::memset(&lead, 0, sizeof lead);
      mp_ctx::HardSlot* rider = pick_rider(ctx, sp->id_hard[ftip ? 1 : 0], hs);
      if (rider) {
        lead.C = rider->C; lead.q = rider->q; lead.qd = rider->qd; lead.qdd = rider->qdd; lead.tau = rider->tau; lead.rows = rider->nrows;
        lead.blocks = std::min(hard_pass_blocks((long)rider->nrows), 512u);
      }
      const unsigned grid = (unsigned)(rows64 / MP_JIT_ID_CO_BLOCK) + lead.blocks;
      void* args[] = {&cc, &q, &qd, &qdd, &tau, &rows64, &lead};
      HIP_TRY(hipModuleLaunchKernel(sp->id_co[ftip ? 1 : 0], grid, 1, 1, MP_JIT_ID_CO_BLOCK, 1, 1, 0, ctx->compute, args, nullptr));
      if (rider) { rider->busy = false; rider->orphan = false; }   // its pass is enqueued: the slot is free for the next launch
      done = rows64;
    }
    if (done == rows) return hard_pass();
    const long off = done * model->d.n;  // the last rows (< 64): per-lane rows
    const float *q2 = q + off, *qd2 = qd + off, *qdd2 = qdd + off;
    float* tau2 = tau + off;
    long left = rows - done;
    cc.hard_row_base = (unsigned)done;
    void* args[] = {&cc, &q2, &qd2, &qdd2, &tau2, &left};
    if (int rc = launch_spec(ctx, sp->id_s[ftip ? 1 : 0], left, args)) return rc;
    return hard_pass();
  }
  {  // generic: one row per lane, device-resident model (a capture's first use uploads it outside the graph)
    const MpModel<float>* dm = nullptr;
    if (int rc = device_model(ctx, model, &dm)) return rc;
    MpCall<float> cc = c;
    mp_ctx::HardSlot* hs = cc.cold_model ? attach_hard_list(ctx, rows, &cc) : nullptr;
    // (as the specialised kernels: one parked pass of an earlier launch of this model rides with this launch's first workgroups)
    MpLead lead;
    std::memset(&lead, 0, sizeof lead);
    mp_ctx::HardSlot* rider = nullptr;
    for (auto& cand : ctx->hp->slot)
      if (cand.busy && &cand != hs && !cand.fn && cand.gen_dm == dm && cand.gen_n == model->d.n && cand.gen_ftip == ftip && cand.nt == 0 &&
          cand.C.cold_model && (!rider || cand.seq < rider->seq))
        rider = &cand;
    if (rider) {
      lead.C = rider->C; lead.q = rider->q; lead.qd = rider->qd; lead.qdd = rider->qdd; lead.tau = rider->tau; lead.rows = rider->nrows;
      lead.blocks = std::min((hard_pass_blocks((long)rider->nrows) + 3u) / 4u, 128u);   // 256-lane workgroups
    }
    bool all_rev = true;   // revolute joints only: the kernel instance without the revolute / prismatic blend (csrc/mp_model.h, MpModelRev)
    for (int i = 0; i < model->d.n; ++i) all_rev = all_rev && model->f.j[i].rev == 1.0f;
    HIP_TRY(mpk_id_dm(ctx->compute, dm, model->d.n, cc, ftip, q, qd, qdd, tau, rows, lead, all_rev));
    if (rider) { rider->busy = false; rider->orphan = false; }
    if (!hs) return MP_OK;
    const int n = model->d.n;
    hard_defer(ctx, hs, nullptr, dm, ftip, cc, q, qd, qdd, tau, rows, n);
    return hard_park_or_run(ctx, q, qd, qdd, tau, (size_t)rows * (size_t)n * sizeof(float), (size_t)rows * (size_t)n * sizeof(float));
  }
}

// template bodies shared by the f32 / f64 entry points (C++ linkage)
template <typename T>
static int id_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const T* d_q, const T* d_qd, const T* d_qdd,
                   int64_t rows, const double* g, const double* Ftip, T* d_tau) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER_NOJOIN(ctx);
  {  // pending float64 passes: only those that may still write rows this launch reads or writes make the compute stream wait
    const size_t nb = (size_t)(rows > 0 ? rows : 0) * (size_t)model->d.n * sizeof(T);
    const void* lo[4] = {d_q, d_qd, d_qdd, d_tau};
    const size_t by[4] = {nb, nb, nb, nb};
    if (int rc = (sizeof(T) == 4 && !ctx->profiling) ? hard_flush_if_overlapping(ctx, lo, by, 4) : hard_flush(ctx)) return rc;
  }
  REQUIRE(rows >= 0, "%s: negative row count %lld", fn, (long long)rows);
  if (rows == 0) return MP_OK;
  REQUIRE(d_q && d_qd && d_qdd && d_tau, "%s: null device pointer", fn);
  REQUIRE(aligned16(d_q) && aligned16(d_qd) && aligned16(d_qdd) && aligned16(d_tau),
          "%s: device pointers must be 16-byte aligned", fn);
  MpCall<T> c;
  make_call_ctx<T>(ctx, model, g, Ftip, &c);
  PROFILE_SCOPE(ctx, fn);
  return launch_id(ctx, model, c, any_nonzero(Ftip), d_q, d_qd, d_qdd, d_tau, (long)rows);
}

// specialised FK + Jacobian + ID (float64 only): -1 = none available, otherwise the launch's return code
int launch_fkjid_spec(mp_ctx* ctx, const mp_model* model, const MpCall<double>& c, bool ftip, const double* q, const double* qd,
                      const double* qdd, double* T, double* J, double* tau, long rows) {
  const MpSpec* sp = find_spec(ctx, model);
  if (!sp) return -1;
  MpCall<double> cc = c;
  void* args[] = {&cc, &q, &qd, &qdd, &T, &J, &tau, &rows};
  return launch_spec(ctx, sp->fk_jac_id_d[ftip ? 1 : 0], rows, args, 64);  // one wave per block (per-wave LDS slice)
}
int launch_fkjid_spec(mp_ctx*, const mp_model*, const MpCall<float>&, bool, const float*, const float*, const float*, float*, float*,
                      float*, long) {
  return -1;
}

template <typename T>
static int fkjid_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const T* d_q, const T* d_qd, const T* d_qdd,
                      int64_t rows, const double* g, const double* Ftip, T* d_T, T* d_J, T* d_tau) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE(rows >= 0, "%s: negative row count %lld", fn, (long long)rows);
  if (rows == 0) return MP_OK;
  REQUIRE(d_q, "%s: null d_q", fn);
  REQUIRE(d_T || d_J || d_tau, "%s: at least one output is required", fn);
  REQUIRE(!d_tau || (d_qd && d_qdd), "%s: d_tau requested without d_qd / d_qdd", fn);
  REQUIRE(aligned16(d_q) && aligned16(d_qd) && aligned16(d_qdd) && aligned16(d_T) && aligned16(d_J) && aligned16(d_tau),
          "%s: device pointers must be 16-byte aligned", fn);
  MpCall<T> c;
  make_call_ctx<T>(ctx, model, g, Ftip, &c, /*generic_kernel=*/sizeof(T) == 4);   // (float32: no specialised program, see below)
  PROFILE_SCOPE(ctx, fn);
  if (model->big) return launch_big_fk_jac_id<T>(ctx, model, c, any_nonzero(Ftip), d_q, d_qd, d_qdd, d_T, d_J, d_tau, (long)rows);
  const int src = launch_fkjid_spec(ctx, model, c, any_nonzero(Ftip), d_q, d_qd, d_qdd, d_T, d_J, d_tau, (long)rows);
  if (src >= 0) return src;
  HIP_TRY(mpk_fk_jac_id<T>(ctx->compute, pick<T>(model), c, any_nonzero(Ftip), d_q, d_qd, d_qdd, d_T, d_J, d_tau, (long)rows));
  return MP_OK;
}

// Chunked three-stage pipeline over `rows` rows in chunks of `chunk`: `up(r0, nr)` queues the uploads of a chunk on the
// copy stream, `run(r0, nr)` launches its kernels on the compute stream, `down(r0, nr)` queues its downloads on the
// copy-out stream; events order the stages of one chunk, so the upload of chunk k+1, the kernels of chunk k and the
// download of chunk k-1 overlap (PCIe is full duplex: with page-locked buffers a call costs about its larger
// direction).  Every stage is drained before returning, also on the error path.
template <class Up, class Run, class Down>
static int host_pipeline(mp_ctx* ctx, int64_t rows, int64_t chunk, Up up, Run run, Down down) {
  EventList ev;
  auto body = [&]() -> int {
    // The scratch blocks of this call come from the pool, whose reuse is ordered with respect to the COMPUTE stream
    // only: work still pending there (an asynchronous device-pointer call whose buffer the caller has already freed)
    // must finish before the copy streams may overwrite a recycled block.
    hipEvent_t tail = nullptr;
    if (int rc = ev.make(&tail)) return rc;
    HIP_TRY(hipEventRecord(tail, ctx->compute));
    HIP_TRY(hipStreamWaitEvent(ctx->copy, tail, 0));
    HIP_TRY(hipStreamWaitEvent(ctx->copy_out, tail, 0));
    for (int64_t r0 = 0; r0 < rows; r0 += chunk) {
      const int64_t nr = std::min(chunk, rows - r0);
      hipEvent_t uploaded = nullptr, done = nullptr;
      if (int rc = ev.make(&uploaded)) return rc;
      if (int rc = ev.make(&done)) return rc;
      if (int rc = up(r0, nr)) return rc;
      HIP_TRY(hipEventRecord(uploaded, ctx->copy));
      HIP_TRY(hipStreamWaitEvent(ctx->compute, uploaded, 0));
      if (int rc = run(r0, nr)) return rc;
      HIP_TRY(hipEventRecord(done, ctx->compute));
      HIP_TRY(hipStreamWaitEvent(ctx->copy_out, done, 0));
      if (int rc = down(r0, nr)) return rc;
    }
    return MP_OK;
  };
  const int rc = body();
  (void)hipStreamSynchronize(ctx->copy);
  (void)hipStreamSynchronize(ctx->compute);
  const hipError_t he = hipStreamSynchronize(ctx->copy_out);
  if (rc == MP_OK && he != hipSuccess) return hip_err(he, "hipStreamSynchronize");
  return rc;
}
#define UP(dst, src, bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->copy))
#define DOWN(dst, src, bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->copy_out))

// Device staging of one *_host call.  The entry point declares every host array once and gets its device pointer back; an absent
// (null) host array maps to a null device pointer and moves nothing.  A failed allocation or copy is kept in `rc`: what follows it
// becomes a no-op, so call sites check nothing, and run() / run_rows() / finish() - an entry's only exit - return the first error.
// On every path, failure included, they drain the compute stream (the pipeline: its three streams), so no transfer to or from the
// caller's arrays is pending when the entry returns.
//   in / out / inout     whole arrays: uploaded at once / downloaded by finish(), in the order they were declared
//   in_tm / out_tm       the same for batch-major host arrays whose device copy is time-major: through the stage block (stage(),
//                        asked for once at the largest size that passes through it) and mp_transpose_rows, in stream order
//   in_rows / out_rows   arrays of `rows` rows, moved by run_rows()
//   work                 scratch only (0 bytes still yields a valid 16-byte block)
// The blocks come from the pool and go back to it with the object; the pool's reuse is ordered on the compute stream (Scratch).
struct HostCall {
  mp_ctx* ctx;
  int rc = MP_OK;
  explicit HostCall(mp_ctx* c, int64_t rows = 0) : ctx(c), sc(c), nrows(rows) {}

  template <class T = void> T* work(size_t bytes) {
    void* p = nullptr;
    if (rc == MP_OK) rc = sc.get(bytes, &p);
    return static_cast<T*>(p);
  }
  template <class T> const T* in(const T* host, size_t bytes) {
    T* d = host ? work<T>(bytes) : nullptr;
    if (d) upload(d, host, bytes);
    return d;
  }
  template <class T> T* out(T* host, size_t bytes) {
    T* d = host ? work<T>(bytes) : nullptr;
    if (d) outs.push_back({host, d, bytes, 0, 0});
    return d;
  }
  template <class T> T* inout(T* host, size_t bytes) {
    T* d = out(host, bytes);
    if (d) upload(d, host, bytes);
    return d;
  }
  void stage(size_t bytes) { staged = work(bytes); }
  // host (outer, inner, row) -> device (inner, outer, row)
  template <class T> const T* in_tm(const T* host, int64_t outer, int64_t inner, size_t row) {
    T* d = host ? work<T>((size_t)(outer * inner) * row) : nullptr;
    if (d) upload_tm(d, host, outer, inner, row);
    return d;
  }
  // device (outer, inner, row) -> host (inner, outer, row)
  template <class T> T* out_tm(T* host, int64_t outer, int64_t inner, size_t row) {
    T* d = host ? work<T>((size_t)(outer * inner) * row) : nullptr;
    if (d) outs.push_back({host, d, row, outer, inner});
    return d;
  }
  template <class T> const T* in_rows(const T* host, size_t row_bytes) {
    T* d = host ? work<T>((size_t)nrows * row_bytes) : nullptr;
    if (d) by_row.push_back({(char*)const_cast<T*>(host), (char*)d, row_bytes, false});
    return d;
  }
  template <class T> T* out_rows(T* host, size_t row_bytes) {
    T* d = host ? work<T>((size_t)nrows * row_bytes) : nullptr;
    if (d) by_row.push_back({(char*)host, (char*)d, row_bytes, true});
    return d;
  }

  // the transfers themselves, on the compute stream (an entry that moves its arrays piecewise calls them directly)
  void upload(void* dst, const void* src, size_t bytes) {
    step([&]() -> int { H2D(dst, src, bytes); return MP_OK; });
  }
  void download(void* dst, const void* src, size_t bytes) {
    step([&]() -> int { D2H(dst, src, bytes); return MP_OK; });
  }
  void upload_tm(void* dst, const void* src, int64_t outer, int64_t inner, size_t row) {
    upload(staged, src, (size_t)(outer * inner) * row);
    step([&] { return mp_transpose_rows(ctx, staged, outer, inner, (int64_t)row, dst); });
  }
  void download_tm(void* dst, const void* src, int64_t outer, int64_t inner, size_t row) {
    step([&] { return mp_transpose_rows(ctx, src, outer, inner, (int64_t)row, staged); });
    download(dst, staged, (size_t)(outer * inner) * row);
  }

  template <class F> void step(F f) {
    if (rc == MP_OK) rc = f();
  }
  // The parked float64 passes run before the downloads read their torques.  Only the float32 inverse-dynamics and fused entries
  // park one; for every other entry CTX_ENTER flushed on the way in and its launches park nothing, so the call finds no busy slot
  // and returns.
  int finish() {
    step([&] { return hard_flush(ctx); });
    for (const Out& o : outs) {
      if (o.outer) download_tm(o.host, o.dev, o.outer, o.inner, o.bytes);
      else download(o.host, o.dev, o.bytes);
    }
    const hipError_t he = hipStreamSynchronize(ctx->compute);
    if (rc == MP_OK && he != hipSuccess) rc = hip_err(he, "hipStreamSynchronize(ctx->compute)");
    return rc;
  }
  template <class F> int run(F launch) {
    step(launch);
    return finish();
  }
  // launch(r0, nr) works on rows [r0, r0 + nr) of the row-declared arrays (device pointers of row r0: at()).
  // Page-locked arrays throughout and at least `min_rows` rows: the rows are cut into chunks of `chunk` and the three stages
  // overlap - upload of chunk k+1 (copy stream), kernels of chunk k (compute stream), download of chunk k-1 (copy-out stream);
  // events order the stages of one chunk (host_pipeline).  PCIe is full duplex, so the call costs about its larger direction.
  // Pageable buffers are staged by the runtime on the calling thread, which serialises the stages anyway (measured: chunking then
  // costs 8 %), so only page-locked calls are chunked; every other call is one upload, one launch, one download.
  template <class F> int run_rows(int64_t chunk, int64_t min_rows, F launch) {
    bool pipelined = rc == MP_OK && nrows >= min_rows;
    for (const Rows& a : by_row) pipelined = pipelined && is_pinned_host(a.host);
    if (!pipelined) {
      for (const Rows& a : by_row) {
        if (a.down) outs.push_back({a.host, a.dev, (size_t)nrows * a.row, 0, 0});
        else upload(a.dev, a.host, (size_t)nrows * a.row);
      }
      return run([&] { return launch((int64_t)0, nrows); });
    }
    return rc = host_pipeline(
               ctx, nrows, chunk,
               [&](int64_t r0, int64_t nr) -> int {
                 for (const Rows& a : by_row)
                   if (!a.down) UP(a.dev + r0 * a.row, a.host + r0 * a.row, nr * a.row);
                 return MP_OK;
               },
               [&](int64_t r0, int64_t nr) -> int {
                 if (int e = launch(r0, nr)) return e;
                 return hard_flush(ctx);  // (as in finish(): the chunk's download follows)
               },
               [&](int64_t r0, int64_t nr) -> int {
                 for (const Rows& a : by_row)
                   if (a.down) DOWN(a.host + r0 * a.row, a.dev + r0 * a.row, nr * a.row);
                 return MP_OK;
               });
  }

 private:
  struct Out { void *host, *dev; size_t bytes; int64_t outer, inner; };  // outer != 0: out_tm, `bytes` is its row
  struct Rows { char *host, *dev; size_t row; bool down; };
  Scratch sc;
  int64_t nrows;
  void* staged = nullptr;
  std::vector<Out> outs;
  std::vector<Rows> by_row;
};
// `p` advanced by `elems` elements; null stays null (an array that was not asked for)
template <class T> T* at(T* p, int64_t elems) { return p ? p + elems : nullptr; }

template <typename T>
static int id_host_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const T* q, const T* qd, const T* qdd,
                        int64_t rows, const double* g, const double* Ftip, T* tau) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  if (rows == 0) return MP_OK;
  REQUIRE(q && qd && qdd && tau, "%s: null host pointer", fn);
  const int64_t n = model->d.n;
  HostCall h(ctx, rows);
  const T *dq = h.in_rows(q, n * sizeof(T)), *dqd = h.in_rows(qd, n * sizeof(T)), *dqdd = h.in_rows(qdd, n * sizeof(T));
  T* dt = h.out_rows(tau, n * sizeof(T));
  const int64_t chunk = host_chunk_rows();  // pipelined from two chunks on
  return h.run_rows(chunk, chunk + 1, [&](int64_t r0, int64_t nr) {
    return id_impl<T>(fn, ctx, model, dq + r0 * n, dqd + r0 * n, dqdd + r0 * n, nr, g, Ftip, dt + r0 * n);
  });
}

template <typename T>
static int mm_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const T* d_q, int64_t rows, T* d_M) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  if (rows == 0) return MP_OK;
  REQUIRE(d_q && d_M, "%s: null device pointer", fn);
  REQUIRE(aligned16(d_q) && aligned16(d_M), "%s: device pointers must be 16-byte aligned", fn);
  PROFILE_SCOPE(ctx, fn);
  if (model->big) {
    const MpBigModel<T>* dm = nullptr;
    if (int rc = device_big_model<T>(ctx, model, &dm)) return rc;
    HIP_TRY(mpk_dyn_mass_matrix<T>(ctx->compute, model->d.n, dm, d_q, d_M, (long)rows));
    return MP_OK;
  }
  HIP_TRY(mpk_mass_matrix<T>(ctx->compute, pick<T>(model), d_q, d_M, (long)rows));
  return MP_OK;
}

template <typename T>
static int fdyn_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const T* d_q, const T* d_qd, const T* d_tau,
                     int64_t rows, const double* g, const double* Ftip, T* d_qdd) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  if (rows == 0) return MP_OK;
  REQUIRE(d_q && d_qd && d_tau && d_qdd, "%s: null device pointer", fn);
  REQUIRE(aligned16(d_q) && aligned16(d_qd) && aligned16(d_tau) && aligned16(d_qdd), "%s: device pointers must be 16-byte aligned", fn);
  MpCall<T> c;
  make_call<T>(model, g, Ftip, &c);
  const bool ftip = any_nonzero(Ftip);
  PROFILE_SCOPE(ctx, fn);
  if (model->big) {
    const MpBigModel<T>* dm = nullptr;
    if (int rc = device_big_model<T>(ctx, model, &dm)) return rc;
    HIP_TRY(mpk_dyn_forward_dynamics<T>(ctx->compute, model->d.n, dm, c, ftip, d_q, d_qd, d_tau, d_qdd, (long)rows));
    return MP_OK;
  }
  if (const MpSpec* sp = find_spec(ctx, model)) {
    long nr = (long)rows;
    void* args[] = {&c, &d_q, &d_qd, &d_tau, &d_qdd, &nr};
    return launch_spec(ctx, (sizeof(T) == 4 ? sp->fd_s : sp->fd_d)[ftip ? 1 : 0], nr, args);
  }
  HIP_TRY(mpk_forward_dynamics<T>(ctx->compute, pick<T>(model), c, ftip, d_q, d_qd, d_tau, d_qdd, (long)rows));
  return MP_OK;
}

// analytical derivatives (mp_deriv.h): float64, unrolled models only - a larger model fails here, it is never sent elsewhere
static int deriv_impl(const char* fn, bool fd, mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd,
                      const double* d_x, int64_t rows, const double* g, const double* Ftip, double* d_y, double* d_dq, double* d_dqd,
                      double* d_mat) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  if (rows == 0) return MP_OK;
  REQUIRE(d_q && d_qd && d_x && d_dq && d_dqd, "%s: null device pointer", fn);
  REQUIRE(aligned16(d_q) && aligned16(d_qd) && aligned16(d_x) && aligned16(d_dq) && aligned16(d_dqd) && (!d_y || aligned16(d_y)) &&
              (!d_mat || aligned16(d_mat)),
          "%s: device pointers must be 16-byte aligned", fn);
  MpCall<double> c;
  make_call<double>(model, g, Ftip, &c);
  const bool ftip = any_nonzero(Ftip);
  PROFILE_SCOPE(ctx, fn);
  if (fd) HIP_TRY(mpk_fd_deriv(ctx->compute, model->d, c, ftip, d_q, d_qd, d_x, d_y, d_dq, d_dqd, d_mat, (long)rows));
  else HIP_TRY(mpk_id_deriv(ctx->compute, model->d, c, ftip, d_q, d_qd, d_x, d_y, d_dq, d_dqd, d_mat, (long)rows));
  return MP_OK;
}

// vector-Jacobian products (mp_adjoint.h): float64, unrolled models only.  x = qdd (ID) / tau (FD), cot = the cotangent;
// ID: o1 = gq, o2 = gqd, o3 = gqdd (may be null), y unused;  FD: y = qdd (may be null), o1 = gq, o2 = gqd, o3 = gtau (may be null)
static int vjp_impl(const char* fn, bool fd, mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_x,
                    const double* d_cot, int64_t rows, const double* g, const double* Ftip, double* d_y, double* d_o1, double* d_o2,
                    double* d_o3) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  if (rows == 0) return MP_OK;
  REQUIRE(d_q && d_qd && d_x && d_cot && d_o1 && d_o2, "%s: null device pointer", fn);
  REQUIRE(aligned16(d_q) && aligned16(d_qd) && aligned16(d_x) && aligned16(d_cot) && aligned16(d_o1) && aligned16(d_o2) &&
              (!d_y || aligned16(d_y)) && (!d_o3 || aligned16(d_o3)),
          "%s: device pointers must be 16-byte aligned", fn);
  MpCall<double> c;
  make_call<double>(model, g, Ftip, &c);
  const bool ftip = any_nonzero(Ftip);
  PROFILE_SCOPE(ctx, fn);
  if (fd) HIP_TRY(mpk_fd_vjp(ctx->compute, model->d, c, ftip, d_q, d_qd, d_x, d_cot, d_y, d_o1, d_o2, d_o3, (long)rows));
  else HIP_TRY(mpk_id_vjp(ctx->compute, model->d, c, ftip, d_q, d_qd, d_x, d_cot, d_o1, d_o2, d_o3, (long)rows));
  return MP_OK;
}

// reverse mode through FK + Jacobian (mp_kin_vjp.h): float64, unrolled models only; frame 0 = space, 1 = body
static int kin_vjp_impl(const char* fn, mp_ctx* ctx, const mp_model* model, int frame, const double* d_q, const double* d_gT,
                        const double* d_gJ, int64_t rows, double* d_T, double* d_J, double* d_gq) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  if (int rc = mp_kin_vjp_check(fn, frame, rows)) return rc;
  if (rows == 0) return MP_OK;
  REQUIRE(d_q, "%s: null device pointer", fn);
  REQUIRE(d_T || d_J || d_gq, "%s: at least one output is required", fn);
  REQUIRE(aligned16(d_q) && aligned16(d_gT) && aligned16(d_gJ) && aligned16(d_T) && aligned16(d_J) && aligned16(d_gq),
          "%s: device pointers must be 16-byte aligned", fn);
  PROFILE_SCOPE(ctx, fn);
  HIP_TRY(mpk_fk_jac_vjp(ctx->compute, model->d, frame, d_q, d_gT, d_gJ, d_T, d_J, d_gq, (long)rows));
  return MP_OK;
}

// operational-space dynamics and task-space torque (mp_opspace.h): float64, unrolled models only; frame 0 = space, 1 = body,
// 2 = hybrid; task 0 = full, 1 = linear, 2 = angular
static int opspace_impl(const char* fn, mp_ctx* ctx, const mp_model* model, int frame, int task, double damping, const double* d_q,
                        const double* d_qd, int64_t rows, const double* g, double* d_T, double* d_J, double* d_Jdqd, double* d_Lambda,
                        double* d_Jbar, double* d_mu, double* d_p) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  if (int rc = mp_opspace_check(fn, frame, task, damping, rows)) return rc;
  if (rows == 0) return MP_OK;
  REQUIRE(d_q && d_qd, "%s: null device pointer", fn);
  REQUIRE(d_T || d_J || d_Jdqd || d_Lambda || d_Jbar || d_mu || d_p, "%s: at least one output is required", fn);
  REQUIRE(aligned16(d_q) && aligned16(d_qd) && aligned16(d_T) && aligned16(d_J) && aligned16(d_Jdqd) && aligned16(d_Lambda) &&
              aligned16(d_Jbar) && aligned16(d_mu) && aligned16(d_p),
          "%s: device pointers must be 16-byte aligned", fn);
  MpCall<double> c;
  make_call<double>(model, g, nullptr, &c);
  PROFILE_SCOPE(ctx, fn);
  HIP_TRY(mpk_opspace(ctx->compute, model->d, c, frame, task, damping * damping, d_q, d_qd, d_T, d_J, d_Jdqd, d_Lambda, d_Jbar, d_mu, d_p,
                      (long)rows));
  return MP_OK;
}
static int opspace_torque_impl(const char* fn, mp_ctx* ctx, const mp_model* model, int frame, int task, double damping, const double* d_q,
                               const double* d_qd, const double* d_acc, const double* d_tau0, int64_t rows, const double* g,
                               double* d_tau) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  if (int rc = mp_opspace_check(fn, frame, task, damping, rows)) return rc;
  if (rows == 0) return MP_OK;
  REQUIRE(d_q && d_qd && d_acc && d_tau, "%s: null device pointer", fn);
  REQUIRE(aligned16(d_q) && aligned16(d_qd) && aligned16(d_acc) && aligned16(d_tau0) && aligned16(d_tau),
          "%s: device pointers must be 16-byte aligned", fn);
  MpCall<double> c;
  make_call<double>(model, g, nullptr, &c);
  PROFILE_SCOPE(ctx, fn);
  HIP_TRY(mpk_opspace_torque(ctx->compute, model->d, c, frame, task, damping * damping, d_q, d_qd, d_acc, d_tau0, d_tau, (long)rows));
  return MP_OK;
}

// dynamics regressor (mp_regressor.h): float64, unrolled models only; the kernels read the inertial-parameter map from the
// model's device copy.  Y's row holds n x 10n values, A 10n x 10n.
constexpr int MP_REG_P = 10;
static int regressor_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_qdd,
                          int64_t rows, const double* g, const double* Ftip, double* d_Y, double* d_tau_ext) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  if (int rc = mp_regressor_check(fn, rows)) return rc;
  if (rows == 0) return MP_OK;
  REQUIRE(d_q && d_qd && d_qdd && d_Y, "%s: null device pointer", fn);
  REQUIRE(aligned16(d_q) && aligned16(d_qd) && aligned16(d_qdd) && aligned16(d_Y) && aligned16(d_tau_ext),
          "%s: device pointers must be 16-byte aligned", fn);
  const MpModel<float>* dm = nullptr;
  if (int rc = device_model(ctx, model, &dm)) return rc;
  const double* dmap = (const double*)((const char*)dm + kDevModelMap);
  MpCall<double> c;
  make_call<double>(model, g, Ftip, &c);
  PROFILE_SCOPE(ctx, fn);
  HIP_TRY(mpk_id_regressor(ctx->compute, model->d, dmap, c, any_nonzero(Ftip), d_q, d_qd, d_qdd, d_Y, d_tau_ext, (long)rows));
  return MP_OK;
}
static int regressor_normal_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd,
                                 const double* d_qdd, const double* d_rhs, int64_t rows, const double* g, const double* Ftip,
                                 void* d_work, double* d_A, double* d_b, double* d_rr) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  if (int rc = mp_regressor_check(fn, rows)) return rc;
  REQUIRE(d_b && d_rr, "%s: null device pointer", fn);
  REQUIRE(aligned16(d_A) && aligned16(d_b) && aligned16(d_rr), "%s: device pointers must be 16-byte aligned", fn);
  const size_t w = (size_t)MP_REG_P * (size_t)model->d.n;
  PROFILE_SCOPE(ctx, fn);
  if (rows == 0) {
    if (d_A) HIP_TRY(hipMemsetAsync(d_A, 0, w * w * sizeof(double), ctx->compute));
    HIP_TRY(hipMemsetAsync(d_b, 0, w * sizeof(double), ctx->compute));
    HIP_TRY(hipMemsetAsync(d_rr, 0, sizeof(double), ctx->compute));
    return MP_OK;
  }
  REQUIRE(d_q && d_qd && d_qdd && d_rhs && d_work, "%s: null device pointer", fn);
  REQUIRE(aligned16(d_q) && aligned16(d_qd) && aligned16(d_qdd) && aligned16(d_rhs) && aligned16(d_work),
          "%s: device pointers must be 16-byte aligned", fn);
  const MpModel<float>* dm = nullptr;
  if (int rc = device_model(ctx, model, &dm)) return rc;
  const double* dmap = (const double*)((const char*)dm + kDevModelMap);
  MpCall<double> c;
  make_call<double>(model, g, Ftip, &c);
  HIP_TRY(mpk_id_regressor_normal(ctx->compute, model->d, dmap, c, any_nonzero(Ftip), d_q, d_qd, d_qdd, d_rhs, (long)rows,
                                  (double*)d_work, d_A, d_b, d_rr));
  return MP_OK;
}
int64_t regressor_normal_work_bytes(int n, int64_t rows) {
  return rows <= 0 ? 0 : (int64_t)mp_reg_normal_groups((long)rows) * (int64_t)mp_reg_normal_stride(n) * (int64_t)sizeof(double);
}

// reverse mode through the roll-out (mp_rollout_vjp.h): float64, unrolled models only
int64_t vjp_work_doubles(int n, int64_t B, int64_t N, int intRes) { return (B * N + B * (int64_t)intRes) * 2 * (int64_t)n; }
static int fdtraj_vjp_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const double* d_theta0, const double* d_dtheta0,
                           const double* d_taumat, const double* d_Ftipmat, int64_t B, int64_t N, const double* g, double dt, int intRes,
                           const double* d_gpos, const double* d_gvel, const double* d_gacc, void* d_work, double* d_gtheta0,
                           double* d_gdtheta0, double* d_gtaumat) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  REQUIRE(B >= 0 && N >= 0, "%s: negative B (%lld) or N (%lld)", fn, (long long)B, (long long)N);
  REQUIRE(intRes >= 1, "%s: intRes must be >= 1 (got %d)", fn, intRes);
  if (B == 0 || N == 0) return MP_OK;
  REQUIRE(d_theta0 && d_dtheta0 && d_taumat && d_work && d_gtheta0 && d_gdtheta0 && d_gtaumat, "%s: null device pointer", fn);
  REQUIRE(aligned16(d_theta0) && aligned16(d_dtheta0) && aligned16(d_taumat) && aligned16(d_Ftipmat) && aligned16(d_gpos) &&
              aligned16(d_gvel) && aligned16(d_gacc) && aligned16(d_work) && aligned16(d_gtheta0) && aligned16(d_gdtheta0) &&
              aligned16(d_gtaumat),
          "%s: device pointers must be 16-byte aligned", fn);
  MpCall<double> c;
  make_call<double>(model, g, nullptr, &c);
  PROFILE_SCOPE(ctx, fn);
  HIP_TRY(mpk_fd_traj_vjp(ctx->compute, model->d, c, d_theta0, d_dtheta0, d_taumat, d_Ftipmat, (long)B, (long)N, dt / intRes, intRes,
                          d_gpos, d_gvel, d_gacc, (double*)d_work, d_gtheta0, d_gdtheta0, d_gtaumat));
  return MP_OK;
}
// The host form's workspace cap (MANIPULAPY_HIP_VJP_WORK_BYTES, read at every call; default 1 GiB): the batch is cut into chunks of
// whole trajectories whose workspace stays under it
int64_t vjp_work_cap() {
  const char* e = getenv("MANIPULAPY_HIP_VJP_WORK_BYTES");
  const long long v = e ? atoll(e) : 0;
  return v > 0 ? (int64_t)v : (int64_t)1 << 30;
}
// batch-major host arrays: per chunk, upload -> (B, N, *) to (N, B, *) on the device -> the time-major VJP -> back -> download
static int fdtraj_vjp_host_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const double* theta0, const double* dtheta0,
                                const double* taumat, const double* Ftipmat, int64_t B, int64_t N, const double* g, double dt,
                                int intRes, const double* gpos, const double* gvel, const double* gacc, double* gtheta0,
                                double* gdtheta0, double* gtaumat) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  REQUIRE(B >= 0 && N >= 0, "%s: negative B (%lld) or N (%lld)", fn, (long long)B, (long long)N);
  REQUIRE(intRes >= 1, "%s: intRes must be >= 1 (got %d)", fn, intRes);
  if (B == 0 || N == 0) return MP_OK;
  REQUIRE(theta0 && dtheta0 && taumat && gtheta0 && gdtheta0 && gtaumat, "%s: null host pointer", fn);
  const int n = model->d.n;
  const int64_t per = vjp_work_doubles(n, 1, N, intRes) * (int64_t)sizeof(double);  // workspace bytes of one trajectory
  int64_t cb = std::max<int64_t>(1, vjp_work_cap() / per);
  if (cb >= 64) cb &= ~(int64_t)63;
  cb = std::min(cb, B);
  const size_t sr = (size_t)n * sizeof(double), tr = (size_t)N * sr, fr = (size_t)N * 6 * sizeof(double);
  // the blocks hold one chunk and serve every chunk, so the arrays are moved chunk by chunk rather than declared
  HostCall h(ctx);
  h.stage(cb * std::max(tr, fr));  // batch-major staging, reused in stream order
  double *d0 = h.work<double>(cb * sr), *d1 = h.work<double>(cb * sr), *dtau = h.work<double>(cb * tr);
  double *dF = Ftipmat ? h.work<double>(cb * fr) : nullptr, *dgp = gpos ? h.work<double>(cb * tr) : nullptr;
  double *dgv = gvel ? h.work<double>(cb * tr) : nullptr, *dga = gacc ? h.work<double>(cb * tr) : nullptr;
  void* dwork = h.work((size_t)vjp_work_doubles(n, cb, N, intRes) * sizeof(double));
  double *dg0 = h.work<double>(cb * sr), *dg1 = h.work<double>(cb * sr), *dgt = h.work<double>(cb * tr);
  for (int64_t b0 = 0; b0 < B; b0 += cb) {
    const int64_t nb = std::min(cb, B - b0);
    h.upload(d0, theta0 + b0 * n, nb * sr);
    h.upload(d1, dtheta0 + b0 * n, nb * sr);
    h.upload_tm(dtau, taumat + b0 * N * n, nb, N, sr);
    if (dF) h.upload_tm(dF, Ftipmat + b0 * N * 6, nb, N, 6 * sizeof(double));
    if (dgp) h.upload_tm(dgp, gpos + b0 * N * n, nb, N, sr);
    if (dgv) h.upload_tm(dgv, gvel + b0 * N * n, nb, N, sr);
    if (dga) h.upload_tm(dga, gacc + b0 * N * n, nb, N, sr);
    h.step([&] {
      return fdtraj_vjp_impl(fn, ctx, model, d0, d1, dtau, dF, nb, N, g, dt, intRes, dgp, dgv, dga, dwork, dg0, dg1, dgt);
    });
    h.download(gtheta0 + b0 * n, dg0, nb * sr);
    h.download(gdtheta0 + b0 * n, dg1, nb * sr);
    h.download_tm(gtaumat + b0 * N * n, dgt, N, nb, sr);
  }
  return h.finish();
}

// batched iLQR (mp_ilqr.h): float64, unrolled models only, intRes = 1.  The weights are host vectors (2n, n, 2n) and travel as kernel
// arguments.  k_batch_major: K / k are (B, N, ...) instead of (N, B, ...) - what the host forms hand back.
static int ilqr_weights(const char* fn, int n, const double* wq, const double* wr, const double* wf, MpIlqrWeights* W) {
  if (int rc = mp_ilqr_weights_check(fn, n, wq, wr, wf)) return rc;
  std::memset(W, 0, sizeof *W);
  std::copy(wq, wq + 2 * n, W->wq);
  std::copy(wr, wr + n, W->wr);
  std::copy(wf, wf + 2 * n, W->wf);
  return MP_OK;
}
// MANIPULAPY_HIP_ILQR_BACKWARD=lane (read at every call): the one-lane-per-trajectory kernel and its global workspace instead of the
// cooperative LDS kernel - kept for A/B measurements (tools/ilqr_bench.py)
static bool ilqr_lane_variant() {
  const char* e = getenv("MANIPULAPY_HIP_ILQR_BACKWARD");
  return e && std::strcmp(e, "lane") == 0;
}
static int ilqr_backward_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const double* d_pos, const double* d_vel,
                              const double* d_taumat, const double* d_dq, const double* d_dqd, const double* d_Minv, const double* d_xref,
                              const double* wq, const double* wr, const double* wf, const double* d_reg, int64_t B, int64_t N, double dt,
                              bool k_batch_major, void* d_work, double* d_K, double* d_k, double* d_dV, int32_t* d_status) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  REQUIRE(B >= 0, "%s: negative B (%lld)", fn, (long long)B);
  REQUIRE(N >= 2, "%s: N must be >= 2 (got %lld)", fn, (long long)N);
  MpIlqrWeights W;
  if (int rc = ilqr_weights(fn, model->d.n, wq, wr, wf, &W)) return rc;
  if (B == 0) return MP_OK;
  const bool lane = ilqr_lane_variant();
  REQUIRE(d_pos && d_vel && d_taumat && d_dq && d_dqd && d_Minv && d_xref && d_reg && (d_work || !lane) && d_K && d_k && d_dV && d_status,
          "%s: null device pointer", fn);
  REQUIRE(aligned16(d_pos) && aligned16(d_vel) && aligned16(d_taumat) && aligned16(d_dq) && aligned16(d_dqd) && aligned16(d_Minv) &&
              aligned16(d_xref) && aligned16(d_reg) && aligned16(d_work) && aligned16(d_K) && aligned16(d_k) && aligned16(d_dV) &&
              aligned16(d_status),
          "%s: device pointers must be 16-byte aligned", fn);
  PROFILE_SCOPE(ctx, fn);
  HIP_TRY(mpk_ilqr_backward(ctx->compute, model->d, W, d_pos, d_vel, d_taumat, d_dq, d_dqd, d_Minv, d_xref, d_reg, (long)B, (long)N, dt,
                            k_batch_major, lane ? (double*)d_work : nullptr, d_K, d_k, d_dV, (int*)d_status));
  return MP_OK;
}
static int ilqr_rollout_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const double* d_theta0, const double* d_dtheta0,
                             const double* d_taumat, const double* d_pos, const double* d_vel, const double* d_K, const double* d_k,
                             const double* d_alpha, const double* d_xref, const double* wq, const double* wr, const double* wf, int64_t A,
                             int64_t B, int64_t N, const double* g, double dt, bool k_batch_major, double* d_cost, double* d_opos,
                             double* d_ovel, double* d_otau) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  REQUIRE(A >= 0 && B >= 0, "%s: negative A (%lld) or B (%lld)", fn, (long long)A, (long long)B);
  REQUIRE(N >= 2, "%s: N must be >= 2 (got %lld)", fn, (long long)N);
  MpIlqrWeights W;
  if (int rc = ilqr_weights(fn, model->d.n, wq, wr, wf, &W)) return rc;
  if (A == 0 || B == 0) return MP_OK;
  REQUIRE(d_theta0 && d_dtheta0 && d_taumat && d_alpha && d_xref && d_cost, "%s: null device pointer", fn);
  REQUIRE((d_K != nullptr) == (d_k != nullptr), "%s: K and k must both be given or both be null", fn);
  REQUIRE(!d_K || (d_pos && d_vel), "%s: the gains need the nominal pos and vel", fn);
  REQUIRE((d_opos != nullptr) == (d_ovel != nullptr) && (d_opos != nullptr) == (d_otau != nullptr),
          "%s: the three row outputs must all be given or all be null", fn);
  REQUIRE(aligned16(d_theta0) && aligned16(d_dtheta0) && aligned16(d_taumat) && aligned16(d_pos) && aligned16(d_vel) && aligned16(d_K) &&
              aligned16(d_k) && aligned16(d_alpha) && aligned16(d_xref) && aligned16(d_cost) && aligned16(d_opos) && aligned16(d_ovel) &&
              aligned16(d_otau),
          "%s: device pointers must be 16-byte aligned", fn);
  MpCall<double> c;
  make_call<double>(model, g, nullptr, &c);
  PROFILE_SCOPE(ctx, fn);
  HIP_TRY(mpk_ilqr_rollout(ctx->compute, model->d, c, W, d_theta0, d_dtheta0, d_taumat, d_pos, d_vel, d_K, d_k, d_alpha, d_xref, (long)A,
                           (long)B, (long)N, dt, k_batch_major, d_cost, d_opos, d_ovel, d_otau));
  return MP_OK;
}
// batch-major host arrays: upload -> (B, N, *) to (N, B, *) on the device -> the derivative launch and the backward pass -> download;
// the kernel writes K / k batch-major itself (a row of K is wider than mp_transpose_rows moves)
static int ilqr_backward_host_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const double* pos, const double* vel,
                                   const double* taumat, const double* xref, const double* wq, const double* wr, const double* wf,
                                   const double* reg, int64_t B, int64_t N, const double* g, double dt, double* K, double* k, double* dV,
                                   int32_t* status) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  REQUIRE(B >= 0, "%s: negative B (%lld)", fn, (long long)B);
  REQUIRE(N >= 2, "%s: N must be >= 2 (got %lld)", fn, (long long)N);
  if (B == 0) return MP_OK;
  REQUIRE(pos && vel && taumat && xref && reg && K && k && dV && status, "%s: null host pointer", fn);
  const int n = model->d.n;
  const size_t sr = (size_t)n * sizeof(double), tr = (size_t)N * sr, blk = (size_t)(N - 1) * B * n * sr;
  HostCall h(ctx);
  h.stage(2 * B * tr);
  const double *dp = h.in_tm(pos, B, N, sr), *dv = h.in_tm(vel, B, N, sr), *dt_ = h.in_tm(taumat, B, N, sr);
  const double *dx = h.in_tm(xref, B, N, 2 * sr), *dr = h.in(reg, B * sizeof(double));
  double *dq = h.work<double>(blk), *dqd = h.work<double>(blk), *dmi = h.work<double>(blk);
  void* dwork = h.work(ilqr_lane_variant() ? (size_t)B * mp_ilqr_work_doubles(n) * sizeof(double) : 0);
  double *dK = h.out(K, 2 * B * tr * n), *dk = h.out(k, B * tr), *ddV = h.out(dV, B * 2 * sizeof(double));
  int32_t* dst = h.out(status, B * sizeof(int32_t));
  // torque rows 1..N-1; with B n odd they start 8 bytes off the alignment asked for and are copied to a block of their own
  double* realigned = ((B * n) & 1) ? h.work<double>((size_t)(N - 1) * B * sr) : nullptr;
  return h.run([&]() -> int {
    const double* dtau1 = dt_ + B * n;
    if (realigned) {
      if (int rc = mp_transpose_rows(ctx, dtau1, 1, (N - 1) * B, (int64_t)sr, realigned)) return rc;  // outer = 1: a device copy
      dtau1 = realigned;
    }
    if (int rc = deriv_impl(fn, true, ctx, model, dp, dv, dtau1, (N - 1) * B, g, nullptr, nullptr, dq, dqd, dmi)) return rc;
    return ilqr_backward_impl(fn, ctx, model, dp, dv, dt_, dq, dqd, dmi, dx, wq, wr, wf, dr, B, N, dt, true, dwork, dK, dk, ddV, dst);
  });
}
static int ilqr_rollout_host_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const double* theta0, const double* dtheta0,
                                  const double* taumat, const double* pos, const double* vel, const double* K, const double* k,
                                  const double* alpha, const double* xref, const double* wq, const double* wr, const double* wf, int64_t A,
                                  int64_t B, int64_t N, const double* g, double dt, double* cost, double* opos, double* ovel,
                                  double* otau) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  REQUIRE(A >= 0 && B >= 0, "%s: negative A (%lld) or B (%lld)", fn, (long long)A, (long long)B);
  REQUIRE(N >= 2, "%s: N must be >= 2 (got %lld)", fn, (long long)N);
  if (A == 0 || B == 0) return MP_OK;
  REQUIRE(theta0 && dtheta0 && taumat && alpha && xref && cost, "%s: null host pointer", fn);
  REQUIRE((K != nullptr) == (k != nullptr), "%s: K and k must both be given or both be null", fn);
  REQUIRE(!K || (pos && vel), "%s: the gains need the nominal pos and vel", fn);
  REQUIRE((opos != nullptr) == (ovel != nullptr) && (opos != nullptr) == (otau != nullptr),
          "%s: the three row outputs must all be given or all be null", fn);
  const int n = model->d.n;
  const size_t sr = (size_t)n * sizeof(double), tr = (size_t)N * sr, L = (size_t)A * B;
  HostCall h(ctx);
  h.stage(std::max(2 * B * tr, opos ? L * tr : (size_t)0));
  const double *d0 = h.in(theta0, B * sr), *d1 = h.in(dtheta0, B * sr), *dt_ = h.in_tm(taumat, B, N, sr);
  const double *dp = h.in_tm(K ? pos : nullptr, B, N, sr), *dv = h.in_tm(K ? vel : nullptr, B, N, sr);  // the nominal: with gains only
  const double *dK = h.in(K, 2 * B * tr * n), *dk = h.in(k, B * tr);
  const double *dx = h.in_tm(xref, B, N, 2 * sr), *da = h.in(alpha, L * sizeof(double));
  double* dc = h.out(cost, L * sizeof(double));
  double *dop = h.out_tm(opos, N, (int64_t)L, sr), *dov = h.out_tm(ovel, N, (int64_t)L, sr), *dot = h.out_tm(otau, N, (int64_t)L, sr);
  return h.run([&] {
    return ilqr_rollout_impl(fn, ctx, model, d0, d1, dt_, dp, dv, dK, dk, da, dx, wq, wr, wf, A, B, N, g, dt, true, dc, dop, dov, dot);
  });
}

// time-optimal path parameterisation (mp_toppra.h): float64, unrolled models only.  The limits are host vectors and travel as kernel
// arguments: velocity (n, finite and positive), torque (n, 2) or null (none), acceleration (n) or null (none).
// The row outputs are written by the sweep's forward pass: measured 0.85 (xArm6) and 0.90 (Panda) of the time of the sweep followed
// by the row-parallel launch k_path_rows.  MANIPULAPY_HIP_TOPPRA_EPILOGUE=separate (read at every call, so a captured
// graph keeps the variant it was captured with) selects that launch instead; it exists for tools/toppra_bench.py to time the loser.
static bool toppra_separate_epilogue() {
  const char* e = getenv("MANIPULAPY_HIP_TOPPRA_EPILOGUE");
  return e && std::strcmp(e, "separate") == 0;
}
static int path_dynamics_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_dq,
                              const double* d_ddq, int64_t rows, const double* vlim, const double* g, const double* Ftip, double* d_a,
                              double* d_b, double* d_c, double* d_xbar) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  MpToppraVmax V;
  if (int rc = mp_toppra_vmax_check(fn, model->d.n, vlim, &V)) return rc;
  if (rows == 0) return MP_OK;
  REQUIRE(d_q && d_dq && d_ddq && d_a && d_b && d_c && d_xbar, "%s: null device pointer", fn);
  REQUIRE(aligned16(d_q) && aligned16(d_dq) && aligned16(d_ddq) && aligned16(d_a) && aligned16(d_b) && aligned16(d_c) && aligned16(d_xbar),
          "%s: device pointers must be 16-byte aligned", fn);
  MpCall<double> c;
  make_call<double>(model, g, Ftip, &c);
  PROFILE_SCOPE(ctx, fn);
  HIP_TRY(mpk_path_coeffs(ctx->compute, model->d, c, any_nonzero(Ftip), V, d_q, d_dq, d_ddq, d_a, d_b, d_c, d_xbar, (long)rows));
  return MP_OK;
}
static int toppra_tm_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const double* d_a, const double* d_b, const double* d_c,
                          const double* d_xbar, const double* d_dq, const double* d_ddq, const double* tlim, const double* alim,
                          const double* d_sd_start, const double* d_sd_end, int64_t B, int64_t N, double* d_K, double* d_x, double* d_u,
                          double* d_t, double* d_dur, int32_t* d_status, double* d_qd, double* d_qdd, double* d_tau) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  REQUIRE(B >= 0, "%s: negative B (%lld)", fn, (long long)B);
  REQUIRE(N >= 3, "%s: N must be >= 3 (got %lld)", fn, (long long)N);
  MpToppraLimits L;
  if (int rc = mp_toppra_limits_check(fn, model->d.n, tlim, alim, &L)) return rc;
  if (B == 0) return MP_OK;
  REQUIRE(d_a && d_b && d_c && d_xbar && d_sd_start && d_sd_end && d_K && d_x && d_u && d_t && d_dur && d_status,
          "%s: null device pointer", fn);
  REQUIRE((d_qd != nullptr) == (d_qdd != nullptr) && (d_qd != nullptr) == (d_tau != nullptr),
          "%s: the three row outputs must all be given or all be null", fn);
  REQUIRE(!(alim || d_tau) || (d_dq && d_ddq), "%s: acceleration limits and the row outputs need the path derivatives dq and ddq", fn);
  REQUIRE(aligned16(d_a) && aligned16(d_b) && aligned16(d_c) && aligned16(d_xbar) && aligned16(d_dq) && aligned16(d_ddq) &&
              aligned16(d_sd_start) && aligned16(d_sd_end) && aligned16(d_K) && aligned16(d_x) && aligned16(d_u) && aligned16(d_t) &&
              aligned16(d_dur) && aligned16(d_status) && aligned16(d_qd) && aligned16(d_qdd) && aligned16(d_tau),
          "%s: device pointers must be 16-byte aligned", fn);
  const bool fused = d_tau && !toppra_separate_epilogue();
  PROFILE_SCOPE(ctx, fn);
  HIP_TRY(mpk_toppra_sweep(ctx->compute, model->d.n, L, alim != nullptr, d_a, d_b, d_c, d_xbar, d_dq, d_ddq, d_sd_start, d_sd_end, (long)B,
                           (long)N, d_K, d_x, d_u, d_t, d_dur, (int*)d_status, fused ? d_qd : nullptr, fused ? d_qdd : nullptr,
                           fused ? d_tau : nullptr));
  if (d_tau && !fused)
    HIP_TRY(mpk_path_rows(ctx->compute, model->d.n, d_a, d_b, d_c, d_dq, d_ddq, d_x, d_u, d_qd, d_qdd, d_tau, (long)(B * N)));
  return MP_OK;
}
// batch-major host arrays: upload -> (B, N, n) to (N, B, n) on the device -> coefficients, sweep, rows -> back to batch-major -> download
static int toppra_host_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const double* q, const double* dq, const double* ddq,
                            const double* vlim, const double* tlim, const double* alim, const double* sd_start, const double* sd_end,
                            int64_t B, int64_t N, const double* g, const double* Ftip, double* K, double* x, double* u, double* t,
                            double* dur, int32_t* status, double* qd, double* qdd, double* tau) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  REQUIRE(B >= 0, "%s: negative B (%lld)", fn, (long long)B);
  REQUIRE(N >= 3, "%s: N must be >= 3 (got %lld)", fn, (long long)N);
  MpToppraVmax V;
  MpToppraLimits L;
  if (int rc = mp_toppra_vmax_check(fn, model->d.n, vlim, &V)) return rc;
  if (int rc = mp_toppra_limits_check(fn, model->d.n, tlim, alim, &L)) return rc;
  if (B == 0) return MP_OK;
  REQUIRE(q && dq && ddq && sd_start && sd_end && K && x && u && t && dur && status, "%s: null host pointer", fn);
  REQUIRE((qd != nullptr) == (qdd != nullptr) && (qd != nullptr) == (tau != nullptr),
          "%s: the three row outputs must all be given or all be null", fn);
  const int n = model->d.n;
  const size_t sr = (size_t)n * sizeof(double), rows = (size_t)B * N, col = rows * sizeof(double);
  HostCall h(ctx);
  h.stage(std::max(rows * sr, 2 * col));
  const double *dq0 = h.in_tm(q, B, N, sr), *dq1 = h.in_tm(dq, B, N, sr), *dq2 = h.in_tm(ddq, B, N, sr);
  const double *ds0 = h.in(sd_start, B * sizeof(double)), *ds1 = h.in(sd_end, B * sizeof(double));
  double *da = h.work<double>(rows * sr), *db = h.work<double>(rows * sr), *dc = h.work<double>(rows * sr), *dxb = h.work<double>(col);
  double *dK = h.out_tm(K, N, B, 2 * sizeof(double)), *dx = h.out_tm(x, N, B, sizeof(double)), *du = h.out_tm(u, N, B, sizeof(double));
  double* dt_ = h.out_tm(t, N, B, sizeof(double));
  double *dqd = h.out_tm(qd, N, B, sr), *dqdd = h.out_tm(qdd, N, B, sr), *dtau = h.out_tm(tau, N, B, sr);
  double* ddur = h.out(dur, B * sizeof(double));
  int32_t* dst = h.out(status, B * sizeof(int32_t));
  return h.run([&]() -> int {
    if (int rc = path_dynamics_impl(fn, ctx, model, dq0, dq1, dq2, (int64_t)rows, vlim, g, Ftip, da, db, dc, dxb)) return rc;
    return toppra_tm_impl(fn, ctx, model, da, db, dc, dxb, dq1, dq2, tlim, alim, ds0, ds1, B, N, dK, dx, du, dt_, ddur, dst, dqd, dqdd, dtau);
  });
}

// specialised forward-dynamics roll-out (float32 only): -1 = none available, otherwise the launch's return code
int launch_fd_spec(mp_ctx* ctx, const mp_model* model, const MpCall<float>& c, const float* th0, const float* dth0,
                    const float* taumat, const float* Fm, long B, long Nt, float h, int intRes, float* pos, float* vel, float* acc,
                    bool time_major) {
  const MpSpec* sp = find_spec(ctx, model);
  if (!sp) return -1;
  MpCall<float> cc = c;
  void* args[] = {&cc, &th0, &dth0, &taumat, &Fm, &B, &Nt, &h, &intRes, &pos, &vel, &acc};
  if (time_major) return launch_spec(ctx, sp->fd_traj_tm[Fm ? 1 : 0], B, args, 64);
  return launch_spec(ctx, sp->fd_traj[Fm ? 1 : 0], B, args, 64);  // one wave per block (per-wave LDS tile)
}
int launch_fd_spec(mp_ctx*, const mp_model*, const MpCall<double>&, const double*, const double*, const double*, const double*,
                   long, long, double, int, float*, float*, float*, bool) {
  return -1;
}

template <typename T>
static int fdtraj_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const T* d_theta0, const T* d_dtheta0,
                       const T* d_taumat, const T* d_Ftipmat, int64_t B, int64_t N, const double* g, double dt, int intRes,
                       float* d_pos, float* d_vel, float* d_acc, bool time_major = false) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE(B >= 0 && N >= 0, "%s: negative B or N", fn);
  REQUIRE(intRes >= 0, "%s: negative intRes", fn);
  if (B == 0 || N == 0) return MP_OK;
  REQUIRE(d_theta0 && d_dtheta0 && d_taumat && d_pos && d_vel && d_acc, "%s: null device pointer", fn);
  REQUIRE(aligned16(d_theta0) && aligned16(d_dtheta0) && aligned16(d_taumat) && aligned16(d_Ftipmat) && aligned16(d_pos) &&
              aligned16(d_vel) && aligned16(d_acc), "%s: device pointers must be 16-byte aligned", fn);
  MpCall<T> c;
  make_call<T>(model, g, nullptr, &c);
  const T h = intRes > 0 ? (T)(dt / intRes) : (T)0;
  PROFILE_SCOPE(ctx, fn);
  if (model->big) {
    const MpBigModel<T>* dm = nullptr;
    if (int rc = device_big_model<T>(ctx, model, &dm)) return rc;
    HIP_TRY(mpk_dyn_fd_traj<T>(ctx->compute, model->d.n, dm, c, d_theta0, d_dtheta0, d_taumat, d_Ftipmat, (long)B, (long)N, h, intRes, d_pos, d_vel,
                               d_acc, time_major));
    return MP_OK;
  }
  const int src = launch_fd_spec(ctx, model, c, d_theta0, d_dtheta0, d_taumat, d_Ftipmat, (long)B, (long)N, h, intRes, d_pos, d_vel, d_acc,
                                 time_major);
  if (src >= 0) return src;  // a specialised kernel exists for this model: launched (0) or failed (error code)
  if (time_major) {
    HIP_TRY(mpk_fd_traj_tm<T>(ctx->compute, pick<T>(model), c, d_theta0, d_dtheta0, d_taumat, d_Ftipmat, (long)B, (long)N, h, intRes,
                              d_pos, d_vel, d_acc));
    return MP_OK;
  }
  HIP_TRY(mpk_fd_traj<T>(ctx->compute, pick<T>(model), c, d_theta0, d_dtheta0, d_taumat, d_Ftipmat, (long)B, (long)N, h, intRes,
                         d_pos, d_vel, d_acc));
  return MP_OK;
}

template <typename T>
static int fdtraj_host_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const T* theta0, const T* dtheta0,
                            const T* taumat, const T* Ftipmat, int64_t B, int64_t N, const double* g, double dt, int intRes,
                            float* pos, float* vel, float* acc) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE(B >= 0 && N >= 0, "%s: negative B or N", fn);
  if (B == 0 || N == 0) return MP_OK;
  REQUIRE(theta0 && dtheta0 && taumat && pos && vel && acc, "%s: null host pointer", fn);
  // Rows are whole trajectories: one moves (n + 6) sizeof(T) bytes up and 12 n down per step.
  const int64_t n = model->d.n, tn = N * n;
  HostCall h(ctx, B);
  const T *d0 = h.in_rows(theta0, n * sizeof(T)), *d1 = h.in_rows(dtheta0, n * sizeof(T)), *dt_ = h.in_rows(taumat, tn * sizeof(T));
  const T* df = h.in_rows(Ftipmat, N * 6 * sizeof(T));
  float *dp = h.out_rows(pos, tn * sizeof(float)), *dv = h.out_rows(vel, tn * sizeof(float)), *da = h.out_rows(acc, tn * sizeof(float));
  const int64_t cb = std::max<int64_t>(64, (host_chunk_rows() / std::max<int64_t>(N, 1)) & ~(int64_t)63);  // trajectories per chunk
  return h.run_rows(cb, 2 * cb, [&](int64_t b0, int64_t nb) {
    return fdtraj_impl<T>(fn, ctx, model, d0 + b0 * n, d1 + b0 * n, dt_ + b0 * tn, at(df, b0 * N * 6), nb, N, g, dt, intRes, dp + b0 * tn,
                          dv + b0 * tn, da + b0 * tn);
  });
}
}  // namespace

extern "C" {

// ------------------------------------------------------------------------------ library / device
int mp_version(void) { return 1; }
const char* mp_last_error(void) { return g_err; }

int mp_device_count(int* count) {
  REQUIRE(count, "mp_device_count: null output");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e == hipErrorNoDevice) { *count = 0; (void)hipGetLastError(); return MP_OK; }
  if (e != hipSuccess) { *count = 0; return hip_err(e, "hipGetDeviceCount"); }
  *count = n;
  return MP_OK;
}

int mp_ctx_create(int device_id, mp_ctx** out) {
  REQUIRE(out, "mp_ctx_create: null output");
  *out = nullptr;
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  REQUIRE(device_id >= 0 && device_id < n, "mp_ctx_create: device %d not in [0, %d)", device_id, n);
  HIP_TRY(hipSetDevice(device_id));
  mp_ctx* c = new (std::nothrow) mp_ctx;
  REQUIRE(c, "mp_ctx_create: out of host memory");
  c->device = device_id;
  {
    static std::atomic<uint64_t> next_uid{1};
    c->uid = next_uid.fetch_add(1);
  }
  {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device_id) == hipSuccess) c->compute_units = p.multiProcessorCount;
  }
  hipError_t e = hipStreamCreateWithFlags(&c->compute, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->copy_out, hipStreamNonBlocking);
  if (e != hipSuccess) { delete c; return hip_err(e, "hipStreamCreate"); }
  {
    std::lock_guard<std::mutex> lk(g_ctxs_mu);
    g_ctxs.insert(c);
  }
  *out = c;
  return MP_OK;
}

int mp_ctx_destroy(mp_ctx* ctx) {
  if (!ctx) return MP_OK;
  {
    std::lock_guard<std::mutex> lk(g_ctxs_mu);
    g_ctxs.erase(ctx);
  }
  (void)hipSetDevice(ctx->device);
  if (!ctx->capturing) (void)hard_flush(ctx);  // parked float64 passes: their launches' results are complete before the memory goes
  (void)hipDeviceSynchronize();
  for (auto& pe : ctx->prof_pending) { (void)hipEventDestroy(pe.a); (void)hipEventDestroy(pe.b); }
  for (auto& kv : ctx->specs) {
    if (kv.second.mod_ilp) (void)hipModuleUnload(kv.second.mod_ilp);
    if (kv.second.mod) (void)hipModuleUnload(kv.second.mod);
  }
  for (hipModule_t m : ctx->retired_mods) (void)hipModuleUnload(m);
  for (auto& kv : ctx->live) (void)hipFree(kv.first);
  if (ctx->queue_counter) (void)hipFree(ctx->queue_counter);
  free_hard_pool(&ctx->own_pool);
  if (ctx->hp != &ctx->own_pool) { free_hard_pool(ctx->hp); delete ctx->hp; }  // a capture left open
  if (ctx->time_tab) (void)hipFree(ctx->time_tab);
  for (void* p : ctx->retired_tabs) (void)hipFree(p);
  if (ctx->compute) (void)hipStreamDestroy(ctx->compute);
  if (ctx->copy) (void)hipStreamDestroy(ctx->copy);
  if (ctx->copy_out) (void)hipStreamDestroy(ctx->copy_out);
  if (ctx->aux) (void)hipStreamDestroy(ctx->aux);
  if (ctx->clock_buf) (void)hipFree(ctx->clock_buf);
  delete ctx;
  return MP_OK;
}

int mp_ctx_set_profiling(mp_ctx* ctx, int on) {
  REQUIRE(ctx, "mp_ctx_set_profiling: null context");
  CTX_ENTER(ctx);
  ctx->profiling = on != 0;
  return MP_OK;
}

int mp_ctx_profile(mp_ctx* ctx, double* kernel_ms_total, int64_t* timed_calls, double* kernel_ms_last, int reset) {
  REQUIRE(ctx, "mp_ctx_profile: null context");
  CTX_ENTER(ctx);
  for (auto& pe : ctx->prof_pending) {  // resolve the event pairs recorded since the last read
    float ms = 0.f;
    if (hipEventSynchronize(pe.b) == hipSuccess && hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess) {
      ctx->prof_total_ms += ms;
      ctx->prof_last_ms = ms;
      ctx->prof_launches += 1;
    }
    (void)hipEventDestroy(pe.a);
    (void)hipEventDestroy(pe.b);
  }
  ctx->prof_pending.clear();
  if (kernel_ms_total) *kernel_ms_total = ctx->prof_total_ms;
  if (timed_calls) *timed_calls = ctx->prof_launches;
  if (kernel_ms_last) *kernel_ms_last = ctx->prof_last_ms;
  if (reset) { ctx->prof_total_ms = 0; ctx->prof_last_ms = 0; ctx->prof_launches = 0; }
  return MP_OK;
}

int mp_ctx_get_stream(mp_ctx* ctx, void** hip_stream) {
  REQUIRE(ctx && hip_stream, "mp_ctx_get_stream: null argument");
  CTX_ENTER(ctx);  // (parked float64 passes run first: what the caller enqueues behind this call sees complete results)
  ctx->stream_exported = true;  // sticky: every later float32 launch enqueues its float64 pass at once, whoever owns its arrays
  *hip_stream = (void*)ctx->compute;
  return MP_OK;
}

// Stream order between the compute stream and a caller's stream through a fresh HIP event (recorded on `from`, waited on by `to`,
// released at once: the wait keeps what it needs).  Neither hands the compute stream out, so parking stays as it was.
static int join_streams(const char* fn, mp_ctx* ctx, hipStream_t from, hipStream_t to) {
  hipEvent_t ev = nullptr;
  HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, from);
  if (e == hipSuccess) e = hipStreamWaitEvent(to, ev, 0);
  (void)hipEventDestroy(ev);
  if (e != hipSuccess) return hip_err(e, fn);
  (void)ctx;
  return MP_OK;
}
int mp_ctx_wait_for_stream(mp_ctx* ctx, void* hip_stream) {
  REQUIRE(ctx, "mp_ctx_wait_for_stream: null context");
  CTX_ENTER(ctx);
  return join_streams("mp_ctx_wait_for_stream", ctx, (hipStream_t)hip_stream, ctx->compute);
}
int mp_ctx_stream_wait_for_ctx(mp_ctx* ctx, void* hip_stream) {
  REQUIRE(ctx, "mp_ctx_stream_wait_for_ctx: null context");
  CTX_ENTER(ctx);  // (parked float64 passes run first: hip_stream then waits for their torques too)
  return join_streams("mp_ctx_stream_wait_for_ctx", ctx, ctx->compute, (hipStream_t)hip_stream);
}

int mp_ctx_synchronize(mp_ctx* ctx) {
  REQUIRE(ctx, "mp_ctx_synchronize: null context");
  CTX_ENTER(ctx);
  HIP_TRY(hipStreamSynchronize(ctx->compute));
  HIP_TRY(hipStreamSynchronize(ctx->copy));
  HIP_TRY(hipStreamSynchronize(ctx->copy_out));
  return MP_OK;
}

int mp_ctx_properties(mp_ctx* ctx, char* name, size_t name_len, int* compute_units, uint64_t* hbm_bytes) {
  REQUIRE(ctx, "mp_ctx_properties: null context");
  hipDeviceProp_t p;
  HIP_TRY(hipGetDeviceProperties(&p, ctx->device));
  if (name && name_len) std::snprintf(name, name_len, "%s (%s)", p.name, p.gcnArchName);
  if (compute_units) *compute_units = p.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (uint64_t)p.totalGlobalMem;
  return MP_OK;
}

int mp_selftest(mp_ctx* ctx) {
  REQUIRE(ctx, "mp_selftest: null context");
  CTX_ENTER(ctx);
  Scratch sc(ctx);
  void* d = nullptr;
  if (int rc = sc.get(64 * sizeof(int), &d)) return rc;
  HIP_TRY(hipMemsetAsync(d, 0xFF, 64 * sizeof(int), ctx->compute));
  HIP_TRY(mpk_selftest(ctx->compute, static_cast<int*>(d)));
  int h[64];
  HIP_TRY(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, ctx->compute));
  HIP_TRY(hipStreamSynchronize(ctx->compute));
  for (int i = 0; i < 64; ++i)
    if (h[i] != i) return mp_fail(MP_ERR_HIP, "mp_selftest: lane %d wrote %d", i, h[i]);
  return MP_OK;
}

int mp_stream_bandwidth(mp_ctx* ctx, size_t bytes_per_array, int reads, int reps, double* gb_per_s) {
  REQUIRE(ctx && gb_per_s, "mp_stream_bandwidth: null argument");
  const bool nt = reads > 10;  // 11 / 13: the same two kernels with non-temporal loads and stores
  if (nt) reads -= 10;
  REQUIRE(reads == 1 || reads == 3, "mp_stream_bandwidth: reads must be 1 or 3 (plain accesses), 11 or 13 (non-temporal)");
  REQUIRE(bytes_per_array >= 16 && reps >= 1, "mp_stream_bandwidth: nothing to move");
  CTX_ENTER(ctx);
  const size_t nb = bytes_per_array & ~(size_t)15;
  Scratch sc(ctx);
  void* buf[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < (reads == 3 ? 4 : 2); ++k) {
    if (int rc = sc.get(nb, &buf[k])) return rc;
    HIP_TRY(hipMemsetAsync(buf[k], 0, nb, ctx->compute));
  }
  void *a = buf[0], *d = buf[reads == 3 ? 3 : 1];
  const long n4 = (long)(nb / 16);
  for (int w = 0; w < 3; ++w) HIP_TRY(mpk_stream(ctx->compute, reads, nt, a, buf[1], buf[2], d, n4));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return mp_fail(MP_ERR_HIP, "mp_stream_bandwidth: hipEventCreate failed"); }
  hipError_t e = hipEventRecord(e0, ctx->compute);
  for (int r = 0; r < reps && e == hipSuccess; ++r) e = mpk_stream(ctx->compute, reads, nt, a, buf[1], buf[2], d, n4);
  if (e == hipSuccess) e = hipEventRecord(e1, ctx->compute);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (e != hipSuccess) return mp_fail(MP_ERR_HIP, "mp_stream_bandwidth: %s", hipGetErrorString(e));
  *gb_per_s = (double)(reads + 1) * (double)nb * (double)reps / ((double)ms * 1e-3) / 1e9;
  return MP_OK;
}

int mp_stream_bandwidth_mix(mp_ctx* ctx, size_t bytes_per_array, int reads, int writes, int nontemporal, int reps, double* gb_per_s) {
  REQUIRE(ctx && gb_per_s, "mp_stream_bandwidth_mix: null argument");
  REQUIRE(bytes_per_array >= 16 && reps >= 1 && reads >= 0 && writes >= 1, "mp_stream_bandwidth_mix: nothing to move");
  CTX_ENTER(ctx);
  const size_t nb = bytes_per_array & ~(size_t)15;
  Scratch sc(ctx);
  void *a = nullptr, *d = nullptr;
  if (int rc = sc.get(nb * (size_t)std::max(reads, 1), &a)) return rc;
  if (int rc = sc.get(nb * (size_t)writes, &d)) return rc;
  HIP_TRY(hipMemsetAsync(a, 0, nb * (size_t)std::max(reads, 1), ctx->compute));
  HIP_TRY(hipMemsetAsync(d, 0, nb * (size_t)writes, ctx->compute));
  const long n4 = (long)(nb / 16);
  hipError_t e = hipSuccess;
  for (int w = 0; w < 2 && e == hipSuccess; ++w) e = mpk_stream_mix(ctx->compute, reads, writes, nontemporal != 0, a, d, n4);
  if (e == hipErrorInvalidValue) return mp_fail(MP_ERR_INVALID, "mp_stream_bandwidth_mix: no probe kernel for %d reads : %d writes", reads, writes);
  if (e != hipSuccess) return hip_err(e, "mp_stream_bandwidth_mix");
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return mp_fail(MP_ERR_HIP, "mp_stream_bandwidth_mix: hipEventCreate failed"); }
  e = hipEventRecord(e0, ctx->compute);
  for (int r = 0; r < reps && e == hipSuccess; ++r) e = mpk_stream_mix(ctx->compute, reads, writes, nontemporal != 0, a, d, n4);
  if (e == hipSuccess) e = hipEventRecord(e1, ctx->compute);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (e != hipSuccess) return mp_fail(MP_ERR_HIP, "mp_stream_bandwidth_mix: %s", hipGetErrorString(e));
  *gb_per_s = (double)(reads + writes) * (double)nb * (double)reps / ((double)ms * 1e-3) / 1e9;
  return MP_OK;
}

// The shader clock the chip holds WHILE the caller's launches run (bench.py: `clock_hz` beside a kernel's time, so that two boxes'
// figures can be compared at equal clock).  begin: a bounded sampler (k_clock_sampler: 8 one-wave blocks, 32 stamp pairs spread over
// about duration_ms) starts on a stream of its own; the caller then launches what it wants measured on the compute stream; end: waits
// for the sampler and returns the median over the blocks of delta s_memtime / delta s_memrealtime x 100 MHz.
constexpr unsigned kClockBlocks = 8, kClockSamples = 32;
int mp_clock_sample_begin(mp_ctx* ctx, double duration_ms) {
  REQUIRE(ctx, "mp_clock_sample_begin: null context");
  REQUIRE(duration_ms > 0 && duration_ms <= 2000.0, "mp_clock_sample_begin: duration %.3f ms outside (0, 2000]", duration_ms);
  CTX_ENTER(ctx);
  REQUIRE(!ctx->capturing, "mp_clock_sample_begin: not while a launch graph is being captured");
  REQUIRE(!ctx->clock_sampling, "mp_clock_sample_begin: a sampler is already running (call mp_clock_sample_end)");
  if (!ctx->aux) HIP_TRY(hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking));
  if (!ctx->clock_buf) HIP_TRY(hipMalloc((void**)&ctx->clock_buf, (size_t)kClockBlocks * kClockSamples * 2 * sizeof(unsigned long long)));
  // one nap = 64 x 127 shader cycles, ~3.9 us at 2.1 GHz
  const unsigned naps = (unsigned)std::max(1.0, duration_ms * 1e3 / ((double)(kClockSamples - 1) * 3.9));
  HIP_TRY(mpk_clock_sampler(ctx->aux, ctx->clock_buf, kClockBlocks, kClockSamples, naps));
  ctx->clock_sampling = true;
  return MP_OK;
}
int mp_clock_sample_end(mp_ctx* ctx, double* clock_hz, double* sampled_ms) {
  REQUIRE(ctx && clock_hz, "mp_clock_sample_end: null argument");
  CTX_ENTER(ctx);
  REQUIRE(ctx->clock_sampling, "mp_clock_sample_end: no sampler running");
  ctx->clock_sampling = false;
  std::vector<unsigned long long> h((size_t)kClockBlocks * kClockSamples * 2);
  HIP_TRY(hipMemcpyAsync(h.data(), ctx->clock_buf, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->aux));
  HIP_TRY(hipStreamSynchronize(ctx->aux));
  std::vector<double> hz;
  double span = 0;
  for (unsigned b = 0; b < kClockBlocks; ++b) {
    const unsigned long long* o = h.data() + (size_t)b * kClockSamples * 2;
    const double cyc = (double)(o[2 * (kClockSamples - 1)] - o[0]), ref = (double)(o[2 * (kClockSamples - 1) + 1] - o[1]);
    if (ref > 0) { hz.push_back(cyc / ref * 1e8); span = std::max(span, ref / 1e5); }
  }
  REQUIRE(!hz.empty(), "mp_clock_sample_end: the sampler recorded nothing");
  std::sort(hz.begin(), hz.end());
  *clock_hz = hz[hz.size() / 2];
  if (sampled_ms) *sampled_ms = span;
  return MP_OK;
}

// ---------------------------------------------------------------------------------- device memory
int mp_malloc(mp_ctx* ctx, size_t bytes, void** d_ptr) {
  REQUIRE(ctx && d_ptr, "mp_malloc: null argument");
  *d_ptr = nullptr;
  CTX_ENTER(ctx);
  REQUIRE(!ctx->capturing, "mp_malloc: not allowed while a launch graph is being captured (mp_graph_begin)");
  if (bytes == 0) bytes = 16;
  bytes = (bytes + 255) & ~size_t(255);
  auto it = ctx->free_by_size.find(bytes);
  if (it != ctx->free_by_size.end() && !it->second.empty()) {
    *d_ptr = it->second.back();
    it->second.pop_back();
    return MP_OK;
  }
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e == hipErrorOutOfMemory) {  // give the pool back and retry once
    (void)hipGetLastError();
    mp_pool_trim(ctx);
    e = hipMalloc(&p, bytes);
  }
  if (e != hipSuccess) return hip_err(e, "hipMalloc");
  ctx->live[p] = bytes;
  *d_ptr = p;
  return MP_OK;
}

int mp_free(mp_ctx* ctx, void* d_ptr) {
  REQUIRE(ctx, "mp_free: null context");
  if (!d_ptr) return MP_OK;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  auto it = ctx->live.find(d_ptr);
  REQUIRE(it != ctx->live.end(), "mp_free: pointer %p was not allocated by this context", d_ptr);
  ctx->free_by_size[it->second].push_back(d_ptr);
  return MP_OK;
}

int mp_pool_trim(mp_ctx* ctx) {
  REQUIRE(ctx, "mp_pool_trim: null context");
  CTX_ENTER(ctx);
  (void)hipStreamSynchronize(ctx->compute);
  (void)hipStreamSynchronize(ctx->copy);
  for (auto& kv : ctx->free_by_size)
    for (void* p : kv.second) {
      (void)hipFree(p);
      ctx->live.erase(p);
    }
  ctx->free_by_size.clear();
  return MP_OK;
}

// page-locked host memory: DMA reads / writes it directly, so the host-buffer entry points overlap upload, kernel
// and download on such buffers (pageable buffers are staged by the runtime and serialise).  The buffers are portable
// (usable from every device) and outlive the context that allocated them: a caller may still hold views of one
// when it destroys its context, so only mp_host_free releases them.
namespace {
std::mutex g_pinned_mu;
std::map<void*, size_t> g_pinned;
}  // namespace
int mp_host_alloc(mp_ctx* ctx, size_t bytes, void** h_ptr) {
  REQUIRE(ctx && h_ptr, "mp_host_alloc: null argument");
  *h_ptr = nullptr;
  CTX_ENTER(ctx);
  void* p = nullptr;
  HIP_TRY(hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocPortable));
  {
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    g_pinned[p] = bytes;
  }
  *h_ptr = p;
  return MP_OK;
}
int mp_host_free(mp_ctx* ctx, void* h_ptr) {
  (void)ctx;  // may be null or already destroyed: the buffer does not belong to a context
  if (!h_ptr) return MP_OK;
  {
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    auto it = g_pinned.find(h_ptr);
    REQUIRE(it != g_pinned.end(), "mp_host_free: pointer %p was not allocated by mp_host_alloc", h_ptr);
    g_pinned.erase(it);
  }
  HIP_TRY(hipHostFree(h_ptr));
  return MP_OK;
}

int mp_memcpy_h2d(mp_ctx* ctx, void* d_dst, const void* h_src, size_t bytes) {
  REQUIRE(ctx && (bytes == 0 || (d_dst && h_src)), "mp_memcpy_h2d: null argument");
  if (bytes == 0) return MP_OK;
  CTX_ENTER(ctx);
  HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->compute));
  HIP_TRY(hipStreamSynchronize(ctx->compute));
  return MP_OK;
}
int mp_memcpy_d2h(mp_ctx* ctx, void* h_dst, const void* d_src, size_t bytes) {
  REQUIRE(ctx && (bytes == 0 || (h_dst && d_src)), "mp_memcpy_d2h: null argument");
  if (bytes == 0) return MP_OK;
  CTX_ENTER(ctx);
  HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->compute));
  HIP_TRY(hipStreamSynchronize(ctx->compute));
  return MP_OK;
}
int mp_memset(mp_ctx* ctx, void* d_dst, int value, size_t bytes) {
  REQUIRE(ctx && (bytes == 0 || d_dst), "mp_memset: null argument");
  if (bytes == 0) return MP_OK;
  CTX_ENTER(ctx);
  HIP_TRY(hipMemsetAsync(d_dst, value, bytes, ctx->compute));
  return MP_OK;
}

// ----------------------------------------------------------------------------------------- events
int mp_event_create(mp_ctx* ctx, mp_event** out) {
  REQUIRE(ctx && out, "mp_event_create: null argument");
  CTX_ENTER(ctx);
  mp_event* e = new (std::nothrow) mp_event;
  REQUIRE(e, "mp_event_create: out of host memory");
  e->device = ctx->device;
  hipError_t he = hipEventCreate(&e->ev);
  if (he != hipSuccess) { delete e; return hip_err(he, "hipEventCreate"); }
  *out = e;
  return MP_OK;
}
int mp_event_destroy(mp_event* ev) {
  if (!ev) return MP_OK;
  (void)hipSetDevice(ev->device);
  (void)hipEventDestroy(ev->ev);
  delete ev;
  return MP_OK;
}
int mp_event_record(mp_ctx* ctx, mp_event* ev) {
  REQUIRE(ctx && ev, "mp_event_record: null argument");
  CTX_ENTER(ctx);
  HIP_TRY(hipEventRecord(ev->ev, ctx->compute));
  return MP_OK;
}
int mp_event_elapsed_ms(mp_event* start, mp_event* stop, float* ms) {
  REQUIRE(start && stop && ms, "mp_event_elapsed_ms: null argument");
  HIP_TRY(hipSetDevice(stop->device));
  HIP_TRY(hipEventSynchronize(stop->ev));
  HIP_TRY(hipEventElapsedTime(ms, start->ev, stop->ev));
  return MP_OK;
}

// ----------------------------------------------------------------------------------------- graphs
int mp_graph_begin(mp_ctx* ctx) {
  REQUIRE(ctx, "mp_graph_begin: null context");
  CTX_ENTER(ctx);
  REQUIRE(!ctx->capturing, "mp_graph_begin: a capture is already open on this context");
  // (CTX_ENTER has run the context's own parked passes on the stream.)  Captured float32 inverse-dynamics launches park their
  // float64 passes in a pool of the graph's own: lists and counters live as long as the graph, the passes become its nodes
  mp_ctx::HardPool* pool = new (std::nothrow) mp_ctx::HardPool;
  REQUIRE(pool, "mp_graph_begin: out of host memory");
  hipError_t he = hipStreamBeginCapture(ctx->compute, hipStreamCaptureModeThreadLocal);
  if (he != hipSuccess) { delete pool; return hip_err(he, "hipStreamBeginCapture"); }
  ctx->hp = pool;
  ctx->capturing = true;
  return MP_OK;
}
int mp_graph_end(mp_ctx* ctx, mp_graph** out) {
  REQUIRE(ctx && out, "mp_graph_end: null argument");
  *out = nullptr;
  CTX_ENTER(ctx);
  REQUIRE(ctx->capturing, "mp_graph_end: no capture is open on this context");
  // (CTX_ENTER has captured the passes still parked in the capture's pool: they are the graph's last nodes)
  mp_ctx::HardPool* pool = ctx->hp;
  ctx->hp = &ctx->own_pool;
  ctx->capturing = false;
  auto drop_pool = [&] { (void)hipStreamSynchronize(ctx->compute); free_hard_pool(pool); delete pool; };
  hipGraph_t g = nullptr;
  hipError_t he = hipStreamEndCapture(ctx->compute, &g);
  if (he != hipSuccess) { drop_pool(); return hip_err(he, "hipStreamEndCapture"); }
  if (!g) drop_pool();
  REQUIRE(g, "mp_graph_end: the capture was invalidated (a non-capturable call ran between begin and end)");
  hipGraphExec_t ex = nullptr;
  he = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  if (he != hipSuccess) { (void)hipGraphDestroy(g); drop_pool(); return hip_err(he, "hipGraphInstantiate"); }
  mp_graph* gr = new (std::nothrow) mp_graph;
  if (!gr) { (void)hipGraphExecDestroy(ex); (void)hipGraphDestroy(g); drop_pool(); }
  REQUIRE(gr, "mp_graph_end: out of host memory");
  gr->graph = g; gr->exec = ex; gr->device = ctx->device; gr->ctx = ctx; gr->ctx_uid = ctx->uid; gr->pool = pool;
  ++ctx->live_graphs;
  *out = gr;
  return MP_OK;
}
int mp_graph_launch(mp_ctx* ctx, mp_graph* graph) {
  REQUIRE(ctx && graph, "mp_graph_launch: null argument");
  REQUIRE(graph->device == ctx->device, "mp_graph_launch: graph captured on device %d, context is on %d", graph->device, ctx->device);
  CTX_ENTER(ctx);
  HIP_TRY(hipGraphLaunch(graph->exec, ctx->compute));
  return MP_OK;
}
// what destroyed models left behind for the sake of live graphs (ctx->mu held, device bound, no capture open)
static void release_retired(mp_ctx* ctx) {
  (void)hipStreamSynchronize(ctx->compute);
  for (hipModule_t m : ctx->retired_mods) (void)hipModuleUnload(m);
  ctx->retired_mods.clear();
  for (void* p : ctx->retired_bufs) (void)mp_free(ctx, p);
  ctx->retired_bufs.clear();
}

int mp_graph_destroy(mp_graph* graph) {
  if (!graph) return MP_OK;
  int prev = -1;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(graph->device);
  (void)hipDeviceSynchronize();  // a replay still running writes the graph's row lists
  (void)hipGraphExecDestroy(graph->exec);
  (void)hipGraphDestroy(graph->graph);
  if (graph->pool) { free_hard_pool(graph->pool); delete graph->pool; }
  {
    std::lock_guard<std::mutex> lk(g_ctxs_mu);
    // the context may have been destroyed first (it took the retired objects with it) - and another one created at its address
    if (graph->ctx && g_ctxs.count(graph->ctx) && graph->ctx->uid == graph->ctx_uid) {
      std::lock_guard<std::recursive_mutex> cl(graph->ctx->mu);
      if (--graph->ctx->live_graphs <= 0 && !graph->ctx->capturing) {
        graph->ctx->live_graphs = 0;
        release_retired(graph->ctx);
      }
    }
  }
  delete graph;
  if (prev >= 0) (void)hipSetDevice(prev);
  return MP_OK;
}

// ------------------------------------------------------------------------------------------ model
int mp_model_create(int n, const double* S, const double* Mcom, const double* G, const double* M_ee,
                    const double* joint_limits, const double* torque_limits, mp_model** out) {
  REQUIRE(out, "mp_model_create: null output");
  *out = nullptr;
  REQUIRE(S && Mcom && G && M_ee, "mp_model_create: S, Mcom, G and M_ee are required");
  REQUIRE(n >= 1 && n <= MP_BIG_DOF, "mp_model_create: dof %d outside 1..%d", n, MP_BIG_DOF);
  mp_model* m = new (std::nothrow) mp_model;
  REQUIRE(m, "mp_model_create: out of host memory");
  char msg[400] = "";
  int rc;
  // MANIPULAPY_HIP_LOOPED=1 (tests): build every model for the run-time-n kernels, so that the looped recursions can be
  // checked against the unrolled ones and the goldens on the 6..8-joint robots too
  const char* looped = getenv("MANIPULAPY_HIP_LOOPED");
  if (n <= MP_MAX_DOF && !(looped && looped[0] == '1')) {
    std::memset(m->pmap, 0, sizeof m->pmap);
    rc = mp_compile_model(n, S, Mcom, G, M_ee, joint_limits, torque_limits, &m->d, msg, sizeof msg, m->pmap);
    if (!rc) mp_model_cast(m->d, &m->f);
  } else {  // 9..32 joints: the looped kernels' model; d / f only carry the joint count
    m->big = true;
    rc = mp_compile_model_big(n, S, Mcom, G, M_ee, joint_limits, torque_limits, &m->bd, msg, sizeof msg);
    if (!rc) {
      mp_model_cast(m->bd, &m->bf);
      std::memset(&m->d, 0, sizeof m->d);
      std::memset(&m->f, 0, sizeof m->f);
      m->d.n = n;
      m->f.n = n;
    }
  }
  if (rc) {
    delete m;
    return mp_fail(MP_ERR_MODEL, "mp_model_create: %s", msg);
  }
  static std::atomic<uint64_t> next_uid{1};
  m->uid = next_uid.fetch_add(1);
  *out = m;
  return MP_OK;
}
int mp_model_destroy(mp_model* model) {
  if (!model) return MP_OK;
  // Drop what the live contexts hold for this model: its specialised code objects and its device-resident copies.  A launch
  // graph captured on a context keeps kernel nodes of those code objects and the addresses of those copies (the handles
  // hold no reference to the models they captured), and during an open capture neither a stream synchronisation nor a
  // buffer release is legal - so with a live graph or an open capture they are RETIRED (released with the last graph, or
  // with the context) instead of released here.  Called from Python's garbage collector at arbitrary times: the calling
  // thread's current device is restored.
  int prev = -1;
  {
    std::lock_guard<std::mutex> lk(g_ctxs_mu);
    if (!g_ctxs.empty()) (void)hipGetDevice(&prev);  // (no context, no HIP call: CPU-launcher processes never touch the runtime)
    for (mp_ctx* ctx : g_ctxs) {
      std::lock_guard<std::recursive_mutex> cl(ctx->mu);
      auto sp = ctx->specs.find(model->uid);
      auto dm = ctx->dev_models.find(model->uid);
      const bool has_big = ctx->dev_big[0].count(model->uid) || ctx->dev_big[1].count(model->uid);
      if (sp == ctx->specs.end() && dm == ctx->dev_models.end() && !has_big) continue;
      const bool retire = ctx->capturing || ctx->live_graphs > 0;
      if (!ctx->capturing) {  // parked float64 passes may belong to this model's code object
        (void)hipSetDevice(ctx->device);
        (void)hard_flush(ctx);
      }
      if (!retire) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->compute);  // a launch of this model's kernels may still be in flight
      }
      if (sp != ctx->specs.end()) {
        for (hipModule_t m : {sp->second.mod_ilp, sp->second.mod}) {
          if (!m) continue;
          if (retire) ctx->retired_mods.push_back(m);
          else (void)hipModuleUnload(m);
        }
        ctx->specs.erase(sp);
      }
      auto drop = [&](void* p) {
        if (retire) ctx->retired_bufs.push_back(p);
        else (void)mp_free(ctx, p);
      };
      if (dm != ctx->dev_models.end()) { drop(dm->second); ctx->dev_models.erase(dm); }
      for (auto& table : ctx->dev_big) {
        auto it = table.find(model->uid);
        if (it != table.end()) { drop(it->second); table.erase(it); }
      }
    }
  }
  delete model;
  if (prev >= 0) (void)hipSetDevice(prev);
  return MP_OK;
}
int mp_model_dof(const mp_model* model, int* n) {
  REQUIRE(model && n, "mp_model_dof: null argument");
  *n = model->d.n;
  return MP_OK;
}
int mp_model_params(const mp_model* model, double* out) {
  REQUIRE(model && out, "mp_model_params: null argument");
  static_assert(sizeof(MpJoint<double>) == MP_JOINT_FIELDS * sizeof(double), "MpJoint layout");  // the first 16 fields are the documented ones
  for (int i = 0; i < model->d.n; ++i) std::memcpy(out + 16 * i, model->big ? &model->bd.j[i] : &model->d.j[i], 16 * sizeof(double));
  return MP_OK;
}
int mp_model_specialize_source(const mp_model* model, char* buf, size_t* len) {
  REQUIRE(model && len, "mp_model_specialize_source: null argument");
  REQUIRE_SMALL("mp_model_specialize_source");
  // both translation units, the second behind a separator line (they are compiled separately: csrc/mp_jit.cpp)
  const std::string src = mp_jit_source(model->f, model->d) + "\n// ==== second program (max-ILP scheduling strategy) ====\n" + mp_jit_source(model->f, model->d, 1);
  if (buf) {
    REQUIRE(*len >= src.size() + 1, "mp_model_specialize_source: buffer too small");
    std::memcpy(buf, src.c_str(), src.size() + 1);
  }
  *len = src.size() + 1;
  return MP_OK;
}
int mp_model_specialize_compile(const mp_model* model, size_t* code_bytes, int* from_cache) {
  REQUIRE(model, "mp_model_specialize_compile: null model");
  REQUIRE_SMALL("mp_model_specialize_compile");
  std::vector<char> code;
  std::string err;
  bool cached = false;
  if (mp_jit_compile(model->f, model->d, &code, &cached, &err)) return mp_fail(MP_ERR_UNSUPPORTED, "mp_model_specialize_compile: %s", err.c_str());
  {  // the second program (the one-row float32 inverse dynamics under the max-ILP scheduling strategy): both are needed
    std::vector<char> code2;
    bool cached2 = false;
    if (mp_jit_compile(model->f, model->d, &code2, &cached2, &err, 1)) return mp_fail(MP_ERR_UNSUPPORTED, "mp_model_specialize_compile: %s", err.c_str());
    code.insert(code.end(), code2.begin(), code2.end());   // (the size reported is both programs')
    cached = cached && cached2;
  }
  if (code_bytes) *code_bytes = code.size();
  if (from_cache) *from_cache = cached ? 1 : 0;
  return MP_OK;
}
int mp_model_is_specialized(mp_ctx* ctx, const mp_model* model, int* yes) {
  REQUIRE(ctx && model && yes, "mp_model_is_specialized: null argument");
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  *yes = ctx->specs.count(model->uid) ? 1 : 0;
  return MP_OK;
}
int mp_model_specialize(mp_ctx* ctx, const mp_model* model) {
  REQUIRE(ctx && model, "mp_model_specialize: null argument");
  REQUIRE_SMALL("mp_model_specialize");
  CTX_ENTER(ctx);
  if (ctx->specs.count(model->uid)) return MP_OK;
  std::vector<char> code;
  std::string err;
  if (mp_jit_compile(model->f, model->d, &code, nullptr, &err)) return mp_fail(MP_ERR_UNSUPPORTED, "mp_model_specialize: %s", err.c_str());
  MpSpec sp;
  HIP_TRY(hipModuleLoadData(&sp.mod, code.data()));
  // every kernel of the two programs is required: a program that lacks one is refused and the generic kernels serve
  const char* names[9][2] = {{"mp_spec_traj_id_pk_f0", "mp_spec_traj_id_pk_f1"}, {"mp_spec_fd_traj_f0", "mp_spec_fd_traj_f1"},
                            {"mp_spec_id_d_f0", "mp_spec_id_d_f1"}, {"mp_spec_fk_jac_id_d_f0", "mp_spec_fk_jac_id_d_f1"},
                            {"mp_spec_fd_s_f0", "mp_spec_fd_s_f1"}, {"mp_spec_fd_d_f0", "mp_spec_fd_d_f1"},
                            {"mp_spec_fd_traj_tm_f0", "mp_spec_fd_traj_tm_f1"}, {"mp_spec_id_hard_f0", "mp_spec_id_hard_f1"},
                            {"mp_spec_traj_id_hard_f0", "mp_spec_traj_id_hard_f1"}};
  hipFunction_t* slots[9] = {sp.traj_id_pk, sp.fd_traj, sp.id_d, sp.fk_jac_id_d, sp.fd_s, sp.fd_d, sp.fd_traj_tm, sp.id_hard, sp.traj_id_hard};
  for (int k = 0; k < 9; ++k)
    for (int f = 0; f < 2; ++f) {
      hipError_t e = hipModuleGetFunction(&slots[k][f], sp.mod, names[k][f]);
      if (e != hipSuccess) { (void)hipModuleUnload(sp.mod); return hip_err(e, names[k][f]); }
    }
  {
    hipError_t e = hipModuleGetFunction(&sp.ik, sp.mod, "mp_spec_ik");
    if (e != hipSuccess) { (void)hipModuleUnload(sp.mod); return hip_err(e, "mp_spec_ik"); }
  }
  // The second program: the float32 inverse dynamics, one row per lane - mp_spec_id_co (whole waves, rows as whole lines) and
  // mp_spec_id_s (the last < 64 rows) - compiled with LLVM's max-ILP scheduling strategy (c2 0.0704 -> 0.0695 ms, c4 0.1417 -> 0.1411;
  // as a flag for the whole program it costs the float64 and fused kernels as much as it gives: profiles/r02_d_c5_experiments.txt)
  {
    std::vector<char> code2;
    hipModule_t m2 = nullptr;
    if (mp_jit_compile(model->f, model->d, &code2, nullptr, &err, 1)) {
      (void)hipModuleUnload(sp.mod);
      return mp_fail(MP_ERR_UNSUPPORTED, "mp_model_specialize: %s", err.c_str());
    }
    hipError_t e = hipModuleLoadData(&m2, code2.data());
    if (e != hipSuccess) { (void)hipModuleUnload(sp.mod); return hip_err(e, "hipModuleLoadData (second program)"); }
    const char* names2[2][2] = {{"mp_spec_id_s_f0", "mp_spec_id_s_f1"}, {"mp_spec_id_co_f0", "mp_spec_id_co_f1"}};
    hipFunction_t* slots2[2] = {sp.id_s, sp.id_co};
    for (int k = 0; k < 2; ++k)
      for (int f = 0; f < 2; ++f) {
        e = hipModuleGetFunction(&slots2[k][f], m2, names2[k][f]);
        if (e != hipSuccess) { (void)hipModuleUnload(m2); (void)hipModuleUnload(sp.mod); return hip_err(e, names2[k][f]); }
      }
    sp.mod_ilp = m2;
  }
  // Self-check of THIS code object's non-finite guard.  The specialised kernels are built with -ffinite-math-only; their guard
  // works on bit patterns (csrc/mp_core.h) and today's compiler leaves it alone, but that flag would let a future one fold it.
  // A row with a NaN and a row with an infinity must come back NaN and their neighbours finite - from the per-lane float32 kernel,
  // the whole-line one (whose finite rows must carry the per-lane kernel's bits) and the float64 kernel - or the code object is
  // refused and the generic kernels (built without the flag) serve.
  {
    const int n = model->d.n;
    const long rows = 128;
    std::vector<float> h((size_t)rows * n, 0.25f), out((size_t)rows * n * 2, 0.0f);
    std::vector<double> hd((size_t)rows * n, 0.25), outd((size_t)rows * n, 0.0);
    h[3 * n] = __builtin_nanf(""); h[(size_t)70 * n + (n > 1 ? 1 : 0)] = __builtin_inff();
    hd[3 * n] = __builtin_nan(""); hd[(size_t)70 * n + (n > 1 ? 1 : 0)] = -__builtin_inf();
    const size_t fb = h.size() * sizeof(float), db = hd.size() * sizeof(double);
    Scratch sc(ctx);
    void *dq, *dz, *d0, *d1, *dqd, *dzd, *d2;
    auto unload = [&] { (void)hipModuleUnload(sp.mod_ilp); (void)hipModuleUnload(sp.mod); };
    {  // an allocation that fails (out of memory, an open graph capture) must not leak the two code objects loaded above
      void** slot[7] = {&dq, &dz, &d0, &d1, &dqd, &dzd, &d2};
      for (int k = 0; k < 7; ++k)
        if (int rc = sc.get(k < 4 ? fb : db, slot[k])) { unload(); return rc; }
    }
    hipError_t he = hipMemcpyAsync(dq, h.data(), fb, hipMemcpyHostToDevice, ctx->compute);
    if (he == hipSuccess) he = hipMemsetAsync(dz, 0, fb, ctx->compute);
    if (he == hipSuccess) he = hipMemcpyAsync(dqd, hd.data(), db, hipMemcpyHostToDevice, ctx->compute);
    if (he == hipSuccess) he = hipMemsetAsync(dzd, 0, db, ctx->compute);
    if (he != hipSuccess) { unload(); return hip_err(he, "mp_model_specialize: self-check upload"); }
    MpCall<float> cf;
    MpCall<double> cd;
    make_call<float>(model, nullptr, nullptr, &cf);
    make_call<double>(model, nullptr, nullptr, &cd);
    long nr = rows;
    const float *q = (const float*)dq, *z = (const float*)dz;
    float *o0 = (float*)d0, *o1 = (float*)d1;
    const double *qd_ = (const double*)dqd, *zd = (const double*)dzd;
    double* o2 = (double*)d2;
    MpLead no_lead;
    std::memset(&no_lead, 0, sizeof no_lead);
    void* a0[] = {&cf, &q, &z, &z, &o0, &nr};
    void* a1[] = {&cf, &q, &z, &z, &o1, &nr, &no_lead};
    void* a2[] = {&cd, &qd_, &zd, &zd, &o2, &nr};
    int rc = launch_spec(ctx, sp.id_s[0], rows, a0);
    if (!rc) rc = launch_spec(ctx, sp.id_co[0], rows, a1, MP_JIT_ID_CO_BLOCK);
    if (!rc) rc = launch_spec(ctx, sp.id_d[0], rows, a2);
    if (rc) { unload(); return rc; }
    he = hipMemcpyAsync(out.data(), d0, fb, hipMemcpyDeviceToHost, ctx->compute);
    if (he == hipSuccess) he = hipMemcpyAsync(out.data() + h.size(), d1, fb, hipMemcpyDeviceToHost, ctx->compute);
    if (he == hipSuccess) he = hipMemcpyAsync(outd.data(), d2, db, hipMemcpyDeviceToHost, ctx->compute);
    if (he == hipSuccess) he = hipStreamSynchronize(ctx->compute);
    if (he != hipSuccess) { unload(); return hip_err(he, "mp_model_specialize: self-check download"); }
    bool ok = true;
    for (int k = 0; k < 3 && ok; ++k) {  // 0: one row per lane, 1: whole-line row movement, 2: float64
      for (long r : {3L, 70L, 4L, 69L, 0L, 127L}) {
        const bool want_nan = r == 3 || r == 70;
        for (int j = 0; j < n; ++j) {
          const double v = k == 2 ? outd[(size_t)r * n + j] : (double)out[(size_t)k * h.size() + (size_t)r * n + j];
          if ((v != v) != want_nan) ok = false;
          if (k == 1 && !want_nan && out[h.size() + (size_t)r * n + j] != out[(size_t)r * n + j]) ok = false;  // = the per-lane kernel's bits
        }
      }
    }
    if (!ok) {
      unload();
      return mp_fail(MP_ERR_UNSUPPORTED, "mp_model_specialize: the specialised kernels of this toolchain do not keep the non-finite row "
                                         "contract (self-check failed); the generic kernels are used instead");
    }
  }
  ctx->specs[model->uid] = sp;
  return MP_OK;
}
int mp_model_blob(const mp_model* model, int use_f64, void* out, size_t* bytes) {
  REQUIRE(model && bytes, "mp_model_blob: null argument");
  const size_t need = model->big ? (use_f64 ? sizeof(MpBigModel<double>) : sizeof(MpBigModel<float>))
                                 : (use_f64 ? sizeof(MpModel<double>) : sizeof(MpModel<float>));
  if (out) {
    REQUIRE(*bytes >= need, "mp_model_blob: buffer of %zu bytes, need %zu", *bytes, need);
    const void* src = model->big ? (use_f64 ? (const void*)&model->bd : (const void*)&model->bf)
                                 : (use_f64 ? (const void*)&model->d : (const void*)&model->f);
    std::memcpy(out, src, need);
  }
  *bytes = need;
  return MP_OK;
}
int mp_model_fk_host(const mp_model* model, const double* q, double* T) {
  REQUIRE(model && q && T, "mp_model_fk_host: null argument");
  if (model->big) mp_compiled_fk(model->bd, q, T);
  else mp_compiled_fk(model->d, q, T);
  return MP_OK;
}

// ---------------------------------------------------------------------- hot path, device pointers
#define CHECK_COMMON(fn)                                              \
  REQUIRE(ctx && model, fn ": null context or model");                \
  CTX_ENTER(ctx);

int mp_batch_trajectory_f32(mp_ctx* ctx, const mp_model* model, const float* d_start, const float* d_end, int64_t B,
                            int64_t N, double Tf, int method, float* d_pos, float* d_vel, float* d_acc) {
  CHECK_COMMON("mp_batch_trajectory_f32");
  REQUIRE(B >= 0 && N >= 0, "mp_batch_trajectory_f32: negative B (%lld) or N (%lld)", (long long)B, (long long)N);
  if (B == 0 || N == 0) return MP_OK;
  REQUIRE(d_start && d_end && d_pos && d_vel && d_acc, "mp_batch_trajectory_f32: null device pointer");
  REQUIRE(aligned16(d_start) && aligned16(d_end) && aligned16(d_pos) && aligned16(d_vel) && aligned16(d_acc),
          "mp_batch_trajectory_f32: device pointers must be 16-byte aligned");
  PROFILE_SCOPE(ctx, "mp_batch_trajectory_f32");
  if (model->big) {
    const MpBigModel<float>* dm = nullptr;
    if (int rc = device_big_model<float>(ctx, model, &dm)) return rc;
    MpCall<float> c0 = {};
    HIP_TRY(mpk_dyn_traj(ctx->compute, model->d.n, dm, c0, false, d_start, d_end, (long)B, (long)N, Tf, method, d_pos, d_vel, d_acc, nullptr));
    return MP_OK;
  }
  HIP_TRY(mpk_batch_traj(ctx->compute, model->f, d_start, d_end, (long)B, (long)N, Tf, method, d_pos, d_vel, d_acc));
  return MP_OK;
}

int mp_id_trajectory_f32(mp_ctx* ctx, const mp_model* model, const float* d_q, const float* d_qd, const float* d_qdd,
                         int64_t rows, const double* g, const double* Ftip, float* d_tau) {
  return id_impl<float>("mp_id_trajectory_f32", ctx, model, d_q, d_qd, d_qdd, rows, g, Ftip, d_tau);
}
int mp_id_trajectory_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd,
                         const double* d_qdd, int64_t rows, const double* g, const double* Ftip, double* d_tau) {
  return id_impl<double>("mp_id_trajectory_f64", ctx, model, d_q, d_qd, d_qdd, rows, g, Ftip, d_tau);
}

int mp_traj_id_fused_f32(mp_ctx* ctx, const mp_model* model, const float* d_start, const float* d_end, int64_t B,
                         int64_t N, double Tf, int method, const double* g, const double* Ftip, float* d_tau) {
  REQUIRE(ctx && model, "mp_traj_id_fused_f32: null context or model");
  CTX_ENTER_NOJOIN(ctx);
  {  // parked float64 passes run first only where they touch this launch's arrays (as in id_impl): its own pass is parked too
    const size_t in_b = (size_t)(B > 0 ? B : 0) * (size_t)model->d.n * sizeof(float), out_b = in_b * (size_t)(N > 0 ? N : 0);
    const void* lo[3] = {d_start, d_end, d_tau};
    const size_t by[3] = {in_b, in_b, out_b};
    if (int rc = ctx->profiling ? hard_flush(ctx) : hard_flush_if_overlapping(ctx, lo, by, 3)) return rc;
  }
  REQUIRE(B >= 0 && N >= 0, "mp_traj_id_fused_f32: negative B (%lld) or N (%lld)", (long long)B, (long long)N);
  if (B == 0 || N == 0) return MP_OK;
  REQUIRE(d_start && d_end && d_tau, "mp_traj_id_fused_f32: null device pointer");
  REQUIRE(aligned16(d_start) && aligned16(d_end) && aligned16(d_tau),
          "mp_traj_id_fused_f32: device pointers must be 16-byte aligned");
  MpCall<float> c;
  make_call_f32(ctx, model, g, Ftip, &c);
  const bool ftip = any_nonzero(Ftip);
  PROFILE_SCOPE(ctx, "mp_traj_id_fused_f32");
  if (model->big) {
    const MpBigModel<float>* dm = nullptr;
    if (int rc = device_big_model<float>(ctx, model, &dm)) return rc;
    if (int rc = big_cold_model(ctx, model, &c)) return rc;
    HIP_TRY(mpk_dyn_traj(ctx->compute, model->d.n, dm, c, ftip, d_start, d_end, (long)B, (long)N, Tf, method, nullptr, nullptr, nullptr, d_tau));
    return MP_OK;
  }
  // per-timestep table of (s, s', s''): rebuilt on the stream only when (N, Tf, method) differ from the last call
  if (ctx->tab_cap < (long)N) {
    REQUIRE(!ctx->capturing, "mp_traj_id_fused_f32: the first call for this N allocates; run it once before capturing a launch graph");
    if (int rc = hard_flush(ctx)) return rc;      // parked passes of fused launches read the old table
    HIP_TRY(hipStreamSynchronize(ctx->compute));  // earlier kernels may still read the old table
    if (ctx->time_tab && ctx->tab_volatile) ctx->retired_tabs.push_back(ctx->time_tab);  // a launch graph still points at it
    else if (ctx->time_tab) (void)hipFree(ctx->time_tab);
    ctx->time_tab = nullptr; ctx->tab_cap = 0; ctx->tab_Nt = -1;
    HIP_TRY(hipMalloc((void**)&ctx->time_tab, (size_t)N * 3 * sizeof(double)));
    ctx->tab_cap = (long)N;
  }
  // A captured call RECORDS its table kernel (the graph is self-contained), and every later replay rewrites the shared
  // table behind the cache's back - so once a capture has happened on this context the cache is off for good: every
  // call then writes its own table first (one extra ~2 us kernel, stream-ordered before the kernel that reads it).
  if (ctx->capturing) ctx->tab_volatile = true;
  if (ctx->tab_volatile || ctx->tab_Nt != (long)N || ctx->tab_Tf != Tf || ctx->tab_method != method) {
    if (int rc = hard_flush(ctx)) return rc;      // (as above)
    HIP_TRY(mpk_time_table(ctx->compute, ctx->time_tab, (long)N, Tf, method));
    ctx->tab_Nt = (long)N; ctx->tab_Tf = Tf; ctx->tab_method = method;
  }
  if (const MpSpec* sp = find_spec(ctx, model)) {
    long nt = (long)N;
    const double* tab = ctx->time_tab;
    unsigned bpt = mpk_traj_blocks_per_trajectory(nt);
    const long rows_l = (long)B * (long)N;
    mp_ctx::HardSlot* hs = attach_hard_list(ctx, rows_l, &c);
    // (as launch_id: one parked pass of an earlier fused launch of this program rides with this launch's first workgroups)
    MpLead lead;
    std::memset(&lead, 0, sizeof lead);
    mp_ctx::HardSlot* rider = !ctx->tab_volatile ? pick_rider(ctx, sp->traj_id_hard[ftip ? 1 : 0], hs, true) : nullptr;
    if (rider) {
      lead.C = rider->C; lead.q = rider->q; lead.qd = rider->qd; lead.qdd = rider->qdd; lead.tau = rider->tau; lead.rows = rider->nrows;
      lead.nt = rider->nt;
      lead.blocks = std::min((hard_pass_blocks((long)rider->nrows) + 3u) / 4u, 128u);   // 256-lane workgroups
    }
    void* args[] = {&c, &d_start, &d_end, &nt, &bpt, &tab, &d_tau, &lead};
    {
      const unsigned grid = (unsigned)((long)B * bpt) + lead.blocks;
      HIP_TRY(hipModuleLaunchKernel(sp->traj_id_pk[ftip ? 1 : 0], grid, 1, 1, 256, 1, 1, 0, ctx->compute, args, nullptr));
    }
    if (rider) { rider->busy = false; rider->orphan = false; }
    if (!hs) return MP_OK;
    // the generated rows' float64 pass is parked like a given-rows launch's; it reads the time table, so a call that rewrites the
    // table runs the parked passes first (above)
    hard_defer_generated(ctx, hs, sp->traj_id_hard[ftip ? 1 : 0], c, d_start, d_end, tab, d_tau, rows_l, model->d.n, (long)B, (unsigned)N);
    if (ctx->tab_volatile) return hard_flush(ctx);  // (a table rewritten by every call cannot wait for a parked pass)
    return hard_park_or_run(ctx, d_start, d_end, nullptr, d_tau, (size_t)rows_l * (size_t)model->d.n * sizeof(float), (size_t)B * (size_t)model->d.n * sizeof(float));
  }
  {
    // generic kernels: the same hand-over (the float64 model and the float32 limits come from the device copy)
    const long rows_l = (long)B * (long)N;
    mp_ctx::HardSlot* hs = nullptr;
    const MpModel<float>* dm = nullptr;
    if (c.cold_model && device_model(ctx, model, &dm) == MP_OK) hs = attach_hard_list(ctx, rows_l, &c);
    HIP_TRY(mpk_traj_id_tab(ctx->compute, model->f, c, ftip, d_start, d_end, (long)B, (long)N, ctx->time_tab, d_tau));
    if (hs) {
      HIP_TRY(mpk_traj_id_hard(ctx->compute, dm, model->d.n, c, ftip, d_start, d_end, (unsigned)N, ctx->time_tab, d_tau, (unsigned)rows_l,
                               hard_pass_blocks(rows_l)));
      (void)hard_passed(hs, MP_OK);
    }
  }
  return MP_OK;
}

int mp_fk_jac_id_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_qdd,
                     int64_t rows, const double* g, const double* Ftip, double* d_T, double* d_J, double* d_tau) {
  return fkjid_impl<double>("mp_fk_jac_id_f64", ctx, model, d_q, d_qd, d_qdd, rows, g, Ftip, d_T, d_J, d_tau);
}
int mp_fk_jac_id_f32(mp_ctx* ctx, const mp_model* model, const float* d_q, const float* d_qd, const float* d_qdd,
                     int64_t rows, const double* g, const double* Ftip, float* d_T, float* d_J, float* d_tau) {
  return fkjid_impl<float>("mp_fk_jac_id_f32", ctx, model, d_q, d_qd, d_qdd, rows, g, Ftip, d_T, d_J, d_tau);
}

// ------------------------------------------------------------------------ hot path, host pointers
int mp_batch_trajectory_host_f32(mp_ctx* ctx, const mp_model* model, const float* start, const float* end, int64_t B,
                                 int64_t N, double Tf, int method, float* pos, float* vel, float* acc) {
  CHECK_COMMON("mp_batch_trajectory_host_f32");
  REQUIRE(B >= 0 && N >= 0, "mp_batch_trajectory_host_f32: negative B or N");
  if (B == 0 || N == 0) return MP_OK;
  REQUIRE(start && end && pos && vel && acc, "mp_batch_trajectory_host_f32: null host pointer");
  const size_t n = (size_t)model->d.n, in_b = (size_t)B * n * sizeof(float), out_b = (size_t)B * (size_t)N * n * sizeof(float);
  HostCall h(ctx);
  const float *ds = h.in(start, in_b), *de = h.in(end, in_b);
  float *dp = h.out(pos, out_b), *dv = h.out(vel, out_b), *da = h.out(acc, out_b);
  return h.run([&] { return mp_batch_trajectory_f32(ctx, model, ds, de, B, N, Tf, method, dp, dv, da); });
}

int mp_id_trajectory_host_f32(mp_ctx* ctx, const mp_model* model, const float* q, const float* qd, const float* qdd,
                              int64_t rows, const double* g, const double* Ftip, float* tau) {
  return id_host_impl<float>("mp_id_trajectory_host_f32", ctx, model, q, qd, qdd, rows, g, Ftip, tau);
}
int mp_id_trajectory_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd,
                              const double* qdd, int64_t rows, const double* g, const double* Ftip, double* tau) {
  return id_host_impl<double>("mp_id_trajectory_host_f64", ctx, model, q, qd, qdd, rows, g, Ftip, tau);
}

int mp_traj_id_fused_host_f32(mp_ctx* ctx, const mp_model* model, const float* start, const float* end, int64_t B,
                              int64_t N, double Tf, int method, const double* g, const double* Ftip, float* tau) {
  CHECK_COMMON("mp_traj_id_fused_host_f32");
  REQUIRE(B >= 0 && N >= 0, "mp_traj_id_fused_host_f32: negative B or N");
  if (B == 0 || N == 0) return MP_OK;
  REQUIRE(start && end && tau, "mp_traj_id_fused_host_f32: null host pointer");
  const size_t n = (size_t)model->d.n, in_b = (size_t)B * n * sizeof(float), out_b = (size_t)B * (size_t)N * n * sizeof(float);
  HostCall h(ctx);
  const float *ds = h.in(start, in_b), *de = h.in(end, in_b);
  float* dt = h.out(tau, out_b);
  return h.run([&] { return mp_traj_id_fused_f32(ctx, model, ds, de, B, N, Tf, method, g, Ftip, dt); });
}

int mp_fk_jac_id_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd, const double* qdd,
                          int64_t rows, const double* g, const double* Ftip, double* T, double* J, double* tau) {
  CHECK_COMMON("mp_fk_jac_id_host_f64");
  REQUIRE(rows >= 0, "mp_fk_jac_id_host_f64: negative row count");
  if (rows == 0) return MP_OK;
  REQUIRE(q && (T || J || tau), "mp_fk_jac_id_host_f64: q and at least one output are required");
  REQUIRE(!tau || (qd && qdd), "mp_fk_jac_id_host_f64: tau requested without qd / qdd");
  const int64_t n = model->d.n;
  const size_t row_b = (size_t)n * sizeof(double);
  HostCall h(ctx, rows);
  const double *dq = h.in_rows(q, row_b), *dqd = h.in_rows(tau ? qd : nullptr, row_b), *dqdd = h.in_rows(tau ? qdd : nullptr, row_b);
  double *dT = h.out_rows(T, 16 * sizeof(double)), *dJ = h.out_rows(J, 6 * row_b), *dt = h.out_rows(tau, row_b);
  const int64_t chunk = host_chunk_rows();  // pipelined from two chunks on: the download is much the larger direction
  return h.run_rows(chunk, chunk + 1, [&](int64_t r0, int64_t nr) {
    return mp_fk_jac_id_f64(ctx, model, dq + r0 * n, at(dqd, r0 * n), at(dqdd, r0 * n), nr, g, Ftip, at(dT, r0 * 16), at(dJ, r0 * 6 * n),
                            at(dt, r0 * n));
  });
}

int mp_mass_matrix_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, int64_t rows, double* d_M) {
  return mm_impl<double>("mp_mass_matrix_f64", ctx, model, d_q, rows, d_M);
}
int mp_mass_matrix_f32(mp_ctx* ctx, const mp_model* model, const float* d_q, int64_t rows, float* d_M) {
  return mm_impl<float>("mp_mass_matrix_f32", ctx, model, d_q, rows, d_M);
}
int mp_forward_dynamics_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_tau,
                            int64_t rows, const double* g, const double* Ftip, double* d_qdd) {
  return fdyn_impl<double>("mp_forward_dynamics_f64", ctx, model, d_q, d_qd, d_tau, rows, g, Ftip, d_qdd);
}
int mp_forward_dynamics_f32(mp_ctx* ctx, const mp_model* model, const float* d_q, const float* d_qd, const float* d_tau,
                            int64_t rows, const double* g, const double* Ftip, float* d_qdd) {
  return fdyn_impl<float>("mp_forward_dynamics_f32", ctx, model, d_q, d_qd, d_tau, rows, g, Ftip, d_qdd);
}
int mp_id_derivatives_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_qdd,
                          int64_t rows, const double* g, const double* Ftip, double* d_tau, double* d_dtau_dq, double* d_dtau_dqd,
                          double* d_M) {
  return deriv_impl("mp_id_derivatives_f64", false, ctx, model, d_q, d_qd, d_qdd, rows, g, Ftip, d_tau, d_dtau_dq, d_dtau_dqd, d_M);
}
int mp_fd_derivatives_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_tau,
                          int64_t rows, const double* g, const double* Ftip, double* d_qdd, double* d_dqdd_dq, double* d_dqdd_dqd,
                          double* d_Minv) {
  return deriv_impl("mp_fd_derivatives_f64", true, ctx, model, d_q, d_qd, d_tau, rows, g, Ftip, d_qdd, d_dqdd_dq, d_dqdd_dqd, d_Minv);
}
int mp_id_vjp_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_qdd, const double* d_gtau,
                  int64_t rows, const double* g, const double* Ftip, double* d_gq, double* d_gqd, double* d_gqdd) {
  return vjp_impl("mp_id_vjp_f64", false, ctx, model, d_q, d_qd, d_qdd, d_gtau, rows, g, Ftip, nullptr, d_gq, d_gqd, d_gqdd);
}
int mp_fd_vjp_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_tau, const double* d_gqdd,
                  int64_t rows, const double* g, const double* Ftip, double* d_qdd, double* d_gq, double* d_gqd, double* d_gtau) {
  return vjp_impl("mp_fd_vjp_f64", true, ctx, model, d_q, d_qd, d_tau, d_gqdd, rows, g, Ftip, d_qdd, d_gq, d_gqd, d_gtau);
}
int mp_fk_jac_vjp_f64(mp_ctx* ctx, const mp_model* model, int frame, const double* d_q, const double* d_gT, const double* d_gJ,
                      int64_t rows, double* d_T, double* d_J, double* d_gq) {
  return kin_vjp_impl("mp_fk_jac_vjp_f64", ctx, model, frame, d_q, d_gT, d_gJ, rows, d_T, d_J, d_gq);
}
int mp_opspace_f64(mp_ctx* ctx, const mp_model* model, int frame, int task, double damping, const double* d_q, const double* d_qd,
                   int64_t rows, const double* g, double* d_T, double* d_J, double* d_Jdqd, double* d_Lambda, double* d_Jbar, double* d_mu,
                   double* d_p) {
  return opspace_impl("mp_opspace_f64", ctx, model, frame, task, damping, d_q, d_qd, rows, g, d_T, d_J, d_Jdqd, d_Lambda, d_Jbar, d_mu, d_p);
}
int mp_opspace_torque_f64(mp_ctx* ctx, const mp_model* model, int frame, int task, double damping, const double* d_q, const double* d_qd,
                          const double* d_acc, const double* d_tau0, int64_t rows, const double* g, double* d_tau) {
  return opspace_torque_impl("mp_opspace_torque_f64", ctx, model, frame, task, damping, d_q, d_qd, d_acc, d_tau0, rows, g, d_tau);
}
int mp_id_regressor_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_qdd, int64_t rows,
                        const double* g, const double* Ftip, double* d_Y, double* d_tau_ext) {
  return regressor_impl("mp_id_regressor_f64", ctx, model, d_q, d_qd, d_qdd, rows, g, Ftip, d_Y, d_tau_ext);
}
int64_t mp_id_regressor_normal_workspace_bytes(const mp_model* model, int64_t rows) {
  if (!model) return -mp_fail(MP_ERR_INVALID, "mp_id_regressor_normal_workspace_bytes: null model");
  if (rows < 0) return -mp_fail(MP_ERR_INVALID, "mp_id_regressor_normal_workspace_bytes: negative row count");
  if (model->big) return -mp_too_many_joints("mp_id_regressor_normal_workspace_bytes", model->d.n);
  return regressor_normal_work_bytes(model->d.n, rows);
}
int mp_id_regressor_normal_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_qd, const double* d_qdd,
                               const double* d_rhs, int64_t rows, const double* g, const double* Ftip, void* d_work, double* d_A,
                               double* d_b, double* d_rr) {
  return regressor_normal_impl("mp_id_regressor_normal_f64", ctx, model, d_q, d_qd, d_qdd, d_rhs, rows, g, Ftip, d_work, d_A, d_b, d_rr);
}
int64_t mp_fd_trajectory_vjp_workspace_bytes(const mp_model* model, int64_t B, int64_t N, int intRes) {
  if (!model) return -mp_fail(MP_ERR_INVALID, "mp_fd_trajectory_vjp_workspace_bytes: null model");
  if (B < 0 || N < 0 || intRes < 1)
    return -mp_fail(MP_ERR_INVALID, "mp_fd_trajectory_vjp_workspace_bytes: negative B or N, or intRes < 1");
  return vjp_work_doubles(model->d.n, B, N, intRes) * (int64_t)sizeof(double);
}
int mp_fd_trajectory_vjp_tm_f64(mp_ctx* ctx, const mp_model* model, const double* d_theta0, const double* d_dtheta0,
                                const double* d_taumat, const double* d_Ftipmat, int64_t B, int64_t N, const double* g, double dt,
                                int intRes, const double* d_gpos, const double* d_gvel, const double* d_gacc, void* d_work,
                                double* d_gtheta0, double* d_gdtheta0, double* d_gtaumat) {
  return fdtraj_vjp_impl("mp_fd_trajectory_vjp_tm_f64", ctx, model, d_theta0, d_dtheta0, d_taumat, d_Ftipmat, B, N, g, dt, intRes, d_gpos,
                         d_gvel, d_gacc, d_work, d_gtheta0, d_gdtheta0, d_gtaumat);
}
int mp_fd_trajectory_vjp_host_f64(mp_ctx* ctx, const mp_model* model, const double* theta0, const double* dtheta0,
                                  const double* taumat, const double* Ftipmat, int64_t B, int64_t N, const double* g, double dt,
                                  int intRes, const double* gpos, const double* gvel, const double* gacc, double* gtheta0,
                                  double* gdtheta0, double* gtaumat) {
  return fdtraj_vjp_host_impl("mp_fd_trajectory_vjp_host_f64", ctx, model, theta0, dtheta0, taumat, Ftipmat, B, N, g, dt, intRes, gpos,
                              gvel, gacc, gtheta0, gdtheta0, gtaumat);
}
int64_t mp_ilqr_backward_workspace_bytes(const mp_model* model, int64_t B, int64_t N) {
  if (!model) return -mp_fail(MP_ERR_INVALID, "mp_ilqr_backward_workspace_bytes: null model");
  if (B < 0 || N < 2) return -mp_fail(MP_ERR_INVALID, "mp_ilqr_backward_workspace_bytes: negative B, or N < 2");
  if (model->big) return -mp_too_many_joints("mp_ilqr_backward_workspace_bytes", model->d.n);
  return ilqr_lane_variant() ? B * (int64_t)mp_ilqr_work_doubles(model->d.n) * (int64_t)sizeof(double) : 0;
}
int mp_ilqr_backward_tm_f64(mp_ctx* ctx, const mp_model* model, const double* d_pos, const double* d_vel, const double* d_taumat,
                            const double* d_dqdd_dq, const double* d_dqdd_dqd, const double* d_Minv, const double* d_xref,
                            const double* wq, const double* wr, const double* wf, const double* d_reg, int64_t B, int64_t N, double dt,
                            void* d_work, double* d_K, double* d_k, double* d_dV, int32_t* d_status) {
  return ilqr_backward_impl("mp_ilqr_backward_tm_f64", ctx, model, d_pos, d_vel, d_taumat, d_dqdd_dq, d_dqdd_dqd, d_Minv, d_xref, wq, wr, wf,
                            d_reg, B, N, dt, false, d_work, d_K, d_k, d_dV, d_status);
}
int mp_ilqr_rollout_tm_f64(mp_ctx* ctx, const mp_model* model, const double* d_theta0, const double* d_dtheta0, const double* d_taumat,
                           const double* d_pos, const double* d_vel, const double* d_K, const double* d_k, const double* d_alpha,
                           const double* d_xref, const double* wq, const double* wr, const double* wf, int64_t A, int64_t B, int64_t N,
                           const double* g, double dt, double* d_cost, double* d_opos, double* d_ovel, double* d_otau) {
  return ilqr_rollout_impl("mp_ilqr_rollout_tm_f64", ctx, model, d_theta0, d_dtheta0, d_taumat, d_pos, d_vel, d_K, d_k, d_alpha, d_xref, wq,
                           wr, wf, A, B, N, g, dt, false, d_cost, d_opos, d_ovel, d_otau);
}
int mp_ilqr_backward_host_f64(mp_ctx* ctx, const mp_model* model, const double* pos, const double* vel, const double* taumat,
                              const double* xref, const double* wq, const double* wr, const double* wf, const double* reg, int64_t B,
                              int64_t N, const double* g, double dt, double* K, double* k, double* dV, int32_t* status) {
  return ilqr_backward_host_impl("mp_ilqr_backward_host_f64", ctx, model, pos, vel, taumat, xref, wq, wr, wf, reg, B, N, g, dt, K, k, dV,
                                 status);
}
int mp_ilqr_rollout_host_f64(mp_ctx* ctx, const mp_model* model, const double* theta0, const double* dtheta0, const double* taumat,
                             const double* pos, const double* vel, const double* K, const double* k, const double* alpha,
                             const double* xref, const double* wq, const double* wr, const double* wf, int64_t A, int64_t B, int64_t N,
                             const double* g, double dt, double* cost, double* opos, double* ovel, double* otau) {
  return ilqr_rollout_host_impl("mp_ilqr_rollout_host_f64", ctx, model, theta0, dtheta0, taumat, pos, vel, K, k, alpha, xref, wq, wr, wf, A,
                                B, N, g, dt, cost, opos, ovel, otau);
}
int mp_path_dynamics_f64(mp_ctx* ctx, const mp_model* model, const double* d_q, const double* d_dq, const double* d_ddq, int64_t rows,
                         const double* velocity_limits, const double* g, const double* Ftip, double* d_a, double* d_b, double* d_c,
                         double* d_xbar) {
  return path_dynamics_impl("mp_path_dynamics_f64", ctx, model, d_q, d_dq, d_ddq, rows, velocity_limits, g, Ftip, d_a, d_b, d_c, d_xbar);
}
int mp_toppra_tm_f64(mp_ctx* ctx, const mp_model* model, const double* d_a, const double* d_b, const double* d_c, const double* d_xbar,
                     const double* d_dq, const double* d_ddq, const double* torque_limits, const double* acceleration_limits,
                     const double* d_sd_start, const double* d_sd_end, int64_t B, int64_t N, double* d_K, double* d_x, double* d_u,
                     double* d_t, double* d_duration, int32_t* d_status, double* d_qd, double* d_qdd, double* d_tau) {
  return toppra_tm_impl("mp_toppra_tm_f64", ctx, model, d_a, d_b, d_c, d_xbar, d_dq, d_ddq, torque_limits, acceleration_limits, d_sd_start,
                        d_sd_end, B, N, d_K, d_x, d_u, d_t, d_duration, d_status, d_qd, d_qdd, d_tau);
}
int mp_toppra_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* dq, const double* ddq,
                       const double* velocity_limits, const double* torque_limits, const double* acceleration_limits,
                       const double* sd_start, const double* sd_end, int64_t B, int64_t N, const double* g, const double* Ftip, double* K,
                       double* x, double* u, double* t, double* duration, int32_t* status, double* qd, double* qdd, double* tau) {
  return toppra_host_impl("mp_toppra_host_f64", ctx, model, q, dq, ddq, velocity_limits, torque_limits, acceleration_limits, sd_start,
                          sd_end, B, N, g, Ftip, K, x, u, t, duration, status, qd, qdd, tau);
}
int mp_fd_trajectory_f32(mp_ctx* ctx, const mp_model* model, const float* d_theta0, const float* d_dtheta0,
                         const float* d_taumat, const float* d_Ftipmat, int64_t B, int64_t N, const double* g, double dt,
                         int intRes, float* d_pos, float* d_vel, float* d_acc) {
  return fdtraj_impl<float>("mp_fd_trajectory_f32", ctx, model, d_theta0, d_dtheta0, d_taumat, d_Ftipmat, B, N, g, dt, intRes,
                            d_pos, d_vel, d_acc);
}
int mp_fd_trajectory_f64(mp_ctx* ctx, const mp_model* model, const double* d_theta0, const double* d_dtheta0,
                         const double* d_taumat, const double* d_Ftipmat, int64_t B, int64_t N, const double* g, double dt,
                         int intRes, float* d_pos, float* d_vel, float* d_acc) {
  return fdtraj_impl<double>("mp_fd_trajectory_f64", ctx, model, d_theta0, d_dtheta0, d_taumat, d_Ftipmat, B, N, g, dt, intRes,
                             d_pos, d_vel, d_acc);
}
int mp_fd_trajectory_tm_f32(mp_ctx* ctx, const mp_model* model, const float* d_theta0, const float* d_dtheta0,
                            const float* d_taumat, const float* d_Ftipmat, int64_t B, int64_t N, const double* g, double dt,
                            int intRes, float* d_pos, float* d_vel, float* d_acc) {
  return fdtraj_impl<float>("mp_fd_trajectory_tm_f32", ctx, model, d_theta0, d_dtheta0, d_taumat, d_Ftipmat, B, N, g, dt, intRes,
                            d_pos, d_vel, d_acc, true);
}
int mp_fd_trajectory_tm_f64(mp_ctx* ctx, const mp_model* model, const double* d_theta0, const double* d_dtheta0,
                            const double* d_taumat, const double* d_Ftipmat, int64_t B, int64_t N, const double* g, double dt,
                            int intRes, float* d_pos, float* d_vel, float* d_acc) {
  return fdtraj_impl<double>("mp_fd_trajectory_tm_f64", ctx, model, d_theta0, d_dtheta0, d_taumat, d_Ftipmat, B, N, g, dt, intRes,
                             d_pos, d_vel, d_acc, true);
}
int mp_transpose_rows(mp_ctx* ctx, const void* d_src, int64_t outer, int64_t inner, int64_t row_bytes, void* d_dst) {
  REQUIRE(ctx, "mp_transpose_rows: null context");
  CTX_ENTER(ctx);
  REQUIRE(outer >= 0 && inner >= 0, "mp_transpose_rows: negative extent");
  REQUIRE(row_bytes > 0 && row_bytes % 4 == 0 && row_bytes <= MP_BIG_DOF * 8, "mp_transpose_rows: row_bytes %lld must be a multiple of 4 in 4..%d",
          (long long)row_bytes, MP_BIG_DOF * 8);
  if (outer == 0 || inner == 0) return MP_OK;
  REQUIRE(d_src && d_dst && d_src != d_dst, "mp_transpose_rows: null or aliased device pointer");
  PROFILE_SCOPE(ctx, "mp_transpose_rows");
  const int W = (int)(row_bytes / 4);
  HIP_TRY(mpk_transpose_rows(ctx->compute, d_src, d_dst, (long)outer, (long)inner, W));
  return MP_OK;
}
int mp_fd_trajectory_host_f32(mp_ctx* ctx, const mp_model* model, const float* theta0, const float* dtheta0,
                              const float* taumat, const float* Ftipmat, int64_t B, int64_t N, const double* g, double dt,
                              int intRes, float* pos, float* vel, float* acc) {
  return fdtraj_host_impl<float>("mp_fd_trajectory_host_f32", ctx, model, theta0, dtheta0, taumat, Ftipmat, B, N, g, dt, intRes,
                                 pos, vel, acc);
}
int mp_fd_trajectory_host_f64(mp_ctx* ctx, const mp_model* model, const double* theta0, const double* dtheta0,
                              const double* taumat, const double* Ftipmat, int64_t B, int64_t N, const double* g, double dt,
                              int intRes, float* pos, float* vel, float* acc) {
  return fdtraj_host_impl<double>("mp_fd_trajectory_host_f64", ctx, model, theta0, dtheta0, taumat, Ftipmat, B, N, g, dt,
                                  intRes, pos, vel, acc);
}
int mp_mass_matrix_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, int64_t rows, double* M) {
  CHECK_COMMON("mp_mass_matrix_host_f64");
  REQUIRE(rows >= 0, "mp_mass_matrix_host_f64: negative row count");
  if (rows == 0) return MP_OK;
  REQUIRE(q && M, "mp_mass_matrix_host_f64: null host pointer");
  const size_t n = (size_t)model->d.n, qb = (size_t)rows * n * sizeof(double), mb = qb * n;
  HostCall h(ctx);
  const double* dq = h.in(q, qb);
  double* dM = h.out(M, mb);
  return h.run([&] { return mp_mass_matrix_f64(ctx, model, dq, rows, dM); });
}
int mp_forward_dynamics_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd, const double* tau,
                                 int64_t rows, const double* g, const double* Ftip, double* qdd) {
  CHECK_COMMON("mp_forward_dynamics_host_f64");
  REQUIRE(rows >= 0, "mp_forward_dynamics_host_f64: negative row count");
  if (rows == 0) return MP_OK;
  REQUIRE(q && qd && tau && qdd, "mp_forward_dynamics_host_f64: null host pointer");
  const size_t bytes = (size_t)rows * (size_t)model->d.n * sizeof(double);
  HostCall h(ctx);
  const double *dq = h.in(q, bytes), *dqd = h.in(qd, bytes), *dt = h.in(tau, bytes);
  double* dout = h.out(qdd, bytes);
  return h.run([&] { return mp_forward_dynamics_f64(ctx, model, dq, dqd, dt, rows, g, Ftip, dout); });
}

static int deriv_host_impl(const char* fn, bool fd, mp_ctx* ctx, const mp_model* model, const double* q, const double* qd,
                           const double* x, int64_t rows, const double* g, const double* Ftip, double* y, double* dq, double* dqd,
                           double* mat) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  if (rows == 0) return MP_OK;
  REQUIRE(q && qd && x && dq && dqd, "%s: null host pointer", fn);
  const size_t vb = (size_t)rows * (size_t)model->d.n * sizeof(double), mb = vb * (size_t)model->d.n;
  HostCall h(ctx);
  const double *dq_in = h.in(q, vb), *dqd_in = h.in(qd, vb), *dx = h.in(x, vb);
  double *dy = h.out(y, vb), *ddq = h.out(dq, mb), *ddqd = h.out(dqd, mb), *dmat = h.out(mat, mb);
  return h.run([&] { return deriv_impl(fn, fd, ctx, model, dq_in, dqd_in, dx, rows, g, Ftip, dy, ddq, ddqd, dmat); });
}
int mp_id_derivatives_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd, const double* qdd,
                               int64_t rows, const double* g, const double* Ftip, double* tau, double* dtau_dq, double* dtau_dqd,
                               double* M) {
  return deriv_host_impl("mp_id_derivatives_host_f64", false, ctx, model, q, qd, qdd, rows, g, Ftip, tau, dtau_dq, dtau_dqd, M);
}
int mp_fd_derivatives_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd, const double* tau,
                               int64_t rows, const double* g, const double* Ftip, double* qdd, double* dqdd_dq, double* dqdd_dqd,
                               double* Minv) {
  return deriv_host_impl("mp_fd_derivatives_host_f64", true, ctx, model, q, qd, tau, rows, g, Ftip, qdd, dqdd_dq, dqdd_dqd, Minv);
}

static int vjp_host_impl(const char* fn, bool fd, mp_ctx* ctx, const mp_model* model, const double* q, const double* qd, const double* x,
                         const double* cot, int64_t rows, const double* g, const double* Ftip, double* y, double* o1, double* o2,
                         double* o3) {
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  if (rows == 0) return MP_OK;
  REQUIRE(q && qd && x && cot && o1 && o2, "%s: null host pointer", fn);
  const size_t vb = (size_t)rows * (size_t)model->d.n * sizeof(double);
  HostCall h(ctx);
  const double *dq = h.in(q, vb), *dqd = h.in(qd, vb), *dx = h.in(x, vb), *dc = h.in(cot, vb);
  double *dy = h.out(y, vb), *d1 = h.out(o1, vb), *d2 = h.out(o2, vb), *d3 = h.out(o3, vb);
  return h.run([&] { return vjp_impl(fn, fd, ctx, model, dq, dqd, dx, dc, rows, g, Ftip, dy, d1, d2, d3); });
}
int mp_id_vjp_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd, const double* qdd, const double* gtau,
                       int64_t rows, const double* g, const double* Ftip, double* gq, double* gqd, double* gqdd) {
  return vjp_host_impl("mp_id_vjp_host_f64", false, ctx, model, q, qd, qdd, gtau, rows, g, Ftip, nullptr, gq, gqd, gqdd);
}
int mp_fd_vjp_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd, const double* tau, const double* gqdd,
                       int64_t rows, const double* g, const double* Ftip, double* qdd, double* gq, double* gqd, double* gtau) {
  return vjp_host_impl("mp_fd_vjp_host_f64", true, ctx, model, q, qd, tau, gqdd, rows, g, Ftip, qdd, gq, gqd, gtau);
}

int mp_fk_jac_vjp_host_f64(mp_ctx* ctx, const mp_model* model, int frame, const double* q, const double* gT, const double* gJ,
                           int64_t rows, double* T, double* J, double* gq) {
  const char* fn = "mp_fk_jac_vjp_host_f64";
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  if (int rc = mp_kin_vjp_check(fn, frame, rows)) return rc;
  if (rows == 0) return MP_OK;
  REQUIRE(q, "%s: null host pointer", fn);
  REQUIRE(T || J || gq, "%s: at least one output is required", fn);
  const size_t vb = (size_t)rows * (size_t)model->d.n * sizeof(double), tb = (size_t)rows * 16 * sizeof(double);
  HostCall h(ctx);
  const double *dq = h.in(q, vb), *dgT = h.in(gq ? gT : nullptr, tb), *dgJ = h.in(gq ? gJ : nullptr, 6 * vb);  // cotangents: for gq only
  double *dT = h.out(T, tb), *dJ = h.out(J, 6 * vb), *dgq = h.out(gq, vb);
  return h.run([&] { return kin_vjp_impl(fn, ctx, model, frame, dq, dgT, dgJ, rows, dT, dJ, dgq); });
}

int mp_opspace_host_f64(mp_ctx* ctx, const mp_model* model, int frame, int task, double damping, const double* q, const double* qd,
                        int64_t rows, const double* g, double* T, double* J, double* Jdqd, double* Lambda, double* Jbar, double* mu,
                        double* p) {
  const char* fn = "mp_opspace_host_f64";
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  if (int rc = mp_opspace_check(fn, frame, task, damping, rows)) return rc;
  if (rows == 0) return MP_OK;
  REQUIRE(q && qd, "%s: null host pointer", fn);
  REQUIRE(T || J || Jdqd || Lambda || Jbar || mu || p, "%s: at least one output is required", fn);
  const size_t n = (size_t)model->d.n, m = task == 0 ? 6 : 3, rb = (size_t)rows * sizeof(double);
  HostCall h(ctx);
  const double *dq = h.in(q, n * rb), *dqd = h.in(qd, n * rb);
  double *dT = h.out(T, 16 * rb), *dJ = h.out(J, m * n * rb), *dJdqd = h.out(Jdqd, m * rb), *dLambda = h.out(Lambda, m * m * rb);
  double *dJbar = h.out(Jbar, n * m * rb), *dmu = h.out(mu, m * rb), *dp = h.out(p, m * rb);
  return h.run([&] { return opspace_impl(fn, ctx, model, frame, task, damping, dq, dqd, rows, g, dT, dJ, dJdqd, dLambda, dJbar, dmu, dp); });
}

int mp_opspace_torque_host_f64(mp_ctx* ctx, const mp_model* model, int frame, int task, double damping, const double* q, const double* qd,
                               const double* acc, const double* tau0, int64_t rows, const double* g, double* tau) {
  const char* fn = "mp_opspace_torque_host_f64";
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  if (int rc = mp_opspace_check(fn, frame, task, damping, rows)) return rc;
  if (rows == 0) return MP_OK;
  REQUIRE(q && qd && acc && tau, "%s: null host pointer", fn);
  const size_t vb = (size_t)rows * (size_t)model->d.n * sizeof(double), ab = (size_t)rows * (task == 0 ? 6 : 3) * sizeof(double);
  HostCall h(ctx);
  const double *dq = h.in(q, vb), *dqd = h.in(qd, vb), *dacc = h.in(acc, ab), *dt0 = h.in(tau0, vb);
  double* dtau = h.out(tau, vb);
  return h.run([&] { return opspace_torque_impl(fn, ctx, model, frame, task, damping, dq, dqd, dacc, dt0, rows, g, dtau); });
}

int mp_id_regressor_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd, const double* qdd, int64_t rows,
                             const double* g, const double* Ftip, double* Y, double* tau_ext) {
  const char* fn = "mp_id_regressor_host_f64";
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  if (int rc = mp_regressor_check(fn, rows)) return rc;
  if (rows == 0) return MP_OK;
  REQUIRE(q && qd && qdd && Y, "%s: null host pointer", fn);
  const size_t n = (size_t)model->d.n, vb = (size_t)rows * n * sizeof(double), yb = vb * n * MP_REG_P;
  HostCall h(ctx);
  const double *dq = h.in(q, vb), *dqd = h.in(qd, vb), *dqdd = h.in(qdd, vb);
  double *dY = h.out(Y, yb), *dte = h.out(tau_ext, vb);
  return h.run([&] { return regressor_impl(fn, ctx, model, dq, dqd, dqdd, rows, g, Ftip, dY, dte); });
}
int mp_id_regressor_normal_host_f64(mp_ctx* ctx, const mp_model* model, const double* q, const double* qd, const double* qdd,
                                    const double* rhs, int64_t rows, const double* g, const double* Ftip, double* A, double* b,
                                    double* rr) {
  const char* fn = "mp_id_regressor_normal_host_f64";
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  if (int rc = mp_regressor_check(fn, rows)) return rc;
  REQUIRE(b && rr && (rows == 0 || (q && qd && qdd && rhs)), "%s: null host pointer", fn);
  const size_t n = (size_t)model->d.n, vb = (size_t)rows * n * sizeof(double), w = n * MP_REG_P;
  HostCall h(ctx);
  const double *dq = nullptr, *dqd = nullptr, *dqdd = nullptr, *drhs = nullptr;
  void* dwork = nullptr;
  if (rows > 0) {  // (no rows: the launch only zeroes A, b and rr, which are downloaded all the same)
    dq = h.in(q, vb), dqd = h.in(qd, vb), dqdd = h.in(qdd, vb), drhs = h.in(rhs, vb);
    dwork = h.work((size_t)regressor_normal_work_bytes((int)n, rows));
  }
  double *dA = h.out(A, w * w * sizeof(double)), *db = h.out(b, w * sizeof(double)), *drr = h.out(rr, sizeof(double));
  return h.run([&] { return regressor_normal_impl(fn, ctx, model, dq, dqd, dqdd, drhs, rows, g, Ftip, dwork, dA, db, drr); });
}

int mp_pd_regulation_host_f64(mp_ctx* ctx, const mp_model* model, const double* theta0, const double* theta_des, const double* Kp,
                              const double* Kd, int64_t K, const double* g, double dt, int steps, double* errors, int32_t* count) {
  CHECK_COMMON("mp_pd_regulation_host_f64");
  REQUIRE(K >= 0 && steps >= 0, "mp_pd_regulation_host_f64: negative run or step count");
  if (K == 0) return MP_OK;
  REQUIRE(theta0 && theta_des && Kp && Kd && count && (errors || steps == 0), "mp_pd_regulation_host_f64: null host pointer");
  REQUIRE(std::isfinite(dt), "mp_pd_regulation_host_f64: dt must be finite");
  const size_t qb = (size_t)K * (size_t)model->d.n * sizeof(double), kb = (size_t)K * sizeof(double),
               eb = (size_t)K * (size_t)steps * sizeof(double), cb = (size_t)K * sizeof(int32_t);
  HostCall h(ctx);
  const double *d0 = h.in(theta0, qb), *dd = h.in(theta_des, qb), *dkp = h.in(Kp, kb), *dkd = h.in(Kd, kb);
  double* de = eb ? h.inout(errors, eb) : h.work<double>(0);  // in-out: entries past a run's count keep the caller's values
  int32_t* dc = h.out(count, cb);
  MpCall<double> c;
  make_call<double>(model, g, nullptr, &c);
  return h.run([&]() -> int {
    PROFILE_SCOPE(ctx, "mp_pd_regulation_host_f64");
    if (model->big) {
      const MpBigModel<double>* dm = nullptr;
      if (int rc = device_big_model<double>(ctx, model, &dm)) return rc;
      HIP_TRY(mpk_dyn_pd_regulation(ctx->compute, model->d.n, dm, c, d0, dd, dkp, dkd, (long)K, dt, steps, de, (int*)dc));
    } else {
      HIP_TRY(mpk_pd_regulation(ctx->compute, model->d, c, d0, dd, dkp, dkd, (long)K, dt, steps, de, (int*)dc));
    }
    return MP_OK;
  });
}

int mp_cartesian_trajectory_f32(mp_ctx* ctx, const double* d_Xstart, const double* d_Xend, int64_t B, int64_t N, double Tf,
                                int method, float* d_pos, float* d_vel, float* d_acc, float* d_orient) {
  REQUIRE(ctx, "mp_cartesian_trajectory_f32: null context");
  CTX_ENTER(ctx);
  REQUIRE(B >= 0 && N >= 0, "mp_cartesian_trajectory_f32: negative B or N");
  if (B == 0 || N == 0) return MP_OK;
  REQUIRE(N >= 2, "mp_cartesian_trajectory_f32: N = 1 divides by zero (Tf / (N - 1))");
  REQUIRE(d_Xstart && d_Xend && d_pos && d_vel && d_acc && d_orient, "mp_cartesian_trajectory_f32: null device pointer");
  REQUIRE(aligned16(d_Xstart) && aligned16(d_Xend), "mp_cartesian_trajectory_f32: pose pointers must be 16-byte aligned");
  HIP_TRY(mpk_cartesian_traj(ctx->compute, d_Xstart, d_Xend, (long)B, (long)N, Tf, method, d_pos, d_vel, d_acc, d_orient));
  return MP_OK;
}
int mp_cartesian_trajectory_host_f32(mp_ctx* ctx, const double* Xstart, const double* Xend, int64_t B, int64_t N, double Tf,
                                     int method, float* pos, float* vel, float* acc, float* orient) {
  REQUIRE(ctx, "mp_cartesian_trajectory_host_f32: null context");
  CTX_ENTER(ctx);
  REQUIRE(B >= 0 && N >= 0, "mp_cartesian_trajectory_host_f32: negative B or N");
  if (B == 0 || N == 0) return MP_OK;
  REQUIRE(Xstart && Xend && pos && vel && acc && orient, "mp_cartesian_trajectory_host_f32: null host pointer");
  const size_t xb = (size_t)B * 16 * sizeof(double), pb = (size_t)B * (size_t)N * 3 * sizeof(float);
  HostCall h(ctx);
  const double *ds = h.in(Xstart, xb), *de = h.in(Xend, xb);
  float *dp = h.out(pos, pb), *dv = h.out(vel, pb), *da = h.out(acc, pb), *dor = h.out(orient, pb * 3);
  return h.run([&] { return mp_cartesian_trajectory_f32(ctx, ds, de, B, N, Tf, method, dp, dv, da, dor); });
}

int mp_potential_field_f32(mp_ctx* ctx, const float* d_positions, const float* goal, const float* d_obstacles, int64_t P,
                           int64_t O, float influence_distance, float* d_potential, float* d_gradient) {
  REQUIRE(ctx, "mp_potential_field_f32: null context");
  CTX_ENTER(ctx);
  REQUIRE(P >= 0 && O >= 0, "mp_potential_field_f32: negative P or O");
  if (P == 0) return MP_OK;
  REQUIRE(d_positions && goal && d_potential && d_gradient && (O == 0 || d_obstacles), "mp_potential_field_f32: null pointer");
  HIP_TRY(mpk_potential_field(ctx->compute, d_positions, goal, d_obstacles, (long)P, (long)O, influence_distance, d_potential, d_gradient));
  return MP_OK;
}
int mp_potential_field_host_f32(mp_ctx* ctx, const float* positions, const float* goal, const float* obstacles, int64_t P,
                                int64_t O, float influence_distance, float* potential, float* gradient) {
  REQUIRE(ctx, "mp_potential_field_host_f32: null context");
  CTX_ENTER(ctx);
  REQUIRE(P >= 0 && O >= 0, "mp_potential_field_host_f32: negative P or O");
  if (P == 0) return MP_OK;
  REQUIRE(positions && goal && potential && gradient && (O == 0 || obstacles), "mp_potential_field_host_f32: null pointer");
  const size_t pb = (size_t)P * 3 * sizeof(float), ob = (size_t)O * 3 * sizeof(float);
  HostCall h(ctx);
  const float *dp = h.in(positions, pb), *dob = h.in(O ? obstacles : nullptr, ob);
  float *du = h.out(potential, (size_t)P * sizeof(float)), *dg = h.out(gradient, pb);
  return h.run([&] { return mp_potential_field_f32(ctx, dp, goal, dob, P, O, influence_distance, du, dg); });
}

}  // extern "C"
// the settings of the IK entries, packed by mp_ik_pack (mp_handles.h); these entries' words say which joint's limits are crossed
template <int CAP>
static int ik_params(const char* fn, const mp_model* model, const double* joint_limits, double eomg, double ev, int max_iterations,
                     double damping, double step_cap, double w_o, double w_p, int adaptive, int backtracking, uint32_t seed,
                     MpIkParamsT<CAP>* P) {
  REQUIRE(max_iterations >= 1, "%s: max_iterations must be at least 1 (got %d)", fn, max_iterations);
  const int rc = mp_ik_pack(fn, model->d.n, joint_limits, eomg, ev, max_iterations, damping, step_cap, w_o, w_p, adaptive, backtracking, seed, P);
  REQUIRE(rc >= 0, "%s: joint %d has lower limit above upper limit", fn, -rc - 1);
  return rc;
}
extern "C" {

int mp_inverse_kinematics_f64(mp_ctx* ctx, const mp_model* model, const double* d_T_desired, const double* d_theta0, int64_t B,
                              const double* joint_limits, double eomg, double ev, int max_iterations, double damping,
                              double step_cap, double weight_orientation, double weight_position, int adaptive_tuning, int backtracking,
                              uint32_t seed,
                              double* d_theta, int32_t* d_success, int32_t* d_iterations, int32_t* d_restarts) {
  CHECK_COMMON("mp_inverse_kinematics_f64");
  REQUIRE(B >= 0, "mp_inverse_kinematics_f64: negative problem count");
  if (B == 0) return MP_OK;
  REQUIRE(d_T_desired && d_theta0 && d_theta && d_success && d_iterations && d_restarts, "mp_inverse_kinematics_f64: null device pointer");
  REQUIRE(aligned16(d_T_desired) && aligned16(d_theta0) && aligned16(d_theta), "mp_inverse_kinematics_f64: device pointers must be 16-byte aligned");
  if (!ctx->queue_counter) {
    REQUIRE(!ctx->capturing, "mp_inverse_kinematics_f64: first use allocates; call it once before capturing a launch graph");
    HIP_TRY(hipMalloc(&ctx->queue_counter, 256));
  }
  if (model->big) {  // 9..32 joints: the same iteration on the run-time-n kinematics (csrc/mp_dyn.h)
    MpIkBigParams PB;
    if (int rc = ik_params("mp_inverse_kinematics_f64", model, joint_limits, eomg, ev, max_iterations, damping,
                                                      step_cap, weight_orientation, weight_position, adaptive_tuning, backtracking, seed, &PB))
      return rc;
    const MpBigModel<double>* dm = nullptr;
    if (int rc = device_big_model<double>(ctx, model, &dm)) return rc;
    HIP_TRY(mpk_dyn_ik(ctx->compute, model->d.n, dm, PB, d_T_desired, d_theta0, (long)B, d_theta, d_success, d_iterations, d_restarts,
                       (unsigned long long*)ctx->queue_counter, ctx->compute_units));
    return MP_OK;
  }
  MpIkParams P;
  if (int rc = ik_params("mp_inverse_kinematics_f64", model, joint_limits, eomg, ev, max_iterations, damping, step_cap,
                                                 weight_orientation, weight_position, adaptive_tuning, backtracking, seed, &P))
    return rc;
  if (const MpSpec* sp = find_spec(ctx, model)) {  // this robot's constants baked in (mp_model_specialize)
    for (int j = 0; j < MP_MAX_DOF; ++j) {  // the specialised build assumes finite arithmetic: open limits become huge ones
      if (!(P.lo[j] > -1e300)) P.lo[j] = -1e300;
      if (!(P.hi[j] < 1e300)) P.hi[j] = 1e300;
    }
    HIP_TRY(hipMemsetAsync(ctx->queue_counter, 0, sizeof(unsigned long long), ctx->compute));
    long nb = (long)B;
    void* counter = ctx->queue_counter;
    void* args[] = {&P, &d_T_desired, &d_theta0, &nb, &d_theta, &d_success, &d_iterations, &d_restarts, &counter};
    const long want = (nb + 255) / 256, cap = 1L * (ctx->compute_units > 0 ? ctx->compute_units : 256);  // one block per CU: see mp_spec_ik
    return launch_spec(ctx, sp->ik, (want < cap ? want : cap) * 256, args);
  }
  HIP_TRY(mpk_ik(ctx->compute, model->d, P, d_T_desired, d_theta0, (long)B, d_theta, d_success, d_iterations, d_restarts,
                 (unsigned long long*)ctx->queue_counter, ctx->compute_units));
  return MP_OK;
}

int mp_inverse_kinematics_host_f64(mp_ctx* ctx, const mp_model* model, const double* T_desired, const double* theta0, int64_t B,
                                   const double* joint_limits, double eomg, double ev, int max_iterations, double damping,
                                   double step_cap, double weight_orientation, double weight_position, int adaptive_tuning, int backtracking,
                              uint32_t seed,
                                   double* theta, int32_t* success, int32_t* iterations, int32_t* restarts) {
  CHECK_COMMON("mp_inverse_kinematics_host_f64");
  REQUIRE(B >= 0, "mp_inverse_kinematics_host_f64: negative problem count");
  if (B == 0) return MP_OK;
  REQUIRE(T_desired && theta0 && theta && success && iterations && restarts, "mp_inverse_kinematics_host_f64: null host pointer");
  const size_t tb = (size_t)B * 16 * sizeof(double), qb = (size_t)B * (size_t)model->d.n * sizeof(double), ib = (size_t)B * sizeof(int32_t);
  HostCall h(ctx);
  const double *dT = h.in(T_desired, tb), *d0 = h.in(theta0, qb);
  double* dq = h.out(theta, qb);
  int32_t *dok = h.out(success, ib), *dit = h.out(iterations, ib), *drs = h.out(restarts, ib);
  return h.run([&] {
    return mp_inverse_kinematics_f64(ctx, model, dT, d0, B, joint_limits, eomg, ev, max_iterations, damping, step_cap, weight_orientation,
                                     weight_position, adaptive_tuning, backtracking, seed, dq, dok, dit, drs);
  });
}

}  // extern "C"


// exposed to mp_comm.cpp
// (whoever asks for the stream is about to enqueue something that may read torques: parked float64 passes run first)
hipStream_t mp_ctx_compute_stream(mp_ctx* ctx) { return ctx->compute; }
// ... after this: the communicator is about to enqueue something that reads torques, so the parked float64 passes run first - and
// a pass that cannot be launched fails the collective instead of letting it send float32-only rows
int mp_ctx_flush_parked(mp_ctx* ctx) {
  CTX_ENTER(ctx);
  return MP_OK;
}
int mp_ctx_device(mp_ctx* ctx) { return ctx->device; }
// ---- sphere-model collision (mp_collision.h).  The handle's tables live in device memory of their own (not the pool: a handle
// outlives contexts), one copy per context that has used it; mp_collision_destroy (mp_cpu.cpp) releases them through `release`.
static void collision_release(mp_collision* h) {
  if (h->resident.empty()) return;
  int prev = -1;
  (void)hipGetDevice(&prev);
  for (auto& kv : h->resident) {
    mp_collision::Resident& R = kv.second;
    (void)hipSetDevice(R.device);
    if (R.sph) (void)hipFree(R.sph);
    if (R.world) (void)hipFree(R.world);
    if (R.cloud) (void)hipFree(R.cloud);
    if (R.counter) (void)hipFree(R.counter);
    for (void* p : R.retired) (void)hipFree(p);
  }
  h->resident.clear();
  if (prev >= 0) (void)hipSetDevice(prev);
}
// header + obstacles to the context's table, growing it in steps of 64 obstacles; the header keeps the address of the context's
// cloud; returns when the copy is done
static int collision_upload_world(mp_ctx* ctx, mp_collision::Resident& R, const std::vector<MpColObstacle>& w) {
  const int O = (int)w.size();
  if (!R.world || O > R.cap) {
    const int cap = O <= 64 ? 64 : ((O + 63) / 64) * 64;
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, sizeof(MpColWorld) + (size_t)cap * sizeof(MpColObstacle)));
    if (R.world) R.retired.push_back(R.world);
    R.world = p;
    R.cap = cap;
  }
  std::vector<char> img(sizeof(MpColWorld) + (size_t)O * sizeof(MpColObstacle));
  const MpColWorld hdr = {O, 0, static_cast<const MpColCloud*>(R.cloud)};
  std::memcpy(img.data(), &hdr, sizeof hdr);
  if (O) std::memcpy(img.data() + sizeof hdr, w.data(), (size_t)O * sizeof(MpColObstacle));
  H2D(R.world, img.data(), img.size());
  HIP_TRY(hipStreamSynchronize(ctx->compute));
  return MP_OK;
}
// The cloud's image to a device buffer of its own (the old one is retired: a captured graph's kernels may still be reading it), then
// the world table's header with its address - the kernels find the cloud through the header, so a replayed graph sees the new one.
// An empty image removes the cloud.  Both copies go behind the launches already on the compute stream; returns when they are done.
static int collision_upload_cloud(mp_ctx* ctx, mp_collision::Resident& R, const std::vector<MpCloudPoint>& img) {
  void* p = nullptr;
  if (!img.empty()) {
    HIP_TRY(hipMalloc(&p, img.size() * sizeof(MpCloudPoint)));
    if (hipMemcpyAsync(p, img.data(), img.size() * sizeof(MpCloudPoint), hipMemcpyHostToDevice, ctx->compute) != hipSuccess ||
        hipStreamSynchronize(ctx->compute) != hipSuccess) {
      (void)hipFree(p);
      return mp_fail(MP_ERR_HIP, "mp_collision_set_cloud: the copy of the cloud failed");
    }
  }
  if (R.cloud) R.retired.push_back(R.cloud);
  R.cloud = p;
  if (!R.world) return MP_OK;  // (the first upload of the world follows and writes the header)
  const MpColCloud* at = static_cast<const MpColCloud*>(p);
  H2D(static_cast<char*>(R.world) + offsetof(MpColWorld, cloud), &at, sizeof at);
  HIP_TRY(hipStreamSynchronize(ctx->compute));
  return MP_OK;
}
// whether a launch of `h` on this context takes the kernels' cloud instances
// (the caller holds h->mu, as every *_impl does: mp_collision_set_cloud changes both under it)
static bool collision_has_cloud(mp_ctx* ctx, mp_collision* h) {
  auto it = h->resident.find(ctx->uid);
  return it != h->resident.end() ? it->second.cloud != nullptr : !h->cloud.empty();
}
static int collision_resident(const char* fn, mp_ctx* ctx, mp_collision* h, mp_collision::Resident** out) {
  auto it = h->resident.find(ctx->uid);
  if (it != h->resident.end()) { *out = &it->second; return MP_OK; }
  REQUIRE(!ctx->capturing, "%s: the collision handle is not on this context's device yet: call mp_collision_set_world or launch once before the capture", fn);
  mp_collision::Resident R;
  R.device = ctx->device;
  const size_t pb = h->pairs.size() * sizeof(MpColPair);
  HIP_TRY(hipMalloc(&R.sph, sizeof(MpColSpheres) + (pb ? pb : sizeof(MpColPair))));
  if (hipMalloc(&R.counter, 256) != hipSuccess) {
    (void)hipFree(R.sph);
    return mp_fail(MP_ERR_HIP, "%s: out of device memory", fn);
  }
  h->release = collision_release;
  mp_collision::Resident& K = h->resident[ctx->uid] = R;
  H2D(K.sph, &h->sph, sizeof(MpColSpheres));
  if (pb) H2D(static_cast<char*>(K.sph) + sizeof(MpColSpheres), h->pairs.data(), pb);
  if (int rc = collision_upload_cloud(ctx, K, h->cloud)) return rc;
  if (int rc = collision_upload_world(ctx, K, h->world)) return rc;
  *out = &K;
  return MP_OK;
}
// what every sphere-model entry checks first (`fn`: the entry's name, a const char*)
#define CHECK_SPHERE_ENTRY(fn)                                                                                          \
  REQUIRE(ctx && model && h, "%s: null context, model or collision handle", fn);                                        \
  CTX_ENTER(ctx);                                                                                                       \
  REQUIRE_SMALL(fn);                                                                                                    \
  REQUIRE(h->n == model->d.n, "%s: the collision handle was made for a model of %d joints, this one has %d", fn, h->n, model->d.n)

// ... for an entry that holds no lock yet (the host forms size their workspace before they enter the impl)
static bool collision_has_cloud_locked(mp_ctx* ctx, mp_collision* h) {
  std::lock_guard<std::mutex> hl(h->mu);
  return collision_has_cloud(ctx, h);
}
static MpColDevice collision_device(const mp_collision* h, const mp_collision::Resident* R) {
  return {h->sph.S, static_cast<const MpColSpheres*>(R->sph),
          reinterpret_cast<const MpColPair*>(static_cast<const char*>(R->sph) + sizeof(MpColSpheres)),
          static_cast<const MpColWorld*>(R->world), static_cast<unsigned long long*>(R->counter), R->cloud != nullptr};
}
// The grid of a work-queue launch (mpk_queue_plan): the resident blocks, ceil(B / 64), max_blocks if that is positive and the blocks
// the workspace holds, whichever is smallest.
static long queue_grid(const MpQueuePlan& plan, int64_t B, int max_blocks, size_t ws_blocks = SIZE_MAX) {
  long grid = std::min<long>(plan.resident, (long)((B + 63) / 64));
  if (max_blocks > 0) grid = std::min<long>(grid, max_blocks);
  return (long)std::min<size_t>((size_t)grid, ws_blocks);
}
// The planners' host entries take their workspace from the pool: as many blocks as the launch can use, at most 1 GiB of them (never
// less than one block).
static size_t host_workspace_bytes(const MpQueuePlan& plan, int64_t B, size_t block_bytes) {
  const long blocks = std::min<long>(queue_grid(plan, B, 0), (long)(((size_t)1 << 30) / block_bytes));
  return (size_t)std::max<long>(1, blocks) * block_bytes;
}

static int collision_impl(const char* fn, mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_q, int64_t rows,
                          double eps_world, double eps_self, const MpColOut& O) {
  CHECK_SPHERE_ENTRY(fn);
  REQUIRE(eps_world > 0.0 && eps_self > 0.0 && std::isfinite(eps_world) && std::isfinite(eps_self),
          "%s: eps_world and eps_self must be positive and finite", fn);
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  if (rows == 0) return MP_OK;
  REQUIRE(d_q, "%s: null device pointer", fn);
  REQUIRE(mp_out_any(O), "%s: at least one output is required", fn);
  REQUIRE(aligned16(d_q) && mp_out_aligned16(O), "%s: device pointers must be 16-byte aligned", fn);
  std::lock_guard<std::mutex> hl(h->mu);
  mp_collision::Resident* R = nullptr;
  if (int rc = collision_resident(fn, ctx, h, &R)) return rc;
  PROFILE_SCOPE(ctx, fn);
  HIP_TRY(mpk_collision(ctx->compute, model->d, collision_device(h, R), d_q, (long)rows, eps_world, eps_self, O));
  return MP_OK;
}

static int collision_edges_impl(const char* fn, mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_qa,
                                const double* d_qb, int64_t edges, double margin, double tol, int max_steps, int max_blocks,
                                const MpColEdgeOut& O) {
  CHECK_SPHERE_ENTRY(fn);
  if (int rc = mp_collision_edges_check(fn, margin, tol, max_steps)) return rc;
  REQUIRE(max_blocks >= 0, "%s: negative max_blocks", fn);
  REQUIRE(edges >= 0, "%s: negative edge count", fn);
  if (edges == 0) return MP_OK;
  REQUIRE(d_qa && d_qb, "%s: null device pointer", fn);
  REQUIRE(mp_out_any(O), "%s: at least one output is required", fn);
  REQUIRE(aligned16(d_qa) && aligned16(d_qb) && mp_out_aligned16(O), "%s: device pointers must be 16-byte aligned", fn);
  std::lock_guard<std::mutex> hl(h->mu);
  mp_collision::Resident* R = nullptr;
  if (int rc = collision_resident(fn, ctx, h, &R)) return rc;
  PROFILE_SCOPE(ctx, fn);
  const MpColEdgeParams P = {margin, tol, max_steps, 0};
  MpQueuePlan plan;
  HIP_TRY(mpk_queue_plan(MP_QUEUE_EDGES, model->d.n, h->sph.S, collision_has_cloud(ctx, h), ctx->compute_units, &plan));
  HIP_TRY(mpk_collision_edges(ctx->compute, model->d, collision_device(h, R), d_qa, d_qb, (long)edges, P, O,
                              queue_grid(plan, edges, max_blocks), plan.lds));
  return MP_OK;
}

extern "C" {

int mp_collision_edges_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_q_from, const double* d_q_to, int64_t edges,
                           double margin, double tol, int max_steps, int max_blocks, int32_t* d_status, double* d_t, int32_t* d_steps,
                           double* d_clearance, int32_t* d_witness) {
  return collision_edges_impl("mp_collision_edges_f64", ctx, model, h, d_q_from, d_q_to, edges, margin, tol, max_steps, max_blocks,
                              {d_status, d_t, d_steps, d_clearance, d_witness});
}

int mp_collision_edges_host_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* q_from, const double* q_to, int64_t edges,
                                double margin, double tol, int max_steps, int32_t* status, double* t, int32_t* steps, double* clearance,
                                int32_t* witness) {
  const char* fn = "mp_collision_edges_host_f64";
  CHECK_SPHERE_ENTRY(fn);
  REQUIRE(edges >= 0, "%s: negative edge count", fn);
  if (edges == 0) return mp_collision_edges_check(fn, margin, tol, max_steps);
  REQUIRE(q_from && q_to, "%s: null host pointer", fn);
  const size_t n = (size_t)model->d.n, rb = (size_t)edges * sizeof(double), ib = (size_t)edges * sizeof(int32_t);
  HostCall hc(ctx);  // (h is the collision handle)
  const double *da = hc.in(q_from, n * rb), *db = hc.in(q_to, n * rb);
  const MpColEdgeOut O = {hc.out(status, ib), hc.out(t, rb), hc.out(steps, ib), hc.out(clearance, rb), hc.out(witness, 3 * ib)};
  return hc.run([&] { return collision_edges_impl(fn, ctx, model, h, da, db, edges, margin, tol, max_steps, 0, O); });
}

}  // extern "C"

// ---- batched RRT-Connect over the sphere model (mp_rrt.h).  `made`: the launch plan where the entry has made it already (the host
// entry sizes its workspace by it); every entry call makes one.
static int rrt_connect_impl(const char* fn, mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_qs, const double* d_qg,
                            int64_t B, const MpRrtParams& P, void* d_ws, size_t ws_bytes, int max_blocks, const MpQueuePlan* made,
                            const MpRrtOut& O) {
  REQUIRE(max_blocks >= 0, "%s: negative max_blocks", fn);
  REQUIRE(B >= 0, "%s: negative problem count", fn);
  if (B == 0) return MP_OK;
  REQUIRE(d_qs && d_qg, "%s: null device pointer", fn);
  REQUIRE(mp_out_any(O), "%s: at least one output is required", fn);
  REQUIRE(aligned16(d_qs) && aligned16(d_qg) && mp_out_aligned16(O) && aligned16(d_ws), "%s: device pointers must be 16-byte aligned", fn);
  const size_t block_bytes = (size_t)mp_rrt_connect_workspace_bytes(model->d.n, P.max_nodes, 1);
  REQUIRE(d_ws && ws_bytes >= block_bytes, "%s: the workspace holds %zu bytes, one block needs %zu (mp_rrt_connect_workspace_bytes)", fn,
          d_ws ? ws_bytes : (size_t)0, block_bytes);
  std::lock_guard<std::mutex> hl(h->mu);
  mp_collision::Resident* R = nullptr;
  if (int rc = collision_resident(fn, ctx, h, &R)) return rc;
  PROFILE_SCOPE(ctx, fn);
  MpQueuePlan plan;
  if (made) plan = *made;
  else HIP_TRY(mpk_queue_plan(MP_QUEUE_RRT, model->d.n, h->sph.S, collision_has_cloud(ctx, h), ctx->compute_units, &plan));
  HIP_TRY(mpk_rrt_connect(ctx->compute, model->d, collision_device(h, R), d_qs, d_qg, (long)B, P, O, static_cast<double*>(d_ws),
                          queue_grid(plan, B, max_blocks, ws_bytes / block_bytes), plan.lds));
  return MP_OK;
}

extern "C" {

int mp_rrt_connect_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_q_start, const double* d_q_goal, int64_t B,
                       const double* lo, const double* hi, uint32_t seed, double step, double min_advance, int max_iters, int max_nodes,
                       int max_waypoints, double margin, double tol, int max_steps, void* d_workspace, size_t workspace_bytes,
                       int max_blocks, int32_t* d_status, int32_t* d_count, double* d_waypoints, int32_t* d_iterations, int32_t* d_nodes,
                       int32_t* d_evaluations) {
  const char* fn = "mp_rrt_connect_f64";
  CHECK_SPHERE_ENTRY(fn);
  MpRrtParams P;
  if (int rc = mp_rrt_connect_check(fn, model->d.n, lo, hi, seed, step, min_advance, max_iters, max_nodes, max_waypoints, margin, tol,
                                    max_steps, &P))
    return rc;
  return rrt_connect_impl(fn, ctx, model, h, d_q_start, d_q_goal, B, P, d_workspace, workspace_bytes, max_blocks, nullptr,
                          {d_status, d_count, d_waypoints, d_iterations, d_nodes, d_evaluations});
}

int mp_rrt_connect_host_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* q_start, const double* q_goal, int64_t B,
                            const double* lo, const double* hi, uint32_t seed, double step, double min_advance, int max_iters,
                            int max_nodes, int max_waypoints, double margin, double tol, int max_steps, int32_t* status, int32_t* count,
                            double* waypoints, int32_t* iterations, int32_t* nodes, int32_t* evaluations) {
  const char* fn = "mp_rrt_connect_host_f64";
  CHECK_SPHERE_ENTRY(fn);
  MpRrtParams P;
  if (int rc = mp_rrt_connect_check(fn, model->d.n, lo, hi, seed, step, min_advance, max_iters, max_nodes, max_waypoints, margin, tol,
                                    max_steps, &P))
    return rc;
  REQUIRE(B >= 0, "%s: negative problem count", fn);
  if (B == 0) return MP_OK;
  REQUIRE(q_start && q_goal, "%s: null host pointer", fn);
  MpQueuePlan plan;
  HIP_TRY(mpk_queue_plan(MP_QUEUE_RRT, model->d.n, h->sph.S, collision_has_cloud_locked(ctx, h), ctx->compute_units, &plan));
  const size_t n = (size_t)model->d.n, qb = (size_t)B * n * sizeof(double), ib = (size_t)B * sizeof(int32_t);
  const size_t ws_bytes = host_workspace_bytes(plan, B, (size_t)mp_rrt_connect_workspace_bytes(model->d.n, max_nodes, 1));
  HostCall hc(ctx);  // (h is the collision handle)
  const double *ds = hc.in(q_start, qb), *dg = hc.in(q_goal, qb);
  const MpRrtOut O = {hc.out(status, ib), hc.out(count, ib), hc.out(waypoints, (size_t)B * (size_t)max_waypoints * n * sizeof(double)),
                      hc.out(iterations, ib), hc.out(nodes, 2 * ib), hc.out(evaluations, ib)};
  void* dws = hc.work(ws_bytes);
  return hc.run([&] { return rrt_connect_impl(fn, ctx, model, h, ds, dg, B, P, dws, ws_bytes, 0, &plan, O); });
}

}  // extern "C"

// ---- batched path shortcutting over the sphere model (mp_shortcut.h).  `made`: as in rrt_connect_impl.
static int path_shortcut_impl(const char* fn, mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_in,
                              const int32_t* d_count_in, int64_t B, const MpShortcutParams& P, void* d_ws, size_t ws_bytes,
                              int max_blocks, const MpQueuePlan* made, const MpShortcutOut& O) {
  REQUIRE(max_blocks >= 0, "%s: negative max_blocks", fn);
  REQUIRE(B >= 0, "%s: negative problem count", fn);
  if (B == 0) return MP_OK;
  REQUIRE(d_in && d_count_in, "%s: null device pointer", fn);
  REQUIRE(mp_out_any(O), "%s: at least one output is required", fn);
  REQUIRE(aligned16(d_in) && aligned16(d_count_in) && mp_out_aligned16(O) && aligned16(d_ws), "%s: device pointers must be 16-byte aligned",
          fn);
  const size_t block_bytes = (size_t)mp_path_shortcut_workspace_bytes(model->d.n, P.max_waypoints, 1);
  REQUIRE(d_ws && ws_bytes >= block_bytes, "%s: the workspace holds %zu bytes, one block needs %zu (mp_path_shortcut_workspace_bytes)", fn,
          d_ws ? ws_bytes : (size_t)0, block_bytes);
  std::lock_guard<std::mutex> hl(h->mu);
  mp_collision::Resident* R = nullptr;
  if (int rc = collision_resident(fn, ctx, h, &R)) return rc;
  PROFILE_SCOPE(ctx, fn);
  MpQueuePlan plan;
  if (made) plan = *made;
  else HIP_TRY(mpk_queue_plan(MP_QUEUE_SHORTCUT, model->d.n, h->sph.S, collision_has_cloud(ctx, h), ctx->compute_units, &plan));
  HIP_TRY(mpk_path_shortcut(ctx->compute, model->d, collision_device(h, R), d_in, d_count_in, (long)B, P, O, static_cast<double*>(d_ws),
                            queue_grid(plan, B, max_blocks, ws_bytes / block_bytes), plan.lds));
  return MP_OK;
}

extern "C" {

int mp_path_shortcut_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_waypoints_in, const int32_t* d_count_in,
                         int64_t B, int64_t W_in, uint32_t seed, int max_iters, double min_gain, int max_waypoints, double margin,
                         double tol, int max_steps, void* d_workspace, size_t workspace_bytes, int max_blocks, int32_t* d_status,
                         int32_t* d_count, double* d_waypoints, double* d_length_in, double* d_length_out, int32_t* d_iterations,
                         int32_t* d_accepted, int32_t* d_skipped_full, int32_t* d_evaluations) {
  const char* fn = "mp_path_shortcut_f64";
  CHECK_SPHERE_ENTRY(fn);
  MpShortcutParams P;
  if (int rc = mp_path_shortcut_check(fn, W_in, seed, max_iters, min_gain, max_waypoints, margin, tol, max_steps, &P)) return rc;
  return path_shortcut_impl(fn, ctx, model, h, d_waypoints_in, d_count_in, B, P, d_workspace, workspace_bytes, max_blocks, nullptr,
                            {d_status, d_count, d_waypoints, d_length_in, d_length_out, d_iterations, d_accepted, d_skipped_full,
                             d_evaluations});
}

int mp_path_shortcut_host_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* waypoints_in, const int32_t* count_in,
                              int64_t B, int64_t W_in, uint32_t seed, int max_iters, double min_gain, int max_waypoints, double margin,
                              double tol, int max_steps, int32_t* status, int32_t* count, double* waypoints, double* length_in,
                              double* length_out, int32_t* iterations, int32_t* accepted, int32_t* skipped_full, int32_t* evaluations) {
  const char* fn = "mp_path_shortcut_host_f64";
  CHECK_SPHERE_ENTRY(fn);
  MpShortcutParams P;
  if (int rc = mp_path_shortcut_check(fn, W_in, seed, max_iters, min_gain, max_waypoints, margin, tol, max_steps, &P)) return rc;
  REQUIRE(B >= 0, "%s: negative problem count", fn);
  if (B == 0) return MP_OK;
  REQUIRE(waypoints_in && count_in, "%s: null host pointer", fn);
  MpQueuePlan plan;
  HIP_TRY(mpk_queue_plan(MP_QUEUE_SHORTCUT, model->d.n, h->sph.S, collision_has_cloud_locked(ctx, h), ctx->compute_units, &plan));
  const size_t n = (size_t)model->d.n, ib = (size_t)B * sizeof(int32_t), db = (size_t)B * sizeof(double);
  const size_t ws_bytes = host_workspace_bytes(plan, B, (size_t)mp_path_shortcut_workspace_bytes(model->d.n, max_waypoints, 1));
  HostCall hc(ctx);  // (h is the collision handle)
  const double* din = hc.in(waypoints_in, (size_t)B * (size_t)W_in * n * sizeof(double));
  const int32_t* dcin = hc.in(count_in, ib);
  const MpShortcutOut O = {hc.out(status, ib), hc.out(count, ib),
                           hc.out(waypoints, (size_t)B * (size_t)max_waypoints * n * sizeof(double)), hc.out(length_in, db),
                           hc.out(length_out, db), hc.out(iterations, ib), hc.out(accepted, ib), hc.out(skipped_full, ib),
                           hc.out(evaluations, ib)};
  void* dws = hc.work(ws_bytes);
  return hc.run([&] { return path_shortcut_impl(fn, ctx, model, h, din, dcin, B, P, dws, ws_bytes, 0, &plan, O); });
}

}  // extern "C"

// ---- goal configurations for pose goals over the sphere model (mp_goal.h): no workspace, so one plan per call, made here
static int goal_ik_impl(const char* fn, mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_Tg, const double* d_q0,
                        int64_t B, const MpGoalParams& P, int max_blocks, const MpGoalOut& O) {
  REQUIRE(max_blocks >= 0, "%s: negative max_blocks", fn);
  REQUIRE(B >= 0, "%s: negative problem count", fn);
  if (B == 0) return MP_OK;
  REQUIRE(d_Tg && d_q0, "%s: null device pointer", fn);
  REQUIRE(mp_out_any(O), "%s: at least one output is required", fn);
  REQUIRE(aligned16(d_Tg) && aligned16(d_q0) && mp_out_aligned16(O), "%s: device pointers must be 16-byte aligned", fn);
  std::lock_guard<std::mutex> hl(h->mu);
  mp_collision::Resident* R = nullptr;
  if (int rc = collision_resident(fn, ctx, h, &R)) return rc;
  PROFILE_SCOPE(ctx, fn);
  MpQueuePlan plan;
  HIP_TRY(mpk_queue_plan(MP_QUEUE_GOAL, model->d.n, h->sph.S, collision_has_cloud(ctx, h), ctx->compute_units, &plan));
  HIP_TRY(mpk_goal_ik(ctx->compute, model->d, collision_device(h, R), d_Tg, d_q0, (long)B, P, O, queue_grid(plan, B, max_blocks),
                      plan.lds));
  return MP_OK;
}

extern "C" {

int mp_goal_ik_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_T_goal, const double* d_q_seed, int64_t B,
                   const double* lo, const double* hi, uint32_t seed, double eomg, double ev, double damping, double step_cap,
                   int max_iters, int max_attempts, double margin, double tol, int max_blocks, int32_t* d_status, double* d_q,
                   int32_t* d_attempts, int32_t* d_iterations, int32_t* d_converged, double* d_pose_error, double* d_clearance,
                   int32_t* d_witness) {
  const char* fn = "mp_goal_ik_f64";
  CHECK_SPHERE_ENTRY(fn);
  MpGoalParams P;
  if (int rc = mp_goal_ik_check(fn, model->d.n, lo, hi, seed, eomg, ev, damping, step_cap, max_iters, max_attempts, margin, tol, &P))
    return rc;
  return goal_ik_impl(fn, ctx, model, h, d_T_goal, d_q_seed, B, P, max_blocks,
                      {d_status, d_q, d_attempts, d_iterations, d_converged, d_pose_error, d_clearance, d_witness});
}

int mp_goal_ik_host_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* T_goal, const double* q_seed, int64_t B,
                        const double* lo, const double* hi, uint32_t seed, double eomg, double ev, double damping, double step_cap,
                        int max_iters, int max_attempts, double margin, double tol, int32_t* status, double* q, int32_t* attempts,
                        int32_t* iterations, int32_t* converged, double* pose_error, double* clearance, int32_t* witness) {
  const char* fn = "mp_goal_ik_host_f64";
  CHECK_SPHERE_ENTRY(fn);
  MpGoalParams P;
  if (int rc = mp_goal_ik_check(fn, model->d.n, lo, hi, seed, eomg, ev, damping, step_cap, max_iters, max_attempts, margin, tol, &P))
    return rc;
  REQUIRE(B >= 0, "%s: negative problem count", fn);
  if (B == 0) return MP_OK;
  REQUIRE(T_goal && q_seed, "%s: null host pointer", fn);
  const size_t n = (size_t)model->d.n, ib = (size_t)B * sizeof(int32_t), db = (size_t)B * sizeof(double);
  HostCall hc(ctx);  // (h is the collision handle)
  const double *dtg = hc.in(T_goal, 16 * db), *dq0 = hc.in(q_seed, n * db);
  const MpGoalOut O = {hc.out(status, ib), hc.out(q, n * db), hc.out(attempts, ib), hc.out(iterations, ib), hc.out(converged, ib),
                       hc.out(pose_error, 2 * db), hc.out(clearance, db), hc.out(witness, 3 * ib)};
  return hc.run([&] { return goal_ik_impl(fn, ctx, model, h, dtg, dq0, B, P, 0, O); });
}

}  // extern "C"

// ---- C2 corner blending of waypoint paths over the sphere model (mp_blend.h): the corners on the work queue, then the grid.  No
// workspace, so one plan per call, made here
static int path_blend_impl(const char* fn, mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_in, const int32_t* d_count_in,
                           int64_t B, const MpBlendParams& P, int max_blocks, const MpBlendOut& O, double* d_q, double* d_dq,
                           double* d_ddq) {
  REQUIRE(max_blocks >= 0, "%s: negative max_blocks", fn);
  REQUIRE(B >= 0, "%s: negative problem count", fn);
  if (B == 0) return MP_OK;
  REQUIRE(d_in && d_count_in, "%s: null device pointer", fn);
  const bool grid = d_q || d_dq || d_ddq;
  REQUIRE(mp_out_any(O) || grid, "%s: at least one output is required", fn);
  REQUIRE(!grid || (O.status && O.count && O.points && O.cut && O.knot && O.length),
          "%s: q, dq and ddq are sampled from status, count, points, cut, knot and length: all six are required with them", fn);
  REQUIRE(aligned16(d_in) && aligned16(d_count_in) && mp_out_aligned16(O) && aligned16(d_q) && aligned16(d_dq) && aligned16(d_ddq),
          "%s: device pointers must be 16-byte aligned", fn);
  std::lock_guard<std::mutex> hl(h->mu);
  mp_collision::Resident* R = nullptr;
  if (int rc = collision_resident(fn, ctx, h, &R)) return rc;
  PROFILE_SCOPE(ctx, fn);
  MpQueuePlan plan;
  HIP_TRY(mpk_queue_plan(MP_QUEUE_BLEND, model->d.n, h->sph.S, collision_has_cloud(ctx, h), ctx->compute_units, &plan));
  HIP_TRY(mpk_path_blend(ctx->compute, model->d, collision_device(h, R), d_in, d_count_in, (long)B, P, O,
                         queue_grid(plan, B, max_blocks), plan.lds));
  if (grid)
    HIP_TRY(mpk_path_blend_sample(ctx->compute, model->d.n, (long)B, P, O.status, O.count, O.points, O.cut, O.knot, O.length, d_q, d_dq,
                                  d_ddq));
  return MP_OK;
}

extern "C" {

int mp_path_blend_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_waypoints_in, const int32_t* d_count_in,
                      int64_t B, int64_t W_in, int64_t N, double blend, int max_halvings, double margin, double tol, int max_steps,
                      int max_blocks, int32_t* d_status, int32_t* d_corner, int32_t* d_count, double* d_points, double* d_cut,
                      double* d_knot, double* d_length, int32_t* d_halvings, int32_t* d_evaluations, double* d_clearance, double* d_q,
                      double* d_dq, double* d_ddq) {
  const char* fn = "mp_path_blend_f64";
  CHECK_SPHERE_ENTRY(fn);
  MpBlendParams P;
  if (int rc = mp_path_blend_check(fn, W_in, N, blend, max_halvings, margin, tol, max_steps, &P)) return rc;
  return path_blend_impl(fn, ctx, model, h, d_waypoints_in, d_count_in, B, P, max_blocks,
                         {d_status, d_corner, d_count, d_points, d_cut, d_knot, d_length, d_halvings, d_evaluations, d_clearance}, d_q,
                         d_dq, d_ddq);
}

int mp_path_blend_host_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* waypoints_in, const int32_t* count_in,
                           int64_t B, int64_t W_in, int64_t N, double blend, int max_halvings, double margin, double tol, int max_steps,
                           int32_t* status, int32_t* corner, int32_t* count, double* points, double* cut, double* knot, double* length,
                           int32_t* halvings, int32_t* evaluations, double* clearance, double* q, double* dq, double* ddq) {
  const char* fn = "mp_path_blend_host_f64";
  CHECK_SPHERE_ENTRY(fn);
  MpBlendParams P;
  if (int rc = mp_path_blend_check(fn, W_in, N, blend, max_halvings, margin, tol, max_steps, &P)) return rc;
  REQUIRE(B >= 0, "%s: negative problem count", fn);
  if (B == 0) return MP_OK;
  REQUIRE(waypoints_in && count_in, "%s: null host pointer", fn);
  const bool grid = q || dq || ddq;
  REQUIRE(mp_out_any(MpBlendOut{status, corner, count, points, cut, knot, length, halvings, evaluations, clearance}) || grid,
          "%s: at least one output is required", fn);
  const size_t n = (size_t)model->d.n, ib = (size_t)B * sizeof(int32_t), db = (size_t)B * sizeof(double);
  const size_t wb = (size_t)W_in * db, gb = (size_t)N * n * db;
  HostCall hc(ctx);  // (h is the collision handle)
  const double* din = hc.in(waypoints_in, wb * n);
  const int32_t* dcin = hc.in(count_in, ib);
  // the tables the grid reads back stay on the device where the caller did not ask for them
  auto table_i = [&](int32_t* host, size_t bytes) { return host ? hc.out(host, bytes) : (grid ? hc.work<int32_t>(bytes) : nullptr); };
  auto table_d = [&](double* host, size_t bytes) { return host ? hc.out(host, bytes) : (grid ? hc.work<double>(bytes) : nullptr); };
  const MpBlendOut O = {table_i(status, ib), hc.out(corner, ib), table_i(count, ib), table_d(points, wb * n), table_d(cut, wb),
                        table_d(knot, wb), table_d(length, db), hc.out(halvings, ib), hc.out(evaluations, ib), hc.out(clearance, db)};
  double *dq_ = hc.out(q, gb), *ddq_ = hc.out(dq, gb), *dddq_ = hc.out(ddq, gb);
  return hc.run([&] { return path_blend_impl(fn, ctx, model, h, din, dcin, B, P, 0, O, dq_, ddq_, dddq_); });
}

}  // extern "C"

// ---- Cartesian straight-line paths over the sphere model (mp_cartesian.h): tracking, the spans on the work queue, the reduction.
// The spans' records pass through the caller's workspace; one plan per call, made here.
static int cartesian_path_impl(const char* fn, mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_q0, const double* d_Tg,
                               int64_t B, const MpCartParams& P, void* d_ws, size_t ws_bytes, int max_blocks, const MpCartOut& O,
                               double* d_q, double* d_dq, double* d_ddq) {
  REQUIRE(max_blocks >= 0, "%s: negative max_blocks", fn);
  if (B == 0) return MP_OK;
  REQUIRE(d_q0 && d_Tg, "%s: null device pointer", fn);
  REQUIRE(d_q && d_dq && d_ddq, "%s: q, dq and ddq are what the spans are read from: all three are required", fn);
  REQUIRE(aligned16(d_q0) && aligned16(d_Tg) && mp_out_aligned16(O) && aligned16(d_q) && aligned16(d_dq) && aligned16(d_ddq) &&
              aligned16(d_ws),
          "%s: device pointers must be 16-byte aligned", fn);
  const size_t need = mp_cart_work_bytes((long)B, P.grid);
  REQUIRE(d_ws && ws_bytes >= need, "%s: the workspace holds %zu bytes, the call needs %zu (mp_cartesian_path_workspace_bytes)", fn,
          d_ws ? ws_bytes : (size_t)0, need);
  std::lock_guard<std::mutex> hl(h->mu);
  mp_collision::Resident* R = nullptr;
  if (int rc = collision_resident(fn, ctx, h, &R)) return rc;
  PROFILE_SCOPE(ctx, fn);
  MpQueuePlan plan;
  HIP_TRY(mpk_cart_plan(model->d.n, P.task, h->sph.S, collision_has_cloud(ctx, h), ctx->compute_units, &plan));
  HIP_TRY(mpk_cartesian_path(ctx->compute, model->d, collision_device(h, R), P, d_q0, d_Tg, (long)B, mp_cart_work(d_ws, (long)B, P.grid), d_q,
                             d_dq, d_ddq, O, queue_grid(plan, B * (P.grid - 1), max_blocks), plan.lds));
  return MP_OK;
}

extern "C" {

int mp_cartesian_path_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_q_start, const double* d_T_goal, int64_t B,
                          const double* lo, const double* hi, int64_t N, int task, double eomg, double ev, double damping, int max_iters,
                          double max_joint_step, double margin, double tol, int max_steps, void* d_workspace, size_t workspace_bytes,
                          int max_blocks, int32_t* d_status, int32_t* d_reached, int32_t* d_span, double* d_t, double* d_clearance,
                          double* d_deviation_pos, double* d_deviation_rot, double* d_pose_error, int32_t* d_iterations,
                          int32_t* d_evaluations, double* d_q, double* d_dq, double* d_ddq, int32_t* d_span_status,
                          double* d_span_clearance) {
  const char* fn = "mp_cartesian_path_f64";
  CHECK_SPHERE_ENTRY(fn);
  MpCartParams P;
  if (int rc = mp_cartesian_path_check(fn, model->d.n, B, lo, hi, N, task, eomg, ev, damping, max_iters, max_joint_step, margin, tol,
                                       max_steps, &P))
    return rc;
  const MpCartOut O = {d_status, d_reached, d_span, d_t, d_clearance, d_deviation_pos, d_deviation_rot, d_pose_error, d_iterations,
                       d_evaluations, d_span_status, d_span_clearance};
  return cartesian_path_impl(fn, ctx, model, h, d_q_start, d_T_goal, B, P, d_workspace, workspace_bytes, max_blocks, O, d_q, d_dq, d_ddq);
}

int mp_cartesian_path_host_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* q_start, const double* T_goal, int64_t B,
                               const double* lo, const double* hi, int64_t N, int task, double eomg, double ev, double damping,
                               int max_iters, double max_joint_step, double margin, double tol, int max_steps, int32_t* status,
                               int32_t* reached, int32_t* span, double* t, double* clearance, double* deviation_pos,
                               double* deviation_rot, double* pose_error, int32_t* iterations, int32_t* evaluations, double* q, double* dq,
                               double* ddq, int32_t* span_status, double* span_clearance) {
  const char* fn = "mp_cartesian_path_host_f64";
  CHECK_SPHERE_ENTRY(fn);
  MpCartParams P;
  if (int rc = mp_cartesian_path_check(fn, model->d.n, B, lo, hi, N, task, eomg, ev, damping, max_iters, max_joint_step, margin, tol,
                                       max_steps, &P))
    return rc;
  if (B == 0) return MP_OK;
  REQUIRE(q_start && T_goal, "%s: null host pointer", fn);
  REQUIRE(mp_out_any(MpCartOut{status, reached, span, t, clearance, deviation_pos, deviation_rot, pose_error, iterations, evaluations,
                               span_status, span_clearance}) ||
              q || dq || ddq,
          "%s: at least one output is required", fn);
  const size_t n = (size_t)model->d.n, ib = (size_t)B * sizeof(int32_t), db = (size_t)B * sizeof(double);
  const size_t gb = (size_t)N * n * db, sp = (size_t)(N - 1);
  const size_t ws_bytes = mp_cart_work_bytes((long)B, (long)N);
  HostCall hc(ctx);  // (h is the collision handle)
  const double *dq0 = hc.in(q_start, n * db), *dtg = hc.in(T_goal, 16 * db);
  // the grid arrays the spans read stay on the device where the caller did not ask for them
  auto grid = [&](double* host) { return host ? hc.out(host, gb) : hc.work<double>(gb); };
  const MpCartOut O = {hc.out(status, ib), hc.out(reached, ib), hc.out(span, ib), hc.out(t, db), hc.out(clearance, db),
                       hc.out(deviation_pos, db), hc.out(deviation_rot, db), hc.out(pose_error, db), hc.out(iterations, ib),
                       hc.out(evaluations, ib), hc.out(span_status, sp * ib), hc.out(span_clearance, sp * db)};
  double *dq_ = grid(q), *ddq_ = grid(dq), *dddq_ = grid(ddq);
  void* dws = hc.work(ws_bytes);
  return hc.run([&] { return cartesian_path_impl(fn, ctx, model, h, dq0, dtg, B, P, dws, ws_bytes, 0, O, dq_, ddq_, dddq_); });
}

}  // extern "C"

// ---- fixed-rate sampling of timed paths (mp_sample.h).  I: checked and packed by mp_trajectory_sample_check, its pointers
// filled in by the caller.  The torques: up to 6 joints the same launch writes them (the fused form: measured 0.75 - 0.82 of the time
// of the launch without them followed by the inverse-dynamics kernel over the same rows, xArm6).  From 7 joints on the entry ALWAYS
// runs the split form - k_traj_sample without torques, then k_id over the rows it wrote - and never dispatches a torque instance of
// k_traj_sample: those take more than 256 registers, were measured 1.6 - 1.9 times slower than the split form (Panda, 8 joints;
// DESIGN 4.15), and k_traj_sample<8, grid, torques with a wrench> has written behind its output arrays (the cause is not
// known).  Where the caller gave no positions, velocities or accelerations for the rows, the missing arrays come from the context's
// pool for the length of the call (its reuse is ordered on the compute stream) - so such a call cannot be captured into a launch
// graph, and mp_malloc says so.
static int trajectory_sample_impl(const char* fn, mp_ctx* ctx, const mp_model* model, const MpSampleIn& I, const double* g, const double* Ftip,
                                  int max_blocks, const MpSampleOut& O) {
  REQUIRE(max_blocks >= 0, "%s: negative max_blocks", fn);
  if (I.B == 0) return MP_OK;
  REQUIRE(I.t && I.x, "%s: null device pointer", fn);
  REQUIRE(mp_out_any(O), "%s: at least one output is required", fn);
  REQUIRE(aligned16(I.t) && aligned16(I.x) && aligned16(I.q) && aligned16(I.dq) && aligned16(I.ddq) && aligned16(I.bstatus) &&
              aligned16(I.bcount) && aligned16(I.points) && aligned16(I.cut) && aligned16(I.knot) && aligned16(I.length) &&
              mp_out_aligned16(O),
          "%s: device pointers must be 16-byte aligned", fn);
  MpCall<double> c;
  make_call<double>(model, g, Ftip, &c);
  PROFILE_SCOPE(ctx, fn);
  const bool split = O.tau && model->d.n >= 7;
  MpSampleOut W = O;
  Scratch sc(ctx);
  if (split) {
    W.tau = nullptr;
    const size_t bytes = (size_t)(I.B * I.M) * (size_t)model->d.n * sizeof(double);
    for (double** rows : {&W.pos, &W.vel, &W.acc}) {
      void* p = nullptr;
      if (*rows == nullptr) {
        if (int rc = sc.get(bytes, &p)) return rc;
        *rows = static_cast<double*>(p);
      }
    }
  }
  HIP_TRY(mpk_traj_sample(ctx->compute, model->d, c, any_nonzero(Ftip), I.points != nullptr, I, W, (long)max_blocks));
  if (split) HIP_TRY(mpk_id<double>(ctx->compute, model->d, c, any_nonzero(Ftip), W.pos, W.vel, W.acc, O.tau, (long)(I.B * I.M)));
  return MP_OK;
}

extern "C" {

int mp_trajectory_sample_f64(mp_ctx* ctx, const mp_model* model, const double* d_t, const double* d_x, int64_t B, int64_t N, const double* d_q,
                             const double* d_dq, const double* d_ddq, const int32_t* d_blend_status, const int32_t* d_blend_count,
                             const double* d_points, const double* d_cut, const double* d_knot, const double* d_length, int64_t W_in,
                             double dt, int64_t M, const double* g, const double* Ftip, int max_blocks, int32_t* d_status,
                             int32_t* d_count, int32_t* d_needed, double* d_s, double* d_sd, double* d_sdd, double* d_positions,
                             double* d_velocities, double* d_accelerations, double* d_torques) {
  const char* fn = "mp_trajectory_sample_f64";
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  MpSampleIn I;
  if (int rc = mp_trajectory_sample_check(fn, B, N, W_in, dt, M, model->d.n, (d_q != nullptr) + (d_dq != nullptr) + (d_ddq != nullptr),
                                          (d_blend_status != nullptr) + (d_blend_count != nullptr) + (d_points != nullptr) +
                                              (d_cut != nullptr) + (d_knot != nullptr) + (d_length != nullptr), &I))
    return rc;
  I.t = d_t; I.x = d_x; I.q = d_q; I.dq = d_dq; I.ddq = d_ddq;
  I.bstatus = d_blend_status; I.bcount = d_blend_count; I.points = d_points; I.cut = d_cut; I.knot = d_knot; I.length = d_length;
  const MpSampleOut O = {d_status, d_count, d_needed, d_s, d_sd, d_sdd, d_positions, d_velocities, d_accelerations, d_torques};
  return trajectory_sample_impl(fn, ctx, model, I, g, Ftip, max_blocks, O);
}

int mp_trajectory_sample_host_f64(mp_ctx* ctx, const mp_model* model, const double* t, const double* x, int64_t B, int64_t N, const double* q,
                                  const double* dq, const double* ddq, const int32_t* blend_status, const int32_t* blend_count,
                                  const double* points, const double* cut, const double* knot, const double* length, int64_t W_in,
                                  double dt, int64_t M, const double* g, const double* Ftip, int32_t* status, int32_t* count,
                                  int32_t* needed, double* s, double* sd, double* sdd, double* positions, double* velocities,
                                  double* accelerations, double* torques) {
  const char* fn = "mp_trajectory_sample_host_f64";
  REQUIRE(ctx && model, "%s: null context or model", fn);
  CTX_ENTER(ctx);
  REQUIRE_SMALL(fn);
  MpSampleIn I;
  if (int rc = mp_trajectory_sample_check(fn, B, N, W_in, dt, M, model->d.n, (q != nullptr) + (dq != nullptr) + (ddq != nullptr),
                                          (blend_status != nullptr) + (blend_count != nullptr) + (points != nullptr) + (cut != nullptr) +
                                              (knot != nullptr) + (length != nullptr), &I))
    return rc;
  if (B == 0) return MP_OK;
  REQUIRE(t && x, "%s: null host pointer", fn);
  REQUIRE(mp_out_any(MpSampleOut{status, count, needed, s, sd, sdd, positions, velocities, accelerations, torques}),
          "%s: at least one output is required", fn);
  const size_t n = (size_t)model->d.n, ib = (size_t)B * sizeof(int32_t), db = (size_t)B * sizeof(double);
  const size_t gb = (size_t)N * db, wb = (size_t)W_in * db, mb = (size_t)M * db;
  HostCall hc(ctx);
  I.t = hc.in(t, gb); I.x = hc.in(x, gb);
  I.q = hc.in(q, gb * n); I.dq = hc.in(dq, gb * n); I.ddq = hc.in(ddq, gb * n);
  I.bstatus = hc.in(blend_status, ib); I.bcount = hc.in(blend_count, ib);
  I.points = hc.in(points, wb * n); I.cut = hc.in(cut, wb); I.knot = hc.in(knot, wb); I.length = hc.in(length, db);
  MpSampleOut O;
  O.status = hc.out(status, ib); O.count = hc.out(count, ib); O.needed = hc.out(needed, ib);
  O.s = hc.out(s, mb); O.sd = hc.out(sd, mb); O.sdd = hc.out(sdd, mb);
  O.pos = hc.out(positions, mb * n); O.vel = hc.out(velocities, mb * n); O.acc = hc.out(accelerations, mb * n);
  O.tau = hc.out(torques, mb * n);
  return hc.run([&] { return trajectory_sample_impl(fn, ctx, model, I, g, Ftip, 0, O); });
}

int mp_collision_set_world(mp_ctx* ctx, mp_collision* h, int O, const int32_t* kind, const double* params) {
  const char* fn = "mp_collision_set_world";
  REQUIRE(h, "%s: null collision handle", fn);
  std::vector<MpColObstacle> w;
  if (int rc = mp_collision_pack_world(fn, O, kind, params, &w)) return rc;
  if (!ctx) {
    std::lock_guard<std::mutex> hl(h->mu);
    h->world.swap(w);
    return MP_OK;
  }
  CTX_ENTER(ctx);
  REQUIRE(!ctx->capturing, "%s: not allowed while a launch graph is being captured (mp_graph_begin)", fn);
  std::lock_guard<std::mutex> hl(h->mu);
  h->world.swap(w);
  auto it = h->resident.find(ctx->uid);
  if (it != h->resident.end()) return collision_upload_world(ctx, it->second, h->world);
  mp_collision::Resident* R = nullptr;
  return collision_resident(fn, ctx, h, &R);  // (uploads the world with the rest)
}

int mp_collision_set_cloud(mp_ctx* ctx, mp_collision* h, int64_t M, const double* points, double radius, double d_max, double cell) {
  const char* fn = "mp_collision_set_cloud";
  REQUIRE(h, "%s: null collision handle", fn);
  std::vector<MpCloudPoint> img;
  if (int rc = mp_cloud_build(fn, M, points, radius, d_max, cell, &img)) return rc;
  if (!ctx) {
    std::lock_guard<std::mutex> hl(h->mu);
    h->cloud.swap(img);
    return MP_OK;
  }
  CTX_ENTER(ctx);
  REQUIRE(!ctx->capturing, "%s: not allowed while a launch graph is being captured (mp_graph_begin)", fn);
  std::lock_guard<std::mutex> hl(h->mu);
  h->cloud.swap(img);
  auto it = h->resident.find(ctx->uid);
  mp_collision::Resident* R = nullptr;
  const int rc = it != h->resident.end() ? collision_upload_cloud(ctx, it->second, h->cloud)
                                         : collision_resident(fn, ctx, h, &R);  // (uploads the cloud with the rest)
  if (rc) h->cloud.swap(img);  // the device kept its cloud: so does the twin
  return rc;
}

int mp_collision_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* d_q, int64_t rows, double eps_world,
                     double eps_self, double* d_dist_world, int32_t* d_arg_world, double* d_dist_self, int32_t* d_arg_self,
                     double* d_grad_dist_world, double* d_grad_dist_self, double* d_cost, double* d_grad) {
  return collision_impl("mp_collision_f64", ctx, model, h, d_q, rows, eps_world, eps_self,
                        {d_dist_world, d_arg_world, d_dist_self, d_arg_self, d_grad_dist_world, d_grad_dist_self, d_cost, d_grad});
}

int mp_collision_host_f64(mp_ctx* ctx, const mp_model* model, mp_collision* h, const double* q, int64_t rows, double eps_world,
                          double eps_self, double* dist_world, int32_t* arg_world, double* dist_self, int32_t* arg_self,
                          double* grad_dist_world, double* grad_dist_self, double* cost, double* grad) {
  const char* fn = "mp_collision_host_f64";
  CHECK_SPHERE_ENTRY(fn);
  REQUIRE(rows >= 0, "%s: negative row count", fn);
  if (rows == 0) return MP_OK;
  REQUIRE(q, "%s: null host pointer", fn);
  const size_t n = (size_t)model->d.n, rb = (size_t)rows * sizeof(double), ib = (size_t)rows * 2 * sizeof(int32_t);
  HostCall hc(ctx);  // (h is the collision handle)
  const double* dq = hc.in(q, n * rb);
  const MpColOut O = {hc.out(dist_world, rb), hc.out(arg_world, ib), hc.out(dist_self, rb), hc.out(arg_self, ib),
                      hc.out(grad_dist_world, n * rb), hc.out(grad_dist_self, n * rb), hc.out(cost, rb), hc.out(grad, n * rb)};
  return hc.run([&] { return collision_impl(fn, ctx, model, h, dq, rows, eps_world, eps_self, O); });
}

}  // extern "C"

int mp_set_error(int code, const char* msg) {
  std::snprintf(g_err, sizeof g_err, "%s", msg);
  return code;
}
