// host.h -- what the units of the host driver (host/*.hip: the C ABI of include/gpmp2mi.h) share: the handle structs, the
// plan, and the guards the entry points repeat.  The driver deliberately has no CPU path: every call launches kernels.
#pragma once
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../common.h"
#include "../../../include/gpmp2mi_debug.h"
#include "../launch.h"
#include "../plan.h"
#include "staging.h"

namespace g2 {
// The thread_local last-error string is private to handles.hip: set_error (common.h) writes it, this reads it.
const std::string& last_error();

// hipMalloc with the library's error plumbing; `no_device`: the code for hipErrorNoDevice (DevBuf: the calls that may be
// the first to touch the runtime)
inline int dev_malloc(void** p, size_t bytes, int no_device = GPMP2MI_ERR_ALLOC) {
  const hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess) return GPMP2MI_OK;
  *p = nullptr;
  set_error(std::string("hipMalloc: ") + hipGetErrorString(e));
  return (e == hipErrorNoDevice) ? no_device : GPMP2MI_ERR_ALLOC;
}

// RAII device buffer used by the host-pointer convenience entry points: upload() an input, alloc() scratch, out() room
// for an output that fetch() copies back to the caller's array (a null array is left alone)
template <class T>
struct DevBuf {
  T* p = nullptr;
  T* host = nullptr;
  size_t n = 0;
  int alloc(size_t count) {
    n = count;
    return count ? dev_malloc((void**)&p, count * sizeof(T), GPMP2MI_ERR_NO_DEVICE) : GPMP2MI_OK;
  }
  int upload(const T* h, size_t count) {
    G2_TRY(alloc(count));
    if (count) G2_HIP(hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice));
    return GPMP2MI_OK;
  }
  int out(T* h, size_t count) {
    host = h;
    return alloc(count);
  }
  int fetch() const {
    if (n && host) G2_HIP(hipMemcpy(host, p, n * sizeof(T), hipMemcpyDeviceToHost));
    return GPMP2MI_OK;
  }
  ~DevBuf() { if (p) (void)hipFree(p); }
};
// the closing step of a host-array call on the null stream: wait for the kernels, then copy the outputs back
template <class... Bufs>
int fetch_all(const Bufs&... bufs) {
  G2_HIP(hipStreamSynchronize(nullptr));
  int rc = GPMP2MI_OK;
  ((rc = rc != GPMP2MI_OK ? rc : bufs.fetch()), ...);
  return rc;
}

// A device workspace that only grows, owned by its handle (the stage workspaces of a plan, the records of a robot
// handle; laid out by staging.h).  hipFree waits for the device, so whatever still reads the old block is done before it
// goes; a call whose shape the block already holds neither allocates nor synchronises.
struct Workspace {
  void* p = nullptr;
  size_t bytes = 0;
  Workspace() = default;
  Workspace(const Workspace&) = delete;
  int reserve(size_t need) {
    if (need <= bytes) return GPMP2MI_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    G2_TRY(dev_malloc(&p, need));
    bytes = need;
    return GPMP2MI_OK;
  }
  void leak() { p = nullptr; bytes = 0; }   // a hung kernel may still write the block: it goes with a poisoned plan
  ~Workspace() { if (p) (void)hipFree(p); }
};
// Carves `ws` by `layout` (base -> a staging.h layout with its .bytes) into *w.  A call whose shape the block already
// holds carves once; otherwise the block grows first and is carved again (the first carving gave the size alone).
template <class W, class L>
int carve_into(Workspace& ws, L&& layout, W* w) {
  *w = layout(ws.p);
  if (w->bytes <= ws.bytes) return GPMP2MI_OK;
  G2_TRY(ws.reserve(w->bytes));
  *w = layout(ws.p);
  return GPMP2MI_OK;
}

// The two lower Cholesky factors of the sampled clearance (sampled.hip; include/gpmp2mi.h "sampled clearance"): formed on
// the host for a key (Qc, delta_t, inter_step, dof), kept on the host and the device.  A handle keeps the factors of its
// last SAMPLED_FAC_KEYS keys, so calls that alternate between a few inter_steps neither copy nor wait; a new key takes the
// oldest entry's place.
constexpr int SAMPLED_FAC_KEYS = 4;
struct SampledFacEntry {
  double* dev = nullptr;      // Lp packed by rows at +0 (room for inter_step = SAMPLED_MAX_INTER), C [D][D] behind it
  std::vector<double> host;   // what `dev` holds
  std::vector<double> qc;     // the key: Qc (empty: identity), delta_t, inter_step, dof
  double dt = 0.0;
  int inter = -1, dof = 0;
};
struct SampledFac {
  SampledFacEntry e[SAMPLED_FAC_KEYS];
  int next = 0;               // the entry a new key replaces
  void release() {            // by the owner's destructor (a poisoned plan leaks its blocks: hipFree would wait for it)
    for (auto& x : e)
      if (x.dev) (void)hipFree(x.dev);
  }
};

// handles.hip
int ensure_device();
void gp_winv(double dt, double W[4]);
GpCoef gp_coef(double dt, double tau);
bool invert_small(int n, const double* A, double* Ainv);
// copies of robot / field handles on other devices (multi_plan.hip) alive now: gpmp2mi_debug_replica_counts
extern std::atomic<long> g_robot_replicas, g_sdf_replicas;

}  // namespace g2

struct gpmp2mi_robot {
  g2::RobotDev h;
  g2::RobotDev* d = nullptr;
  int device = -1;        // the device `d` lives on (current device at creation)
  bool replica = false;   // a multi plan's copy (robot_replica)
  // records of gpmp2mi_score_traj(_dev) calls on this handle (score.hip), on `device`, grown on demand and kept.
  // score_mu guards the pointer against host threads that share the handle; the records themselves belong to one
  // call at a time, so such calls must be in stream order (include/gpmp2mi.h "scoring", Memory).
  mutable std::mutex score_mu;
  mutable g2::Workspace score_ws;
  // the bridge factors of gpmp2mi_sampled_clearance_traj(_dev) calls on this handle, under the same guard and rule
  mutable g2::SampledFac sampled_fac;
  // the records of gpmp2mi_motion_score_traj(_dev) calls on this handle (motion_score.hip), under the same guard and rule
  mutable g2::Workspace motion_ws;
  // the records of gpmp2mi_moving_score_traj(_dev) calls on this handle (moving.hip), under the same guard and rule
  mutable g2::Workspace moving_ws;
  // the records of gpmp2mi_path_score_traj(_dev) calls on this handle (path.hip), under the same guard and rule
  mutable g2::Workspace path_ws;
  // the records of gpmp2mi_carried_score_traj(_dev) calls on this handle (carried.hip), under the same guard and rule
  mutable g2::Workspace carried_ws;
  // the workspace of gpmp2mi_retime_traj(_dev) calls on this handle (retime.hip), under the same guard and rule
  mutable g2::Workspace retime_ws;
  ~gpmp2mi_robot() {
    if (d) (void)hipFree(d);
    sampled_fac.release();
    if (replica) g2::g_robot_replicas.fetch_sub(1);
  }
};
struct gpmp2mi_sdf {
  g2::SdfDev h;
  double* plain = nullptr;
  double* cells = nullptr;
  int device = -1;        // the device `plain` / `cells` live on (current device at sdf_alloc)
  bool replica = false;   // a multi plan's copy (sdf_replica)
  // live map (map.hip; include/gpmp2mi.h "live map"): two int32 volumes, the byte mask of the base, [MAXS][3] sphere
  // centres and four counters in one block on `device`, taken at the first update or by gpmp2mi_sdf_reserve_update and
  // kept.  has_base: the mask holds the obstacle set of the last gpmp2mi_sdf_update_from_occupancy(_dev).
  void* map_ws = nullptr;
  bool has_base = false;
  // gpmp2mi_debug_sdf_update_timing: five events around the four stages of an update, recorded while map_timing
  hipEvent_t map_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  bool map_timing = false;
  // sensor map (sensor.hip; include/gpmp2mi.h "sensor map"): the int16 evidence, the two byte volumes of marks and six
  // counters in one block on `device`, taken at the first call of that section or by gpmp2mi_sdf_reserve_evidence and
  // kept.  ray_ws: the records of one frame's rays ([M][3] cell coordinates, [M] classes), grown when a frame has more
  // rays than any before.  sensor_ev: the events in front of the three sensor stages (the rest are map_ev's).
  void* ev_ws = nullptr;
  g2::Workspace ray_ws;
  hipEvent_t sensor_ev[3] = {nullptr, nullptr, nullptr};
  ~gpmp2mi_sdf() {   // also runs when a create function fails half-way (unique_ptr)
    if (plain) (void)hipFree(plain);
    if (cells) (void)hipFree(cells);
    if (map_ws) (void)hipFree(map_ws);
    if (ev_ws) (void)hipFree(ev_ws);
    for (hipEvent_t e : map_ev)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : sensor_ev)
      if (e) (void)hipEventDestroy(e);
    if (replica) g2::g_sdf_replicas.fetch_sub(1);
  }
};

// A pair table of the self-collision check (self_score.hip; include/gpmp2mi.h "self-collision check"), bound to the
// sphere model of the robot it was made for.  An empty table holds nothing on the device.
struct gpmp2mi_self_pairs {
  int P = 0, S = 0, dof = 0, kind = 0;
  int device = -1;            // the device `d` lives on (-1: empty table)
  std::vector<double> data;   // [P][4] as the caller gave it
  g2::SelfPair* d = nullptr;  // [P]
  // records of gpmp2mi_self_score_traj(_dev) calls with this table, by the rules of gpmp2mi_robot::score_ws
  mutable std::mutex mu;
  mutable g2::Workspace ws;
  ~gpmp2mi_self_pairs() {
    if (d) (void)hipFree(d);
  }
};

// The inertial table of a fixed-base arm (torque.hip; include/gpmp2mi.h "torque limits"), bound to the kinematics of
// the robot it was made for: the table on the device, the limits and gravity on the host (they travel as a kernel
// argument).
struct gpmp2mi_dynamics {
  g2::RobotDev robot;          // the kinematics the table belongs to, as the robot handle had them at creation
  g2::TorqueLimitsDev lim;     // +inf: no limit
  int device = -1;             // the device `d` lives on
  g2::DynDev* d = nullptr;
  // records (and nothing else) of gpmp2mi_torque_score_traj(_dev) calls with this handle, by the rules of
  // gpmp2mi_robot::score_ws: mu guards the pointer, the calls themselves must be in stream order
  mutable std::mutex mu;
  mutable g2::Workspace ws;
  // the workspace of gpmp2mi_retime_dynamic_traj(_dev) calls with this handle (retime_dynamic.hip), under the same guard
  // and rule
  mutable g2::Workspace retime_ws;
  ~gpmp2mi_dynamics() {
    if (d) (void)hipFree(d);
  }
};

// A scene (scene.hip; include/gpmp2mi.h "scene"): the objects on the host as they were given (poses and enabled flags
// change in place), the meshes' vertices and triangles on the device, and the workspace of a rasterisation.
struct gpmp2mi_scene {
  struct Object {
    int kind = 0, enabled = 0;
    double s[3] = {0.0, 0.0, 0.0};   // size + inflate of a primitive
    double pose[12] = {};
    int V = 0, T = 0;
    size_t vert_off = 0, tri_off = 0, q_off = 0;   // bytes into `geo` (meshes)
  };
  std::vector<Object> obj;
  int device = -1;
  char* geo = nullptr;        // every mesh's vertices [V][3] fp64, triangles [T][3] and fixed-point vertices [V][3] int32
  int* counts = nullptr;      // [K] cells of the call in flight, behind them [K] out-of-range flags
  // crossing bits of one mesh, [nz][ny][nx rounded up to 32], all 0 between two meshes; taken at the first call for a
  // grid (or by gpmp2mi_scene_reserve) and grown when a later grid needs more
  mutable g2::Workspace bits;
  // gpmp2mi_debug_scene_timing: events in front of the primitives, between them and the meshes, and behind the meshes
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  bool timing = false;
  ~gpmp2mi_scene() {
    if (geo) (void)hipFree(geo);
    if (counts) (void)hipFree(counts);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace g2 {
// geometry + device storage of a field handle; the caller fills s->plain ([nz][ny][nx]) and packs (handles.hip)
int sdf_alloc(int dim, const double origin[3], double cell, int nx, int ny, int nz, std::unique_ptr<gpmp2mi_sdf>& s);
// caller layout -> [nz][ny][nx] (handles.hip); `tmp` holds the reordered copy when one is needed
const double* to_zyx(const double* vox, int layout, int nx, int ny, int nz, std::vector<double>& tmp);

// map.hip, shared with sensor.hip.  The handle's update workspace for n cells:
struct MapWs {
  int *wa, *wb;          // [n] squared distance to the obstacle set / to the free set
  unsigned char* mask;   // [n] the base: 1 on the obstacle cells of the last update from occupancy
  double* cen;           // [MAXS][3] sphere centres of the self filter
  int* cnt;              // [4] kept, non-finite, self, outside
  size_t bytes;
};
MapWs map_ws_layout(char* base, size_t n);
inline size_t cells_of(const gpmp2mi_sdf* s) { return (size_t)s->h.nx * s->h.ny * s->h.nz; }
// what every update does once its arguments are accepted: a device, the handle's device current, the workspace
int map_ready(gpmp2mi_sdf* s, bool transform);
// the event in front of stage k while the handle's stage timer is on
void mark_stage(gpmp2mi_sdf* s, int k, hipStream_t st);
// the two seeded volumes -> plain -> cells on `st`
int map_transform(gpmp2mi_sdf* s, const MapWs& w, hipStream_t st);
// sensor.hip, for scene.hip: the two volumes seeded from {E >= occupied_at}, united with the base if use_base, on `st`.
// E, the marks and the base stay as they are; the handle must have its evidence (s->ev_ws) and its update workspace.
int evidence_seed(gpmp2mi_sdf* s, int occupied_at, int use_base, hipStream_t st);

struct KernelTimer {
  // One HIP event per kernel boundary on the launch stream: begin(name) is recorded right before kernel `name`,
  // close() after the last kernel of a pass; a kernel's time is the distance to the next mark.
  bool enabled = false;
  struct Rec {
    const char* name;  // nullptr = closing mark
    hipEvent_t ev;
  };
  std::vector<Rec> recs;
  std::vector<std::string> names;
  std::vector<double> ms;
  std::vector<int> launches;
  std::vector<const char*> cnames;
  std::vector<hipEvent_t> pool;
  size_t pool_used = 0;
  hipEvent_t get() {
    if (pool_used == pool.size()) {
      hipEvent_t e;
      // timing only: no system-scope fence when the event fires (the default flushes caches between the
      // two kernels it separates)
      (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
      pool.push_back(e);
    }
    return pool[pool_used++];
  }
  void begin(const char* name, hipStream_t st) {
    if (!enabled) return;
    Rec r{name, get()};
    (void)hipEventRecord(r.ev, st);
    recs.push_back(r);
  }
  void close(hipStream_t st) { begin(nullptr, st); }
  void reset() {
    recs.clear();
    pool_used = 0;
    names.clear();
    ms.clear();
    launches.clear();
  }
  void collect();   // plan_run.hip
  ~KernelTimer() {
    for (auto e : pool) (void)hipEventDestroy(e);
  }
};

// a pinned, device-mapped int array from the pool of flags_acquire / flags_release
struct FlagBuf {
  int* host = nullptr;
  int* dev = nullptr;
  int cap = 0;
  int device = -1;   // pooled buffers are reused on the device they were mapped / allocated for only
};
// plan_create.hip; the pools, their mutex and the live counters are private to that unit
int flags_acquire(int need, FlagBuf* out);
void flags_release(const FlagBuf& f);   // a buffer that was never acquired (host == nullptr) is left alone

// The kernel forms of a plan, chosen once at creation (choose_forms).  The int fields go to PlanParams (plan.h), where
// the kernels read them; `dense` and `generic_gn` are host-only choices of the drivers in plan_run_impl.
struct PlanForms {
  int wide = 0, split_back = 0, wide_h0 = 2, lin_split = 1, fuse_finish = 0, spart_groups = 0;
  bool dense = false;        // dense normal equations + cyclic reduction over dense blocks: dof 12..18, or forced for 8..11
  bool generic_gn = false;   // forced: the plan's Gauss-Newton optimize runs through the trial-step driver
  bool no_early_stop = false;   // forced: the Gauss-Newton fast driver keeps the step control behind k_assemble
  // Gauss-Newton takes the fast driver (3 launches per pass) on every plan that is not wide; a forced generic GN sends
  // only the plan's own optimize through the trial-step driver, not plan_update
  bool gn_fast(bool update) const { return !wide && (update || !generic_gn); }
  // Gauss-Newton fast driver: the step control reads the per-chunk error shares of k_linearize_arm, in k_assemble (which
  // then builds nothing for a trajectory that stops) and in k_gn_step_cr alike.  A property of the run, not of the
  // parameter block: gpmp2mi_plan_update sends LM / Dogleg plans through that driver too, and a plan's extra factors
  // (`extras`) add their errors to the records behind the linearization, where the shares do not see them.
  bool early_stop(bool extras) const { return lin_split == 4 && !extras && !no_early_stop; }
  // trial-step driver, LM / GN (Dogleg's step kernel does the whole back-substitution): k_finish_trial(_wide) finishes
  // the step, or the trial linearization forms the trial point cur (+) delta itself (k_linearize_arm, `trial`)
  bool finish_trial(int opt) const { return split_back && opt != GPMP2MI_OPT_DOGLEG && !fuse_finish; }
  bool trial_lin_steps(int opt) const { return fuse_finish && opt != GPMP2MI_OPT_DOGLEG; }
};
}  // namespace g2

struct gpmp2mi_plan {
  const gpmp2mi_robot* robot = nullptr;
  const gpmp2mi_sdf* sdf = nullptr;
  g2::PlanParams hp;
  g2::PlanForms forms;         // the kernel forms chosen at creation (choose_forms); hp carries the device-visible ones
  g2::PlanBuffers pb;
  std::vector<void*> allocs;   // arena chunks (plan_alloc)
  std::vector<size_t> alloc_bytes;
  char* arena_cur = nullptr;   // bump pointer into the newest chunk
  size_t arena_left = 0;
  int alloc_calls = 0;         // plan_alloc calls so far
  int fail_alloc_at = 0;       // gpmp2mi_debug_forms::fail_alloc_at: the k-th plan_alloc call fails (0: none)
  int device = -1;             // the device the plan was created on: its chunks / flags go back to that device's pools
  g2::FlagBuf flagbuf;
  int* h_flags = nullptr;    // pinned + device-mapped [n_active_len]: per-pass active count, -1 = not yet known
  g2::KernelTimer timer;
  int n_active_len = 0;
  std::vector<int> h_xp_n;   // host mirror of the extra-prior counts
  std::vector<char> goal_removed;   // 1 after gpmp2mi_plan_remove_goal until gpmp2mi_plan_change_goal (queue runs refuse it)
  g2::PlanExtras ex;         // extra factors carried as data (host copy of the specs + device workspace)
  bool has_extras = false;
  bool problem_set = false;
  bool optimized = false;
  // Streams that may still carry work of this plan (asynchronous copies / kernels enqueued without a closing
  // synchronisation).  gpmp2mi_plan_destroy waits for exactly these, never for the whole device.
  std::vector<hipStream_t> dirty_streams;
  bool null_stream_dirty = false;
  // A pass that did not finish within GPMP2MI_WAIT_TIMEOUT_MS: the stream may hold a hung kernel of this plan.  The
  // plan refuses further work, and its memory is neither waited for nor recycled (a hung kernel would hang the wait,
  // a late one would write into recycled memory): it is deliberately leaked.
  bool poisoned = false;
  // queue runs (plan_queue_impl): device workspace of the per-slot words and the pass-indexed scratch of the step
  // kernels, grown on demand; host-mapped per-pass counts; the statistics of the last run
  g2::FlagBuf qflags;
  gpmp2mi_queue_stats qstats{};
  bool queue_ran = false;
  // The workspaces of the stages, one each (calls of different stages may be in flight at once), taken at a stage's first
  // call and kept, grown when a later call needs more.  An array, so that a poisoned plan leaks every one of them.
  //   QUEUE    the per-slot words and the pass-indexed scratch of the step kernels of a queue run
  //   SCORE    the records of k_score and the staging of the host-pointer forms (CheckWs: staging.h)
  //   POST     the exported normal equations and the factor scratch of k_posterior
  //   SEED     H_seed on the device with its factors (uploaded and factored at the first seeded call)
  //   RISK     the band of Sigma, ok and the records of k_risk
  //   SAMPLED  a chunk of delta, its records, the carried counts and ok
  //   SELF     CheckWs with the records of k_self_clearance and those of k_score for select_checked
  //   GROUP    the bit matrix of k_traj_pairs, the per-row scores the rule reads, what k_group_rule leaves, the staging
  //   MOTION, MOVING, PATH, CARRIED   CheckWs with the stage's records and the per-row scores of the earlier stages its rule reads
  //   RETIME   ps, the caps and the sets of k_retime, the profile, the scores of the earlier stages, the staging
  //   TORQUE   the records of k_torque, the scores of the earlier stages, the staging with the torques, the pick
  //   RETIME_DYN   what RETIME keeps, the coefficients, the stage rows of k_retime_rows and the torques of every row
  enum Ws { WS_QUEUE, WS_SCORE, WS_POST, WS_SEED, WS_RISK, WS_SAMPLED, WS_SELF, WS_GROUP, WS_MOTION, WS_MOVING, WS_PATH,
            WS_RETIME, WS_TORQUE, WS_CARRIED, WS_RETIME_DYN, WS_COUNT };
  g2::Workspace ws[WS_COUNT];
  // seeding (seed.hip): H_seed of the plan's linear prior graph on the host (built at the first seeded call or read-out)
  std::vector<double> seed_Hd, seed_Ho;
  bool seed_ready = false;
  // posterior on the executed timeline (risk.hip): Qc of the setting, on the host from creation and on the device from
  // the first marginals_dense / risk call
  std::vector<double> Qc;
  double* risk_qc = nullptr;
  // sampled clearance (sampled.hip): the bridge factors of the last (inter_step)s asked for
  g2::SampledFac sampled_fac;
  size_t tsz() const { return (size_t)hp.B * (hp.N + 1) * hp.n; }
  void mark_dirty(hipStream_t st) {
    if (!st) { null_stream_dirty = true; return; }
    if (std::find(dirty_streams.begin(), dirty_streams.end(), st) == dirty_streams.end()) dirty_streams.push_back(st);
  }
  void mark_clean(hipStream_t st) {
    if (!st) { null_stream_dirty = false; return; }
    dirty_streams.erase(std::remove(dirty_streams.begin(), dirty_streams.end(), st), dirty_streams.end());
  }
  // closes a group of copies enqueued on `st`: host-side ones are waited for, device-side ones leave the stream dirty
  int close_copies(hipMemcpyKind kind, hipStream_t st) {
    mark_dirty(st);
    if (kind == hipMemcpyDeviceToDevice) return GPMP2MI_OK;
    G2_HIP(hipStreamSynchronize(st));
    mark_clean(st);
    return GPMP2MI_OK;
  }
  // wait for whatever this plan still has in flight (a no-op after the usual optimize -> get_result sequence)
  void drain() {
    if (poisoned) return;
    for (hipStream_t st : dirty_streams) (void)hipStreamSynchronize(st);
    dirty_streams.clear();
    if (null_stream_dirty) (void)hipStreamSynchronize(nullptr);
    null_stream_dirty = false;
  }
  ~gpmp2mi_plan();   // plan_create.hip, next to the pools it returns the plan's memory to
};

// The liveness guards: a plan (a multi plan) whose pass timed out refuses further work.  They stand in the entry points
// after the null-argument checks.
#define G2_PLAN_LIVE(p)                         \
  G2_CHECK(!(p)->poisoned, GPMP2MI_ERR_TIMEOUT, \
           "this plan timed out earlier and may still have a hung kernel in its stream: destroy it and create a new one")
#define G2_MULTI_LIVE(m)                                                                                            \
  do {                                                                                                              \
    G2_CHECK(m, GPMP2MI_ERR_INVALID, "null multi plan");                                                            \
    G2_CHECK(!(m)->poisoned, GPMP2MI_ERR_TIMEOUT,                                                                   \
             "a shard of this multi plan timed out earlier and may still have a hung kernel: destroy it and create a new one"); \
  } while (0)

namespace g2 {
// restores the calling thread's current device on scope exit (multi-plan calls switch devices shard by shard)
struct DeviceGuard {
  int dev = -1;
  DeviceGuard() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
  ~DeviceGuard() { if (dev >= 0) (void)hipSetDevice(dev); }
};

// Device staging of M problems of a queue run given in host arrays `io`: one slab, the ten arrays of a QueueRun carved
// out of it (doubles first, ints after; an output the caller does not ask for gets no room).  upload / download copy rows
// [j, j + M) of the caller's arrays on a stream; the caller synchronises.
struct QueueStage {
  QueueStage() = default;
  QueueStage(const QueueStage&) = delete;   // owns `base`
  void* base = nullptr;
  QueueRun q{};   // M and the ten array pointers
  size_t D = 0, tr = 0, T = 0;
  int alloc(int M, const QueueRun& io, int D_, size_t trow, int T_);
  // with_init = false: the four end arrays only (the seeded queue makes the inits on the device)
  int upload(const QueueRun& io, size_t j, hipStream_t st, bool with_init = true) const;
  int download(const QueueRun& io, size_t j, hipStream_t st) const;
  void leak() { base = nullptr; }   // a hung kernel may still write the slab: it goes with the poisoned plan
  void release() {                  // hipFree waits for the whole device
    if (base) (void)hipFree(base);
    base = nullptr;
  }
  ~QueueStage() { release(); }
};

// plan_run.hip
int plan_set_problem(gpmp2mi_plan* p, const double* sc, const double* sv, const double* ec, const double* ev,
                     const double* init, hipMemcpyKind kind, hipStream_t st);
int plan_get_result(gpmp2mi_plan* p, double* traj, int* iters, double* ferr, int* status, double* trace,
                    hipMemcpyKind kind, hipStream_t st);
// `io`: M and the ten arrays of the queue run; `host`: they are host arrays, staged here
int plan_optimize_queue(gpmp2mi_plan* p, QueueRun io, bool host, hipStream_t st);
// linearize `traj` into record buffer `bufsel` of every (active) trajectory, extra factors included
int plan_linearize(gpmp2mi_plan* p, const double* traj, int bufsel, const int* active, hipStream_t st,
                   double* dst = nullptr, int pass = 0, bool trial = false);
int spin_wait_flag(const volatile int* flag, bool st_valid, hipStream_t st, double timeout_s, int* count);

// posterior.hip: linearize -> export -> factor-only k_posterior at the plan's current estimate on `st`; *fac: the factor
// scratch it leaves, [B][N+1][512] (V at +0, W at +256), valid until the next posterior call on the plan
int plan_posterior_factor(gpmp2mi_plan* p, int* ok, const double** fac, hipStream_t st);
// the state rules of the plan posterior calls (null, poisoned, no problem, blocks wider than one tile), and the band of
// Sigma at the current estimate into device arrays on `st` (risk.hip: the plan's band workspace)
int plan_posterior_check(gpmp2mi_plan* p);
int plan_posterior_band(gpmp2mi_plan* p, double* Sd, double* So, int* ok, hipStream_t st);
// seed.hip: the checks of a seeded restart call (arguments, liveness, the limits), then M restarts of problems
// first .. first + M - 1 into `init` on `st` (device pointers; mean null: the straight line from sc to ec)
int plan_seed_check(gpmp2mi_plan* p, int M, int first, double scale);
int plan_seed_restarts(gpmp2mi_plan* p, int M, uint64_t seed, int first, double scale, int keep_first, const double* sc,
                       const double* ec, const double* mean, double* init, hipStream_t st);

// score.hip: the selection of a select call (any pointer may be null); the per-row outputs are staging.h's ScoreOut
struct ScoreSel {
  double required_clearance = 0.0;
  int require_in_range = 0;
  int *best = nullptr, *n_eligible = nullptr;
  double *traj_best = nullptr, *dense_best = nullptr;
  double* best_error = nullptr;   // host forms only: final_error of the chosen row (the multi plan's pick needs it)
};
// Scores the plan's resident result on `st`; sel != null: applies the rule and copies the chosen row as well.
// host: the outputs are host arrays (staged in the plan's scoring workspace, copied back, `st` synchronised);
// otherwise device pointers, and the call returns without a host synchronisation.
int plan_score(gpmp2mi_plan* p, int inter, const ScoreOut& out, const ScoreSel* sel, bool host, hipStream_t st);
// self_score.hip: the same for the self-collision check against `t` (out.oor: invalid); sel adds k_score for the same
// rows and the rule with both clearances
struct SelfSel : ScoreSel {
  double required_self_clearance = 0.0;
};
int plan_self_score(gpmp2mi_plan* p, const gpmp2mi_self_pairs* t, int inter, const ScoreOut& out, const SelfSel* sel,
                    bool host, hipStream_t st);
// the argument rules the score calls share (inter_step, B, total_step, delta_t, the launch limits)
int check_score_args(int inter, int B, int total_step, double delta_t);

// check_common.hip: the driver the check stages share.  A plan form goes: its own argument checks, check_plan_ready,
// its workspace (carve_into by a staging.h layout), plan_shape and, for a selection, point_selection and
// enqueue_prior_stages, mark_dirty, its launches, and for a host form finish_host.
// What every plan form checks once its own arguments are accepted: live, optimized, check_score_args, the dof.
int check_plan_ready(gpmp2mi_plan* p, int inter);
// B, N, D, lie, inter, Md, dt and traj of a finish kernel on the plan's resident result
void plan_shape(ScoreFinish& g, const gpmp2mi_plan* p, int inter);
// the same shape for a staging.h layout
inline Shape shape_of(const gpmp2mi_plan* p, int inter) {
  const PlanParams& P = p->hp;
  return Shape{(size_t)P.B, (size_t)P.N, (size_t)P.D, (size_t)P.N * (inter + 1) + 1};
}
// What a stage's selection adds to ScoreSel's outputs (motion limits: time_scale_best; re-timing: duration_best and
// stamps_best): one double about the chosen row, carried in the pick, and one more array of that row.
struct SelExtra {
  double* value = nullptr;
  double* row = nullptr;
  size_t row_bytes = 0;
};
// The selection of `g`: the rule's inputs, and its outputs pointed at the caller's arrays (device form) or at the
// workspace (host form; only what the caller asked for).  x: the caller's extra outputs, or null for a stage without;
// returns where the stage's kernel writes them.
SelExtra point_selection(ScoreFinish& g, const gpmp2mi_plan* p, const ScoreSel& sel, const SelExtra* x, bool host,
                         const PickRows& w);
// Enqueues plan_self_score (pairs != null) and plan_score for the plan's rows into `w` on `st`; *got: the rows written
// (the self pair null without a table)
int enqueue_prior_stages(gpmp2mi_plan* p, const gpmp2mi_self_pairs* pairs, int inter, const PriorRows& w, hipStream_t st,
                         PriorRows* got);
// the one read-back: an asynchronous copy to a host array on `st`; a null array or no bytes is left alone
int copy_back(void* dst, const void* src, size_t bytes, hipStream_t st);
// Closes a host form: the staged rows back, the pick in one copy, a synchronisation, the caller's scalars; if a row was
// chosen and its arrays are asked for, those and a second synchronisation; the stream clean.
int finish_host(gpmp2mi_plan* p, int inter, const RowOut* rows, int n_rows, const ScoreSel* sel, const SelExtra* x,
                const PickRows& w, hipStream_t st);
// What a caller-buffer `_dev` form does once its arguments are accepted and B > 0: a device, the handle(s) on the current
// one, the lock that guards the handle's records (t != null: the pair table's, else the robot's) and room for them
int records_ready(const gpmp2mi_robot* r, const gpmp2mi_self_pairs* t, Workspace& ws, size_t bytes,
                  std::unique_lock<std::mutex>& lk);
// motion_score.hip, shared with retime.hip: the rules of a gpmp2mi_motion_limits that need no robot handle (the struct
// itself and its scalar), and its arrays [dof] as the kernels read them (+-inf where there is no limit)
int check_limits_head(const gpmp2mi_motion_limits* l);
int read_limits(const gpmp2mi_motion_limits* l, int dof, MotionLimitsDev* out);
// retime.hip and torque.hip, shared with retime_dynamic.hip: the rules of the three rates and of the arrays of
// gpmp2mi_retime_path (acc [D] or null -> acc_out [GPMP2MI_MAX_DOF], +inf: none), and the binding of a dynamics handle to
// the robot it was made for
struct RetimeRates {
  double max_rate, rate_start, rate_end;
};
int check_retime_rates(const RetimeRates& r);
int check_retime_path_call(int B, int Md, int dof, const double* qd, const double* ql, const double* qr, const double* cap,
                           const double* acc, double h, const RetimeRates& rt, double* acc_out);
int check_dynamics_binding(const gpmp2mi_robot* r, const gpmp2mi_dynamics* y);
// B comparisons on the host: the rule of gpmp2mi_select_best
void select_rule_host(int B, const double* ferr, const int* status, const double* clearance, const int* oor,
                      double required_clearance, int require_in_range, int* best, int* n_eligible);
}  // namespace g2
