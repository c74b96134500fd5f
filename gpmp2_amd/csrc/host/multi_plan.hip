// multi_plan.hip -- multi-device plans (gpmp2mi_multi_plan_*): one batch over several devices of
// this process.  One ordinary plan per shard on its own device and non-blocking stream, the robot and the field copied
// once to every other device, no exchange between the shards until the results are gathered.  Everything here is host
// code around the plan drivers.
#include <functional>
#include <thread>

#include "host.h"

using namespace g2;

// A copy of a robot handle on device `dev`: the same host-side model, a new device copy of it.
static int robot_replica(const gpmp2mi_robot* src, int dev, std::unique_ptr<gpmp2mi_robot>& out) {
  G2_HIP(hipSetDevice(dev));
  auto r = std::make_unique<gpmp2mi_robot>();
  r->h = src->h;
  r->device = dev;
  r->replica = true;
  g_robot_replicas.fetch_add(1);
  G2_HIP(hipMalloc((void**)&r->d, sizeof(RobotDev)));
  G2_HIP(hipMemcpy(r->d, &r->h, sizeof(RobotDev), hipMemcpyHostToDevice));
  out = std::move(r);
  return GPMP2MI_OK;
}
// A copy of a field handle on device `dev`: the same geometry, a peer copy of the voxels, packed there by the same
// kernel as the source (so the cells are bit-identical).
static int sdf_replica(const gpmp2mi_sdf* src, int dev, std::unique_ptr<gpmp2mi_sdf>& out) {
  G2_HIP(hipSetDevice(dev));
  const SdfDev& g = src->h;
  const double origin[3] = {g.ox, g.oy, g.oz};
  std::unique_ptr<gpmp2mi_sdf> s;
  G2_TRY(sdf_alloc(g.dim, origin, g.cell, g.nx, g.ny, g.nz, s));
  s->replica = true;
  g_sdf_replicas.fetch_add(1);
  s->h = g;   // every geometry word exactly as the source's
  s->h.plain = s->plain;
  s->h.cells = s->cells;
  G2_HIP(hipMemcpyPeer(s->plain, dev, src->plain, src->device, (size_t)g.nx * g.ny * g.nz * sizeof(double)));
  G2_TRY(launch_sdf_pack(s->h, s->cells, nullptr));
  G2_HIP(hipStreamSynchronize(nullptr));
  out = std::move(s);
  return GPMP2MI_OK;
}
struct MultiShard {
  int device = -1;
  int row0 = 0, rows = 0;          // batch rows [row0, row0 + rows)
  gpmp2mi_plan* plan = nullptr;
  hipStream_t stream = nullptr;    // non-blocking: null-stream work of other shards on the device does not wait for it
  hipEvent_t copied = nullptr;     // get_result_dev: recorded after this shard's gather copies
  gpmp2mi_queue_stats qstats{};    // of the last multi-plan queue run (zero when the shard sat out)
  bool poisoned() const { return plan && plan->poisoned; }
};
struct MultiReplica {
  int device = -1;
  std::unique_ptr<gpmp2mi_robot> robot;   // null: the caller's handle lives on this device
  std::unique_ptr<gpmp2mi_sdf> sdf;
};

struct gpmp2mi_multi_plan {
  int B = 0, D = 0, N = 0, T = 0;  // T = max_iter + 1 (error trace columns)
  std::vector<MultiShard> shards;
  std::vector<MultiReplica> replicas;
  const gpmp2mi_sdf* src_sdf = nullptr;            // the caller's field handle: what refresh_field copies from
  std::vector<std::pair<int, hipEvent_t>> entry;   // get_result_dev: per gather device, recorded on the caller's stream
  bool problem_set = false, optimized = false, queue_ran = false;
  bool poisoned = false;           // a shard timed out: every later call returns GPMP2MI_ERR_TIMEOUT
  size_t trow() const { return (size_t)(N + 1) * 2 * D; }
  // Per shard: its plan (leaked by gpmp2mi_plan_destroy when poisoned), then its stream and event unless poisoned; then
  // the copies, except on a device where a poisoned shard may still run.
  ~gpmp2mi_multi_plan() {
    DeviceGuard guard;
    std::vector<int> bad;
    for (MultiShard& sh : shards) {
      (void)hipSetDevice(sh.device);
      const bool pz = sh.poisoned();
      if (pz) bad.push_back(sh.device);
      if (sh.plan) gpmp2mi_plan_destroy(sh.plan);   // drains the plan's streams unless poisoned
      if (pz) continue;
      if (sh.copied) (void)hipEventDestroy(sh.copied);
      if (sh.stream) (void)hipStreamDestroy(sh.stream);
    }
    for (auto& e : entry) {
      (void)hipSetDevice(e.first);
      (void)hipEventDestroy(e.second);
    }
    for (MultiReplica& r : replicas) {
      if (std::find(bad.begin(), bad.end(), r.device) != bad.end()) {
        (void)r.robot.release();
        (void)r.sdf.release();
        continue;
      }
      (void)hipSetDevice(r.device);
      r.robot.reset();
      r.sdf.reset();
    }
  }
};

static int shard_error(const gpmp2mi_multi_plan* m, int k, int rc, const std::string& msg) {
  set_error("shard " + std::to_string(k) + " (device " + std::to_string(m->shards[k].device) + "): " + msg);
  return rc;
}
// contiguous split of `total` rows: the first total % n shards get one more (gpmp2_amd/sharding.py shard_range)
static void split_rows(int total, int n, std::vector<int>& row0, std::vector<int>& rows) {
  row0.assign(n, 0);
  rows.assign(n, 0);
  const int base = total / n, extra = total % n;
  for (int k = 0; k < n; k++) {
    row0[k] = k * base + std::min(k, extra);
    rows[k] = base + (k < extra ? 1 : 0);
  }
}

// fn(k) for every shard k with work[k]: shard 0 on the calling thread, the others on one std::thread each.  Each first
// makes its shard's device current (HIP's current device is per thread; a new thread starts on device 0).  The rc and
// message of every shard come back to this thread; the first failure in shard order is returned.
static int run_shards(gpmp2mi_multi_plan* m, const std::vector<char>& work, const std::function<int(int)>& fn) {
  const int n = (int)m->shards.size();
  std::vector<int> rc(n, GPMP2MI_OK);
  std::vector<std::string> msg(n);
  auto body = [&](int k) {
    const hipError_t e = hipSetDevice(m->shards[k].device);
    if (e != hipSuccess) {
      rc[k] = GPMP2MI_ERR_HIP;
      msg[k] = std::string("hipSetDevice: ") + hipGetErrorString(e);
      return;
    }
    rc[k] = fn(k);
    if (rc[k] != GPMP2MI_OK) msg[k] = last_error();
  };
  std::vector<std::thread> threads;
  for (int k = 1; k < n; k++) {
    if (!work[k]) continue;
    try {
      threads.emplace_back(body, k);
    } catch (const std::exception& ex) {
      rc[k] = GPMP2MI_ERR_HIP;
      msg[k] = std::string("cannot start a host thread: ") + ex.what();
    }
  }
  if (work[0]) body(0);
  for (std::thread& t : threads) t.join();
  for (const MultiShard& sh : m->shards)
    if (sh.poisoned()) m->poisoned = true;
  for (int k = 0; k < n; k++)
    if (rc[k] != GPMP2MI_OK) return shard_error(m, k, rc[k], msg[k]);
  return GPMP2MI_OK;
}

// f() with shard k's device current, for the calls that visit the shards in turn; a failure comes back as shard_error
template <class F>
static int on_shard(gpmp2mi_multi_plan* m, int k, F f) {
  if (hipSetDevice(m->shards[k].device) != hipSuccess) return shard_error(m, k, GPMP2MI_ERR_HIP, "hipSetDevice failed");
  const int rc = f();
  return rc == GPMP2MI_OK ? rc : shard_error(m, k, rc, last_error());
}

// A queue run over the shards, the one body of the plain and the seeded entry point: the split, the staging, the run, the
// drain after a failure and the statistics.  With `make_inits` the caller's `io.init` is null: only the four end arrays
// are uploaded, and make_inits(k, row0, stage, extra, stream) fills shard k's staged inits on its stream; `extra` is
// `extra_row` doubles a problem of further device staging (null when 0), freed with the rest.
using MakeInits = std::function<int(int, int, const QueueStage&, double*, hipStream_t)>;
static int multi_queue(gpmp2mi_multi_plan* m, const QueueRun& io, size_t extra_row, const MakeInits& make_inits) {
  const int n = (int)m->shards.size();
  std::vector<int> row0, rows;
  split_rows(io.M, n, row0, rows);
  std::vector<char> work(n);
  for (int k = 0; k < n; k++) work[k] = rows[k] > 0;
  DeviceGuard guard;
  // Staging for every shard with problems, allocated before any shard starts and freed after all have joined: hipFree
  // waits for the whole device, so it would stall the other shards there.  Leaked with a shard that timed out.
  struct StageSet {
    gpmp2mi_multi_plan* m;
    std::vector<QueueStage> st;
    std::vector<void*> extra;
    ~StageSet() {
      for (size_t k = 0; k < st.size(); k++) {
        if (m->shards[k].poisoned()) {
          st[k].leak();
          continue;
        }
        if ((st[k].base || extra[k]) && hipSetDevice(m->shards[k].device) == hipSuccess) {
          st[k].release();
          if (extra[k]) (void)hipFree(extra[k]);
        }
      }
    }
  } stage{m, std::vector<QueueStage>(n), std::vector<void*>(n, nullptr)};
  for (int k = 0; k < n; k++) {
    if (!work[k]) continue;
    G2_TRY(on_shard(m, k, [&]() -> int {
      G2_TRY(stage.st[k].alloc(rows[k], io, m->D, m->trow(), m->T));
      return extra_row ? dev_malloc(&stage.extra[k], rows[k] * extra_row * sizeof(double)) : GPMP2MI_OK;
    }));
  }
  m->problem_set = m->optimized = m->queue_ran = false;
  const int rc = run_shards(m, work, [&](int k) -> int {
    const QueueStage& g = stage.st[k];
    hipStream_t st = m->shards[k].stream;
    G2_TRY(g.upload(io, row0[k], st, !make_inits));
    if (make_inits) G2_TRY(make_inits(k, row0[k], g, (double*)stage.extra[k], st));
    G2_TRY(plan_optimize_queue(m->shards[k].plan, g.q, false, st));
    G2_TRY(g.download(io, row0[k], st));
    G2_HIP(hipStreamSynchronize(st));
    return GPMP2MI_OK;
  });
  if (rc != GPMP2MI_OK) {
    // a shard's stream may still hold copies if it failed half-way: wait for them before the staging is freed
    for (const MultiShard& sh : m->shards)
      if (!sh.poisoned()) (void)hipStreamSynchronize(sh.stream);
    return rc;
  }
  for (int k = 0; k < n; k++) m->shards[k].qstats = work[k] ? m->shards[k].plan->qstats : gpmp2mi_queue_stats{};
  m->queue_ran = true;
  return GPMP2MI_OK;
}

extern "C" {

int gpmp2mi_multi_plan_create(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, const gpmp2mi_settings* s,
                              const gpmp2mi_graph_opts* o, int B, int nshards, const int* devices,
                              gpmp2mi_multi_plan** out) {
  return gpmp2mi_debug_multi_plan_create(robot, sdf, s, o, B, nshards, devices, nullptr, 0, out);
}

int gpmp2mi_debug_multi_plan_create(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, const gpmp2mi_settings* s,
                                    const gpmp2mi_graph_opts* o, int B, int nshards, const int* devices,
                                    const gpmp2mi_debug_forms* forms, int replicate_all, gpmp2mi_multi_plan** out) {
  G2_CHECK(robot && sdf && s && devices && out, GPMP2MI_ERR_INVALID, "null argument");
  *out = nullptr;
  G2_CHECK(nshards >= 1 && nshards <= GPMP2MI_MAX_SHARDS, GPMP2MI_ERR_INVALID,
           "nshards must be in 1.." + std::to_string(GPMP2MI_MAX_SHARDS));
  G2_CHECK(B >= nshards, GPMP2MI_ERR_INVALID, "batch size must be >= nshards (every shard holds a row)");
  G2_TRY(ensure_device());
  const int ndev = gpmp2mi_device_count();
  for (int k = 0; k < nshards; k++)
    G2_CHECK(devices[k] >= 0 && devices[k] < ndev, GPMP2MI_ERR_INVALID,
             "shard " + std::to_string(k) + ": device id " + std::to_string(devices[k]) + " out of range (" +
                 std::to_string(ndev) + " devices)");
  DeviceGuard guard;
  auto m = std::make_unique<gpmp2mi_multi_plan>();   // its destructor releases whatever was built if anything fails
  m->B = B;
  m->D = robot->h.dof;
  m->N = s->total_step;
  m->T = s->max_iter + 1;
  m->src_sdf = sdf;
  std::vector<int> row0, rows;
  split_rows(B, nshards, row0, rows);
  m->shards.resize(nshards);
  for (int k = 0; k < nshards; k++) {
    MultiShard& sh = m->shards[k];
    const int dev = devices[k];
    sh.device = dev;
    sh.row0 = row0[k];
    sh.rows = rows[k];
    // one robot copy and one field copy per device that needs them, shared by that device's shards
    const bool own_robot = !replicate_all && robot->device == dev, own_sdf = !replicate_all && sdf->device == dev;
    MultiReplica* rep = nullptr;
    for (MultiReplica& r : m->replicas)
      if (r.device == dev) rep = &r;
    if (!rep && !(own_robot && own_sdf)) {
      m->replicas.emplace_back();
      rep = &m->replicas.back();
      rep->device = dev;
      int rc = own_robot ? GPMP2MI_OK : robot_replica(robot, dev, rep->robot);
      if (rc == GPMP2MI_OK && !own_sdf) rc = sdf_replica(sdf, dev, rep->sdf);
      if (rc != GPMP2MI_OK) return shard_error(m.get(), k, rc, last_error());
    }
    const gpmp2mi_robot* r_k = own_robot ? robot : rep->robot.get();
    const gpmp2mi_sdf* s_k = own_sdf ? sdf : rep->sdf.get();
    G2_TRY(on_shard(m.get(), k, [&] { return gpmp2mi_debug_plan_create(r_k, s_k, s, o, sh.rows, forms, &sh.plan); }));
    hipError_t e = hipStreamCreateWithFlags(&sh.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&sh.copied, hipEventDisableTiming);
    if (e != hipSuccess) return shard_error(m.get(), k, GPMP2MI_ERR_HIP, std::string("stream / event: ") + hipGetErrorString(e));
  }
  *out = m.release();
  return GPMP2MI_OK;
}

void gpmp2mi_multi_plan_destroy(gpmp2mi_multi_plan* m) { delete m; }

int gpmp2mi_multi_plan_shards(const gpmp2mi_multi_plan* m, int* nshards, int* devices, int* row_begin) {
  G2_CHECK(m, GPMP2MI_ERR_INVALID, "null multi plan");
  G2_CHECK(nshards, GPMP2MI_ERR_INVALID, "null argument");
  const int n = (int)m->shards.size();
  *nshards = n;
  for (int k = 0; k < n; k++) {
    if (devices) devices[k] = m->shards[k].device;
    if (row_begin) row_begin[k] = m->shards[k].row0;
  }
  if (row_begin) row_begin[n] = m->B;
  return GPMP2MI_OK;
}

// Live map (map.hip): the voxels of the caller's handle again to every copy this multi plan owns, by the steps of
// sdf_replica: a peer copy of `plain`, then the pack kernel on the copy's device.
int gpmp2mi_multi_plan_refresh_field(gpmp2mi_multi_plan* m) {
  G2_MULTI_LIVE(m);
  DeviceGuard guard;
  const gpmp2mi_sdf* src = m->src_sdf;
  const size_t bytes = (size_t)src->h.nx * src->h.ny * src->h.nz * sizeof(double);
  for (MultiReplica& r : m->replicas) {
    if (!r.sdf) continue;
    G2_HIP(hipSetDevice(r.device));
    G2_HIP(hipMemcpyPeer(r.sdf->plain, r.device, src->plain, src->device, bytes));
    G2_TRY(launch_sdf_pack(r.sdf->h, r.sdf->cells, nullptr));
  }
  for (MultiReplica& r : m->replicas) {
    if (!r.sdf) continue;
    G2_HIP(hipSetDevice(r.device));
    G2_HIP(hipStreamSynchronize(nullptr));
  }
  return GPMP2MI_OK;
}

int gpmp2mi_multi_plan_set_problem(gpmp2mi_multi_plan* m, const double* sc, const double* sv, const double* ec,
                                   const double* ev, const double* init) {
  G2_MULTI_LIVE(m);
  G2_CHECK(sc && sv && ec && ev && init, GPMP2MI_ERR_INVALID, "null argument");
  DeviceGuard guard;
  m->problem_set = m->optimized = false;
  for (int k = 0; k < (int)m->shards.size(); k++) {
    const MultiShard& sh = m->shards[k];
    const size_t d = (size_t)sh.row0 * m->D, t = sh.row0 * m->trow();
    G2_TRY(on_shard(m, k, [&] {
      return plan_set_problem(sh.plan, sc + d, sv + d, ec + d, ev + d, init + t, hipMemcpyHostToDevice, sh.stream);
    }));
  }
  m->problem_set = true;
  return GPMP2MI_OK;
}

int gpmp2mi_multi_plan_optimize(gpmp2mi_multi_plan* m) {
  G2_MULTI_LIVE(m);
  G2_CHECK(m->problem_set, GPMP2MI_ERR_INVALID, "call gpmp2mi_multi_plan_set_problem first");
  DeviceGuard guard;
  m->optimized = false;
  const std::vector<char> all(m->shards.size(), 1);
  G2_TRY(run_shards(m, all, [&](int k) { return gpmp2mi_plan_optimize(m->shards[k].plan, m->shards[k].stream); }));
  m->optimized = true;
  return GPMP2MI_OK;
}

int gpmp2mi_multi_plan_get_result(gpmp2mi_multi_plan* m, double* traj, int* iters, double* ferr, int* status,
                                  double* trace) {
  G2_MULTI_LIVE(m);
  G2_CHECK(m->optimized, GPMP2MI_ERR_INVALID, "multi plan has not been optimized");
  DeviceGuard guard;
  for (int k = 0; k < (int)m->shards.size(); k++) {
    const MultiShard& sh = m->shards[k];
    const size_t r = sh.row0;
    G2_TRY(on_shard(m, k, [&] {
      return plan_get_result(sh.plan, traj ? traj + r * m->trow() : nullptr, iters ? iters + r : nullptr,
                             ferr ? ferr + r : nullptr, status ? status + r : nullptr, trace ? trace + r * m->T : nullptr,
                             hipMemcpyDeviceToHost, sh.stream);
    }));
  }
  return GPMP2MI_OK;
}

int gpmp2mi_multi_plan_get_result_dev(gpmp2mi_multi_plan* m, int device, double* traj, int* iters, double* ferr,
                                      int* status, void* stream) {
  G2_MULTI_LIVE(m);
  G2_CHECK(m->optimized, GPMP2MI_ERR_INVALID, "multi plan has not been optimized");
  G2_CHECK(device >= 0 && device < gpmp2mi_device_count(), GPMP2MI_ERR_INVALID,
           "device id " + std::to_string(device) + " out of range");
  DeviceGuard guard;
  hipStream_t cs = (hipStream_t)stream;
  // the shards write the caller's buffers only after what the caller enqueued before this call
  G2_HIP(hipSetDevice(device));
  hipEvent_t entry = nullptr;
  for (auto& e : m->entry)
    if (e.first == device) entry = e.second;
  if (!entry) {
    G2_HIP(hipEventCreateWithFlags(&entry, hipEventDisableTiming));
    m->entry.push_back({device, entry});
  }
  G2_HIP(hipEventRecord(entry, cs));
  for (int k = 0; k < (int)m->shards.size(); k++) {
    MultiShard& sh = m->shards[k];
    const PlanBuffers& pb = sh.plan->pb;
    const size_t r = sh.row0;
    auto copy = [&](void* dst, const void* src, size_t bytes) -> int {
      if (sh.device == device) G2_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, sh.stream));
      else G2_HIP(hipMemcpyPeerAsync(dst, device, src, sh.device, bytes, sh.stream));
      return GPMP2MI_OK;
    };
    sh.plan->mark_dirty(sh.stream);
    G2_TRY(on_shard(m, k, [&]() -> int {
      G2_HIP(hipStreamWaitEvent(sh.stream, entry, 0));
      if (traj) G2_TRY(copy(traj + r * m->trow(), pb.result, sh.rows * m->trow() * sizeof(double)));
      if (iters) G2_TRY(copy(iters + r, pb.iters, sh.rows * sizeof(int)));
      if (ferr) G2_TRY(copy(ferr + r, pb.final_err, sh.rows * sizeof(double)));
      if (status) G2_TRY(copy(status + r, pb.status, sh.rows * sizeof(int)));
      G2_HIP(hipEventRecord(sh.copied, sh.stream));
      return GPMP2MI_OK;
    }));
  }
  G2_HIP(hipSetDevice(device));
  for (const MultiShard& sh : m->shards) G2_HIP(hipStreamWaitEvent(cs, sh.copied, 0));
  return GPMP2MI_OK;
}

int gpmp2mi_multi_plan_optimize_queue(gpmp2mi_multi_plan* m, int M, const double* sc, const double* sv,
                                      const double* ec, const double* ev, const double* init, double* traj, int* iters,
                                      double* ferr, int* status, double* trace) {
  G2_MULTI_LIVE(m);
  G2_CHECK(M >= 1, GPMP2MI_ERR_INVALID, "queue: M must be >= 1");
  G2_CHECK(sc && sv && ec && ev && init, GPMP2MI_ERR_INVALID, "queue: null input");
  return multi_queue(m, QueueRun{M, 0, sc, sv, ec, ev, init, traj, iters, ferr, status, trace}, 0, nullptr);
}

// The queue with its initial values made on the device (include/gpmp2mi.h "seeding"): shard k draws the problems
// first + row0 .. from the same function, so the rows are those of one plan.  The extra staging holds the rows of a
// caller's mean.
int gpmp2mi_multi_plan_optimize_queue_seeded(gpmp2mi_multi_plan* m, int M, uint64_t seed, int first, double scale,
                                             int keep_first, const double* sc, const double* sv, const double* ec,
                                             const double* ev, const double* mean, double* traj, int* iters, double* ferr,
                                             int* status, double* trace, double* init_out) {
  G2_MULTI_LIVE(m);
  G2_CHECK(sc && sv && ec && ev, GPMP2MI_ERR_INVALID, "queue: null input");
  G2_TRY(plan_seed_check(m->shards[0].plan, M, first, scale));   // the shards' plans share the setting and the robot
  const size_t trow = m->trow();
  return multi_queue(m, QueueRun{M, 0, sc, sv, ec, ev, nullptr, traj, iters, ferr, status, trace}, mean ? trow : 0,
                     [&](int k, int row0, const QueueStage& g, double* dmean, hipStream_t st) -> int {
                       const size_t bytes = (size_t)g.q.M * trow * sizeof(double);
                       if (mean) G2_HIP(hipMemcpyAsync(dmean, mean + row0 * trow, bytes, hipMemcpyHostToDevice, st));
                       G2_TRY(plan_seed_restarts(m->shards[k].plan, g.q.M, seed, first + row0, scale, keep_first,
                                                 g.q.start_conf, g.q.end_conf, dmean, (double*)g.q.init, st));
                       if (init_out) G2_HIP(hipMemcpyAsync(init_out + row0 * trow, g.q.init, bytes, hipMemcpyDeviceToHost, st));
                       return GPMP2MI_OK;
                     });
}

int gpmp2mi_multi_plan_queue_stats(const gpmp2mi_multi_plan* m, int shard, gpmp2mi_queue_stats* out) {
  G2_CHECK(m, GPMP2MI_ERR_INVALID, "null multi plan");
  G2_CHECK(out, GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK(shard >= 0 && shard < (int)m->shards.size(), GPMP2MI_ERR_INVALID, "shard index out of range");
  G2_CHECK(m->queue_ran, GPMP2MI_ERR_INVALID, "no queue run on this multi plan yet");
  *out = m->shards[shard].qstats;
  return GPMP2MI_OK;
}

// Scoring (score.hip): every shard scores its rows on its own device and stream, the outputs land in batch order.
int gpmp2mi_multi_plan_score(gpmp2mi_multi_plan* m, int inter_step, double* support_cost, double* dense_cost,
                             double* min_clearance, int* worst, int* out_of_range) {
  G2_MULTI_LIVE(m);
  G2_CHECK(m->optimized, GPMP2MI_ERR_INVALID, "multi plan has not been optimized");
  G2_CHECK(inter_step >= 0, GPMP2MI_ERR_INVALID, "inter_step must be >= 0");
  DeviceGuard guard;
  const std::vector<char> all(m->shards.size(), 1);
  return run_shards(m, all, [&](int k) {
    const MultiShard& sh = m->shards[k];
    const size_t r = sh.row0;
    ScoreOut o;
    o.support = support_cost ? support_cost + r : nullptr;
    o.dense = dense_cost ? dense_cost + r : nullptr;
    o.clearance = min_clearance ? min_clearance + r : nullptr;
    o.worst = worst ? worst + 2 * r : nullptr;
    o.oor = out_of_range ? out_of_range + r : nullptr;
    return plan_score(sh.plan, inter_step, o, nullptr, true, sh.stream);
  });
}

// Every shard selects among its rows; the pick over the shards' candidates is the same rule on the host: the smallest
// final_error, the lowest shard (= the lowest row) on ties.
int gpmp2mi_multi_plan_select(gpmp2mi_multi_plan* m, int inter_step, double required_clearance, int require_in_range,
                              int* best, int* n_eligible, double* traj_best, double* dense_best) {
  G2_MULTI_LIVE(m);
  G2_CHECK(m->optimized, GPMP2MI_ERR_INVALID, "multi plan has not been optimized");
  G2_CHECK(inter_step >= 0, GPMP2MI_ERR_INVALID, "inter_step must be >= 0");
  DeviceGuard guard;
  const int n = (int)m->shards.size();
  const size_t Md = (size_t)m->N * (inter_step + 1) + 1;
  std::vector<int> cand(n, -1), cnt(n, 0);
  std::vector<double> fe(n, 0.0);
  std::vector<std::vector<double>> tb(n), db(n);
  const std::vector<char> all(n, 1);
  G2_TRY(run_shards(m, all, [&](int k) -> int {
    const MultiShard& sh = m->shards[k];
    if (traj_best) tb[k].resize(m->trow());
    if (dense_best) db[k].resize(Md * 2 * m->D);
    ScoreSel sel;
    sel.required_clearance = required_clearance;
    sel.require_in_range = require_in_range;
    sel.best = &cand[k];
    sel.n_eligible = &cnt[k];
    sel.traj_best = traj_best ? tb[k].data() : nullptr;
    sel.dense_best = dense_best ? db[k].data() : nullptr;
    sel.best_error = &fe[k];
    return plan_score(sh.plan, inter_step, ScoreOut{}, &sel, true, sh.stream);
  }));
  int win = -1, total = 0;
  for (int k = 0; k < n; k++) {
    total += cnt[k];
    if (cand[k] >= 0 && (win < 0 || fe[k] < fe[win])) win = k;
  }
  if (best) *best = win < 0 ? -1 : m->shards[win].row0 + cand[win];
  if (n_eligible) *n_eligible = total;
  if (win >= 0) {
    if (traj_best) std::copy(tb[win].begin(), tb[win].end(), traj_best);
    if (dense_best) std::copy(db[win].begin(), db[win].end(), dense_best);
  }
  return GPMP2MI_OK;
}

}  // extern "C"
