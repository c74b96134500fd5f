// seed.hip -- seeding on the device (include/gpmp2mi.h "seeding"): normals of the counter function of rng.h, restart
// trajectories drawn from the plan's linear prior graph, and the seeded forms of the queue and of posterior sampling.
// The prior precision H_seed is built here on the host from the plan's parameters, uploaded and factored once per plan by
// a factor-only launch of k_posterior on one system, and kept with the plan; every seeded call afterwards is one launch
// of k_sample_seeded (seed_kernels.hip) in front of the unseeded path.  The `_dev` forms enqueue and return.
#include <climits>
#include <cmath>

#include "host.h"

#include "../rng.h"

using namespace g2;

namespace {

constexpr int SEED_MAX_N = TILE - 1;   // one tile per block, as k_posterior

// the plan's seeding workspace: H_seed, its factor scratch, the factorization's ok word
struct SeedWs {
  double *Hd, *Ho, *fac;
  int* ok;
  size_t bytes;
};
SeedWs seed_ws_layout(char* base, const PlanParams& P) {
  const size_t nb = (size_t)P.N + 1, nn = (size_t)P.n * P.n;
  SeedWs w{};
  Carver take{base};
  w.Hd = (double*)take(nb * nn * sizeof(double));
  w.Ho = (double*)take((size_t)P.N * nn * sizeof(double));
  w.fac = (double*)take(nb * 512 * sizeof(double));
  w.ok = (int*)take(sizeof(int));
  w.bytes = take.off;
  return w;
}

// H_seed of the plan's linear prior graph: PriorFactors on x_0, v_0, x_N, v_N and the N GaussianProcessPriorLinear
// factors, from the constant blocks the plan already holds (KA = Phi^T W Phi, KB = W, KO = -Phi^T W = block (i, i+1)).
// Hd [N+1][n][n], Ho [N][n][n] = block (i+1, i), the layouts of gpmp2mi_plan_linearize.
void build_seed_prior(const PlanParams& P, std::vector<double>& Hd, std::vector<double>& Ho) {
  const int n = P.n, D = P.D, N = P.N;
  const size_t nn = (size_t)n * n;
  Hd.assign((size_t)(N + 1) * nn, 0.0);
  Ho.assign((size_t)N * nn, 0.0);
  for (int i = 0; i <= N; i++)
    for (int r = 0; r < n; r++)
      for (int c = 0; c < n; c++) {
        double v = 0.0;
        if (i > 0) v += P.KB[r * n + c];
        if (i < N) v += P.KA[r * n + c];
        if ((i == 0 || i == N) && r == c) v += r < D ? P.conf_prior_w : P.vel_prior_w;
        Hd[(size_t)i * nn + r * n + c] = v;
        if (i < N) Ho[(size_t)i * nn + r * n + c] = P.KO[c * n + r];
      }
}

// what every seeded plan call checks first; nothing is enqueued before it passes
int check_seed_plan(gpmp2mi_plan* p) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_PLAN_LIVE(p);
  if (p->hp.n > SEED_MAX_N) {
    set_error("seeding: built for blocks of one tile, 2 dof <= 15 (dof <= 7); this plan has dof " + std::to_string(p->hp.D));
    return GPMP2MI_ERR_UNSUPPORTED;
  }
  G2_CHECK(!p->hp.lie, GPMP2MI_ERR_UNSUPPORTED,
           "seeding: vector-space robots only (arm, point robot); the Pose2 robot kinds would need a bridge in the "
           "tangent space");
  return GPMP2MI_OK;
}

int check_restart_args(int M, int first, double scale) {
  G2_CHECK(M >= 1, GPMP2MI_ERR_INVALID, "seeding: M must be >= 1");
  G2_CHECK(first >= 0 && first <= INT_MAX - M, GPMP2MI_ERR_INVALID, "seeding: first must be >= 0 (and first + M an int)");
  G2_CHECK(std::isfinite(scale) && scale >= 0.0, GPMP2MI_ERR_INVALID, "seeding: scale must be finite and >= 0");
  return GPMP2MI_OK;
}

// H_seed on the host (first use), then on the device with its factors (first use on a device path)
void ensure_seed_host(gpmp2mi_plan* p) {
  if (p->seed_Hd.empty()) build_seed_prior(p->hp, p->seed_Hd, p->seed_Ho);
}
int ensure_seed_prior(gpmp2mi_plan* p, hipStream_t st) {
  if (p->seed_ready) return GPMP2MI_OK;
  const PlanParams& P = p->hp;
  ensure_seed_host(p);
  G2_TRY(p->ws[p->WS_SEED].reserve(seed_ws_layout(nullptr, P).bytes));
  const SeedWs w = seed_ws_layout((char*)p->ws[p->WS_SEED].p, P);
  G2_HIP(hipMemcpyAsync(w.Hd, p->seed_Hd.data(), p->seed_Hd.size() * sizeof(double), hipMemcpyHostToDevice, st));
  G2_HIP(hipMemcpyAsync(w.Ho, p->seed_Ho.data(), p->seed_Ho.size() * sizeof(double), hipMemcpyHostToDevice, st));
  const PosteriorArgs a{P.N + 1, 0, w.Hd, w.Ho, nullptr, nullptr, nullptr, nullptr, w.ok, w.fac};
  G2_TRY(launch_posterior(1, P.n, a, st));
  // once per plan: the factors are read by every later call on whatever stream it names, so they are complete -- and
  // known to exist -- before the first of them is enqueued
  int ok = 0;
  G2_HIP(hipMemcpyAsync(&ok, w.ok, sizeof(int), hipMemcpyDeviceToHost, st));
  G2_HIP(hipStreamSynchronize(st));
  G2_CHECK(ok == 1, GPMP2MI_ERR_INVALID, "seeding: the prior precision of this plan is not positive definite");
  p->seed_ready = true;
  return GPMP2MI_OK;
}

// raw device memory that goes with a poisoned plan instead of waiting for it
struct DevMem {
  void* p = nullptr;
  ~DevMem() { if (p) (void)hipFree(p); }
  void leak() { p = nullptr; }
};

int plan_posterior_seeded(gpmp2mi_plan* p, int K, uint64_t seed, int row_first, int sample_first, double* delta, int* ok,
                          hipStream_t st) {
  const PlanParams& P = p->hp;
  const double* fac = nullptr;
  G2_TRY(plan_posterior_factor(p, ok, &fac, st));
  SeedSampleArgs a{};
  a.seed = seed;
  a.stream = RNG_STREAM_POSTERIOR;
  a.nblk = P.N + 1;
  a.count = K;
  a.a_first = row_first;
  a.b_first = sample_first;
  a.fac = fac;
  a.out = delta;
  return launch_sample_seeded(P.B, P.n, false, a, st);
}

int check_posterior_args(gpmp2mi_plan* p, int K, int row_first, int sample_first, const double* delta) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_CHECK(K >= 1 && delta, GPMP2MI_ERR_INVALID, "seeding: K must be >= 1, delta not null");
  G2_CHECK(row_first >= 0 && sample_first >= 0 && sample_first <= INT_MAX - K && row_first <= INT_MAX - p->hp.B,
           GPMP2MI_ERR_INVALID, "seeding: row_first and sample_first must be >= 0");
  G2_TRY(check_seed_plan(p));
  G2_CHECK(p->problem_set, GPMP2MI_ERR_INVALID, "call gpmp2mi_plan_set_problem first");
  return GPMP2MI_OK;
}

int check_fill_args(int stream, int a_first, int a_count, int b_first, int b_count, int nblk, int n, const double* out) {
  G2_CHECK(stream >= 0 && (uint32_t)stream <= RNG_STREAM_MAX, GPMP2MI_ERR_INVALID, "normal_fill: stream must be 0 .. 2^24 - 1");
  G2_CHECK(a_first >= 0 && b_first >= 0 && a_count >= 0 && b_count >= 0 && nblk >= 0, GPMP2MI_ERR_INVALID,
           "normal_fill: indices and counts must be >= 0");
  G2_CHECK(a_first <= INT_MAX - a_count && b_first <= INT_MAX - b_count, GPMP2MI_ERR_INVALID,
           "normal_fill: first + count must be an int");
  G2_CHECK(n >= 1 && n <= TILE, GPMP2MI_ERR_INVALID, "normal_fill: n must be 1..16 (the coordinates of one block)");
  G2_CHECK(out, GPMP2MI_ERR_INVALID, "null argument");
  return GPMP2MI_OK;
}

}  // namespace

// `sc`, `ec`, `mean`, `init` are device pointers; everything is enqueued on `st`
int g2::plan_seed_restarts(gpmp2mi_plan* p, int M, uint64_t seed, int first, double scale, int keep_first,
                           const double* sc, const double* ec, const double* mean, double* init, hipStream_t st) {
  const PlanParams& P = p->hp;
  G2_TRY(ensure_seed_prior(p, st));
  p->mark_dirty(st);
  SeedSampleArgs a{};
  a.seed = seed;
  a.stream = RNG_STREAM_RESTARTS;
  a.nblk = P.N + 1;
  a.count = M;
  a.a_first = first;
  a.fac = seed_ws_layout((char*)p->ws[p->WS_SEED].p, P).fac;
  a.out = init;
  a.scale = scale;
  a.keep_first = keep_first ? 1 : 0;
  a.D = P.D;
  a.mean = mean;
  a.start_conf = sc;
  a.end_conf = ec;
  return launch_sample_seeded(1, P.n, true, a, st);
}

int g2::plan_seed_check(gpmp2mi_plan* p, int M, int first, double scale) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_TRY(check_restart_args(M, first, scale));
  return check_seed_plan(p);
}

extern "C" {

int gpmp2mi_normal_fill_dev(uint64_t seed, int stream, int a_first, int a_count, int b_first, int b_count, int nblk, int n,
                            double* out, void* hip_stream) {
  G2_TRY(check_fill_args(stream, a_first, a_count, b_first, b_count, nblk, n, out));
  const NormalFillArgs a{seed, (uint32_t)stream, a_first, a_count, b_first, b_count, nblk, n, out};
  return launch_normal_fill(a, (hipStream_t)hip_stream);
}
int gpmp2mi_normal_fill(uint64_t seed, int stream, int a_first, int a_count, int b_first, int b_count, int nblk, int n,
                        double* out) {
  G2_TRY(check_fill_args(stream, a_first, a_count, b_first, b_count, nblk, n, out));
  const size_t count = (size_t)a_count * b_count * nblk * n;
  if (count == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  DevBuf<double> d;
  G2_TRY(d.out(out, count));
  G2_TRY(gpmp2mi_normal_fill_dev(seed, stream, a_first, a_count, b_first, b_count, nblk, n, d.p, nullptr));
  return fetch_all(d);
}

int gpmp2mi_plan_seed_restarts_dev(gpmp2mi_plan* p, int M, uint64_t seed, int first, double scale, int keep_first,
                                   const double* start_conf, const double* end_conf, const double* mean, double* init,
                                   void* stream) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_CHECK(init && (mean || (start_conf && end_conf)), GPMP2MI_ERR_INVALID,
           "seeding: init, and start_conf / end_conf unless a mean is given, must not be null");
  G2_TRY(plan_seed_check(p, M, first, scale));
  return plan_seed_restarts(p, M, seed, first, scale, keep_first, start_conf, end_conf, mean, init, (hipStream_t)stream);
}
int gpmp2mi_plan_seed_restarts(gpmp2mi_plan* p, int M, uint64_t seed, int first, double scale, int keep_first,
                               const double* start_conf, const double* end_conf, const double* mean, double* init) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_CHECK(init && (mean || (start_conf && end_conf)), GPMP2MI_ERR_INVALID,
           "seeding: init, and start_conf / end_conf unless a mean is given, must not be null");
  G2_TRY(plan_seed_check(p, M, first, scale));
  const size_t md = (size_t)M * p->hp.D, mt = (size_t)M * (p->hp.N + 1) * p->hp.n;
  DevBuf<double> dsc, dec, dm, di;
  if (!mean) {
    G2_TRY(dsc.upload(start_conf, md));
    G2_TRY(dec.upload(end_conf, md));
  } else {
    G2_TRY(dm.upload(mean, mt));
  }
  G2_TRY(di.out(init, mt));
  G2_TRY(plan_seed_restarts(p, M, seed, first, scale, keep_first, dsc.p, dec.p, dm.p, di.p, nullptr));
  G2_TRY(fetch_all(di));
  p->mark_clean(nullptr);
  return GPMP2MI_OK;
}

int gpmp2mi_plan_optimize_queue_seeded_dev(gpmp2mi_plan* p, int M, uint64_t seed, int first, double scale, int keep_first,
                                           const double* start_conf, const double* start_vel, const double* end_conf,
                                           const double* end_vel, const double* mean, double* traj, int* iters,
                                           double* final_error, int* status, double* error_trace, double* init_out,
                                           void* stream) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_CHECK(start_conf && start_vel && end_conf && end_vel, GPMP2MI_ERR_INVALID, "queue: null input");
  G2_TRY(plan_seed_check(p, M, first, scale));
  hipStream_t st = (hipStream_t)stream;
  DevMem own;   // the inits, when the caller does not want them
  double* init = init_out;
  if (!init) {
    G2_TRY(dev_malloc(&own.p, (size_t)M * (p->hp.N + 1) * p->hp.n * sizeof(double)));
    init = (double*)own.p;
  }
  G2_TRY(plan_seed_restarts(p, M, seed, first, scale, keep_first, start_conf, end_conf, mean, init, st));
  const QueueRun io{M, 0, start_conf, start_vel, end_conf, end_vel, init, traj, iters, final_error, status, error_trace};
  const int rc = plan_optimize_queue(p, io, false, st);   // returns with the queue drained
  if (p->poisoned) own.leak();
  return rc;
}

int gpmp2mi_plan_optimize_queue_seeded(gpmp2mi_plan* p, int M, uint64_t seed, int first, double scale, int keep_first,
                                       const double* start_conf, const double* start_vel, const double* end_conf,
                                       const double* end_vel, const double* mean, double* traj, int* iters,
                                       double* final_error, int* status, double* error_trace, double* init_out) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_CHECK(start_conf && start_vel && end_conf && end_vel, GPMP2MI_ERR_INVALID, "queue: null input");
  G2_TRY(plan_seed_check(p, M, first, scale));
  const PlanParams& P = p->hp;
  const size_t trow = (size_t)(P.N + 1) * P.n;
  const QueueRun io{M, 0, start_conf, start_vel, end_conf, end_vel, nullptr, traj, iters, final_error, status, error_trace};
  QueueStage stage;
  DevMem dmean;
  G2_TRY(stage.alloc(M, io, P.D, trow, P.rules.max_iter + 1));
  G2_TRY(stage.upload(io, 0, nullptr, false));   // the four end arrays; the inits are made on the device
  if (mean) {
    G2_TRY(dev_malloc(&dmean.p, M * trow * sizeof(double)));
    G2_HIP(hipMemcpyAsync(dmean.p, mean, M * trow * sizeof(double), hipMemcpyHostToDevice, nullptr));
  }
  int rc = plan_seed_restarts(p, M, seed, first, scale, keep_first, stage.q.start_conf, stage.q.end_conf,
                              (const double*)dmean.p, (double*)stage.q.init, nullptr);
  if (rc == GPMP2MI_OK) rc = plan_optimize_queue(p, stage.q, false, nullptr);
  if (p->poisoned) {   // a hung kernel may still write the staging: it goes with the plan
    stage.leak();
    dmean.leak();
    return rc;
  }
  if (rc == GPMP2MI_OK) rc = stage.download(io, 0, nullptr);
  if (rc == GPMP2MI_OK && init_out)
    G2_HIP(hipMemcpyAsync(init_out, stage.q.init, M * trow * sizeof(double), hipMemcpyDeviceToHost, nullptr));
  G2_HIP(hipStreamSynchronize(nullptr));
  return rc;
}

int gpmp2mi_plan_sample_posterior_seeded_dev(gpmp2mi_plan* p, int K, uint64_t seed, int row_first, int sample_first,
                                             double* delta, int* ok, void* stream) {
  G2_TRY(check_posterior_args(p, K, row_first, sample_first, delta));
  return plan_posterior_seeded(p, K, seed, row_first, sample_first, delta, ok, (hipStream_t)stream);
}
int gpmp2mi_plan_sample_posterior_seeded(gpmp2mi_plan* p, int K, uint64_t seed, int row_first, int sample_first,
                                         double* delta, int* ok) {
  G2_TRY(check_posterior_args(p, K, row_first, sample_first, delta));
  const PlanParams& P = p->hp;
  DevBuf<double> dde;
  DevBuf<int> dk;
  G2_TRY(dde.out(delta, (size_t)P.B * K * (P.N + 1) * P.n));
  if (ok) G2_TRY(dk.out(ok, P.B));
  G2_TRY(plan_posterior_seeded(p, K, seed, row_first, sample_first, dde.p, dk.p, nullptr));
  G2_TRY(fetch_all(dde, dk));
  p->mark_clean(nullptr);
  return GPMP2MI_OK;
}

int gpmp2mi_debug_plan_seed_prior(gpmp2mi_plan* p, double* Hdiag, double* Hoff) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_TRY(check_seed_plan(p));
  ensure_seed_host(p);
  if (Hdiag) std::copy(p->seed_Hd.begin(), p->seed_Hd.end(), Hdiag);
  if (Hoff) std::copy(p->seed_Ho.begin(), p->seed_Ho.end(), Hoff);
  return GPMP2MI_OK;
}

}  // extern "C"
