// sampled.hip -- the sampled clearance (include/gpmp2mi.h "sampled clearance"): K joint draws of the configurations on
// the executed timeline per row through the collision check, for caller buffers and for a plan at its current estimate.
// The plan forms run linearize -> export -> factor-only k_posterior through plan_posterior_factor, then chunk after chunk
// on the one stream k_sample_seeded into a delta workspace the plan owns and the kernels of sample_clearance_kernels.hip;
// the optimizer's records, factors and estimate are not touched.  The two Cholesky factors of the bridge noise are formed
// here, on the host, once per (Qc, delta_t, inter_step).  The `_dev` forms enqueue and return.
#include <atomic>
#include <climits>
#include <cmath>

#include "host.h"

#include "../rng.h"

using namespace g2;

namespace {

constexpr int SAMPLED_MAX_N = TILE - 1;   // the limit of k_posterior: one tile per block
constexpr size_t SAMPLED_LP = (size_t)SAMPLED_MAX_INTER * (SAMPLED_MAX_INTER + 1) / 2;

std::atomic<size_t> g_chunk_bytes{0};   // gpmp2mi_debug_sampled_chunk_bytes; 0: SAMPLED_CHUNK_BYTES

int check_sampled_args(int inter, int B, int total_step, double delta_t, int K, int row_first, int sample_first,
                       double required) {
  G2_CHECK(inter >= 0, GPMP2MI_ERR_INVALID, "inter_step must be >= 0");
  G2_CHECK(B >= 0, GPMP2MI_ERR_INVALID, "B must be >= 0");
  G2_CHECK(total_step >= 1, GPMP2MI_ERR_INVALID, "total_step must be >= 1");
  G2_CHECK(delta_t > 0, GPMP2MI_ERR_INVALID, "delta_t must be > 0");
  G2_CHECK(K >= 1, GPMP2MI_ERR_INVALID, "sampled clearance: K must be >= 1");
  G2_CHECK(row_first >= 0 && sample_first >= 0 && sample_first <= INT_MAX - K && row_first <= INT_MAX - B,
           GPMP2MI_ERR_INVALID, "sampled clearance: row_first and sample_first must be >= 0 (and first + count an int)");
  G2_CHECK(!std::isnan(required), GPMP2MI_ERR_INVALID, "sampled clearance: required_clearance must not be NaN");
  G2_CHECK(inter <= SAMPLED_MAX_INTER, GPMP2MI_ERR_UNSUPPORTED,
           "sampled clearance: built for inter_step <= 63 (the bridge factor of an interval is held on chip)");
  const long long Md = (long long)total_step * (inter + 1) + 1;
  G2_CHECK(Md < (1ll << 31) / GPMP2MI_MAX_DOF && (long long)score_blocks((int)Md) * std::max(B, 1) < (1ll << 31),
           GPMP2MI_ERR_INVALID, "too many checked states for one launch");
  return GPMP2MI_OK;
}

const char* const POSE2_MSG =
    "sampled clearance: vector-space robots only (arm, point robot); the Pose2 robot kinds would need a bridge in the "
    "tangent space";

// the robot kinds k_sampled_clearance is instantiated for; refused before dispatch
int check_sampled_robot(const RobotDev& h) {
  G2_CHECK(h.kind < GPMP2MI_ROBOT_POSE2_MOBILE_BASE, GPMP2MI_ERR_UNSUPPORTED, POSE2_MSG);
  if (2 * h.dof > SAMPLED_MAX_N) {
    set_error("sampled clearance: built for blocks of one tile, 2 dof <= 15 (dof <= 7); this robot has dof " +
              std::to_string(h.dof));
    return GPMP2MI_ERR_UNSUPPORTED;
  }
  return GPMP2MI_OK;
}

// Row-wise Cholesky without pivoting, fp64: for each row a, for b = 0 .. a:  s = A[a][b] - sum_{k < b} L[a][k] L[b][k],
// L[a][b] = s / L[b][b] below the diagonal, sqrt(s) on it.  A and L packed by rows of the lower triangle (a (a+1) / 2 + b).
bool cholesky_packed(int n, const double* A, double* L) {
  for (int a = 0; a < n; a++)
    for (int b = 0; b <= a; b++) {
      double s = A[a * (a + 1) / 2 + b];
      for (int k = 0; k < b; k++) s -= L[a * (a + 1) / 2 + k] * L[b * (b + 1) / 2 + k];
      if (a == b) {
        if (!(s > 0.0) || !std::isfinite(s)) return false;
        L[a * (a + 1) / 2 + b] = std::sqrt(s);
      } else {
        L[a * (a + 1) / 2 + b] = s / L[b * (b + 1) / 2 + b];
      }
    }
  return true;
}

// host[0 .. J (J+1) / 2): Lp packed by rows; host[SAMPLED_LP .. + D D): C row-major, zero above the diagonal
int bridge_factors(const double* Qc, int D, double dt, int J, std::vector<double>& host) {
  host.assign(SAMPLED_LP + (size_t)D * D, 0.0);
  std::vector<double> P((size_t)J * (J + 1) / 2);
  const double d3 = dt * dt * dt;
  for (int a = 0; a < J; a++)
    for (int b = 0; b <= a; b++) {
      // s = tau_b <= t = tau_a, the tau of the kernels: j (Delta / (J + 1))
      const double t = (double)(a + 1) * (dt / (double)(J + 1)), s = (double)(b + 1) * (dt / (double)(J + 1));
      const double r = dt - t;
      P[(size_t)a * (a + 1) / 2 + b] = s * s * r * r * (3.0 * t * dt - s * dt - 2.0 * s * t) / (6.0 * d3);
    }
  G2_CHECK(cholesky_packed(J, P.data(), host.data()), GPMP2MI_ERR_INVALID,
           "sampled clearance: the bridge covariance of this delta_t / inter_step is not positive definite in fp64");
  std::vector<double> q((size_t)D * (D + 1) / 2), c(q.size());
  for (int a = 0; a < D; a++)
    for (int b = 0; b <= a; b++) q[(size_t)a * (a + 1) / 2 + b] = Qc ? Qc[a * D + b] : (a == b ? 1.0 : 0.0);
  G2_CHECK(cholesky_packed(D, q.data(), c.data()), GPMP2MI_ERR_INVALID,
           "sampled clearance: Qc must be symmetric positive definite");
  for (int a = 0; a < D; a++)
    for (int b = 0; b <= a; b++) host[SAMPLED_LP + (size_t)a * D + b] = c[(size_t)a * (a + 1) / 2 + b];
  return GPMP2MI_OK;
}

// Qc is SPD and the bridge covariance of (dt, J) factors in fp64: checked on the host before any device work
int check_factors(const double* Qc, int D, double dt, int J) {
  std::vector<double> host;
  return bridge_factors(Qc, D, dt, J, host);
}

// The factors of (Qc, dt, J) on the device: the entry of `f` that holds this key, or, for a new key, the oldest entry
// formed and uploaded again; only then the call waits for that copy on `st` (the host vector is the source).  A call
// whose key one of the handle's SAMPLED_FAC_KEYS entries holds neither copies nor waits.
int ensure_factors(SampledFac& f, const double* Qc, int D, double dt, int J, hipStream_t st, const double** dev) {
  const size_t nq = Qc ? (size_t)D * D : 0;
  for (const SampledFacEntry& x : f.e)
    if (x.dev && x.inter == J && x.dof == D && x.dt == dt && x.qc.size() == nq &&
        (nq == 0 || std::equal(x.qc.begin(), x.qc.end(), Qc))) {
      *dev = x.dev;
      return GPMP2MI_OK;
    }
  std::vector<double> host;
  G2_TRY(bridge_factors(Qc, D, dt, J, host));
  SampledFacEntry& x = f.e[f.next];
  if (!x.dev) G2_TRY(dev_malloc((void**)&x.dev, (SAMPLED_LP + (size_t)MAXD * MAXD) * sizeof(double)));
  x.inter = -1;   // until the copy has landed
  x.host.swap(host);
  G2_HIP(hipMemcpyAsync(x.dev, x.host.data(), x.host.size() * sizeof(double), hipMemcpyHostToDevice, st));
  G2_HIP(hipStreamSynchronize(st));
  if (nq) x.qc.assign(Qc, Qc + nq);
  else x.qc.clear();
  x.dt = dt;
  x.dof = D;
  x.inter = J;
  f.next = (f.next + 1) % SAMPLED_FAC_KEYS;
  *dev = x.dev;
  return GPMP2MI_OK;
}

struct SampledOut {
  int *hits = nullptr, *worst = nullptr, *state_hits = nullptr, *oor = nullptr;
  double *probability = nullptr, *clearance = nullptr, *state_clearance = nullptr, *conf = nullptr;
};

// the geometry of a call, filled once; s0 / cnt / delta / recs per chunk
SampledArgs sampled_args(double dt, int inter, int B, int N, int K, uint64_t seed, int row_first, int sample_first,
                         int bridge, double required, const double* est, const int* ok, const double* fac,
                         const SampledOut& o) {
  SampledArgs a{};
  a.dt = dt;
  a.required = required;
  a.seed = seed;
  a.inter = inter;
  a.B = B;
  a.N = N;
  a.Md = N * (inter + 1) + 1;
  a.nblk = score_blocks(a.Md);
  a.K = K;
  a.row_first = row_first;
  a.sample_first = sample_first;
  a.bridge = bridge != 0;
  a.est = est;
  a.ok = ok;
  a.Lp = fac;
  a.C = fac + SAMPLED_LP;
  a.state_clearance = o.state_clearance;
  a.state_hits = o.state_hits;
  a.conf = o.conf;
  return a;
}

// k_sampled_clearance over samples s0 .. s0 + cnt - 1 (delta [B][cnt][N+1][2D]) into `recs`, then k_sampled_finish
int enqueue_chunk(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, SampledArgs a, int s0, int cnt, const double* delta,
                  SampledRec* recs, int* acc, const SampledOut& o, hipStream_t st) {
  a.s0 = s0;
  a.cnt = cnt;
  a.delta = delta;
  a.recs = recs;
  G2_TRY(launch_sampled_clearance(r->h, r->d, s->h, a, st));
  SampledFinish f{};
  f.B = a.B;
  f.Md = a.Md;
  f.nblk = a.nblk;
  f.K = a.K;
  f.s0 = s0;
  f.cnt = cnt;
  f.first = s0 == 0;
  f.last = s0 + cnt == a.K;
  f.required = a.required;
  f.recs = recs;
  f.ok = a.ok;
  f.acc = acc;
  f.hits = o.hits;
  f.worst = o.worst;
  f.state_hits = o.state_hits;
  f.oor_samples = o.oor;
  f.probability = o.probability;
  f.clearance = o.clearance;
  return launch_sampled_finish(f, st);
}

// a plan's workspace for (B, N, n, inter) and a chunk of `chunk` samples: the delta chunk, its records, the carried
// counts, ok
struct PlanSampledWs {
  double* delta;
  SampledRec* recs;
  int *acc, *ok;
  size_t bytes;
};
PlanSampledWs sampled_ws_layout(char* base, const PlanParams& P, int inter, size_t chunk) {
  const size_t Md = (size_t)P.N * (inter + 1) + 1;
  PlanSampledWs w{};
  Carver take{base};
  w.delta = (double*)take((size_t)P.B * chunk * (P.N + 1) * P.n * sizeof(double));
  w.recs = (SampledRec*)take((size_t)P.B * chunk * score_blocks((int)Md) * sizeof(SampledRec));
  w.acc = (int*)take((size_t)2 * P.B * sizeof(int));
  w.ok = (int*)take(P.B * sizeof(int));
  w.bytes = take.off;
  return w;
}

// the largest multiple of 16 samples whose delta fits the byte budget (at least 16), no more than K needs
size_t chunk_samples(const PlanParams& P, int K) {
  const size_t budget = g_chunk_bytes.load() ? g_chunk_bytes.load() : SAMPLED_CHUNK_BYTES;
  const size_t per = (size_t)P.B * (P.N + 1) * P.n * sizeof(double);
  const size_t fit = std::max<size_t>(budget / per / 16 * 16, 16);
  const size_t most = std::min<size_t>(((size_t)K + 15) / 16 * 16, (size_t)65535 * SAMPLED_PER_WG / 16 * 16);
  return std::min(fit, most);
}

// what every plan call of this unit checks first; nothing is enqueued before it passes
int check_sampled_plan(gpmp2mi_plan* p, int inter, int K, int row_first, int sample_first, double required) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_CHECK(inter >= 0, GPMP2MI_ERR_INVALID, "inter_step must be >= 0");
  G2_PLAN_LIVE(p);
  if (p->hp.n > SAMPLED_MAX_N) {
    set_error("sampled clearance: built for blocks of one tile, 2 dof <= 15 (dof <= 7); this plan has dof " +
              std::to_string(p->hp.D));
    return GPMP2MI_ERR_UNSUPPORTED;
  }
  G2_CHECK(!p->hp.lie, GPMP2MI_ERR_UNSUPPORTED, POSE2_MSG);
  G2_TRY(check_sampled_args(inter, p->hp.B, p->hp.N, p->hp.delta_t, K, row_first, sample_first, required));
  G2_CHECK(p->problem_set, GPMP2MI_ERR_INVALID, "call gpmp2mi_plan_set_problem first");
  G2_CHECK(p->robot->h.dof == p->hp.D, GPMP2MI_ERR_INVALID, "robot dof does not fit the plan");
  return GPMP2MI_OK;
}

int plan_sampled_dev(gpmp2mi_plan* p, int inter, int K, uint64_t seed, int row_first, int sample_first, int bridge,
                     double required, const SampledOut& o, int* ok_out, hipStream_t st) {
  const PlanParams& P = p->hp;
  const int Md = P.N * (inter + 1) + 1;
  const double* bf = nullptr;
  G2_TRY(ensure_factors(p->sampled_fac, p->Qc.data(), P.D, P.delta_t, inter, st, &bf));
  const size_t chunk = chunk_samples(P, K);
  G2_TRY(p->ws[p->WS_SAMPLED].reserve(sampled_ws_layout(nullptr, P, inter, chunk).bytes));
  const PlanSampledWs w = sampled_ws_layout((char*)p->ws[p->WS_SAMPLED].p, P, inter, chunk);
  const double* fac = nullptr;
  G2_TRY(plan_posterior_factor(p, w.ok, &fac, st));   // marks `st` dirty
  if (ok_out) G2_HIP(hipMemcpyAsync(ok_out, w.ok, P.B * sizeof(int), hipMemcpyDeviceToDevice, st));
  if (o.state_hits) G2_HIP(hipMemsetAsync(o.state_hits, 0, (size_t)P.B * Md * sizeof(int), st));
  const double* est = p->optimized ? p->pb.result : p->pb.init;
  const SampledArgs a = sampled_args(P.delta_t, inter, P.B, P.N, K, seed, row_first, sample_first, bridge, required, est,
                                     w.ok, bf, o);
  for (int s0 = 0; s0 < K; s0 += (int)chunk) {
    const int cnt = std::min<int>((int)chunk, K - s0);
    SeedSampleArgs sa{};
    sa.seed = seed;
    sa.stream = RNG_STREAM_POSTERIOR;
    sa.nblk = P.N + 1;
    sa.count = cnt;
    sa.a_first = row_first;
    sa.b_first = sample_first + s0;
    sa.fac = fac;
    sa.out = w.delta;
    G2_TRY(launch_sample_seeded(P.B, P.n, false, sa, st));
    G2_TRY(enqueue_chunk(p->robot, p->sdf, a, s0, cnt, w.delta, w.recs, w.acc, o, st));
  }
  return GPMP2MI_OK;
}

// host arrays of a plan call: staged in DevBufs, the null stream, one synchronisation at the end
int plan_sampled_host(gpmp2mi_plan* p, int inter, int K, uint64_t seed, int row_first, int sample_first, int bridge,
                      double required, const SampledOut& out, int* ok) {
  const PlanParams& P = p->hp;
  const size_t Md = (size_t)P.N * (inter + 1) + 1, BK = (size_t)P.B * K;
  DevBuf<int> dh, dw, dsh, dor, dk;
  DevBuf<double> dp, dc, dsc, dcf;
  if (out.hits) G2_TRY(dh.out(out.hits, P.B));
  if (out.probability) G2_TRY(dp.out(out.probability, P.B));
  if (out.clearance) G2_TRY(dc.out(out.clearance, BK));
  if (out.worst) G2_TRY(dw.out(out.worst, 2 * BK));
  if (out.state_clearance) G2_TRY(dsc.out(out.state_clearance, BK * Md));
  if (out.state_hits) G2_TRY(dsh.out(out.state_hits, (size_t)P.B * Md));
  if (out.oor) G2_TRY(dor.out(out.oor, P.B));
  if (out.conf) G2_TRY(dcf.out(out.conf, BK * Md * P.D));
  if (ok) G2_TRY(dk.out(ok, P.B));
  SampledOut o;
  o.hits = dh.p; o.probability = dp.p; o.clearance = dc.p; o.worst = dw.p; o.state_clearance = dsc.p;
  o.state_hits = dsh.p; o.oor = dor.p; o.conf = dcf.p;
  G2_TRY(plan_sampled_dev(p, inter, K, seed, row_first, sample_first, bridge, required, o, dk.p, nullptr));
  G2_TRY(fetch_all(dh, dp, dc, dw, dsc, dsh, dor, dcf, dk));
  p->mark_clean(nullptr);
  return GPMP2MI_OK;
}

}  // namespace

extern "C" {

int gpmp2mi_sampled_clearance_traj_dev(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, const double* Qc, double delta_t,
                                       int inter_step, int B, int total_step, int K, const double* traj,
                                       const double* delta, const int* ok, uint64_t seed, int row_first, int sample_first,
                                       int bridge, double required_clearance, int* hits, double* probability,
                                       double* clearance, int* worst, double* state_clearance, int* state_hits,
                                       int* oor_samples, double* conf, void* stream) {
  G2_CHECK(r && s && traj && delta, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_sampled_args(inter_step, B, total_step, delta_t, K, row_first, sample_first, required_clearance));
  G2_TRY(check_sampled_robot(r->h));
  G2_TRY(check_factors(Qc, r->h.dof, delta_t, inter_step));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  int cur = -1;
  G2_HIP(hipGetDevice(&cur));
  G2_CHECK(cur == r->device, GPMP2MI_ERR_INVALID, "the robot handle lives on another device than the current one");
  hipStream_t st = (hipStream_t)stream;
  const int Md = total_step * (inter_step + 1) + 1;
  // the records share the robot handle's workspace with gpmp2mi_score_traj_dev, under its rule: calls in stream order
  std::lock_guard<std::mutex> lk(r->score_mu);
  const double* bf = nullptr;
  G2_TRY(ensure_factors(r->sampled_fac, Qc, r->h.dof, delta_t, inter_step, st, &bf));
  const size_t rec_bytes = ws_round((size_t)B * K * score_blocks(Md) * sizeof(SampledRec));
  G2_TRY(r->score_ws.reserve(rec_bytes + (size_t)2 * B * sizeof(int)));
  SampledOut o;
  o.hits = hits; o.probability = probability; o.clearance = clearance; o.worst = worst;
  o.state_clearance = state_clearance; o.state_hits = state_hits; o.oor = oor_samples; o.conf = conf;
  if (state_hits) G2_HIP(hipMemsetAsync(state_hits, 0, (size_t)B * Md * sizeof(int), st));
  const SampledArgs a = sampled_args(delta_t, inter_step, B, total_step, K, seed, row_first, sample_first, bridge,
                                     required_clearance, traj, ok, bf, o);
  return enqueue_chunk(r, s, a, 0, K, delta, (SampledRec*)r->score_ws.p, (int*)((char*)r->score_ws.p + rec_bytes), o, st);
}

int gpmp2mi_sampled_clearance_traj(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, const double* Qc, double delta_t,
                                   int inter_step, int B, int total_step, int K, const double* traj, const double* delta,
                                   const int* ok, uint64_t seed, int row_first, int sample_first, int bridge,
                                   double required_clearance, int* hits, double* probability, double* clearance,
                                   int* worst, double* state_clearance, int* state_hits, int* oor_samples, double* conf) {
  G2_CHECK(r && s && traj && delta, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_sampled_args(inter_step, B, total_step, delta_t, K, row_first, sample_first, required_clearance));
  G2_TRY(check_sampled_robot(r->h));
  G2_TRY(check_factors(Qc, r->h.dof, delta_t, inter_step));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const int D = r->h.dof;
  const size_t Md = (size_t)total_step * (inter_step + 1) + 1, BK = (size_t)B * K, trow = (size_t)(total_step + 1) * 2 * D;
  DevBuf<double> dt, dde, dp, dc, dsc, dcf;
  DevBuf<int> dk, dh, dw, dsh, dor;
  G2_TRY(dt.upload(traj, (size_t)B * trow));
  G2_TRY(dde.upload(delta, BK * trow));
  if (ok) G2_TRY(dk.upload(ok, B));
  if (hits) G2_TRY(dh.out(hits, B));
  if (probability) G2_TRY(dp.out(probability, B));
  if (clearance) G2_TRY(dc.out(clearance, BK));
  if (worst) G2_TRY(dw.out(worst, 2 * BK));
  if (state_clearance) G2_TRY(dsc.out(state_clearance, BK * Md));
  if (state_hits) G2_TRY(dsh.out(state_hits, (size_t)B * Md));
  if (oor_samples) G2_TRY(dor.out(oor_samples, B));
  if (conf) G2_TRY(dcf.out(conf, BK * Md * D));
  G2_TRY(gpmp2mi_sampled_clearance_traj_dev(r, s, Qc, delta_t, inter_step, B, total_step, K, dt.p, dde.p, dk.p, seed,
                                            row_first, sample_first, bridge, required_clearance, dh.p, dp.p, dc.p, dw.p,
                                            dsc.p, dsh.p, dor.p, dcf.p, nullptr));
  return fetch_all(dh, dp, dc, dw, dsc, dsh, dor, dcf);
}

int gpmp2mi_plan_collision_probability_dev(gpmp2mi_plan* p, int inter_step, int K, uint64_t seed, int row_first,
                                           int sample_first, int bridge, double required_clearance, int* hits,
                                           double* probability, double* clearance, int* worst, double* state_clearance,
                                           int* state_hits, int* oor_samples, int* ok, void* stream) {
  G2_TRY(check_sampled_plan(p, inter_step, K, row_first, sample_first, required_clearance));
  SampledOut o;
  o.hits = hits; o.probability = probability; o.clearance = clearance; o.worst = worst;
  o.state_clearance = state_clearance; o.state_hits = state_hits; o.oor = oor_samples;
  return plan_sampled_dev(p, inter_step, K, seed, row_first, sample_first, bridge, required_clearance, o, ok,
                          (hipStream_t)stream);
}

int gpmp2mi_plan_collision_probability(gpmp2mi_plan* p, int inter_step, int K, uint64_t seed, int row_first,
                                       int sample_first, int bridge, double required_clearance, int* hits,
                                       double* probability, double* clearance, int* worst, double* state_clearance,
                                       int* state_hits, int* oor_samples, int* ok) {
  G2_TRY(check_sampled_plan(p, inter_step, K, row_first, sample_first, required_clearance));
  SampledOut o;
  o.hits = hits; o.probability = probability; o.clearance = clearance; o.worst = worst;
  o.state_clearance = state_clearance; o.state_hits = state_hits; o.oor = oor_samples;
  return plan_sampled_host(p, inter_step, K, seed, row_first, sample_first, bridge, required_clearance, o, ok);
}

int gpmp2mi_plan_sample_dense_seeded_dev(gpmp2mi_plan* p, int inter_step, int K, uint64_t seed, int row_first,
                                         int sample_first, int bridge, double* conf, int* ok, void* stream) {
  G2_TRY(check_sampled_plan(p, inter_step, K, row_first, sample_first, 0.0));
  SampledOut o;
  o.conf = conf;
  return plan_sampled_dev(p, inter_step, K, seed, row_first, sample_first, bridge, 0.0, o, ok, (hipStream_t)stream);
}

int gpmp2mi_plan_sample_dense_seeded(gpmp2mi_plan* p, int inter_step, int K, uint64_t seed, int row_first,
                                     int sample_first, int bridge, double* conf, int* ok) {
  G2_TRY(check_sampled_plan(p, inter_step, K, row_first, sample_first, 0.0));
  SampledOut o;
  o.conf = conf;
  return plan_sampled_host(p, inter_step, K, seed, row_first, sample_first, bridge, 0.0, o, ok);
}

int gpmp2mi_debug_sampled_chunk_bytes(size_t bytes) {
  g_chunk_bytes.store(bytes);
  return GPMP2MI_OK;
}

}  // extern "C"
