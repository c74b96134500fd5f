// group.hip -- "distinct alternatives" (include/gpmp2mi.h): all-pairs trajectory distances, the leader rule on a given
// matrix (host and device), both in one enqueue over a bit matrix, and the plan form that scores, groups and copies one
// representative per mode.  Kernels: group_kernels.hip; the rule itself: group_rule.h; eligibility of the plan form
// comes from plan_score / plan_self_score (score.hip, self_score.hip), untouched.
#include <cmath>

#include "host.h"
#include "../group_rule.h"

using namespace g2;

namespace {

// the argument rules of the distance side; `w`: host array or null
int check_dist_args(int dof, int B, int total_step, const double* w, int metric) {
  G2_CHECK(dof >= 1 && dof <= GPMP2MI_MAX_DOF, GPMP2MI_ERR_INVALID, "dof must be in 1..GPMP2MI_MAX_DOF");
  G2_CHECK(B >= 0, GPMP2MI_ERR_INVALID, "B must be >= 0");
  G2_CHECK(total_step >= 1, GPMP2MI_ERR_INVALID, "total_step must be >= 1");
  G2_CHECK(metric == GPMP2MI_DIST_MAX_STATE || metric == GPMP2MI_DIST_RMS, GPMP2MI_ERR_INVALID, "unknown metric");
  if (w)
    for (int d = 0; d < dof; d++)
      G2_CHECK(std::isfinite(w[d]) && w[d] >= 0.0, GPMP2MI_ERR_INVALID, "a weight is negative or not finite");
  return GPMP2MI_OK;
}
int check_radius(double radius) {
  G2_CHECK(radius >= 0.0, GPMP2MI_ERR_INVALID, "radius must be >= 0 (NaN is refused)");
  return GPMP2MI_OK;
}
int check_rows(int B) {
  G2_CHECK(B <= GPMP2MI_MAX_GROUP_ROWS, GPMP2MI_ERR_UNSUPPORTED,
           "more than GPMP2MI_MAX_GROUP_ROWS = " + std::to_string(GPMP2MI_MAX_GROUP_ROWS) + " rows");
  return GPMP2MI_OK;
}

PairArgs pair_args(int dof, int B, int N, const double* traj, const double* w, int metric, double radius, double* dist,
                   unsigned long long* bits) {
  PairArgs a{};
  a.B = B;
  a.N = N;
  a.D = dof;
  a.metric = metric;
  a.traj = traj;
  for (int d = 0; d < GPMP2MI_MAX_DOF; d++) a.w[d] = (w && d < dof) ? w[d] : 1.0;
  a.radius = radius;
  a.dist = dist;
  a.bits = bits;
  return a;
}

struct DistinctArgs {
  int inter, require_in_range, metric, max_alt;
  double required_clearance, required_self_clearance, radius;
  const gpmp2mi_self_pairs* pairs;
  const double* weights;
  int *n_modes, *n_eligible, *alt, *alt_size, *mode;
  double *alt_error, *traj_alt, *dense_alt;
};

// host: the outputs are host arrays (staged in the plan's grouping workspace, copied back, `st` synchronised);
// otherwise device pointers, and the call returns without a host synchronisation
int plan_select_distinct(gpmp2mi_plan* p, const DistinctArgs& a, bool host, hipStream_t st) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_PLAN_LIVE(p);   // before anything is enqueued
  const PlanParams& P = p->hp;
  G2_CHECK(a.max_alt >= 1 && a.max_alt <= GPMP2MI_MAX_ALTERNATIVES, GPMP2MI_ERR_INVALID,
           "max_alt must be in 1..GPMP2MI_MAX_ALTERNATIVES");
  G2_TRY(check_dist_args(P.D, P.B, P.N, a.weights, a.metric));
  G2_TRY(check_radius(a.radius));
  G2_CHECK(p->optimized, GPMP2MI_ERR_INVALID, "plan has not been optimized");
  G2_TRY(check_score_args(a.inter, P.B, P.N, P.delta_t));
  G2_CHECK(p->robot->h.dof == P.D, GPMP2MI_ERR_INVALID, "robot dof does not fit the plan");
  G2_TRY(check_rows(P.B));
  const int Md = P.N * (a.inter + 1) + 1;
  const auto layout = [&](void* base) {
    return carve_group((char*)base, shape_of(p, a.inter), group_words(P.B), GPMP2MI_MAX_ALTERNATIVES, a.max_alt);
  };
  GroupWs w;
  G2_TRY(carve_into(p->ws[p->WS_GROUP], layout, &w));
  PriorRows got;   // eligibility: the scores of the existing stages, into the workspace
  G2_TRY(enqueue_prior_stages(p, a.pairs, a.inter, w.prior, st, &got));
  G2_TRY(launch_traj_pairs(pair_args(P.D, P.B, P.N, p->pb.result, a.weights, a.metric, a.radius, nullptr, w.bits), st));
  GroupRule r{};
  r.B = P.B;
  r.plan_rule = 1;
  r.require_in_range = a.require_in_range;
  r.radius = a.radius;
  r.required_clearance = a.required_clearance;
  r.required_self_clearance = a.required_self_clearance;
  r.bits = w.bits;
  r.score = p->pb.final_err;
  r.status = p->pb.status;
  r.clearance = got.clearance;
  r.oor = got.oor;
  r.self_clearance = got.self_clearance;
  r.self_invalid = got.self_invalid;
  r.mode = host ? w.mode : a.mode;
  r.leaders = w.leaders;
  r.sizes = w.sizes;
  r.n_modes = w.pick;
  r.n_eligible = w.pick + 1;
  G2_TRY(launch_group_rule(r, st));
  GroupCopy c{};
  c.N = P.N;
  c.D = P.D;
  c.lie = p->robot->h.kind >= GPMP2MI_ROBOT_POSE2_MOBILE_BASE;
  c.inter = a.inter;
  c.Md = Md;
  c.max_alt = a.max_alt;
  c.dt = P.delta_t;
  c.traj = p->pb.result;
  c.ferr = p->pb.final_err;
  c.leaders = w.leaders;
  c.sizes = w.sizes;
  c.n_modes = w.pick;
  c.n_eligible = w.pick + 1;
  c.alt = host ? w.alt : a.alt;
  c.alt_size = host ? w.alt_size : a.alt_size;
  c.alt_error = host ? w.alt_error : a.alt_error;
  c.traj_alt = host ? (a.traj_alt ? w.traj_alt : nullptr) : a.traj_alt;
  c.dense_alt = host ? (a.dense_alt ? w.dense_alt : nullptr) : a.dense_alt;
  c.out_n_modes = host ? nullptr : a.n_modes;
  c.out_n_eligible = host ? nullptr : a.n_eligible;
  G2_TRY(launch_group_copy(c, st));
  if (!host) return GPMP2MI_OK;
  const auto back = [&](void* dst, const void* src, size_t bytes) { return copy_back(dst, src, bytes, st); };
  int pick[2] = {0, 0};
  G2_TRY(back(pick, w.pick, sizeof(pick)));
  G2_TRY(back(a.alt, w.alt, a.max_alt * sizeof(int)));
  G2_TRY(back(a.alt_size, w.alt_size, a.max_alt * sizeof(int)));
  G2_TRY(back(a.mode, w.mode, P.B * sizeof(int)));
  G2_HIP(hipStreamSynchronize(st));
  if (a.n_modes) *a.n_modes = pick[0];
  if (a.n_eligible) *a.n_eligible = pick[1];
  const size_t k = (size_t)std::min(pick[0], a.max_alt);   // the slabs and errors beyond stay as they are
  if (k > 0 && (a.alt_error || a.traj_alt || a.dense_alt)) {
    G2_TRY(back(a.alt_error, w.alt_error, k * sizeof(double)));
    G2_TRY(back(a.traj_alt, w.traj_alt, k * (P.N + 1) * 2 * P.D * sizeof(double)));
    G2_TRY(back(a.dense_alt, w.dense_alt, k * Md * 2 * P.D * sizeof(double)));
    G2_HIP(hipStreamSynchronize(st));
  }
  p->mark_clean(st);
  return GPMP2MI_OK;
}

}  // namespace

extern "C" {

int gpmp2mi_traj_distances_dev(int dof, int B, int total_step, const double* traj, const double* weights, int metric,
                               double* dist, void* stream) {
  G2_CHECK(traj && dist, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_dist_args(dof, B, total_step, weights, metric));
  G2_TRY(check_rows(B));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  return launch_traj_pairs(pair_args(dof, B, total_step, traj, weights, metric, 0.0, dist, nullptr), (hipStream_t)stream);
}

int gpmp2mi_traj_distances(int dof, int B, int total_step, const double* traj, const double* weights, int metric,
                           double* dist) {
  G2_CHECK(traj && dist, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_dist_args(dof, B, total_step, weights, metric));
  G2_TRY(check_rows(B));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  DevBuf<double> dt, dd;
  G2_TRY(dt.upload(traj, (size_t)B * (total_step + 1) * 2 * dof));
  G2_TRY(dd.out(dist, (size_t)B * B));
  G2_TRY(gpmp2mi_traj_distances_dev(dof, B, total_step, dt.p, weights, metric, dd.p, nullptr));
  return fetch_all(dd);
}

int gpmp2mi_group_rows(int B, const double* dist, const double* score, const int* eligible, double radius, int* mode,
                       int* leaders, int* sizes, int* n_modes) {
  G2_CHECK(B >= 0, GPMP2MI_ERR_INVALID, "B must be >= 0");
  G2_CHECK(score && (dist || B == 0), GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_radius(radius));   // no row limit: that is the rule kernel's, and this form is a loop on the host
  std::vector<int> work((size_t)B);
  group_rule_host(B, score, eligible,
                  [&](int leader, int row) { return group_within(dist[(size_t)leader * B + row], radius); }, mode, leaders,
                  sizes, n_modes, work.data());
  return GPMP2MI_OK;
}

int gpmp2mi_group_rows_dev(int B, const double* dist, const double* score, const int* eligible, double radius, int* mode,
                           int* leaders, int* sizes, int* n_modes, void* stream) {
  G2_CHECK(B >= 0, GPMP2MI_ERR_INVALID, "B must be >= 0");
  G2_CHECK(score && (dist || B == 0), GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_radius(radius));
  G2_TRY(check_rows(B));
  G2_TRY(ensure_device());
  GroupRule r{};
  r.B = B;
  r.radius = radius;
  r.dist = dist;
  r.score = score;
  r.eligible = eligible;
  r.mode = mode;
  r.leaders = leaders;
  r.sizes = sizes;
  r.n_modes = n_modes;
  return launch_group_rule(r, (hipStream_t)stream);   // B = 0: the kernel writes n_modes = 0
}

int gpmp2mi_group_traj_dev(int dof, int B, int total_step, const double* traj, const double* weights, int metric,
                           double radius, const double* score, const int* eligible, int* mode, int* leaders, int* sizes,
                           int* n_modes, void* stream) {
  G2_CHECK(traj && score, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_dist_args(dof, B, total_step, weights, metric));
  G2_TRY(check_radius(radius));
  G2_TRY(check_rows(B));
  G2_TRY(ensure_device());
  // No handle to keep a workspace with: the bit matrix is allocated here and freed once the kernels are through, so
  // this form waits for `stream` once per call (include/gpmp2mi.h "distinct alternatives", Memory).
  DevBuf<unsigned long long> bits;
  G2_TRY(bits.alloc((size_t)B * group_words(B)));
  const hipStream_t st = (hipStream_t)stream;
  struct Wait {   // also on an error path: nothing may still use the bits when they go
    hipStream_t st;
    ~Wait() { (void)hipStreamSynchronize(st); }
  } wait{st};
  G2_TRY(launch_traj_pairs(pair_args(dof, B, total_step, traj, weights, metric, radius, nullptr, bits.p), st));
  GroupRule r{};
  r.B = B;
  r.radius = radius;
  r.bits = bits.p;
  r.score = score;
  r.eligible = eligible;
  r.mode = mode;
  r.leaders = leaders;
  r.sizes = sizes;
  r.n_modes = n_modes;
  return launch_group_rule(r, st);
}

int gpmp2mi_group_traj(int dof, int B, int total_step, const double* traj, const double* weights, int metric,
                       double radius, const double* score, const int* eligible, int* mode, int* leaders, int* sizes,
                       int* n_modes) {
  G2_CHECK(traj && score, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_dist_args(dof, B, total_step, weights, metric));
  G2_TRY(check_radius(radius));
  G2_TRY(check_rows(B));
  if (B == 0) {
    if (n_modes) *n_modes = 0;
    return GPMP2MI_OK;
  }
  G2_TRY(ensure_device());
  DevBuf<double> dt, ds;
  DevBuf<int> de, dm, dl, dz, dn;
  G2_TRY(dt.upload(traj, (size_t)B * (total_step + 1) * 2 * dof));
  G2_TRY(ds.upload(score, B));
  if (eligible) G2_TRY(de.upload(eligible, B));
  if (mode) G2_TRY(dm.out(mode, B));
  if (leaders) G2_TRY(dl.out(leaders, B));
  if (sizes) G2_TRY(dz.out(sizes, B));
  if (n_modes) G2_TRY(dn.out(n_modes, 1));
  G2_TRY(gpmp2mi_group_traj_dev(dof, B, total_step, dt.p, weights, metric, radius, ds.p, de.p, dm.p, dl.p, dz.p, dn.p,
                                nullptr));
  return fetch_all(dm, dl, dz, dn);
}

int gpmp2mi_plan_select_distinct(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                 const gpmp2mi_self_pairs* pairs, double required_self_clearance, int metric,
                                 const double* weights, double radius, int max_alt, int* n_modes, int* n_eligible,
                                 int* alt, int* alt_size, double* alt_error, int* mode, double* traj_alt,
                                 double* dense_alt) {
  const DistinctArgs a{inter_step, require_in_range, metric, max_alt, required_clearance, required_self_clearance, radius,
                       pairs, weights, n_modes, n_eligible, alt, alt_size, mode, alt_error, traj_alt, dense_alt};
  return plan_select_distinct(p, a, true, nullptr);
}
int gpmp2mi_plan_select_distinct_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                     const gpmp2mi_self_pairs* pairs, double required_self_clearance, int metric,
                                     const double* weights, double radius, int max_alt, int* n_modes, int* n_eligible,
                                     int* alt, int* alt_size, double* alt_error, int* mode, double* traj_alt,
                                     double* dense_alt, void* stream) {
  const DistinctArgs a{inter_step, require_in_range, metric, max_alt, required_clearance, required_self_clearance, radius,
                       pairs, weights, n_modes, n_eligible, alt, alt_size, mode, alt_error, traj_alt, dense_alt};
  return plan_select_distinct(p, a, false, (hipStream_t)stream);
}

}  // extern "C"
