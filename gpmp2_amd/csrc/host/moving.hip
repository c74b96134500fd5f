// moving.hip -- moving obstacles (include/gpmp2mi.h "moving obstacles"): the plan's sphere set, the factor-level entry
// point, the check of the executed trajectory for caller buffers and for a plan's resident result, and the selection
// that asks for the moving clearance as well.  Kernels: moving_kernels.hip; the factor inside a plan is launched by
// plan_linearize (plan_run.hip).  The obstacle and self-collision sides of select_moving are the existing stages
// (plan_score, plan_self_score), enqueued ahead with their per-row outputs in this unit's workspace.
#include <cmath>

#include "host.h"

using namespace g2;

namespace {

// the rules of check_score_args, then the launch limits of this stage (the tile of the self check, Md S K pairs per row)
int check_moving_args(const gpmp2mi_robot* r, int K, int inter, int B, int total_step, double delta_t) {
  G2_TRY(check_score_args(inter, B, total_step, delta_t));
  const int S = r->h.nr_spheres;
  const long long Md = (long long)total_step * (inter + 1) + 1;
  G2_CHECK((long long)self_blocks((int)Md, S) * std::max(B, 1) < (1ll << 31) && Md * std::max(S * K, 1) < (1ll << 31),
           GPMP2MI_ERR_INVALID, "too many checked (state, sphere, moving sphere)s for one launch");
  return GPMP2MI_OK;
}

int check_set_args(int K, int cap, const double* radius, const double* centers) {
  G2_CHECK(K >= 0 && K <= cap, GPMP2MI_ERR_INVALID, "K < 0 or more moving spheres than there is room for");
  G2_CHECK(K == 0 || (radius && centers), GPMP2MI_ERR_INVALID, "null radius / centers with K > 0");
  return GPMP2MI_OK;
}

int set_moving(gpmp2mi_plan* p, int K, const double* radius, const double* centers, bool host, hipStream_t st) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_TRY(check_set_args(K, GPMP2MI_MAX_MOVING_SPHERES, radius, centers));   // what needs no look at the plan
  G2_CHECK(K <= p->ex.mv_cap, GPMP2MI_ERR_INVALID, "more moving spheres than the plan was created with room for");
  const size_t nc = (size_t)K * (p->hp.N + 1) * 3;
  if (host) {
    for (int k = 0; k < K; k++)
      G2_CHECK(std::isfinite(radius[k]) && radius[k] >= 0, GPMP2MI_ERR_INVALID, "a radius is negative or not finite");
    for (size_t i = 0; i < nc; i++) G2_CHECK(std::isfinite(centers[i]), GPMP2MI_ERR_INVALID, "a centre is not finite");
  }
  G2_PLAN_LIVE(p);
  if (K > 0) {
    PlanExtras& ex = p->ex;
    if (host) {
      G2_HIP(hipMemcpy(ex.mv_radius, radius, K * sizeof(double), hipMemcpyHostToDevice));
      G2_HIP(hipMemcpy(ex.mv_centers, centers, nc * sizeof(double), hipMemcpyHostToDevice));
    } else {
      p->mark_dirty(st);
      G2_HIP(hipMemcpyAsync(ex.mv_radius, radius, K * sizeof(double), hipMemcpyDeviceToDevice, st));
      G2_HIP(hipMemcpyAsync(ex.mv_centers, centers, nc * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
  }
  p->ex.mv_K = K;
  return GPMP2MI_OK;
}

struct MovingSel : ScoreSel {
  double required_self_clearance = 0.0, required_moving_clearance = 0.0;
  const gpmp2mi_self_pairs* pairs = nullptr;
};

// Layout of a plan's moving workspace for (B, N, D, S, inter): the records, the per-row scores of the existing stages,
// then the staging of the host-pointer forms
struct PlanMovingWs {
  ScoreRec* recs;
  double *clearance, *self_clearance;
  int *oor, *self_invalid;
  ScoreOut out;   // worst: [B][3]
  int* pick;      // best, n_eligible, then (8-byte aligned) the chosen row's final_error: one 16-byte copy
  double *traj_best, *dense_best;
  size_t bytes;
};
PlanMovingWs plan_ws_layout(char* base, int B, int N, int D, int S, int inter) {
  const size_t Md = (size_t)N * (inter + 1) + 1;
  PlanMovingWs w{};
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base + off;
    off += ws_round(bytes);
    return p;
  };
  w.recs = (ScoreRec*)take((size_t)B * self_blocks((int)Md, S) * sizeof(ScoreRec));
  w.clearance = (double*)take(B * sizeof(double));
  w.self_clearance = (double*)take(B * sizeof(double));
  w.oor = (int*)take(B * sizeof(int));
  w.self_invalid = (int*)take(B * sizeof(int));
  w.out.support = (double*)take(B * sizeof(double));
  w.out.dense = (double*)take(B * sizeof(double));
  w.out.clearance = (double*)take(B * sizeof(double));
  w.out.worst = (int*)take((size_t)3 * B * sizeof(int));
  w.out.oor = (int*)take(B * sizeof(int));
  w.pick = (int*)take(2 * sizeof(int) + sizeof(double));
  w.traj_best = (double*)take((size_t)(N + 1) * 2 * D * sizeof(double));
  w.dense_best = (double*)take(Md * 2 * D * sizeof(double));
  w.bytes = off;
  return w;
}

// Scores the plan's resident result against its resident set on `st`; sel != null: the existing stages for the same
// rows first, then the extended rule and the copy of the chosen row.  host / out / sel as plan_score (score.hip);
// out.oor: invalid.
int plan_moving(gpmp2mi_plan* p, int inter, const ScoreOut& out, const MovingSel* sel, bool host, hipStream_t st) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_CHECK(p->ex.mv_cap > 0, GPMP2MI_ERR_INVALID, "the plan was created without room for moving spheres");
  G2_PLAN_LIVE(p);   // before anything is enqueued
  G2_CHECK(p->optimized, GPMP2MI_ERR_INVALID, "plan has not been optimized");
  const PlanParams& P = p->hp;
  const PlanExtras& ex = p->ex;
  G2_CHECK(p->robot->h.dof == P.D, GPMP2MI_ERR_INVALID, "robot dof does not fit the plan");
  G2_TRY(check_moving_args(p->robot, ex.mv_K, inter, P.B, P.N, P.delta_t));
  const int S = p->robot->h.nr_spheres;
  G2_TRY(ws_reserve(&p->moving_ws, &p->moving_ws_bytes, plan_ws_layout(nullptr, P.B, P.N, P.D, S, inter).bytes));
  const PlanMovingWs w = plan_ws_layout((char*)p->moving_ws, P.B, P.N, P.D, S, inter);
  const size_t Md = (size_t)P.N * (inter + 1) + 1;
  MovingFinish f{};
  const ScoreOut& o = host ? w.out : out;
  // the host form computes only what the caller asked for
  f.support = (!host || out.support) ? o.support : nullptr;
  f.dense = (!host || out.dense) ? o.dense : nullptr;
  f.min_clearance = (!host || out.clearance) ? o.clearance : nullptr;
  f.worst = (!host || out.worst) ? o.worst : nullptr;
  f.invalid = (!host || out.oor) ? o.oor : nullptr;
  f.recs = w.recs;
  f.nblk = self_blocks((int)Md, S);
  f.K = ex.mv_K;
  ScoreFinish& g = f.sel;
  g.B = P.B;
  g.N = P.N;
  g.D = P.D;
  g.lie = p->robot->h.kind >= GPMP2MI_ROBOT_POSE2_MOBILE_BASE;
  g.inter = inter;
  g.Md = (int)Md;
  g.dt = P.delta_t;
  g.traj = p->pb.result;
  if (sel) {
    g.select = 1;
    g.required_clearance = sel->required_clearance;
    g.require_in_range = sel->require_in_range;
    f.required_self_clearance = sel->required_self_clearance;
    f.required_moving_clearance = sel->required_moving_clearance;
    g.ferr = p->pb.final_err;
    g.status = p->pb.status;
    g.best = host ? w.pick : sel->best;
    g.n_eligible = host ? w.pick + 1 : sel->n_eligible;
    g.best_err = host ? (double*)(w.pick + 2) : nullptr;
    g.traj_best = host ? (sel->traj_best ? w.traj_best : nullptr) : sel->traj_best;
    g.dense_best = host ? (sel->dense_best ? w.dense_best : nullptr) : sel->dense_best;
    // the per-row scores of the existing stages, into the workspace.  The self check goes first: it is the one that
    // can still refuse (a table made for another robot), and a refused call enqueues nothing.
    if (sel->pairs) {
      ScoreOut so;
      so.clearance = w.self_clearance;
      so.oor = w.self_invalid;
      G2_TRY(plan_self_score(p, sel->pairs, inter, so, nullptr, false, st));
      f.self_clearance = w.self_clearance;
      f.self_invalid = w.self_invalid;
    }
    ScoreOut so;
    so.clearance = w.clearance;
    so.oor = w.oor;
    G2_TRY(plan_score(p, inter, so, nullptr, false, st));
    f.clearance = w.clearance;
    f.oor = w.oor;
  }
  p->mark_dirty(st);
  G2_TRY(launch_moving_clearance(p->robot->h, p->robot->d, ex.mv_K, ex.mv_radius, ex.mv_centers, ex.mv_eps, P.delta_t, inter,
                                 P.B, P.N, p->pb.result, w.recs, st));
  G2_TRY(launch_moving_finish(f, st));
  if (!host) return GPMP2MI_OK;
  auto back = [&](void* dst, const void* src, size_t bytes) -> int {
    if (dst) G2_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    return GPMP2MI_OK;
  };
  G2_TRY(back(out.support, w.out.support, P.B * sizeof(double)));
  G2_TRY(back(out.dense, w.out.dense, P.B * sizeof(double)));
  G2_TRY(back(out.clearance, w.out.clearance, P.B * sizeof(double)));
  G2_TRY(back(out.worst, w.out.worst, (size_t)3 * P.B * sizeof(int)));
  G2_TRY(back(out.oor, w.out.oor, P.B * sizeof(int)));
  struct { int best, n; double err; } pick{-1, 0, 0.0};
  if (sel) G2_TRY(back(&pick, w.pick, sizeof(pick)));
  G2_HIP(hipStreamSynchronize(st));
  if (sel) {
    if (sel->best) *sel->best = pick.best;
    if (sel->n_eligible) *sel->n_eligible = pick.n;
    if (pick.best >= 0 && (sel->traj_best || sel->dense_best)) {   // nothing chosen: the trajectory outputs stay as they are
      G2_TRY(back(sel->traj_best, w.traj_best, (size_t)(P.N + 1) * 2 * P.D * sizeof(double)));
      G2_TRY(back(sel->dense_best, w.dense_best, Md * 2 * P.D * sizeof(double)));
      G2_HIP(hipStreamSynchronize(st));
    }
  }
  p->mark_clean(st);
  return GPMP2MI_OK;
}

int check_traj_call(const gpmp2mi_robot* r, int K, const double* radius, const double* centers, double epsilon,
                    double delta_t, int inter, int B, int total_step, const double* traj) {
  G2_CHECK(r && traj, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_set_args(K, GPMP2MI_MAX_MOVING_SPHERES, radius, centers));
  G2_CHECK(!std::isnan(epsilon), GPMP2MI_ERR_INVALID, "epsilon is NaN");
  return check_moving_args(r, K, inter, B, total_step, delta_t);
}

ScoreOut make_out(double* support, double* dense, double* clearance, int* worst, int* invalid) {
  ScoreOut o;
  o.support = support; o.dense = dense; o.clearance = clearance; o.worst = worst; o.oor = invalid;
  return o;
}
MovingSel make_sel(double required_clearance, int require_in_range, const gpmp2mi_self_pairs* pairs,
                   double required_self_clearance, double required_moving_clearance, int* best, int* n_eligible,
                   double* traj_best, double* dense_best) {
  MovingSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.pairs = pairs; sel.required_self_clearance = required_self_clearance;
  sel.required_moving_clearance = required_moving_clearance;
  sel.best = best; sel.n_eligible = n_eligible; sel.traj_best = traj_best; sel.dense_best = dense_best;
  return sel;
}

}  // namespace

extern "C" {

int gpmp2mi_plan_set_moving_spheres(gpmp2mi_plan* p, int K, const double* radius, const double* centers) {
  return set_moving(p, K, radius, centers, true, nullptr);
}
int gpmp2mi_plan_set_moving_spheres_dev(gpmp2mi_plan* p, int K, const double* radius, const double* centers, void* stream) {
  return set_moving(p, K, radius, centers, false, (hipStream_t)stream);
}

int gpmp2mi_moving_sphere_factor(const gpmp2mi_robot* r, int K, const double* radius, double epsilon, int M,
                                 const double* conf, const double* centers, double* err, double* H) {
  G2_CHECK(r && conf && err && M >= 0, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_set_args(K, GPMP2MI_MAX_MOVING_SPHERES, radius, centers));
  G2_CHECK(!std::isnan(epsilon), GPMP2MI_ERR_INVALID, "epsilon is NaN");
  if (M == 0 || K == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const int D = r->h.dof, S = r->h.nr_spheres;
  std::vector<double> rr(S);
  for (int s = 0; s < S; s++) rr[r->h.sph_orig[s]] = r->h.sph_r[s];
  DevBuf<double> dq, dc, dj, drr, dr, dm, de, dh;
  G2_TRY(dq.upload(conf, (size_t)M * D));
  G2_TRY(drr.upload(rr.data(), S));
  G2_TRY(dr.upload(radius, K));
  G2_TRY(dm.upload(centers, (size_t)M * K * 3));
  G2_TRY(dc.alloc((size_t)M * S * 3));
  if (H) G2_TRY(dj.alloc((size_t)M * S * 3 * D));
  G2_TRY(de.out(err, (size_t)M * S * K));
  if (H) G2_TRY(dh.out(H, (size_t)M * S * K * D));
  G2_TRY(launch_sphere_centers(r->h, r->d, M, dq.p, dc.p, dj.p, nullptr));
  G2_TRY(launch_moving_factor(S, D, K, M, drr.p, dr.p, epsilon, dm.p, dc.p, dj.p, de.p, dh.p, nullptr));
  return fetch_all(de, dh);
}

int gpmp2mi_moving_score_traj_dev(const gpmp2mi_robot* r, int K, const double* radius, const double* centers,
                                  double epsilon, double delta_t, int inter_step, int B, int total_step,
                                  const double* traj, double* moving_support_cost, double* moving_dense_cost,
                                  double* min_moving_clearance, int* worst, int* invalid, void* stream) {
  G2_TRY(check_traj_call(r, K, radius, centers, epsilon, delta_t, inter_step, B, total_step, traj));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  int cur = -1;
  G2_HIP(hipGetDevice(&cur));
  G2_CHECK(cur == r->device, GPMP2MI_ERR_INVALID, "the robot handle lives on another device than the current one");
  const int Md = total_step * (inter_step + 1) + 1;
  const int nblk = self_blocks(Md, r->h.nr_spheres);
  std::lock_guard<std::mutex> lk(r->score_mu);
  G2_TRY(ws_reserve(&r->moving_ws, &r->moving_ws_bytes, (size_t)B * nblk * sizeof(ScoreRec)));
  MovingFinish f{};
  f.sel.B = B;
  f.recs = (ScoreRec*)r->moving_ws;
  f.nblk = nblk;
  f.K = K;
  f.support = moving_support_cost;
  f.dense = moving_dense_cost;
  f.min_clearance = min_moving_clearance;
  f.worst = worst;
  f.invalid = invalid;
  G2_TRY(launch_moving_clearance(r->h, r->d, K, radius, centers, epsilon, delta_t, inter_step, B, total_step, traj,
                                 (ScoreRec*)r->moving_ws, (hipStream_t)stream));
  return launch_moving_finish(f, (hipStream_t)stream);
}

int gpmp2mi_moving_score_traj(const gpmp2mi_robot* r, int K, const double* radius, const double* centers, double epsilon,
                              double delta_t, int inter_step, int B, int total_step, const double* traj,
                              double* moving_support_cost, double* moving_dense_cost, double* min_moving_clearance,
                              int* worst, int* invalid) {
  G2_TRY(check_traj_call(r, K, radius, centers, epsilon, delta_t, inter_step, B, total_step, traj));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  DevBuf<double> dt, dr, dm, ds, dd, dc;
  DevBuf<int> dw, di;
  G2_TRY(dt.upload(traj, (size_t)B * (total_step + 1) * 2 * r->h.dof));
  G2_TRY(dr.upload(radius, K));
  G2_TRY(dm.upload(centers, (size_t)K * (total_step + 1) * 3));
  if (moving_support_cost) G2_TRY(ds.out(moving_support_cost, B));
  if (moving_dense_cost) G2_TRY(dd.out(moving_dense_cost, B));
  if (min_moving_clearance) G2_TRY(dc.out(min_moving_clearance, B));
  if (worst) G2_TRY(dw.out(worst, (size_t)3 * B));
  if (invalid) G2_TRY(di.out(invalid, B));
  G2_TRY(gpmp2mi_moving_score_traj_dev(r, K, dr.p, dm.p, epsilon, delta_t, inter_step, B, total_step, dt.p, ds.p, dd.p, dc.p,
                                       dw.p, di.p, nullptr));
  return fetch_all(ds, dd, dc, dw, di);
}

int gpmp2mi_plan_moving_score(gpmp2mi_plan* p, int inter_step, double* moving_support_cost, double* moving_dense_cost,
                              double* min_moving_clearance, int* worst, int* invalid) {
  return plan_moving(p, inter_step, make_out(moving_support_cost, moving_dense_cost, min_moving_clearance, worst, invalid),
                     nullptr, true, nullptr);
}
int gpmp2mi_plan_moving_score_dev(gpmp2mi_plan* p, int inter_step, double* moving_support_cost,
                                  double* moving_dense_cost, double* min_moving_clearance, int* worst, int* invalid,
                                  void* stream) {
  return plan_moving(p, inter_step, make_out(moving_support_cost, moving_dense_cost, min_moving_clearance, worst, invalid),
                     nullptr, false, (hipStream_t)stream);
}

int gpmp2mi_plan_select_moving(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                               const gpmp2mi_self_pairs* pairs, double required_self_clearance,
                               double required_moving_clearance, int* best, int* n_eligible, double* traj_best,
                               double* dense_best) {
  const MovingSel sel = make_sel(required_clearance, require_in_range, pairs, required_self_clearance,
                                 required_moving_clearance, best, n_eligible, traj_best, dense_best);
  return plan_moving(p, inter_step, ScoreOut{}, &sel, true, nullptr);
}
int gpmp2mi_plan_select_moving_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                   const gpmp2mi_self_pairs* pairs, double required_self_clearance,
                                   double required_moving_clearance, int* best, int* n_eligible, double* traj_best,
                                   double* dense_best, void* stream) {
  const MovingSel sel = make_sel(required_clearance, require_in_range, pairs, required_self_clearance,
                                 required_moving_clearance, best, n_eligible, traj_best, dense_best);
  return plan_moving(p, inter_step, ScoreOut{}, &sel, false, (hipStream_t)stream);
}

}  // extern "C"
