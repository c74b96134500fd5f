// moving.hip -- moving obstacles (include/gpmp2mi.h "moving obstacles"): the plan's sphere set, the factor-level entry
// point, the check of the executed trajectory for caller buffers and for a plan's resident result, and the selection
// that asks for the moving clearance as well.  Kernels: moving_kernels.hip; the factor inside a plan is launched by
// plan_linearize (plan_run.hip).  The obstacle and self-collision sides of select_moving are the existing stages
// (plan_score, plan_self_score), enqueued ahead with their per-row outputs in this unit's workspace.
#include <cmath>

#include "host.h"

using namespace g2;

namespace {

// behind the rules of check_score_args: the launch limits of this stage (the tile of the self check, Md S K pairs per row)
int check_moving_limits(const gpmp2mi_robot* r, int K, int inter, int B, int total_step) {
  const int S = r->h.nr_spheres;
  const long long Md = (long long)total_step * (inter + 1) + 1;
  G2_CHECK((long long)self_blocks((int)Md, S) * std::max(B, 1) < (1ll << 31) && Md * std::max(S * K, 1) < (1ll << 31),
           GPMP2MI_ERR_INVALID, "too many checked (state, sphere, moving sphere)s for one launch");
  return GPMP2MI_OK;
}
int check_moving_args(const gpmp2mi_robot* r, int K, int inter, int B, int total_step, double delta_t) {
  G2_TRY(check_score_args(inter, B, total_step, delta_t));
  return check_moving_limits(r, K, inter, B, total_step);
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

// Scores the plan's resident result against its resident set on `st`; sel != null: the existing stages for the same
// rows first, then the extended rule and the copy of the chosen row.  host / out / sel as plan_score (score.hip);
// out.oor: invalid, out.worst: [B][3].
int plan_moving(gpmp2mi_plan* p, int inter, const ScoreOut& out, const MovingSel* sel, bool host, hipStream_t st) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_CHECK(p->ex.mv_cap > 0, GPMP2MI_ERR_INVALID, "the plan was created without room for moving spheres");
  G2_TRY(check_plan_ready(p, inter));
  const PlanParams& P = p->hp;
  const PlanExtras& ex = p->ex;
  G2_TRY(check_moving_limits(p->robot, ex.mv_K, inter, P.B, P.N));
  const int S = p->robot->h.nr_spheres, Md = P.N * (inter + 1) + 1;
  const size_t rec_bytes = (size_t)P.B * self_blocks(Md, S) * sizeof(ScoreRec);
  RowOut rows[SCORE_ROWS];
  rows_of(out, MOVING_WORST, rows);
  const auto layout = [&](void* base) { return carve_moving((char*)base, rec_bytes, rows, shape_of(p, inter)); };
  CheckWs w;
  G2_TRY(carve_into(p->ws[p->WS_MOVING], layout, &w));
  MovingFinish f{};
  const ScoreOut o = score_out(rows, host);
  f.support = o.support;
  f.dense = o.dense;
  f.min_clearance = o.clearance;
  f.worst = o.worst;
  f.invalid = o.oor;
  f.recs = (ScoreRec*)w.recs;
  f.nblk = self_blocks(Md, S);
  f.K = ex.mv_K;
  plan_shape(f.sel, p, inter);
  if (sel) {
    point_selection(f.sel, p, *sel, nullptr, host, w.sel);
    f.required_self_clearance = sel->required_self_clearance;
    f.required_moving_clearance = sel->required_moving_clearance;
    PriorRows got;
    G2_TRY(enqueue_prior_stages(p, sel->pairs, inter, w.prior, st, &got));
    f.clearance = got.clearance;
    f.oor = got.oor;
    f.self_clearance = got.self_clearance;
    f.self_invalid = got.self_invalid;
  }
  p->mark_dirty(st);
  G2_TRY(launch_moving_clearance(p->robot->h, p->robot->d, ex.mv_K, ex.mv_radius, ex.mv_centers, ex.mv_eps, P.delta_t, inter,
                                 P.B, P.N, p->pb.result, (ScoreRec*)w.recs, st));
  G2_TRY(launch_moving_finish(f, st));
  return host ? finish_host(p, inter, rows, SCORE_ROWS, sel, nullptr, w.sel, st) : GPMP2MI_OK;
}

int check_traj_call(const gpmp2mi_robot* r, int K, const double* radius, const double* centers, double epsilon,
                    double delta_t, int inter, int B, int total_step, const double* traj) {
  G2_CHECK(r && traj, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_set_args(K, GPMP2MI_MAX_MOVING_SPHERES, radius, centers));
  G2_CHECK(!std::isnan(epsilon), GPMP2MI_ERR_INVALID, "epsilon is NaN");
  return check_moving_args(r, K, inter, B, total_step, delta_t);
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
  const int Md = total_step * (inter_step + 1) + 1;
  const int nblk = self_blocks(Md, r->h.nr_spheres);
  std::unique_lock<std::mutex> lk;
  G2_TRY(records_ready(r, nullptr, r->moving_ws, (size_t)B * nblk * sizeof(ScoreRec), lk));
  MovingFinish f{};
  f.sel.B = B;
  f.recs = (ScoreRec*)r->moving_ws.p;
  f.nblk = nblk;
  f.K = K;
  f.support = moving_support_cost;
  f.dense = moving_dense_cost;
  f.min_clearance = min_moving_clearance;
  f.worst = worst;
  f.invalid = invalid;
  G2_TRY(launch_moving_clearance(r->h, r->d, K, radius, centers, epsilon, delta_t, inter_step, B, total_step, traj,
                                 (ScoreRec*)r->moving_ws.p, (hipStream_t)stream));
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
