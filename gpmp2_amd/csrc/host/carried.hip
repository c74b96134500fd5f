// carried.hip -- carried object (include/gpmp2mi.h "carried object"): the plan's sphere set and its link, the
// factor-level entry point, the check of the executed trajectory for caller buffers and for a plan's resident result,
// and the selection that asks for the carried clearance as well.  Kernels: carried_kernels.hip; the factor inside a plan
// is launched by plan_linearize (plan_run.hip).  The obstacle and self-collision sides of select_carried are the
// existing stages (plan_score, plan_self_score), enqueued ahead with their per-row outputs in this unit's workspace.
#include <cmath>

#include "../dispatch.h"
#include "host.h"

using namespace g2;

namespace {

// the size against `cap` and the arrays: no handle is looked at
int check_set_sizes(int A, int cap, const double* radius, const double* centers) {
  G2_CHECK(A >= 0 && A <= cap, GPMP2MI_ERR_INVALID, "A < 0 or more carried spheres than there is room for");
  G2_CHECK(A == 0 || (radius && centers), GPMP2MI_ERR_INVALID, "null radius / centers with A > 0");
  return GPMP2MI_OK;
}
// ... then the link; host: the values as well
int check_set_args(const gpmp2mi_robot* r, int link, int A, int cap, const double* radius, const double* centers,
                   bool host) {
  G2_TRY(check_set_sizes(A, cap, radius, centers));
  G2_CHECK(link >= 0 && link < r->h.nr_links, GPMP2MI_ERR_INVALID, "link out of range");
  if (host) {
    for (int a = 0; a < A; a++)   // NaN compares false
      G2_CHECK(radius[a] >= 0, GPMP2MI_ERR_INVALID, "a radius is negative or NaN");
    for (int i = 0; i < 3 * A; i++) G2_CHECK(std::isfinite(centers[i]), GPMP2MI_ERR_INVALID, "a centre is not finite");
  }
  return GPMP2MI_OK;
}

// the kernels are instantiated per (kind, dof) and per field dimension
int check_handles(const gpmp2mi_robot* r, const gpmp2mi_sdf* s) {
  G2_CHECK(r && s, GPMP2MI_ERR_INVALID, "null robot or field handle");
  G2_CHECK(s->h.dim == 2 || s->h.dim == 3, GPMP2MI_ERR_INVALID, "the field is neither planar nor a volume");
  G2_DISPATCH_ROBOT_H(r->h, (void)0);   // GPMP2MI_ERR_UNSUPPORTED for a (kind, dof) the chain kernels do not cover
  return GPMP2MI_OK;
}

int set_carried(gpmp2mi_plan* p, int link, int A, const double* radius, const double* centers, bool host,
                hipStream_t st) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_TRY(check_set_sizes(A, GPMP2MI_MAX_CARRIED_SPHERES, radius, centers));   // what needs no look at the plan
  G2_TRY(check_set_args(p->robot, link, A, GPMP2MI_MAX_CARRIED_SPHERES, radius, centers, host));
  G2_CHECK(A <= p->ex.cr_cap, GPMP2MI_ERR_INVALID, "more carried spheres than the plan was created with room for");
  G2_PLAN_LIVE(p);
  PlanExtras& ex = p->ex;
  if (A > 0) {
    if (host) {
      G2_HIP(hipMemcpy(ex.cr_radius, radius, A * sizeof(double), hipMemcpyHostToDevice));
      G2_HIP(hipMemcpy(ex.cr_centers, centers, (size_t)A * 3 * sizeof(double), hipMemcpyHostToDevice));
    } else {
      p->mark_dirty(st);
      G2_HIP(hipMemcpyAsync(ex.cr_radius, radius, A * sizeof(double), hipMemcpyDeviceToDevice, st));
      G2_HIP(hipMemcpyAsync(ex.cr_centers, centers, (size_t)A * 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
  }
  ex.cr_link = link;
  ex.cr_A = A;
  return GPMP2MI_OK;
}

struct CarriedSel : ScoreSel {
  double required_self_clearance = 0.0, required_carried_clearance = 0.0;
  const gpmp2mi_self_pairs* pairs = nullptr;
};

// behind the rules of check_score_args: Md A (state, sphere)s per row are numbered in an int
int check_carried_limits(int A, int inter, int B, int total_step) {
  const long long Md = (long long)total_step * (inter + 1) + 1;
  G2_CHECK((long long)score_blocks((int)Md) * std::max(B, 1) < (1ll << 31) && Md * std::max(A, 1) < (1ll << 31),
           GPMP2MI_ERR_INVALID, "too many checked (state, carried sphere)s for one launch");
  return GPMP2MI_OK;
}

// Scores the plan's resident result against its resident set on `st`; sel != null: the existing stages for the same
// rows first, then the extended rule and the copy of the chosen row.  host / out / sel as plan_score (score.hip).
int plan_carried(gpmp2mi_plan* p, int inter, const ScoreOut& out, const CarriedSel* sel, bool host, hipStream_t st) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_CHECK(p->ex.cr_cap > 0, GPMP2MI_ERR_INVALID, "the plan was created without room for a carried object");
  G2_TRY(check_plan_ready(p, inter));
  const PlanParams& P = p->hp;
  const PlanExtras& ex = p->ex;
  G2_TRY(check_carried_limits(ex.cr_A, inter, P.B, P.N));
  const int Md = P.N * (inter + 1) + 1, nblk = score_blocks(Md);
  const size_t rec_bytes = (size_t)P.B * nblk * sizeof(ScoreRec);
  RowOut rows[SCORE_ROWS];
  rows_of(out, CARRIED_WORST, rows);
  const auto layout = [&](void* base) { return carve_carried((char*)base, rec_bytes, rows, shape_of(p, inter)); };
  CheckWs w;
  G2_TRY(carve_into(p->ws[p->WS_CARRIED], layout, &w));
  CarriedFinish f{};
  const ScoreOut o = score_out(rows, host);
  f.support = o.support;
  f.dense = o.dense;
  f.min_clearance = o.clearance;
  f.worst = o.worst;
  f.oor = o.oor;
  f.recs = (ScoreRec*)w.recs;
  f.nblk = nblk;
  plan_shape(f.sel, p, inter);
  if (sel) {
    point_selection(f.sel, p, *sel, nullptr, host, w.sel);
    f.required_self_clearance = sel->required_self_clearance;
    f.required_carried_clearance = sel->required_carried_clearance;
    PriorRows got;
    G2_TRY(enqueue_prior_stages(p, sel->pairs, inter, w.prior, st, &got));
    f.clearance = got.clearance;
    f.obs_oor = got.oor;
    f.self_clearance = got.self_clearance;
    f.self_invalid = got.self_invalid;
  }
  p->mark_dirty(st);
  G2_TRY(launch_carried_clearance(p->robot->h, p->robot->d, p->sdf->h, ex.cr_link, ex.cr_A, ex.cr_radius, ex.cr_centers,
                                  P.delta_t, inter, P.B, P.N, p->pb.result, (ScoreRec*)w.recs, st));
  G2_TRY(launch_carried_finish(f, st));
  return host ? finish_host(p, inter, rows, SCORE_ROWS, sel, nullptr, w.sel, st) : GPMP2MI_OK;
}

int check_traj_call(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, int link, int A, const double* radius,
                    const double* centers, bool host, double delta_t, int inter, int B, int total_step,
                    const double* traj) {
  G2_CHECK(r && s && traj, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_score_args(inter, B, total_step, delta_t));
  G2_TRY(check_set_args(r, link, A, GPMP2MI_MAX_CARRIED_SPHERES, radius, centers, host));
  G2_TRY(check_handles(r, s));
  return check_carried_limits(A, inter, B, total_step);
}

CarriedSel make_sel(double required_clearance, int require_in_range, const gpmp2mi_self_pairs* pairs,
                    double required_self_clearance, double required_carried_clearance, int* best, int* n_eligible,
                    double* traj_best, double* dense_best) {
  CarriedSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.pairs = pairs; sel.required_self_clearance = required_self_clearance;
  sel.required_carried_clearance = required_carried_clearance;
  sel.best = best; sel.n_eligible = n_eligible; sel.traj_best = traj_best; sel.dense_best = dense_best;
  return sel;
}

// the `_dev` form behind both trajectory entry points, its arguments accepted
int score_traj_dev(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, int link, int A, const double* radius,
                   const double* centers, double delta_t, int inter_step, int B, int total_step, const double* traj,
                   double* support, double* dense, double* clearance, int* worst, int* oor, hipStream_t st) {
  const int Md = total_step * (inter_step + 1) + 1;
  const int nblk = score_blocks(Md);
  std::unique_lock<std::mutex> lk;
  G2_TRY(records_ready(r, nullptr, r->carried_ws, (size_t)B * nblk * sizeof(ScoreRec), lk));
  G2_CHECK(s->device == r->device, GPMP2MI_ERR_INVALID, "the field handle lives on another device than the robot handle");
  CarriedFinish f{};
  f.sel.B = B;
  f.recs = (ScoreRec*)r->carried_ws.p;
  f.nblk = nblk;
  f.support = support;
  f.dense = dense;
  f.min_clearance = clearance;
  f.worst = worst;
  f.oor = oor;
  G2_TRY(launch_carried_clearance(r->h, r->d, s->h, link, A, radius, centers, delta_t, inter_step, B, total_step, traj,
                                  (ScoreRec*)r->carried_ws.p, st));
  return launch_carried_finish(f, st);
}

}  // namespace

extern "C" {

int gpmp2mi_plan_set_carried(gpmp2mi_plan* p, int link, int A, const double* radius, const double* centers) {
  return set_carried(p, link, A, radius, centers, true, nullptr);
}
int gpmp2mi_plan_set_carried_dev(gpmp2mi_plan* p, int link, int A, const double* radius, const double* centers,
                                 void* stream) {
  return set_carried(p, link, A, radius, centers, false, (hipStream_t)stream);
}
int gpmp2mi_plan_carried_count(const gpmp2mi_plan* p) {
  if (!p) {
    set_error("null plan");
    return -1;
  }
  return p->ex.cr_A;
}

int gpmp2mi_carried_sphere_factor(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, int link, int A, const double* radius,
                                  const double* centers, double epsilon, int M, const double* conf, double* err,
                                  double* H) {
  G2_CHECK(r && s && conf && err && M >= 0, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_set_args(r, link, A, GPMP2MI_MAX_CARRIED_SPHERES, radius, centers, true));
  G2_TRY(check_handles(r, s));
  G2_CHECK(std::isfinite(epsilon), GPMP2MI_ERR_INVALID, "epsilon is not finite");
  G2_CHECK((long long)M * A * r->h.dof < (1ll << 40), GPMP2MI_ERR_INVALID, "too many rows for one call");
  if (M == 0 || A == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const int D = r->h.dof;
  DevBuf<double> dq, dr, dc, de, dh;
  G2_TRY(dq.upload(conf, (size_t)M * D));
  G2_TRY(dr.upload(radius, A));
  G2_TRY(dc.upload(centers, (size_t)A * 3));
  G2_TRY(de.out(err, (size_t)M * A));
  if (H) G2_TRY(dh.out(H, (size_t)M * A * D));
  G2_TRY(launch_carried_factor(r->h, r->d, s->h, link, A, dr.p, dc.p, epsilon, M, dq.p, de.p, dh.p, nullptr));
  return fetch_all(de, dh);
}

int gpmp2mi_carried_score_traj_dev(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, int link, int A, const double* radius,
                                   const double* centers, double delta_t, int inter_step, int B, int total_step,
                                   const double* traj, double* carried_support_cost, double* carried_dense_cost,
                                   double* min_carried_clearance, int* worst, int* out_of_range, void* stream) {
  G2_TRY(check_traj_call(r, s, link, A, radius, centers, false, delta_t, inter_step, B, total_step, traj));
  if (B == 0) return GPMP2MI_OK;
  return score_traj_dev(r, s, link, A, radius, centers, delta_t, inter_step, B, total_step, traj, carried_support_cost,
                        carried_dense_cost, min_carried_clearance, worst, out_of_range, (hipStream_t)stream);
}

int gpmp2mi_carried_score_traj(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, int link, int A, const double* radius,
                               const double* centers, double delta_t, int inter_step, int B, int total_step,
                               const double* traj, double* carried_support_cost, double* carried_dense_cost,
                               double* min_carried_clearance, int* worst, int* out_of_range) {
  G2_TRY(check_traj_call(r, s, link, A, radius, centers, true, delta_t, inter_step, B, total_step, traj));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  DevBuf<double> dt, dr, dm, ds, dd, dc;
  DevBuf<int> dw, di;
  G2_TRY(dt.upload(traj, (size_t)B * (total_step + 1) * 2 * r->h.dof));
  G2_TRY(dr.upload(radius, A));
  G2_TRY(dm.upload(centers, (size_t)A * 3));
  if (carried_support_cost) G2_TRY(ds.out(carried_support_cost, B));
  if (carried_dense_cost) G2_TRY(dd.out(carried_dense_cost, B));
  if (min_carried_clearance) G2_TRY(dc.out(min_carried_clearance, B));
  if (worst) G2_TRY(dw.out(worst, (size_t)2 * B));
  if (out_of_range) G2_TRY(di.out(out_of_range, B));
  G2_TRY(score_traj_dev(r, s, link, A, dr.p, dm.p, delta_t, inter_step, B, total_step, dt.p, ds.p, dd.p, dc.p, dw.p, di.p,
                        nullptr));
  return fetch_all(ds, dd, dc, dw, di);
}

int gpmp2mi_plan_carried_score(gpmp2mi_plan* p, int inter_step, double* carried_support_cost, double* carried_dense_cost,
                               double* min_carried_clearance, int* worst, int* out_of_range) {
  return plan_carried(p, inter_step,
                      make_out(carried_support_cost, carried_dense_cost, min_carried_clearance, worst, out_of_range),
                      nullptr, true, nullptr);
}
int gpmp2mi_plan_carried_score_dev(gpmp2mi_plan* p, int inter_step, double* carried_support_cost,
                                   double* carried_dense_cost, double* min_carried_clearance, int* worst,
                                   int* out_of_range, void* stream) {
  return plan_carried(p, inter_step,
                      make_out(carried_support_cost, carried_dense_cost, min_carried_clearance, worst, out_of_range),
                      nullptr, false, (hipStream_t)stream);
}

int gpmp2mi_plan_select_carried(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                const gpmp2mi_self_pairs* pairs, double required_self_clearance,
                                double required_carried_clearance, int* best, int* n_eligible, double* traj_best,
                                double* dense_best) {
  const CarriedSel sel = make_sel(required_clearance, require_in_range, pairs, required_self_clearance,
                                  required_carried_clearance, best, n_eligible, traj_best, dense_best);
  return plan_carried(p, inter_step, ScoreOut{}, &sel, true, nullptr);
}
int gpmp2mi_plan_select_carried_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                    const gpmp2mi_self_pairs* pairs, double required_self_clearance,
                                    double required_carried_clearance, int* best, int* n_eligible, double* traj_best,
                                    double* dense_best, void* stream) {
  const CarriedSel sel = make_sel(required_clearance, require_in_range, pairs, required_self_clearance,
                                  required_carried_clearance, best, n_eligible, traj_best, dense_best);
  return plan_carried(p, inter_step, ScoreOut{}, &sel, false, (hipStream_t)stream);
}

}  // extern "C"
