// motion_score.hip -- the motion limits of the executed trajectory (include/gpmp2mi.h "motion limits"): the per-row
// scores for caller buffers and for a plan's resident result, and the selection that asks for an executable row.
// Kernels: motion_kernels.hip; the obstacle and self-collision sides of select_feasible are the existing stages
// (plan_score, plan_self_score), enqueued ahead with their per-row outputs in this unit's workspace.
#include <cmath>
#include <limits>

#include "host.h"

using namespace g2;

constexpr double INF = std::numeric_limits<double>::infinity();

// what needs no robot handle: the struct itself and its scalar
int g2::check_limits_head(const gpmp2mi_motion_limits* l) {
  G2_CHECK(l, GPMP2MI_ERR_INVALID, "null motion limits");
  G2_CHECK((l->pos_down == nullptr) == (l->pos_up == nullptr), GPMP2MI_ERR_INVALID,
           "pos_down and pos_up are given together or not at all");
  G2_CHECK(l->point_speed > 0, GPMP2MI_ERR_INVALID, "point_speed must be > 0 (+inf: no limit)");   // false for NaN
  return GPMP2MI_OK;
}

// the arrays, [dof]: read here, before the call returns
int g2::read_limits(const gpmp2mi_motion_limits* l, int dof, MotionLimitsDev* out) {
  G2_CHECK(dof >= 1 && dof <= GPMP2MI_MAX_DOF, GPMP2MI_ERR_INVALID, "dof outside 1..GPMP2MI_MAX_DOF");
  for (int d = 0; d < GPMP2MI_MAX_DOF; d++) {
    out->down[d] = -INF;
    out->up[d] = out->vel[d] = out->acc[d] = INF;
  }
  for (int d = 0; d < dof; d++) {
    if (l->pos_down) {
      const double lo = l->pos_down[d], hi = l->pos_up[d];
      G2_CHECK(!std::isnan(lo) && !std::isnan(hi), GPMP2MI_ERR_INVALID, "a position limit is NaN");
      G2_CHECK(!(lo > hi), GPMP2MI_ERR_INVALID, "pos_down > pos_up");
      out->down[d] = lo;
      out->up[d] = hi;
    }
    if (l->vel) {
      G2_CHECK(l->vel[d] > 0, GPMP2MI_ERR_INVALID, "a velocity limit is NaN or <= 0");
      out->vel[d] = l->vel[d];
    }
    if (l->acc) {
      G2_CHECK(l->acc[d] > 0, GPMP2MI_ERR_INVALID, "an acceleration limit is NaN or <= 0");
      out->acc[d] = l->acc[d];
    }
  }
  return GPMP2MI_OK;
}

namespace {

struct MotionSel : ScoreSel {
  double required_self_clearance = 0.0, required_pos_margin = 0.0, max_time_scale = 0.0;
  const gpmp2mi_self_pairs* pairs = nullptr;
  double* time_scale_best = nullptr;
};

void set_outputs(MotionFinish& f, const MotionOut& o) {
  f.pos_margin = o.pos_margin;
  f.vel_ratio = o.vel_ratio;
  f.acc_ratio = o.acc_ratio;
  f.point_speed = o.point_speed;
  f.time_scale = o.time_scale;
  f.worst = o.worst;
  f.invalid = o.invalid;
}

// Scores the plan's resident result on `st`; sel != null: the existing stages for the same rows first, then the
// extended rule and the copy of the chosen row.  host / out / sel as plan_score (score.hip).
int plan_motion(gpmp2mi_plan* p, const gpmp2mi_motion_limits* l, int inter, const MotionOut& out, const MotionSel* sel,
                bool host, hipStream_t st) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_TRY(check_limits_head(l));
  if (sel)
    G2_CHECK(!std::isnan(sel->required_pos_margin) && !std::isnan(sel->max_time_scale), GPMP2MI_ERR_INVALID,
             "required_pos_margin / max_time_scale is NaN");
  G2_TRY(check_plan_ready(p, inter));
  const PlanParams& P = p->hp;
  MotionLimitsDev lim;
  G2_TRY(read_limits(l, P.D, &lim));
  const int Md = P.N * (inter + 1) + 1;
  const size_t rec_bytes = (size_t)P.B * score_blocks(Md) * sizeof(MotionRec);
  RowOut rows[MOTION_ROWS];
  rows_of(out, rows);
  const auto layout = [&](void* base) { return carve_motion((char*)base, rec_bytes, rows, shape_of(p, inter)); };
  CheckWs w;
  G2_TRY(carve_into(p->ws[p->WS_MOTION], layout, &w));
  MotionFinish f{};
  set_outputs(f, motion_out(rows, host));
  f.recs = (MotionRec*)w.recs;
  f.nblk = score_blocks(Md);
  f.limit_point_speed = l->point_speed;
  plan_shape(f.sel, p, inter);
  SelExtra x;
  if (sel) {
    x.value = sel->time_scale_best;
    f.time_scale_best = point_selection(f.sel, p, *sel, &x, host, w.sel).value;
    f.required_self_clearance = sel->required_self_clearance;
    f.required_pos_margin = sel->required_pos_margin;
    f.max_time_scale = sel->max_time_scale;
    PriorRows got;
    G2_TRY(enqueue_prior_stages(p, sel->pairs, inter, w.prior, st, &got));
    f.clearance = got.clearance;
    f.oor = got.oor;
    f.self_clearance = got.self_clearance;
    f.self_invalid = got.self_invalid;
  }
  p->mark_dirty(st);
  G2_TRY(launch_motion(p->robot->h, p->robot->d, lim, P.delta_t, inter, P.B, P.N, p->pb.result, (MotionRec*)w.recs, st));
  G2_TRY(launch_motion_finish(f, st));
  return host ? finish_host(p, inter, rows, MOTION_ROWS, sel, &x, w.sel, st) : GPMP2MI_OK;
}

int check_traj_call(const gpmp2mi_robot* r, const gpmp2mi_motion_limits* l, double delta_t, int inter, int B,
                    int total_step, const double* traj) {
  G2_CHECK(r && traj, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_limits_head(l));
  return check_score_args(inter, B, total_step, delta_t);
}

MotionOut make_out(double* pos_margin, double* vel_ratio, double* acc_ratio, double* point_speed, double* time_scale,
                   int* worst, int* invalid) {
  MotionOut o;
  o.pos_margin = pos_margin; o.vel_ratio = vel_ratio; o.acc_ratio = acc_ratio; o.point_speed = point_speed;
  o.time_scale = time_scale; o.worst = worst; o.invalid = invalid;
  return o;
}
MotionSel make_sel(double required_clearance, int require_in_range, const gpmp2mi_self_pairs* pairs,
                   double required_self_clearance, double required_pos_margin, double max_time_scale, int* best,
                   int* n_eligible, double* time_scale_best, double* traj_best, double* dense_best) {
  MotionSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.pairs = pairs; sel.required_self_clearance = required_self_clearance;
  sel.required_pos_margin = required_pos_margin; sel.max_time_scale = max_time_scale;
  sel.best = best; sel.n_eligible = n_eligible; sel.time_scale_best = time_scale_best;
  sel.traj_best = traj_best; sel.dense_best = dense_best;
  return sel;
}

}  // namespace

extern "C" {

void gpmp2mi_motion_limits_default(gpmp2mi_motion_limits* l) {
  if (!l) return;
  l->pos_down = l->pos_up = l->vel = l->acc = nullptr;
  l->point_speed = INF;
}

int gpmp2mi_motion_score_traj_dev(const gpmp2mi_robot* r, const gpmp2mi_motion_limits* l, double delta_t, int inter_step,
                                  int B, int total_step, const double* traj, double* pos_margin, double* vel_ratio,
                                  double* acc_ratio, double* point_speed, double* time_scale, int* worst, int* invalid,
                                  void* stream) {
  G2_TRY(check_traj_call(r, l, delta_t, inter_step, B, total_step, traj));
  MotionLimitsDev lim;
  G2_TRY(read_limits(l, r->h.dof, &lim));
  if (B == 0) return GPMP2MI_OK;
  const int Md = total_step * (inter_step + 1) + 1;
  const int nblk = score_blocks(Md);
  std::unique_lock<std::mutex> lk;
  G2_TRY(records_ready(r, nullptr, r->motion_ws, (size_t)B * nblk * sizeof(MotionRec), lk));
  MotionFinish f{};
  f.sel.B = B;
  f.recs = (MotionRec*)r->motion_ws.p;
  f.nblk = nblk;
  f.limit_point_speed = l->point_speed;
  set_outputs(f, make_out(pos_margin, vel_ratio, acc_ratio, point_speed, time_scale, worst, invalid));
  G2_TRY(launch_motion(r->h, r->d, lim, delta_t, inter_step, B, total_step, traj, (MotionRec*)r->motion_ws.p,
                       (hipStream_t)stream));
  return launch_motion_finish(f, (hipStream_t)stream);
}

int gpmp2mi_motion_score_traj(const gpmp2mi_robot* r, const gpmp2mi_motion_limits* l, double delta_t, int inter_step,
                              int B, int total_step, const double* traj, double* pos_margin, double* vel_ratio,
                              double* acc_ratio, double* point_speed, double* time_scale, int* worst, int* invalid) {
  G2_TRY(check_traj_call(r, l, delta_t, inter_step, B, total_step, traj));
  MotionLimitsDev lim;
  G2_TRY(read_limits(l, r->h.dof, &lim));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  DevBuf<double> dt, dp, dv, da, ds, dm;
  DevBuf<int> dw, di;
  G2_TRY(dt.upload(traj, (size_t)B * (total_step + 1) * 2 * r->h.dof));
  if (pos_margin) G2_TRY(dp.out(pos_margin, B));
  if (vel_ratio) G2_TRY(dv.out(vel_ratio, B));
  if (acc_ratio) G2_TRY(da.out(acc_ratio, B));
  if (point_speed) G2_TRY(ds.out(point_speed, B));
  if (time_scale) G2_TRY(dm.out(time_scale, B));
  if (worst) G2_TRY(dw.out(worst, (size_t)8 * B));
  if (invalid) G2_TRY(di.out(invalid, B));
  G2_TRY(gpmp2mi_motion_score_traj_dev(r, l, delta_t, inter_step, B, total_step, dt.p, dp.p, dv.p, da.p, ds.p, dm.p, dw.p,
                                       di.p, nullptr));
  return fetch_all(dp, dv, da, ds, dm, dw, di);
}

int gpmp2mi_plan_motion_score(gpmp2mi_plan* p, const gpmp2mi_motion_limits* l, int inter_step, double* pos_margin,
                              double* vel_ratio, double* acc_ratio, double* point_speed, double* time_scale, int* worst,
                              int* invalid) {
  return plan_motion(p, l, inter_step, make_out(pos_margin, vel_ratio, acc_ratio, point_speed, time_scale, worst, invalid),
                     nullptr, true, nullptr);
}
int gpmp2mi_plan_motion_score_dev(gpmp2mi_plan* p, const gpmp2mi_motion_limits* l, int inter_step, double* pos_margin,
                                  double* vel_ratio, double* acc_ratio, double* point_speed, double* time_scale,
                                  int* worst, int* invalid, void* stream) {
  return plan_motion(p, l, inter_step, make_out(pos_margin, vel_ratio, acc_ratio, point_speed, time_scale, worst, invalid),
                     nullptr, false, (hipStream_t)stream);
}

int gpmp2mi_plan_select_feasible(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                 const gpmp2mi_self_pairs* pairs, double required_self_clearance,
                                 const gpmp2mi_motion_limits* l, double required_pos_margin, double max_time_scale,
                                 int* best, int* n_eligible, double* time_scale_best, double* traj_best,
                                 double* dense_best) {
  const MotionSel sel = make_sel(required_clearance, require_in_range, pairs, required_self_clearance, required_pos_margin,
                                 max_time_scale, best, n_eligible, time_scale_best, traj_best, dense_best);
  return plan_motion(p, l, inter_step, MotionOut{}, &sel, true, nullptr);
}
int gpmp2mi_plan_select_feasible_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                     const gpmp2mi_self_pairs* pairs, double required_self_clearance,
                                     const gpmp2mi_motion_limits* l, double required_pos_margin, double max_time_scale,
                                     int* best, int* n_eligible, double* time_scale_best, double* traj_best,
                                     double* dense_best, void* stream) {
  const MotionSel sel = make_sel(required_clearance, require_in_range, pairs, required_self_clearance, required_pos_margin,
                                 max_time_scale, best, n_eligible, time_scale_best, traj_best, dense_best);
  return plan_motion(p, l, inter_step, MotionOut{}, &sel, false, (hipStream_t)stream);
}

}  // extern "C"
