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

struct MotionOut {
  double *pos_margin = nullptr, *vel_ratio = nullptr, *acc_ratio = nullptr, *point_speed = nullptr, *time_scale = nullptr;
  int *worst = nullptr, *invalid = nullptr;
};
struct MotionSel {
  double required_clearance = 0.0, required_self_clearance = 0.0, required_pos_margin = 0.0, max_time_scale = 0.0;
  int require_in_range = 0;
  const gpmp2mi_self_pairs* pairs = nullptr;
  int *best = nullptr, *n_eligible = nullptr;
  double *time_scale_best = nullptr, *traj_best = nullptr, *dense_best = nullptr;
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

// Layout of a plan's motion workspace for (B, N, D, inter): the records, the per-row scores of the existing stages,
// then the staging of the host-pointer forms
struct PlanMotionWs {
  MotionRec* recs;
  double *clearance, *self_clearance;
  int *oor, *self_invalid;
  MotionOut out;
  char* pick;   // best, n_eligible, then (8-byte aligned) the chosen row's final_error and time_scale: one 24-byte copy
  double *traj_best, *dense_best;
  size_t bytes;
};
PlanMotionWs plan_ws_layout(char* base, int B, int N, int D, int inter) {
  const size_t Md = (size_t)N * (inter + 1) + 1;
  PlanMotionWs w{};
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base + off;
    off += ws_round(bytes);
    return p;
  };
  w.recs = (MotionRec*)take((size_t)B * score_blocks((int)Md) * sizeof(MotionRec));
  w.clearance = (double*)take(B * sizeof(double));
  w.self_clearance = (double*)take(B * sizeof(double));
  w.oor = (int*)take(B * sizeof(int));
  w.self_invalid = (int*)take(B * sizeof(int));
  w.out.pos_margin = (double*)take(B * sizeof(double));
  w.out.vel_ratio = (double*)take(B * sizeof(double));
  w.out.acc_ratio = (double*)take(B * sizeof(double));
  w.out.point_speed = (double*)take(B * sizeof(double));
  w.out.time_scale = (double*)take(B * sizeof(double));
  w.out.worst = (int*)take((size_t)8 * B * sizeof(int));
  w.out.invalid = (int*)take(B * sizeof(int));
  w.pick = take(2 * sizeof(int) + 2 * sizeof(double));
  w.traj_best = (double*)take((size_t)(N + 1) * 2 * D * sizeof(double));
  w.dense_best = (double*)take(Md * 2 * D * sizeof(double));
  w.bytes = off;
  return w;
}

struct Pick {
  int best, n;
  double err, time_scale;
};

// Scores the plan's resident result on `st`; sel != null: the existing stages for the same rows first, then the
// extended rule and the copy of the chosen row.  host / out / sel as plan_score (score.hip).
int plan_motion(gpmp2mi_plan* p, const gpmp2mi_motion_limits* l, int inter, const MotionOut& out, const MotionSel* sel,
                bool host, hipStream_t st) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_TRY(check_limits_head(l));
  if (sel)
    G2_CHECK(!std::isnan(sel->required_pos_margin) && !std::isnan(sel->max_time_scale), GPMP2MI_ERR_INVALID,
             "required_pos_margin / max_time_scale is NaN");
  G2_PLAN_LIVE(p);   // before anything is enqueued
  G2_CHECK(p->optimized, GPMP2MI_ERR_INVALID, "plan has not been optimized");
  const PlanParams& P = p->hp;
  G2_TRY(check_score_args(inter, P.B, P.N, P.delta_t));
  G2_CHECK(p->robot->h.dof == P.D, GPMP2MI_ERR_INVALID, "robot dof does not fit the plan");
  MotionLimitsDev lim;
  G2_TRY(read_limits(l, P.D, &lim));
  G2_TRY(ws_reserve(&p->motion_ws, &p->motion_ws_bytes, plan_ws_layout(nullptr, P.B, P.N, P.D, inter).bytes));
  const PlanMotionWs w = plan_ws_layout((char*)p->motion_ws, P.B, P.N, P.D, inter);
  const size_t Md = (size_t)P.N * (inter + 1) + 1;
  Pick* pick = (Pick*)w.pick;
  MotionFinish f{};
  MotionOut o;   // the host form computes only what the caller asked for
  if (host) {
    o.pos_margin = out.pos_margin ? w.out.pos_margin : nullptr;
    o.vel_ratio = out.vel_ratio ? w.out.vel_ratio : nullptr;
    o.acc_ratio = out.acc_ratio ? w.out.acc_ratio : nullptr;
    o.point_speed = out.point_speed ? w.out.point_speed : nullptr;
    o.time_scale = out.time_scale ? w.out.time_scale : nullptr;
    o.worst = out.worst ? w.out.worst : nullptr;
    o.invalid = out.invalid ? w.out.invalid : nullptr;
  } else {
    o = out;
  }
  set_outputs(f, o);
  f.recs = w.recs;
  f.nblk = score_blocks((int)Md);
  f.limit_point_speed = l->point_speed;
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
    f.required_pos_margin = sel->required_pos_margin;
    f.max_time_scale = sel->max_time_scale;
    g.ferr = p->pb.final_err;
    g.status = p->pb.status;
    // the kernel reads `best` back for time_scale_best: a device form without one gets the workspace's
    g.best = (host || !sel->best) ? &pick->best : sel->best;
    g.n_eligible = host ? &pick->n : sel->n_eligible;
    g.best_err = host ? &pick->err : nullptr;
    f.time_scale_best = host ? &pick->time_scale : sel->time_scale_best;
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
  G2_TRY(launch_motion(p->robot->h, p->robot->d, lim, P.delta_t, inter, P.B, P.N, p->pb.result, w.recs, st));
  G2_TRY(launch_motion_finish(f, st));
  if (!host) return GPMP2MI_OK;
  auto back = [&](void* dst, const void* src, size_t bytes) -> int {
    if (dst) G2_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    return GPMP2MI_OK;
  };
  G2_TRY(back(out.pos_margin, w.out.pos_margin, P.B * sizeof(double)));
  G2_TRY(back(out.vel_ratio, w.out.vel_ratio, P.B * sizeof(double)));
  G2_TRY(back(out.acc_ratio, w.out.acc_ratio, P.B * sizeof(double)));
  G2_TRY(back(out.point_speed, w.out.point_speed, P.B * sizeof(double)));
  G2_TRY(back(out.time_scale, w.out.time_scale, P.B * sizeof(double)));
  G2_TRY(back(out.worst, w.out.worst, (size_t)8 * P.B * sizeof(int)));
  G2_TRY(back(out.invalid, w.out.invalid, P.B * sizeof(int)));
  Pick got{-1, 0, 0.0, 0.0};
  if (sel) G2_TRY(back(&got, w.pick, sizeof(got)));
  G2_HIP(hipStreamSynchronize(st));
  if (sel) {
    if (sel->best) *sel->best = got.best;
    if (sel->n_eligible) *sel->n_eligible = got.n;
    if (got.best >= 0) {   // nothing chosen: the outputs about the chosen row stay as they are
      if (sel->time_scale_best) *sel->time_scale_best = got.time_scale;
      if (sel->traj_best || sel->dense_best) {
        G2_TRY(back(sel->traj_best, w.traj_best, (size_t)(P.N + 1) * 2 * P.D * sizeof(double)));
        G2_TRY(back(sel->dense_best, w.dense_best, Md * 2 * P.D * sizeof(double)));
        G2_HIP(hipStreamSynchronize(st));
      }
    }
  }
  p->mark_clean(st);
  return GPMP2MI_OK;
}

int check_traj_call(const gpmp2mi_robot* r, const gpmp2mi_motion_limits* l, double delta_t, int inter, int B,
                    int total_step, const double* traj) {
  G2_CHECK(r && traj, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_limits_head(l));
  return check_score_args(inter, B, total_step, delta_t);
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
  G2_TRY(ensure_device());
  int cur = -1;
  G2_HIP(hipGetDevice(&cur));
  G2_CHECK(cur == r->device, GPMP2MI_ERR_INVALID, "the robot handle lives on another device than the current one");
  const int Md = total_step * (inter_step + 1) + 1;
  const int nblk = score_blocks(Md);
  std::lock_guard<std::mutex> lk(r->score_mu);
  G2_TRY(ws_reserve(&r->motion_ws, &r->motion_ws_bytes, (size_t)B * nblk * sizeof(MotionRec)));
  MotionFinish f{};
  f.sel.B = B;
  f.recs = (MotionRec*)r->motion_ws;
  f.nblk = nblk;
  f.limit_point_speed = l->point_speed;
  MotionOut o;
  o.pos_margin = pos_margin; o.vel_ratio = vel_ratio; o.acc_ratio = acc_ratio; o.point_speed = point_speed;
  o.time_scale = time_scale; o.worst = worst; o.invalid = invalid;
  set_outputs(f, o);
  G2_TRY(launch_motion(r->h, r->d, lim, delta_t, inter_step, B, total_step, traj, (MotionRec*)r->motion_ws,
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
  MotionOut o;
  o.pos_margin = pos_margin; o.vel_ratio = vel_ratio; o.acc_ratio = acc_ratio; o.point_speed = point_speed;
  o.time_scale = time_scale; o.worst = worst; o.invalid = invalid;
  return plan_motion(p, l, inter_step, o, nullptr, true, nullptr);
}
int gpmp2mi_plan_motion_score_dev(gpmp2mi_plan* p, const gpmp2mi_motion_limits* l, int inter_step, double* pos_margin,
                                  double* vel_ratio, double* acc_ratio, double* point_speed, double* time_scale,
                                  int* worst, int* invalid, void* stream) {
  MotionOut o;
  o.pos_margin = pos_margin; o.vel_ratio = vel_ratio; o.acc_ratio = acc_ratio; o.point_speed = point_speed;
  o.time_scale = time_scale; o.worst = worst; o.invalid = invalid;
  return plan_motion(p, l, inter_step, o, nullptr, false, (hipStream_t)stream);
}

int gpmp2mi_plan_select_feasible(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                 const gpmp2mi_self_pairs* pairs, double required_self_clearance,
                                 const gpmp2mi_motion_limits* l, double required_pos_margin, double max_time_scale,
                                 int* best, int* n_eligible, double* time_scale_best, double* traj_best,
                                 double* dense_best) {
  MotionSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.pairs = pairs; sel.required_self_clearance = required_self_clearance;
  sel.required_pos_margin = required_pos_margin; sel.max_time_scale = max_time_scale;
  sel.best = best; sel.n_eligible = n_eligible; sel.time_scale_best = time_scale_best;
  sel.traj_best = traj_best; sel.dense_best = dense_best;
  return plan_motion(p, l, inter_step, MotionOut{}, &sel, true, nullptr);
}
int gpmp2mi_plan_select_feasible_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                     const gpmp2mi_self_pairs* pairs, double required_self_clearance,
                                     const gpmp2mi_motion_limits* l, double required_pos_margin, double max_time_scale,
                                     int* best, int* n_eligible, double* time_scale_best, double* traj_best,
                                     double* dense_best, void* stream) {
  MotionSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.pairs = pairs; sel.required_self_clearance = required_self_clearance;
  sel.required_pos_margin = required_pos_margin; sel.max_time_scale = max_time_scale;
  sel.best = best; sel.n_eligible = n_eligible; sel.time_scale_best = time_scale_best;
  sel.traj_best = traj_best; sel.dense_best = dense_best;
  return plan_motion(p, l, inter_step, MotionOut{}, &sel, false, (hipStream_t)stream);
}

}  // extern "C"
