// torque.hip -- the torque limits of the executed trajectory (include/gpmp2mi.h "torque limits"): the dynamics handle,
// the per-row scores for caller buffers and for a plan's resident result, and the selection that asks for a row the
// drives can produce.  Kernels: torque_kernels.hip; the obstacle, self-collision and motion sides of select_dynamic are
// the existing stages (enqueue_prior_stages, gpmp2mi_plan_motion_score_dev), enqueued ahead with their per-row outputs in
// this unit's workspace.
#include <cmath>
#include <cstring>
#include <limits>

#include "host.h"

using namespace g2;

constexpr double INF = std::numeric_limits<double>::infinity();

namespace {

int check_kind(const RobotDev& h) {
  G2_CHECK(h.kind == GPMP2MI_ROBOT_ARM, GPMP2MI_ERR_UNSUPPORTED,
           "torque limits are built for fixed-base arms only: the mobile kinds need a moving base in the recursion");
  G2_CHECK(h.arm_dof >= 1 && h.arm_dof <= TORQUE_MAX_AD, GPMP2MI_ERR_UNSUPPORTED,
           "torque limits are instantiated for arms of 1..8 joints");
  return GPMP2MI_OK;
}

// the kinematics a dynamics handle is bound to: kind, joint count, DH table and base pose
bool same_kinematics(const RobotDev& a, const RobotDev& b) {
  if (a.kind != b.kind || a.dof != b.dof || a.arm_dof != b.arm_dof || a.nr_links != b.nr_links) return false;
  const size_t n = (size_t)a.arm_dof * sizeof(double);
  return !std::memcmp(a.ca, b.ca, n) && !std::memcmp(a.sa, b.sa, n) && !std::memcmp(a.a, b.a, n) &&
         !std::memcmp(a.d, b.d, n) && !std::memcmp(a.bias, b.bias, n) && !std::memcmp(a.base, b.base, sizeof(a.base));
}
int check_dynamics(const gpmp2mi_robot* r, const gpmp2mi_dynamics* y) {
  G2_CHECK(same_kinematics(y->robot, r->h), GPMP2MI_ERR_INVALID,
           "the dynamics handle was made for another robot (kind / dof / DH table / base pose)");
  return GPMP2MI_OK;
}

struct DynamicSel : ScoreSel {
  double required_self_clearance = 0.0, required_pos_margin = 0.0, max_time_scale = 0.0;
  const gpmp2mi_self_pairs* pairs = nullptr;
  const gpmp2mi_motion_limits* limits = nullptr;
  double *time_scale_best = nullptr, *tau_best = nullptr;
};

void set_outputs(TorqueFinish& f, const TorqueOut& o) {
  f.torque_ratio = o.torque_ratio;
  f.static_ratio = o.static_ratio;
  f.time_scale = o.time_scale;
  f.worst = o.worst;
  f.invalid = o.invalid;
}

// Scores the plan's resident result on `st`; sel != null: the existing stages for the same rows first, then the
// extended rule and the copy of the chosen row.  host / out / sel as plan_score (score.hip).
int plan_torque(gpmp2mi_plan* p, const gpmp2mi_dynamics* y, int inter, const TorqueOut& out, const DynamicSel* sel,
                bool host, hipStream_t st) {
  G2_CHECK(p && y, GPMP2MI_ERR_INVALID, "null plan or dynamics handle");
  if (sel) {
    G2_TRY(check_limits_head(sel->limits));
    G2_CHECK(!std::isnan(sel->required_pos_margin) && !std::isnan(sel->max_time_scale), GPMP2MI_ERR_INVALID,
             "required_pos_margin / max_time_scale is NaN");
  }
  G2_TRY(check_plan_ready(p, inter));
  G2_TRY(check_dynamics(p->robot, y));
  G2_CHECK(y->device == p->device, GPMP2MI_ERR_INVALID, "the dynamics handle lives on another device than the plan");
  const PlanParams& P = p->hp;
  if (sel) {   // the limit arrays, before anything is enqueued
    MotionLimitsDev lim;
    G2_TRY(read_limits(sel->limits, P.D, &lim));
  }
  const size_t Md = (size_t)P.N * (inter + 1) + 1;
  const size_t rec_bytes = (size_t)P.B * score_blocks((int)Md) * sizeof(TorqueRec);
  RowOut rows[TORQUE_ROWS];
  rows_of(out, Md, P.D, rows);
  const auto layout = [&](void* base) { return carve_torque((char*)base, rec_bytes, rows, shape_of(p, inter)); };
  TorqueWs w;
  G2_TRY(carve_into(p->ws[p->WS_TORQUE], layout, &w));
  const TorqueOut o = torque_out(rows, host);
  TorqueFinish f{};
  set_outputs(f, o);
  f.recs = (TorqueRec*)w.recs;
  f.nblk = score_blocks((int)Md);
  plan_shape(f.sel, p, inter);
  double* tau = o.tau;
  SelExtra x;
  if (sel) {
    x.value = sel->time_scale_best;
    x.row = sel->tau_best;
    x.row_bytes = Md * P.D * sizeof(double);
    const SelExtra k = point_selection(f.sel, p, *sel, &x, host, w.sel);
    f.time_scale_best = k.value;
    f.tau_best = k.row;
    f.required_self_clearance = sel->required_self_clearance;
    f.required_pos_margin = sel->required_pos_margin;
    f.max_time_scale = sel->max_time_scale;
    PriorRows got;
    G2_TRY(enqueue_prior_stages(p, sel->pairs, inter, w.prior, st, &got));
    f.clearance = got.clearance;
    f.oor = got.oor;
    f.self_clearance = got.self_clearance;
    f.self_invalid = got.self_invalid;
    G2_TRY(gpmp2mi_plan_motion_score_dev(p, sel->limits, inter, w.prior.pos_margin, nullptr, nullptr, nullptr,
                                         w.motion_time_scale, nullptr, w.prior.motion_invalid, st));
    f.pos_margin = w.prior.pos_margin;
    f.motion_invalid = w.prior.motion_invalid;
    f.motion_time_scale = w.motion_time_scale;
    tau = (double*)rows[5].staged;   // a selection has no per-row outputs: the torques of every row, for tau_best
    f.tau = tau;
  }
  p->mark_dirty(st);
  G2_TRY(launch_torque(p->robot->h, p->robot->d, y->d, y->lim, P.delta_t, inter, P.B, P.N, p->pb.result,
                       (TorqueRec*)w.recs, tau, st));
  G2_TRY(launch_torque_finish(f, st));
  return host ? finish_host(p, inter, rows, TORQUE_ROWS, sel, &x, w.sel, st) : GPMP2MI_OK;
}

int check_traj_call(const gpmp2mi_robot* r, const gpmp2mi_dynamics* y, double delta_t, int inter, int B, int total_step,
                    const double* traj) {
  G2_CHECK(r && y && traj, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_score_args(inter, B, total_step, delta_t));
  return check_dynamics(r, y);
}

TorqueOut make_out(double* torque_ratio, double* static_ratio, double* time_scale, int* worst, int* invalid, double* tau) {
  TorqueOut o;
  o.torque_ratio = torque_ratio; o.static_ratio = static_ratio; o.time_scale = time_scale; o.worst = worst;
  o.invalid = invalid; o.tau = tau;
  return o;
}
DynamicSel make_sel(double required_clearance, int require_in_range, const gpmp2mi_self_pairs* pairs,
                    double required_self_clearance, const gpmp2mi_motion_limits* limits, double required_pos_margin,
                    double max_time_scale, int* best, int* n_eligible, double* time_scale_best, double* tau_best,
                    double* traj_best, double* dense_best) {
  DynamicSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.pairs = pairs; sel.required_self_clearance = required_self_clearance; sel.limits = limits;
  sel.required_pos_margin = required_pos_margin; sel.max_time_scale = max_time_scale;
  sel.best = best; sel.n_eligible = n_eligible; sel.time_scale_best = time_scale_best; sel.tau_best = tau_best;
  sel.traj_best = traj_best; sel.dense_best = dense_best;
  return sel;
}

}  // namespace

// what retime_dynamic.hip shares (host.h)
int g2::check_dynamics_binding(const gpmp2mi_robot* r, const gpmp2mi_dynamics* y) { return check_dynamics(r, y); }

extern "C" {

void gpmp2mi_dynamics_desc_default(gpmp2mi_dynamics_desc* d) {
  if (!d) return;
  d->mass = d->com = d->inertia = d->torque = nullptr;
  d->gravity[0] = d->gravity[1] = 0.0;
  d->gravity[2] = -9.81;
}

int gpmp2mi_dynamics_create(const gpmp2mi_robot* r, const gpmp2mi_dynamics_desc* d, gpmp2mi_dynamics** out) {
  G2_CHECK(r && d && out, GPMP2MI_ERR_INVALID, "null argument");
  *out = nullptr;
  G2_CHECK(d->mass && d->com && d->inertia, GPMP2MI_ERR_INVALID, "null mass / com / inertia");
  G2_TRY(check_kind(r->h));
  const int L = r->h.nr_links;
  auto y = std::make_unique<gpmp2mi_dynamics>();
  DynDev h{};
  for (int j = 0; j < L; j++) {
    G2_CHECK(std::isfinite(d->mass[j]) && d->mass[j] >= 0, GPMP2MI_ERR_INVALID, "a mass is not finite or negative");
    h.mass[j] = d->mass[j];
    for (int i = 0; i < 3; i++) {
      G2_CHECK(std::isfinite(d->com[3 * j + i]), GPMP2MI_ERR_INVALID, "a centre of mass is not finite");
      h.com[3 * j + i] = d->com[3 * j + i];
    }
    for (int i = 0; i < 6; i++) {
      const double v = d->inertia[6 * j + i];
      G2_CHECK(std::isfinite(v), GPMP2MI_ERR_INVALID, "an inertia entry is not finite");
      G2_CHECK(i >= 3 || v >= 0, GPMP2MI_ERR_INVALID, "a diagonal inertia is negative");
      h.inertia[6 * j + i] = v;
    }
  }
  for (int i = 0; i < 3; i++) {
    G2_CHECK(std::isfinite(d->gravity[i]), GPMP2MI_ERR_INVALID, "gravity is not finite");
    y->lim.gravity[i] = d->gravity[i];
  }
  for (int k = 0; k < TORQUE_MAX_AD; k++) y->lim.limit[k] = INF;
  if (d->torque)
    for (int k = 0; k < r->h.dof; k++) {
      G2_CHECK(d->torque[k] > 0, GPMP2MI_ERR_INVALID, "a torque limit is NaN or <= 0");   // false for NaN
      y->lim.limit[k] = d->torque[k];
    }
  y->robot = r->h;
  G2_TRY(ensure_device());
  G2_HIP(hipGetDevice(&y->device));
  G2_CHECK(y->device == r->device, GPMP2MI_ERR_INVALID, "the robot handle lives on another device than the current one");
  G2_TRY(dev_malloc((void**)&y->d, sizeof(DynDev), GPMP2MI_ERR_NO_DEVICE));
  G2_HIP(hipMemcpy(y->d, &h, sizeof(DynDev), hipMemcpyHostToDevice));
  *out = y.release();
  return GPMP2MI_OK;
}

void gpmp2mi_dynamics_destroy(gpmp2mi_dynamics* y) { delete y; }

int gpmp2mi_torque_score_traj_dev(const gpmp2mi_robot* r, const gpmp2mi_dynamics* y, double delta_t, int inter_step, int B,
                                  int total_step, const double* traj, double* torque_ratio, double* static_ratio,
                                  double* torque_time_scale, int* worst, int* invalid, double* tau, void* stream) {
  G2_TRY(check_traj_call(r, y, delta_t, inter_step, B, total_step, traj));
  if (B == 0) return GPMP2MI_OK;
  const int Md = total_step * (inter_step + 1) + 1;
  const int nblk = score_blocks(Md);
  G2_TRY(ensure_device());
  int cur = -1;
  G2_HIP(hipGetDevice(&cur));
  G2_CHECK(cur == r->device && cur == y->device, GPMP2MI_ERR_INVALID,
           "the robot handle or the dynamics handle lives on another device than the current one");
  std::unique_lock<std::mutex> lk(y->mu);
  G2_TRY(y->ws.reserve((size_t)B * nblk * sizeof(TorqueRec)));
  TorqueFinish f{};
  f.sel.B = B;
  f.recs = (TorqueRec*)y->ws.p;
  f.nblk = nblk;
  set_outputs(f, make_out(torque_ratio, static_ratio, torque_time_scale, worst, invalid, tau));
  G2_TRY(launch_torque(r->h, r->d, y->d, y->lim, delta_t, inter_step, B, total_step, traj, (TorqueRec*)y->ws.p, tau,
                       (hipStream_t)stream));
  return launch_torque_finish(f, (hipStream_t)stream);
}

int gpmp2mi_torque_score_traj(const gpmp2mi_robot* r, const gpmp2mi_dynamics* y, double delta_t, int inter_step, int B,
                              int total_step, const double* traj, double* torque_ratio, double* static_ratio,
                              double* torque_time_scale, int* worst, int* invalid, double* tau) {
  G2_TRY(check_traj_call(r, y, delta_t, inter_step, B, total_step, traj));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const size_t Md = (size_t)total_step * (inter_step + 1) + 1;
  DevBuf<double> dt, dr, ds, dm, da;
  DevBuf<int> dw, di;
  G2_TRY(dt.upload(traj, (size_t)B * (total_step + 1) * 2 * r->h.dof));
  if (torque_ratio) G2_TRY(dr.out(torque_ratio, B));
  if (static_ratio) G2_TRY(ds.out(static_ratio, B));
  if (torque_time_scale) G2_TRY(dm.out(torque_time_scale, B));
  if (worst) G2_TRY(dw.out(worst, (size_t)6 * B));
  if (invalid) G2_TRY(di.out(invalid, B));
  if (tau) G2_TRY(da.out(tau, (size_t)B * Md * r->h.dof));
  G2_TRY(gpmp2mi_torque_score_traj_dev(r, y, delta_t, inter_step, B, total_step, dt.p, dr.p, ds.p, dm.p, dw.p, di.p, da.p,
                                       nullptr));
  return fetch_all(dr, ds, dm, dw, di, da);
}

int gpmp2mi_plan_torque_score(gpmp2mi_plan* p, const gpmp2mi_dynamics* y, int inter_step, double* torque_ratio,
                              double* static_ratio, double* torque_time_scale, int* worst, int* invalid, double* tau) {
  return plan_torque(p, y, inter_step, make_out(torque_ratio, static_ratio, torque_time_scale, worst, invalid, tau),
                     nullptr, true, nullptr);
}
int gpmp2mi_plan_torque_score_dev(gpmp2mi_plan* p, const gpmp2mi_dynamics* y, int inter_step, double* torque_ratio,
                                  double* static_ratio, double* torque_time_scale, int* worst, int* invalid, double* tau,
                                  void* stream) {
  return plan_torque(p, y, inter_step, make_out(torque_ratio, static_ratio, torque_time_scale, worst, invalid, tau),
                     nullptr, false, (hipStream_t)stream);
}

int gpmp2mi_plan_select_dynamic(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                const gpmp2mi_self_pairs* pairs, double required_self_clearance,
                                const gpmp2mi_motion_limits* l, double required_pos_margin, double max_time_scale,
                                const gpmp2mi_dynamics* y, int* best, int* n_eligible, double* time_scale_best,
                                double* tau_best, double* traj_best, double* dense_best) {
  const DynamicSel sel = make_sel(required_clearance, require_in_range, pairs, required_self_clearance, l,
                                  required_pos_margin, max_time_scale, best, n_eligible, time_scale_best, tau_best,
                                  traj_best, dense_best);
  return plan_torque(p, y, inter_step, TorqueOut{}, &sel, true, nullptr);
}
int gpmp2mi_plan_select_dynamic_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                    const gpmp2mi_self_pairs* pairs, double required_self_clearance,
                                    const gpmp2mi_motion_limits* l, double required_pos_margin, double max_time_scale,
                                    const gpmp2mi_dynamics* y, int* best, int* n_eligible, double* time_scale_best,
                                    double* tau_best, double* traj_best, double* dense_best, void* stream) {
  const DynamicSel sel = make_sel(required_clearance, require_in_range, pairs, required_self_clearance, l,
                                  required_pos_margin, max_time_scale, best, n_eligible, time_scale_best, tau_best,
                                  traj_best, dense_best);
  return plan_torque(p, y, inter_step, TorqueOut{}, &sel, false, (hipStream_t)stream);
}

}  // extern "C"
