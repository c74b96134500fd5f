// retime_dynamic.hip -- the speed profile of the executed trajectory under joint torque limits (include/gpmp2mi.h
// "re-timing under torque limits"): the bare rule with affine rows on caller arrays, the profile for caller trajectories
// and for a plan's resident result, and the selection that asks for the re-timed duration.  Kernels:
// retime_dynamic_kernels.hip (and k_retime_caps of retime_kernels.hip for ps); the rule: retime_affine_rule.h.  The
// argument rules are those of retime.hip and torque.hip (host.h).  The obstacle, self-collision and motion sides of
// select_retimed_dynamic are the existing stages, enqueued ahead with their per-row outputs in this unit's workspace.
#include <cmath>

#include "../retime_affine_rule.h"
#include "host.h"

using namespace g2;

static_assert(GPMP2MI_RETIME_STATIC == RETIME_STATIC, "retime_affine_rule.h states the value of GPMP2MI_RETIME_STATIC");

namespace {

// the robots the torque rows are built for: those of "torque limits", ahead of the handle's binding
int check_arm(const gpmp2mi_robot* r) {
  G2_CHECK(r->h.kind == GPMP2MI_ROBOT_ARM, GPMP2MI_ERR_UNSUPPORTED,
           "re-timing under torque limits is built for fixed-base arms only: the mobile kinds need a moving base in the "
           "recursion, the Pose2 kinds the acceleration of the tangent-space interpolation");
  G2_CHECK(r->h.arm_dof >= 1 && r->h.arm_dof <= TORQUE_MAX_AD, GPMP2MI_ERR_UNSUPPORTED,
           "torque limits are instantiated for arms of 1..8 joints");
  return GPMP2MI_OK;
}

// k_retime_caps, k_retime_coef, then k_retime_rows and k_retime_dynamic over `traj`; o: device pointers, a null sdot /
// u / stamps / coef takes the workspace's
int enqueue_retime_dynamic(const gpmp2mi_robot* r, const gpmp2mi_dynamics* y, const MotionLimitsDev& lim,
                           double point_speed, double dt, int inter, int B, int N, const double* traj,
                           const RetimeRates& rt, const RetimeDynCore& w, const RowOut* rows, const RetimeDynOut& o,
                           hipStream_t st) {
  const int D = r->h.dof;
  RetimeDynArgs g{};
  RetimeArgs& a = g.rt;
  a.B = B;
  a.N = N;
  a.inter = inter;
  a.Md = N * (inter + 1) + 1;
  a.D = D;
  a.dt = dt;
  a.h = dt / (double)(inter + 1);
  a.max_rate = rt.max_rate;
  a.rate_start = rt.rate_start;
  a.rate_end = rt.rate_end;
  a.point_speed = point_speed;
  for (int d = 0; d < GPMP2MI_MAX_DOF; d++) {
    a.acc[d] = lim.acc[d];
    a.vel[d] = lim.vel[d];
  }
  a.traj = traj;
  a.ps = w.core.ps;
  a.X = w.core.X;
  a.K = w.core.K;
  a.sdot = o.sdot ? o.sdot : (double*)rows[0].staged;
  a.u = o.u ? o.u : (double*)rows[1].staged;
  a.stamps = o.stamps ? o.stamps : (double*)rows[2].staged;
  a.duration = o.duration;
  a.achieved = o.achieved;
  a.dense = o.dense;
  a.status = o.status;
  double* coef = o.coef ? o.coef : (double*)rows[8].staged;
  g.R = D;
  g.stride = 4 * D;
  for (int d = 0; d < RETIME_DYN_MAX_ROWS; d++) g.bound[d] = y->lim.limit[d];
  g.cu = coef;
  g.cxl = coef + D;
  g.cxr = coef + 2 * D;
  g.off = coef + 3 * D;
  g.rows = w.stage_rows;
  g.tau = o.tau;
  g.nonfinite = w.nonfinite;
  G2_TRY(launch_retime_caps(r->h, r->d, dt, inter, B, N, traj, w.core.ps, st));
  G2_TRY(launch_retime_coef(r->h, r->d, y->d, y->lim, dt, inter, B, N, traj, coef, st));
  return launch_retime_dynamic(g, true, st);
}

struct RetimeDynSel : ScoreSel {
  double required_self_clearance = 0.0, required_pos_margin = 0.0, max_duration = 0.0;
  const gpmp2mi_self_pairs* pairs = nullptr;
  double *duration_best = nullptr, *stamps_best = nullptr, *tau_best = nullptr;
};

// Re-times the plan's resident result on `st`; sel != null: the existing stages for the same rows first, then the rule
// and the copy of the chosen row.  host / out / sel as plan_score (score.hip).
int plan_retime_dynamic(gpmp2mi_plan* p, const gpmp2mi_dynamics* y, const gpmp2mi_motion_limits* l, int inter,
                        const RetimeRates& rt, const RetimeDynOut& out, const RetimeDynSel* sel, bool host,
                        hipStream_t st) {
  G2_CHECK(p && y, GPMP2MI_ERR_INVALID, "null plan or dynamics handle");
  G2_TRY(check_limits_head(l));
  G2_TRY(check_retime_rates(rt));
  if (sel)
    G2_CHECK(!std::isnan(sel->required_pos_margin) && !std::isnan(sel->max_duration), GPMP2MI_ERR_INVALID,
             "required_pos_margin / max_duration is NaN");
  G2_TRY(check_plan_ready(p, inter));
  const PlanParams& P = p->hp;
  G2_TRY(check_arm(p->robot));
  G2_TRY(check_dynamics_binding(p->robot, y));
  G2_CHECK(y->device == p->device, GPMP2MI_ERR_INVALID, "the dynamics handle lives on another device than the plan");
  MotionLimitsDev lim;
  G2_TRY(read_limits(l, P.D, &lim));
  const size_t Md = (size_t)P.N * (inter + 1) + 1;
  RowOut rows[RETIME_DYN_ROWS];
  rows_of(out, Md, P.D, rows);
  const auto layout = [&](void* base) { return carve_retime_dyn((char*)base, rows, shape_of(p, inter)); };
  RetimeDynWs w;
  G2_TRY(carve_into(p->ws[p->WS_RETIME_DYN], layout, &w));
  RetimeDynOut o = sel ? RetimeDynOut{} : retime_dyn_out(rows, host);
  RetimeDynFinish f{};
  SelExtra x;
  int best_here = -1;
  RetimeDynSel s;
  if (sel) {   // a selection has no per-row outputs of its own: the rule reads the workspace's duration and status
    s = *sel;
    if (host && !s.best) s.best = &best_here;   // the torques of the chosen row are fetched behind finish_host
    o.duration = (double*)rows[3].staged;
    o.status = (int*)rows[6].staged;
    o.tau = (double*)rows[7].staged;
    RetimeFinish& q = f.rt;
    plan_shape(q.sel, p, inter);
    q.sel.lie = 0;   // the Pose2 kinds were refused above
    x.value = s.duration_best;
    x.row = s.stamps_best;
    x.row_bytes = Md * sizeof(double);
    const SelExtra k = point_selection(q.sel, p, s, &x, host, w.sel);
    q.duration_best = k.value;
    q.stamps_best = k.row;
    // the pick's extra row is [Md] stamps, then [Md][D] torques
    f.tau_best = host ? (s.tau_best ? w.sel.extra_row + Md : nullptr) : s.tau_best;
    q.required_self_clearance = s.required_self_clearance;
    q.required_pos_margin = s.required_pos_margin;
    q.max_duration = s.max_duration;
    q.rstatus = o.status;
    q.duration = o.duration;
    q.sdot = (double*)rows[0].staged;
    q.stamps = (double*)rows[2].staged;
    f.tau = o.tau;
    f.nonfinite = w.core.nonfinite;
    PriorRows got;
    G2_TRY(enqueue_prior_stages(p, s.pairs, inter, w.prior, st, &got));
    q.clearance = got.clearance;
    q.oor = got.oor;
    q.self_clearance = got.self_clearance;
    q.self_invalid = got.self_invalid;
    G2_TRY(gpmp2mi_plan_motion_score_dev(p, l, inter, w.prior.pos_margin, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         w.prior.motion_invalid, st));
    q.pos_margin = w.prior.pos_margin;
    q.motion_invalid = w.prior.motion_invalid;
  }
  p->mark_dirty(st);
  G2_TRY(enqueue_retime_dynamic(p->robot, y, lim, l->point_speed, P.delta_t, inter, P.B, P.N, p->pb.result, rt, w.core,
                                rows, o, st));
  if (sel) G2_TRY(launch_retime_dynamic_finish(f, st));
  if (!host) return GPMP2MI_OK;
  G2_TRY(finish_host(p, inter, rows, RETIME_DYN_ROWS, sel ? &s : nullptr, &x, w.sel, st));
  if (sel && s.tau_best && *s.best >= 0)
    G2_HIP(hipMemcpy(s.tau_best, w.sel.extra_row + Md, Md * P.D * sizeof(double), hipMemcpyDeviceToHost));
  return GPMP2MI_OK;
}

int check_traj_call(const gpmp2mi_robot* r, const gpmp2mi_dynamics* y, const gpmp2mi_motion_limits* l, double delta_t,
                    int inter, int B, int total_step, const double* traj, const RetimeRates& rt) {
  G2_CHECK(r && y && traj, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_limits_head(l));
  G2_TRY(check_retime_rates(rt));
  G2_TRY(check_score_args(inter, B, total_step, delta_t));
  G2_TRY(check_arm(r));
  return check_dynamics_binding(r, y);
}

// the rules of gpmp2mi_retime_path_affine beyond those of gpmp2mi_retime_path; bound [R] -> the kernel's [8]
int check_affine_call(int R, const double* cxl, const double* cxr, const double* cu, const double* off,
                      const double* bound, double* bound_out) {
  G2_CHECK(R >= 0 && R <= RETIME_DYN_MAX_ROWS, GPMP2MI_ERR_INVALID, "R outside 0..8");
  G2_CHECK(R == 0 || (cxl && cxr && cu && off && bound), GPMP2MI_ERR_INVALID, "null argument");
  for (int r = 0; r < RETIME_DYN_MAX_ROWS; r++) bound_out[r] = HUGE_VAL;
  for (int r = 0; r < R; r++) {
    G2_CHECK(bound[r] > 0, GPMP2MI_ERR_INVALID, "a bound is NaN or <= 0");   // false for NaN
    bound_out[r] = bound[r];
  }
  return GPMP2MI_OK;
}

RetimeDynOut make_out(double* sdot, double* u, double* stamps, double* duration, int* status, double* achieved,
                      double* dense, double* tau, double* coef) {
  RetimeDynOut o;
  o.sdot = sdot; o.u = u; o.stamps = stamps; o.duration = duration; o.status = status; o.achieved = achieved;
  o.dense = dense; o.tau = tau; o.coef = coef;
  return o;
}
RetimeDynSel make_sel(double required_clearance, int require_in_range, const gpmp2mi_self_pairs* pairs,
                      double required_self_clearance, double required_pos_margin, double max_duration, int* best,
                      int* n_eligible, double* duration_best, double* stamps_best, double* tau_best, double* traj_best,
                      double* dense_best) {
  RetimeDynSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.pairs = pairs; sel.required_self_clearance = required_self_clearance;
  sel.required_pos_margin = required_pos_margin; sel.max_duration = max_duration;
  sel.best = best; sel.n_eligible = n_eligible; sel.duration_best = duration_best; sel.stamps_best = stamps_best;
  sel.tau_best = tau_best; sel.traj_best = traj_best; sel.dense_best = dense_best;
  return sel;
}

}  // namespace

extern "C" {

int gpmp2mi_retime_path_affine_dev(int B, int Md, int dof, const double* qd, const double* qdd_left,
                                   const double* qdd_right, const double* cap, const double* acc, int R,
                                   const double* cx_left, const double* cx_right, const double* cu, const double* off,
                                   const double* bound, double h, double max_rate, double rate_start, double rate_end,
                                   double* sdot, double* u, double* stamps, double* duration, int* status,
                                   double* achieved, double* workspace, void* stream) {
  const RetimeRates rt{max_rate, rate_start, rate_end};
  RetimeDynArgs g{};
  RetimeArgs& a = g.rt;
  G2_TRY(check_retime_path_call(B, Md, dof, qd, qdd_left, qdd_right, cap, acc, h, rt, a.acc));
  G2_TRY(check_affine_call(R, cx_left, cx_right, cu, off, bound, g.bound));
  G2_CHECK(sdot && u && stamps && workspace, GPMP2MI_ERR_INVALID,
           "the device form needs sdot, u, stamps and a workspace of B Md (3 + 4 (2 dof + 2 R)) doubles");
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  a.B = B;
  a.Md = Md;
  a.D = dof;
  a.h = h;
  a.max_rate = max_rate;
  a.rate_start = rate_start;
  a.rate_end = rate_end;
  a.point_speed = HUGE_VAL;
  for (int d = 0; d < GPMP2MI_MAX_DOF; d++) a.vel[d] = HUGE_VAL;
  a.qd = qd;
  a.ql = qdd_left;
  a.qr = qdd_right;
  a.cap = cap;
  a.X = workspace;
  a.K = workspace + (size_t)B * Md;
  a.sdot = sdot;
  a.u = u;
  a.stamps = stamps;
  a.duration = duration;
  a.achieved = achieved;
  a.status = status;
  g.R = R;
  g.stride = R;
  g.cxl = cx_left;
  g.cxr = cx_right;
  g.cu = cu;
  g.off = off;
  g.rows = workspace + (size_t)3 * B * Md;
  return launch_retime_dynamic(g, false, (hipStream_t)stream);
}

int gpmp2mi_retime_path_affine(int B, int Md, int dof, const double* qd, const double* qdd_left, const double* qdd_right,
                               const double* cap, const double* acc, int R, const double* cx_left,
                               const double* cx_right, const double* cu, const double* off, const double* bound, double h,
                               double max_rate, double rate_start, double rate_end, double* sdot, double* u,
                               double* stamps, double* duration, int* status, double* achieved) {
  double acc_checked[GPMP2MI_MAX_DOF], bound_checked[RETIME_DYN_MAX_ROWS];
  G2_TRY(check_retime_path_call(B, Md, dof, qd, qdd_left, qdd_right, cap, acc, h,
                                RetimeRates{max_rate, rate_start, rate_end}, acc_checked));
  G2_TRY(check_affine_call(R, cx_left, cx_right, cu, off, bound, bound_checked));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const size_t n = (size_t)B * Md;
  DevBuf<double> dq, dl, dr, dc, dxl, dxr, dcu, dfo, ds, du, dt, dd, da, dw;
  DevBuf<int> di;
  G2_TRY(dq.upload(qd, n * dof));
  G2_TRY(dl.upload(qdd_left, n * dof));
  G2_TRY(dr.upload(qdd_right, n * dof));
  G2_TRY(dc.upload(cap, n));
  G2_TRY(dxl.upload(cx_left, n * R));
  G2_TRY(dxr.upload(cx_right, n * R));
  G2_TRY(dcu.upload(cu, n * R));
  G2_TRY(dfo.upload(off, n * R));
  G2_TRY(ds.out(sdot, n));
  G2_TRY(du.out(u, n));
  G2_TRY(dt.out(stamps, n));
  G2_TRY(dw.alloc(n * (3 + 4 * (2 * (size_t)dof + 2 * (size_t)R))));
  if (duration) G2_TRY(dd.out(duration, B));
  if (status) G2_TRY(di.out(status, B));
  if (achieved) G2_TRY(da.out(achieved, (size_t)6 * B));
  G2_TRY(gpmp2mi_retime_path_affine_dev(B, Md, dof, dq.p, dl.p, dr.p, dc.p, acc, R, dxl.p, dxr.p, dcu.p, dfo.p, bound, h,
                                        max_rate, rate_start, rate_end, ds.p, du.p, dt.p, dd.p, di.p, da.p, dw.p,
                                        nullptr));
  return fetch_all(ds, du, dt, dd, di, da);
}

int gpmp2mi_retime_dynamic_traj_dev(const gpmp2mi_robot* r, const gpmp2mi_dynamics* y, const gpmp2mi_motion_limits* l,
                                    double delta_t, int inter_step, int B, int total_step, const double* traj,
                                    double max_rate, double rate_start, double rate_end, double* sdot, double* u,
                                    double* stamps, double* duration, int* status, double* achieved,
                                    double* dense_retimed, double* tau_retimed, double* coef, void* stream) {
  const RetimeRates rt{max_rate, rate_start, rate_end};
  G2_TRY(check_traj_call(r, y, l, delta_t, inter_step, B, total_step, traj, rt));
  MotionLimitsDev lim;
  G2_TRY(read_limits(l, r->h.dof, &lim));
  if (B == 0) return GPMP2MI_OK;
  const size_t Md = (size_t)total_step * (inter_step + 1) + 1;
  const RetimeDynOut o = make_out(sdot, u, stamps, duration, status, achieved, dense_retimed, tau_retimed, coef);
  RowOut rows[RETIME_DYN_ROWS];
  rows_of(o, Md, r->h.dof, rows);
  Carver need{nullptr};
  (void)carve_retime_dyn_core(need, rows, B, Md, r->h.dof);
  G2_TRY(ensure_device());
  int cur = -1;
  G2_HIP(hipGetDevice(&cur));
  G2_CHECK(cur == r->device && cur == y->device, GPMP2MI_ERR_INVALID,
           "the robot handle or the dynamics handle lives on another device than the current one");
  std::unique_lock<std::mutex> lk(y->mu);
  G2_TRY(y->retime_ws.reserve(need.off));
  Carver take{(char*)y->retime_ws.p};
  const RetimeDynCore w = carve_retime_dyn_core(take, rows, B, Md, r->h.dof);
  return enqueue_retime_dynamic(r, y, lim, l->point_speed, delta_t, inter_step, B, total_step, traj, rt, w, rows, o,
                                (hipStream_t)stream);
}

int gpmp2mi_retime_dynamic_traj(const gpmp2mi_robot* r, const gpmp2mi_dynamics* y, const gpmp2mi_motion_limits* l,
                                double delta_t, int inter_step, int B, int total_step, const double* traj,
                                double max_rate, double rate_start, double rate_end, double* sdot, double* u,
                                double* stamps, double* duration, int* status, double* achieved, double* dense_retimed,
                                double* tau_retimed, double* coef) {
  G2_TRY(check_traj_call(r, y, l, delta_t, inter_step, B, total_step, traj, RetimeRates{max_rate, rate_start, rate_end}));
  MotionLimitsDev lim;
  G2_TRY(read_limits(l, r->h.dof, &lim));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const size_t D = r->h.dof, n = (size_t)B * ((size_t)total_step * (inter_step + 1) + 1);
  DevBuf<double> dtr, ds, du, dt, dd, da, de, dta, dco;
  DevBuf<int> di;
  G2_TRY(dtr.upload(traj, (size_t)B * (total_step + 1) * 2 * D));
  if (sdot) G2_TRY(ds.out(sdot, n));
  if (u) G2_TRY(du.out(u, n));
  if (stamps) G2_TRY(dt.out(stamps, n));
  if (duration) G2_TRY(dd.out(duration, B));
  if (status) G2_TRY(di.out(status, B));
  if (achieved) G2_TRY(da.out(achieved, (size_t)6 * B));
  if (dense_retimed) G2_TRY(de.out(dense_retimed, n * 2 * D));
  if (tau_retimed) G2_TRY(dta.out(tau_retimed, n * D));
  if (coef) G2_TRY(dco.out(coef, n * 4 * D));
  G2_TRY(gpmp2mi_retime_dynamic_traj_dev(r, y, l, delta_t, inter_step, B, total_step, dtr.p, max_rate, rate_start,
                                         rate_end, ds.p, du.p, dt.p, dd.p, di.p, da.p, de.p, dta.p, dco.p, nullptr));
  return fetch_all(ds, du, dt, dd, di, da, de, dta, dco);
}

int gpmp2mi_plan_retime_dynamic(gpmp2mi_plan* p, const gpmp2mi_dynamics* y, const gpmp2mi_motion_limits* l,
                                int inter_step, double max_rate, double rate_start, double rate_end, double* sdot,
                                double* u, double* stamps, double* duration, int* status, double* achieved,
                                double* dense_retimed, double* tau_retimed, double* coef) {
  return plan_retime_dynamic(p, y, l, inter_step, RetimeRates{max_rate, rate_start, rate_end},
                             make_out(sdot, u, stamps, duration, status, achieved, dense_retimed, tau_retimed, coef),
                             nullptr, true, nullptr);
}
int gpmp2mi_plan_retime_dynamic_dev(gpmp2mi_plan* p, const gpmp2mi_dynamics* y, const gpmp2mi_motion_limits* l,
                                    int inter_step, double max_rate, double rate_start, double rate_end, double* sdot,
                                    double* u, double* stamps, double* duration, int* status, double* achieved,
                                    double* dense_retimed, double* tau_retimed, double* coef, void* stream) {
  return plan_retime_dynamic(p, y, l, inter_step, RetimeRates{max_rate, rate_start, rate_end},
                             make_out(sdot, u, stamps, duration, status, achieved, dense_retimed, tau_retimed, coef),
                             nullptr, false, (hipStream_t)stream);
}

int gpmp2mi_plan_select_retimed_dynamic(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                        const gpmp2mi_self_pairs* pairs, double required_self_clearance,
                                        const gpmp2mi_motion_limits* l, double required_pos_margin, double max_rate,
                                        double rate_start, double rate_end, double max_duration,
                                        const gpmp2mi_dynamics* y, int* best, int* n_eligible, double* duration_best,
                                        double* stamps_best, double* tau_best, double* traj_best, double* dense_best) {
  const RetimeDynSel sel = make_sel(required_clearance, require_in_range, pairs, required_self_clearance,
                                    required_pos_margin, max_duration, best, n_eligible, duration_best, stamps_best,
                                    tau_best, traj_best, dense_best);
  return plan_retime_dynamic(p, y, l, inter_step, RetimeRates{max_rate, rate_start, rate_end}, RetimeDynOut{}, &sel, true,
                             nullptr);
}
int gpmp2mi_plan_select_retimed_dynamic_dev(gpmp2mi_plan* p, int inter_step, double required_clearance,
                                            int require_in_range, const gpmp2mi_self_pairs* pairs,
                                            double required_self_clearance, const gpmp2mi_motion_limits* l,
                                            double required_pos_margin, double max_rate, double rate_start,
                                            double rate_end, double max_duration, const gpmp2mi_dynamics* y, int* best,
                                            int* n_eligible, double* duration_best, double* stamps_best, double* tau_best,
                                            double* traj_best, double* dense_best, void* stream) {
  const RetimeDynSel sel = make_sel(required_clearance, require_in_range, pairs, required_self_clearance,
                                    required_pos_margin, max_duration, best, n_eligible, duration_best, stamps_best,
                                    tau_best, traj_best, dense_best);
  return plan_retime_dynamic(p, y, l, inter_step, RetimeRates{max_rate, rate_start, rate_end}, RetimeDynOut{}, &sel,
                             false, (hipStream_t)stream);
}

}  // extern "C"
