// retime.hip -- the speed profile of the executed trajectory (include/gpmp2mi.h "re-timing"): the bare rule on caller
// arrays, the profile for caller trajectories and for a plan's resident result, and the selection that asks for the
// re-timed duration.  Kernels: retime_kernels.hip; the rule: retime_rule.h.  The obstacle, self-collision and motion sides
// of select_retimed are the existing stages, enqueued ahead with their per-row outputs in this unit's workspace.
#include <cmath>

#include "../retime_rule.h"
#include "host.h"

using namespace g2;

static_assert(GPMP2MI_RETIME_OK == RETIME_OK && GPMP2MI_RETIME_BOUNDARY == RETIME_BOUNDARY &&
                  GPMP2MI_RETIME_EMPTY == RETIME_EMPTY && GPMP2MI_RETIME_INVALID == RETIME_INVALID,
              "retime_rule.h states the values of GPMP2MI_RETIME_*");

namespace {

struct Rates {
  double max_rate, rate_start, rate_end;
};
int check_rates(const Rates& r) {
  G2_CHECK(!std::isnan(r.max_rate) && !std::isnan(r.rate_start) && !std::isnan(r.rate_end), GPMP2MI_ERR_INVALID,
           "max_rate / rate_start / rate_end is NaN");
  G2_CHECK(r.max_rate > 0 && std::isfinite(r.max_rate), GPMP2MI_ERR_INVALID, "max_rate must be finite and > 0");
  return GPMP2MI_OK;
}
int check_kind(const gpmp2mi_robot* r) {
  G2_CHECK(r->h.kind < GPMP2MI_ROBOT_POSE2_MOBILE_BASE, GPMP2MI_ERR_UNSUPPORTED,
           "re-timing is not built for the Pose2 kinds: the acceleration of the tangent-space interpolation is missing");
  return GPMP2MI_OK;
}

// k_retime_caps, then k_retime over `traj`; o: device pointers, a null sdot / u / stamps takes the workspace's (the
// first rows of `rows`, carved with `w`)
int enqueue_retime(const gpmp2mi_robot* r, const MotionLimitsDev& lim, double point_speed, double dt, int inter, int B,
                   int N, const double* traj, const Rates& rt, const RetimeCore& w, const RowOut* rows, const RetimeOut& o,
                   hipStream_t st) {
  RetimeArgs a{};
  a.B = B;
  a.N = N;
  a.inter = inter;
  a.Md = N * (inter + 1) + 1;
  a.D = r->h.dof;
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
  a.ps = w.ps;
  a.X = w.X;
  a.K = w.K;
  a.sdot = o.sdot ? o.sdot : (double*)rows[0].staged;
  a.u = o.u ? o.u : (double*)rows[1].staged;
  a.stamps = o.stamps ? o.stamps : (double*)rows[2].staged;
  a.duration = o.duration;
  a.achieved = o.achieved;
  a.dense = o.dense;
  a.status = o.status;
  G2_TRY(launch_retime_caps(r->h, r->d, dt, inter, B, N, traj, w.ps, st));
  return launch_retime(a, true, st);
}

struct RetimeSel : ScoreSel {
  double required_self_clearance = 0.0, required_pos_margin = 0.0, max_duration = 0.0;
  const gpmp2mi_self_pairs* pairs = nullptr;
  double *duration_best = nullptr, *stamps_best = nullptr;
};

// Re-times the plan's resident result on `st`; sel != null: the existing stages for the same rows first, then the rule
// and the copy of the chosen row.  host / out / sel as plan_score (score.hip).
int plan_retime(gpmp2mi_plan* p, const gpmp2mi_motion_limits* l, int inter, const Rates& rt, const RetimeOut& out,
                const RetimeSel* sel, bool host, hipStream_t st) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_TRY(check_limits_head(l));
  G2_TRY(check_rates(rt));
  if (sel)
    G2_CHECK(!std::isnan(sel->required_pos_margin) && !std::isnan(sel->max_duration), GPMP2MI_ERR_INVALID,
             "required_pos_margin / max_duration is NaN");
  G2_TRY(check_plan_ready(p, inter));
  const PlanParams& P = p->hp;
  G2_TRY(check_kind(p->robot));
  MotionLimitsDev lim;
  G2_TRY(read_limits(l, P.D, &lim));
  const size_t Md = (size_t)P.N * (inter + 1) + 1;
  RowOut rows[RETIME_ROWS];
  rows_of(out, Md, P.D, rows);
  const auto layout = [&](void* base) { return carve_retime((char*)base, rows, shape_of(p, inter)); };
  RetimeWs w;
  G2_TRY(carve_into(p->ws[p->WS_RETIME], layout, &w));
  RetimeOut o = sel ? RetimeOut{} : retime_out(rows, host);
  RetimeFinish f{};
  SelExtra x;
  if (sel) {   // a selection has no per-row outputs of its own: the rule reads the workspace's duration and status
    o.duration = (double*)rows[3].staged;
    o.status = (int*)rows[6].staged;
    plan_shape(f.sel, p, inter);
    f.sel.lie = 0;   // the Pose2 kinds were refused above
    x.value = sel->duration_best;
    x.row = sel->stamps_best;
    x.row_bytes = Md * sizeof(double);
    const SelExtra k = point_selection(f.sel, p, *sel, &x, host, w.sel);
    f.duration_best = k.value;
    f.stamps_best = k.row;
    f.required_self_clearance = sel->required_self_clearance;
    f.required_pos_margin = sel->required_pos_margin;
    f.max_duration = sel->max_duration;
    f.rstatus = o.status;
    f.duration = o.duration;
    f.sdot = (double*)rows[0].staged;
    f.stamps = (double*)rows[2].staged;
    PriorRows got;
    G2_TRY(enqueue_prior_stages(p, sel->pairs, inter, w.prior, st, &got));
    f.clearance = got.clearance;
    f.oor = got.oor;
    f.self_clearance = got.self_clearance;
    f.self_invalid = got.self_invalid;
    G2_TRY(gpmp2mi_plan_motion_score_dev(p, l, inter, w.prior.pos_margin, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         w.prior.motion_invalid, st));
    f.pos_margin = w.prior.pos_margin;
    f.motion_invalid = w.prior.motion_invalid;
  }
  p->mark_dirty(st);
  G2_TRY(enqueue_retime(p->robot, lim, l->point_speed, P.delta_t, inter, P.B, P.N, p->pb.result, rt, w.core, rows, o, st));
  if (sel) G2_TRY(launch_retime_finish(f, st));
  return host ? finish_host(p, inter, rows, RETIME_ROWS, sel, &x, w.sel, st) : GPMP2MI_OK;
}

int check_traj_call(const gpmp2mi_robot* r, const gpmp2mi_motion_limits* l, double delta_t, int inter, int B,
                    int total_step, const double* traj, const Rates& rt) {
  G2_CHECK(r && traj, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_limits_head(l));
  G2_TRY(check_rates(rt));
  G2_TRY(check_score_args(inter, B, total_step, delta_t));
  return check_kind(r);
}

// the rules of gpmp2mi_retime_path; acc [D] or null -> the kernel's [GPMP2MI_MAX_DOF]
int check_path_call(int B, int Md, int dof, const double* qd, const double* ql, const double* qr, const double* cap,
                    const double* acc, double h, const Rates& rt, double* acc_out) {
  G2_CHECK(qd && ql && qr && cap, GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK(B >= 0, GPMP2MI_ERR_INVALID, "B must be >= 0");
  G2_CHECK(Md >= 2, GPMP2MI_ERR_INVALID, "a path has at least two states");
  G2_CHECK(dof >= 1 && dof <= GPMP2MI_MAX_DOF, GPMP2MI_ERR_INVALID, "dof outside 1..GPMP2MI_MAX_DOF");
  G2_CHECK((long long)Md * dof * std::max(B, 1) < (1ll << 31), GPMP2MI_ERR_INVALID, "too many states for one launch");
  G2_CHECK(h > 0 && std::isfinite(h), GPMP2MI_ERR_INVALID, "h must be finite and > 0");
  G2_TRY(check_rates(rt));
  for (int d = 0; d < GPMP2MI_MAX_DOF; d++) acc_out[d] = HUGE_VAL;
  if (acc)
    for (int d = 0; d < dof; d++) {
      G2_CHECK(acc[d] > 0, GPMP2MI_ERR_INVALID, "an acceleration limit is NaN or <= 0");
      acc_out[d] = acc[d];
    }
  return GPMP2MI_OK;
}

RetimeOut make_out(double* sdot, double* u, double* stamps, double* duration, int* status, double* achieved,
                   double* dense) {
  RetimeOut o;
  o.sdot = sdot; o.u = u; o.stamps = stamps; o.duration = duration; o.status = status; o.achieved = achieved;
  o.dense = dense;
  return o;
}
RetimeSel make_sel(double required_clearance, int require_in_range, const gpmp2mi_self_pairs* pairs,
                   double required_self_clearance, double required_pos_margin, double max_duration, int* best,
                   int* n_eligible, double* duration_best, double* stamps_best, double* traj_best, double* dense_best) {
  RetimeSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.pairs = pairs; sel.required_self_clearance = required_self_clearance;
  sel.required_pos_margin = required_pos_margin; sel.max_duration = max_duration;
  sel.best = best; sel.n_eligible = n_eligible; sel.duration_best = duration_best; sel.stamps_best = stamps_best;
  sel.traj_best = traj_best; sel.dense_best = dense_best;
  return sel;
}

}  // namespace

// what retime_dynamic.hip shares (host.h)
int g2::check_retime_rates(const RetimeRates& r) { return check_rates(Rates{r.max_rate, r.rate_start, r.rate_end}); }
int g2::check_retime_path_call(int B, int Md, int dof, const double* qd, const double* ql, const double* qr,
                               const double* cap, const double* acc, double h, const RetimeRates& rt, double* acc_out) {
  return check_path_call(B, Md, dof, qd, ql, qr, cap, acc, h, Rates{rt.max_rate, rt.rate_start, rt.rate_end}, acc_out);
}

extern "C" {

int gpmp2mi_retime_path_dev(int B, int Md, int dof, const double* qd, const double* qdd_left, const double* qdd_right,
                            const double* cap, const double* acc, double h, double max_rate, double rate_start,
                            double rate_end, double* sdot, double* u, double* stamps, double* duration, int* status,
                            double* achieved, double* workspace, void* stream) {
  const Rates rt{max_rate, rate_start, rate_end};
  RetimeArgs a{};
  G2_TRY(check_path_call(B, Md, dof, qd, qdd_left, qdd_right, cap, acc, h, rt, a.acc));
  G2_CHECK(sdot && u && stamps && workspace, GPMP2MI_ERR_INVALID,
           "the device form needs sdot, u, stamps and a workspace of 3 B Md doubles");
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
  return launch_retime(a, false, (hipStream_t)stream);
}

int gpmp2mi_retime_path(int B, int Md, int dof, const double* qd, const double* qdd_left, const double* qdd_right,
                        const double* cap, const double* acc, double h, double max_rate, double rate_start,
                        double rate_end, double* sdot, double* u, double* stamps, double* duration, int* status,
                        double* achieved) {
  double acc_checked[GPMP2MI_MAX_DOF];
  G2_TRY(check_path_call(B, Md, dof, qd, qdd_left, qdd_right, cap, acc, h, Rates{max_rate, rate_start, rate_end},
                         acc_checked));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const size_t n = (size_t)B * Md;
  DevBuf<double> dq, dl, dr, dc, ds, du, dt, dd, da, dw;
  DevBuf<int> di;
  G2_TRY(dq.upload(qd, n * dof));
  G2_TRY(dl.upload(qdd_left, n * dof));
  G2_TRY(dr.upload(qdd_right, n * dof));
  G2_TRY(dc.upload(cap, n));
  G2_TRY(ds.out(sdot, n));
  G2_TRY(du.out(u, n));
  G2_TRY(dt.out(stamps, n));
  G2_TRY(dw.alloc(3 * n));
  if (duration) G2_TRY(dd.out(duration, B));
  if (status) G2_TRY(di.out(status, B));
  if (achieved) G2_TRY(da.out(achieved, (size_t)4 * B));
  G2_TRY(gpmp2mi_retime_path_dev(B, Md, dof, dq.p, dl.p, dr.p, dc.p, acc, h, max_rate, rate_start, rate_end, ds.p, du.p,
                                 dt.p, dd.p, di.p, da.p, dw.p, nullptr));
  return fetch_all(ds, du, dt, dd, di, da);
}

int gpmp2mi_retime_traj_dev(const gpmp2mi_robot* r, const gpmp2mi_motion_limits* l, double delta_t, int inter_step, int B,
                            int total_step, const double* traj, double max_rate, double rate_start, double rate_end,
                            double* sdot, double* u, double* stamps, double* duration, int* status, double* achieved,
                            double* dense_retimed, void* stream) {
  const Rates rt{max_rate, rate_start, rate_end};
  G2_TRY(check_traj_call(r, l, delta_t, inter_step, B, total_step, traj, rt));
  MotionLimitsDev lim;
  G2_TRY(read_limits(l, r->h.dof, &lim));
  if (B == 0) return GPMP2MI_OK;
  const size_t Md = (size_t)total_step * (inter_step + 1) + 1;
  const RetimeOut o = make_out(sdot, u, stamps, duration, status, achieved, dense_retimed);
  RowOut rows[RETIME_ROWS];
  rows_of(o, Md, r->h.dof, rows);
  Carver need{nullptr};
  (void)carve_retime_core(need, rows, B, Md);
  std::unique_lock<std::mutex> lk;
  G2_TRY(records_ready(r, nullptr, r->retime_ws, need.off, lk));
  Carver take{(char*)r->retime_ws.p};
  const RetimeCore w = carve_retime_core(take, rows, B, Md);
  return enqueue_retime(r, lim, l->point_speed, delta_t, inter_step, B, total_step, traj, rt, w, rows, o,
                        (hipStream_t)stream);
}

int gpmp2mi_retime_traj(const gpmp2mi_robot* r, const gpmp2mi_motion_limits* l, double delta_t, int inter_step, int B,
                        int total_step, const double* traj, double max_rate, double rate_start, double rate_end,
                        double* sdot, double* u, double* stamps, double* duration, int* status, double* achieved,
                        double* dense_retimed) {
  G2_TRY(check_traj_call(r, l, delta_t, inter_step, B, total_step, traj, Rates{max_rate, rate_start, rate_end}));
  MotionLimitsDev lim;
  G2_TRY(read_limits(l, r->h.dof, &lim));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const size_t n = (size_t)B * ((size_t)total_step * (inter_step + 1) + 1);
  DevBuf<double> dtr, ds, du, dt, dd, da, de;
  DevBuf<int> di;
  G2_TRY(dtr.upload(traj, (size_t)B * (total_step + 1) * 2 * r->h.dof));
  if (sdot) G2_TRY(ds.out(sdot, n));
  if (u) G2_TRY(du.out(u, n));
  if (stamps) G2_TRY(dt.out(stamps, n));
  if (duration) G2_TRY(dd.out(duration, B));
  if (status) G2_TRY(di.out(status, B));
  if (achieved) G2_TRY(da.out(achieved, (size_t)4 * B));
  if (dense_retimed) G2_TRY(de.out(dense_retimed, n * 2 * r->h.dof));
  G2_TRY(gpmp2mi_retime_traj_dev(r, l, delta_t, inter_step, B, total_step, dtr.p, max_rate, rate_start, rate_end, ds.p,
                                 du.p, dt.p, dd.p, di.p, da.p, de.p, nullptr));
  return fetch_all(ds, du, dt, dd, di, da, de);
}

int gpmp2mi_plan_retime(gpmp2mi_plan* p, const gpmp2mi_motion_limits* l, int inter_step, double max_rate,
                        double rate_start, double rate_end, double* sdot, double* u, double* stamps, double* duration,
                        int* status, double* achieved, double* dense_retimed) {
  return plan_retime(p, l, inter_step, Rates{max_rate, rate_start, rate_end},
                     make_out(sdot, u, stamps, duration, status, achieved, dense_retimed), nullptr, true, nullptr);
}
int gpmp2mi_plan_retime_dev(gpmp2mi_plan* p, const gpmp2mi_motion_limits* l, int inter_step, double max_rate,
                            double rate_start, double rate_end, double* sdot, double* u, double* stamps,
                            double* duration, int* status, double* achieved, double* dense_retimed, void* stream) {
  return plan_retime(p, l, inter_step, Rates{max_rate, rate_start, rate_end},
                     make_out(sdot, u, stamps, duration, status, achieved, dense_retimed), nullptr, false,
                     (hipStream_t)stream);
}

int gpmp2mi_plan_select_retimed(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                const gpmp2mi_self_pairs* pairs, double required_self_clearance,
                                const gpmp2mi_motion_limits* l, double required_pos_margin, double max_rate,
                                double rate_start, double rate_end, double max_duration, int* best, int* n_eligible,
                                double* duration_best, double* stamps_best, double* traj_best, double* dense_best) {
  const RetimeSel sel = make_sel(required_clearance, require_in_range, pairs, required_self_clearance, required_pos_margin,
                                 max_duration, best, n_eligible, duration_best, stamps_best, traj_best, dense_best);
  return plan_retime(p, l, inter_step, Rates{max_rate, rate_start, rate_end}, RetimeOut{}, &sel, true, nullptr);
}
int gpmp2mi_plan_select_retimed_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                    const gpmp2mi_self_pairs* pairs, double required_self_clearance,
                                    const gpmp2mi_motion_limits* l, double required_pos_margin, double max_rate,
                                    double rate_start, double rate_end, double max_duration, int* best,
                                    int* n_eligible, double* duration_best, double* stamps_best, double* traj_best,
                                    double* dense_best, void* stream) {
  const RetimeSel sel = make_sel(required_clearance, require_in_range, pairs, required_self_clearance, required_pos_margin,
                                 max_duration, best, n_eligible, duration_best, stamps_best, traj_best, dense_best);
  return plan_retime(p, l, inter_step, Rates{max_rate, rate_start, rate_end}, RetimeOut{}, &sel, false,
                     (hipStream_t)stream);
}

}  // extern "C"
