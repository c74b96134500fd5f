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

struct RetimeOut {
  double *sdot = nullptr, *u = nullptr, *stamps = nullptr, *duration = nullptr, *achieved = nullptr, *dense = nullptr;
  int* status = nullptr;
};

// what k_retime_caps and k_retime need for (B, Md), whoever keeps it: ps and X [B][Md], K [B][Md][2], then the profile
struct CoreWs {
  double *ps, *X, *K, *sdot, *u, *stamps;
};
template <class Take>
CoreWs core_layout(Take&& take, int B, size_t Md) {
  CoreWs w;
  w.ps = (double*)take(B * Md * sizeof(double));
  w.X = (double*)take(B * Md * sizeof(double));
  w.K = (double*)take(2 * B * Md * sizeof(double));
  w.sdot = (double*)take(B * Md * sizeof(double));
  w.u = (double*)take(B * Md * sizeof(double));
  w.stamps = (double*)take(B * Md * sizeof(double));
  return w;
}
struct Carver {
  char* base;
  size_t off = 0;
  char* operator()(size_t bytes) {
    char* p = base + off;
    off += ws_round(bytes);
    return p;
  }
};

// k_retime_caps, then k_retime over `traj`; o: device pointers, a null sdot / u / stamps takes the workspace's
int enqueue_retime(const gpmp2mi_robot* r, const MotionLimitsDev& lim, double point_speed, double dt, int inter, int B,
                   int N, const double* traj, const Rates& rt, const CoreWs& w, const RetimeOut& o, hipStream_t st) {
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
  a.sdot = o.sdot ? o.sdot : w.sdot;
  a.u = o.u ? o.u : w.u;
  a.stamps = o.stamps ? o.stamps : w.stamps;
  a.duration = o.duration;
  a.achieved = o.achieved;
  a.dense = o.dense;
  a.status = o.status;
  G2_TRY(launch_retime_caps(r->h, r->d, dt, inter, B, N, traj, w.ps, st));
  return launch_retime(a, true, st);
}

struct RetimeSel {
  double required_clearance = 0.0, required_self_clearance = 0.0, required_pos_margin = 0.0, max_duration = 0.0;
  int require_in_range = 0;
  const gpmp2mi_self_pairs* pairs = nullptr;
  int *best = nullptr, *n_eligible = nullptr;
  double *duration_best = nullptr, *stamps_best = nullptr, *traj_best = nullptr, *dense_best = nullptr;
};

// Layout of a plan's re-timing workspace for (B, N, D, inter): the core, the per-row results, the per-row scores of the
// existing stages, then the staging of the host-pointer forms
struct PlanRetimeWs {
  CoreWs core;
  double *duration, *achieved, *dense;
  int* status;
  double *clearance, *self_clearance, *pos_margin;
  int *oor, *self_invalid, *motion_invalid;
  char* pick;   // best, n_eligible, then the chosen row's final_error and duration: one 24-byte copy
  double *traj_best, *dense_best, *stamps_best;
  size_t bytes;
};
PlanRetimeWs plan_ws_layout(char* base, int B, int N, int D, int inter) {
  const size_t Md = (size_t)N * (inter + 1) + 1;
  PlanRetimeWs w{};
  Carver take{base};
  w.core = core_layout(take, B, Md);
  w.duration = (double*)take(B * sizeof(double));
  w.achieved = (double*)take((size_t)4 * B * sizeof(double));
  w.dense = (double*)take(B * Md * 2 * D * sizeof(double));
  w.status = (int*)take(B * sizeof(int));
  w.clearance = (double*)take(B * sizeof(double));
  w.self_clearance = (double*)take(B * sizeof(double));
  w.pos_margin = (double*)take(B * sizeof(double));
  w.oor = (int*)take(B * sizeof(int));
  w.self_invalid = (int*)take(B * sizeof(int));
  w.motion_invalid = (int*)take(B * sizeof(int));
  w.pick = take(2 * sizeof(int) + 2 * sizeof(double));
  w.traj_best = (double*)take((size_t)(N + 1) * 2 * D * sizeof(double));
  w.dense_best = (double*)take(Md * 2 * D * sizeof(double));
  w.stamps_best = (double*)take(Md * sizeof(double));
  w.bytes = take.off;
  return w;
}

struct Pick {
  int best, n;
  double err, duration;
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
  G2_PLAN_LIVE(p);   // before anything is enqueued
  G2_CHECK(p->optimized, GPMP2MI_ERR_INVALID, "plan has not been optimized");
  const PlanParams& P = p->hp;
  G2_TRY(check_score_args(inter, P.B, P.N, P.delta_t));
  G2_CHECK(p->robot->h.dof == P.D, GPMP2MI_ERR_INVALID, "robot dof does not fit the plan");
  G2_TRY(check_kind(p->robot));
  MotionLimitsDev lim;
  G2_TRY(read_limits(l, P.D, &lim));
  G2_TRY(ws_reserve(&p->retime_ws, &p->retime_ws_bytes, plan_ws_layout(nullptr, P.B, P.N, P.D, inter).bytes));
  const PlanRetimeWs w = plan_ws_layout((char*)p->retime_ws, P.B, P.N, P.D, inter);
  const size_t Md = (size_t)P.N * (inter + 1) + 1;
  Pick* pick = (Pick*)w.pick;
  RetimeOut o;
  if (sel) {   // the rule reads the workspace's
    o.duration = w.duration;
    o.status = w.status;
  } else if (host) {   // the host form computes only what the caller asked for
    o.duration = out.duration ? w.duration : nullptr;
    o.achieved = out.achieved ? w.achieved : nullptr;
    o.dense = out.dense ? w.dense : nullptr;
    o.status = out.status ? w.status : nullptr;
  } else {
    o = out;
  }
  RetimeFinish f{};
  if (sel) {
    ScoreFinish& g = f.sel;
    g.B = P.B;
    g.N = P.N;
    g.D = P.D;
    g.lie = 0;
    g.inter = inter;
    g.Md = (int)Md;
    g.dt = P.delta_t;
    g.traj = p->pb.result;
    g.select = 1;
    g.required_clearance = sel->required_clearance;
    g.require_in_range = sel->require_in_range;
    g.ferr = p->pb.final_err;
    g.status = p->pb.status;
    // the kernel reads `best` back for the chosen row's outputs: a device form without one gets the workspace's
    g.best = (host || !sel->best) ? &pick->best : sel->best;
    g.n_eligible = host ? &pick->n : sel->n_eligible;
    g.best_err = host ? &pick->err : nullptr;
    g.traj_best = host ? (sel->traj_best ? w.traj_best : nullptr) : sel->traj_best;
    g.dense_best = host ? (sel->dense_best ? w.dense_best : nullptr) : sel->dense_best;
    f.duration_best = host ? &pick->duration : sel->duration_best;
    f.stamps_best = host ? (sel->stamps_best ? w.stamps_best : nullptr) : sel->stamps_best;
    f.required_self_clearance = sel->required_self_clearance;
    f.required_pos_margin = sel->required_pos_margin;
    f.max_duration = sel->max_duration;
    f.rstatus = w.status;
    f.duration = w.duration;
    f.sdot = w.core.sdot;
    f.stamps = w.core.stamps;
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
    G2_TRY(gpmp2mi_plan_motion_score_dev(p, l, inter, w.pos_margin, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         w.motion_invalid, st));
    f.pos_margin = w.pos_margin;
    f.motion_invalid = w.motion_invalid;
  }
  p->mark_dirty(st);
  G2_TRY(enqueue_retime(p->robot, lim, l->point_speed, P.delta_t, inter, P.B, P.N, p->pb.result, rt, w.core, o, st));
  if (sel) G2_TRY(launch_retime_finish(f, st));
  if (!host) return GPMP2MI_OK;
  auto back = [&](void* dst, const void* src, size_t bytes) -> int {
    if (dst) G2_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    return GPMP2MI_OK;
  };
  if (!sel) {
    G2_TRY(back(out.sdot, w.core.sdot, P.B * Md * sizeof(double)));
    G2_TRY(back(out.u, w.core.u, P.B * Md * sizeof(double)));
    G2_TRY(back(out.stamps, w.core.stamps, P.B * Md * sizeof(double)));
    G2_TRY(back(out.duration, w.duration, P.B * sizeof(double)));
    G2_TRY(back(out.status, w.status, P.B * sizeof(int)));
    G2_TRY(back(out.achieved, w.achieved, (size_t)4 * P.B * sizeof(double)));
    G2_TRY(back(out.dense, w.dense, P.B * Md * 2 * P.D * sizeof(double)));
  }
  Pick got{-1, 0, 0.0, 0.0};
  if (sel) G2_TRY(back(&got, w.pick, sizeof(got)));
  G2_HIP(hipStreamSynchronize(st));
  if (sel) {
    if (sel->best) *sel->best = got.best;
    if (sel->n_eligible) *sel->n_eligible = got.n;
    if (got.best >= 0) {   // nothing chosen: the outputs about the chosen row stay as they are
      if (sel->duration_best) *sel->duration_best = got.duration;
      if (sel->traj_best || sel->dense_best || sel->stamps_best) {
        G2_TRY(back(sel->traj_best, w.traj_best, (size_t)(P.N + 1) * 2 * P.D * sizeof(double)));
        G2_TRY(back(sel->dense_best, w.dense_best, Md * 2 * P.D * sizeof(double)));
        G2_TRY(back(sel->stamps_best, w.stamps_best, Md * sizeof(double)));
        G2_HIP(hipStreamSynchronize(st));
      }
    }
  }
  p->mark_clean(st);
  return GPMP2MI_OK;
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

}  // namespace

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
  G2_TRY(ensure_device());
  int cur = -1;
  G2_HIP(hipGetDevice(&cur));
  G2_CHECK(cur == r->device, GPMP2MI_ERR_INVALID, "the robot handle lives on another device than the current one");
  const size_t Md = (size_t)total_step * (inter_step + 1) + 1;
  std::lock_guard<std::mutex> lk(r->score_mu);
  Carver need{nullptr};
  (void)core_layout(need, B, Md);
  G2_TRY(ws_reserve(&r->retime_ws, &r->retime_ws_bytes, need.off));
  Carver take{(char*)r->retime_ws};
  const CoreWs w = core_layout(take, B, Md);
  RetimeOut o;
  o.sdot = sdot; o.u = u; o.stamps = stamps; o.duration = duration; o.status = status; o.achieved = achieved;
  o.dense = dense_retimed;
  return enqueue_retime(r, lim, l->point_speed, delta_t, inter_step, B, total_step, traj, rt, w, o, (hipStream_t)stream);
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
  RetimeOut o;
  o.sdot = sdot; o.u = u; o.stamps = stamps; o.duration = duration; o.status = status; o.achieved = achieved;
  o.dense = dense_retimed;
  return plan_retime(p, l, inter_step, Rates{max_rate, rate_start, rate_end}, o, nullptr, true, nullptr);
}
int gpmp2mi_plan_retime_dev(gpmp2mi_plan* p, const gpmp2mi_motion_limits* l, int inter_step, double max_rate,
                            double rate_start, double rate_end, double* sdot, double* u, double* stamps,
                            double* duration, int* status, double* achieved, double* dense_retimed, void* stream) {
  RetimeOut o;
  o.sdot = sdot; o.u = u; o.stamps = stamps; o.duration = duration; o.status = status; o.achieved = achieved;
  o.dense = dense_retimed;
  return plan_retime(p, l, inter_step, Rates{max_rate, rate_start, rate_end}, o, nullptr, false, (hipStream_t)stream);
}

int gpmp2mi_plan_select_retimed(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                const gpmp2mi_self_pairs* pairs, double required_self_clearance,
                                const gpmp2mi_motion_limits* l, double required_pos_margin, double max_rate,
                                double rate_start, double rate_end, double max_duration, int* best, int* n_eligible,
                                double* duration_best, double* stamps_best, double* traj_best, double* dense_best) {
  RetimeSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.pairs = pairs; sel.required_self_clearance = required_self_clearance;
  sel.required_pos_margin = required_pos_margin; sel.max_duration = max_duration;
  sel.best = best; sel.n_eligible = n_eligible; sel.duration_best = duration_best; sel.stamps_best = stamps_best;
  sel.traj_best = traj_best; sel.dense_best = dense_best;
  return plan_retime(p, l, inter_step, Rates{max_rate, rate_start, rate_end}, RetimeOut{}, &sel, true, nullptr);
}
int gpmp2mi_plan_select_retimed_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                    const gpmp2mi_self_pairs* pairs, double required_self_clearance,
                                    const gpmp2mi_motion_limits* l, double required_pos_margin, double max_rate,
                                    double rate_start, double rate_end, double max_duration, int* best,
                                    int* n_eligible, double* duration_best, double* stamps_best, double* traj_best,
                                    double* dense_best, void* stream) {
  RetimeSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.pairs = pairs; sel.required_self_clearance = required_self_clearance;
  sel.required_pos_margin = required_pos_margin; sel.max_duration = max_duration;
  sel.best = best; sel.n_eligible = n_eligible; sel.duration_best = duration_best; sel.stamps_best = stamps_best;
  sel.traj_best = traj_best; sel.dense_best = dense_best;
  return plan_retime(p, l, inter_step, Rates{max_rate, rate_start, rate_end}, RetimeOut{}, &sel, false,
                     (hipStream_t)stream);
}

}  // extern "C"
