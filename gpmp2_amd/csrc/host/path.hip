// path.hip -- workspace path (include/gpmp2mi.h "workspace path"): the plan's resident path, the factor-level entry
// point, the check of the executed trajectory for caller buffers and for a plan's resident result, and the selection
// that asks for the deviations as well.  Kernels: path_kernels.hip; the factor inside a plan is launched by
// plan_linearize (plan_run.hip).  The obstacle side of select_path is the existing stage (plan_score), enqueued ahead
// with its per-row outputs in this unit's workspace.
#include <cmath>

#include "host.h"

using namespace g2;

namespace {

constexpr double kPi = 3.14159265358979323846;

int check_mode_link(const gpmp2mi_robot* r, int mode, int link) {
  G2_CHECK(mode >= GPMP2MI_WORKSPACE_POSITION && mode <= GPMP2MI_WORKSPACE_POSE, GPMP2MI_ERR_INVALID, "unknown mode");
  G2_CHECK(link >= 0 && link < r->h.nr_links, GPMP2MI_ERR_INVALID, "link out of range");
  return GPMP2MI_OK;
}

// angle of Ra^T Rb (row-major 4x4 poses), from the antisymmetric part and the trace: well conditioned up to pi
double relative_angle(const double* Ta, const double* Tb) {
  double Rr[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double a = 0;
      for (int c = 0; c < 3; c++) a += Ta[c * 4 + i] * Tb[c * 4 + j];
      Rr[i * 3 + j] = a;
    }
  const double sx = Rr[7] - Rr[5], sy = Rr[2] - Rr[6], sz = Rr[3] - Rr[1];
  return std::atan2(0.5 * std::sqrt(sx * sx + sy * sy + sz * sz), 0.5 * (Rr[0] + Rr[4] + Rr[8] - 1.0));
}

// the rules of the host setter; *count: the constrained states
int check_path_values(int N, int mode, const double* des, const double* sigma, std::vector<int>& list) {
  list.clear();
  for (int i = 0; i <= N; i++) {
    const double* T = des + (size_t)i * 16;
    for (int k = 0; k < 16; k++) G2_CHECK(std::isfinite(T[k]), GPMP2MI_ERR_INVALID, "a pose entry is not finite");
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) {
        double d = 0;
        for (int c = 0; c < 3; c++) d += T[c * 4 + a] * T[c * 4 + b];
        G2_CHECK(std::fabs(d - (a == b ? 1.0 : 0.0)) <= 1e-6, GPMP2MI_ERR_INVALID,
                 "a rotation block is not orthonormal (max |R^T R - I| > 1e-6)");
      }
    G2_CHECK(sigma[i] > 0, GPMP2MI_ERR_INVALID, "a sigma is <= 0 or NaN");   // NaN compares false
    if (std::isfinite(sigma[i])) list.push_back(i);
  }
  if (mode != GPMP2MI_WORKSPACE_POSITION)
    for (int i = 0; i < N; i++)
      if (std::isfinite(sigma[i]) && std::isfinite(sigma[i + 1]))
        G2_CHECK(relative_angle(des + (size_t)i * 16, des + (size_t)(i + 1) * 16) <= kPi - 1e-3, GPMP2MI_ERR_INVALID,
                 "two consecutive constrained targets are more than pi - 1e-3 apart: the interpolation is undefined");
  return GPMP2MI_OK;
}

int set_path(gpmp2mi_plan* p, const double* des, const double* sigma, bool host, hipStream_t st) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_CHECK(p->ex.wp_cap > 0, GPMP2MI_ERR_INVALID, "the plan was created without workspace_path");
  G2_CHECK(!des || sigma, GPMP2MI_ERR_INVALID, "null sigma with a path");
  PlanExtras& ex = p->ex;
  const int N = p->hp.N;
  std::vector<int> list;
  if (des && host) G2_TRY(check_path_values(N, ex.wp_mode, des, sigma, list));
  G2_PLAN_LIVE(p);
  if (!des) {   // clears the path
    ex.wp_n = 0;
    return GPMP2MI_OK;
  }
  if (host) {
    const int count = (int)list.size();
    G2_HIP(hipMemcpy(ex.wp_des, des, (size_t)(N + 1) * 16 * sizeof(double), hipMemcpyHostToDevice));
    G2_HIP(hipMemcpy(ex.wp_sigma, sigma, (size_t)(N + 1) * sizeof(double), hipMemcpyHostToDevice));
    if (count > 0) G2_HIP(hipMemcpy(ex.wp_list, list.data(), count * sizeof(int), hipMemcpyHostToDevice));
    G2_HIP(hipMemcpy(ex.wp_count, &count, sizeof(int), hipMemcpyHostToDevice));
    ex.wp_n = count;
  } else {
    p->mark_dirty(st);
    G2_HIP(hipMemcpyAsync(ex.wp_des, des, (size_t)(N + 1) * 16 * sizeof(double), hipMemcpyDeviceToDevice, st));
    G2_HIP(hipMemcpyAsync(ex.wp_sigma, sigma, (size_t)(N + 1) * sizeof(double), hipMemcpyDeviceToDevice, st));
    G2_TRY(launch_path_list(N, ex.wp_sigma, ex.wp_list, ex.wp_count, st));
    ex.wp_n = N + 1;   // the count stays on the device: one wavefront per state, the ones past it leave at once
  }
  return GPMP2MI_OK;
}

struct PathSel : ScoreSel {
  double allowed_pos = 0.0, allowed_rot = 0.0;
};

// Scores the plan's resident result against its resident path on `st`; sel != null: the obstacle stage for the same
// rows first, then the extended rule and the copy of the chosen row.  host / out / sel as plan_score (score.hip).
int plan_path(gpmp2mi_plan* p, int inter, const PathOut& out, const PathSel* sel, bool host, hipStream_t st) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_CHECK(p->ex.wp_cap > 0, GPMP2MI_ERR_INVALID, "the plan was created without workspace_path");
  G2_TRY(check_plan_ready(p, inter));
  const PlanParams& P = p->hp;
  const PlanExtras& ex = p->ex;
  const int Md = P.N * (inter + 1) + 1;
  const size_t rec_bytes = (size_t)P.B * path_blocks(Md) * sizeof(PathRec);
  RowOut rows[PATH_ROWS];
  rows_of(out, rows);
  const auto layout = [&](void* base) { return carve_path((char*)base, rec_bytes, rows, shape_of(p, inter)); };
  CheckWs w;
  G2_TRY(carve_into(p->ws[p->WS_PATH], layout, &w));
  PathFinish f{};
  const PathOut o = path_out(rows, host);
  f.max_pos = o.max_pos;
  f.max_rot = o.max_rot;
  f.worst = o.worst;
  f.support = o.support;
  f.dense = o.dense;
  f.invalid = o.invalid;
  f.recs = (PathRec*)w.recs;
  f.nblk = path_blocks(Md);
  plan_shape(f.sel, p, inter);
  if (sel) {
    point_selection(f.sel, p, *sel, nullptr, host, w.sel);
    f.allowed_pos = sel->allowed_pos;
    f.allowed_rot = sel->allowed_rot;
    PriorRows got;   // the obstacle stage alone: this rule asks for no self clearance
    G2_TRY(enqueue_prior_stages(p, nullptr, inter, w.prior, st, &got));
    f.clearance = got.clearance;
    f.oor = got.oor;
  }
  p->mark_dirty(st);
  G2_TRY(launch_path_deviation(p->robot->h, p->robot->d, ex.wp_mode, ex.wp_link, ex.wp_des,
                               ex.wp_n > 0 ? ex.wp_sigma : nullptr, P.delta_t, inter, P.B, P.N, p->pb.result,
                               (PathRec*)w.recs, st));
  G2_TRY(launch_path_finish(f, st));
  return host ? finish_host(p, inter, rows, PATH_ROWS, sel, nullptr, w.sel, st) : GPMP2MI_OK;
}

int check_traj_call(const gpmp2mi_robot* r, int mode, int link, const double* des, const double* sigma, double delta_t,
                    int inter, int B, int total_step, const double* traj) {
  G2_CHECK(r && traj && des && sigma, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_mode_link(r, mode, link));
  return check_score_args(inter, B, total_step, delta_t);
}

PathOut make_out(double* max_pos, double* max_rot, int* worst, double* support, double* dense, int* invalid) {
  PathOut o;
  o.max_pos = max_pos; o.max_rot = max_rot; o.worst = worst; o.support = support; o.dense = dense; o.invalid = invalid;
  return o;
}
PathSel make_sel(double required_clearance, int require_in_range, double allowed_pos, double allowed_rot, int* best,
                 int* n_eligible, double* traj_best, double* dense_best) {
  PathSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.allowed_pos = allowed_pos; sel.allowed_rot = allowed_rot;
  sel.best = best; sel.n_eligible = n_eligible; sel.traj_best = traj_best; sel.dense_best = dense_best;
  return sel;
}

}  // namespace

extern "C" {

int gpmp2mi_plan_set_workspace_path(gpmp2mi_plan* p, const double* des, const double* sigma) {
  return set_path(p, des, sigma, true, nullptr);
}
int gpmp2mi_plan_set_workspace_path_dev(gpmp2mi_plan* p, const double* des, const double* sigma, void* stream) {
  return set_path(p, des, sigma, false, (hipStream_t)stream);
}

int gpmp2mi_workspace_path_factor(const gpmp2mi_robot* r, int mode, int link, int M, const double* conf,
                                  const double* des, double* err, double* H) {
  G2_CHECK(r && conf && des && err && M >= 0, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_mode_link(r, mode, link));
  if (M == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const int D = r->h.dof, rows = mode == GPMP2MI_WORKSPACE_POSE ? 6 : 3;
  DevBuf<double> dq, dd, de, dh;
  G2_TRY(dq.upload(conf, (size_t)M * D));
  G2_TRY(dd.upload(des, (size_t)M * 16));
  G2_TRY(de.out(err, (size_t)M * rows));
  if (H) G2_TRY(dh.out(H, (size_t)M * rows * D));
  G2_TRY(launch_path_factor(r->h, r->d, mode, link, M, dq.p, dd.p, de.p, dh.p, nullptr));
  return fetch_all(de, dh);
}

int gpmp2mi_path_score_traj_dev(const gpmp2mi_robot* r, int mode, int link, const double* des, const double* sigma,
                                double delta_t, int inter_step, int B, int total_step, const double* traj,
                                double* max_pos_dev, double* max_rot_dev, int* worst, double* support_cost,
                                double* dense_cost, int* invalid, void* stream) {
  G2_TRY(check_traj_call(r, mode, link, des, sigma, delta_t, inter_step, B, total_step, traj));
  if (B == 0) return GPMP2MI_OK;
  const int Md = total_step * (inter_step + 1) + 1;
  const int nblk = path_blocks(Md);
  std::unique_lock<std::mutex> lk;
  G2_TRY(records_ready(r, nullptr, r->path_ws, (size_t)B * nblk * sizeof(PathRec), lk));
  PathFinish f{};
  f.sel.B = B;
  f.recs = (PathRec*)r->path_ws.p;
  f.nblk = nblk;
  f.max_pos = max_pos_dev;
  f.max_rot = max_rot_dev;
  f.worst = worst;
  f.support = support_cost;
  f.dense = dense_cost;
  f.invalid = invalid;
  G2_TRY(launch_path_deviation(r->h, r->d, mode, link, des, sigma, delta_t, inter_step, B, total_step, traj,
                               (PathRec*)r->path_ws.p, (hipStream_t)stream));
  return launch_path_finish(f, (hipStream_t)stream);
}

int gpmp2mi_path_score_traj(const gpmp2mi_robot* r, int mode, int link, const double* des, const double* sigma,
                            double delta_t, int inter_step, int B, int total_step, const double* traj,
                            double* max_pos_dev, double* max_rot_dev, int* worst, double* support_cost, double* dense_cost,
                            int* invalid) {
  G2_TRY(check_traj_call(r, mode, link, des, sigma, delta_t, inter_step, B, total_step, traj));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  DevBuf<double> dt, dd, dg, dp, dr, ds, dn;
  DevBuf<int> dw, di;
  G2_TRY(dt.upload(traj, (size_t)B * (total_step + 1) * 2 * r->h.dof));
  G2_TRY(dd.upload(des, (size_t)(total_step + 1) * 16));
  G2_TRY(dg.upload(sigma, (size_t)total_step + 1));
  if (max_pos_dev) G2_TRY(dp.out(max_pos_dev, B));
  if (max_rot_dev) G2_TRY(dr.out(max_rot_dev, B));
  if (worst) G2_TRY(dw.out(worst, (size_t)2 * B));
  if (support_cost) G2_TRY(ds.out(support_cost, B));
  if (dense_cost) G2_TRY(dn.out(dense_cost, B));
  if (invalid) G2_TRY(di.out(invalid, B));
  G2_TRY(gpmp2mi_path_score_traj_dev(r, mode, link, dd.p, dg.p, delta_t, inter_step, B, total_step, dt.p, dp.p, dr.p, dw.p,
                                     ds.p, dn.p, di.p, nullptr));
  return fetch_all(dp, dr, dw, ds, dn, di);
}

int gpmp2mi_plan_path_score(gpmp2mi_plan* p, int inter_step, double* max_pos_dev, double* max_rot_dev, int* worst,
                            double* support_cost, double* dense_cost, int* invalid) {
  return plan_path(p, inter_step, make_out(max_pos_dev, max_rot_dev, worst, support_cost, dense_cost, invalid), nullptr,
                   true, nullptr);
}
int gpmp2mi_plan_path_score_dev(gpmp2mi_plan* p, int inter_step, double* max_pos_dev, double* max_rot_dev, int* worst,
                                double* support_cost, double* dense_cost, int* invalid, void* stream) {
  return plan_path(p, inter_step, make_out(max_pos_dev, max_rot_dev, worst, support_cost, dense_cost, invalid), nullptr,
                   false, (hipStream_t)stream);
}

int gpmp2mi_plan_select_path(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                             double max_pos_dev_allowed, double max_rot_dev_allowed, int* best, int* n_eligible,
                             double* traj_best, double* dense_best) {
  const PathSel sel = make_sel(required_clearance, require_in_range, max_pos_dev_allowed, max_rot_dev_allowed, best,
                               n_eligible, traj_best, dense_best);
  return plan_path(p, inter_step, PathOut{}, &sel, true, nullptr);
}
int gpmp2mi_plan_select_path_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                 double max_pos_dev_allowed, double max_rot_dev_allowed, int* best, int* n_eligible,
                                 double* traj_best, double* dense_best, void* stream) {
  const PathSel sel = make_sel(required_clearance, require_in_range, max_pos_dev_allowed, max_rot_dev_allowed, best,
                               n_eligible, traj_best, dense_best);
  return plan_path(p, inter_step, PathOut{}, &sel, false, (hipStream_t)stream);
}

}  // extern "C"
