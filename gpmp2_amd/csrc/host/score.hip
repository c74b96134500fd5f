// score.hip -- the score-and-select stage (include/gpmp2mi.h "scoring"): dense collision cost, minimum clearance and
// best-of-batch selection for caller buffers and for a plan's resident result.  Two launches per call (k_score,
// k_score_finish: score_kernels.hip); the `_dev` forms enqueue them and return.  The multi-plan forms are in
// multi_plan.hip, next to the shards they visit.
#include <cmath>

#include "host.h"

using namespace g2;

int g2::check_score_args(int inter, int B, int total_step, double delta_t) {
  G2_CHECK(inter >= 0, GPMP2MI_ERR_INVALID, "inter_step must be >= 0");
  G2_CHECK(B >= 0, GPMP2MI_ERR_INVALID, "B must be >= 0");
  G2_CHECK(total_step >= 1, GPMP2MI_ERR_INVALID, "total_step must be >= 1");
  G2_CHECK(delta_t > 0, GPMP2MI_ERR_INVALID, "delta_t must be > 0");
  const long long Md = (long long)total_step * (inter + 1) + 1;
  G2_CHECK(Md < (1ll << 31) / GPMP2MI_MAX_DOF && (long long)score_blocks((int)Md) * std::max(B, 1) < (1ll << 31),
           GPMP2MI_ERR_INVALID, "too many checked states for one launch");
  return GPMP2MI_OK;
}

namespace {

// k_score over `traj` into `recs`, then k_score_finish with the outputs (and the selection) of `f`
int enqueue_score(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, double dt, int inter, int B, int N, const double* traj,
                  ScoreRec* recs, ScoreFinish f, hipStream_t st) {
  const int Md = N * (inter + 1) + 1;
  f.B = B;
  f.N = N;
  f.D = r->h.dof;
  f.lie = r->h.kind >= GPMP2MI_ROBOT_POSE2_MOBILE_BASE;
  f.inter = inter;
  f.Md = Md;
  f.nblk = score_blocks(Md);
  f.dt = dt;
  f.recs = recs;
  f.traj = traj;
  G2_TRY(launch_score(r->h, r->d, s->h, dt, inter, B, N, traj, recs, st));
  return launch_score_finish(f, st);
}

}  // namespace

void g2::select_rule_host(int B, const double* ferr, const int* status, const double* clearance, const int* oor,
                          double required_clearance, int require_in_range, int* best, int* n_eligible) {
  int bb = -1, n = 0;
  for (int b = 0; b < B; b++) {
    const bool ok = (!status || status[b] != GPMP2MI_TRAJ_NOT_SPD) && std::isfinite(ferr[b]) &&
                    clearance[b] >= required_clearance && (!require_in_range || !oor || oor[b] == 0);
    if (!ok) continue;
    n++;
    if (bb < 0 || ferr[b] < ferr[bb]) bb = b;
  }
  if (best) *best = bb;
  if (n_eligible) *n_eligible = n;
}

// The simplest client of the shared driver (check_common.hip): one record set, no earlier stage, no extra output
int g2::plan_score(gpmp2mi_plan* p, int inter, const ScoreOut& out, const ScoreSel* sel, bool host, hipStream_t st) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_TRY(check_plan_ready(p, inter));
  const PlanParams& P = p->hp;
  const int Md = P.N * (inter + 1) + 1;
  const size_t rec_bytes = (size_t)P.B * score_blocks(Md) * sizeof(ScoreRec);
  RowOut rows[SCORE_ROWS];
  rows_of(out, SCORE_WORST, rows);
  const auto layout = [&](void* base) { return carve_score((char*)base, rec_bytes, rows, shape_of(p, inter)); };
  CheckWs w;
  G2_TRY(carve_into(p->ws[p->WS_SCORE], layout, &w));
  ScoreFinish f{};
  const ScoreOut o = score_out(rows, host);
  f.support = o.support;
  f.dense = o.dense;
  f.clearance = o.clearance;
  f.worst = o.worst;
  f.oor = o.oor;
  if (sel) point_selection(f, p, *sel, nullptr, host, w.sel);
  p->mark_dirty(st);
  G2_TRY(enqueue_score(p->robot, p->sdf, P.delta_t, inter, P.B, P.N, p->pb.result, (ScoreRec*)w.recs, f, st));
  return host ? finish_host(p, inter, rows, SCORE_ROWS, sel, nullptr, w.sel, st) : GPMP2MI_OK;
}

namespace {
ScoreSel make_sel(double required_clearance, int require_in_range, int* best, int* n_eligible, double* traj_best,
                  double* dense_best) {
  ScoreSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.best = best; sel.n_eligible = n_eligible; sel.traj_best = traj_best; sel.dense_best = dense_best;
  return sel;
}
}  // namespace

extern "C" {

int gpmp2mi_score_traj_dev(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, double delta_t, int inter_step, int B,
                           int total_step, const double* traj, double* support_cost, double* dense_cost,
                           double* min_clearance, int* worst, int* out_of_range, void* stream) {
  G2_CHECK(r && s && traj, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_score_args(inter_step, B, total_step, delta_t));
  if (B == 0) return GPMP2MI_OK;
  const size_t Md = (size_t)total_step * (inter_step + 1) + 1;
  std::unique_lock<std::mutex> lk;
  G2_TRY(records_ready(r, nullptr, r->score_ws, (size_t)B * score_blocks((int)Md) * sizeof(ScoreRec), lk));
  ScoreFinish f{};
  f.support = support_cost;
  f.dense = dense_cost;
  f.clearance = min_clearance;
  f.worst = worst;
  f.oor = out_of_range;
  return enqueue_score(r, s, delta_t, inter_step, B, total_step, traj, (ScoreRec*)r->score_ws.p, f, (hipStream_t)stream);
}

int gpmp2mi_score_traj(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, double delta_t, int inter_step, int B,
                       int total_step, const double* traj, double* support_cost, double* dense_cost,
                       double* min_clearance, int* worst, int* out_of_range) {
  G2_CHECK(r && s && traj, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_score_args(inter_step, B, total_step, delta_t));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  DevBuf<double> dt, ds, dd, dc;
  DevBuf<int> dw, dr;
  G2_TRY(dt.upload(traj, (size_t)B * (total_step + 1) * 2 * r->h.dof));
  if (support_cost) G2_TRY(ds.out(support_cost, B));
  if (dense_cost) G2_TRY(dd.out(dense_cost, B));
  if (min_clearance) G2_TRY(dc.out(min_clearance, B));
  if (worst) G2_TRY(dw.out(worst, (size_t)2 * B));
  if (out_of_range) G2_TRY(dr.out(out_of_range, B));
  G2_TRY(gpmp2mi_score_traj_dev(r, s, delta_t, inter_step, B, total_step, dt.p, ds.p, dd.p, dc.p, dw.p, dr.p, nullptr));
  return fetch_all(ds, dd, dc, dw, dr);
}

int gpmp2mi_select_best(int B, const double* final_error, const int* status, const double* min_clearance,
                        const int* out_of_range, double required_clearance, int require_in_range, int* best,
                        int* n_eligible) {
  G2_CHECK(B >= 0, GPMP2MI_ERR_INVALID, "B must be >= 0");
  G2_CHECK(final_error && min_clearance, GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK(!require_in_range || out_of_range, GPMP2MI_ERR_INVALID, "require_in_range needs out_of_range");
  select_rule_host(B, final_error, status, min_clearance, out_of_range, required_clearance, require_in_range, best,
                   n_eligible);
  return GPMP2MI_OK;
}

int gpmp2mi_select_best_dev(int B, const double* final_error, const int* status, const double* min_clearance,
                            const int* out_of_range, double required_clearance, int require_in_range, int* best,
                            int* n_eligible, void* stream) {
  G2_CHECK(B >= 0, GPMP2MI_ERR_INVALID, "B must be >= 0");
  G2_CHECK(final_error && min_clearance, GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK(!require_in_range || out_of_range, GPMP2MI_ERR_INVALID, "require_in_range needs out_of_range");
  G2_TRY(ensure_device());
  ScoreFinish f{};
  f.B = B;
  f.in_clearance = min_clearance;
  f.in_oor = out_of_range;
  f.select = 1;
  f.required_clearance = required_clearance;
  f.require_in_range = require_in_range;
  f.ferr = final_error;
  f.status = status;
  f.best = best;
  f.n_eligible = n_eligible;
  return launch_score_finish(f, (hipStream_t)stream);   // B = 0: the kernel writes best = -1, n_eligible = 0
}

int gpmp2mi_plan_score(gpmp2mi_plan* p, int inter_step, double* support_cost, double* dense_cost,
                       double* min_clearance, int* worst, int* out_of_range) {
  return plan_score(p, inter_step, make_out(support_cost, dense_cost, min_clearance, worst, out_of_range), nullptr, true,
                    nullptr);
}
int gpmp2mi_plan_score_dev(gpmp2mi_plan* p, int inter_step, double* support_cost, double* dense_cost,
                           double* min_clearance, int* worst, int* out_of_range, void* stream) {
  return plan_score(p, inter_step, make_out(support_cost, dense_cost, min_clearance, worst, out_of_range), nullptr, false,
                    (hipStream_t)stream);
}

int gpmp2mi_plan_select(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range, int* best,
                        int* n_eligible, double* traj_best, double* dense_best) {
  const ScoreSel sel = make_sel(required_clearance, require_in_range, best, n_eligible, traj_best, dense_best);
  return plan_score(p, inter_step, ScoreOut{}, &sel, true, nullptr);
}
int gpmp2mi_plan_select_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range, int* best,
                            int* n_eligible, double* traj_best, double* dense_best, void* stream) {
  const ScoreSel sel = make_sel(required_clearance, require_in_range, best, n_eligible, traj_best, dense_best);
  return plan_score(p, inter_step, ScoreOut{}, &sel, false, (hipStream_t)stream);
}

}  // extern "C"
