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

// Layout of a plan's scoring workspace for (B, N, D, inter): the records, then the staging of the host-pointer forms
namespace {
struct PlanScoreWs {
  ScoreRec* recs;
  ScoreOut out;
  int* pick;   // best, n_eligible, then (8-byte aligned) the chosen row's final_error: one 16-byte copy
  double *traj_best, *dense_best;
  size_t bytes;
};
PlanScoreWs plan_ws_layout(char* base, int B, int N, int D, int inter) {
  const size_t Md = (size_t)N * (inter + 1) + 1;
  PlanScoreWs w{};
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base + off;
    off += ws_round(bytes);
    return p;
  };
  w.recs = (ScoreRec*)take((size_t)B * score_blocks((int)Md) * sizeof(ScoreRec));
  w.out.support = (double*)take(B * sizeof(double));
  w.out.dense = (double*)take(B * sizeof(double));
  w.out.clearance = (double*)take(B * sizeof(double));
  w.out.worst = (int*)take(2 * B * sizeof(int));
  w.out.oor = (int*)take(B * sizeof(int));
  w.pick = (int*)take(2 * sizeof(int) + sizeof(double));
  w.traj_best = (double*)take((size_t)(N + 1) * 2 * D * sizeof(double));
  w.dense_best = (double*)take(Md * 2 * D * sizeof(double));
  w.bytes = off;
  return w;
}
}  // namespace

int g2::plan_score(gpmp2mi_plan* p, int inter, const ScoreOut& out, const ScoreSel* sel, bool host, hipStream_t st) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_PLAN_LIVE(p);   // before anything is enqueued
  G2_CHECK(p->optimized, GPMP2MI_ERR_INVALID, "plan has not been optimized");
  const PlanParams& P = p->hp;
  G2_TRY(check_score_args(inter, P.B, P.N, P.delta_t));
  G2_CHECK(p->robot->h.dof == P.D, GPMP2MI_ERR_INVALID, "robot dof does not fit the plan");
  G2_TRY(ws_reserve(&p->score_ws, &p->score_ws_bytes, plan_ws_layout(nullptr, P.B, P.N, P.D, inter).bytes));
  const PlanScoreWs w = plan_ws_layout((char*)p->score_ws, P.B, P.N, P.D, inter);
  const size_t Md = (size_t)P.N * (inter + 1) + 1;
  ScoreFinish f{};
  const ScoreOut& o = host ? w.out : out;
  // the host form computes only what the caller asked for
  f.support = (!host || out.support) ? o.support : nullptr;
  f.dense = (!host || out.dense) ? o.dense : nullptr;
  f.clearance = (!host || out.clearance) ? o.clearance : nullptr;
  f.worst = (!host || out.worst) ? o.worst : nullptr;
  f.oor = (!host || out.oor) ? o.oor : nullptr;
  if (sel) {
    f.select = 1;
    f.required_clearance = sel->required_clearance;
    f.require_in_range = sel->require_in_range;
    f.ferr = p->pb.final_err;
    f.status = p->pb.status;
    f.best = host ? w.pick : sel->best;
    f.n_eligible = host ? w.pick + 1 : sel->n_eligible;
    f.best_err = host ? (double*)(w.pick + 2) : nullptr;
    f.traj_best = host ? (sel->traj_best ? w.traj_best : nullptr) : sel->traj_best;
    f.dense_best = host ? (sel->dense_best ? w.dense_best : nullptr) : sel->dense_best;
  }
  p->mark_dirty(st);
  G2_TRY(enqueue_score(p->robot, p->sdf, P.delta_t, inter, P.B, P.N, p->pb.result, w.recs, f, st));
  if (!host) return GPMP2MI_OK;
  auto back = [&](void* dst, const void* src, size_t bytes) -> int {
    if (dst) G2_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    return GPMP2MI_OK;
  };
  G2_TRY(back(out.support, w.out.support, P.B * sizeof(double)));
  G2_TRY(back(out.dense, w.out.dense, P.B * sizeof(double)));
  G2_TRY(back(out.clearance, w.out.clearance, P.B * sizeof(double)));
  G2_TRY(back(out.worst, w.out.worst, 2 * P.B * sizeof(int)));
  G2_TRY(back(out.oor, w.out.oor, P.B * sizeof(int)));
  struct { int best, n; double err; } pick{-1, 0, 0.0};
  if (sel) G2_TRY(back(&pick, w.pick, sizeof(pick)));
  G2_HIP(hipStreamSynchronize(st));
  if (sel) {
    if (sel->best) *sel->best = pick.best;
    if (sel->n_eligible) *sel->n_eligible = pick.n;
    if (pick.best >= 0) {
      if (sel->best_error) *sel->best_error = pick.err;
      if (sel->traj_best || sel->dense_best) {   // nothing chosen: the trajectory outputs stay as they are
        G2_TRY(back(sel->traj_best, w.traj_best, (size_t)(P.N + 1) * 2 * P.D * sizeof(double)));
        G2_TRY(back(sel->dense_best, w.dense_best, Md * 2 * P.D * sizeof(double)));
        G2_HIP(hipStreamSynchronize(st));
      }
    }
  }
  p->mark_clean(st);
  return GPMP2MI_OK;
}

extern "C" {

int gpmp2mi_score_traj_dev(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, double delta_t, int inter_step, int B,
                           int total_step, const double* traj, double* support_cost, double* dense_cost,
                           double* min_clearance, int* worst, int* out_of_range, void* stream) {
  G2_CHECK(r && s && traj, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_score_args(inter_step, B, total_step, delta_t));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  int cur = -1;
  G2_HIP(hipGetDevice(&cur));
  G2_CHECK(cur == r->device, GPMP2MI_ERR_INVALID, "the robot handle lives on another device than the current one");
  const size_t Md = (size_t)total_step * (inter_step + 1) + 1;
  std::lock_guard<std::mutex> lk(r->score_mu);
  G2_TRY(ws_reserve(&r->score_ws, &r->score_ws_bytes, (size_t)B * score_blocks((int)Md) * sizeof(ScoreRec)));
  ScoreFinish f{};
  f.support = support_cost;
  f.dense = dense_cost;
  f.clearance = min_clearance;
  f.worst = worst;
  f.oor = out_of_range;
  return enqueue_score(r, s, delta_t, inter_step, B, total_step, traj, (ScoreRec*)r->score_ws, f, (hipStream_t)stream);
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
  ScoreOut o;
  o.support = support_cost; o.dense = dense_cost; o.clearance = min_clearance; o.worst = worst; o.oor = out_of_range;
  return plan_score(p, inter_step, o, nullptr, true, nullptr);
}
int gpmp2mi_plan_score_dev(gpmp2mi_plan* p, int inter_step, double* support_cost, double* dense_cost,
                           double* min_clearance, int* worst, int* out_of_range, void* stream) {
  ScoreOut o;
  o.support = support_cost; o.dense = dense_cost; o.clearance = min_clearance; o.worst = worst; o.oor = out_of_range;
  return plan_score(p, inter_step, o, nullptr, false, (hipStream_t)stream);
}

int gpmp2mi_plan_select(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range, int* best,
                        int* n_eligible, double* traj_best, double* dense_best) {
  ScoreSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.best = best; sel.n_eligible = n_eligible; sel.traj_best = traj_best; sel.dense_best = dense_best;
  return plan_score(p, inter_step, ScoreOut{}, &sel, true, nullptr);
}
int gpmp2mi_plan_select_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range, int* best,
                            int* n_eligible, double* traj_best, double* dense_best, void* stream) {
  ScoreSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.best = best; sel.n_eligible = n_eligible; sel.traj_best = traj_best; sel.dense_best = dense_best;
  return plan_score(p, inter_step, ScoreOut{}, &sel, false, (hipStream_t)stream);
}

}  // extern "C"
