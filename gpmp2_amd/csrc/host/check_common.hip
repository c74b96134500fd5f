// check_common.hip -- the host-side driver that the check stages of the executed trajectory share (score.hip,
// self_score.hip, motion_score.hip, moving.hip, path.hip, retime.hip, torque.hip; group.hip takes the parts that fit): the
// preamble
// of a plan form, the shape and the selection of its finish kernel, the earlier stages a later one's rule reads, the
// closing read-back of a host form, and the preamble of a caller-buffer `_dev` form.  The layouts and the staging rule
// are in staging.h; the kernels and what they compute stay with the stages.
#include "host.h"

using namespace g2;

int g2::check_plan_ready(gpmp2mi_plan* p, int inter) {
  G2_PLAN_LIVE(p);   // before anything is enqueued
  G2_CHECK(p->optimized, GPMP2MI_ERR_INVALID, "plan has not been optimized");
  const PlanParams& P = p->hp;
  G2_TRY(check_score_args(inter, P.B, P.N, P.delta_t));
  G2_CHECK(p->robot->h.dof == P.D, GPMP2MI_ERR_INVALID, "robot dof does not fit the plan");
  return GPMP2MI_OK;
}

void g2::plan_shape(ScoreFinish& g, const gpmp2mi_plan* p, int inter) {
  const PlanParams& P = p->hp;
  g.B = P.B;
  g.N = P.N;
  g.D = P.D;
  g.lie = p->robot->h.kind >= GPMP2MI_ROBOT_POSE2_MOBILE_BASE;
  g.inter = inter;
  g.Md = P.N * (inter + 1) + 1;
  g.dt = P.delta_t;
  g.traj = p->pb.result;
}

SelExtra g2::point_selection(ScoreFinish& g, const gpmp2mi_plan* p, const ScoreSel& sel, const SelExtra* x, bool host,
                             const PickRows& w) {
  g.select = 1;
  g.required_clearance = sel.required_clearance;
  g.require_in_range = sel.require_in_range;
  g.ferr = p->pb.final_err;
  g.status = p->pb.status;
  // a stage with extra outputs has its kernel read `best` back for them: a device form without one gets the workspace's
  g.best = (host || (x && !sel.best)) ? &w.pick->best : sel.best;
  g.n_eligible = host ? &w.pick->n_eligible : sel.n_eligible;
  g.best_err = host ? &w.pick->best_err : nullptr;
  g.traj_best = (double*)staging_rule(host, sel.traj_best, w.traj_best);
  g.dense_best = (double*)staging_rule(host, sel.dense_best, w.dense_best);
  SelExtra k;
  if (x) {
    k.value = host ? &w.pick->extra : x->value;
    k.row = (double*)staging_rule(host, x->row, w.extra_row);
  }
  return k;
}

// The per-row scores of the earlier stages, by their own plan forms on the same stream.  The self check goes first: it
// is the one that can still refuse (a table made for another robot), and a refused call enqueues nothing.
int g2::enqueue_prior_stages(gpmp2mi_plan* p, const gpmp2mi_self_pairs* pairs, int inter, const PriorRows& w,
                             hipStream_t st, PriorRows* got) {
  *got = PriorRows{};
  ScoreOut so;
  if (pairs) {
    so.clearance = w.self_clearance;
    so.oor = w.self_invalid;
    G2_TRY(plan_self_score(p, pairs, inter, so, nullptr, false, st));
    got->self_clearance = w.self_clearance;
    got->self_invalid = w.self_invalid;
  }
  so.clearance = w.clearance;
  so.oor = w.oor;
  G2_TRY(plan_score(p, inter, so, nullptr, false, st));
  got->clearance = w.clearance;
  got->oor = w.oor;
  return GPMP2MI_OK;
}

int g2::copy_back(void* dst, const void* src, size_t bytes, hipStream_t st) {
  if (dst && bytes) G2_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
  return GPMP2MI_OK;
}

int g2::finish_host(gpmp2mi_plan* p, int inter, const RowOut* rows, int n_rows, const ScoreSel* sel, const SelExtra* x,
                    const PickRows& w, hipStream_t st) {
  const PlanParams& P = p->hp;
  for (int i = 0; i < n_rows; i++) G2_TRY(copy_back(rows[i].caller, rows[i].staged, rows[i].bytes(P.B), st));
  PickBlock got{-1, 0, 0.0, 0.0};
  if (sel) G2_TRY(copy_back(&got, w.pick, sizeof(got) - (x ? 0 : sizeof(double)), st));   // one copy
  G2_HIP(hipStreamSynchronize(st));
  if (sel) {
    if (sel->best) *sel->best = got.best;
    if (sel->n_eligible) *sel->n_eligible = got.n_eligible;
    if (got.best >= 0) {   // nothing chosen: the outputs about the chosen row stay as they are
      if (sel->best_error) *sel->best_error = got.best_err;
      if (x && x->value) *x->value = got.extra;
      double* extra_row = x ? x->row : nullptr;
      if (sel->traj_best || sel->dense_best || extra_row) {
        const size_t Md = (size_t)P.N * (inter + 1) + 1;
        G2_TRY(copy_back(sel->traj_best, w.traj_best, (size_t)(P.N + 1) * 2 * P.D * sizeof(double), st));
        G2_TRY(copy_back(sel->dense_best, w.dense_best, Md * 2 * P.D * sizeof(double), st));
        if (extra_row) G2_TRY(copy_back(extra_row, w.extra_row, x->row_bytes, st));
        G2_HIP(hipStreamSynchronize(st));
      }
    }
  }
  p->mark_clean(st);
  return GPMP2MI_OK;
}

int g2::records_ready(const gpmp2mi_robot* r, const gpmp2mi_self_pairs* t, Workspace& ws, size_t bytes,
                      std::unique_lock<std::mutex>& lk) {
  G2_TRY(ensure_device());
  int cur = -1;
  G2_HIP(hipGetDevice(&cur));
  if (t) {
    G2_CHECK(cur == r->device && (t->P == 0 || cur == t->device), GPMP2MI_ERR_INVALID,
             "the robot handle or the pair table lives on another device than the current one");
  } else {
    G2_CHECK(cur == r->device, GPMP2MI_ERR_INVALID, "the robot handle lives on another device than the current one");
  }
  lk = std::unique_lock<std::mutex>(t ? t->mu : r->score_mu);
  return ws.reserve(bytes);
}
