// self_score.hip -- the self-collision check of the executed trajectory (include/gpmp2mi.h "self-collision check"): pair
// tables (given or generated from the kinematic tree), the per-row scores for caller buffers and for a plan's resident
// result, and the selection that asks for both clearances.  Kernels: self_clearance_kernels.hip; the obstacle side of
// select_checked is k_score (score_kernels.hip), untouched.
#include <cmath>

#include "host.h"

using namespace g2;

namespace {

// the rules of check_score_args, then the launch limits of this stage (a smaller tile, a count of Md * P per row)
int check_self_args(const gpmp2mi_robot* r, const gpmp2mi_self_pairs* t, int inter, int B, int total_step, double delta_t) {
  G2_TRY(check_score_args(inter, B, total_step, delta_t));
  G2_CHECK(t->S == r->h.nr_spheres && t->dof == r->h.dof && t->kind == r->h.kind, GPMP2MI_ERR_INVALID,
           "the pair table was made for another robot (sphere count / dof / kind)");
  const long long Md = (long long)total_step * (inter + 1) + 1;
  G2_CHECK((long long)self_blocks((int)Md, t->S) * std::max(B, 1) < (1ll << 31) && Md * std::max(t->P, 1) < (1ll << 31),
           GPMP2MI_ERR_INVALID, "too many checked (state, pair)s for one launch");
  return GPMP2MI_OK;
}

// parent of every link in the tree Kin::walk_links (device_math.h) walks, -1 for the root
std::vector<int> link_parents(const RobotDev& h) {
  std::vector<int> par(h.nr_links, -1);
  for (int l = 1; l < h.nr_links; l++) par[l] = l - 1;   // a chain, unless there is a second arm
  if (h.arm2_dof > 0) {
    const bool lift = h.kind == GPMP2MI_ROBOT_POSE2_MOBILE_VETLIN_2ARMS;
    const int first1 = lift ? 2 : 1, first2 = first1 + (h.arm_dof - h.arm2_dof);
    par[first2] = par[first1];   // both arms start from the vehicle (the torso)
  }
  return par;
}
int tree_distance(const std::vector<int>& par, int a, int b) {
  auto depth = [&](int l) { int d = 0; while (par[l] >= 0) { l = par[l]; d++; } return d; };
  int da = depth(a), db = depth(b), n = 0;
  while (da > db) { a = par[a]; da--; n++; }
  while (db > da) { b = par[b]; db--; n++; }
  while (a != b) { a = par[a]; b = par[b]; n += 2; }
  return n;
}

// Layout of a plan's self-check workspace for (B, N, D, S, inter): the two record sets, then the staging of the
// host-pointer forms
struct PlanSelfWs {
  ScoreRec *recs, *obs_recs;
  ScoreOut out;
  int* pick;   // best, n_eligible, then (8-byte aligned) the chosen row's final_error: one 16-byte copy
  double *traj_best, *dense_best;
  size_t bytes;
};
PlanSelfWs plan_ws_layout(char* base, int B, int N, int D, int S, int inter) {
  const size_t Md = (size_t)N * (inter + 1) + 1;
  PlanSelfWs w{};
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base + off;
    off += ws_round(bytes);
    return p;
  };
  w.recs = (ScoreRec*)take((size_t)B * self_blocks((int)Md, S) * sizeof(ScoreRec));
  w.obs_recs = (ScoreRec*)take((size_t)B * score_blocks((int)Md) * sizeof(ScoreRec));
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

// Scores the plan's resident result against `t` on `st`; sel != null: k_score for the same rows first, then the rule
// with both clearances and the copy of the chosen row.  host / out / sel as plan_score (score.hip); out.oor: invalid.
int g2::plan_self_score(gpmp2mi_plan* p, const gpmp2mi_self_pairs* t, int inter, const ScoreOut& out, const SelfSel* sel,
                    bool host, hipStream_t st) {
  G2_CHECK(p && t, GPMP2MI_ERR_INVALID, "null argument");
  G2_PLAN_LIVE(p);   // before anything is enqueued
  G2_CHECK(p->optimized, GPMP2MI_ERR_INVALID, "plan has not been optimized");
  const PlanParams& P = p->hp;
  G2_CHECK(p->robot->h.dof == P.D, GPMP2MI_ERR_INVALID, "robot dof does not fit the plan");
  G2_TRY(check_self_args(p->robot, t, inter, P.B, P.N, P.delta_t));
  G2_CHECK(t->P == 0 || t->device == p->device, GPMP2MI_ERR_INVALID, "the pair table lives on another device than the plan");
  const int S = p->robot->h.nr_spheres;
  G2_TRY(ws_reserve(&p->self_ws, &p->self_ws_bytes, plan_ws_layout(nullptr, P.B, P.N, P.D, S, inter).bytes));
  const PlanSelfWs w = plan_ws_layout((char*)p->self_ws, P.B, P.N, P.D, S, inter);
  const size_t Md = (size_t)P.N * (inter + 1) + 1;
  SelfFinish f{};
  const ScoreOut& o = host ? w.out : out;
  // the host form computes only what the caller asked for
  f.support = (!host || out.support) ? o.support : nullptr;
  f.dense = (!host || out.dense) ? o.dense : nullptr;
  f.clearance = (!host || out.clearance) ? o.clearance : nullptr;
  f.worst = (!host || out.worst) ? o.worst : nullptr;
  f.invalid = (!host || out.oor) ? o.oor : nullptr;
  f.recs = w.recs;
  f.nblk = self_blocks((int)Md, S);
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
    g.recs = w.obs_recs;
    g.nblk = score_blocks((int)Md);
    g.required_clearance = sel->required_clearance;
    g.require_in_range = sel->require_in_range;
    f.required_self_clearance = sel->required_self_clearance;
    g.ferr = p->pb.final_err;
    g.status = p->pb.status;
    g.best = host ? w.pick : sel->best;
    g.n_eligible = host ? w.pick + 1 : sel->n_eligible;
    g.best_err = host ? (double*)(w.pick + 2) : nullptr;
    g.traj_best = host ? (sel->traj_best ? w.traj_best : nullptr) : sel->traj_best;
    g.dense_best = host ? (sel->dense_best ? w.dense_best : nullptr) : sel->dense_best;
  }
  p->mark_dirty(st);
  if (sel) G2_TRY(launch_score(p->robot->h, p->robot->d, p->sdf->h, P.delta_t, inter, P.B, P.N, p->pb.result, w.obs_recs, st));
  G2_TRY(launch_self_clearance(p->robot->h, p->robot->d, t->d, t->P, P.delta_t, inter, P.B, P.N, p->pb.result, w.recs, st));
  G2_TRY(launch_self_finish(f, st));
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
    if (pick.best >= 0 && (sel->traj_best || sel->dense_best)) {   // nothing chosen: the trajectory outputs stay as they are
      G2_TRY(back(sel->traj_best, w.traj_best, (size_t)(P.N + 1) * 2 * P.D * sizeof(double)));
      G2_TRY(back(sel->dense_best, w.dense_best, Md * 2 * P.D * sizeof(double)));
      G2_HIP(hipStreamSynchronize(st));
    }
  }
  p->mark_clean(st);
  return GPMP2MI_OK;
}

namespace {

// the table as the kernels read it: sorted-order sphere indices and total_eps
int upload_pairs(const gpmp2mi_robot* r, gpmp2mi_self_pairs* t) {
  const RobotDev& h = r->h;
  std::vector<int> sorted(h.nr_spheres);
  std::vector<double> radius(h.nr_spheres);
  for (int s = 0; s < h.nr_spheres; s++) {
    sorted[h.sph_orig[s]] = s;
    radius[h.sph_orig[s]] = h.sph_r[s];
  }
  std::vector<SelfPair> dev(t->P);
  for (int i = 0; i < t->P; i++) {
    const int a = (int)t->data[4 * i], b = (int)t->data[4 * i + 1];
    dev[i].total_eps = radius[a] + radius[b] + t->data[4 * i + 2];
    dev[i].a = sorted[a];
    dev[i].b = sorted[b];
  }
  G2_TRY(ensure_device());
  G2_HIP(hipGetDevice(&t->device));
  G2_CHECK(t->device == r->device, GPMP2MI_ERR_INVALID, "the robot handle lives on another device than the current one");
  G2_TRY(dev_malloc((void**)&t->d, (size_t)t->P * sizeof(SelfPair), GPMP2MI_ERR_NO_DEVICE));
  G2_HIP(hipMemcpy(t->d, dev.data(), (size_t)t->P * sizeof(SelfPair), hipMemcpyHostToDevice));
  return GPMP2MI_OK;
}

}  // namespace

extern "C" {

int gpmp2mi_self_pairs_create(const gpmp2mi_robot* r, int P, const double* data, gpmp2mi_self_pairs** out) {
  G2_CHECK(r && out && P >= 0 && (data || P == 0), GPMP2MI_ERR_INVALID, "null argument or P < 0");
  *out = nullptr;
  const int S = r->h.nr_spheres;
  for (int i = 0; i < P; i++) {
    const double a = data[4 * i], b = data[4 * i + 1];
    G2_CHECK(a >= 0 && a < S && b >= 0 && b < S && a == std::floor(a) && b == std::floor(b), GPMP2MI_ERR_INVALID,
             "sphere id is not an integer in [0, nr_spheres)");
    G2_CHECK(a != b, GPMP2MI_ERR_INVALID, "a pair names the same sphere twice");
  }
  auto t = std::make_unique<gpmp2mi_self_pairs>();
  t->P = P;
  t->S = S;
  t->dof = r->h.dof;
  t->kind = r->h.kind;
  if (P > 0) {
    t->data.assign(data, data + (size_t)P * 4);
    G2_TRY(upload_pairs(r, t.get()));
  }
  *out = t.release();
  return GPMP2MI_OK;
}

int gpmp2mi_self_pairs_generate(const gpmp2mi_robot* r, int min_joint_gap, int n_ref, const double* ref_conf,
                                double epsilon, double sigma, gpmp2mi_self_pairs** out) {
  G2_CHECK(r && out, GPMP2MI_ERR_INVALID, "null argument");
  *out = nullptr;
  G2_CHECK(min_joint_gap >= 1, GPMP2MI_ERR_INVALID, "min_joint_gap must be >= 1");
  G2_CHECK(n_ref >= 0 && (ref_conf || n_ref == 0), GPMP2MI_ERR_INVALID, "n_ref < 0, or reference configurations missing");
  G2_CHECK(std::isfinite(epsilon) && sigma > 0, GPMP2MI_ERR_INVALID, "epsilon must be finite and sigma > 0");
  const RobotDev& h = r->h;
  const int S = h.nr_spheres;
  std::vector<int> link(S);
  std::vector<double> radius(S);
  for (int s = 0; s < S; s++) {
    link[h.sph_orig[s]] = h.sph_link[s];
    radius[h.sph_orig[s]] = h.sph_r[s];
  }
  std::vector<double> data;
  if (h.kind != GPMP2MI_ROBOT_POINT) {
    const std::vector<int> par = link_parents(h);
    for (int a = 0; a < S; a++)
      for (int b = a + 1; b < S; b++)
        if (tree_distance(par, link[a], link[b]) >= min_joint_gap) data.insert(data.end(), {(double)a, (double)b, epsilon, sigma});
  }
  if (n_ref > 0 && !data.empty()) {
    std::vector<double> c((size_t)n_ref * S * 3);
    G2_TRY(gpmp2mi_sphere_centers(r, n_ref, ref_conf, c.data(), nullptr));
    std::vector<double> kept;
    for (size_t i = 0; i < data.size(); i += 4) {
      const int a = (int)data[i], b = (int)data[i + 1];
      bool clear = true;
      for (int m = 0; m < n_ref && clear; m++) {
        const double* ca = &c[((size_t)m * S + a) * 3];
        const double* cb = &c[((size_t)m * S + b) * 3];
        const double dx = ca[0] - cb[0], dy = ca[1] - cb[1], dz = ca[2] - cb[2];
        clear = !(std::sqrt(dx * dx + dy * dy + dz * dz) - (radius[a] + radius[b]) < 0.0);
      }
      if (clear) kept.insert(kept.end(), data.begin() + i, data.begin() + i + 4);
    }
    data.swap(kept);
  }
  return gpmp2mi_self_pairs_create(r, (int)(data.size() / 4), data.data(), out);
}

int gpmp2mi_self_pairs_count(const gpmp2mi_self_pairs* t) { return t ? t->P : -1; }

int gpmp2mi_self_pairs_get(const gpmp2mi_self_pairs* t, double* data) {
  G2_CHECK(t && (data || t->P == 0), GPMP2MI_ERR_INVALID, "null argument");
  std::copy(t->data.begin(), t->data.end(), data);
  return GPMP2MI_OK;
}

void gpmp2mi_self_pairs_destroy(gpmp2mi_self_pairs* t) { delete t; }

int gpmp2mi_self_score_traj_dev(const gpmp2mi_robot* r, const gpmp2mi_self_pairs* t, double delta_t, int inter_step,
                                int B, int total_step, const double* traj, double* self_support_cost,
                                double* self_dense_cost, double* min_self_clearance, int* worst, int* invalid,
                                void* stream) {
  G2_CHECK(r && t && traj, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_self_args(r, t, inter_step, B, total_step, delta_t));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  int cur = -1;
  G2_HIP(hipGetDevice(&cur));
  G2_CHECK(cur == r->device && (t->P == 0 || cur == t->device), GPMP2MI_ERR_INVALID,
           "the robot handle or the pair table lives on another device than the current one");
  const int Md = total_step * (inter_step + 1) + 1;
  const int nblk = self_blocks(Md, t->S);
  std::lock_guard<std::mutex> lk(t->mu);
  G2_TRY(ws_reserve(&t->ws, &t->ws_bytes, (size_t)B * nblk * sizeof(ScoreRec)));
  SelfFinish f{};
  f.sel.B = B;
  f.recs = (ScoreRec*)t->ws;
  f.nblk = nblk;
  f.support = self_support_cost;
  f.dense = self_dense_cost;
  f.clearance = min_self_clearance;
  f.worst = worst;
  f.invalid = invalid;
  G2_TRY(launch_self_clearance(r->h, r->d, t->d, t->P, delta_t, inter_step, B, total_step, traj, (ScoreRec*)t->ws,
                               (hipStream_t)stream));
  return launch_self_finish(f, (hipStream_t)stream);
}

int gpmp2mi_self_score_traj(const gpmp2mi_robot* r, const gpmp2mi_self_pairs* t, double delta_t, int inter_step, int B,
                            int total_step, const double* traj, double* self_support_cost, double* self_dense_cost,
                            double* min_self_clearance, int* worst, int* invalid) {
  G2_CHECK(r && t && traj, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_self_args(r, t, inter_step, B, total_step, delta_t));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  DevBuf<double> dt, ds, dd, dc;
  DevBuf<int> dw, di;
  G2_TRY(dt.upload(traj, (size_t)B * (total_step + 1) * 2 * r->h.dof));
  if (self_support_cost) G2_TRY(ds.out(self_support_cost, B));
  if (self_dense_cost) G2_TRY(dd.out(self_dense_cost, B));
  if (min_self_clearance) G2_TRY(dc.out(min_self_clearance, B));
  if (worst) G2_TRY(dw.out(worst, (size_t)2 * B));
  if (invalid) G2_TRY(di.out(invalid, B));
  G2_TRY(gpmp2mi_self_score_traj_dev(r, t, delta_t, inter_step, B, total_step, dt.p, ds.p, dd.p, dc.p, dw.p, di.p, nullptr));
  return fetch_all(ds, dd, dc, dw, di);
}

int gpmp2mi_plan_self_score(gpmp2mi_plan* p, const gpmp2mi_self_pairs* t, int inter_step, double* self_support_cost,
                            double* self_dense_cost, double* min_self_clearance, int* worst, int* invalid) {
  ScoreOut o;
  o.support = self_support_cost; o.dense = self_dense_cost; o.clearance = min_self_clearance; o.worst = worst; o.oor = invalid;
  return plan_self_score(p, t, inter_step, o, nullptr, true, nullptr);
}
int gpmp2mi_plan_self_score_dev(gpmp2mi_plan* p, const gpmp2mi_self_pairs* t, int inter_step, double* self_support_cost,
                                double* self_dense_cost, double* min_self_clearance, int* worst, int* invalid,
                                void* stream) {
  ScoreOut o;
  o.support = self_support_cost; o.dense = self_dense_cost; o.clearance = min_self_clearance; o.worst = worst; o.oor = invalid;
  return plan_self_score(p, t, inter_step, o, nullptr, false, (hipStream_t)stream);
}

int gpmp2mi_plan_select_checked(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                const gpmp2mi_self_pairs* t, double required_self_clearance, int* best, int* n_eligible,
                                double* traj_best, double* dense_best) {
  SelfSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.required_self_clearance = required_self_clearance;
  sel.best = best; sel.n_eligible = n_eligible; sel.traj_best = traj_best; sel.dense_best = dense_best;
  return plan_self_score(p, t, inter_step, ScoreOut{}, &sel, true, nullptr);
}
int gpmp2mi_plan_select_checked_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                    const gpmp2mi_self_pairs* t, double required_self_clearance, int* best,
                                    int* n_eligible, double* traj_best, double* dense_best, void* stream) {
  SelfSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.required_self_clearance = required_self_clearance;
  sel.best = best; sel.n_eligible = n_eligible; sel.traj_best = traj_best; sel.dense_best = dense_best;
  return plan_self_score(p, t, inter_step, ScoreOut{}, &sel, false, (hipStream_t)stream);
}

}  // extern "C"
