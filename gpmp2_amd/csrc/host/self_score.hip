// self_score.hip -- the self-collision check of the executed trajectory (include/gpmp2mi.h "self-collision check"): pair
// tables (given or generated from the kinematic tree), the per-row scores for caller buffers and for a plan's resident
// result, and the selection that asks for both clearances.  Kernels: self_clearance_kernels.hip; the obstacle side of
// select_checked is k_score (score_kernels.hip), untouched.
#include <cmath>

#include "host.h"

using namespace g2;

namespace {

// behind the rules of check_score_args: the table's robot and the launch limits of this stage (a smaller tile, a count
// of Md * P per row)
int check_self_table(const gpmp2mi_robot* r, const gpmp2mi_self_pairs* t, int inter, int B, int total_step) {
  G2_CHECK(t->S == r->h.nr_spheres && t->dof == r->h.dof && t->kind == r->h.kind, GPMP2MI_ERR_INVALID,
           "the pair table was made for another robot (sphere count / dof / kind)");
  const long long Md = (long long)total_step * (inter + 1) + 1;
  G2_CHECK((long long)self_blocks((int)Md, t->S) * std::max(B, 1) < (1ll << 31) && Md * std::max(t->P, 1) < (1ll << 31),
           GPMP2MI_ERR_INVALID, "too many checked (state, pair)s for one launch");
  return GPMP2MI_OK;
}
int check_self_args(const gpmp2mi_robot* r, const gpmp2mi_self_pairs* t, int inter, int B, int total_step, double delta_t) {
  G2_TRY(check_score_args(inter, B, total_step, delta_t));
  return check_self_table(r, t, inter, B, total_step);
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

SelfSel make_sel(double required_clearance, int require_in_range, double required_self_clearance, int* best,
                 int* n_eligible, double* traj_best, double* dense_best) {
  SelfSel sel;
  sel.required_clearance = required_clearance; sel.require_in_range = require_in_range;
  sel.required_self_clearance = required_self_clearance;
  sel.best = best; sel.n_eligible = n_eligible; sel.traj_best = traj_best; sel.dense_best = dense_best;
  return sel;
}

}  // namespace

// Scores the plan's resident result against `t` on `st`; sel != null: k_score for the same rows first (its records are
// the second set of the workspace), then the rule with both clearances and the copy of the chosen row.  host / out / sel
// as plan_score (score.hip); out.oor: invalid.
int g2::plan_self_score(gpmp2mi_plan* p, const gpmp2mi_self_pairs* t, int inter, const ScoreOut& out, const SelfSel* sel,
                    bool host, hipStream_t st) {
  G2_CHECK(p && t, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_plan_ready(p, inter));
  const PlanParams& P = p->hp;
  G2_TRY(check_self_table(p->robot, t, inter, P.B, P.N));
  G2_CHECK(t->P == 0 || t->device == p->device, GPMP2MI_ERR_INVALID, "the pair table lives on another device than the plan");
  const int S = p->robot->h.nr_spheres, Md = P.N * (inter + 1) + 1;
  const size_t rec_bytes = (size_t)P.B * self_blocks(Md, S) * sizeof(ScoreRec);
  const size_t obs_bytes = (size_t)P.B * score_blocks(Md) * sizeof(ScoreRec);
  RowOut rows[SCORE_ROWS];
  rows_of(out, SELF_WORST, rows);
  const auto layout = [&](void* base) { return carve_self((char*)base, rec_bytes, obs_bytes, rows, shape_of(p, inter)); };
  CheckWs w;
  G2_TRY(carve_into(p->ws[p->WS_SELF], layout, &w));
  SelfFinish f{};
  const ScoreOut o = score_out(rows, host);
  f.support = o.support;
  f.dense = o.dense;
  f.clearance = o.clearance;
  f.worst = o.worst;
  f.invalid = o.oor;
  f.recs = (ScoreRec*)w.recs;
  f.nblk = self_blocks(Md, S);
  plan_shape(f.sel, p, inter);
  if (sel) {
    point_selection(f.sel, p, *sel, nullptr, host, w.sel);
    f.sel.recs = (ScoreRec*)w.recs2;
    f.sel.nblk = score_blocks(Md);
    f.required_self_clearance = sel->required_self_clearance;
  }
  p->mark_dirty(st);
  if (sel)
    G2_TRY(launch_score(p->robot->h, p->robot->d, p->sdf->h, P.delta_t, inter, P.B, P.N, p->pb.result, (ScoreRec*)w.recs2, st));
  G2_TRY(launch_self_clearance(p->robot->h, p->robot->d, t->d, t->P, P.delta_t, inter, P.B, P.N, p->pb.result,
                               (ScoreRec*)w.recs, st));
  G2_TRY(launch_self_finish(f, st));
  return host ? finish_host(p, inter, rows, SCORE_ROWS, sel, nullptr, w.sel, st) : GPMP2MI_OK;
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
  const int Md = total_step * (inter_step + 1) + 1;
  const int nblk = self_blocks(Md, t->S);
  std::unique_lock<std::mutex> lk;
  G2_TRY(records_ready(r, t, t->ws, (size_t)B * nblk * sizeof(ScoreRec), lk));
  SelfFinish f{};
  f.sel.B = B;
  f.recs = (ScoreRec*)t->ws.p;
  f.nblk = nblk;
  f.support = self_support_cost;
  f.dense = self_dense_cost;
  f.clearance = min_self_clearance;
  f.worst = worst;
  f.invalid = invalid;
  G2_TRY(launch_self_clearance(r->h, r->d, t->d, t->P, delta_t, inter_step, B, total_step, traj, (ScoreRec*)t->ws.p,
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
  return plan_self_score(p, t, inter_step, make_out(self_support_cost, self_dense_cost, min_self_clearance, worst, invalid),
                         nullptr, true, nullptr);
}
int gpmp2mi_plan_self_score_dev(gpmp2mi_plan* p, const gpmp2mi_self_pairs* t, int inter_step, double* self_support_cost,
                                double* self_dense_cost, double* min_self_clearance, int* worst, int* invalid,
                                void* stream) {
  return plan_self_score(p, t, inter_step, make_out(self_support_cost, self_dense_cost, min_self_clearance, worst, invalid),
                         nullptr, false, (hipStream_t)stream);
}

int gpmp2mi_plan_select_checked(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                const gpmp2mi_self_pairs* t, double required_self_clearance, int* best, int* n_eligible,
                                double* traj_best, double* dense_best) {
  const SelfSel sel = make_sel(required_clearance, require_in_range, required_self_clearance, best, n_eligible, traj_best,
                               dense_best);
  return plan_self_score(p, t, inter_step, ScoreOut{}, &sel, true, nullptr);
}
int gpmp2mi_plan_select_checked_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                    const gpmp2mi_self_pairs* t, double required_self_clearance, int* best,
                                    int* n_eligible, double* traj_best, double* dense_best, void* stream) {
  const SelfSel sel = make_sel(required_clearance, require_in_range, required_self_clearance, best, n_eligible, traj_best,
                               dense_best);
  return plan_self_score(p, t, inter_step, ScoreOut{}, &sel, false, (hipStream_t)stream);
}

}  // extern "C"
