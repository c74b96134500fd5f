// ik.hip -- "goal configurations" (include/gpmp2mi.h): the argument rules, the IK forms (one kernel, nothing allocated)
// and the goal stage: IK -> rows (clearance, eligibility, score) -> per pose the pair kernel and the rule kernel of
// "distinct alternatives" (group_kernels.hip, untouched) -> the leaders' rows.  Kernels: ik_kernels.hip.
#include <cmath>
#include <limits>

#include "host.h"
#include "../group_rule.h"

using namespace g2;

namespace {

struct Seeding {
  const double* seeds;   // device [G][M][D], or null: drawn
  uint64_t seed;
  int first;
};

// everything that can be refused without the device; fills the kernel's arguments from the options
int check_ik(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, int G, const double* des, int M, bool need_seeds,
             const Seeding& sd, IkArgs* out) {
  G2_CHECK(r && o && des, GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK(!need_seeds || sd.seeds, GPMP2MI_ERR_INVALID, "null seeds");
  G2_CHECK(G >= 0 && M >= 0, GPMP2MI_ERR_INVALID, "G and M must be >= 0");
  G2_CHECK(sd.first >= 0, GPMP2MI_ERR_INVALID, "first must be >= 0");
  G2_CHECK(o->mode == GPMP2MI_WORKSPACE_POSITION || o->mode == GPMP2MI_WORKSPACE_ORIENTATION ||
               o->mode == GPMP2MI_WORKSPACE_POSE,
           GPMP2MI_ERR_INVALID, "unknown mode");
  G2_CHECK(o->pos_tol > 0.0 && o->rot_tol > 0.0, GPMP2MI_ERR_INVALID, "pos_tol and rot_tol must be > 0");
  G2_CHECK(o->rot_weight > 0.0, GPMP2MI_ERR_INVALID, "rot_weight must be > 0");
  G2_CHECK(o->lambda_initial > 0.0 && o->lambda_factor > 0.0 && o->lambda_lower > 0.0 && o->lambda_upper > 0.0,
           GPMP2MI_ERR_INVALID, "lambda_initial, lambda_factor, lambda_lower and lambda_upper must be > 0");
  G2_CHECK(o->lambda_lower <= o->lambda_upper, GPMP2MI_ERR_INVALID, "lambda_lower must be <= lambda_upper");
  G2_CHECK(o->max_iter >= 1 && o->max_iter <= GPMP2MI_IK_MAX_ITER, GPMP2MI_ERR_INVALID,
           "max_iter must be in 1..GPMP2MI_IK_MAX_ITER");
  G2_CHECK((o->pos_down == nullptr) == (o->pos_up == nullptr), GPMP2MI_ERR_INVALID,
           "pos_down and pos_up go together");
  G2_CHECK(sd.seeds || o->pos_down, GPMP2MI_ERR_INVALID, "the seeded forms need joint limits");
  G2_CHECK((long long)G * M < (1ll << 31) / 32, GPMP2MI_ERR_INVALID, "too many problems for one launch");
  // from here on the robot handle is read
  G2_CHECK(r->h.kind == GPMP2MI_ROBOT_ARM, GPMP2MI_ERR_UNSUPPORTED,
           "inverse kinematics is built for GPMP2MI_ROBOT_ARM only (the Pose2 kinds need a retraction on the base)");
  G2_CHECK(r->h.dof >= 1 && r->h.dof <= IK_MAX_DOF, GPMP2MI_ERR_UNSUPPORTED,
           "inverse kinematics is instantiated for arms of dof 1..7");
  G2_CHECK(o->link >= 0 && o->link < r->h.nr_links, GPMP2MI_ERR_INVALID, "link out of range");
  IkArgs a{};
  const double inf = std::numeric_limits<double>::infinity();
  for (int d = 0; d < IK_MAX_DOF; d++) {
    a.down[d] = -inf;
    a.up[d] = inf;
    if (d >= r->h.dof || !o->pos_down) continue;
    a.down[d] = o->pos_down[d];
    a.up[d] = o->pos_up[d];
    G2_CHECK(a.down[d] <= a.up[d], GPMP2MI_ERR_INVALID, "pos_down must be <= pos_up (NaN is refused)");
    G2_CHECK(sd.seeds || (std::isfinite(a.down[d]) && std::isfinite(a.up[d])), GPMP2MI_ERR_INVALID,
             "the seeded forms need finite joint limits");
  }
  a.G = G;
  a.M = M;
  a.mode = o->mode;
  a.link = o->link;
  a.max_iter = o->max_iter;
  a.first = sd.first;
  a.pos_tol = o->pos_tol;
  a.rot_tol = o->rot_tol;
  a.rot_weight = o->rot_weight;
  a.lam0 = o->lambda_initial;
  a.lam_factor = o->lambda_factor;
  a.lam_lo = o->lambda_lower;
  a.lam_hi = o->lambda_upper;
  a.seed = sd.seed;
  a.des = des;
  a.seeds = sd.seeds;
  *out = a;
  return GPMP2MI_OK;
}

int check_current(const gpmp2mi_robot* r) {
  int dev = -1;
  G2_HIP(hipGetDevice(&dev));
  G2_CHECK(dev == r->device, GPMP2MI_ERR_INVALID, "the robot handle lives on another device than the current one");
  return GPMP2MI_OK;
}

int ik_solve_dev(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, int G, const double* des, int M, bool need_seeds,
                 const Seeding& sd, double* conf, double* residual, int* iters, int* status, hipStream_t st) {
  IkArgs a;
  G2_TRY(check_ik(r, o, G, des, M, need_seeds, sd, &a));
  if (G == 0 || M == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  G2_TRY(check_current(r));
  a.conf = conf;
  a.residual = residual;
  a.iters = iters;
  a.status = status;
  return launch_ik(r->h, r->d, a, st);
}

int ik_solve_host(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, int G, const double* des, int M, bool need_seeds,
                  const double* seeds, uint64_t seed, int first, double* conf, double* residual, int* iters,
                  int* status) {
  IkArgs a;
  G2_TRY(check_ik(r, o, G, des, M, need_seeds, Seeding{seeds, seed, first}, &a));
  if (G == 0 || M == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const size_t P = (size_t)G * M, D = r->h.dof;
  DevBuf<double> dd, ds, dc, dr;
  DevBuf<int> di, dst;
  G2_TRY(dd.upload(des, (size_t)G * 16));
  if (seeds) G2_TRY(ds.upload(seeds, P * D));
  if (conf) G2_TRY(dc.out(conf, P * D));
  if (residual) G2_TRY(dr.out(residual, P * 2));
  if (iters) G2_TRY(di.out(iters, P));
  if (status) G2_TRY(dst.out(status, P));
  G2_TRY(ik_solve_dev(r, o, G, dd.p, M, need_seeds, Seeding{ds.p, seed, first}, dc.p, dr.p, di.p, dst.p, nullptr));
  return fetch_all(dc, dr, di, dst);
}

struct GoalArgs {
  const gpmp2mi_sdf* sdf;
  double required_clearance;
  int require_in_range;
  const double *near_conf, *weights;   // host
  double radius;
  int max_goals;
  double* conf;
  int* status;
  double* clearance;
  int *oor, *mode, *n_goals, *n_converged, *n_eligible;
  double* goal_conf;
  int* goal_seed;
  double *goal_score, *goal_clearance;
};

// the goal stage's rules that need no handle, ahead of check_ik; check_goals: those that read the robot's dof
int check_goal_sizes(double radius, int max_goals) {
  G2_CHECK(radius >= 0.0, GPMP2MI_ERR_INVALID, "radius must be >= 0 (NaN is refused)");
  G2_CHECK(max_goals >= 1 && max_goals <= GPMP2MI_MAX_ALTERNATIVES, GPMP2MI_ERR_INVALID,
           "max_goals must be in 1..GPMP2MI_MAX_ALTERNATIVES");
  return GPMP2MI_OK;
}
int check_goals(const gpmp2mi_robot* r, int M, const GoalArgs& g) {
  G2_CHECK(g.required_clearance == g.required_clearance, GPMP2MI_ERR_INVALID, "required_clearance is NaN");
  G2_CHECK(M <= GPMP2MI_MAX_GROUP_ROWS, GPMP2MI_ERR_UNSUPPORTED,
           "more than GPMP2MI_MAX_GROUP_ROWS = " + std::to_string(GPMP2MI_MAX_GROUP_ROWS) + " seed rows per pose");
  for (int d = 0; d < r->h.dof; d++) {
    G2_CHECK(!g.near_conf || std::isfinite(g.near_conf[d]), GPMP2MI_ERR_INVALID, "near is not finite");
    G2_CHECK(!g.weights || (std::isfinite(g.weights[d]) && g.weights[d] >= 0.0), GPMP2MI_ERR_INVALID,
             "a weight is negative or not finite");
  }
  return GPMP2MI_OK;
}

// device pointers throughout; allocates the workspace and waits for `st` before it goes
int ik_goals_dev(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, int G, const double* des, int M, const Seeding& sd,
                 const GoalArgs& g, hipStream_t st) {
  IkArgs a;
  // the checks that need no handle first (a refused call never looks at one)
  G2_TRY(check_goal_sizes(g.radius, g.max_goals));
  G2_TRY(check_ik(r, o, G, des, M, false, sd, &a));
  G2_TRY(check_goals(r, M, g));
  if (g.sdf) {
    const int dim = g.sdf->h.dim;
    G2_CHECK(dim == 2 || dim == 3, GPMP2MI_ERR_INVALID, "the field is neither planar nor a volume");
  }
  if (G == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  G2_TRY(check_current(r));
  const int D = r->h.dof, W = group_words(M);
  const size_t P = (size_t)G * M;
  // the workspace: what the caller did not give room for, and what only the stages among themselves read
  Carver take{nullptr};   // a null base: the offsets, until the size is known and the block allocated
  const size_t o_conf = (size_t)take(g.conf ? 0 : P * D * sizeof(double)), o_clr = (size_t)take(g.clearance ? 0 : P * sizeof(double)),
               o_score = (size_t)take(P * sizeof(double)), o_stage = (size_t)take(P * 2 * D * sizeof(double)),
               o_bits = (size_t)take(P * W * sizeof(unsigned long long)), o_status = (size_t)take(g.status ? 0 : P * sizeof(int)),
               o_el = (size_t)take(P * sizeof(int)), o_lead = (size_t)take(P * sizeof(int)), o_nm = (size_t)take((size_t)G * sizeof(int)),
               o_ne = (size_t)take((size_t)G * sizeof(int));
  DevBuf<char> ws;
  G2_TRY(ws.alloc(take.off));
  struct Wait {   // also on an error path: nothing may still use the workspace when it goes
    hipStream_t st;
    ~Wait() { (void)hipStreamSynchronize(st); }
  } wait{st};
  double* conf = g.conf ? g.conf : (double*)(ws.p + o_conf);
  double* clr = g.clearance ? g.clearance : (double*)(ws.p + o_clr);
  int* status = g.status ? g.status : (int*)(ws.p + o_status);
  double* score = (double*)(ws.p + o_score);
  double* stage = (double*)(ws.p + o_stage);
  unsigned long long* bits = (unsigned long long*)(ws.p + o_bits);
  int *el = (int*)(ws.p + o_el), *lead = (int*)(ws.p + o_lead), *nm = (int*)(ws.p + o_nm), *ne = (int*)(ws.p + o_ne);
  if (M == 0) {   // no rows: the counts are 0 and every goal_seed is -1
    G2_HIP(hipMemsetAsync(nm, 0, (size_t)G * sizeof(int), st));
    G2_HIP(hipMemsetAsync(ne, 0, (size_t)G * sizeof(int), st));
  } else {
    a.conf = conf;
    a.status = status;
    G2_TRY(launch_ik(r->h, r->d, a, st));
    IkRows w{};
    w.G = G;
    w.M = M;
    w.has_near = g.near_conf != nullptr;
    w.require_in_range = g.require_in_range;
    w.required_clearance = g.required_clearance;
    for (int d = 0; d < IK_MAX_DOF; d++) {
      w.near_conf[d] = (g.near_conf && d < D) ? g.near_conf[d] : 0.0;
      w.w[d] = (g.weights && d < D) ? g.weights[d] : 1.0;
    }
    w.conf = conf;
    w.status = status;
    w.clearance = clr;
    w.score = score;
    w.stage = stage;
    w.oor = g.oor;
    w.eligible = el;
    G2_TRY(launch_ik_rows(r->h, r->d, g.sdf ? &g.sdf->h : nullptr, w, st));
    for (int i = 0; i < G; i++) {   // the rule kernel is one workgroup per batch: one launch per pose
      PairArgs pa{};
      pa.B = M;
      pa.N = 0;   // rows of one state
      pa.D = D;
      pa.metric = GPMP2MI_DIST_MAX_STATE;
      pa.traj = stage + (size_t)i * M * 2 * D;
      for (int d = 0; d < GPMP2MI_MAX_DOF; d++) pa.w[d] = d < D ? w.w[d] : 1.0;
      pa.radius = g.radius;
      pa.bits = bits + (size_t)i * M * W;
      G2_TRY(launch_traj_pairs(pa, st));
      GroupRule gr{};
      gr.B = M;
      gr.radius = g.radius;
      gr.bits = pa.bits;
      gr.score = score + (size_t)i * M;
      gr.eligible = el + (size_t)i * M;
      gr.mode = g.mode ? g.mode + (size_t)i * M : nullptr;
      gr.leaders = lead + (size_t)i * M;
      gr.n_modes = nm + i;
      gr.n_eligible = ne + i;
      G2_TRY(launch_group_rule(gr, st));
    }
  }
  IkGoalCopy c{};
  c.M = M;
  c.D = D;
  c.max_goals = g.max_goals;
  c.conf = conf;
  c.score = score;
  c.clearance = clr;
  c.status = status;
  c.leaders = lead;
  c.n_modes = nm;
  c.n_eligible = ne;
  c.n_goals = g.n_goals;
  c.n_converged = g.n_converged;
  c.out_n_eligible = g.n_eligible;
  c.goal_seed = g.goal_seed;
  c.goal_conf = g.goal_conf;
  c.goal_score = g.goal_score;
  c.goal_clearance = g.goal_clearance;
  return launch_ik_goal_copy(c, G, st);
}

}  // namespace

extern "C" {

void gpmp2mi_ik_opts_default(gpmp2mi_ik_opts* o) {
  if (!o) return;
  o->mode = GPMP2MI_WORKSPACE_POSE;
  o->link = 0;
  o->pos_tol = 1e-6;
  o->rot_tol = 1e-6;
  o->rot_weight = 1.0;
  o->max_iter = 100;
  o->lambda_initial = 1e-2;
  o->lambda_factor = 4.0;
  o->lambda_lower = 1e-9;
  o->lambda_upper = 1e6;
  o->pos_down = nullptr;
  o->pos_up = nullptr;
}

int gpmp2mi_ik_solve(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, int G, const double* des_pose, int M,
                     const double* seeds, double* conf, double* residual, int* iters, int* status) {
  return ik_solve_host(r, o, G, des_pose, M, true, seeds, 0, 0, conf, residual, iters, status);
}
int gpmp2mi_ik_solve_dev(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, int G, const double* des_pose, int M,
                         const double* seeds, double* conf, double* residual, int* iters, int* status, void* stream) {
  return ik_solve_dev(r, o, G, des_pose, M, true, Seeding{seeds, 0, 0}, conf, residual, iters, status,
                      (hipStream_t)stream);
}
int gpmp2mi_ik_solve_seeded(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, int G, const double* des_pose, int M,
                            uint64_t seed, int first, double* conf, double* residual, int* iters, int* status) {
  return ik_solve_host(r, o, G, des_pose, M, false, nullptr, seed, first, conf, residual, iters, status);
}
int gpmp2mi_ik_solve_seeded_dev(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, int G, const double* des_pose, int M,
                                uint64_t seed, int first, double* conf, double* residual, int* iters, int* status,
                                void* stream) {
  return ik_solve_dev(r, o, G, des_pose, M, false, Seeding{nullptr, seed, first}, conf, residual, iters, status,
                      (hipStream_t)stream);
}

int gpmp2mi_ik_goals_dev(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, const gpmp2mi_sdf* sdf, int G,
                         const double* des_pose, int M, const double* seeds, uint64_t seed, int first,
                         double required_clearance, int require_in_range, const double* near_conf, const double* weights,
                         double radius, int max_goals, double* conf, int* status, double* clearance, int* out_of_range,
                         int* mode, int* n_goals, int* n_converged, int* n_eligible, double* goal_conf, int* goal_seed,
                         double* goal_score, double* goal_clearance, void* stream) {
  const GoalArgs g{sdf, required_clearance, require_in_range, near_conf, weights, radius, max_goals, conf, status,
                   clearance, out_of_range, mode, n_goals, n_converged, n_eligible, goal_conf, goal_seed, goal_score,
                   goal_clearance};
  return ik_goals_dev(r, o, G, des_pose, M, Seeding{seeds, seed, first}, g, (hipStream_t)stream);
}

int gpmp2mi_ik_goals(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, const gpmp2mi_sdf* sdf, int G,
                     const double* des_pose, int M, const double* seeds, uint64_t seed, int first,
                     double required_clearance, int require_in_range, const double* near_conf, const double* weights,
                     double radius, int max_goals, double* conf, int* status, double* clearance, int* out_of_range,
                     int* mode, int* n_goals, int* n_converged, int* n_eligible, double* goal_conf, int* goal_seed,
                     double* goal_score, double* goal_clearance) {
  GoalArgs g{sdf, required_clearance, require_in_range, near_conf, weights, radius, max_goals, nullptr, nullptr,
             nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  IkArgs a;
  G2_TRY(check_goal_sizes(radius, max_goals));
  // des_pose / seeds stand in for their device copies: check_ik tests them for null only
  G2_TRY(check_ik(r, o, G, des_pose, M, false, Seeding{seeds, seed, first}, &a));
  G2_TRY(check_goals(r, M, g));
  if (G == 0) return GPMP2MI_OK;
  if (M == 0) {   // no rows: nothing to launch
    for (int i = 0; i < G; i++) {
      if (n_goals) n_goals[i] = 0;
      if (n_converged) n_converged[i] = 0;
      if (n_eligible) n_eligible[i] = 0;
      for (int k = 0; goal_seed && k < max_goals; k++) goal_seed[(size_t)i * max_goals + k] = -1;
    }
    return GPMP2MI_OK;
  }
  G2_TRY(ensure_device());
  const size_t P = (size_t)G * M, D = r->h.dof, K = (size_t)G * max_goals;
  DevBuf<double> dd, ds, dc, dcl, dgc, dgs, dgl;
  DevBuf<int> dst, doo, dm, dng, dnc, dne, dgi;
  G2_TRY(dd.upload(des_pose, (size_t)G * 16));
  if (seeds) G2_TRY(ds.upload(seeds, P * D));
  if (conf) G2_TRY(dc.out(conf, P * D));
  if (status) G2_TRY(dst.out(status, P));
  if (clearance) G2_TRY(dcl.out(clearance, P));
  if (out_of_range) G2_TRY(doo.out(out_of_range, P));
  if (mode) G2_TRY(dm.out(mode, P));
  if (n_goals) G2_TRY(dng.out(n_goals, G));
  if (n_converged) G2_TRY(dnc.out(n_converged, G));
  if (n_eligible) G2_TRY(dne.out(n_eligible, G));
  // "untouched beyond n_goals": the caller's values go up first and come back where the kernel left them
  if (goal_conf) G2_TRY(dgc.upload(goal_conf, K * D));
  if (goal_score) G2_TRY(dgs.upload(goal_score, K));
  if (goal_clearance) G2_TRY(dgl.upload(goal_clearance, K));
  dgc.host = goal_conf;
  dgs.host = goal_score;
  dgl.host = goal_clearance;
  if (goal_seed) G2_TRY(dgi.out(goal_seed, K));
  g.conf = dc.p;
  g.status = dst.p;
  g.clearance = dcl.p;
  g.oor = doo.p;
  g.mode = dm.p;
  g.n_goals = dng.p;
  g.n_converged = dnc.p;
  g.n_eligible = dne.p;
  g.goal_conf = dgc.p;
  g.goal_seed = dgi.p;
  g.goal_score = dgs.p;
  g.goal_clearance = dgl.p;
  G2_TRY(ik_goals_dev(r, o, G, dd.p, M, Seeding{ds.p, seed, first}, g, nullptr));
  return fetch_all(dc, dst, dcl, doo, dm, dng, dnc, dne, dgc, dgi, dgs, dgl);
}

}  // extern "C"
