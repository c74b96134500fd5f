// plan_create.hip -- where a plan's memory comes from and goes back to (the pinned-flag pool, the arena-chunk pool,
// plan_alloc), the choice of its kernel forms, and plan create / destroy.
#include <cmath>
#include <cstring>
#include <mutex>

#include "host.h"
#include "../cr_schedule.h"
#include "../dispatch.h"

namespace g2 {
// Host-mapped pass-flag arrays are recycled across plans: pinning and unpinning host memory costs more than the
// whole solve of a small plan (one-shot gpmp2mi_batch_optimize calls create and destroy a plan each time).
static std::mutex g_flag_mu;   // guards g_flag_pool and g_chunk_pool
static std::vector<FlagBuf> g_flag_pool;
// live-resource counters for the lifetime tests (gpmp2mi_debug_resource_counts)
static std::atomic<long> g_live_chunks{0}, g_live_flagbufs{0}, g_leaked_plans{0};
int flags_acquire(int need, FlagBuf* out) {
  {
    std::lock_guard<std::mutex> lk(g_flag_mu);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (size_t k = 0; k < g_flag_pool.size(); k++)
      if (g_flag_pool[k].cap >= need && g_flag_pool[k].device == cur) {
        *out = g_flag_pool[k];
        g_flag_pool.erase(g_flag_pool.begin() + k);
        g_live_flagbufs.fetch_add(1);
        return GPMP2MI_OK;
      }
  }
  FlagBuf f;
  (void)hipGetDevice(&f.device);
  f.cap = std::max(need, 1024);
  G2_HIP(hipHostMalloc((void**)&f.host, (size_t)f.cap * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
  G2_HIP(hipHostGetDevicePointer((void**)&f.dev, f.host, 0));
  g_live_flagbufs.fetch_add(1);
  *out = f;
  return GPMP2MI_OK;
}
void flags_release(const FlagBuf& f) {
  if (!f.host) return;
  g_live_flagbufs.fetch_sub(1);
  std::lock_guard<std::mutex> lk(g_flag_mu);
  if (g_flag_pool.size() < 16) g_flag_pool.push_back(f);
  else (void)hipHostFree(f.host);
}

// Plan buffers come out of a few zero-filled arena chunks instead of one hipMalloc + hipMemset + hipFree each (a plan
// has about 65 of them: 0.6 ms of a one-shot gpmp2mi_batch_optimize call was allocation and release).
// standard-size chunks are recycled as well (zero-filled again on reuse); larger ones go back to the driver
constexpr size_t ARENA_CHUNK = (size_t)8 << 20;
static std::vector<std::pair<void*, int>> g_chunk_pool;   // (chunk, device); guarded by g_flag_mu
static void* chunk_acquire() {
  int cur = 0;
  (void)hipGetDevice(&cur);
  std::lock_guard<std::mutex> lk(g_flag_mu);
  for (size_t k = 0; k < g_chunk_pool.size(); k++)
    if (g_chunk_pool[k].second == cur) {
      void* q = g_chunk_pool[k].first;
      g_chunk_pool.erase(g_chunk_pool.begin() + k);
      return q;
    }
  return nullptr;
}
static void chunk_release(void* q, int device) {
  {
    std::lock_guard<std::mutex> lk(g_flag_mu);
    if (g_chunk_pool.size() < 8) {
      g_chunk_pool.push_back({q, device});
      return;
    }
  }
  (void)hipFree(q);
}
}  // namespace g2

using namespace g2;

// Returns every arena chunk and the flag buffer (also on a create that failed half-way: the unique_ptr in
// gpmp2mi_plan_create runs this).  The caller has drained the plan's streams.
gpmp2mi_plan::~gpmp2mi_plan() {
  if (poisoned) {
    g_leaked_plans.fetch_add(1);
    for (Workspace& w : ws) w.leak();   // the members are destroyed behind this body: hipFree would wait for the kernel
    return;
  }
  drain();
  for (size_t k = 0; k < allocs.size(); k++) {
    g_live_chunks.fetch_sub(1);
    if (alloc_bytes[k] == ARENA_CHUNK) chunk_release(allocs[k], device);
    else (void)hipFree(allocs[k]);
  }
  flags_release(flagbuf);
  if (risk_qc) (void)hipFree(risk_qc);
  sampled_fac.release();
  flags_release(qflags);
}

template <class T>
static int plan_alloc(gpmp2mi_plan* p, T** ptr, size_t count) {
  constexpr size_t ALIGN = 256, CHUNK = ARENA_CHUNK;
  const size_t bytes = (std::max<size_t>(count, 1) * sizeof(T) + ALIGN - 1) / ALIGN * ALIGN;
  // fail_alloc_at (tests): fails as if the device were out of memory, so that the half-built plan's release path runs
  if (++p->alloc_calls == p->fail_alloc_at) {
    set_error("hipMalloc: injected failure (gpmp2mi_debug_forms::fail_alloc_at)");
    return GPMP2MI_ERR_ALLOC;
  }
  if (bytes > p->arena_left) {
    const size_t chunk = std::max(bytes, CHUNK);
    void* q = (chunk == CHUNK) ? chunk_acquire() : nullptr;
    if (!q) G2_TRY(dev_malloc(&q, chunk));
    // owned by the plan from here on: a failing memset below is released with everything else by ~gpmp2mi_plan
    p->allocs.push_back(q);
    p->alloc_bytes.push_back(chunk);
    g_live_chunks.fetch_add(1);
    p->arena_cur = (char*)q;
    p->arena_left = chunk;
    p->null_stream_dirty = true;   // the zero fill runs on the null stream; plan_create's closing copy waits for it
    G2_HIP(hipMemsetAsync(q, 0, chunk, nullptr));
  }
  *ptr = (T*)p->arena_cur;
  p->arena_cur += bytes;
  p->arena_left -= bytes;
  return GPMP2MI_OK;
}

// The one place where a plan's forms are decided.  `force` (gpmp2mi_debug_plan_create, NULL: none) overrides the choice;
// a forced form the plan cannot take is refused.
static int choose_forms(const RobotDev& h, const gpmp2mi_settings& s, int B, const gpmp2mi_debug_forms* force,
                        PlanForms* out) {
  const gpmp2mi_debug_forms f = force ? *force : gpmp2mi_debug_forms{};
  const int D = h.dof, N = s.total_step, I = s.obs_check_inter;
  const bool fixed_arm = h.kind == GPMP2MI_ROBOT_ARM;
  G2_CHECK(f.lin_split == 0 || f.lin_split == 1 || (fixed_arm && (f.lin_split == 2 || f.lin_split == 4)), GPMP2MI_ERR_UNSUPPORTED,
           "forced lin_split: 1, or 2 / 4 on a fixed-base arm");
  // (the four-wavefront form keeps the <= ZNS states of a chunk in LDS: two or more sub-steps per interval)
  static_assert(chunk_states(2) <= ZNS && chunk_states(1) > ZNS, "the I >= 2 below and at the default choice");
  G2_CHECK(f.lin_split != 4 || I >= 2, GPMP2MI_ERR_UNSUPPORTED, "forced lin_split 4: needs obs_check_inter >= 2");
  PlanForms F;
  F.wide = 2 * D > 15;
  G2_CHECK(!f.wide_dense || F.wide, GPMP2MI_ERR_UNSUPPORTED, "forced wide_dense: the plan has no wide blocks (dof < 8)");
  F.dense = D > 11 || f.wide_dense;
  F.split_back = !F.dense && N >= 16;   // the finish kernels take groups of 8 blocks (levels 4, 2, 1)
  // wide blocks: the first forward levels (2, 4) run chip-wide when they are not among the last two of the tree (up to
  // level 8; 16 measured: see DESIGN)
  while (F.wide && F.wide_h0 < 8 && 4 * F.wide_h0 <= N) F.wide_h0 *= 2;
  // sphere-split linearization for fixed-base arms: four wavefronts per 64 points sharing one walk of the chain
  // (k_linearize_arm), or two wavefronts that each walk it (k_linearize NSPLIT = 2).  Alone, the four-wavefront form wins
  // up to 256 trajectories (round 3: 14.4 / 16.8 / 22.5 / 35.5 / 59.3 us against 17.6 / 18.7 / 24.2 / 35.6 / 58.1 us at
  // 32 / 64 / 128 / 256 / 512); with the fused finish, which only it has, it wins the Gauss-Newton pass at every size
  // (195.3 / 226.9 / 224.8 k against 193.4 / 225.1 / 218.6 k traj/s at 256 / 512 / 1 024), and the LM pass too, if barely
  // (97.7 / 102.0 k against 96.6 / 101.3 k at 512 / 1 024).  So: Gauss-Newton and LM plans always, Dogleg plans (no fusion
  // there) up to 256 trajectories.
  const bool four = B <= 256 || s.opt_type != GPMP2MI_OPT_DOGLEG;
  F.lin_split = (fixed_arm && h.nr_spheres >= 2) ? (four ? 4 : 2) : 1;
  if (F.lin_split == 4 && I < 2) F.lin_split = 2;
  if (f.lin_split) F.lin_split = f.lin_split;
  // fused finish (k_linearize_arm applies the step: GN fast path, LM / GN trial steps); the trial-step shares then come
  // per chunk of 64 of the 1 + N (I + 1) evaluation points instead of per group of 8 blocks (k_finish_trial)
  F.fuse_finish = F.lin_split == 4 && F.split_back && !F.wide && !f.no_fused_finish;
  F.spart_groups = F.fuse_finish ? (1 + N * (I + 1) + 63) / 64 : F.wide ? (N + 8) / 8 : crr_groups(N, 8);
  F.generic_gn = f.generic_gn != 0;
  F.no_early_stop = f.no_early_stop != 0;
  *out = F;
  return GPMP2MI_OK;
}

// PlanParams from robot, settings, options and forms: pure host arithmetic, the GP blocks included
static int fill_params(const RobotDev& h, const gpmp2mi_settings* s, const gpmp2mi_graph_opts& o, const PlanForms& F,
                       int B, PlanParams& P) {
  const int D = h.dof;
  std::memset(&P, 0, sizeof(P));
  P.B = B;
  P.N = s->total_step;
  P.I = s->obs_check_inter;
  P.P = 1 + P.N * (P.I + 1);
  P.Ppad = (P.P + 63) / 64 * 64;
  P.D = D;
  P.n = 2 * D;
  P.NG = D * (D + 1) / 2;
  P.REC = P.NG + D + 1 + ((h.base_dof == 3 && P.I > 0) ? 36 : 0);
  P.Npad = (P.N + 1 + 63) / 64 * 64;
  P.lie = h.base_dof == 3 ? 1 : 0;
  P.wide = F.wide; P.split_back = F.split_back; P.spart_groups = F.spart_groups;
  P.wide_h0 = F.wide_h0; P.lin_split = F.lin_split; P.fuse_finish = F.fuse_finish;
  P.GPREC = P.n + 1 + (P.lie ? 18 : 0);
  P.RECS = (P.REC + 1) & ~1;
  P.GPS = (P.GPREC + 1) & ~1;
  P.obs_skip_first = o.obs_skip_first_state;
  P.flag_pos_limit = s->flag_pos_limit;
  P.flag_vel_limit = s->flag_vel_limit;
  P.rules.opt_type = s->opt_type;
  P.rules.max_iter = s->max_iter;
  P.rules.no_increase = s->final_iter_no_increase;
  P.rules.fixed_iters = o.fixed_iterations;
  P.end_conf_prior_off = o.end_conf_prior_off ? 1 : 0;
  P.eps = s->epsilon;
  P.obs_w = 1.0 / (s->cost_sigma * s->cost_sigma);
  // planner/BatchTrajOptimizer-inl.h:30-31
  P.delta_t = s->total_time / static_cast<double>(s->total_step);
  const double inter_dt = P.delta_t / static_cast<double>(s->obs_check_inter + 1);
  P.conf_prior_w = 1.0 / (s->conf_prior_sigma * s->conf_prior_sigma);
  P.vel_prior_w = 1.0 / (s->vel_prior_sigma * s->vel_prior_sigma);
  P.vdyn_w = o.vehicle_dynamics_sigma > 0 ? 1.0 / (o.vehicle_dynamics_sigma * o.vehicle_dynamics_sigma) : 0.0;
  P.rules.rel_thresh = s->rel_thresh;
  P.rules.abs_tol = o.abs_error_tol;
  P.rules.err_tol = o.error_tol;
  P.rules.lm_lambda0 = o.lm_lambda_initial;
  P.rules.lm_factor = o.lm_lambda_factor;
  P.rules.lm_upper = o.lm_lambda_upper;
  P.rules.lm_lower = o.lm_lambda_lower;
  P.rules.lm_min_fidelity = o.lm_min_model_fidelity;
  P.rules.dl_delta0 = o.dogleg_delta_initial;
  for (int j = 0; j < P.I; j++) {
    P.coef[j] = gp_coef(P.delta_t, inter_dt * static_cast<double>(j + 1));
    const double lam[2] = {P.coef[j].l11, P.coef[j].l12}, psi[2] = {P.coef[j].p11, P.coef[j].p12};
    double* q = P.coefq[j];
    for (int ar = 0; ar < 2; ar++)
      for (int ac = 0; ac < 2; ac++) {
        q[0 + ar * 2 + ac] = psi[ar] * psi[ac];
        q[4 + ar * 2 + ac] = lam[ar] * lam[ac];
        q[8 + ar * 2 + ac] = lam[ar] * psi[ac];
        q[12 + ar * 2 + ac] = psi[ar] * lam[ac];
      }
    q[16] = lam[0]; q[17] = lam[1]; q[18] = psi[0]; q[19] = psi[1];
  }
  gp_winv(P.delta_t, P.Winv);
  std::vector<double> Qc(D * D, 0.0), Qi(D * D, 0.0);
  for (int i = 0; i < D; i++) Qc[i * D + i] = 1.0;
  if (s->Qc) std::copy(s->Qc, s->Qc + D * D, Qc.begin());
  G2_CHECK(invert_small(D, Qc.data(), Qi.data()), GPMP2MI_ERR_INVALID, "Qc is singular");
  std::copy(Qi.begin(), Qi.end(), P.Qc_inv);
  for (int k = 0; k < D; k++) {
    P.pos_lo[k] = s->joint_pos_limits_down ? s->joint_pos_limits_down[k] : -1e6;
    P.pos_hi[k] = s->joint_pos_limits_up ? s->joint_pos_limits_up[k] : 1e6;
    P.pos_th[k] = s->pos_limit_thresh ? s->pos_limit_thresh[k] : 1e-3;
    const double ps = s->pos_limit_sigmas ? s->pos_limit_sigmas[k] : 1e-3;
    P.pos_w[k] = 1.0 / (ps * ps);
    P.vel_lim[k] = s->vel_limits ? s->vel_limits[k] : 1e6;
    P.vel_th[k] = s->vel_limit_thresh ? s->vel_limit_thresh[k] : 1e-3;
    const double vs = s->vel_limit_sigmas ? s->vel_limit_sigmas[k] : 1e-3;
    P.vel_w[k] = 1.0 / (vs * vs);
  }
  // GP prior Hessian blocks: W = B(dt) (x) Qc^-1, Phi = [[I, dt I],[0, I]]
  {
    const int n = P.n;
    const double dt = P.delta_t;
    auto W = [&](int r, int c) { return P.Winv[(r / D) * 2 + (c / D)] * Qi[(r % D) * D + (c % D)]; };
    // (Phi^T W)[r][c] = W[r][c] for x rows; for v rows: dt * W[x row][c] + W[v row][c]
    auto PtW = [&](int r, int c) { return r < D ? W(r, c) : dt * W(r - D, c) + W(r, c); };
    for (int r = 0; r < n; r++)
      for (int c = 0; c < n; c++) {
        P.KB[r * n + c] = W(r, c);
        P.KO[r * n + c] = -PtW(r, c);
        // (Phi^T W Phi)[r][c] = PtW[r][c] for x cols; v cols: dt * PtW[r][x col] + PtW[r][c]
        P.KA[r * n + c] = c < D ? PtW(r, c) : dt * PtW(r, c - D) + PtW(r, c);
      }
  }
  // passes: GN one per iteration (+1); LM up to ~5 lambda retries per iterate; Dogleg up to ~16 halvings
  const int cap = std::max(P.rules.fixed_iters, P.rules.max_iter);   // plan_update may run any iterations <= max_iter
  P.max_pass = cap * (P.rules.opt_type == GPMP2MI_OPT_LM ? 6 : P.rules.opt_type == GPMP2MI_OPT_DOGLEG ? 18 : 1) + 3;
  return GPMP2MI_OK;
}

// host copies of the extra-factor data (desired poses, sphere pairs, radii in the caller's sphere order)
struct ExtrasHost {
  std::vector<double> des, scd, radius;
};
// extra factors as data: checked and copied to host vectors BEFORE the first allocation (an invalid description must
// not cost a round trip through the allocator)
static int check_extras(const RobotDev& h, const gpmp2mi_graph_opts& o, int N, PlanExtras& ex, ExtrasHost& hx) {
  std::memset(&ex, 0, sizeof(ex));
  G2_CHECK(o.n_workspace >= 0 && o.n_workspace <= GPMP2MI_MAX_WORKSPACE_FACTORS, GPMP2MI_ERR_INVALID, "too many workspace factors");
  G2_CHECK(o.n_self_collision >= 0 && o.n_self_collision <= GPMP2MI_MAX_SELF_COLLISION_PAIRS, GPMP2MI_ERR_INVALID,
           "too many self-collision pairs");
  ex.n_ws = o.n_workspace;
  ex.n_sc = o.n_self_collision;
  hx.des.assign(16 * std::max(ex.n_ws, 1), 0.0);
  hx.scd.assign(4 * std::max(ex.n_sc, 1), 0.0);
  hx.radius.assign(std::max(h.nr_spheres, 1), 0.0);
  for (int f = 0; f < ex.n_ws; f++) {
    const gpmp2mi_workspace_factor& w = o.workspace[f];
    G2_CHECK(w.mode >= GPMP2MI_WORKSPACE_POSITION && w.mode <= GPMP2MI_WORKSPACE_POSE, GPMP2MI_ERR_INVALID, "unknown workspace factor mode");
    G2_CHECK(w.link >= 0 && w.link < h.nr_links, GPMP2MI_ERR_INVALID, "workspace factor: link out of range");
    G2_CHECK(w.sigma > 0, GPMP2MI_ERR_INVALID, "workspace factor: sigma must be positive");
    G2_CHECK(w.first_state >= 0 && w.first_state <= w.last_state && w.last_state <= N, GPMP2MI_ERR_INVALID,
             "workspace factor: bad state range");
    ex.ws_mode[f] = w.mode;
    ex.ws_link[f] = w.link;
    ex.ws_first[f] = w.first_state;
    ex.ws_last[f] = w.last_state;
    ex.ws_w[f] = 1.0 / (w.sigma * w.sigma);
    std::copy(w.des_pose, w.des_pose + 16, hx.des.begin() + 16 * f);
  }
  if (ex.n_sc > 0) {
    G2_CHECK(o.self_collision_first >= 0 && o.self_collision_first <= o.self_collision_last && o.self_collision_last <= N,
             GPMP2MI_ERR_INVALID, "self collision: bad state range");
    ex.sc_first = o.self_collision_first;
    ex.sc_last = o.self_collision_last;
    for (int k = 0; k < ex.n_sc; k++) {
      const double a = o.self_collision[k][0], bb = o.self_collision[k][1], sg = o.self_collision[k][3];
      G2_CHECK(a >= 0 && a < h.nr_spheres && bb >= 0 && bb < h.nr_spheres, GPMP2MI_ERR_INVALID, "self collision: sphere id out of range");
      G2_CHECK(sg > 0, GPMP2MI_ERR_INVALID, "self collision: sigma must be positive");
      for (int t = 0; t < 4; t++) hx.scd[4 * k + t] = o.self_collision[k][t];
      ex.sc_w[k] = 1.0 / (sg * sg);
    }
  }
  G2_CHECK(o.max_moving_spheres >= 0 && o.max_moving_spheres <= GPMP2MI_MAX_MOVING_SPHERES, GPMP2MI_ERR_INVALID,
           "max_moving_spheres outside 0..GPMP2MI_MAX_MOVING_SPHERES");
  if (o.max_moving_spheres > 0) {
    G2_CHECK(o.moving_sigma > 0 && std::isfinite(o.moving_sigma), GPMP2MI_ERR_INVALID, "moving spheres: sigma must be positive");
    G2_CHECK(std::isfinite(o.moving_epsilon), GPMP2MI_ERR_INVALID, "moving spheres: epsilon must be finite");
    G2_CHECK(o.moving_first >= 0 && o.moving_first <= o.moving_last && o.moving_last <= N, GPMP2MI_ERR_INVALID,
             "moving spheres: bad state range");
    ex.mv_cap = o.max_moving_spheres;
    ex.mv_first = o.moving_first;
    ex.mv_last = o.moving_last;
    ex.mv_eps = o.moving_epsilon;
    ex.mv_w = 1.0 / (o.moving_sigma * o.moving_sigma);
  }
  G2_CHECK(o.max_self_pairs >= 0, GPMP2MI_ERR_INVALID, "max_self_pairs is negative");
  G2_CHECK(o.max_self_pairs <= GPMP2MI_MAX_PLAN_SELF_PAIRS, GPMP2MI_ERR_INVALID,
           "max_self_pairs above GPMP2MI_MAX_PLAN_SELF_PAIRS");
  if (o.max_self_pairs > 0) {
    G2_CHECK(o.self_pairs_first >= 0 && o.self_pairs_first <= o.self_pairs_last && o.self_pairs_last <= N,
             GPMP2MI_ERR_INVALID, "self-collision table: bad state range");
    ex.sp_cap = o.max_self_pairs;
    ex.sp_first = o.self_pairs_first;
    ex.sp_last = o.self_pairs_last;
  }
  G2_CHECK(o.max_carried_spheres >= 0 && o.max_carried_spheres <= GPMP2MI_MAX_CARRIED_SPHERES, GPMP2MI_ERR_INVALID,
           "max_carried_spheres outside 0..GPMP2MI_MAX_CARRIED_SPHERES");
  if (o.max_carried_spheres > 0) {   // without capacity the other four fields are not read
    G2_CHECK(o.carried_sigma > 0 && std::isfinite(o.carried_sigma), GPMP2MI_ERR_INVALID, "carried object: sigma must be positive");
    G2_CHECK(std::isfinite(o.carried_epsilon), GPMP2MI_ERR_INVALID, "carried object: epsilon must be finite");
    G2_CHECK(o.carried_first >= 0 && o.carried_first <= o.carried_last && o.carried_last <= N, GPMP2MI_ERR_INVALID,
             "carried object: bad state range");
    G2_DISPATCH_ROBOT_H(h, (void)0);   // a (kind, dof) the chain kernels are not instantiated for: GPMP2MI_ERR_UNSUPPORTED
    ex.cr_cap = o.max_carried_spheres;
    ex.cr_first = o.carried_first;
    ex.cr_last = o.carried_last;
    ex.cr_eps = o.carried_epsilon;
    ex.cr_w = 1.0 / (o.carried_sigma * o.carried_sigma);
  }
  // the robot's radii in the caller's sphere order: read by the self-collision rows and the moving-sphere factor
  if (ex.n_sc > 0 || ex.mv_cap > 0)
    for (int sidx = 0; sidx < h.nr_spheres; sidx++) hx.radius[h.sph_orig[sidx]] = h.sph_r[sidx];
  G2_CHECK(o.workspace_path == 0 || o.workspace_path == 1, GPMP2MI_ERR_INVALID, "workspace_path must be 0 or 1");
  if (o.workspace_path) {
    G2_CHECK(o.workspace_path_mode >= GPMP2MI_WORKSPACE_POSITION && o.workspace_path_mode <= GPMP2MI_WORKSPACE_POSE,
             GPMP2MI_ERR_INVALID, "workspace path: unknown mode");
    G2_CHECK(o.workspace_path_link >= 0 && o.workspace_path_link < h.nr_links, GPMP2MI_ERR_INVALID,
             "workspace path: link out of range");
    G2_DISPATCH_ROBOT_H(h, (void)0);   // a (kind, dof) the chain kernels are not instantiated for: GPMP2MI_ERR_UNSUPPORTED
    ex.wp_cap = 1;
    ex.wp_mode = o.workspace_path_mode;
    ex.wp_link = o.workspace_path_link;
  }
  return GPMP2MI_OK;
}

// Every device buffer of the plan, in the one order gpmp2mi_debug_forms::fail_alloc_at counts (plan_alloc calls), and
// the host-mapped pass flags
static int alloc_buffers(gpmp2mi_plan* p, const ExtrasHost& hx) {
  const PlanParams& P = p->hp;
  const PlanForms& F = p->forms;
  const RobotDev& h = p->robot->h;
  PlanBuffers& pb = p->pb;
  PlanExtras& ex = p->ex;
  const int B = P.B, D = P.D;
  const size_t tsz = p->tsz(), M = (size_t)B * (P.N + 1);
  std::memset(&pb, 0, sizeof(pb));
  G2_TRY(plan_alloc(p, &pb.params, 1));
  for (double** q : {&pb.start_conf, &pb.start_vel, &pb.end_conf, &pb.end_vel}) G2_TRY(plan_alloc(p, q, (size_t)B * D));
  for (double** q : {&pb.cur, &pb.last, &pb.trial, &pb.init, &pb.result, &pb.delta}) G2_TRY(plan_alloc(p, q, tsz));
  const size_t tq = F.wide ? 4 : 1;  // wide blocks: 2 x 2 tiles, 32-wide vectors
  G2_TRY(plan_alloc(p, &pb.gvec, (size_t)B * (P.N + 1) * (F.wide ? 32 : 16)));
  G2_TRY(plan_alloc(p, &pb.htiles, P.rules.opt_type == GPMP2MI_OPT_DOGLEG ? (size_t)B * (P.N + 1) * 512 * tq : 1));
  G2_TRY(plan_alloc(p, &pb.hgpart, (size_t)B * P.Npad));
  G2_TRY(plan_alloc(p, &pb.scal, (size_t)B * SC_COUNT));
  for (int** q : {&pb.which, &pb.stepped}) G2_TRY(plan_alloc(p, q, B));
  G2_TRY(plan_alloc(p, &pb.spart, (size_t)B * std::max((P.N + 4) / 4, P.Ppad / 64) * 3));
  G2_TRY(plan_alloc(p, &pb.xg, (size_t)B * (P.N + 1) * (F.wide ? 32 : 16)));
  if (F.dense) {   // dense normal equations + the factors of the dense cyclic reduction
    G2_TRY(plan_alloc(p, &pb.wHd, (size_t)B * (P.N + 1) * P.n * P.n));
    G2_TRY(plan_alloc(p, &pb.wHo, (size_t)B * P.N * P.n * P.n));
    G2_TRY(plan_alloc(p, &pb.wg, (size_t)B * (P.N + 1) * P.n));
    for (double** q : {&pb.wWl, &pb.wWr}) G2_TRY(plan_alloc(p, q, (size_t)B * (P.N + 1) * P.n * P.n));
    for (double** q : {&pb.wy, &pb.wrb, &pb.wx}) G2_TRY(plan_alloc(p, q, (size_t)B * (P.N + 1) * P.n));
  }
  G2_TRY(plan_alloc(p, &pb.xp_n, B));
  for (int** q : {&pb.xp_state, &pb.xp_has_vel}) G2_TRY(plan_alloc(p, q, (size_t)B * XP_MAX));
  G2_TRY(plan_alloc(p, &pb.xp_target, (size_t)B * XP_MAX * P.n));
  G2_TRY(plan_alloc(p, &pb.xp_info, (size_t)B * XP_MAX * 2 * D * D));
  G2_TRY(plan_alloc(p, &pb.goal_on, B));
  for (double** q : {&pb.rec, &pb.rec2}) G2_TRY(plan_alloc(p, q, (size_t)B * P.RECS * P.Ppad));
  for (double** q : {&pb.gpu, &pb.gpu2}) G2_TRY(plan_alloc(p, q, (size_t)B * P.GPS * P.Npad));
  G2_TRY(plan_alloc(p, &pb.tiles, (size_t)B * (P.N + 1) * 256 * tq));
  G2_TRY(plan_alloc(p, &pb.fac, (size_t)B * (P.N + 1) * 768 * tq));
  for (double** q : {&pb.pend, &pb.coup}) G2_TRY(plan_alloc(p, q, (size_t)B * crr_groups(P.N, 4) * 256));
  for (double** q : {&pb.cur_err, &pb.prev_err, &pb.last_err, &pb.final_err, &pb.lambda}) G2_TRY(plan_alloc(p, q, B));
  G2_TRY(plan_alloc(p, &pb.trace, (size_t)B * (P.rules.max_iter + 1)));
  for (int** q : {&pb.iters, &pb.status, &pb.active, &pb.phase, &pb.notspd}) G2_TRY(plan_alloc(p, q, B));
  G2_TRY(plan_alloc(p, &pb.epart, (size_t)B * P.Npad));
  G2_TRY(plan_alloc(p, &pb.cshare, (size_t)B * (P.Ppad / 64) * 3));
  if (ex.n_ws > 0) {
    G2_TRY(plan_alloc(p, &ex.des, hx.des.size()));
    G2_TRY(plan_alloc(p, &ex.poses, M * h.nr_links * 16));
    G2_TRY(plan_alloc(p, &ex.Jp, M * h.nr_links * 6 * D));
    G2_TRY(plan_alloc(p, &ex.ws_err, (size_t)ex.n_ws * M * 6));
    G2_TRY(plan_alloc(p, &ex.ws_H, (size_t)ex.n_ws * M * 6 * D));
  }
  if (ex.n_sc > 0) {
    G2_TRY(plan_alloc(p, &ex.sc_data, hx.scd.size()));
    G2_TRY(plan_alloc(p, &ex.radius, hx.radius.size()));
    G2_TRY(plan_alloc(p, &ex.cen, M * h.nr_spheres * 3));
    G2_TRY(plan_alloc(p, &ex.Jc, M * h.nr_spheres * 3 * D));
    G2_TRY(plan_alloc(p, &ex.sc_err, M * ex.n_sc));
    G2_TRY(plan_alloc(p, &ex.sc_H, M * ex.n_sc * D));
  }
  if (ex.mv_cap > 0) {   // the centres and their Jacobians are shared with the self-collision rows
    if (ex.n_sc == 0) {
      G2_TRY(plan_alloc(p, &ex.radius, hx.radius.size()));
      G2_TRY(plan_alloc(p, &ex.cen, M * h.nr_spheres * 3));
      G2_TRY(plan_alloc(p, &ex.Jc, M * h.nr_spheres * 3 * D));
    }
    G2_TRY(plan_alloc(p, &ex.mv_radius, (size_t)ex.mv_cap));
    G2_TRY(plan_alloc(p, &ex.mv_centers, (size_t)ex.mv_cap * (P.N + 1) * 3));
  }
  if (ex.sp_cap > 0) {   // the pair records; the centres and their Jacobians unless an extra above has them
    if (ex.n_sc == 0 && ex.mv_cap == 0) {
      G2_TRY(plan_alloc(p, &ex.cen, M * h.nr_spheres * 3));
      G2_TRY(plan_alloc(p, &ex.Jc, M * h.nr_spheres * 3 * D));
    }
    G2_TRY(plan_alloc(p, &ex.sp_rec, (size_t)ex.sp_cap));
  }
  if (ex.wp_cap > 0) {   // the path and the list of its constrained states; no poses, Jacobians or rows
    G2_TRY(plan_alloc(p, &ex.wp_des, (size_t)(P.N + 1) * 16));
    G2_TRY(plan_alloc(p, &ex.wp_sigma, (size_t)P.N + 1));
    G2_TRY(plan_alloc(p, &ex.wp_list, (size_t)P.N + 1));
    G2_TRY(plan_alloc(p, &ex.wp_count, 1));
  }
  if (ex.cr_cap > 0) {   // the set alone: no poses, Jacobians or rows
    G2_TRY(plan_alloc(p, &ex.cr_radius, (size_t)ex.cr_cap));
    G2_TRY(plan_alloc(p, &ex.cr_centers, (size_t)ex.cr_cap * 3));
  }
  G2_TRY(plan_alloc(p, &pb.n_active, p->n_active_len));
  G2_TRY(plan_alloc(p, &pb.stamps, (size_t)B * 128));   // rows 0..B-1: kernel phases, rows B..2B-1: one CR task per level
  G2_TRY(flags_acquire(p->n_active_len, &p->flagbuf));
  p->h_flags = p->flagbuf.host;
  pb.host_flags = p->flagbuf.dev;
  G2_TRY(plan_alloc(p, &pb.pass_word, p->n_active_len));
  return GPMP2MI_OK;
}

// what the kernels read and the host knows: the goal switches (all on), the extra-factor data, the parameters
static int upload_constants(gpmp2mi_plan* p, const ExtrasHost& hx) {
  const std::vector<int> ones(p->hp.B, 1);
  G2_HIP(hipMemcpy(p->pb.goal_on, ones.data(), ones.size() * sizeof(int), hipMemcpyHostToDevice));
  const PlanExtras& ex = p->ex;
  if (ex.n_ws > 0) G2_HIP(hipMemcpy(ex.des, hx.des.data(), hx.des.size() * sizeof(double), hipMemcpyHostToDevice));
  if (ex.n_sc > 0) {
    G2_HIP(hipMemcpy(ex.sc_data, hx.scd.data(), hx.scd.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (ex.n_sc > 0 || ex.mv_cap > 0)
    G2_HIP(hipMemcpy(ex.radius, hx.radius.data(), hx.radius.size() * sizeof(double), hipMemcpyHostToDevice));
  G2_HIP(hipMemcpy(p->pb.params, &p->hp, sizeof(p->hp), hipMemcpyHostToDevice));
  // the zero fills of the arena chunks ran on the null stream: done before the caller may use any other stream
  G2_HIP(hipStreamSynchronize(nullptr));
  p->null_stream_dirty = false;
  return GPMP2MI_OK;
}

extern "C" {

int gpmp2mi_plan_create(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, const gpmp2mi_settings* s,
                        const gpmp2mi_graph_opts* o, int B, gpmp2mi_plan** out) {
  return gpmp2mi_debug_plan_create(robot, sdf, s, o, B, nullptr, out);
}

int gpmp2mi_debug_plan_create(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, const gpmp2mi_settings* s,
                              const gpmp2mi_graph_opts* o_in, int B, const gpmp2mi_debug_forms* forms,
                              gpmp2mi_plan** out) {
  G2_CHECK(robot && sdf && s && out, GPMP2MI_ERR_INVALID, "null argument");
  *out = nullptr;
  gpmp2mi_graph_opts o;
  if (o_in) o = *o_in;
  else gpmp2mi_graph_opts_default(&o);
  const int D = robot->h.dof;
  G2_CHECK(B > 0, GPMP2MI_ERR_INVALID, "batch size must be positive");
  G2_CHECK(s->dof == D, GPMP2MI_ERR_INVALID, "[TrajOptimizerSetting] dof does not match the robot");
  G2_CHECK(s->total_step >= 1 && s->total_time > 0, GPMP2MI_ERR_INVALID, "bad total_step / total_time");
  G2_CHECK(s->obs_check_inter >= 0 && s->obs_check_inter <= MAXI, GPMP2MI_ERR_UNSUPPORTED, "obs_check_inter > 16");
  G2_CHECK(D <= MAXD, GPMP2MI_ERR_UNSUPPORTED, "plans are instantiated for dof <= 18");
  // the dense path (dof > 11) exists for the reference's PR2-class models only: normal-equation export and the dense
  // block solve are instantiated for dof 17 and 18 (plan_kernels.hip G2_EXP_CASE), so 12..16 would be created and then
  // fail inside optimize
  G2_CHECK(D <= 11 || D == 17 || D == 18, GPMP2MI_ERR_UNSUPPORTED,
           "plans are instantiated for dof <= 11 and for dof 17 / 18 (SE(2) base [+ lift] + two 7-joint arms)");
  PlanForms F;
  G2_TRY(choose_forms(robot->h, *s, B, forms, &F));
  {
    // the assembler stages an interval with at most NLD2 16-B loads per lane (assembler.h: 6, 9 on the wide path)
    const int nd = D * (D + 1) / 2 + D + 1 + ((robot->h.base_dof == 3 && s->obs_check_inter > 0) ? 36 : 0);
    const int gpr = 2 * D + 1 + (robot->h.base_dof == 3 ? 18 : 0);
    const int nds = (nd + 1) & ~1, gps = (gpr + 1) & ~1;
    G2_CHECK((s->obs_check_inter + 1) * nds + gps + 24 * s->obs_check_inter <= 2 * 64 * (D > 11 ? 14 : F.wide ? 9 : 6), GPMP2MI_ERR_UNSUPPORTED,
             "obs_check_inter too large for the staged assembly");
  }
  G2_CHECK(s->opt_type >= GPMP2MI_OPT_GAUSS_NEWTON && s->opt_type <= GPMP2MI_OPT_DOGLEG, GPMP2MI_ERR_INVALID,
           "unknown opt_type");
  G2_CHECK(s->cost_sigma > 0 && s->conf_prior_sigma > 0 && s->vel_prior_sigma > 0, GPMP2MI_ERR_INVALID,
           "sigmas must be positive");
  if (s->flag_vel_limit && s->vel_limits)
    for (int k = 0; k < D; k++)
      G2_CHECK(s->vel_limits[k] > 0, GPMP2MI_ERR_INVALID, "[VelocityLimitFactorVector] velocity limit <= 0");
  G2_TRY(ensure_device());

  auto p = std::make_unique<gpmp2mi_plan>();   // ~gpmp2mi_plan returns whatever has been allocated if anything below fails
  p->robot = robot;
  p->sdf = sdf;
  p->forms = F;
  p->fail_alloc_at = forms ? forms->fail_alloc_at : 0;
  G2_HIP(hipGetDevice(&p->device));
  G2_TRY(fill_params(robot->h, s, o, F, B, p->hp));
  p->n_active_len = p->hp.max_pass;
  p->Qc.assign((size_t)D * D, 0.0);
  for (int i = 0; i < D; i++) p->Qc[(size_t)i * D + i] = 1.0;
  if (s->Qc) std::copy(s->Qc, s->Qc + (size_t)D * D, p->Qc.begin());
  ExtrasHost hx;
  G2_TRY(check_extras(robot->h, o, p->hp.N, p->ex, hx));
  p->has_extras = p->ex.n_ws > 0 || p->ex.n_sc > 0 || p->ex.mv_cap > 0 || p->ex.wp_cap > 0 || p->ex.sp_cap > 0 ||
                  p->ex.cr_cap > 0;
  p->h_xp_n.assign(B, 0);
  p->goal_removed.assign(B, 0);
  G2_TRY(alloc_buffers(p.get(), hx));
  G2_TRY(upload_constants(p.get(), hx));
  *out = p.release();
  return GPMP2MI_OK;
}

// Waits only for what THIS plan still has in flight (streams it was given since their last synchronisation; nothing
// after the usual optimize -> get_result sequence), never for the device: other host threads' plans keep running.
// A poisoned plan (timed-out pass) is not waited for at all and its memory is not recycled.
void gpmp2mi_plan_destroy(gpmp2mi_plan* p) { delete p; }

// test hook: what the library currently holds (arena chunks / flag buffers owned by live plans, pooled ones, plans
// leaked because they were poisoned).  Works without a GPU (all zeros then).
int gpmp2mi_debug_resource_counts(long* live_chunks, long* pooled_chunks, long* live_flagbufs, long* pooled_flagbufs,
                                  long* leaked_plans) {
  std::lock_guard<std::mutex> lk(g_flag_mu);
  if (live_chunks) *live_chunks = g_live_chunks.load();
  if (pooled_chunks) *pooled_chunks = (long)g_chunk_pool.size();
  if (live_flagbufs) *live_flagbufs = g_live_flagbufs.load();
  if (pooled_flagbufs) *pooled_flagbufs = (long)g_flag_pool.size();
  if (leaked_plans) *leaked_plans = g_leaked_plans.load();
  return GPMP2MI_OK;
}

}  // extern "C"
