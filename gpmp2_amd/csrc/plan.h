// plan.h -- device-resident state of a batch of trajectory problems (gpmp2mi_plan) and the
// launchers of the fused hot-path kernels (linearize_kernels.hip, plan_kernels.hip, cr_kernels.hip, dense_kernels.hip).
#pragma once
#include <cstdint>

#include "common.h"
#include "step_control.h"

namespace g2 {

constexpr int MAXI = 16;   // max obs_check_inter
constexpr int TILE = 16;
constexpr int XP_MAX = GPMP2MI_MAX_STATE_PRIORS;  // extra per-state priors per trajectory (replanning)   // block-tridiagonal tile edge (n = 2*dof <= 16 in the MFMA solver)

// Uniform parameters of a plan; lives in HBM, read through scalar loads.
struct PlanParams {
  int B, N, I, P, Ppad, D, n, NG, REC, Npad, GPREC;
  int RECS, GPS;                       // record strides in HBM and LDS: REC / GPREC rounded up to even (16-B pieces)
  int max_pass;
  int obs_skip_first, flag_pos_limit, flag_vel_limit, lie;
  int lin_split;                       // 2: k_linearize splits the spheres of a point over 2 wavefronts (fixed-base arms)
  int end_conf_prior_off;              // 1: no PriorFactor on x_N (a goal / workspace factor stands in)
  int wide;                            // 2 dof > 15: blocks wider than one tile (2x2-tile kernels of wide_cr.h, or the dense path of dense_kernels.hip)
  int split_back;                      // GN: back-substitution levels 1, 2 and the retract run in k_finish_step
  int spart_groups;                    // shares per trajectory in pb.spart: workgroups of k_finish_trial(_wide) (finish_trial_group), or the chunks of
                                       // k_linearize_arm when it applies the trial step itself (fuse_finish)
  int wide_h0;                         // wide blocks: first forward level k_solve_step<WcrForm> runs itself (levels below: k_cr_level_wide)
  int fuse_finish;                     // GN fast path: levels 4, 2, 1 of the back-substitution and the retract run at the head of the
                                       // NEXT pass's k_linearize_arm (no k_finish_step); the state buffers cur / last swap roles every pass
  double eps, obs_w, delta_t;          // obs_w = 1 / cost_sigma^2
  double conf_prior_w, vel_prior_w;    // 1 / sigma^2
  double vdyn_w;                       // 1 / dynamics_sigma^2 or 0
  StepRules rules;                     // optimizer, iteration limits, thresholds (step_control.h)
  alignas(16) GpCoef coef[MAXI];
  // per sub-step, for the assembler (staged into LDS): [0..3] Psi_r Psi_c, [4..7] Lam_r Lam_c, [8..11] Lam_r Psi_c,
  // [12..15] Psi_r Lam_c at index ar * 2 + ac (a = 0 conf / 1 vel; Lam = (l11, l12), Psi = (p11, p12)); [16..19]
  // l11 l12 p11 p12; rest padding
  alignas(16) double coefq[MAXI][24];
  double Winv[4];                      // B(delta_t): 12/dt^3, -6/dt^2, -6/dt^2, 4/dt
  double Qc_inv[MAXD * MAXD];
  double pos_lo[MAXD], pos_hi[MAXD], pos_th[MAXD], pos_w[MAXD];
  double vel_lim[MAXD], vel_th[MAXD], vel_w[MAXD];
  // GP prior constant Hessian blocks (n x n row-major, ld = n): KA = Phi^T W Phi, KB = W,
  // KO = -Phi^T W (block (i, i+1))
  double KA[4 * MAXD * MAXD], KB[4 * MAXD * MAXD], KO[4 * MAXD * MAXD];
};

// What a workgroup of the three pass kernels (k_linearize_arm, k_assemble, k_gn_step_cr) needs before its first
// data-dependent load, passed BY VALUE in the kernel arguments: the sizes that turn a workgroup index into a trajectory
// and into addresses, the step rules and the form switches.  Read through `pp`, each of them is a dependent load (kernel
// arguments -> *pp -> the word) in front of everything else at the head of the kernel.  The launcher fills it from the
// host copy of PlanParams it is handed; everything else still comes from *pp.
struct PassConsts {
  int N, Ppad, P, I, RECS, GPS, Npad;
  int fuse_finish, split_back, lie;
  StepRules rules;
};
inline PassConsts pass_consts(const PlanParams& hp) {
  return PassConsts{hp.N, hp.Ppad, hp.P, hp.I, hp.RECS, hp.GPS, hp.Npad, hp.fuse_finish, hp.split_back, hp.lie, hp.rules};
}

// Extra factors a plan carries as data (gpmp2mi_graph_opts): workspace priors / goal factor and self collision on
// ranges of support states.  They are unary in x_i, so their J^T J / sigma^2, J^T r / sigma^2, r^T r / sigma^2 are
// added to the record of the state's unary evaluation point after k_linearize (launch_extra_factors); the solver
// kernels never see them separately.
// one row of a plan's self-collision table as k_selfpair_accumulate reads it, formed on the host when the table is set:
// sphere indices in the order of PlanExtras::cen / Jc (the caller's), radius_A + radius_B + epsilon, 1 / sigma^2.  24 bytes.
struct SelfPairRec {
  double total_eps, w;
  int a, b;
};

struct PlanExtras {
  int n_ws, n_sc, sc_first, sc_last;
  int ws_mode[GPMP2MI_MAX_WORKSPACE_FACTORS], ws_link[GPMP2MI_MAX_WORKSPACE_FACTORS];
  int ws_first[GPMP2MI_MAX_WORKSPACE_FACTORS], ws_last[GPMP2MI_MAX_WORKSPACE_FACTORS];
  double ws_w[GPMP2MI_MAX_WORKSPACE_FACTORS];                       // 1 / sigma^2
  double sc_w[GPMP2MI_MAX_SELF_COLLISION_PAIRS];                    // 1 / sigma^2
  // device workspace, M = B (N + 1) states
  double* des;       // [n_ws][16]
  double* sc_data;   // [n_sc][4]
  double* radius;    // [S] caller's sphere order
  double* poses;     // [M][L][16]
  double* Jp;        // [M][L][6][D]
  double* ws_err;    // [n_ws][M][6]
  double* ws_H;      // [n_ws][M][6][D]
  double* cen;       // [M][S][3]
  double* Jc;        // [M][S][3][D]
  double* sc_err;    // [M][n_sc]
  double* sc_H;      // [M][n_sc][D]
  // moving spheres (include/gpmp2mi.h "moving obstacles"): the capacity, the factor's constants and the resident set.
  // mv_K is the set's current size, a host value that every launch takes as an argument (moving_kernels.hip)
  int mv_cap, mv_K, mv_first, mv_last;
  double mv_eps, mv_w;   // epsilon, 1 / sigma^2
  double* mv_radius;     // [mv_cap]
  double* mv_centers;    // [mv_cap][N+1][3], the first mv_K spheres in use
  // workspace path (include/gpmp2mi.h "workspace path"): the capacity, the factor's constants and the resident path.
  // wp_n is a host value: the entries of wp_list a launch looks at, one wavefront each per trajectory -- the number of
  // constrained states after the host setter, N + 1 after the _dev setter (the count is then known to the device
  // only), 0 for no path (path_kernels.hip)
  int wp_cap, wp_mode, wp_link, wp_n;
  double* wp_des;        // [N+1][16]
  double* wp_sigma;      // [N+1], +inf: the state carries no factor
  int* wp_list;          // [N+1] the constrained states, ascending
  int* wp_count;         // [1] how many
  // self-collision table (include/gpmp2mi.h "self-collision table in a plan"): the capacity, the range and the resident
  // records.  sp_P is the table's current size, a host value that every launch takes as an argument
  // (selfpair_kernels.hip)
  int sp_cap, sp_P, sp_first, sp_last;
  SelfPairRec* sp_rec;   // [sp_cap], the first sp_P rows in use
  // carried object (include/gpmp2mi.h "carried object"): the capacity, the range, the factor's constants and the resident
  // set.  cr_A and cr_link are host values that every launch takes as arguments (carried_kernels.hip)
  int cr_cap, cr_A, cr_link, cr_first, cr_last;
  double cr_eps, cr_w;   // epsilon, 1 / sigma^2
  double* cr_radius;     // [cr_cap]
  double* cr_centers;    // [cr_cap][3] in the frame of link cr_link, the first cr_A spheres in use
};

// Per-plan device buffers.
struct PlanBuffers {
  PlanParams* params;      // device copy
  double* start_conf;      // [B][D]
  double* start_vel;
  double* end_conf;
  double* end_vel;
  double* cur;             // [B][N+1][2D]  opt->values()
  double* last;            // [B][N+1][2D]  last_values
  double* trial;           // [B][N+1][2D]  LM / Dogleg trial point
  double* init;            // [B][N+1][2D]  pristine initial values (optimize() can be re-run)
  double* result;          // [B][N+1][2D]
  double* rec;             // [B][Ppad][RECS] point-major records: G (packed upper), g, e [, M1..M4]   (buffer 0)
  double* rec2;            // second buffer for trial linearizations (LM / Dogleg)
  double* gpu;             // [B][Npad][GPS] per interval end state: GP prior u = W r (n), r^T W r [, J1, J3]
  double* gpu2;
  double* tiles;           // [B][N+1][256] diagonal tile S_i = [D_i | -g_i] of every even block (updated in place)
  double* fac;             // [B][N+1][3][256] factor tiles Wl, Wr (both carry y), V = R^-T
  double* pend;            // [B][crr_groups(N, 4)][256] what tree block v = 4q+4 still owes to blocks 4q+2, 4q+3 (k_assemble -> cr_forward)
  double* coup;            // [B][crr_groups(N, 4)][256] level-4 coupling between tree blocks 4q and 4q+4, q >= 1 (k_assemble -> cr_forward)
  double* delta;           // [B][N+1][2D]
  double* gvec;            // [B][N+1][16] gradient g_i = J^T Sigma^-1 r of the current linearization
  double* htiles;          // [B][N+1][2][256] un-eliminated D_i and H_{i,i+1} (Dogleg: g^T H g)
  double* hgpart;          // [B][Npad] per-block share of g^T H g
  double* scal;            // [B][16] per-trajectory scalars of the current trial step (see SC_*)
  // extra priors (gpmp2mi_plan_fix_state / add_state_estimate) and goal switch (remove_goal)
  int* xp_n;               // [B] number of extra priors
  int* xp_state;           // [B][XP_MAX] state index
  int* xp_has_vel;         // [B][XP_MAX] 1 if the entry also constrains the velocity
  double* xp_target;       // [B][XP_MAX][2D] conf, vel
  double* xp_info;         // [B][XP_MAX][2][D*D] information matrices (conf, vel)
  int* goal_on;            // [B] 0 after removeGoalConfigAndVel
  // dense block-tridiagonal system and its factors (wide path only; n = 2 dof)
  double* wHd;             // [B][N+1][n][n]   diagonal blocks, then their upper Cholesky factors R_i
  double* wHo;             // [B][N][n][n]     block (i+1, i) (read only)
  double* wg;              // [B][N+1][n]      gradient (read only)
  double* wWl;             // [B][N+1][n][n]   dense cyclic reduction: W_l = R^-T C_l of every eliminated block
  double* wWr;             // [B][N+1][n][n]   ... W_r
  double* wy;              // [B][N+1][n]      ... y = R^-T b
  double* wrb;             // [B][N+1][n]      ... running right-hand side of the blocks still in the tree
  double* wx;              // [B][N+1][n]      ... solution
  double* xg;              // [B][N+1][16 or 32] step of the blocks the solve kernel back-substitutes itself (split path)
  int* stepped;            // [B] pass + 1 of the last pass in which the trajectory took a step (split path); trial-step
                           // path: 1 when k_solve_step left a factorisation for k_finish_trial
  double* spart;           // [B][ceil((N+1)/4)][3] per-group shares of g.delta, |delta|^2, |g|^2 (k_finish_trial)
  int* which;              // [B] record buffer (0: rec/gpu, 1: rec2/gpu2) holding the linearization at `cur`
  // per-trajectory scalars
  double* cur_err;         // error at `cur`
  double* prev_err;        // currentError of gpmp2::optimize
  double* last_err;
  double* final_err;
  double* lambda;          // LM lambda / Dogleg delta
  double* trace;           // [B][max_iter+1]
  int* iters;
  int* status;
  int* active;             // 1 while the trajectory is still iterating
  int* phase;              // Dogleg: 1 while the trial point is a retry from the same linearization (dogleg_retry);
                           // LM: its count of calls to iterate(), the index into `trace`
  int* notspd;             // [B] set when a level-1 pivot (k_assemble) was not positive
  double* epart;           // [B][Npad] per-block share of the graph error (k_assemble, or k_error_parts: the whole sum in block
                           // 0); not written when the step control reads cshare instead (early stop)
  double* cshare;          // [B][Ppad/64][3] per-chunk share of the graph error at `cur`: obstacle, GP prior, priors / limits
                           // (k_linearize_arm, buffer 0 only; summed by error_from_shares)
  int* n_active;           // [max_pass] trajectories that iterated in each pass
  unsigned long long* pass_word;  // [max_pass] arrivals of the pass-closing kernel's workgroups and their count (pass_counter.h)
  int* host_flags;         // [max_pass] pinned, device-mapped: n_active[pass] once the pass is complete, else -1
  unsigned long long* stamps;  // [B][64] s_memtime stamps (diagnostic builds only)
};

// A queue run (gpmp2mi_plan_optimize_queue): M problems through the plan's B slots.  At each pass boundary
// k_queue_scan ranks the slots whose problem finished, in slot order, and hands them the next problems;
// k_queue_refill writes the finished problems' results to their output rows and loads the new ones.  Inputs and
// outputs are rows of problem j; the per-slot words live in a workspace of the plan.
struct QueueRun {
  int M;
  int budget;                // trial-step path: iterative passes a problem may take (plain run: n_active_len - 2); 0: none
  const double* start_conf;  // [M][D]
  const double* start_vel;
  const double* end_conf;
  const double* end_vel;
  const double* init;        // [M][N+1][2D]
  double* traj;              // [M][N+1][2D]  outputs; any may be null
  int* iters;                // [M]
  double* final_err;         // [M]
  int* status;               // [M]
  double* trace;             // [M][max_iter+1]
  int* job;                  // [B] problem the slot holds, -1: none
  int* next;                 // [B] problem the scan hands the slot at this boundary, -1: none
  int* act;                  // [B] 1: the problem finished, harvest it; 2: its pass budget is spent (k_finalize_unfinished)
  int* fresh;                // [B] 1: loaded at the last boundary, its first evaluation is still to come
  int* qpass;                // [B] iterative passes of the slot's problem so far (budget)
  int* head;                 // [1] next problem to load
  long long* busy;           // [1] sum over passes of the slots that held a problem
  int* flags;                // [passes] host-mapped: after each pass's scan, the active slots + problems not loaded yet
};

// scalars of a trial step (PlanBuffers::scal)
enum { SC_GD = 0, SC_DD, SC_GG, SC_GHG, SC_GN, SC_NN, SC_Q, SC_XNORM, SC_ZERO_STEP, SC_COUNT = 16 };

// record buffers of trajectory b: sel = 0 -> the linearization at `cur`, 1 -> the other one
__host__ __device__ inline double* rec_of(const PlanBuffers& pb, int which_b, int sel) {
  return (which_b ^ sel) ? pb.rec2 : pb.rec;
}
__host__ __device__ inline double* gpu_of(const PlanBuffers& pb, int which_b, int sel) {
  return (which_b ^ sel) ? pb.gpu2 : pb.gpu;
}

int launch_linearize(const RobotDev& hrobot, const RobotDev* robot, const SdfDev& sdf,
                     const PlanParams& hp, const PlanBuffers& pb, const double* traj, int bufsel,
                     const int* active, hipStream_t st, double* dst = nullptr, int pass = 0, bool trial = false);
int launch_extra_accumulate(const PlanParams& hp, const PlanBuffers& pb, const PlanExtras& ex, int L, int S, int bufsel,
                            const int* active, hipStream_t st);
// moving_kernels.hip: the moving-sphere factor of the states ex.mv_first..mv_last, from ex.cen / ex.Jc and the resident
// set (ex.mv_K > 0), straight into the unary records
int launch_moving_accumulate(const PlanParams& hp, const PlanBuffers& pb, const PlanExtras& ex, int S, int bufsel,
                             const int* active, hipStream_t st);
// selfpair_kernels.hip: the self-collision factor of the states ex.sp_first..sp_last, from ex.cen / ex.Jc and the
// resident table (ex.sp_P > 0), straight into the unary records
int launch_selfpair_accumulate(const PlanParams& hp, const PlanBuffers& pb, const PlanExtras& ex, int S, int bufsel,
                               const int* active, hipStream_t st);
// path_kernels.hip: the workspace-path factor of the constrained states of the resident path (ex.wp_n > 0), from the
// states in `traj` straight into the unary records
int launch_path_accumulate(const RobotDev& h, const RobotDev* R, const PlanParams& hp, const PlanBuffers& pb,
                           const PlanExtras& ex, const double* traj, int bufsel, const int* active, hipStream_t st);
// carried_kernels.hip: the carried-object factor of the states ex.cr_first..cr_last, from the states in `traj`, the field
// and the resident set (ex.cr_A > 0), straight into the unary records
int launch_carried_accumulate(const RobotDev& h, const RobotDev* R, const SdfDev& s, const PlanParams& hp,
                              const PlanBuffers& pb, const PlanExtras& ex, const double* traj, int bufsel,
                              const int* active, hipStream_t st);
int launch_set_mode(const PlanBuffers& pb, int opt_type, int fixed_iters, hipStream_t st);
int launch_error_parts(const PlanParams& hp, const PlanBuffers& pb, const double* traj, int bufsel, const int* active,
                       hipStream_t st);
int launch_plan_reset(const PlanParams& hp, const PlanBuffers& pb, const double* start, hipStream_t st);
// early_stop (Gauss-Newton fast driver, shares in pb.cshare): the step control runs at the head of k_assemble and of
// k_gn_step_cr; a trajectory that stops builds nothing
int launch_assemble(const PlanParams& hp, const PlanBuffers& pb, const double* traj, int bufsel,
                    const int* active, hipStream_t st, bool early_stop = false);
int launch_solve_step(const PlanParams& hp, const PlanBuffers& pb, hipStream_t st);
int launch_ghg(const PlanParams& hp, const PlanBuffers& pb, hipStream_t st);
int launch_decide(const PlanParams& hp, const PlanBuffers& pb, int pass, bool init, hipStream_t st);
int launch_finalize_unfinished(const PlanParams& hp, const PlanBuffers& pb, hipStream_t st);
// queue runs (plan_kernels.hip)
int launch_queue_reset(const PlanParams& hp, const PlanBuffers& pb, const QueueRun& q, hipStream_t st);
int launch_queue_first(const PlanParams& hp, const PlanBuffers& pb, const QueueRun& q, int pass, hipStream_t st);
int launch_queue_scan(const PlanParams& hp, const PlanBuffers& pb, const QueueRun& q, int pass, bool load, hipStream_t st);
int launch_queue_refill(const PlanParams& hp, const PlanBuffers& pb, const QueueRun& q, double* states, hipStream_t st);
int launch_debug_crosslane(const double* in, double* out, hipStream_t st);
int launch_gn_step_cr(const PlanParams& hp, const PlanBuffers& pb, int pass, hipStream_t st, bool early_stop = false);
int launch_finish_step(const PlanParams& hp, const PlanBuffers& pb, int pass, hipStream_t st);
int launch_finish_trial(const PlanParams& hp, const PlanBuffers& pb, hipStream_t st);
int launch_solve_dense(const PlanParams& hp, const PlanBuffers& pb, hipStream_t st);
// wide_cr.h (8 <= dof <= 11 on 2x2 tiles)
int launch_assemble_wide(const PlanParams& hp, const PlanBuffers& pb, const double* traj, int bufsel,
                         const int* active, hipStream_t st);
int launch_ghg_wide(const PlanParams& hp, const PlanBuffers& pb, hipStream_t st);
int launch_solve_step_wide(const PlanParams& hp, const PlanBuffers& pb, hipStream_t st);
int launch_finish_trial_wide(const PlanParams& hp, const PlanBuffers& pb, hipStream_t st);
int launch_cr_level_wide(const PlanParams& hp, const PlanBuffers& pb, int h, hipStream_t st);
int launch_error_reduce(const PlanParams& hp, const PlanBuffers& pb, const double* traj, int bufsel,
                        double* err, hipStream_t st);
int launch_export_normal_eq(const PlanParams& hp, const PlanBuffers& pb, const double* traj, int bufsel,
                            double* Hdiag, double* Hoff, double* g, hipStream_t st, const int* active = nullptr);
int launch_block_tridiag_solve(int B, int nblk, int n, const double* Hd, const double* Ho,
                               const double* b, double* x, int* ok, double* scratch, hipStream_t st);
// posterior_kernels.hip: Sigma = H^-1 on the band and samples delta = L^-T z of B block-tridiagonal systems (layouts of
// launch_block_tridiag_solve).  Sd / So null: no marginals; K = 0: no samples; ok may be null.
struct PosteriorArgs {
  int nblk, K;
  const double *Hd, *Ho;   // [B][nblk][n][n], [B][nblk-1][n][n] block (i+1, i)
  const double* z;         // [B][K][nblk][n]
  double *Sd, *So;         // as Hd, Ho
  double* delta;           // as z
  int* ok;                 // [B]
  double* fac;             // [B][nblk][512] factor scratch
};
int launch_posterior(int B, int n, const PosteriorArgs& a, hipStream_t st);
// seed_kernels.hip: normals of rng.h, and samples whose z is made in registers (include/gpmp2mi.h "seeding")
struct NormalFillArgs {
  uint64_t seed;
  uint32_t stream;
  int a_first, a_count, b_first, b_count, nblk, n;
  double* out;             // [a_count][b_count][nblk][n]
};
int launch_normal_fill(const NormalFillArgs& a, hipStream_t st);
struct SeedSampleArgs {
  uint64_t seed;
  uint32_t stream;
  int nblk, count;         // blocks of a system; columns (restarts, or samples per system)
  int a_first, b_first;    // shared: column s is problem (a_first + s, 0); else sample (a_first + system, b_first + s)
  const double* fac;       // [1 or systems][nblk][512] factor scratch of a factor-only launch_posterior
  double* out;             // shared: [count][nblk][n] = mean + scale delta; else [systems][count][nblk][n] = delta
  // restarts (shared) only
  double scale;
  int keep_first, D;       // keep_first: problem 0 gets delta = 0; n = 2 D
  const double* mean;      // [count][nblk][n], or null: the straight line from start_conf to end_conf
  const double *start_conf, *end_conf;   // [count][D], read when mean is null
};
int launch_sample_seeded(int systems, int n, bool shared, const SeedSampleArgs& a, hipStream_t st);

}  // namespace g2
