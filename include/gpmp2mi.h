/*
 * gpmp2mi.h -- C ABI of the MI355X-native GPMP2 linearize-and-solve engine.
 *
 * This header is the drop-in boundary.  Every entry point is plain C:
 * opaque handles, POD structs, caller-owned flat `double` buffers, `int` status returns, no
 * exceptions, no torch / gtsam / Eigen types.  Each declaration cites the reference interface
 * (path:line relative to the ori-drs/gpmp2 tree) it replaces.
 *
 * Conventions
 *   D  = robot dof, N = total_step (N+1 support states), I = obs_check_inter, S = #body spheres,
 *   B  = number of independent trajectories in a batch.
 *   A trajectory is a flat [N+1][2*D] array, state i = [x_i (D) ; v_i (D)]
 *   (cf. the flat layout precedent gpmp2/utils/OpenRAVEutils.cpp:35-39; keys Symbol('x',i),
 *   Symbol('v',i) of gpmp2/planner/BatchTrajOptimizer.h:39-41 map to row i).
 *   For Pose2-based robots x_i = [x, y, theta, q_arm...] (gpmp2/geometry/Pose2Vector.h:26-73).
 *   All matrices are row-major unless stated otherwise.  Everything is IEEE fp64.
 *
 * Memory spaces: entry points ending in `_dev` take HIP device pointers and a hipStream_t passed
 * as `void*`; all others take host pointers and synchronise before returning.
 *
 * The library has NO CPU fallback: every compute entry point runs hand-written gfx950 HIP
 * kernels and returns GPMP2MI_ERR_NO_DEVICE when no GPU is usable.
 */
#ifndef GPMP2MI_H
#define GPMP2MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPMP2MI_VERSION 100
#define GPMP2MI_MAX_DOF 18      /* largest total dof a plan is instantiated for (csrc/common.h MAXD): the PR2 model */
#define GPMP2MI_MAX_SPHERES 96  /* largest sphere model staged on chip (PR2: 65) */

/* ---- status codes (replace the C++ exceptions of SURVEY.md section 8b "Error convention") --- */
enum {
  GPMP2MI_OK = 0,
  GPMP2MI_ERR_INVALID = 1,      /* bad argument: null pointer, dof/dimension mismatch
                                   (std::runtime_error in kinematics/JointLimitFactorVector.h:52-56,
                                    kinematics/VelocityLimitFactorVector.h:51-56) */
  GPMP2MI_ERR_NO_DEVICE = 2,    /* no usable HIP device / kernel image */
  GPMP2MI_ERR_HIP = 3,          /* a HIP runtime call failed (see gpmp2mi_last_error) */
  GPMP2MI_ERR_UNSUPPORTED = 4,  /* combination not instantiated (dof > GPMP2MI_MAX_DOF, ...) */
  GPMP2MI_ERR_ALLOC = 5,
  GPMP2MI_ERR_TIMEOUT = 6       /* a pass did not finish within GPMP2MI_WAIT_TIMEOUT_MS (default 5 s): the plan is
                                   POISONED -- every later call on it returns this code, gpmp2mi_plan_destroy neither
                                   waits for its stream nor recycles its memory (it is leaked on purpose: a hung kernel
                                   would hang the wait, a late one would write into recycled memory) */
};

/* per-trajectory status written by the optimizers */
enum {
  GPMP2MI_TRAJ_CONVERGED = 0,      /* gtsam::checkConvergence fired */
  GPMP2MI_TRAJ_MAX_ITER = 1,       /* stopped by max_iter */
  GPMP2MI_TRAJ_ROLLED_BACK = 2,    /* final step increased the error; previous values returned
                                      (planner/BatchTrajOptimizer.cpp:297-307) */
  GPMP2MI_TRAJ_NOT_SPD = 3,        /* a Cholesky pivot was <= 0 or NaN
                                      (gtsam::IndeterminantLinearSystemException) */
  GPMP2MI_TRAJ_ALREADY_OPTIMAL = 4 /* initial error <= errorTol (BatchTrajOptimizer.cpp:250-255) */
};

/* ---- robots: gpmp2/kinematics ----------------------------------------------------------- */
enum {
  GPMP2MI_ROBOT_ARM = 0,               /* gpmp2::ArmModel          kinematics/Arm.h:27-146 */
  GPMP2MI_ROBOT_POINT = 1,             /* gpmp2::PointRobotModel   kinematics/PointRobot.cpp:15-49 */
  GPMP2MI_ROBOT_POSE2_MOBILE_BASE = 2, /* gpmp2::Pose2MobileBaseModel kinematics/Pose2MobileBase.cpp:20-55 */
  GPMP2MI_ROBOT_POSE2_MOBILE_ARM = 3,  /* gpmp2::Pose2MobileArmModel  kinematics/Pose2MobileArm.cpp:30-108 */
  GPMP2MI_ROBOT_POSE2_MOBILE_2ARMS = 4,        /* gpmp2::Pose2Mobile2ArmsModel kinematics/Pose2Mobile2Arms.cpp:32-108 */
  GPMP2MI_ROBOT_POSE2_MOBILE_VETLIN_ARM = 5,   /* gpmp2::Pose2MobileVetLinArmModel kinematics/Pose2MobileVetLinArm.cpp:31-108 */
  GPMP2MI_ROBOT_POSE2_MOBILE_VETLIN_2ARMS = 6  /* gpmp2::Pose2MobileVetLin2ArmsModel kinematics/Pose2MobileVetLin2Arms.cpp:36-114 */
};

/* POD description of RobotModel<FK> = FK + BodySphereVector (kinematics/RobotModel.h:20-90). */
typedef struct gpmp2mi_robot_desc {
  int kind;                   /* GPMP2MI_ROBOT_* */
  int dof;                    /* total dof (POINT: 2; MOBILE_BASE: 3; MOBILE_ARM / 2ARMS: 3 + arm_dof;
                                 VETLIN_*: 4 + arm_dof, state [x, y, theta, lift, q...]) */
  int arm_dof;                /* number of DH joints, both arms together (0 for POINT / MOBILE_BASE);
                                 the DH arrays list arm 1 first, then arm 2 */
  const double* a;            /* [arm_dof] DH a        (Arm ctor, kinematics/Arm.cpp:15-28) */
  const double* alpha;        /* [arm_dof] DH alpha */
  const double* d;            /* [arm_dof] DH d */
  const double* theta_bias;   /* [arm_dof] or NULL (= 0) */
  double base_pose[16];       /* row-major 4x4.  ARM: pose of the arm base in the world.
                                 MOBILE_ARM: base_T_arm (Pose2MobileArm ctor).  Others: ignored. */
  int nr_spheres;             /* S */
  const int* sphere_link;     /* [S] link id (BodySphere::link_id) */
  const double* sphere_radius;/* [S] */
  const double* sphere_center;/* [S][3] centre in the link frame */
  /* two-arm / vertical-lift robots (zero / identity otherwise).  Link order: vehicle base,
   * [torso], arm-1 links, arm-2 links. */
  int arm2_dof;               /* DH joints of the second arm (the last arm2_dof of arm_dof) */
  double base_pose2[16];      /* 2ARMS: base_T_arm2 (base_pose = base_T_arm1).
                                 VETLIN_ARM: torso_T_arm (base_pose = base_T_torso).
                                 VETLIN_2ARMS: torso_T_arm1 (base_pose = base_T_torso) */
  double base_pose3[16];      /* VETLIN_2ARMS: torso_T_arm2 */
  int reverse_linact;         /* VETLIN_*: lift moves the torso down (liftBasePose3, mobileBaseUtils.cpp:51-82) */
} gpmp2mi_robot_desc;

typedef struct gpmp2mi_robot gpmp2mi_robot;
int gpmp2mi_robot_create(const gpmp2mi_robot_desc* desc, gpmp2mi_robot** out);
void gpmp2mi_robot_destroy(gpmp2mi_robot* r);
int gpmp2mi_robot_dof(const gpmp2mi_robot* r);
int gpmp2mi_robot_nr_links(const gpmp2mi_robot* r);
int gpmp2mi_robot_nr_spheres(const gpmp2mi_robot* r);

/* ---- signed distance fields: gpmp2/obstacle ---------------------------------------------- */
enum {
  GPMP2MI_SDF_LAYOUT_ZYX = 0,   /* voxels[(z*ny + y)*nx + x]  (x = column index fastest)        */
  GPMP2MI_SDF_LAYOUT_GTSAM = 1  /* voxels[(z*nx + x)*ny + y]  = std::vector<Matrix> with column-
                                   major Eigen slices, data_[z](row=y, col=x)
                                   (obstacle/SignedDistanceField.h:50,170-172)                   */
};
/* 3-D: gpmp2::SignedDistanceField(origin, cell_size, data) obstacle/SignedDistanceField.h:57-60.
 * 2-D: gpmp2::PlanarSDF(origin, cell_size, data)           obstacle/PlanarSDF.h:44-46 (nz = 1).
 * nx = field_cols_, ny = field_rows_, nz = field_z_.  The voxels are copied to the device and
 * re-laid-out there; the caller's buffer may be freed after the call returns. */
typedef struct gpmp2mi_sdf gpmp2mi_sdf;
int gpmp2mi_sdf_create(int dim, const double origin[3], double cell_size, int nx, int ny, int nz,
                       const double* voxels, int layout, gpmp2mi_sdf** out);
void gpmp2mi_sdf_destroy(gpmp2mi_sdf* s);

/* Signed distance field from an occupancy grid, on the device
 * (matlab/+gpmp2/signedDistanceField3D.m:16-34, signedDistanceField2D.m:16-34,
 * gpmp2_python/utils/signedDistanceField3D.py:22-42): cells with occ > 0.75 are obstacles;
 * field = (EDT to the obstacle set - EDT to the free set) * cell_size with exact Euclidean
 * distances; a grid without obstacles (or without free space) gives the constant 1000.
 * occ, field: host [nz][ny][nx] (nz ignored when dim = 2). */
int gpmp2mi_sdf_field_from_occupancy(int dim, int nx, int ny, int nz, const double* occ,
                                     double cell_size, double* field);
/* same, straight into a field handle (no host round trip of the field); occ in `layout` */
int gpmp2mi_sdf_create_from_occupancy(int dim, const double origin[3], double cell_size, int nx,
                                      int ny, int nz, const double* occ, int layout,
                                      gpmp2mi_sdf** out);
/* geometry and voxel data ([nz][ny][nx]) of a handle; any output pointer may be NULL */
int gpmp2mi_sdf_get_field(const gpmp2mi_sdf* s, int* dim, int* nx, int* ny, int* nz,
                          double origin[3], double* cell_size, double* field);
/* gpmp2::readSDFvolfile gpmp2/utils/fileUtils.cpp:17-62: "<pre>.vol.head" (cols rows z, origin
 * xyz, resolution) + "<pre>.vol.data" (text, x outermost, then y, then z) */
int gpmp2mi_sdf_read_vol(const char* filename_pre, gpmp2mi_sdf** out);

/* SignedDistanceField::getSignedDistance(point, g) obstacle/SignedDistanceField.h:93-99 and
 * PlanarSDF::getSignedDistance obstacle/PlanarSDF.h:61-68, batched over M points.
 * points [M][dim]; dist [M]; grad [M][dim] or NULL; in_range [M] or NULL
 * (0 where the reference throws SDFQueryOutOfRange; dist/grad are then 0). */
int gpmp2mi_sdf_query(const gpmp2mi_sdf* s, int M, const double* points, double* dist,
                      double* grad, int* in_range);

/* ---- settings: POD mirror of gpmp2::TrajOptimizerSetting planner/TrajOptimizerSetting.h:17-100 */
enum { GPMP2MI_OPT_GAUSS_NEWTON = 0, GPMP2MI_OPT_LM = 1, GPMP2MI_OPT_DOGLEG = 2 };

typedef struct gpmp2mi_settings {
  int dof;
  int total_step;                  /* N */
  double total_time;
  double conf_prior_sigma;         /* conf_prior_model = Isotropic::Sigma(dof, .) */
  double vel_prior_sigma;          /* vel_prior_model */
  int flag_pos_limit;
  int flag_vel_limit;
  const double* joint_pos_limits_up;   /* [dof] (Pose2 robots: first 3 entries ignored, see
                                          kinematics/JointLimitFactorPose2Vector.h:66-91) */
  const double* joint_pos_limits_down; /* [dof] */
  const double* vel_limits;            /* [dof] */
  const double* pos_limit_thresh;      /* [dof] */
  const double* vel_limit_thresh;      /* [dof] */
  const double* pos_limit_sigmas;      /* [dof] pos_limit_model = Diagonal::Sigmas */
  const double* vel_limit_sigmas;      /* [dof] */
  double epsilon;
  double cost_sigma;
  int obs_check_inter;             /* I */
  const double* Qc;                /* [dof][dof] covariance of Qc_model; NULL = identity */
  int opt_type;                    /* GPMP2MI_OPT_* */
  int verbosity;                   /* 0 = None, 1 = Error (per-iteration errors to stdout) */
  int final_iter_no_increase;
  double rel_thresh;
  int max_iter;
} gpmp2mi_settings;

/* Fill with the defaults of TrajOptimizerSetting(size_t) planner/TrajOptimizerSetting.cpp:32-56
 * (pointer members are left NULL: limits default to +-1e6 / thresh 1e-3 / sigma 1e-3, Qc = I). */
void gpmp2mi_settings_default(gpmp2mi_settings* s, int dof);

/* Knobs that are NOT in TrajOptimizerSetting but differ between BatchTrajOptimize and the
 * hand-built graphs of the example scripts or are hard-coded GTSAM
 * parameters in gpmp2::optimize (planner/BatchTrajOptimizer.cpp:219-234). */
#define GPMP2MI_WORKSPACE_POSITION 0
#define GPMP2MI_WORKSPACE_ORIENTATION 1
#define GPMP2MI_WORKSPACE_POSE 2
#define GPMP2MI_MAX_WORKSPACE_FACTORS 4
#define GPMP2MI_MAX_SELF_COLLISION_PAIRS 16
#define GPMP2MI_MAX_MOVING_SPHERES 64
#define GPMP2MI_MAX_CARRIED_SPHERES 256
/* all pairs of the largest sphere model: the largest table a plan takes ("self-collision table in a plan" below) */
#define GPMP2MI_MAX_PLAN_SELF_PAIRS (GPMP2MI_MAX_SPHERES * (GPMP2MI_MAX_SPHERES - 1) / 2)
/* A workspace factor carried by a plan: GaussianPriorWorkspace{Position,Orientation,Pose}<Arm>
 * (kinematics/GaussianPriorWorkspacePosition.h:52-67, ...Orientation.h:52-69, ...Pose.h:53-70) or GoalFactorArm
 * (kinematics/GoalFactorArm.h:58-77 = POSITION on the last link) on the support states first_state..last_state,
 * isotropic noise `sigma`, as the hand-built graphs of matlab/Arm3GoalReachExample.m:95-110 and
 * matlab/WAMWorkspaceConstraintsExample.m:85-105 add them. */
typedef struct gpmp2mi_workspace_factor {
  int mode;                     /* GPMP2MI_WORKSPACE_POSITION / _ORIENTATION / _POSE */
  int link;                     /* link index of the FK model (GoalFactorArm: arm dof - 1) */
  int first_state, last_state;  /* inclusive range of support states */
  double sigma;
  double des_pose[16];          /* row-major 4x4 (POSITION uses the translation, ORIENTATION the rotation) */
} gpmp2mi_workspace_factor;

typedef struct gpmp2mi_graph_opts {
  int obs_skip_first_state;      /* 1: unary obstacle factors only for i>0
                                    (matlab/WAMFactorGraphExample.m:126-138); default 0 */
  double vehicle_dynamics_sigma; /* >0: add VehicleDynamicsFactorPose2Vector on every state
                                    (matlab/MobileArm2FactorGraphExample.m:122-126); default 0 */
  double lm_lambda_initial;      /* default 100 (BatchTrajOptimizer.cpp:226) */
  double lm_lambda_factor;       /* default 10   (gtsam LevenbergMarquardtParams) */
  double lm_lambda_upper;        /* default 1e5 */
  double lm_lambda_lower;        /* default 0 */
  double lm_min_model_fidelity;  /* default 1e-3 */
  double dogleg_delta_initial;   /* default 0.2 (BatchTrajOptimizer.cpp:222) */
  double abs_error_tol;          /* default 1e-5 (gtsam NonlinearOptimizerParams) */
  double error_tol;              /* default 0 */
  int fixed_iterations;          /* >0: run exactly this many iterations, no convergence test
                                    (receding-horizon budget, BASELINE config 4); default 0 */
  /* ---- extra factors of hand-built graphs, as data (gpmp2::optimize takes any NonlinearFactorGraph,
   * planner/BatchTrajOptimizer.h:206-208); all default to none */
  int end_conf_prior_off;        /* 1: no PriorFactor on x_N (a goal / workspace factor takes its place,
                                    matlab/Arm3GoalReachExample.m:107); the prior on v_N stays */
  int n_workspace;               /* <= GPMP2MI_MAX_WORKSPACE_FACTORS */
  gpmp2mi_workspace_factor workspace[GPMP2MI_MAX_WORKSPACE_FACTORS];
  int n_self_collision;          /* SelfCollision<Arm> (obstacle/SelfCollision.h:66-128) on the support states
                                    self_collision_first..last; <= GPMP2MI_MAX_SELF_COLLISION_PAIRS rows */
  int self_collision_first, self_collision_last;
  double self_collision[GPMP2MI_MAX_SELF_COLLISION_PAIRS][4];  /* sphere A, sphere B, epsilon, sigma */
  /* ---- carried object ("carried object" below): the capacity and the factor's constants; the spheres themselves and
   * their link are data of gpmp2mi_plan_set_carried.  All default to 0 = none; without capacity the other four fields
   * are not read.  (They stand ahead of the workspace-path block; fill the struct by field name.) */
  int max_carried_spheres;       /* capacity reserved at plan creation, <= GPMP2MI_MAX_CARRIED_SPHERES; 0: none */
  int carried_first, carried_last;   /* inclusive range of support states that carry the factor */
  double carried_epsilon, carried_sigma;
  /* ---- workspace path ("workspace path" below): room for one target pose and one sigma per support state; the path
   * itself is data of gpmp2mi_plan_set_workspace_path.  All default to 0 = none.  (They stand ahead of the moving-sphere
   * block, which stays the struct's tail; fill the struct by field name.) */
  int workspace_path;            /* 1: reserve the path at plan creation; 0: none */
  int workspace_path_mode;       /* GPMP2MI_WORKSPACE_POSITION / _ORIENTATION / _POSE */
  int workspace_path_link;       /* link index of the FK model */
  /* ---- self-collision table ("self-collision table in a plan" below): room for a pair table of any size; the table
   * itself is data of gpmp2mi_plan_set_self_pairs.  All default to 0 = none */
  int max_self_pairs;            /* capacity reserved at plan creation, <= GPMP2MI_MAX_PLAN_SELF_PAIRS; 0: none */
  int self_pairs_first, self_pairs_last;   /* inclusive range of support states that carry the factor */
  /* ---- moving spheres ("moving obstacles" below): the capacity and the factor's constants; the spheres themselves are
   * data of gpmp2mi_plan_set_moving_spheres.  Appended at the end of the struct; all default to 0 = none */
  int max_moving_spheres;        /* capacity reserved at plan creation, <= GPMP2MI_MAX_MOVING_SPHERES; 0: none */
  int moving_first, moving_last; /* inclusive range of support states that carry the factor */
  double moving_epsilon, moving_sigma;
} gpmp2mi_graph_opts;
void gpmp2mi_graph_opts_default(gpmp2mi_graph_opts* o);

/* ---- the planner: a resident batch of B trajectory problems ------------------------------- */
/* Replaces gpmp2::BatchTrajOptimize{2DArm,3DArm,Pose2MobileArm2D,Pose2MobileArm}
 * (planner/BatchTrajOptimizer.h:43-73; graph rules planner/BatchTrajOptimizer-inl.h:21-84;
 * optimizer loop planner/BatchTrajOptimizer.cpp:212-308) for B independent problems sharing one
 * robot, one SDF and one setting.  The plan owns all device workspace; nothing is allocated in
 * the optimize call, so it can be enqueued repeatedly (receding horizon).  (The scoring calls take their workspace
 * at their first use for an inter_step and keep it: see "scoring" below; so do the posterior calls, the seeded
 * calls and the sampled-clearance calls at their first use: see "posterior", "seeding" and "sampled clearance".) */
typedef struct gpmp2mi_plan gpmp2mi_plan;
int gpmp2mi_plan_create(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf,
                        const gpmp2mi_settings* setting, const gpmp2mi_graph_opts* opts /*NULL ok*/,
                        int B, gpmp2mi_plan** out);
void gpmp2mi_plan_destroy(gpmp2mi_plan* p);

/* start/end priors (PriorFactor on x_0,v_0,x_N,v_N; BatchTrajOptimizer-inl.h:41-48) and the
 * initial values, host pointers: start_conf,start_vel,end_conf,end_vel [B][D]; init [B][N+1][2D] */
int gpmp2mi_plan_set_problem(gpmp2mi_plan* p, const double* start_conf, const double* start_vel,
                             const double* end_conf, const double* end_vel, const double* init);
/* same with device pointers; copies are enqueued on `stream` (hipStream_t) */
int gpmp2mi_plan_set_problem_dev(gpmp2mi_plan* p, const double* start_conf, const double* start_vel,
                                 const double* end_conf, const double* end_vel, const double* init,
                                 void* stream);

/* Run gpmp2::optimize on every trajectory of the batch.  All work is enqueued on `stream`
 * (hipStream_t; NULL = the default stream) and stays on the device; the host only follows the
 * per-pass active counts (pinned flags, no copies) to know when to stop enqueueing passes, and the call
 * returns once the stream has drained.  Re-running after set_problem re-optimises. */
int gpmp2mi_plan_optimize(gpmp2mi_plan* p, void* stream);

/* Results.  traj [B][N+1][2D]; iters [B] (GTSAM `iterations()`); final_error [B] (graph error of
 * the returned values); status [B] (GPMP2MI_TRAJ_*); error_trace [B][max_iter+1] (error before
 * iteration k, entry 0 = initial error; unused entries NaN).  Any pointer may be NULL. */
int gpmp2mi_plan_get_result(gpmp2mi_plan* p, double* traj, int* iters, double* final_error,
                            int* status, double* error_trace);
int gpmp2mi_plan_get_result_dev(gpmp2mi_plan* p, double* traj, int* iters, double* final_error,
                                int* status, void* stream);
/* device pointer to the resident [B][N+1][2D] result (valid until the plan is destroyed) */
const double* gpmp2mi_plan_traj_dev(const gpmp2mi_plan* p);

/* ---- a queue of problems through one plan -----------------------------------------------------
 * M >= 1 independent problems of this plan's graph (BatchTrajOptimize* called M times with the plan's
 * robot, SDF, setting and graph_opts) through its B slots.  When a slot's problem finishes, the device
 * writes out its result and loads the next problem into the slot at the pass boundary; the host only
 * follows the per-pass counts, as in gpmp2mi_plan_optimize.
 * Inputs: start_conf, start_vel, end_conf, end_vel [M][D]; init [M][N+1][2D].
 * Outputs, row j = problem j whichever slot it ran in; any may be NULL: traj [M][N+1][2D], iters [M],
 * final_error [M], status [M], error_trace [M][max_iter+1].
 * Contract:
 *  - Results.  For problem j the queue returns the iters, status, final_error and error_trace that
 *    set_problem + optimize would return for j on the same plan, and a value-identical trajectory (+0 and
 *    -0 compare equal): the forms are chosen once per plan and no kernel mixes trajectories.
 *  - Coverage: every plan gpmp2mi_plan_optimize accepts (GN, LM, Dogleg, fixed_iterations, all robot
 *    kinds, narrow / wide / dense blocks, plan-level extra factors).
 *  - Slot assignment is deterministic: at each pass boundary the slots whose problem finished take the next
 *    problems in ascending slot order (a rank from a scan over the slots, no atomic pop).  Fixed-iteration
 *    Gauss-Newton plans load new problems only at the boundaries that close a round of fixed_iterations + 1
 *    passes, so that the slots stay in lockstep.
 *  - Errors: GPMP2MI_ERR_INVALID for M < 1 or a NULL input, and for a slot that carries replanning state:
 *    state priors (gpmp2mi_plan_fix_state / add_state_estimate; clear them with
 *    gpmp2mi_plan_clear_state_priors) or a removed goal (gpmp2mi_plan_remove_goal; undo it with
 *    gpmp2mi_plan_change_goal).  A goal set by change_goal alone is fine: every problem brings its own
 *    end conf / vel.  A poisoned plan returns GPMP2MI_ERR_TIMEOUT, and a pass that times out poisons the plan
 *    as in gpmp2mi_plan_optimize.
 *  - Afterwards the plan holds no problem: gpmp2mi_plan_get_result returns GPMP2MI_ERR_INVALID until the
 *    next set_problem + optimize.
 * Host pointers: the M problems are staged on the device once and the results copied back once; the call
 * runs on the default stream and returns when it is done. */
int gpmp2mi_plan_optimize_queue(gpmp2mi_plan* p, int M, const double* start_conf, const double* start_vel,
                                const double* end_conf, const double* end_vel, const double* init,
                                double* traj, int* iters, double* final_error, int* status, double* error_trace);
/* the same on device pointers, all work on `stream` (hipStream_t); returns once the stream has drained */
int gpmp2mi_plan_optimize_queue_dev(gpmp2mi_plan* p, int M, const double* start_conf, const double* start_vel,
                                    const double* end_conf, const double* end_vel, const double* init,
                                    double* traj, int* iters, double* final_error, int* status,
                                    double* error_trace, void* stream);
/* of the last queue run on this plan: passes, B * passes, and the sum over passes of the slots that held a
 * problem (GPMP2MI_ERR_INVALID before the first queue run) */
typedef struct gpmp2mi_queue_stats {
  int passes;
  long slot_passes;
  long busy_slot_passes;
} gpmp2mi_queue_stats;
int gpmp2mi_plan_queue_stats(const gpmp2mi_plan* p, gpmp2mi_queue_stats* out);

/* ---- one batch sharded across several GPUs of this process ------------------------------------
 * A multi plan owns one ordinary gpmp2mi_plan per shard, each on its own device and its own non-blocking stream, with
 * B's rows split into contiguous shards.  The robot and the field are used on the device they
 * were created on; every other device in `devices` gets one copy of each, owned by the multi plan (the field copy is
 * a device-to-device copy of the voxels, re-packed there: bit-identical cells).  As with gpmp2mi_plan_create the
 * caller keeps the robot and the field alive until the multi plan is destroyed.
 * Contract:
 *  - Rows.  Shard k holds batch rows [row_begin[k], row_begin[k+1]); the first B % nshards shards get one row more
 *    (gpmp2_amd/sharding.py shard_range).  The M problems of a queue run are split by the same rule; a shard without
 *    problems sits out, so M < nshards is fine.
 *  - Devices may repeat ({0, 0}): every shard still has its own plan and stream.
 *  - Results.  For every row, iters, status, final_error and error_trace are identical to those of a single-device
 *    gpmp2mi_plan of that shard's size solving the same rows, and traj is value-identical (+0 and -0 compare equal).
 *    The same holds against one plan of size B whenever both choose the same kernel forms: every Gauss-Newton and LM
 *    plan.  Dogleg plans of B > 256 split into shards of <= 256 rows are the exception (the four-wavefront
 *    linearization is taken up to 256 rows only), and agree with the one plan within the parity contract.
 *  - Errors.  GPMP2MI_ERR_INVALID for a NULL argument, nshards outside 1..GPMP2MI_MAX_SHARDS, B < nshards, a device id
 *    outside 0..gpmp2mi_device_count()-1 (checked after the other arguments, once a device is known to be usable),
 *    results requested before optimize, and a NULL queue input.  A failing shard sets gpmp2mi_last_error to
 *    "shard k (device d): <message>", the first failing shard in shard order when several fail.  A shard that times out
 *    poisons its plan as gpmp2mi_plan_optimize does; the multi plan then returns GPMP2MI_ERR_TIMEOUT from every later
 *    call, and gpmp2mi_multi_plan_destroy leaks what the poisoned shards may still use (their plans, streams, staging
 *    and the copies on their devices) and frees the rest.
 *  - The caller's current device is the same on return as on entry.
 *  - Concurrency: shard 0 runs on the calling thread, shards 1.. on one host thread each, which spins on its plan's pass
 *    counts like gpmp2mi_plan_optimize.  Each call returns when every shard is done, except get_result_dev. */
#define GPMP2MI_MAX_SHARDS 16   /* one spinning host thread per shard */
typedef struct gpmp2mi_multi_plan gpmp2mi_multi_plan;
int gpmp2mi_multi_plan_create(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, const gpmp2mi_settings* setting,
                              const gpmp2mi_graph_opts* opts /*NULL ok*/, int B, int nshards, const int* devices,
                              gpmp2mi_multi_plan** out);
void gpmp2mi_multi_plan_destroy(gpmp2mi_multi_plan* m);   /* NULL: no-op */
/* nshards, devices [nshards] and row_begin [nshards + 1] (row_begin[nshards] = B); devices / row_begin may be NULL */
int gpmp2mi_multi_plan_shards(const gpmp2mi_multi_plan* m, int* nshards, int* devices, int* row_begin);
/* host pointers, B rows as gpmp2mi_plan_set_problem */
int gpmp2mi_multi_plan_set_problem(gpmp2mi_multi_plan* m, const double* start_conf, const double* start_vel,
                                   const double* end_conf, const double* end_vel, const double* init);
/* every shard concurrently; returns when all are done */
int gpmp2mi_multi_plan_optimize(gpmp2mi_multi_plan* m);
/* host pointers in batch order, as gpmp2mi_plan_get_result; any may be NULL */
int gpmp2mi_multi_plan_get_result(gpmp2mi_multi_plan* m, double* traj, int* iters, double* final_error, int* status,
                                  double* error_trace);
/* Gather onto `device`: the outputs are device pointers there (any may be NULL).  Each shard copies its rows on its own
 * stream (a peer copy from another device), after `stream` (hipStream_t on `device`, NULL = its default stream) has
 * reached this call; `stream` then waits for every shard's copies.  Returns without a host synchronisation. */
int gpmp2mi_multi_plan_get_result_dev(gpmp2mi_multi_plan* m, int device, double* traj, int* iters, double* final_error,
                                      int* status, void* stream);
/* M problems, host pointers as gpmp2mi_plan_optimize_queue; shard k runs its contiguous share through its plan's queue */
int gpmp2mi_multi_plan_optimize_queue(gpmp2mi_multi_plan* m, int M, const double* start_conf, const double* start_vel,
                                      const double* end_conf, const double* end_vel, const double* init, double* traj,
                                      int* iters, double* final_error, int* status, double* error_trace);
/* of the last queue run, shard `shard` (all zero for a shard that had no problems); GPMP2MI_ERR_INVALID before one */
int gpmp2mi_multi_plan_queue_stats(const gpmp2mi_multi_plan* m, int shard, gpmp2mi_queue_stats* out);

/* ---- incremental replanning ---------------------------------------
 * The role of gpmp2::ISAM2TrajOptimizer{2DArm,3DArm,Pose2MobileArm...}
 * (planner/ISAM2TrajOptimizer.h:57-171, planner/ISAM2TrajOptimizer-inl.h:16-195; usage
 * matlab/WAMReplannerExample.m:102-126) on the same resident plan: the chain graph is re-solved warm
 * from the current estimate with extra per-state priors.  One gpmp2mi_plan_update(p, 1, ...) is one
 * relinearise-and-solve Gauss-Newton step of the WHOLE chain -- iSAM2 would relinearise only the
 * variables whose delta exceeds relinearizeThreshold (1e-3, -inl.h:20-21); exact iSAM2 parity is
 * unpinned (no reference test exercises it, planner/tests/testISAM2TrajOptimizer.cpp:24-67).
 * `b` selects the trajectory of the batch; up to GPMP2MI_MAX_STATE_PRIORS priors per trajectory. */
#define GPMP2MI_MAX_STATE_PRIORS 8
/* fixConfigAndVel(state_idx, conf, vel): tight priors (conf_prior_model / vel_prior_model)  -inl.h:159-169 */
int gpmp2mi_plan_fix_state(gpmp2mi_plan* p, int b, int state_idx, const double* conf, const double* vel);
/* addPoseEstimate / addStateEstimate: Gaussian priors with full covariance [D][D]; vel / vel_cov may be
 * NULL (pose only)  -inl.h:172-195 */
int gpmp2mi_plan_add_state_estimate(gpmp2mi_plan* p, int b, int state_idx, const double* conf,
                                    const double* conf_cov, const double* vel, const double* vel_cov);
/* changeGoalConfigAndVel / removeGoalConfigAndVel  -inl.h:118-156 */
int gpmp2mi_plan_change_goal(gpmp2mi_plan* p, int b, const double* goal_conf, const double* goal_vel);
int gpmp2mi_plan_remove_goal(gpmp2mi_plan* p, int b);
int gpmp2mi_plan_clear_state_priors(gpmp2mi_plan* p, int b);
/* update(): `iterations` Gauss-Newton steps warm-started from the current estimate (the result of the
 * previous optimize / update; the initial values if there is none).  Results via gpmp2mi_plan_get_result. */
int gpmp2mi_plan_update(gpmp2mi_plan* p, int iterations, void* stream);

/* NonlinearFactorGraph::error(values) of the plan's graph for arbitrary trajectories
 * (host pointers; traj [B][N+1][2D] -> err [B]); uses the plan's start/end priors. */
int gpmp2mi_plan_graph_error(gpmp2mi_plan* p, const double* traj, double* err);

/* One linearization of the plan's graph at `traj` (host pointers) exported as the block-
 * tridiagonal normal equations  H delta = -g  with block size n = 2D and ordering z_i=[x_i;v_i]:
 *   Hdiag [B][N+1][n][n]  (full symmetric blocks), Hoff [B][N][n][n] (block (i+1,i)),
 *   g [B][N+1][n] (= J^T Sigma^-1 r), err [B].   Any output may be NULL. */
int gpmp2mi_plan_linearize(gpmp2mi_plan* p, const double* traj, double* Hdiag, double* Hoff,
                           double* g, double* err);

/* One-shot convenience wrapper with host buffers: create plan, set problem, optimize, fetch. */
int gpmp2mi_batch_optimize(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf,
                           const gpmp2mi_settings* setting, const gpmp2mi_graph_opts* opts, int B,
                           const double* start_conf, const double* start_vel,
                           const double* end_conf, const double* end_vel, const double* init,
                           double* traj_out, int* iters, double* final_error, int* status);

/* gpmp2::CollisionCost{2DArm,3DArm,...} planner/BatchTrajOptimizer-inl.h:87-100:
 * sum over all states of the unary obstacle error with epsilon = 0.  traj [B][N+1][2D] host. */
int gpmp2mi_collision_cost(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, int total_step,
                           int B, const double* traj, double* cost);

/* ---- scoring: dense collision check and selection, on the device ----------------------------------
 * gpmp2::CollisionCost* looks at the support states only, and the reference's workflow then up-samples the
 * trajectory for execution (interpolateArmTraj, matlab/WAMPlannerExample.m): between two support states the robot
 * can be inside an obstacle that both of them clear.  These calls check the states that are executed and pick
 * the trajectory to execute, without the trajectories leaving the device.
 *
 * Definitions, for one trajectory traj [N+1][2D], delta_t and inter_step = J >= 0:
 *  - Checked states: gpmp2mi_interpolate_traj(inter_step = J, start 0, end N), Md = N*(J+1) + 1 states (linear GP for
 *    vector-space robots, the Pose2 interpolator for the mobile kinds, following the robot's kind).  State k is a
 *    support state iff k % (J+1) == 0; only the configuration half is used.  J = 0 checks the support states only.
 *  - For checked state k and sphere s (ids in the order of the robot description): centre = sphereCenters(conf_k)[s],
 *    field lookup as gpmp2mi_sdf_query (planar fields use x, y); in_range as there, and a non-finite centre is out of
 *    range; clearance(k, s) = dist - radius_s where in range.
 *  - support_cost [B]: sum over support states and spheres of (dist > radius ? 0 : radius - dist), 0 out of range:
 *    the value of gpmp2mi_collision_cost.  dense_cost [B]: the same sum over all Md checked states.
 *    min_clearance [B]: min of clearance(k, s) over the in-range pairs, +inf if there is none.  worst [B][2]: the
 *    (k, s) attaining it, on exact ties the lowest k, then the lowest s; (-1, -1) if none.  out_of_range [B]: number
 *    of (k, s) pairs out of range.  Any output may be NULL.
 *  - Determinism: a row's results are a function of that row, the robot, the field, delta_t and J alone.  Sums are
 *    taken in an order fixed by (N, J, S), not by B, the row's position, the entry point or the device, and without
 *    floating-point atomics: a row scores bit-identically alone, in any batch, through a plan or a multi plan.
 *  - Selection over B rows with required_clearance and require_in_range:
 *      eligible(b) = status[b] != GPMP2MI_TRAJ_NOT_SPD && isfinite(final_error[b])
 *                    && min_clearance[b] >= required_clearance && (!require_in_range || out_of_range[b] == 0)
 *    best = the eligible row with the smallest final_error, the lowest row on ties, -1 if none; n_eligible = their
 *    number.  status NULL = all fine; a NaN clearance is never eligible.
 * Errors: GPMP2MI_ERR_INVALID (checked before any device work) for a NULL robot / sdf / traj / plan / final_error /
 * min_clearance, inter_step < 0, B < 0, total_step < 1, delta_t <= 0; B == 0 is fine and does nothing.
 * Memory: the `_dev` forms enqueue two kernels on `stream` and return without a host synchronisation.  They need a
 * workspace of one 40-byte record per 64 checked states of every row: a plan takes it (with the staging of its
 * host-pointer forms) at the first score / select call for an inter_step and keeps it -- the one exception to
 * "nothing is allocated after gpmp2mi_plan_create"; gpmp2mi_score_traj_dev keeps it with the robot handle.  A later
 * call that needs no more room neither allocates nor synchronises; one that needs more waits for the device while
 * the block is replaced.  Calls that share a robot handle (gpmp2mi_score_traj*) or a plan therefore belong on one
 * stream, or in stream order. */

/* caller buffers, e.g. the traj output of gpmp2mi_plan_optimize_queue(_dev); traj [B][total_step+1][2D].
 * The record workspace of these two calls lives with the robot handle, on the device the handle was created on: that
 * device must be current (GPMP2MI_ERR_INVALID otherwise).  Host threads may share the handle, but its records serve one
 * call at a time: calls on one robot handle must follow each other in stream order (one stream, or events between
 * streams).  To score concurrently on several streams use one robot handle per stream, or gpmp2mi_plan_score on one
 * plan per stream. */
int gpmp2mi_score_traj(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, double delta_t, int inter_step, int B,
                       int total_step, const double* traj, double* support_cost, double* dense_cost,
                       double* min_clearance, int* worst, int* out_of_range);
int gpmp2mi_score_traj_dev(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, double delta_t, int inter_step, int B,
                           int total_step, const double* traj, double* support_cost, double* dense_cost,
                           double* min_clearance, int* worst, int* out_of_range, void* stream);
/* The selection rule.  Host pointers: B comparisons on the host, no device needed (out_of_range may be NULL unless
 * require_in_range).  _dev: one kernel; best / n_eligible are device ints. */
int gpmp2mi_select_best(int B, const double* final_error, const int* status, const double* min_clearance,
                        const int* out_of_range, double required_clearance, int require_in_range, int* best,
                        int* n_eligible);
int gpmp2mi_select_best_dev(int B, const double* final_error, const int* status, const double* min_clearance,
                            const int* out_of_range, double required_clearance, int require_in_range, int* best,
                            int* n_eligible, void* stream);
/* The plan's resident result (delta_t from its setting).  GPMP2MI_ERR_INVALID before the first optimize / update and
 * after a queue run (the plan then holds no problem, as gpmp2mi_plan_get_result); GPMP2MI_ERR_TIMEOUT for a poisoned
 * plan, before anything is enqueued. */
int gpmp2mi_plan_score(gpmp2mi_plan* p, int inter_step, double* support_cost, double* dense_cost,
                       double* min_clearance, int* worst, int* out_of_range);
int gpmp2mi_plan_score_dev(gpmp2mi_plan* p, int inter_step, double* support_cost, double* dense_cost,
                           double* min_clearance, int* worst, int* out_of_range, void* stream);
/* Score, apply the rule to the plan's final_error / status and copy the chosen row in one enqueue:
 * traj_best [N+1][2D] and its up-sampled form dense_best [Md][2D]: what gpmp2mi_interpolate_traj gives for that row,
 * bit for bit for vector-space robots; for Pose2 robots the same arithmetic evaluated once per coordinate, equal to
 * rounding (tested at 1e-12).  With best == -1 both are left untouched.  Any output may be NULL. */
int gpmp2mi_plan_select(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range, int* best,
                        int* n_eligible, double* traj_best, double* dense_best);
int gpmp2mi_plan_select_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range, int* best,
                            int* n_eligible, double* traj_best, double* dense_best, void* stream);
/* Multi plans, host pointers in batch order: every shard scores its rows concurrently on its own device and stream as
 * in gpmp2mi_multi_plan_optimize; the pick over the shards' candidates is the same rule on the host, so the answer is
 * that of one plan of size B.  Errors and the caller's current device as the other multi-plan calls. */
int gpmp2mi_multi_plan_score(gpmp2mi_multi_plan* m, int inter_step, double* support_cost, double* dense_cost,
                             double* min_clearance, int* worst, int* out_of_range);
int gpmp2mi_multi_plan_select(gpmp2mi_multi_plan* m, int inter_step, double required_clearance, int require_in_range,
                              int* best, int* n_eligible, double* traj_best, double* dense_best);

/* ---- self-collision check: the executed trajectory against the robot itself, on the device ----------------------
 * The calls of "scoring" test the body spheres against the signed-distance field only, and the in-plan SelfCollision
 * factor holds at most GPMP2MI_MAX_SELF_COLLISION_PAIRS rows on support states.  These calls test every checked state
 * of "scoring" against a pair table of any size, and let the selection ask for both clearances.
 *
 * Definitions:
 *  - Pair table: data [P][4] doubles, the matrix of gpmp2::SelfCollision (obstacle/SelfCollision.h:39-45) that
 *    gpmp2mi_self_collision_factor takes: sphere A id, sphere B id (ids in the order of the robot description), epsilon,
 *    sigma.  Column 3 is not read.  total_eps_p = radius_A + radius_B + epsilon_p, evaluated in that order on the host
 *    in fp64 (SelfCollision.h:89).
 *  - Checked states: exactly those of "scoring" for one trajectory, delta_t and inter_step = J: Md = N (J+1) + 1 states;
 *    Pose2 robot kinds go through the Pose2 interpolator; only the configuration half is used.
 *  - For checked state k and pair p: dist = |c_A - c_B| with the centres of sphereCenters(conf_k);
 *    clearance(k, p) = dist - total_eps_p; hinge = dist > total_eps_p ? 0 : total_eps_p - dist (SelfCollision.h:114-127).
 *    A pair whose dist is not finite is invalid: it adds nothing to the sums or the minimum, and it is counted.
 *  - self_support_cost [B]: the hinge sum over support states = the sum of the unwhitened
 *    gpmp2mi_self_collision_factor errors at those states.  self_dense_cost [B]: the same sum over all Md states.
 *    min_self_clearance [B]: min of clearance(k, p) over the valid (k, p), +inf if there is none.  worst [B][2]: the
 *    (k, p) attaining it, p the row of the caller's table; on exact ties the lowest k, then the lowest p; (-1, -1) if
 *    none.  invalid [B]: number of invalid (k, p).  Any output may be NULL.
 *  - Determinism as in "scoring": a row's results are a function of that row, the robot, the table, delta_t and J alone;
 *    sums are taken in an order fixed by (N, J, S, P) and the table's order, without floating-point atomics: a row scores
 *    bit-identically alone, in any batch, through the trajectory form or the plan form.
 *  - Selection: the rule of "scoring" with one more condition,
 *      eligible(b) = <the rule of "scoring"> && invalid[b] == 0 && min_self_clearance[b] >= required_self_clearance;
 *    everything else as there, the lowest row on ties included.
 * Errors: GPMP2MI_ERR_INVALID (checked before any device work) for a NULL argument, the argument errors of "scoring",
 * and a table made for a robot with another sphere count, dof or kind.
 * Memory: the workspace rules of "scoring".  A plan keeps the records (one 40-byte record per tile of checked states of
 * every row: 64 states for S <= 32 spheres, 32 for S <= 64, 16 above) with the staging of its host-pointer forms, taken
 * at the first call and kept; gpmp2mi_self_score_traj_dev keeps them with the PAIR TABLE, not with the robot handle, so
 * calls that share a table belong on one stream, or in stream order.
 * Not here: gpmp2mi_multi_plan_* twins, a self-collision term in the risk / collision-probability calls. */
typedef struct gpmp2mi_self_pairs gpmp2mi_self_pairs;   /* device-resident table, bound to the robot's sphere model */

/* GPMP2MI_ERR_INVALID, before any device work, for a NULL argument, P < 0, an id that is not an integer in
 * [0, nr_spheres), or A == B.  P == 0 is a valid, empty table (data may be NULL): every row then has costs 0,
 * clearance +inf and worst (-1, -1).  A non-empty table lives on the current device, which must be the robot's. */
int gpmp2mi_self_pairs_create(const gpmp2mi_robot* robot, int P, const double* data /*[P][4]*/, gpmp2mi_self_pairs** out);
/* All pairs A < B, in lexicographic order, whose links are at least min_joint_gap (>= 1) joints apart in the kinematic
 * tree of the robot's kind: link 0 is the vehicle of the mobile kinds, link 1 the torso of the lift kinds, the first
 * links of both arms of a two-arm kind are children of the same parent; for a fixed-base arm the distance is the
 * difference of the link indices; a point robot yields no pair.  Less the pairs whose clearance with epsilon 0 is
 * negative at any of the n_ref reference configurations ref_conf [n_ref][D] (n_ref may be 0): spheres that overlap by
 * construction.  Every row gets (epsilon, sigma). */
int gpmp2mi_self_pairs_generate(const gpmp2mi_robot* robot, int min_joint_gap, int n_ref, const double* ref_conf,
                                double epsilon, double sigma, gpmp2mi_self_pairs** out);
int gpmp2mi_self_pairs_count(const gpmp2mi_self_pairs* pairs);   /* -1 for NULL */
int gpmp2mi_self_pairs_get(const gpmp2mi_self_pairs* pairs, double* data /*[P][4]*/);
void gpmp2mi_self_pairs_destroy(gpmp2mi_self_pairs* pairs);      /* NULL: no-op */

/* caller buffers; traj [B][total_step+1][2D].  The device of the robot handle and the table must be current. */
int gpmp2mi_self_score_traj(const gpmp2mi_robot* robot, const gpmp2mi_self_pairs* pairs, double delta_t, int inter_step,
                            int B, int total_step, const double* traj, double* self_support_cost,
                            double* self_dense_cost, double* min_self_clearance, int* worst, int* invalid);
int gpmp2mi_self_score_traj_dev(const gpmp2mi_robot* robot, const gpmp2mi_self_pairs* pairs, double delta_t,
                                int inter_step, int B, int total_step, const double* traj, double* self_support_cost,
                                double* self_dense_cost, double* min_self_clearance, int* worst, int* invalid,
                                void* stream);
/* The plan's resident result; preconditions and errors as gpmp2mi_plan_score. */
int gpmp2mi_plan_self_score(gpmp2mi_plan* p, const gpmp2mi_self_pairs* pairs, int inter_step, double* self_support_cost,
                            double* self_dense_cost, double* min_self_clearance, int* worst, int* invalid);
int gpmp2mi_plan_self_score_dev(gpmp2mi_plan* p, const gpmp2mi_self_pairs* pairs, int inter_step,
                                double* self_support_cost, double* self_dense_cost, double* min_self_clearance,
                                int* worst, int* invalid, void* stream);
/* gpmp2mi_plan_select with the extended rule, one enqueue: the obstacle scores, the self scores, then one finish that
 * reads both.  Outputs as gpmp2mi_plan_select. */
int gpmp2mi_plan_select_checked(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                const gpmp2mi_self_pairs* pairs, double required_self_clearance, int* best,
                                int* n_eligible, double* traj_best, double* dense_best);
int gpmp2mi_plan_select_checked_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                    const gpmp2mi_self_pairs* pairs, double required_self_clearance, int* best,
                                    int* n_eligible, double* traj_best, double* dense_best, void* stream);

/* ---- motion limits: can the robot execute the trajectory, and how much slower must it run, on the device ---------
 * The calls of "scoring" and "self-collision check" ask whether the executed trajectory is free of collisions.  GPMP2's
 * joint and velocity limits are soft hinge factors on support states, off by default; nothing bounds acceleration or
 * Cartesian speed, and between two support states the GP mean is a cubic whose velocity peaks where no factor looks.
 * These calls test every checked state of "scoring" against joint ranges, joint speeds, joint accelerations and a
 * Cartesian speed of the body spheres, give the factor by which a row's duration must be stretched to become
 * executable, and let the selection ask for both.
 *
 * Definitions, for one trajectory traj [N+1][2D], delta_t = dt and inter_step = J >= 0:
 *  - Checked states: exactly those of "scoring", Md = N (J+1) + 1 states; BOTH halves of gpmp2mi_interpolate_traj are
 *    used: configuration q_k and velocity v_k (the linear GP for vector-space robots, the Pose2 interpolator for the
 *    mobile kinds; support states are copies).
 *  - Limits: gpmp2mi_motion_limits, HOST pointers, each [dof] or NULL, and one scalar.  An infinite entry or a NULL array
 *    means no limit of that kind for that coordinate; pos_down / pos_up are both NULL or both given; coordinate d has a
 *    position limit iff pos_down[d] or pos_up[d] is finite.  point_speed = +inf: no Cartesian limit.
 *    gpmp2mi_motion_limits_default fills "no limit".  The arrays are read before the call returns.
 *  - Mobile kinds: position limits and acceleration limits on coordinates 0..2 are not applied (the former as
 *    JointLimitFactorPose2Vector does); velocity limits on 0..2 apply to the velocity half as stored (body frame).
 *  - pos_margin [B]: min over (k, d) with a position limit of min(q_k[d] - down[d], up[d] - q_k[d]), an infinite side
 *    left out.  Negative: outside.  +inf if nothing is limited.
 *  - vel_ratio [B]: max over (k, d) with a finite vel[d] of |v_k[d]| / vel[d]; 0 if nothing is limited.
 *  - acc_ratio [B]: max over interval i < N, end e in {0, 1} and d with a finite acc[d] of |a_i,e[d]| / acc[d], with the
 *    acceleration of the interpolated mean inside interval i (support states x0 v0, x1 v1) at its two ends,
 *      a_i,0 = 6 (x1 - x0) / dt^2 - (4 v0 + 2 v1) / dt,    a_i,1 = -6 (x1 - x0) / dt^2 + (2 v0 + 4 v1) / dt.
 *    The mean is a cubic Hermite in every vector coordinate, so its acceleration is linear in time and these 2N values
 *    bound it over continuous time; acc_ratio does not depend on J.  0 if nothing is limited.
 *  - point_speed [B]: max over (k, s) of |J_s(q_k) v_k|, J_s the 3 x D Jacobian of sphereCenters as
 *    gpmp2mi_sphere_centers returns it, s in the order of the robot description.  Computed whatever the limits are.
 *  - time_scale [B] = max(vel_ratio, sqrt(acc_ratio), point_speed / limits.point_speed): the smallest factor s such that
 *    the same path run over s * total_time meets every rate limit (velocities and point speeds scale by 1/s,
 *    accelerations by 1/s^2); s <= 1: executable as planned.  Position limits cannot be bought with time.
 *  - worst [B][4][2]: the (k, d), (k, d), (2i+e, d), (k, s) attaining the four extrema, on exact ties the lowest first
 *    index, then the lowest second; (-1, -1) if none.
 *  - invalid [B]: the number of evaluated quantities (margins and ratios of limited coordinates, every point speed) that
 *    are not finite.  Such a quantity enters no extremum.  Every quantity is evaluated per coordinate: a non-finite
 *    coordinate of a support state makes that coordinate non-finite in the checked states of the two intervals around
 *    it and leaves the other coordinates alone, and a sphere's speed is the sum over the Jacobian columns of the
 *    joints its link hangs from only (the others are zero), so a non-finite joint further out leaves it finite.  Any
 *    output may be NULL.
 *  - Determinism: every output is an extremum with an index key: no sums, no atomics.  A row's results are a function of
 *    the row, the robot, the limits, delta_t and J alone: bit-identical alone, in any batch, through the trajectory form
 *    or the plan form.
 *  - Selection: the rule of "scoring", extended as in "self-collision check" when pairs != NULL, and then
 *      eligible(b) = <that rule> && invalid[b] == 0 && pos_margin[b] >= required_pos_margin
 *                    && time_scale[b] <= max_time_scale;
 *    the ranking stays final_error, the lowest row on ties.  With all limits off and max_time_scale = +inf the answer is
 *    that of gpmp2mi_plan_select / gpmp2mi_plan_select_checked for rows without a non-finite coordinate.
 *    time_scale_best: time_scale of the chosen row (untouched when none is).  dense_best is not rescaled: the caller
 *    divides its velocities by time_scale_best.
 * Errors, before any device work: GPMP2MI_ERR_INVALID for a NULL robot / limits / traj / plan, the argument errors of
 * "scoring", a NaN limit, down > up, a vel / acc / point_speed entry <= 0, one of pos_down / pos_up alone, a NaN
 * required_pos_margin / max_time_scale, and a pair table made for another robot; GPMP2MI_ERR_TIMEOUT for a poisoned
 * plan.  A refused call writes nothing and leaves the plan usable.
 * Memory: the workspace rules of "scoring": one 72-byte record per 64 checked states of every row.  A plan takes the
 * records, a few [B] arrays and the staging of its host-pointer forms at the first call and keeps them (grown when a
 * later call needs more): one more exception to "nothing is allocated after gpmp2mi_plan_create".
 * gpmp2mi_motion_score_traj_dev keeps its records with the robot handle, under the stream-order rule of
 * gpmp2mi_score_traj_dev.  The `_dev` forms enqueue and return.  The plan forms read the plan's resident result and
 * delta_t, have the preconditions of gpmp2mi_plan_score and leave the optimizer's state untouched.
 * Not here: gpmp2mi_multi_plan_* twins, a motion term inside gpmp2mi_plan_select_distinct, the acceleration of the Pose2
 * coordinates (the acceleration of the tangent-space interpolation is not built), exact continuous-time velocity maxima
 * between checked states, jerk limits.  time_scale is one uniform factor per row; the per-state speed profile is
 * "re-timing" below. */
typedef struct gpmp2mi_motion_limits {
  const double* pos_down;   /* [dof] or NULL (then pos_up is NULL too) */
  const double* pos_up;
  const double* vel;        /* [dof] or NULL, entries > 0 */
  const double* acc;        /* [dof] or NULL, entries > 0 */
  double point_speed;       /* > 0; +inf: no Cartesian limit */
} gpmp2mi_motion_limits;
void gpmp2mi_motion_limits_default(gpmp2mi_motion_limits* limits);

/* caller buffers; traj [B][total_step+1][2D].  The device of the robot handle must be current. */
int gpmp2mi_motion_score_traj(const gpmp2mi_robot* robot, const gpmp2mi_motion_limits* limits, double delta_t,
                              int inter_step, int B, int total_step, const double* traj, double* pos_margin,
                              double* vel_ratio, double* acc_ratio, double* point_speed, double* time_scale, int* worst,
                              int* invalid);
int gpmp2mi_motion_score_traj_dev(const gpmp2mi_robot* robot, const gpmp2mi_motion_limits* limits, double delta_t,
                                  int inter_step, int B, int total_step, const double* traj, double* pos_margin,
                                  double* vel_ratio, double* acc_ratio, double* point_speed, double* time_scale,
                                  int* worst, int* invalid, void* stream);
/* The plan's resident result; preconditions and errors as gpmp2mi_plan_score. */
int gpmp2mi_plan_motion_score(gpmp2mi_plan* p, const gpmp2mi_motion_limits* limits, int inter_step, double* pos_margin,
                              double* vel_ratio, double* acc_ratio, double* point_speed, double* time_scale, int* worst,
                              int* invalid);
int gpmp2mi_plan_motion_score_dev(gpmp2mi_plan* p, const gpmp2mi_motion_limits* limits, int inter_step,
                                  double* pos_margin, double* vel_ratio, double* acc_ratio, double* point_speed,
                                  double* time_scale, int* worst, int* invalid, void* stream);
/* gpmp2mi_plan_select (gpmp2mi_plan_select_checked when pairs != NULL) with the extended rule, one enqueue: the existing
 * score stages, the motion scores, then one finish that reads them all.  Outputs as gpmp2mi_plan_select, plus
 * time_scale_best. */
int gpmp2mi_plan_select_feasible(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                 const gpmp2mi_self_pairs* pairs /*NULL ok*/, double required_self_clearance,
                                 const gpmp2mi_motion_limits* limits, double required_pos_margin, double max_time_scale,
                                 int* best, int* n_eligible, double* time_scale_best, double* traj_best,
                                 double* dense_best);
int gpmp2mi_plan_select_feasible_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                     const gpmp2mi_self_pairs* pairs /*NULL ok*/, double required_self_clearance,
                                     const gpmp2mi_motion_limits* limits, double required_pos_margin,
                                     double max_time_scale, int* best, int* n_eligible, double* time_scale_best,
                                     double* traj_best, double* dense_best, void* stream);

/* ---- re-timing: a speed profile along the unchanged path, per checked state, on the device -------------------------
 * time_scale of "motion limits" is one uniform factor per row: one sharp corner slows the whole trajectory.  These calls
 * keep the path and give every checked state k of "scoring" (Md = N (J+1) + 1 states, spacing h = delta_t / (J+1)) a rate
 * sdot_k = ds/dt' of planned time s against executed time t', such that the duration is as short as the rate limits of
 * gpmp2mi_motion_limits allow (vel, acc, point_speed; the position limits do not depend on time and are not read).  The
 * method is time-optimal path parameterisation by reachability (the TOPP-RA scheme), specialised to box limits so that
 * every step is a minimum or maximum of quotients: no LP solver, no epsilon, and no floating-point sum but the stamps.
 * Every operation is rounded once in the order written (csrc/retime_rule.h states the rule for host and device).
 *
 * The rule, for one row, with x_k = sdot_k^2, u_k constant over stage k = 0 .. Md-2 and x_{k+1} = x_k + 2 h u_k:
 *  - Path derivatives: q'_k is the velocity half of checked state k.  q'' inside interval i is linear between a_i,0 and
 *    a_i,1 of "motion limits": at sub-state j of J+1 it is a_i,0 + (a_i,1 - a_i,0) * (j / (J+1)), the two ends exact.  At a
 *    checked state this gives a right value q''_{k+} and a left value q''_{k-}; they differ only at support states.
 *  - Cap: X_k = min(max_rate^2, min_d (vel[d] / |q'_k[d]|)^2, (point_speed / ps_k)^2), ps_k the largest sphere speed at
 *    state k (the per-state quantity whose row maximum is point_speed of "motion limits").  A zero denominator or an
 *    infinite limit contributes no cap.  max_rate is finite and > 0; with max_rate = 1 the robot never runs faster than
 *    planned.
 *  - Rows of stage k: for every joint d with a finite acc[d] two two-sided rows |a x_k + b u_k| <= acc[d]: at the start
 *    of the stage a = q''_{k+}[d], b = q'_k[d]; at its end a = q''_{(k+1)-}[d], b = q'_{k+1}[d] + 2 h q''_{(k+1)-}[d] (the
 *    acceleration at state k+1 seen from the left, written in (x_k, u_k)).  A row with b == 0 caps x_k at acc[d] / |a| and
 *    bounds no u; every other row gives the bounds -acc/|b| - (a/b) x <= u <= acc/|b| - (a/b) x.  The next set
 *    K_{k+1} = [lo, hi] gives lo/2h - x/2h <= u <= hi/2h - x/2h.
 *  - Backward pass: K_{Md-1} = [0, X_{Md-1}], or [rate_end^2, rate_end^2] when rate_end >= 0.  For k = Md-2 .. 0, K_k is
 *    the set of x in [0, X_k] for which some u meets all bounds: every (lower i, upper j) pair is one inequality
 *    alpha x <= beta with alpha = r_i - r_j, beta = pu_j - pl_i; alpha > 0 lowers the upper end to beta / alpha,
 *    alpha < 0 raises the lower end, alpha == 0 with beta < 0 makes the stage empty.
 *  - Forward pass: x_0 = hi(K_0), or rate_start^2 when rate_start >= 0.  u = the smallest upper bound pu_j + r_j x_k;
 *    x_{k+1} = x_k + 2 h u clamped into K_{k+1}; the reported u_k = (x_{k+1} - x_k) / 2h (u[Md-1] = 0).  The greedy
 *    profile is pointwise maximal over all feasible ones.
 *  - Time: stamps[0] = 0, stamps[k+1] = stamps[k] + 2 h / (sdot_k + sdot_{k+1}), summed in index order;
 *    duration = stamps[Md-1].
 *  - status [B]: GPMP2MI_RETIME_OK; _BOUNDARY: a forced rate lies outside its set (rate_start^2 outside K_0, rate_end^2
 *    above X_{Md-1}); _EMPTY: a stage set is empty, or a denominator of the time is zero; _INVALID: a non-finite q', q''
 *    or ps (path form: a cap that is NaN or < 0).  A row that is not OK has duration = +inf and NaN in sdot, u, stamps
 *    and achieved (and in the velocity half of dense_retimed).
 *  - achieved [B][4], the largest ratios after re-timing: |q'_k[d]| sdot_k / vel[d]; the accelerations
 *    |a x_k + b u_k| / acc[d] of the rows at both ends of every stage; the accelerations at the stage midpoints (x and q''
 *    at their means, q' of the cubic there); ps_k sdot_k / point_speed.  The first, second and fourth are <= 1 up to
 *    rounding.  The third shows what the discretisation leaves between checked states: O(h^2), not bounded here.  The
 *    path form has one cap: its [0] is sdot_k / sqrt(cap_k) over the finite caps, its [3] is 0.
 *  - Determinism: a row's outputs are a function of the row, the robot, the limits, delta_t, J and the three rates
 *    alone: bit-identical alone, in any batch, through the trajectory form or the plan form.
 *  - Selection (gpmp2mi_plan_select_retimed): the rule of gpmp2mi_plan_select_feasible without its time_scale test,
 *      eligible(b) = <that rule> && status[b] == GPMP2MI_RETIME_OK && duration[b] <= max_duration;
 *    the ranking stays final_error, the lowest row on ties.  Outputs as select_feasible, plus duration_best and
 *    stamps_best [Md] (untouched when no row is chosen).  dense_best carries the RE-TIMED velocities here: the velocity
 *    half of state k is multiplied by sdot_k of the chosen row, as in dense_retimed.
 * Re-timing changes WHEN the robot is where: the moving-obstacle and workspace-path checks of a row, which index their
 * spheres and targets by planned time, are not valid for the re-timed row.
 * Errors, before any device work: the argument errors of "motion limits"; GPMP2MI_ERR_INVALID for a NaN rate or
 * max_duration, max_rate <= 0 or not finite, (path form) a NULL array, Md < 2, dof outside 1..GPMP2MI_MAX_DOF, h <= 0 or
 * an acc entry that is NaN or <= 0; GPMP2MI_ERR_UNSUPPORTED, with the reason in the message, for the Pose2 kinds (the
 * acceleration of the tangent-space interpolation is not built).  A refused call writes nothing.
 * Memory: the workspace rules of "scoring".  Seven doubles per checked state of every row (ps, X, K, and sdot / u / stamps
 * where the caller gives no array), with the robot handle for gpmp2mi_retime_traj_dev (under the stream-order rule of
 * gpmp2mi_score_traj_dev), with the plan for the plan forms, taken at the first call and grown on demand.
 * gpmp2mi_retime_path_dev has no handle: the caller gives `workspace`, 3 * B * Md doubles on the device, and none of its
 * sdot / u / stamps may be NULL.  Any other output may be NULL.  The `_dev` forms enqueue and return.
 * Not here: gpmp2mi_multi_plan_* twins, jerk limits, the Pose2 kinds, a guard for quotients that overflow (a row whose
 * |b| is below acc / 1.8e308, such as a denormal velocity, is outside the rule's range). */
enum {
  GPMP2MI_RETIME_OK = 0,
  GPMP2MI_RETIME_BOUNDARY = 1,
  GPMP2MI_RETIME_EMPTY = 2,
  GPMP2MI_RETIME_INVALID = 3,
  GPMP2MI_RETIME_STATIC = 4   /* "re-timing under torque limits" only */
};
/* The bare rule on any joint-space path: qd, qdd_left, qdd_right [B][Md][D] (qdd_left of state 0 and qdd_right of state
 * Md-1 are not read), cap [B][Md] (a bound on x = sdot^2, +inf: none), acc HOST [D] or NULL, rate_start / rate_end < 0:
 * free.  sdot, u, stamps [B][Md], duration, status [B], achieved [B][4]. */
int gpmp2mi_retime_path(int B, int Md, int dof, const double* qd, const double* qdd_left, const double* qdd_right,
                        const double* cap, const double* acc, double h, double max_rate, double rate_start,
                        double rate_end, double* sdot, double* u, double* stamps, double* duration, int* status,
                        double* achieved);
int gpmp2mi_retime_path_dev(int B, int Md, int dof, const double* qd, const double* qdd_left, const double* qdd_right,
                            const double* cap, const double* acc, double h, double max_rate, double rate_start,
                            double rate_end, double* sdot, double* u, double* stamps, double* duration, int* status,
                            double* achieved, double* workspace, void* stream);
/* caller buffers; traj [B][total_step+1][2D]; dense_retimed [B][Md][2D]: the configurations as interpolated, the
 * velocities multiplied by sdot_k.  The device of the robot handle must be current. */
int gpmp2mi_retime_traj(const gpmp2mi_robot* robot, const gpmp2mi_motion_limits* limits, double delta_t, int inter_step,
                        int B, int total_step, const double* traj, double max_rate, double rate_start, double rate_end,
                        double* sdot, double* u, double* stamps, double* duration, int* status, double* achieved,
                        double* dense_retimed);
int gpmp2mi_retime_traj_dev(const gpmp2mi_robot* robot, const gpmp2mi_motion_limits* limits, double delta_t,
                            int inter_step, int B, int total_step, const double* traj, double max_rate,
                            double rate_start, double rate_end, double* sdot, double* u, double* stamps,
                            double* duration, int* status, double* achieved, double* dense_retimed, void* stream);
/* The plan's resident result; preconditions and errors as gpmp2mi_plan_score. */
int gpmp2mi_plan_retime(gpmp2mi_plan* p, const gpmp2mi_motion_limits* limits, int inter_step, double max_rate,
                        double rate_start, double rate_end, double* sdot, double* u, double* stamps, double* duration,
                        int* status, double* achieved, double* dense_retimed);
int gpmp2mi_plan_retime_dev(gpmp2mi_plan* p, const gpmp2mi_motion_limits* limits, int inter_step, double max_rate,
                            double rate_start, double rate_end, double* sdot, double* u, double* stamps,
                            double* duration, int* status, double* achieved, double* dense_retimed, void* stream);
/* gpmp2mi_plan_select_feasible with the duration of the re-timed row in place of time_scale, one enqueue. */
int gpmp2mi_plan_select_retimed(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                const gpmp2mi_self_pairs* pairs /*NULL ok*/, double required_self_clearance,
                                const gpmp2mi_motion_limits* limits, double required_pos_margin, double max_rate,
                                double rate_start, double rate_end, double max_duration, int* best, int* n_eligible,
                                double* duration_best, double* stamps_best, double* traj_best, double* dense_best);
int gpmp2mi_plan_select_retimed_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                    const gpmp2mi_self_pairs* pairs /*NULL ok*/, double required_self_clearance,
                                    const gpmp2mi_motion_limits* limits, double required_pos_margin, double max_rate,
                                    double rate_start, double rate_end, double max_duration, int* best,
                                    int* n_eligible, double* duration_best, double* stamps_best, double* traj_best,
                                    double* dense_best, void* stream);

/* ---- torque limits: the joint torques the executed trajectory asks for, by inverse dynamics on the device -----------
 * acc[d] of "motion limits" is a stand-in for what saturates an arm, which is joint torque: the acceleration a joint can
 * deliver depends on the configuration (gravity, the inertia seen at the joint), on what the other joints do (the
 * velocity products) and on how much torque is already spent holding the arm up.  These calls compute the joint torques
 * of a fixed-base arm at every checked state of "scoring", compare them with per-joint limits, say how much of each limit
 * gravity alone takes, give the factor by which a row's duration must be stretched for the drives to follow, and let the
 * selection ask for it.
 *
 * The dynamics handle (gpmp2mi_dynamics) carries the inertial parameters of the arm on the device and is bound to the
 * kinematics of the robot handle it was made for (kind, joint count, DH table, base pose).  L = gpmp2mi_robot_nr_links.
 * The link frame of link j is the frame gpmp2mi_forward_kinematics returns for it: the DH frame behind joint j's
 * transform.  Joint j turns about the z axis of the frame in front of it.  mass [L] in kg; com [L][3], the centre of mass
 * in the link frame; inertia [L][6] = ixx iyy izz ixy ixz iyz, the entries of the symmetric inertia matrix about the
 * centre of mass in the link frame (the off-diagonal ones with the sign they have in the matrix); gravity in the world
 * frame; torque [dof], the limits L_d > 0, +inf = none for that joint, NULL = none at all.  All HOST pointers, read
 * before gpmp2mi_dynamics_create returns.  gpmp2mi_dynamics_desc_default: NULL arrays, gravity (0, 0, -9.81).
 *
 * Definitions, for one trajectory traj [N+1][2D], delta_t = dt and inter_step = J >= 0:
 *  - Checked states: exactly those of "scoring", Md = N (J+1) + 1 states, with q_k and q'_k as in "motion limits" and
 *    q''_k as in "re-timing": linear between a_i,0 and a_i,1 inside interval i, the two ends exact.  A support state
 *    between two intervals has a left and a right acceleration and is evaluated for both ("sides"); the first state has
 *    the right one only, the last the left one only.
 *  - tau = ID(q, q', q'') is the inverse dynamics of the rigid chain; tau_g = ID(q, 0, 0) holds the arm still against
 *    gravity; m = tau - tau_g is what the motion asks for.  The device accumulates tau_g and m apart and forms
 *    tau = tau_g + m (the dynamics are affine in gravity), so a row at rest has m == 0 exactly.
 *  - torque_ratio [B]: max over (state, side, joint with a finite limit) of |tau_d| / L_d; 0 if nothing is limited.
 *  - static_ratio [B]: max over (state, joint with a finite limit) of |tau_g,d| / L_d.  At >= 1 no timing helps.
 *  - torque_time_scale [B]: the smallest uniform stretch c of the duration that meets every limit.  Under a stretch
 *    q' scales by 1/c and q'' by 1/c^2, so m scales by exactly 1/c^2 while tau_g stays: c^2 = max over (state, side,
 *    joint with a finite limit) of r, with r = m / (L - tau_g) for m > 0, r = -m / (L + tau_g) for m < 0 and r = 0 for
 *    m == 0 (a quotient whose denominator is <= 0 is left out: static_ratio >= 1 says it).  0 when every m is 0; +inf
 *    when static_ratio >= 1.  Consistency: given static_ratio < 1, torque_ratio <= 1 <=> torque_time_scale <= 1 (up to
 *    rounding at the boundary itself).
 *  - worst [B][3][2]: the (state, joint) attaining torque_ratio, static_ratio and c^2, on exact ties the lowest state, then
 *    the lowest joint; (-1, -1) if none.
 *  - invalid [B]: the number of (state, side, joint) whose tau is not finite, limited or not.  Such a value joins no
 *    extremum; a non-finite tau_g joins none either.
 *  - tau [B][Md][dof], optional: the torques at planned timing, the controller's feed-forward term.  At a support state
 *    the right-sided value, at the last state the left-sided one.
 *  - SAMPLED, NOT BOUNDED: the torque between two checked states is not bounded by its values at them (tau is not linear
 *    in time), unlike acc_ratio of "motion limits", whose interval ends are exact.  Raise inter_step for a finer check.
 *  - Determinism: every per-row output is an extremum with an index key or an integer count: no floating-point sum across
 *    states, no atomics.  A row's results are a function of the row, the two handles, delta_t and J alone: bit-identical
 *    alone, anywhere in any batch, through the trajectory form or the plan form.
 *  - Selection (gpmp2mi_plan_select_dynamic): the rule of gpmp2mi_plan_select_feasible with
 *      max(time_scale[b], torque_time_scale[b]) <= max_time_scale
 *    in place of its time-scale test, and the torque invalid[b] == 0 besides.  Ranking and ties are unchanged.
 *    time_scale_best is that maximum for the chosen row, tau_best [Md][dof] its torques (both untouched when none is).
 *    With every torque limit +inf, the row gpmp2mi_plan_select_feasible chooses (for rows without a non-finite torque).
 * Errors, before any device work: GPMP2MI_ERR_INVALID for a NULL argument, a non-finite entry of the description, a
 * negative mass or diagonal inertia, a torque limit that is NaN or <= 0, the argument errors of "scoring" and "motion
 * limits", and a dynamics handle made for another robot or living on another device; GPMP2MI_ERR_UNSUPPORTED, the reason
 * in the message, for any kind but GPMP2MI_ROBOT_ARM and for an arm of more than 8 joints; GPMP2MI_ERR_TIMEOUT for a
 * poisoned plan.  A refused call writes nothing and leaves the plan usable.
 * Memory: one 56-byte record per 64 checked states of every row.  A plan takes the records, the scores of the earlier
 * stages, the staging of its host-pointer forms and the torques of every row ([B][Md][dof]) at the first call and keeps
 * them (grown when a later call needs more).  gpmp2mi_torque_score_traj_dev keeps its records with the dynamics handle,
 * under the stream-order rule of gpmp2mi_score_traj_dev.  The `_dev` forms enqueue and return.  The plan forms read the
 * plan's resident result and delta_t, have the preconditions of gpmp2mi_plan_score and leave the optimizer's state and
 * every existing call's outputs untouched.
 * Not here: the mobile kinds (a moving base in the recursion); friction, rotor inertia, payload changes at run time and
 * external wrenches; a torque factor inside the optimisation; gpmp2mi_multi_plan_* twins.  Torque rows inside the speed
 * profile and the torques of the re-timed row: "re-timing under torque limits" below. */
typedef struct gpmp2mi_dynamics gpmp2mi_dynamics;   /* device-resident inertial table, bound to the robot's kinematics */
typedef struct gpmp2mi_dynamics_desc {
  const double* mass;     /* [L]     kg, >= 0                                             */
  const double* com;      /* [L][3]  centre of mass in the link frame                     */
  const double* inertia;  /* [L][6]  ixx iyy izz ixy ixz iyz about the COM, link frame    */
  double gravity[3];      /* world frame; default (0, 0, -9.81)                           */
  const double* torque;   /* [dof] limits, > 0, +inf: none; NULL: none at all             */
} gpmp2mi_dynamics_desc;
void gpmp2mi_dynamics_desc_default(gpmp2mi_dynamics_desc* desc);
int gpmp2mi_dynamics_create(const gpmp2mi_robot* robot, const gpmp2mi_dynamics_desc* desc, gpmp2mi_dynamics** out);
void gpmp2mi_dynamics_destroy(gpmp2mi_dynamics* dynamics);   /* NULL: no-op */

/* caller buffers; traj [B][total_step+1][2D].  The device of the two handles must be current.  Any output may be NULL. */
int gpmp2mi_torque_score_traj(const gpmp2mi_robot* robot, const gpmp2mi_dynamics* dynamics, double delta_t,
                              int inter_step, int B, int total_step, const double* traj, double* torque_ratio,
                              double* static_ratio, double* torque_time_scale, int* worst, int* invalid, double* tau);
int gpmp2mi_torque_score_traj_dev(const gpmp2mi_robot* robot, const gpmp2mi_dynamics* dynamics, double delta_t,
                                  int inter_step, int B, int total_step, const double* traj, double* torque_ratio,
                                  double* static_ratio, double* torque_time_scale, int* worst, int* invalid, double* tau,
                                  void* stream);
/* The plan's resident result; preconditions and errors as gpmp2mi_plan_score. */
int gpmp2mi_plan_torque_score(gpmp2mi_plan* p, const gpmp2mi_dynamics* dynamics, int inter_step, double* torque_ratio,
                              double* static_ratio, double* torque_time_scale, int* worst, int* invalid, double* tau);
int gpmp2mi_plan_torque_score_dev(gpmp2mi_plan* p, const gpmp2mi_dynamics* dynamics, int inter_step,
                                  double* torque_ratio, double* static_ratio, double* torque_time_scale, int* worst,
                                  int* invalid, double* tau, void* stream);
/* gpmp2mi_plan_select_feasible with the torque rule, one enqueue: the existing score stages, the motion scores, the
 * torques, then one finish that reads them all.  Outputs as gpmp2mi_plan_select_feasible, plus tau_best. */
int gpmp2mi_plan_select_dynamic(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                const gpmp2mi_self_pairs* pairs /*NULL ok*/, double required_self_clearance,
                                const gpmp2mi_motion_limits* limits, double required_pos_margin, double max_time_scale,
                                const gpmp2mi_dynamics* dynamics, int* best, int* n_eligible, double* time_scale_best,
                                double* tau_best, double* traj_best, double* dense_best);
int gpmp2mi_plan_select_dynamic_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                    const gpmp2mi_self_pairs* pairs /*NULL ok*/, double required_self_clearance,
                                    const gpmp2mi_motion_limits* limits, double required_pos_margin,
                                    double max_time_scale, const gpmp2mi_dynamics* dynamics, int* best,
                                    int* n_eligible, double* time_scale_best, double* tau_best, double* traj_best,
                                    double* dense_best, void* stream);

/* ---- re-timing under torque limits: a speed profile that the drives can follow, on the device ------------------------
 * gpmp2mi_plan_retime knows the drives by a per-joint acceleration box, and gpmp2mi_plan_torque_score can only answer with
 * one uniform stretch of the whole row: one demanding stage slows the whole trajectory.  These calls find the fastest speed
 * profile along the unchanged path under the joint torque limits of a gpmp2mi_dynamics handle, with gravity taken off each
 * limit state by state, next to the speed, acceleration and Cartesian-speed limits of "re-timing", which stay in force.
 * They give the feed-forward torques of the re-timed row, and a selection that asks for the re-timed duration.
 *
 * Along a fixed path, with x = sdot^2 and u = sddot, the torque is affine: tau = p u + m x + tau_g, with p = M(q) q' (the
 * inverse dynamics of (q, 0, q') without gravity), m = ID(q, q', q'') without gravity and tau_g = ID(q, 0, 0), all of
 * "torque limits".  The rule is that of "re-timing" with rows that carry an offset (csrc/retime_affine_rule.h states it
 * for host and device; every operation is rounded once in the order written):
 *  - The row |cx x + cu u + off| <= A, with lo = -A - off and hi = A - off: A = +inf bounds nothing; cu > 0 gives
 *    lo/cu - (cx/cu) x <= u <= hi/cu - (cx/cu) x; cu < 0 gives hi/cu - (cx/cu) x <= u <= lo/cu - (cx/cu) x; cu == 0 bounds
 *    no u and caps x at hi/cx for cx > 0, at lo/cx for cx < 0.  With off == 0 this is the two-sided row of "re-timing", bit
 *    for bit.
 *  - Rows of stage k, for every affine constraint r with a finite bound: at the start of the stage
 *    (cx, cu, off) = (cx_right_k, cu_k, off_k); at its end (cx_left_{k+1}, cu_{k+1} + 2 h cx_left_{k+1}, off_{k+1}), the
 *    constraint at state k+1 seen from the left, written in (x_k, u_k).  For the torque of joint d:
 *    (m_{k+}[d], p_k[d], tau_g,k[d]) and (m_{(k+1)-}[d], p_{k+1}[d] + 2 h m_{(k+1)-}[d], tau_g,k+1[d]) against L_d.  They
 *    join the 2 D acceleration rows and the row of the next set: n = 2 D + 2 R + 1 rows per stage, R <= 8.
 *  - Backward pass, forward pass, time and the statuses of "re-timing" are unchanged.  GPMP2MI_RETIME_INVALID also for a
 *    non-finite cx, cu or off of a constraint with a finite bound (cx_left of state 0 and cx_right of state Md-1 are not
 *    read; a constraint without a bound is not looked at).  GPMP2MI_RETIME_STATIC: some constraint with a finite bound
 *    has |off| >= bound at a checked state (gravity alone takes the limit: static_ratio >= 1 of "torque limits"); no
 *    timing helps.  It is tested after INVALID and before everything else.  With |off| < bound everywhere x = 0, u = 0
 *    meets every affine row, and GPMP2MI_RETIME_EMPTY keeps its meaning.
 *  - achieved [B][6]: [0..3] as "re-timing"; [4] the largest |cx x_k + cu u_k + off| / bound over the start and end rows
 *    of every stage (the torque ratio of the re-timed row at the checked states), <= 1 up to rounding; [5] the largest
 *    |off| / bound over the states (static_ratio).  NaN in a row that is not OK.
 *  - coef [B][Md][4][dof] = p, m_left, m_right, tau_g of every checked state; a state with one side carries that side
 *    twice.  Where q'_k == 0 exactly, p_k == 0 exactly, and where q'' == 0 as well, m == 0: a state at rest gives rows that
 *    cap x, not rows with a rounding-level cu.
 *  - tau_retimed [B][Md][dof] = m_{k+} x_k + p_k u_k + tau_g,k, the torques the re-timed row asks for at its checked
 *    states; the last state uses m_- and u_{Md-2}.  NaN in a row that is not OK.
 *  - With R == 0, or with every bound (every torque limit) +inf, sdot, u, stamps, duration, status, achieved[0..3] and
 *    dense_retimed have the bits of gpmp2mi_retime_path / gpmp2mi_retime_traj.
 *  - Determinism as for "re-timing": a row's outputs are bit-identical alone, in any batch and through every entry point.
 *  - Selection (gpmp2mi_plan_select_retimed_dynamic): the rule of gpmp2mi_plan_select_retimed on the profile of these
 *    calls, and no coefficient of the row that is not finite (whether its joint has a limit or not).  Outputs as
 *    gpmp2mi_plan_select_retimed, plus tau_best [Md][dof], the chosen row of tau_retimed (untouched when none is chosen).
 * Re-timing changes WHEN the robot is where: the moving-obstacle and workspace-path checks of a row, which index their
 * spheres and targets by planned time, are not valid for the re-timed row.
 * Errors, before any device work: those of "re-timing" and of "torque limits" (a dynamics handle made for another robot or
 * living on another device; GPMP2MI_ERR_UNSUPPORTED for any kind but GPMP2MI_ROBOT_ARM and for more than 8 joints);
 * GPMP2MI_ERR_INVALID for R outside 0..8, a NULL array of the R > 0 constraints, or a bound that is NaN or <= 0.  A
 * refused call writes nothing.
 * Memory: beyond the seven doubles per checked state of "re-timing", 4 D for the coefficients (room for them is kept
 * whoever asks: the chain reads them), 4 (2 D + 2 R) for the rows of the stages, which are formed ahead of the chain,
 * and D for the torques, with the dynamics handle for gpmp2mi_retime_dynamic_traj_dev (under the stream-order rule of
 * gpmp2mi_score_traj_dev), with the plan for the plan forms, taken at the first call and grown on demand.
 * gpmp2mi_retime_path_affine_dev has no handle: the caller gives `workspace`, B Md (3 + 4 (2 dof + 2 R)) doubles on the
 * device, and none of its sdot / u / stamps may be NULL.  Any other output may be NULL.  The `_dev` forms enqueue and
 * return.
 * Not here: torque rows between checked states (SAMPLED, NOT BOUNDED, as in "torque limits": raise inter_step), jerk
 * limits, the Pose2 and the mobile kinds, gpmp2mi_multi_plan_* twins. */
/* The bare rule: the arguments of gpmp2mi_retime_path, and R constraints per state cx_left, cx_right, cu, off
 * [B][Md][R] with bound HOST [R] (> 0, +inf: none); NULL arrays are fine for R == 0.  achieved [B][6]. */
int gpmp2mi_retime_path_affine(int B, int Md, int dof, const double* qd, const double* qdd_left, const double* qdd_right,
                               const double* cap, const double* acc, int R, const double* cx_left,
                               const double* cx_right, const double* cu, const double* off, const double* bound, double h,
                               double max_rate, double rate_start, double rate_end, double* sdot, double* u,
                               double* stamps, double* duration, int* status, double* achieved);
int gpmp2mi_retime_path_affine_dev(int B, int Md, int dof, const double* qd, const double* qdd_left,
                                   const double* qdd_right, const double* cap, const double* acc, int R,
                                   const double* cx_left, const double* cx_right, const double* cu, const double* off,
                                   const double* bound, double h, double max_rate, double rate_start, double rate_end,
                                   double* sdot, double* u, double* stamps, double* duration, int* status,
                                   double* achieved, double* workspace, void* stream);
/* caller buffers; traj [B][total_step+1][2D].  The device of the two handles must be current.  Any output may be NULL. */
int gpmp2mi_retime_dynamic_traj(const gpmp2mi_robot* robot, const gpmp2mi_dynamics* dynamics,
                                const gpmp2mi_motion_limits* limits, double delta_t, int inter_step, int B,
                                int total_step, const double* traj, double max_rate, double rate_start, double rate_end,
                                double* sdot, double* u, double* stamps, double* duration, int* status, double* achieved,
                                double* dense_retimed, double* tau_retimed, double* coef);
int gpmp2mi_retime_dynamic_traj_dev(const gpmp2mi_robot* robot, const gpmp2mi_dynamics* dynamics,
                                    const gpmp2mi_motion_limits* limits, double delta_t, int inter_step, int B,
                                    int total_step, const double* traj, double max_rate, double rate_start,
                                    double rate_end, double* sdot, double* u, double* stamps, double* duration,
                                    int* status, double* achieved, double* dense_retimed, double* tau_retimed,
                                    double* coef, void* stream);
/* The plan's resident result; preconditions and errors as gpmp2mi_plan_score. */
int gpmp2mi_plan_retime_dynamic(gpmp2mi_plan* p, const gpmp2mi_dynamics* dynamics, const gpmp2mi_motion_limits* limits,
                                int inter_step, double max_rate, double rate_start, double rate_end, double* sdot,
                                double* u, double* stamps, double* duration, int* status, double* achieved,
                                double* dense_retimed, double* tau_retimed, double* coef);
int gpmp2mi_plan_retime_dynamic_dev(gpmp2mi_plan* p, const gpmp2mi_dynamics* dynamics,
                                    const gpmp2mi_motion_limits* limits, int inter_step, double max_rate,
                                    double rate_start, double rate_end, double* sdot, double* u, double* stamps,
                                    double* duration, int* status, double* achieved, double* dense_retimed,
                                    double* tau_retimed, double* coef, void* stream);
/* gpmp2mi_plan_select_retimed with the torque rows in the profile, one enqueue. */
int gpmp2mi_plan_select_retimed_dynamic(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                        const gpmp2mi_self_pairs* pairs /*NULL ok*/, double required_self_clearance,
                                        const gpmp2mi_motion_limits* limits, double required_pos_margin, double max_rate,
                                        double rate_start, double rate_end, double max_duration,
                                        const gpmp2mi_dynamics* dynamics, int* best, int* n_eligible,
                                        double* duration_best, double* stamps_best, double* tau_best, double* traj_best,
                                        double* dense_best);
int gpmp2mi_plan_select_retimed_dynamic_dev(gpmp2mi_plan* p, int inter_step, double required_clearance,
                                            int require_in_range, const gpmp2mi_self_pairs* pairs /*NULL ok*/,
                                            double required_self_clearance, const gpmp2mi_motion_limits* limits,
                                            double required_pos_margin, double max_rate, double rate_start,
                                            double rate_end, double max_duration, const gpmp2mi_dynamics* dynamics,
                                            int* best, int* n_eligible, double* duration_best, double* stamps_best,
                                            double* tau_best, double* traj_best, double* dense_best, void* stream);

/* ---- moving obstacles: time-indexed spheres as a plan factor and a check, on the device ---------------------------
 * Every obstacle of "scoring" lives in one static signed-distance field.  A person or another robot crossing the
 * workspace is a set of K spheres whose centres are indexed by the support time: radius [K], centers [K][N+1][3],
 * sphere k at centers[k][i] at support state i.  One set per plan, shared by its B trajectories.  A plan created with
 * gpmp2mi_graph_opts::max_moving_spheres > 0 reserves room for that many spheres (all device memory is taken at
 * gpmp2mi_plan_create), carries the factor below on the support states moving_first..moving_last, and takes its data
 * from gpmp2mi_plan_set_moving_spheres, which may be repeated every control cycle.
 *
 * Definitions, for robot sphere s (all S spheres, ids in the order of the robot description) and moving sphere k:
 *  - total_eps(s, k) = (radius_s + radius_k) + epsilon, evaluated in that order in fp64.
 *  - The factor, at support state i in [moving_first, moving_last]: dist = |c_s(q_i) - centers[k][i]|;
 *    err = dist > total_eps ? 0 : total_eps - dist (the strictness of obstacle/SelfCollision.h:114-127); the Jacobian row
 *    is -n^T J_s when active and zero otherwise, n = (c_s - o_k) / dist, J_s the sphereCenters Jacobian as
 *    gpmp2mi_sphere_centers returns it (the Pose2 chart for the mobile kinds).  dist == 0: err = total_eps, a zero
 *    row, no NaN.  Noise: isotropic moving_sigma.  In a plan the S K rows of a state are never stored: one kernel adds
 *    sum w h h^T, sum w h r and sum w r^2 (w = 1 / sigma^2) to the record of the state's unary point, in pair order
 *    (s, k) ascending, so a state's contribution is the same bits alone, in any batch and on any run.  Every call that
 *    linearizes a plan carries the factor: optimize, the queue runs, plan_update, plan_linearize, plan_graph_error;
 *    Gauss-Newton, LM and Dogleg; narrow, wide and dense blocks.  With K == 0 nothing is launched for it.
 *  - The check: the checked states of "scoring" (Md = N (J+1) + 1).  At checked state i (J+1) + j sphere k is at
 *    o_i + tau (o_{i+1} - o_i), tau = j / (J+1), evaluated in that form; support states use o_i itself.
 *    clearance(m, s, k) = dist - total_eps; a pair whose dist is not finite is invalid: it enters no sum and no minimum,
 *    and it is counted.  moving_support_cost [B] / moving_dense_cost [B]: the unwhitened hinge sums over the support /
 *    all checked states.  min_moving_clearance [B]: the minimum over the valid (m, s, k), +inf if there is none (K = 0).
 *    worst [B][3]: the (checked state, robot sphere, moving sphere) attaining it; on exact ties the lowest state, then
 *    the lowest sphere, then the lowest moving sphere; (-1, -1, -1) if none.  invalid [B].  Any output may be NULL.
 *  - Determinism as in "self-collision check": sums are taken in an order fixed by (N, J, S, K), without floating-point
 *    atomics; a row scores the same bits alone, in any batch, through the trajectory form or the plan form.
 *  - Selection: the rule of gpmp2mi_plan_select (of gpmp2mi_plan_select_checked when pairs != NULL) with one more
 *    condition,
 *      eligible(b) = <that rule> && moving_invalid[b] == 0 && min_moving_clearance[b] >= required_moving_clearance;
 *    ranking and ties unchanged.  With K == 0 and required_moving_clearance = -inf it answers what the existing call does.
 * Errors: GPMP2MI_ERR_INVALID (checked before any device work) for a NULL plan / robot / traj, K < 0, K above the
 * capacity (the plan forms) or above GPMP2MI_MAX_MOVING_SPHERES (the others), a NULL radius / centers with K > 0, a NaN
 * epsilon, the argument errors of "scoring"; the plan forms of the check also for a plan created without capacity, and
 * with the preconditions of gpmp2mi_plan_score.  GPMP2MI_ERR_TIMEOUT for a poisoned plan.
 * Memory: the workspace rules of "scoring"; the records (one 40-byte record per tile of "self-collision check") are kept
 * with the plan, and by gpmp2mi_moving_score_traj_dev with the robot handle.
 * Not here: gpmp2mi_multi_plan_* twins, C++ facade classes, the factor at GP-interpolated sub-steps (the dense check is
 * what looks between support states), per-trajectory sphere sets, moving spheres in the risk / collision-probability
 * calls, shapes other than spheres. */

/* The plan's sphere set.  Valid at any time between solves; K = 0 clears the set; a fresh plan holds K = 0.  Host form:
 * the data is copied before the call returns, and a non-finite centre or a negative / non-finite radius is refused.
 * _dev: device pointers, the copies are enqueued on `stream`, the values are not inspected.  A refused call changes
 * nothing. */
int gpmp2mi_plan_set_moving_spheres(gpmp2mi_plan* p, int K, const double* radius /*[K]*/,
                                    const double* centers /*[K][N+1][3]*/);
int gpmp2mi_plan_set_moving_spheres_dev(gpmp2mi_plan* p, int K, const double* radius, const double* centers,
                                        void* stream);
/* The factor, batched over M evaluations with one centre set per evaluation: conf [M][D], centers [M][K][3] ->
 * err [M][S][K] (unwhitened), H [M][S][K][D] (NULL ok). */
int gpmp2mi_moving_sphere_factor(const gpmp2mi_robot* r, int K, const double* radius, double epsilon, int M,
                                 const double* conf, const double* centers, double* err, double* H);
/* The check for caller buffers; traj [B][total_step+1][2D], centers [K][total_step+1][3].  The device of the robot
 * handle must be current. */
int gpmp2mi_moving_score_traj(const gpmp2mi_robot* robot, int K, const double* radius, const double* centers,
                              double epsilon, double delta_t, int inter_step, int B, int total_step, const double* traj,
                              double* moving_support_cost, double* moving_dense_cost, double* min_moving_clearance,
                              int* worst, int* invalid);
int gpmp2mi_moving_score_traj_dev(const gpmp2mi_robot* robot, int K, const double* radius, const double* centers,
                                  double epsilon, double delta_t, int inter_step, int B, int total_step,
                                  const double* traj, double* moving_support_cost, double* moving_dense_cost,
                                  double* min_moving_clearance, int* worst, int* invalid, void* stream);
/* The plan's resident result against the plan's resident set, with its moving_epsilon and delta_t. */
int gpmp2mi_plan_moving_score(gpmp2mi_plan* p, int inter_step, double* moving_support_cost, double* moving_dense_cost,
                              double* min_moving_clearance, int* worst, int* invalid);
int gpmp2mi_plan_moving_score_dev(gpmp2mi_plan* p, int inter_step, double* moving_support_cost,
                                  double* moving_dense_cost, double* min_moving_clearance, int* worst, int* invalid,
                                  void* stream);
/* One enqueue: the existing score stages, the moving scores, then one finish that reads them all.  Outputs as
 * gpmp2mi_plan_select. */
int gpmp2mi_plan_select_moving(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                               const gpmp2mi_self_pairs* pairs /*NULL ok*/, double required_self_clearance,
                               double required_moving_clearance, int* best, int* n_eligible, double* traj_best,
                               double* dense_best);
int gpmp2mi_plan_select_moving_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                   const gpmp2mi_self_pairs* pairs /*NULL ok*/, double required_self_clearance,
                                   double required_moving_clearance, int* best, int* n_eligible, double* traj_best,
                                   double* dense_best, void* stream);

/* ---- carried object: spheres rigidly attached to one link as a plan factor and a check, on the device --------------
 * The robot's collision geometry is the sphere table of the robot handle, fixed when the handle is made.  What the robot
 * holds after a grasp is a set of A spheres rigidly attached to one link: radius [A], centers [A][3] in the frame of
 * link `link`.  One set per plan, shared by its B trajectories; it is replaced or cleared between solves without
 * touching the plan (grasp, release, regrasp on another link).  A plan created with
 * gpmp2mi_graph_opts::max_carried_spheres > 0 reserves room for that many spheres (all device memory is taken at
 * gpmp2mi_plan_create), carries the factor below on the support states carried_first..carried_last, and takes its data
 * from gpmp2mi_plan_set_carried.  The spheres are extra body spheres of ObstacleSDFFactor<ROBOT>
 * (gpmp2/obstacle/ObstacleSDFFactor-inl.h:18-56, kinematics/RobotModel-inl.h:12-40) with their own epsilon and sigma.
 *
 * Definitions, for carried sphere a (radius r_a, centre o_a in the frame of link l) and configuration q:
 *  - Centre: c_a(q) = T_l(q) o_a, T_l the frame gpmp2mi_forward_kinematics returns for link l.  In a planar field the
 *    first two coordinates are used, as for body spheres.
 *  - Derivative: d c_a / d q_k = R_l (v_k + omega_k x o_a), [omega_k; v_k] column k of the link's body Jacobian as
 *    gpmp2mi_forward_kinematics returns it (the Pose2 chart for the mobile kinds).
 *  - The factor, at support state i in [carried_first, carried_last]: d and grad d are the field's value and gradient
 *    at c_a.  If c_a is inside the field and !(d > r_a + carried_epsilon): err = (r_a + carried_epsilon) - d and the
 *    Jacobian row is -grad d^T d c_a / d q; otherwise err = 0 with a zero row (what obstacle/ObstacleCost.h:31-38 does
 *    for a query out of range).  Noise: isotropic carried_sigma.  The terms go to the configuration block of the
 *    state's unary record only.  In a plan the A rows of a state are never stored: one kernel adds sum w h h^T,
 *    sum w h r and sum w r^2 (w = 1 / sigma^2) to the record, in sphere order, so a state's contribution is the same
 *    bits alone, in any batch and on any run.  Every call that linearizes a plan carries the factor: optimize, the
 *    queue runs, plan_update, plan_linearize, plan_graph_error; Gauss-Newton, LM and Dogleg; narrow, wide and dense
 *    blocks.  With A == 0 nothing is launched for it.
 *  - Range test before any lookup: inside means x >= origin && x <= upper on every axis of the field, written as that
 *    conjunction, so a NaN centre fails it, counts as out of range and is never turned into a cell index.  The _dev
 *    setters take unvalidated device data; this test is what keeps a bad centre from becoming a wild read.
 *  - The check: the checked states of "scoring" (Md = N (J+1) + 1), with epsilon 0 as there.
 *    carried_support_cost [B] / carried_dense_cost [B]: the sums of max(0, r_a - d) over the support / all checked
 *    states.  min_carried_clearance [B]: the minimum of d - r_a over the in-range (state, sphere), +inf if there is none
 *    (or A = 0).  worst [B][2]: the (checked state, carried sphere) attaining it; on exact ties the lowest state, then
 *    the lowest sphere; (-1, -1) if none.  out_of_range [B].  Any output may be NULL.
 *  - Determinism as in "moving obstacles": an inactive sphere adds an exact zero; active rows are added in ascending
 *    sphere order into one accumulator per record entry, without atomics; a row's check outputs are a function of the
 *    row, the handles, the set, delta_t and inter_step alone.
 *  - Selection: the rule of gpmp2mi_plan_select (of gpmp2mi_plan_select_checked when pairs != NULL) with two more
 *    conditions,
 *      eligible(b) = <that rule> && (!require_in_range || carried_out_of_range[b] == 0)
 *                    && min_carried_clearance[b] >= required_carried_clearance;
 *    ranking and ties unchanged.  With A == 0 and required_carried_clearance = -inf it answers what the existing call
 *    does.
 * Errors: GPMP2MI_ERR_INVALID (checked before any device work) for a NULL plan or handle, a link outside 0..L-1, A < 0,
 * A above the capacity (the plan forms) or above GPMP2MI_MAX_CARRIED_SPHERES (the others), NULL arrays with A > 0, a
 * radius that is NaN or negative and a non-finite centre (host forms), carried_sigma <= 0 or a non-finite epsilon when
 * there is capacity, a bad state range, the argument errors of "scoring"; the plan forms of the check also for a plan
 * created without capacity, and with the preconditions of gpmp2mi_plan_score.  GPMP2MI_ERR_TIMEOUT for a poisoned plan.
 * A refused call writes nothing and leaves the resident set in place.
 * Memory: the workspace rules of "scoring"; the records (one 40-byte record per tile of 64 checked states) are kept
 * with the plan, and by gpmp2mi_carried_score_traj_dev with the robot handle.
 * Not here: the factor at GP-interpolated sub-states (the dense check is what looks between support states, as for the
 * self-collision table); carried spheres against the robot's own spheres, the moving spheres, the posterior-risk and
 * collision-probability calls and the live map's self-filter; more than one link per set, per-trajectory sets;
 * gpmp2mi_multi_plan_* setters (shards pass the capacity through and hold an empty set); C++ facade classes. */

/* The plan's carried set.  Valid at any time between solves; A = 0 clears the set; a fresh plan holds A = 0.  Host form:
 * the data is copied before the call returns.  _dev: device pointers, the copies are enqueued on `stream`, the values
 * are not inspected.  A set call is two copies and two host values (link, A).  A refused call changes nothing. */
int gpmp2mi_plan_set_carried(gpmp2mi_plan* p, int link, int A, const double* radius /*[A]*/,
                             const double* centers /*[A][3]*/);
int gpmp2mi_plan_set_carried_dev(gpmp2mi_plan* p, int link, int A, const double* radius, const double* centers,
                                 void* stream);
/* the size of the resident set; -1 for a NULL plan */
int gpmp2mi_plan_carried_count(const gpmp2mi_plan* p);
/* The factor, batched over M evaluations: conf [M][D] -> err [M][A] (unwhitened), H [M][A][D] (NULL ok). */
int gpmp2mi_carried_sphere_factor(const gpmp2mi_robot* r, const gpmp2mi_sdf* sdf, int link, int A, const double* radius,
                                  const double* centers, double epsilon, int M, const double* conf, double* err,
                                  double* H);
/* The check for caller buffers; traj [B][total_step+1][2D].  The device of the robot handle must be current. */
int gpmp2mi_carried_score_traj(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, int link, int A, const double* radius,
                               const double* centers, double delta_t, int inter_step, int B, int total_step,
                               const double* traj, double* carried_support_cost, double* carried_dense_cost,
                               double* min_carried_clearance, int* worst, int* out_of_range);
int gpmp2mi_carried_score_traj_dev(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, int link, int A,
                                   const double* radius, const double* centers, double delta_t, int inter_step, int B,
                                   int total_step, const double* traj, double* carried_support_cost,
                                   double* carried_dense_cost, double* min_carried_clearance, int* worst,
                                   int* out_of_range, void* stream);
/* The plan's resident result against the plan's resident set, with its field and delta_t. */
int gpmp2mi_plan_carried_score(gpmp2mi_plan* p, int inter_step, double* carried_support_cost, double* carried_dense_cost,
                               double* min_carried_clearance, int* worst, int* out_of_range);
int gpmp2mi_plan_carried_score_dev(gpmp2mi_plan* p, int inter_step, double* carried_support_cost,
                                   double* carried_dense_cost, double* min_carried_clearance, int* worst,
                                   int* out_of_range, void* stream);
/* One enqueue: the existing score stages, the carried scores, then one finish that reads them all.  Outputs as
 * gpmp2mi_plan_select. */
int gpmp2mi_plan_select_carried(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                const gpmp2mi_self_pairs* pairs /*NULL ok*/, double required_self_clearance,
                                double required_carried_clearance, int* best, int* n_eligible, double* traj_best,
                                double* dense_best);
int gpmp2mi_plan_select_carried_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                    const gpmp2mi_self_pairs* pairs /*NULL ok*/, double required_self_clearance,
                                    double required_carried_clearance, int* best, int* n_eligible, double* traj_best,
                                    double* dense_best, void* stream);

/* ---- self-collision table in a plan: a pair table of any size as a plan factor, on the device ----------------------
 * The self-collision rows of gpmp2mi_graph_opts hold at most GPMP2MI_MAX_SELF_COLLISION_PAIRS pairs, while the check of
 * "self-collision check" works with the full table.  A plan created with gpmp2mi_graph_opts::max_self_pairs > 0
 * reserves room for that many pair records (all device memory is taken at gpmp2mi_plan_create: the records, and the
 * sphere centres and their Jacobians if no other extra factor has them yet), carries the factor below on the support
 * states self_pairs_first..self_pairs_last, and takes its table from gpmp2mi_plan_set_self_pairs, which may be
 * repeated between solves.  One table per plan, shared by its B trajectories.
 *
 * Definitions, for row p = (A, B, epsilon_p, sigma_p) of the table (sphere ids in the order of the robot description):
 *  - total_eps_p = radius_A + radius_B + epsilon_p, formed on the host in that order in fp64.
 *  - The factor, at support state i in [self_pairs_first, self_pairs_last]: dist = |c_A(q_i) - c_B(q_i)|;
 *    err = dist > total_eps_p ? 0 : total_eps_p - dist (obstacle/SelfCollision.h:66-128; a NaN distance keeps the hinge
 *    on); the Jacobian row is -n^T (J_A - J_B) when active and zero otherwise, n = (c_A - c_B) / dist, J the
 *    sphereCenters Jacobian as gpmp2mi_sphere_centers returns it (the Pose2 chart for the mobile kinds).  dist == 0:
 *    err = total_eps_p, a zero row, no NaN -- the rule of "moving obstacles"; the n_self_collision rows of
 *    gpmp2mi_graph_opts and gpmp2mi_self_collision_factor divide by the distance and make a NaN row there.
 *    Weight w_p = 1 / sigma_p^2 (column 3 of the table, which the check does not read, is read here).  The P rows of a
 *    state are never stored: one kernel adds sum w h h^T, sum w h r and sum w r^2 to the record of the state's unary
 *    point, in table order, so a state's contribution is the same bits alone, in any batch and on any run.  A chunk of
 *    64 rows without an active one is skipped; it would add exact zeros.  Every call that linearizes a plan carries
 *    the factor: optimize, the queue runs (seeded ones included), plan_update, plan_linearize, plan_graph_error;
 *    Gauss-Newton (without the early stop, as for the other extra factors), LM and Dogleg; narrow, wide and dense
 *    blocks.  With an empty table nothing is launched for it.
 *  - The two routes are independent: a plan may carry n_self_collision rows and a table; a pair in both is two factors.
 * The factor on M evaluations is gpmp2mi_self_collision_factor, which takes any n_pairs.
 * Errors: GPMP2MI_ERR_INVALID at gpmp2mi_plan_create for max_self_pairs < 0 or above GPMP2MI_MAX_PLAN_SELF_PAIRS, and
 * with a capacity for a range outside 0..N or first > last.  The setter refuses with GPMP2MI_ERR_INVALID, before any
 * device work and changing nothing: a NULL plan, a plan created without capacity, more rows than the capacity, a table
 * made for another robot (sphere count / dof / kind), an epsilon that is not finite, a sigma that is not finite or
 * <= 0.  GPMP2MI_ERR_TIMEOUT for a poisoned plan.
 * gpmp2mi_multi_plan_create with a capacity creates shards that hold an empty table.
 * Not here: the factor at GP-interpolated sub-states (the dense check is what looks between support states),
 * gpmp2mi_multi_plan_* setters, C++ facade classes, per-trajectory tables, a self-collision term in the risk /
 * collision-probability calls. */

/* The plan's table.  Valid at any time between solves; NULL or an empty table clears it; a fresh plan holds none.  The
 * plan keeps its own copy of the records (made before the call returns): the handle may be destroyed at once.  A later
 * solve on any stream the plan uses sees the new table.  A refused call changes nothing. */
int gpmp2mi_plan_set_self_pairs(gpmp2mi_plan* p, const gpmp2mi_self_pairs* pairs);
int gpmp2mi_plan_self_pairs_count(const gpmp2mi_plan* p);   /* rows resident in the plan; -1 for NULL */

/* ---- workspace path: time-indexed end-effector targets as a plan factor and a check, on the device ----------------
 * The workspace factors of gpmp2mi_graph_opts hold one constant des_pose over a range of states.  A workspace path is
 * one target pose and one sigma per support state: des [N+1][16] (row-major 4x4) and sigma [N+1], for one link and one
 * mode, shared by the plan's B trajectories and replaceable between solves.  A plan created with
 * gpmp2mi_graph_opts::workspace_path = 1 takes the memory of the path at gpmp2mi_plan_create (2 (N+1) words of list,
 * 17 (N+1) doubles; no link poses, pose Jacobians or rows), carries the factor below on the constrained states and
 * takes its data from gpmp2mi_plan_set_workspace_path, which may be repeated every control cycle.
 *
 * Definitions:
 *  - State i is constrained if sigma[i] is finite (and > 0); sigma[i] = +inf: the state carries no factor, it is
 *    skipped and its record is not touched.
 *  - The factor, at constrained state i: the rows of gpmp2mi_workspace_prior_factor(robot, workspace_path_mode,
 *    workspace_path_link, des[i], q_i) (GaussianPriorWorkspace{Position,Orientation,Pose}; 3 rows, 6 for the POSE mode),
 *    isotropic noise sigma[i].  In a plan the rows are never stored: one kernel (one wavefront per trajectory and
 *    constrained state) adds sum w h h^T, sum w h r and sum w r^2 (w = 1 / sigma_i^2, rows ascending) to the record of
 *    the state's unary point, after the moving-sphere factor on the same stream.  A state's contribution is a function
 *    of (D, mode, link) and its own data: the same bits alone, in any batch and on any run; no floating-point atomics.
 *    Every call that linearizes a plan carries it: optimize, the queue runs, plan_update, plan_linearize,
 *    plan_graph_error; Gauss-Newton, LM and Dogleg; trial points; narrow, wide and dense blocks.  With no constrained
 *    state nothing is launched for it.
 *  - Robot kinds: every kind gpmp2mi_workspace_prior_factor answers for, which is every kind of gpmp2mi_robot_kind in
 *    the instantiated (kind, dof) table, with its chart (the Pose2 chart for the mobile kinds).  A robot outside the
 *    table is refused at plan creation with GPMP2MI_ERR_UNSUPPORTED.
 *  - The check: the checked states of "scoring" (Md = N (J+1) + 1).  At checked state i (J+1) + j, tau = j / (J+1), the
 *    target position is t_i + tau (t_{i+1} - t_i), evaluated in that form, the target rotation
 *    R_i Exp(tau Log(R_i^T R_{i+1})) (Log: SO3::Logmap as the factor uses it; Exp: Rodrigues' formula, and for
 *    theta^2 <= 2.22e-16 the first-order I + [w]x), sigma = sigma_i + tau (sigma_{i+1} - sigma_i); support states use
 *    des[i] and sigma[i] themselves.  A support state is checked if sigma_i is finite, a sub-step if both ends are.
 *    pos_dev = |t(q) - t_target|, rot_dev = |Log(R_target^T R(q))| in radians; only the deviations the mode constrains
 *    are computed, the other output is 0.  r is the factor's residual against the target of the checked state (for the
 *    POSE mode the Pose3 logarithm, 6 numbers).  Outputs, any of which may be NULL: max_pos_dev [B], max_rot_dev [B]
 *    (0 if nothing is checked); worst [B][2]: the checked states attaining them, the lowest state on exact ties, -1 if
 *    nothing is checked (or the mode does not constrain that deviation); support_cost [B] / dense_cost [B]: the sum of
 *    |r|^2 / sigma^2 over the support / all checked states; invalid [B]: the checked states with a non-finite
 *    deviation, which enter no sum and no maximum.  Sums are taken in an order fixed by (N, J), without atomics: a row
 *    scores the same bits alone, in any batch, through the trajectory form or the plan form.
 *  - Selection: the rule of gpmp2mi_plan_select with one more condition,
 *      eligible(b) = <that rule> && invalid[b] == 0 && max_pos_dev[b] <= max_pos_dev_allowed
 *                    && max_rot_dev[b] <= max_rot_dev_allowed;
 *    ranking and ties unchanged.  With no path and +inf allowances it answers what gpmp2mi_plan_select answers.
 * Errors: GPMP2MI_ERR_INVALID (checked before any device work) for a NULL plan / robot / traj / conf, a plan created
 * without workspace_path (the plan forms), an unknown mode or a link out of range (at plan creation and in the
 * robot-handle forms), a NULL sigma with a path, the argument errors of "scoring"; the plan forms of the check also with
 * the preconditions of gpmp2mi_plan_score.  GPMP2MI_ERR_TIMEOUT for a poisoned plan.
 * Memory: the workspace rules of "scoring"; the records (one 48-byte record per 64 checked states) are kept with the
 * plan, and by gpmp2mi_path_score_traj_dev with the robot handle.
 * Not here: gpmp2mi_multi_plan_* twins, C++ facade classes, the factor at GP-interpolated sub-steps (the dense check is
 * what looks between support states), a path per trajectory, anisotropic noise, the path condition combined with the
 * self / moving / motion selections, any change to the <= 4 workspace factors of gpmp2mi_graph_opts or their kernels. */

/* The plan's path.  Valid at any time between solves; des == NULL clears it; a fresh plan holds none.  Queue runs and
 * plan_update use the resident path.  Host form: the data is copied before the call returns; refused are a non-finite
 * pose entry, a rotation block with max |R^T R - I| > 1e-6, a sigma that is <= 0 or NaN and, for the ORIENTATION and
 * POSE modes, two consecutive constrained targets whose relative angle exceeds pi - 1e-3 (the check's interpolation is
 * undefined there).  _dev: device pointers, the copies and the list of constrained states are enqueued on `stream`, the
 * values are not inspected.  A refused call changes nothing. */
int gpmp2mi_plan_set_workspace_path(gpmp2mi_plan* p, const double* des /*[N+1][16]*/, const double* sigma /*[N+1]*/);
int gpmp2mi_plan_set_workspace_path_dev(gpmp2mi_plan* p, const double* des, const double* sigma, void* stream);
/* The factor, batched over M evaluations with one target per evaluation, by the device functions of the plan's kernel
 * (not by forward kinematics plus gpmp2mi_workspace_prior_factor's kernel): conf [M][D], des [M][16] -> err [M][rows]
 * (unwhitened), H [M][rows][D] (NULL ok); rows = 6 for GPMP2MI_WORKSPACE_POSE, else 3. */
int gpmp2mi_workspace_path_factor(const gpmp2mi_robot* r, int mode, int link, int M, const double* conf,
                                  const double* des, double* err, double* H);
/* The check for caller buffers; traj [B][total_step+1][2D], des [total_step+1][16], sigma [total_step+1].  The device
 * of the robot handle must be current. */
int gpmp2mi_path_score_traj(const gpmp2mi_robot* robot, int mode, int link, const double* des, const double* sigma,
                            double delta_t, int inter_step, int B, int total_step, const double* traj,
                            double* max_pos_dev, double* max_rot_dev, int* worst, double* support_cost,
                            double* dense_cost, int* invalid);
int gpmp2mi_path_score_traj_dev(const gpmp2mi_robot* robot, int mode, int link, const double* des, const double* sigma,
                                double delta_t, int inter_step, int B, int total_step, const double* traj,
                                double* max_pos_dev, double* max_rot_dev, int* worst, double* support_cost,
                                double* dense_cost, int* invalid, void* stream);
/* The plan's resident result against the plan's resident path (no path: nothing is checked). */
int gpmp2mi_plan_path_score(gpmp2mi_plan* p, int inter_step, double* max_pos_dev, double* max_rot_dev, int* worst,
                            double* support_cost, double* dense_cost, int* invalid);
int gpmp2mi_plan_path_score_dev(gpmp2mi_plan* p, int inter_step, double* max_pos_dev, double* max_rot_dev, int* worst,
                                double* support_cost, double* dense_cost, int* invalid, void* stream);
/* One enqueue: the obstacle score stage, the deviations, then one finish that reads both.  Outputs as
 * gpmp2mi_plan_select. */
int gpmp2mi_plan_select_path(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                             double max_pos_dev_allowed, double max_rot_dev_allowed, int* best, int* n_eligible,
                             double* traj_best, double* dense_best);
int gpmp2mi_plan_select_path_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                 double max_pos_dev_allowed, double max_rot_dev_allowed, int* best, int* n_eligible,
                                 double* traj_best, double* dense_best, void* stream);

/* ---- live map: a field handle updated in place from a field, an occupancy grid or a point cloud, on the device ------
 * A plan binds one field handle for life.  These calls rewrite the handle's voxels where they are, so the static map can
 * change between two solves without destroying the field and the plans on it.
 *
 * Definitions:
 *  - Geometry is fixed.  An update never changes dim, nx, ny, nz, the origin, the cell size or the addresses of the
 *    handle's device buffers.  Every plan created on the handle, and every call that takes the handle, sees the new
 *    voxels in the calls that follow the update in stream order.  Host forms run on the default stream and synchronise
 *    before they return; `_dev` forms enqueue on `stream` and return without a host synchronisation.  An update
 *    concurrent with a call that reads the field is the caller's error: use the same stream, or events.
 *  - gpmp2mi_sdf_update: the handle afterwards equals, bit for bit, one made by gpmp2mi_sdf_create with the same voxels,
 *    the plain voxels and the packed cells alike.  It clears the base (below).
 *  - gpmp2mi_sdf_update_from_occupancy: the handle afterwards equals one made by gpmp2mi_sdf_create_from_occupancy: cells
 *    with occ > 0.75 are obstacles, an empty or full grid gives the constant 1000.  It records the obstacle set as the
 *    handle's base, one byte per cell.  A handle that never took this call has no base; the constructors record none.
 *  - Point-to-cell rule.  Per axis a < dim, u = (p_a - origin_a) / cell_size + 0.5, evaluated in fp64 in exactly that
 *    form (a true division, not a multiplication by a reciprocal).  The point is in the grid iff u >= 0 && u < n_a on
 *    every axis, compared in double before any conversion to an integer; its cell index on the axis is floor(u).
 *  - Classification of a point; the first rule that matches applies:
 *      1. non-finite: a coordinate (of the first dim) is NaN or infinite;
 *      2. self: robot != NULL and, for some body sphere s, sqrt(dx^2 + dy^2 + dz^2) <= radius_s + margin, the centres
 *         being those of gpmp2mi_sphere_centers(robot, conf) (the same kernel: the same bits); dim == 2 uses x, y only;
 *      3. outside the grid;
 *      4. kept.
 *    stats = {kept, non-finite, self, outside}; the four counts sum to M.
 *  - Occupied set and field.  O = (use_base ? base : empty) united with the cells of the kept points.  The field written
 *    is, bit for bit, what the occupancy path gives for the indicator of O.  M == 0 is valid.  Nothing persists between
 *    calls except the base: the cloud of the previous call is gone.  The result is a function of the set of points, not
 *    of their order; no floating-point atomic is used.
 * Errors, all checked before any device work (a refused call changes nothing): GPMP2MI_ERR_INVALID for a NULL handle, a
 * NULL voxels / occ, NULL points with M > 0, M < 0, an unknown layout, a NaN margin, robot != NULL with a NULL conf,
 * use_base on a handle without a base, a robot on another device than the field, a field whose device is not the current
 * one; GPMP2MI_ERR_UNSUPPORTED for an axis too long for the distance transform (as the constructor); GPMP2MI_ERR_ALLOC
 * and GPMP2MI_ERR_HIP as elsewhere.
 * Memory: the workspace is two int32 volumes, the byte mask, [S][3] centres and four counters.  It is taken at the first
 * update call on the handle, or by gpmp2mi_sdf_reserve_update, and kept until gpmp2mi_sdf_destroy.  A later `_dev` call
 * neither allocates nor synchronises.  (The host forms stage their inputs in temporary device memory.)
 * Multi plans: an update touches the caller's handle only.  gpmp2mi_multi_plan_refresh_field copies the source handle's
 * voxels to every copy the multi plan owns (a peer copy of the plain voxels, packed there by the constructor's kernel, so
 * the cells are bit-identical) and returns when all copies are done.  The source handle must still be alive, its update
 * complete, and the multi plan idle; shards on the source's own device read the caller's handle and need no copy.  A poisoned multi plan returns GPMP2MI_ERR_TIMEOUT.  The caller's current device is the same on return
 * as on entry.
 * Not here: a field per trajectory, a change of geometry, updates of a sub-box of the grid.  Ray casting of free space,
 * accumulation of clouds and depth images are in "sensor map" below; decay over time is in neither. */
int gpmp2mi_sdf_reserve_update(gpmp2mi_sdf* s);
/* voxels in `layout`, [nz][ny][nx] cells as at gpmp2mi_sdf_create; _dev: a device pointer in GPMP2MI_SDF_LAYOUT_ZYX */
int gpmp2mi_sdf_update(gpmp2mi_sdf* s, const double* voxels, int layout);
int gpmp2mi_sdf_update_dev(gpmp2mi_sdf* s, const double* voxels_zyx, void* stream);
int gpmp2mi_sdf_update_from_occupancy(gpmp2mi_sdf* s, const double* occ, int layout);
int gpmp2mi_sdf_update_from_occupancy_dev(gpmp2mi_sdf* s, const double* occ_zyx, void* stream);
/* points [M][dim]; conf [D] of `robot`; stats [4] or NULL.  _dev: points, conf and stats are device pointers. */
int gpmp2mi_sdf_update_from_points(gpmp2mi_sdf* s, int M, const double* points /*[M][dim]*/, int use_base,
                                   const gpmp2mi_robot* robot /*NULL: no self filter*/, const double* conf /*[D]*/,
                                   double margin, int* stats /*[4] or NULL*/);
int gpmp2mi_sdf_update_from_points_dev(gpmp2mi_sdf* s, int M, const double* points, int use_base,
                                       const gpmp2mi_robot* robot, const double* conf, double margin, int* stats,
                                       void* stream);
int gpmp2mi_multi_plan_refresh_field(gpmp2mi_multi_plan* m);

/* ---- sensor map: evidence per cell kept on the field handle, free space carved by ray casting, from clouds or depth --
 * The calls of "live map" build the field from the base and the cloud of one call: nothing is remembered and nothing is
 * cleared.  These calls keep an integer evidence value per cell on the handle.  A frame raises it where rays end and
 * lowers it where rays pass; the field is rebuilt from the cells whose evidence reaches a threshold, by the distance
 * transform the handle already runs.  Geometry, streams, `_dev` forms and the meaning of "the handle afterwards equals"
 * are those of "live map".
 *
 * Data on the handle: E, int16 [nz][ny][nx], all 0 when first allocated; two byte volumes of per-call marks; six
 * counters; the records of one frame's rays.  They are taken at the first call of this section, or by
 * gpmp2mi_sdf_reserve_evidence, together with the workspace of gpmp2mi_sdf_reserve_update, and kept until
 * gpmp2mi_sdf_destroy.  A later `_dev` call neither allocates nor synchronises; the one exception is a frame with more
 * rays than any frame before it on this handle, which grows the ray records (28 bytes a ray).
 * gpmp2mi_sdf_reserve_update and the update calls of "live map" keep their memory and behaviour exactly; they neither
 * read nor change E.
 *
 * Rules.  Every expression is evaluated in IEEE double exactly as written, each operation rounded once (no fused
 * multiply-add); divisions are true divisions.  k runs over the axes x, y(, z) of the handle.
 *  1. Deprojection (depth form).  Pixel column u, row v, z = (double)depth[v][u], P = cam->pose as [3][4]:
 *       xc = (((double)u - cx) / fx) * z,  yc = (((double)v - cy) / fy) * z,
 *       p_i = ((P[i][0]*xc + P[i][1]*yc) + P[i][2]*z) + P[i][3],  sensor origin o_i = P[i][3],  M = width * height.
 *  2. Cell coordinates, the point-to-cell rule of "live map" per axis: a_k = (o_k - origin_k) / cell_size + 0.5 and
 *     b_k = (p_k - origin_k) / cell_size + 0.5.  The end point is in the grid iff 0 <= b_k < n_k on every axis, compared
 *     in double.
 *  3. Class of a ray; the first rule that matches applies:
 *       (1) invalid -- depth form: z is NaN, infinite, <= 0 or < depth_min; points form: a coordinate is not finite;
 *           either form: |b_k - a_k| >= 1048576 on some axis (a difference that is not a number counts as such);
 *       (2) max_range (depth form only): z > depth_max.  The point is recomputed with z = depth_max, and with it b; the
 *           span rule of (1) is applied to the recomputed b as well;
 *       (3) self: the self rule of "live map" on the end point, with the centres of gpmp2mi_sphere_centers(robot, conf)
 *           and radius + margin;
 *       (4) outside: the end point is not in the grid;
 *       (5) hit.
 *     Invalid rays do nothing.  Rays of classes 2-5 carve.  Only class 5 marks its end cell.
 *  4. The walk.  c_k = floor(a_k), e_k = floor(b_k), left_k = |e_k - c_k|, step_k = sign(e_k - c_k).  For the axes with
 *     left_k > 0: d_k = b_k - a_k, inv_k = 1.0 / |d_k|, first_k = (c_k + 1.0) - a_k when step_k > 0, else a_k - c_k.
 *     The walk has sum_k left_k steps.  At each step, among the axes with j_k < left_k (j_k = 0 at the start), the one
 *     with the smallest t_k = (first_k + (double)j_k) * inv_k is taken; ties go to the lowest axis index (x, then y, then
 *     z; a comparison with a NaN t is false, so such an axis is taken last); then c_k += step_k and j_k += 1 on that
 *     axis.  The products are recomputed from j_k, not accumulated, so the last cell is exactly e.  The cells of the
 *     walk are the start cell and the cell after every step.  Every cell of the walk other than its last one that lies
 *     in the grid gets this call's miss mark; the last cell of a class-5 ray gets this call's hit mark.  Cells outside
 *     the grid are walked over, not written.  (The implementation skips a ray whose cells all lie beyond the grid on
 *     one axis, and leaves a walk at a cell beyond the grid on an axis whose remaining motion is away from the grid or
 *     none: neither changes the set of marked cells.)  A planar handle has no z axis.
 *  5. Apply, per cell: E' = clamp(E + (hit mark ? hit : miss mark ? -miss : 0), lo, hi).  A hit wins over any number of
 *     misses in the same call.  The marks are per call and are gone afterwards.  The result depends on the set of rays
 *     only, not on their order: marks are plain stores of one value, no floating-point atomic and no ordered reduction
 *     is used; integer atomics add up the counts only.
 *  6. Field.  With opts->refresh, O = {E' >= occupied_at}, united with the base if use_base.  The handle is then, bit
 *     for bit, what gpmp2mi_sdf_create_from_occupancy gives for the indicator of O (the constant 1000 for an empty or a
 *     full O).  The base is never changed by these calls, and evidence cannot clear a base cell.  With refresh == 0 only
 *     E changes; gpmp2mi_sdf_refresh_from_evidence is the rebuild alone, from E as it stands.
 *  7. stats [6] (NULL ok): entries 0-4 are {hit, invalid, max_range, self, outside} and sum to M; entry 5 is the
 *     number of cells with E' >= occupied_at.
 *  8. Errors, all checked before any device work (a refused call changes nothing): GPMP2MI_ERR_INVALID for a NULL
 *     handle, camera, opts or sensor_origin; M < 0; NULL points / depth with M > 0; a negative width or height, or more
 *     than INT_MAX pixels; a non-finite sensor origin, pose or intrinsics; fx or fy == 0; a depth range that is not
 *     0 <= depth_min < depth_max, both finite; opts outside the ranges given at the struct; occupied_at outside
 *     -32768 .. 32767 for the rebuild alone; a NaN margin; robot != NULL with a NULL conf; use_base on a handle
 *     without a base; a planar handle given to the depth form; and the device rules of "live map" (a robot on another
 *     device than the field, a field whose device is not the current one).  GPMP2MI_ERR_UNSUPPORTED, GPMP2MI_ERR_ALLOC
 *     and GPMP2MI_ERR_HIP as there.
 * `sensor_origin`, `cam` and `opts` are HOST data in every form, read before the call returns.
 * Not here: decay of evidence over time, depth as uint16, gpmp2mi_multi_plan_* twins beyond the existing
 * gpmp2mi_multi_plan_refresh_field, updates of a sub-box of the grid. */
typedef struct gpmp2mi_evidence_opts {
  int hit, miss;        /* added to a cell where a ray ends / subtracted where rays pass; >= 0 (and <= 65535) */
  int lo, hi;           /* E is clamped to [lo, hi]; -32768 <= lo <= 0 <= hi <= 32767 */
  int occupied_at;      /* a cell is an obstacle iff E >= occupied_at; lo < occupied_at <= hi */
  int use_base;         /* unite with the handle's base (as gpmp2mi_sdf_update_from_points) */
  int refresh;          /* 1: rebuild the field after the evidence; 0: evidence only, field untouched */
} gpmp2mi_evidence_opts;
/* hit 2, miss 1, lo -4, hi 8, occupied_at 1, use_base 0, refresh 1 */
void gpmp2mi_evidence_opts_default(gpmp2mi_evidence_opts* opts);

typedef struct gpmp2mi_depth_camera {
  int width, height;
  double fx, fy, cx, cy;
  double depth_min, depth_max;     /* metres along the optical axis; 0 <= depth_min < depth_max, finite */
  double pose[12];                 /* camera -> world, row-major 3 x 4 [R | t] */
} gpmp2mi_depth_camera;

int gpmp2mi_sdf_reserve_evidence(gpmp2mi_sdf* s);
/* rays from sensor_origin [dim] (host) to points [M][dim]; dim 2 or 3 as the handle.  conf [D] of `robot`; stats [6] or
 * NULL.  _dev: points, conf and stats are device pointers. */
int gpmp2mi_sdf_integrate_points(gpmp2mi_sdf* s, int M, const double* points /*[M][dim]*/,
                                 const double* sensor_origin /*[dim]*/, const gpmp2mi_robot* robot /*NULL: no filter*/,
                                 const double* conf /*[D]*/, double margin, const gpmp2mi_evidence_opts* opts,
                                 int* stats /*[6] or NULL*/);
int gpmp2mi_sdf_integrate_points_dev(gpmp2mi_sdf* s, int M, const double* points, const double* sensor_origin,
                                     const gpmp2mi_robot* robot, const double* conf, double margin,
                                     const gpmp2mi_evidence_opts* opts, int* stats, void* stream);
/* depth [height][width] float32, metres along the optical axis; the handle must be 3-D.  _dev: depth, conf and stats are
 * device pointers. */
int gpmp2mi_sdf_integrate_depth(gpmp2mi_sdf* s, const gpmp2mi_depth_camera* cam, const float* depth,
                                const gpmp2mi_robot* robot /*NULL: no filter*/, const double* conf /*[D]*/, double margin,
                                const gpmp2mi_evidence_opts* opts, int* stats /*[6] or NULL*/);
int gpmp2mi_sdf_integrate_depth_dev(gpmp2mi_sdf* s, const gpmp2mi_depth_camera* cam, const float* depth,
                                    const gpmp2mi_robot* robot, const double* conf, double margin,
                                    const gpmp2mi_evidence_opts* opts, int* stats, void* stream);
/* the rebuild alone: O = {E >= occupied_at}, united with the base if use_base */
int gpmp2mi_sdf_refresh_from_evidence(gpmp2mi_sdf* s, int occupied_at, int use_base);
int gpmp2mi_sdf_refresh_from_evidence_dev(gpmp2mi_sdf* s, int occupied_at, int use_base, void* stream);
/* E = 0 everywhere; the field is left as it is */
int gpmp2mi_sdf_evidence_reset(gpmp2mi_sdf* s);
int gpmp2mi_sdf_evidence_reset_dev(gpmp2mi_sdf* s, void* stream);
/* E to a host array (all 0 for a handle that never took a call of this section); waits for the default stream */
int gpmp2mi_sdf_get_evidence(const gpmp2mi_sdf* s, int16_t* E /*[nz][ny][nx]*/);

/* ---- scene: boxes, spheres, cylinders and closed meshes into the field, on the device -------------------------------
 * "live map" takes an occupancy grid or a cloud, "sensor map" takes evidence.  These calls take known geometry: a table
 * as a box, a post as a cylinder, a fixture from CAD as a closed triangle mesh, each with a pose that may change from
 * call to call.  The objects are one more source of the occupied set O; the field is rebuilt from O by the distance
 * transform the handle already runs.  Geometry, streams, `_dev` forms and the meaning of "the handle afterwards equals"
 * are those of "live map".
 *
 * A scene handle holds 1 .. GPMP2MI_MAX_SCENE_OBJECTS objects.  Mesh vertices and triangles are copied to the device of
 * gpmp2mi_scene_create (the current one); poses and enabled flags stay on the host and are HOST data in every form, read
 * before the call returns.  The handle also owns the workspace of a rasterisation: the fixed-point vertices, one count and
 * one flag per object, and a bit volume of nx rounded up to 32 bits per row (j, k).  The bit volume is taken at the first
 * call for a grid, or by gpmp2mi_scene_reserve, and grows when a later grid needs more; a `_dev` call whose grid the
 * handle already holds neither allocates nor synchronises.  The workspace belongs to one call at a time: calls with the
 * same scene must be in stream order.  Neither the base nor E of the field handle is changed by these calls, and the
 * existing update calls keep their behaviour and their memory exactly.
 *
 * Rules.  Every floating-point expression is evaluated in IEEE double exactly as written, each operation rounded once
 * (no fused multiply-add); divisions are true divisions.  pose = [R | t], row-major 3 x 4, object -> world.
 *  1. Cell centres.  Cell (i, j, k) has the centre c = (origin_x + i*cell, origin_y + j*cell, origin_z + k*cell): the
 *     point-to-cell rule of "live map" read backwards.  On a planar handle nz = 1, c_z = 0 and origin_z counts as 0;
 *     every kind works there through the same formulas (the scene is cut by the plane z = 0).
 *  2. Primitives.  d = c - t, local coordinates l_m = (R[0][m]*d_0 + R[1][m]*d_1) + R[2][m]*d_2, s_n = size[n] + inflate.
 *       box:      occupied iff |l_0| <= s_0 and |l_1| <= s_1 and |l_2| <= s_2;
 *       sphere:   occupied iff sqrt((d_0^2 + d_1^2) + d_2^2) <= s_0;
 *       cylinder: occupied iff sqrt(l_0^2 + l_1^2) <= s_0 and |l_2| <= s_1.
 *     R is used as given (it is not made orthonormal).  Only cell CENTRES are tested: an object that contains no centre
 *     marks nothing, however large a part of a cell it covers.  An inflate of cell * sqrt(3) / 2 (half a cell's diagonal)
 *     guarantees that every cell the object touches is marked.  Sizes a kind does not use are not read.
 *  3. Meshes: solid fill by crossing parity along x, in exact integers.  It holds for any closed mesh, any winding and
 *     any triangle order; a point exactly on a vertex or an edge is resolved by a fixed symbolic shift, not by luck.
 *       (1) world vertex   w_m = ((R[m][0]*v_0 + R[m][1]*v_1) + R[m][2]*v_2) + t_m;
 *       (2) grid           g_m = (w_m - origin_m) / cell_size;
 *       (3) fixed point    q_m = (int64) rint(g_m * 1024.0), ties to even;
 *       (4) whole-mesh guard: if any vertex of the mesh has a non-finite g or |g_m * 1024| > 2^29, the WHOLE mesh marks
 *           nothing and its `cells` entry is -1.  Differences then fit in 32 bits, and every product below is exact;
 *       (5) per triangle with fixed-point vertices P0, P1, P2:
 *           a = (P1.y - P0.y)(P2.z - P0.z) - (P1.z - P0.z)(P2.y - P0.y); a == 0: the triangle is skipped; a < 0: P1 and
 *           P2 are swapped and a is negated;
 *       (6) per column (j, k) of the grid, Y = 1024 j, Z = 1024 k, and per edge (A, B) of ((P1,P2), (P2,P0), (P0,P1)):
 *           d = B - A, e = d.y (Z - A.z) - d.z (Y - A.y).  The edge passes iff e > 0, or e == 0 and (d.y > 0 or (d.y == 0
 *           and d.z > 0)).  The column crosses the triangle iff all three edges pass; then e0 + e1 + e2 = a;
 *       (7) crossing abscissa: X_n = (double)P_n.x / 1024.0,
 *           x = (((double)e0*X0 + (double)e1*X1) + (double)e2*X2) / (double)a, first = ceil(x), compared in double;
 *       (8) the crossing flips every cell i >= first of row (j, k): the whole row if first <= 0, nothing if first >= nx;
 *       (9) after all triangles of THIS mesh a cell is occupied by the mesh iff it was flipped an odd number of times.
 *     Parity is per mesh: two overlapping meshes unite, they do not cancel.
 *  4. cells [K] (NULL ok): the number of grid cells occupied by object o alone; 0 for a disabled object, -1 for a mesh
 *     that is out of range.  Integer atomics add the counts and flip the crossing bits; marks are plain stores of one
 *     value; no result depends on an order.
 *  5. Scene set and field.  The scene set is the union over the enabled objects.  gpmp2mi_sdf_update_from_scene builds
 *     O = scene set, united with the base if use_base and with {E >= occupied_at} if use_evidence; the handle is then,
 *     bit for bit, what gpmp2mi_sdf_create_from_occupancy gives for the indicator of O (the constant 1000 for an empty or
 *     a full O).  Nothing of the scene persists on the field handle: the next update of any kind starts without it.
 *  6. Errors, all checked before any device work (a refused call changes nothing).  GPMP2MI_ERR_INVALID: a NULL argument
 *     (cells may be NULL); K outside 1 .. 256; an unknown kind; a non-finite pose, size or inflate; a negative size or
 *     inflate; a mesh with inflate != 0, with V < 4 or T < 4, with NULL vertices or triangles,
 *     with an index outside 0 .. V-1 or with a triangle that repeats an index; a mesh that is not closed: some undirected
 *     edge, taken as a pair of vertex indices, occurs in an odd number of triangles; first / count outside the scene;
 *     a grid with dim not 2 or 3, a size < 1, nz != 1 on a planar grid, a cell size that is not finite and > 0 or a
 *     non-finite origin; use_base on a handle without a base; use_evidence on a handle without evidence (no call of
 *     "sensor map" or gpmp2mi_sdf_reserve_evidence yet); occupied_at outside -32768 .. 32767; a scene on another device
 *     than the field, or on one that is not the current device.  GPMP2MI_ERR_UNSUPPORTED: more than 2^20 triangles in a
 *     mesh; an axis too long for the distance transform.  GPMP2MI_ERR_ALLOC and GPMP2MI_ERR_HIP as elsewhere.
 * Not here: open meshes and surface (shell) voxelisation, mesh inflation, objects attached to a robot link (take the link
 * pose from gpmp2mi_forward_kinematics and call gpmp2mi_scene_set_poses), updates of a sub-box of the grid,
 * gpmp2mi_multi_plan_* twins beyond gpmp2mi_multi_plan_refresh_field, capsules and cones. */
enum { GPMP2MI_SCENE_BOX = 0, GPMP2MI_SCENE_SPHERE = 1, GPMP2MI_SCENE_CYLINDER = 2, GPMP2MI_SCENE_MESH = 3 };
#define GPMP2MI_MAX_SCENE_OBJECTS 256
#define GPMP2MI_MAX_SCENE_TRIANGLES 1048576   /* per mesh */
typedef struct gpmp2mi_scene_object {
  int kind;
  double size[3];        /* box: half extents x,y,z; sphere: radius,-,-; cylinder: radius, half height (local z),- */
  double inflate;        /* >= 0, added to every size of a primitive; must be 0 for a mesh */
  int n_vertices;  const double* vertices;   /* mesh: [V][3], object frame (host) */
  int n_triangles; const int* triangles;     /* mesh: [T][3] vertex indices (host) */
  double pose[12];       /* object -> world, row-major 3 x 4 [R | t] */
  int enabled;
} gpmp2mi_scene_object;
typedef struct gpmp2mi_scene gpmp2mi_scene;

int  gpmp2mi_scene_create(int K, const gpmp2mi_scene_object* objs, gpmp2mi_scene** out);   /* on the current device */
void gpmp2mi_scene_destroy(gpmp2mi_scene* sc);                                            /* NULL: no-op */
int  gpmp2mi_scene_count(const gpmp2mi_scene* sc);                                        /* -1 for NULL */
int  gpmp2mi_scene_set_poses(gpmp2mi_scene* sc, int first, int count, const double* poses /*[count][12], host*/);
int  gpmp2mi_scene_set_enabled(gpmp2mi_scene* sc, int first, int count, const int* enabled /*[count], host*/);
/* takes the bit volume for a grid of this size now, so that the first `_dev` call on it does not allocate */
int  gpmp2mi_scene_reserve(gpmp2mi_scene* sc, int nx, int ny, int nz);
/* the occupied set of the scene alone on a grid, one byte per cell [nz][ny][nx] (1 occupied, 0 free); cells [K] or NULL.
 * _dev: mask and cells are device pointers. */
int gpmp2mi_scene_rasterize(const gpmp2mi_scene* sc, int dim, const double origin[3], double cell_size, int nx, int ny,
                            int nz, unsigned char* mask, int* cells);
int gpmp2mi_scene_rasterize_dev(const gpmp2mi_scene* sc, int dim, const double origin[3], double cell_size, int nx,
                                int ny, int nz, unsigned char* mask, int* cells, void* stream);
/* O = scene  U (use_base ? base : {})  U (use_evidence ? {E >= occupied_at} : {}); the field rebuilt in place.
 * _dev: cells is a device pointer. */
int gpmp2mi_sdf_update_from_scene(gpmp2mi_sdf* s, const gpmp2mi_scene* sc, int use_base, int use_evidence,
                                  int occupied_at, int* cells /*[K] or NULL*/);
int gpmp2mi_sdf_update_from_scene_dev(gpmp2mi_sdf* s, const gpmp2mi_scene* sc, int use_base, int use_evidence,
                                      int occupied_at, int* cells, void* stream);

/* ---- distinct alternatives: how many different solutions the restarts found, one row per mode, on the device ------
 * The calls of "scoring" answer with one row.  These calls say how many different trajectories a batch holds and hand
 * over one representative of each, best first, without the trajectories leaving the device: the fallback when the
 * best row is refused downstream, the count of modes, and the rows to run gpmp2mi_plan_risk /
 * gpmp2mi_plan_collision_probability on.
 *
 * Definitions:
 *  - Rows and metric.  A row is one trajectory [N+1][2D]; only the configuration half of each state is read.  For rows
 *    b and c, state i and weights w[d] >= 0 (finite; NULL = all 1):
 *      s_i(b, c) = sum over d = 0 .. D-1, ascending, of w[d] * (x_b[i][d] - x_c[i][d])^2
 *    GPMP2MI_DIST_MAX_STATE: dist = sqrt(max_i s_i) -- two trajectories are "the same" if at every support state their
 *    configurations are within `radius`: the metric to reason about in joint space.
 *    GPMP2MI_DIST_RMS: dist = sqrt((sum over i, ascending, of s_i) / (N+1)).
 *    No angle is wrapped: the theta of the Pose2 kinds is compared as stored, and a base that arrives a full turn
 *    later is a different execution.
 *  - dist is exactly symmetric; the diagonal and any pair of bit-identical finite rows are exactly 0.  A pair's value
 *    is a function of those two rows, w, N, D and the metric alone: not of B, of where the rows sit in the batch, of
 *    the tile they fall in or of the entry point.  Every operation is rounded once, in the order written above
 *    (difference, square, one fused multiply-add per coordinate; then the max or the sum, the division, the root).  A row
 *    with a non-finite coordinate has NaN distances wherever that arithmetic gives one (a NaN s_i stays in the max).
 *  - Grouping rule ("leader" rule) over score [B], eligible [B] (ints, NULL = all 1) and radius >= 0 (+inf allowed):
 *    a row takes part iff eligible[b] != 0 && isfinite(score[b]).  The participating rows are visited in rank order:
 *    ascending score, the lowest row on ties.  A visited row joins the mode of the first leader, in leader order, with
 *    dist(row, leader) <= radius; if there is none it becomes the next leader.  A comparison with NaN is false, so a
 *    participating row with NaN distances leads a mode of its own.  A given matrix is taken to be symmetric: the entry
 *    read is dist[leader][row].
 *  - Outputs: mode [B]: index of the row's mode, in leader order, -1 for rows that do not take part.  n_modes: number
 *    of modes.  leaders [B]: leaders[k] is the leader of mode k for k < n_modes (by construction the best-ranked row
 *    of its mode), -1 beyond.  sizes [B]: number of members of mode k, 0 beyond.  leaders[0] is the row the selection
 *    rule of "scoring" picks from the same score / eligible.  Any output may be NULL.
 *  - Determinism: the rule is a function of its inputs; no floating-point atomics anywhere.  The device forms evaluate
 *    it in n_modes rounds (argmin over the undecided rows, then every undecided row within radius of that leader is
 *    decided), which gives the answer of the sequential rule.  gpmp2mi_group_traj and the plan form use exactly
 *    dist <= radius with the dist gpmp2mi_traj_distances writes: one kernel computes both, leaving one bit per pair
 *    instead of a B x B matrix of doubles.
 * Errors, before any device work: GPMP2MI_ERR_INVALID for a NULL handle or required pointer (traj; dist for the distance
 * calls and, with B > 0, for gpmp2mi_group_rows*; score for the grouping calls), B < 0 (B == 0 is fine and does
 * nothing, n_modes = 0), total_step < 1, dof outside 1..GPMP2MI_MAX_DOF, an unknown metric, a negative or NaN radius, a
 * negative or non-finite weight, max_alt outside 1..GPMP2MI_MAX_ALTERNATIVES, and the argument and state errors of
 * gpmp2mi_plan_select for the plan forms; GPMP2MI_ERR_UNSUPPORTED, the limit in the message, for
 * B > GPMP2MI_MAX_GROUP_ROWS (every call of this section that uses the device; the host form gpmp2mi_group_rows has
 * no row limit); GPMP2MI_ERR_TIMEOUT for a poisoned plan.  A refused call writes nothing.
 * Memory: `weights` is a HOST array in every form, read before the call returns (as Qc in "sampled clearance").  The
 * bit matrix is B * ceil(B/64) 64-bit words.  A plan takes it, with a few [B] arrays and the staging of its
 * host-pointer form, at the first call and keeps it (grown when a later call needs more): with the scoring, posterior,
 * seeding, band and sampled workspaces the sixth exception to "nothing is allocated after gpmp2mi_plan_create".
 * gpmp2mi_group_traj_dev has no handle to keep a workspace with: it allocates the bit matrix, and waits for `stream`
 * before it frees it again -- ONE synchronising allocation per call.  The stream-ordered allocator is deliberately
 * not used: it draws on a per-device pool the host application (PyTorch) tunes and trims for itself, it needs a second
 * path for devices without pool support, and the caller who must not wait has the plan form.  gpmp2mi_traj_distances_dev,
 * gpmp2mi_group_rows_dev and gpmp2mi_plan_select_distinct_dev (once its workspaces hold the shape) enqueue and return
 * without a host synchronisation.  Calls on one plan belong in stream order.  The optimizer's state is not touched: a
 * gpmp2mi_plan_update afterwards gives what it gives without the call.
 * Not here: gpmp2mi_multi_plan_* twins, time-warp-invariant or workspace (end-effector) metrics, more than
 * GPMP2MI_MAX_GROUP_ROWS rows, a distinctness term inside gpmp2mi_plan_select itself. */
enum { GPMP2MI_DIST_MAX_STATE = 0, GPMP2MI_DIST_RMS = 1 };
#define GPMP2MI_MAX_GROUP_ROWS 8192
#define GPMP2MI_MAX_ALTERNATIVES 64

/* dist [B][B]; traj [B][total_step+1][2 dof] */
int gpmp2mi_traj_distances(int dof, int B, int total_step, const double* traj, const double* weights, int metric,
                           double* dist);
int gpmp2mi_traj_distances_dev(int dof, int B, int total_step, const double* traj, const double* weights, int metric,
                               double* dist, void* stream);
/* The rule on a given matrix.  Host pointers: runs on the host, no device needed (as gpmp2mi_select_best).
 * _dev: device pointers, one kernel. */
int gpmp2mi_group_rows(int B, const double* dist, const double* score, const int* eligible, double radius, int* mode,
                       int* leaders, int* sizes, int* n_modes);
int gpmp2mi_group_rows_dev(int B, const double* dist, const double* score, const int* eligible, double radius, int* mode,
                           int* leaders, int* sizes, int* n_modes, void* stream);
/* Distances and rule in one enqueue (two kernels), without a B x B matrix of doubles. */
int gpmp2mi_group_traj(int dof, int B, int total_step, const double* traj, const double* weights, int metric,
                       double radius, const double* score, const int* eligible, int* mode, int* leaders, int* sizes,
                       int* n_modes);
int gpmp2mi_group_traj_dev(int dof, int B, int total_step, const double* traj, const double* weights, int metric,
                           double radius, const double* score, const int* eligible, int* mode, int* leaders, int* sizes,
                           int* n_modes, void* stream);
/* The plan's resident result, one enqueue: the scores of gpmp2mi_plan_score (and of gpmp2mi_plan_self_score when pairs
 * != NULL), eligibility by the rule of "scoring" (extended as in "self-collision check" when pairs != NULL), score =
 * the plan's final_error, then the grouping, then the copies.
 * alt [max_alt], alt_size [max_alt]: leader and size of the first min(n_modes, max_alt) modes, -1 / 0 beyond; alt_error
 * [max_alt]: their final_error (untouched beyond); mode [B]; traj_alt [max_alt][N+1][2D], dense_alt [max_alt][Md][2D]:
 * slab k as gpmp2mi_plan_select writes traj_best / dense_best for row alt[k]; slabs k >= n_modes untouched.  n_modes
 * counts ALL modes, also beyond max_alt.  alt[0] and n_eligible are the best / n_eligible of gpmp2mi_plan_select (of
 * gpmp2mi_plan_select_checked when pairs is given) for the same arguments; mode, alt and alt_size are what
 * gpmp2mi_group_traj gives on the plan's result with that eligibility.  Any output may be NULL. */
int gpmp2mi_plan_select_distinct(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                 const gpmp2mi_self_pairs* pairs /*NULL ok*/, double required_self_clearance,
                                 int metric, const double* weights, double radius, int max_alt, int* n_modes,
                                 int* n_eligible, int* alt, int* alt_size, double* alt_error, int* mode,
                                 double* traj_alt, double* dense_alt);
int gpmp2mi_plan_select_distinct_dev(gpmp2mi_plan* p, int inter_step, double required_clearance, int require_in_range,
                                     const gpmp2mi_self_pairs* pairs /*NULL ok*/, double required_self_clearance,
                                     int metric, const double* weights, double radius, int max_alt, int* n_modes,
                                     int* n_eligible, int* alt, int* alt_size, double* alt_error, int* mode,
                                     double* traj_alt, double* dense_alt, void* stream);

/* ---- factor-level entry points (the GTSAM plug-in contract: evaluateError(x..., H...)) -----
 * All batched over M independent evaluations, host pointers, Jacobian outputs may be NULL. */

/* ForwardKinematics::forwardKinematics(jp, none, jpx, none, J_jpx_jp)
 * kinematics/Arm.cpp:31-143, PointRobot.cpp:15-49, Pose2MobileArm.cpp:30-108.
 * conf [M][D] -> poses [M][L][16] (row-major 4x4), J_pose [M][L][6][D] (GTSAM Pose3 tangent
 * order [omega; v], body frame). */
int gpmp2mi_forward_kinematics(const gpmp2mi_robot* r, int M, const double* conf, double* poses,
                               double* J_pose);

/* RobotModel::sphereCenters kinematics/RobotModel-inl.h:12-40.
 * conf [M][D] -> centers [M][S][3], J [M][S][3][D]. */
int gpmp2mi_sphere_centers(const gpmp2mi_robot* r, int M, const double* conf, double* centers,
                           double* J);

/* ObstacleSDFFactor / ObstaclePlanarSDFFactor ::evaluateError
 * obstacle/ObstacleSDFFactor-inl.h:18-56, obstacle/ObstaclePlanarSDFFactor-inl.h:18-58.
 * conf [M][D] -> err [M][S] (unwhitened), H1 [M][S][D]. */
int gpmp2mi_obstacle_factor(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, double epsilon, int M,
                            const double* conf, double* err, double* H1);

/* ObstacleSDFFactorGP / ObstaclePlanarSDFFactorGP ::evaluateError
 * obstacle/ObstacleSDFFactorGP-inl.h:18-76, obstacle/ObstaclePlanarSDFFactorGP-inl.h:19-79
 * with GaussianProcessInterpolatorLinear (gp/GaussianProcessInterpolatorLinear.h:48-96) for
 * vector-space robots and GaussianProcessInterpolatorPose2Vector for Pose2 robots.
 * conf1,vel1,conf2,vel2 [M][D]; Qc [D][D] or NULL (= I) -> err [M][S], H1..H4 [M][S][D]. */
int gpmp2mi_obstacle_gp_factor(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, double epsilon,
                               const double* Qc, double delta_t, double tau, int M,
                               const double* conf1, const double* vel1, const double* conf2,
                               const double* vel2, double* err, double* H1, double* H2,
                               double* H3, double* H4);

/* GaussianProcessPriorLinear::evaluateError gp/GaussianProcessPriorLinear.h:57-83 (lie = 0) and
 * GaussianProcessPriorPose2Vector gp/GaussianProcessPriorLie.h:61-86 (lie = 1, first three
 * coordinates are a Pose2).  -> err [M][2D]; H1..H4 [M][2D][D]. */
int gpmp2mi_gp_prior_factor(int dof, int lie, double delta_t, int M, const double* conf1,
                            const double* vel1, const double* conf2, const double* vel2,
                            double* err, double* H1, double* H2, double* H3, double* H4);

/* GaussianProcessInterpolatorLinear::interpolatePose / interpolateVelocity
 * gp/GaussianProcessInterpolatorLinear.h:62-122 (used by interpolateArmTraj,
 * planner/TrajUtils.cpp:96-197).  -> conf [M][D], vel [M][D]. */
int gpmp2mi_gp_interpolate(int dof, int lie, const double* Qc, double delta_t, double tau, int M,
                           const double* conf1, const double* vel1, const double* conf2,
                           const double* vel2, double* conf, double* vel);

/* gpmp2::interpolateArmTraj (both overloads) / interpolatePose2MobileArmTraj
 * planner/TrajUtils.cpp:96-236: up-sample B trajectories with inter_step GP-interpolated states
 * inside every interval of [start_index, end_index] (0 <= start_index < end_index <= total_step;
 * the no-range overload of the reference is start_index = 0, end_index = total_step).
 * traj [B][total_step+1][2D] -> out [B][(end_index - start_index)*(inter_step+1) + 1][2D].
 * Qc is accepted for interface parity; Lambda and Psi do not depend on it (gp/GPutils.h:44-59). */
int gpmp2mi_interpolate_traj(int dof, int lie, const double* Qc, double delta_t, int inter_step,
                             int B, int total_step, int start_index, int end_index,
                             const double* traj, double* out);
/* same on device pointers, enqueued on `stream` (e.g. traj = gpmp2mi_plan_traj_dev(plan)) */
int gpmp2mi_interpolate_traj_dev(int dof, int lie, double delta_t, int inter_step, int B,
                                 int total_step, int start_index, int end_index,
                                 const double* traj, double* out, void* stream);

/* GaussianPriorWorkspace{Position,Orientation,Pose}::evaluateError
 * kinematics/GaussianPriorWorkspacePosition.h:52-67, ...Orientation.h:52-69, ...Pose.h:53-70:
 * prior on the world pose of link `joint`.  des_pose: row-major 4x4 (position mode uses its
 * translation, orientation mode its rotation).  -> err [M][3|3|6] (pose: [omega; u] of
 * Pose3::Logmap(des^-1 * pose)), H [M][rows][D] (may be NULL).  Rot3 / Pose3 log maps follow
 * GTSAM 4.0 (upstream; pinned by the reference's known answers). */
int gpmp2mi_workspace_prior_factor(const gpmp2mi_robot* r, int mode, int joint,
                                   const double des_pose[16], int M, const double* conf,
                                   double* err, double* H);
/* GoalFactorArm::evaluateError kinematics/GoalFactorArm.h:58-77: end-effector position minus
 * dest_point (= the position prior on the last link).  -> err [M][3], H [M][3][D] */
int gpmp2mi_goal_factor_arm(const gpmp2mi_robot* r, const double dest_point[3], int M,
                            const double* conf, double* err, double* H);
/* SelfCollision::evaluateError obstacle/SelfCollision.h:66-128.  data [n_pairs][4] = (sphere A id,
 * sphere B id, epsilon, sigma) with ids in the order of the robot description; hinge on
 * radius_A + radius_B + epsilon - |c_A - c_B|.  -> err [M][n_pairs], H [M][n_pairs][D] */
int gpmp2mi_self_collision_factor(const gpmp2mi_robot* r, int n_pairs, const double* data, int M,
                                  const double* conf, double* err, double* H);

/* VehicleDynamicsFactorPose2 / Pose2Vector (lie = 1) and VehicleDynamicsFactorVector (lie = 0)
 * dynamics/VehicleDynamics.h:19-40, dynamics/VehicleDynamicsFactorPose2Vector.h:55-78,
 * dynamics/VehicleDynamicsFactorVector.h:53-78: sliding velocity of an SE(2) base.  conf, vel [M][D] with
 * D >= 3 (the first three coordinates are x, y, theta).  -> err [M], Hp [M][D], Hv [M][D] (may be NULL). */
int gpmp2mi_vehicle_dynamics_factor(int dof, int lie, int M, const double* conf, const double* vel,
                                    double* err, double* Hp, double* Hv);

/* JointLimitFactorVector / VelocityLimitFactorVector ::evaluateError
 * kinematics/JointLimitFactorVector.h:62-79, kinematics/VelocityLimitFactorVector.h:62-79.
 * x [M][D] -> err [M][D], Hdiag [M][D] (the diagonal of the Jacobian). */
int gpmp2mi_joint_limit_factor(int dof, const double* down, const double* up, const double* thresh,
                               int M, const double* x, double* err, double* Hdiag);

/* Batched block-tridiagonal SPD solve  H x = b  (the replacement for GTSAM's sparse Cholesky,
 * planner/BatchTrajOptimizer.cpp:240-286 -> GaussianFactorGraph::optimize).
 * Hdiag [B][nblk][n][n], Hoff [B][nblk-1][n][n] (block (i+1,i)), b [B][nblk][n] -> x, ok [B]. */
int gpmp2mi_block_tridiag_solve(int B, int nblk, int n, const double* Hdiag, const double* Hoff,
                                const double* b, double* x, int* ok);

/* ---- posterior: marginal covariances and samples, on the device -------------------------------------
 * The MAP trajectory of a plan is the mean of a Gaussian posterior whose covariance is Sigma = H^-1, H the
 * Gauss-Newton Hessian of the graph at that trajectory: what gtsam::Marginals(graph, values).marginalCovariance(key)
 * and ISAM2::marginalCovariance(key) return.  H is block tridiagonal (block n = 2D, z_i = [x_i; v_i]); one kernel
 * eliminates it forward as the solvers do (H = L L^T, L^T block upper bidiagonal) and sweeps back
 * (Rauch-Tung-Striebel) for the blocks of Sigma on the band, or back-substitutes K vectors z for
 * delta = L^-T z: with z ~ N(0, I), delta ~ N(0, Sigma), a perturbation of the trajectory drawn from the posterior.
 *
 * Sigma = H^-1 of B block-tridiagonal SPD systems (layouts of gpmp2mi_block_tridiag_solve):
 * Sdiag [B][nblk][n][n] = Sigma_ii (exactly symmetric), Soff [B][nblk-1][n][n] = block (i+1,i) = Sigma_{i,i+1}^T,
 * ok [B] (0: a pivot was not positive; that system's outputs are then unspecified).  Any output may be NULL.
 * n = 1..15 (GPMP2MI_ERR_UNSUPPORTED above). */
int gpmp2mi_block_tridiag_marginals(int B, int nblk, int n, const double* Hdiag, const double* Hoff,
                                    double* Sdiag, double* Soff, int* ok);
/* delta = L^-T z, H = L L^T:  z, delta [B][K][nblk][n], K >= 1; ok may be NULL */
int gpmp2mi_block_tridiag_sample(int B, int nblk, int n, int K, const double* Hdiag, const double* Hoff,
                                 const double* z, double* delta, int* ok);
/* the plan's graph linearized (Gauss-Newton Hessian, no damping; start/goal and state priors and extra
 * factors included) at `traj` (host, [B][N+1][2D]) or, traj == NULL, at the plan's current estimate (the result of
 * the last optimize / update; the initial values if there is none); tangent space at that estimate for Pose2 robots,
 * as gtsam::Marginals.  Sdiag [B][N+1][2D][2D], Soff [B][N][2D][2D], ok [B]; any output may be NULL.
 * The optimizer's state is not touched: a gpmp2mi_plan_update after these calls gives what it gives without them.
 * Errors: GPMP2MI_ERR_INVALID for a NULL plan, before gpmp2mi_plan_set_problem, K < 1 or a NULL z / delta;
 * GPMP2MI_ERR_TIMEOUT for a poisoned plan, before anything is enqueued; GPMP2MI_ERR_UNSUPPORTED for 2D > 15 (the wide
 * and dense plans, dof >= 8): one 16 x 16 tile per block is the limit of this kernel.
 * Memory: the exported H (2 (2D)^2 doubles per state) and 512 doubles of factors per state are taken at the first call
 * and kept with the plan, as the scoring workspace is.  The `_dev` forms (device pointers, current estimate) enqueue
 * on `stream` and return without a host synchronisation; calls on one plan belong in stream order. */
int gpmp2mi_plan_marginals(gpmp2mi_plan* p, const double* traj, double* Sdiag, double* Soff, int* ok);
int gpmp2mi_plan_marginals_dev(gpmp2mi_plan* p, double* Sdiag, double* Soff, int* ok, void* stream);
/* z, delta [B][K][N+1][2D]: delta ~ N(0, Sigma) for z ~ N(0, I); retract delta onto the estimate for samples of the
 * trajectory (vector-space robots: estimate + delta) */
int gpmp2mi_plan_sample_posterior(gpmp2mi_plan* p, int K, const double* z, double* delta, int* ok);
int gpmp2mi_plan_sample_posterior_dev(gpmp2mi_plan* p, int K, const double* z, double* delta, int* ok, void* stream);

/* ---- posterior on the executed timeline: dense covariances and the k-sigma clearance, on the device -----------
 * gpmp2mi_plan_score checks the Md = N (J + 1) + 1 executed states deterministically; gpmp2mi_plan_marginals gives
 * Sigma = H^-1 at the N + 1 support states only.  These calls carry the posterior to the executed states and ask how
 * sure the planner is that they clear the obstacles.
 *
 * Setting: vector-space robots (the fixed-base arm and the point robot), state z = [x; v], n = 2D, the linear
 * constant-velocity GP, Delta = delta_t, J = inter_step >= 0.
 *  - Checked states as in "scoring": state m has interval i = m / (J+1), sub-step j = m % (J+1), tau = j (Delta / (J+1)).
 *  - Support posterior: Sdiag[i] = Sigma_ii, Soff[i] = Sigma_{i+1,i} (rows of i+1, columns of i), as
 *    gpmp2mi_plan_marginals returns them.
 *  - Covariance of a checked state.  j = 0: Sigma(m) = Sigma_ii, copied bit for bit.  j > 0: with
 *    Lambda = Lambda_2(tau) (x) I_D, Psi = Psi_2(tau) (x) I_D (the scalars of gpmp2mi_gp_interpolate) and C = Sigma_{i+1,i},
 *        Sigma(m) = Lambda Sigma_ii Lambda^T + Psi Sigma_{i+1,i+1} Psi^T + Psi C Lambda^T + (Psi C Lambda^T)^T
 *                   + Q_c(tau) (x) Qc,
 *    Q_c(tau) the 2 x 2 conditional covariance of the prior bridge, evaluated in factored form with t = tau:
 *        [0][0] = t^3 (Delta-t)^3 / (3 Delta^3),   [0][1] = [1][0] = t^2 (Delta-t)^2 (Delta-2t) / (2 Delta^3),
 *        [1][1] = t (Delta-t) (Delta^2 - 3 t Delta + 3 t^2) / Delta^3      (= Q(t) - Psi_2 Q(Delta) Psi_2^T).
 *    Qc is row-major [D][D], SPD, NULL = identity; a plan uses the Qc of its setting.  This is the exact posterior of
 *    z(tau): every factor of the graph, the GP obstacle factors included, depends on the support states only, so
 *    p(z(tau) | data) is the prior conditional integrated over the support posterior.
 *  - Clearance deviation, for checked state m and sphere s with centre, field lookup, in-range rule and clearance(m, s)
 *    exactly as in "scoring": h = grad d . d centre / d x (1 x D; planar fields use x and y only),
 *    sigma^2(m, s) = h Sigma_xx(m) h^T with Sigma_xx the top-left D x D block of Sigma(m), sigma = sqrt(max(sigma^2, 0)).
 *  - Robust clearance, kappa >= 0 finite: c_kappa(m, s) = clearance(m, s) - kappa sigma(m, s).  robust_clearance [B] is
 *    its minimum over the in-range pairs, +inf if there is none; worst [B][2] the (m, s) attaining it, ties as in
 *    "scoring", (-1, -1) if none; sigma_worst [B] is sigma at that pair (0 if none); out_of_range [B] as in "scoring".
 *    No division, no special case for sigma = 0.  sigma [B][Md][S] (sphere ids in the order of the robot description)
 *    is the map of sigma(m, s); NaN at pairs that are out of range.
 *  - Rows that are not SPD (ok[b] == 0): robust_clearance = sigma_worst = NaN, worst = (-1, -1), and the row's sigma
 *    map is NaN where in range.  gpmp2mi_select_best never picks a NaN clearance, so robust_clearance can be passed to
 *    gpmp2mi_select_best(_dev) as its min_clearance with required_clearance = 0: no further selection rule is needed.
 *  - Determinism as in "scoring": a row's outputs are a function of that row, the robot, the field, Delta, J, kappa and
 *    the row's band alone; sums are taken in a fixed order, without floating-point atomics.
 * Every output may be NULL.  The `_dev` forms take device pointers (Qc and ok included) and a stream, enqueue, and
 * return without a host synchronisation.
 * Errors, before any device work: GPMP2MI_ERR_INVALID for a NULL handle or input, inter_step < 0, B < 0 (B == 0 is
 * fine and does nothing), total_step < 1, delta_t <= 0, kappa negative or not finite, dof outside
 * 1..GPMP2MI_MAX_DOF.  gpmp2mi_risk_traj and the plan forms return GPMP2MI_ERR_UNSUPPORTED for dof >= 8 (the limit of
 * the posterior kernel, with its message) and for the Pose2 robot kinds (the covariance of the tangent-space
 * interpolation is not built; the seeded calls refuse these kinds in the same way).
 * Memory: gpmp2mi_risk_traj_dev keeps one 32-byte record per 64 checked states and row with the robot handle, in the
 * block gpmp2mi_score_traj_dev uses and under its rule (calls on one handle in stream order, the handle's device
 * current).  A plan takes the band (2 (2D)^2 doubles per state), ok and its records at the first call below and keeps
 * them, and puts its Qc on the device then (that first call waits for the copy): with the scoring, posterior and
 * seeding workspaces the fourth exception to "nothing is allocated after gpmp2mi_plan_create". */

/* cov [B][Md][n][n] from a band, any dof <= GPMP2MI_MAX_DOF (the interpolation is Kronecker: no tile layout).  cov is
 * exactly symmetric between support states (one triangle is computed and mirrored); support states are copies of Sdiag. */
int gpmp2mi_gp_interpolate_cov(int dof, const double* Qc, double delta_t, int inter_step, int B, int total_step,
                               const double* Sdiag, const double* Soff, double* cov);
int gpmp2mi_gp_interpolate_cov_dev(int dof, const double* Qc, double delta_t, int inter_step, int B, int total_step,
                                   const double* Sdiag, const double* Soff, double* cov, void* stream);
/* traj [B][total_step+1][2D] with its band; ok [B] or NULL = all fine */
int gpmp2mi_risk_traj(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, const double* Qc, double delta_t,
                      int inter_step, int B, int total_step, const double* traj, const double* Sdiag,
                      const double* Soff, const int* ok, double kappa, double* robust_clearance, int* worst,
                      double* sigma_worst, int* out_of_range, double* sigma);
int gpmp2mi_risk_traj_dev(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, const double* Qc, double delta_t,
                          int inter_step, int B, int total_step, const double* traj, const double* Sdiag,
                          const double* Soff, const int* ok, double kappa, double* robust_clearance, int* worst,
                          double* sigma_worst, int* out_of_range, double* sigma, void* stream);
/* The plan at its current estimate, with the state rules of gpmp2mi_plan_marginals (a problem is set, the plan is not
 * poisoned): linearize -> export -> the posterior sweep into the plan's band workspace, then the kernels above.  The
 * optimizer's records, factors and estimate are not touched.  ok [B] as gpmp2mi_plan_marginals. */
int gpmp2mi_plan_marginals_dense(gpmp2mi_plan* p, int inter_step, double* cov, int* ok);
int gpmp2mi_plan_marginals_dense_dev(gpmp2mi_plan* p, int inter_step, double* cov, int* ok, void* stream);
int gpmp2mi_plan_risk(gpmp2mi_plan* p, int inter_step, double kappa, double* robust_clearance, int* worst,
                      double* sigma_worst, int* out_of_range, double* sigma, int* ok);
int gpmp2mi_plan_risk_dev(gpmp2mi_plan* p, int inter_step, double kappa, double* robust_clearance, int* worst,
                          double* sigma_worst, int* out_of_range, double* sigma, int* ok, void* stream);

/* ---- seeding: restarts and samples from a counter RNG, on the device ------------------------------------
 * The random function.  normal(seed, stream, a, b, i, r) is a standard normal that is a pure function of its arguments
 * (gpmp2_amd/csrc/rng.h states it once, for the kernels and for a host compiler alike): Philox4x32-10 keyed by the 64-bit
 * seed on the counter (a, b, i, stream << 8 | pair), Box-Muller in fp64 on the two 53-bit uniforms of a block;
 * coordinates r and r + 4 (bit 2 of r clear) are the cosine and sine member of one pair; r = 0..15, stream < 2^24.
 * Every value is finite, |z| <= 8.57.  `stream` separates the uses: the library draws restarts from
 * GPMP2MI_RNG_RESTARTS and posterior samples from GPMP2MI_RNG_POSTERIOR.
 * Determinism: a problem's numbers depend on (seed, problem index) alone -- not on M, B, the slot, the shard, or the
 * entry point that asked.
 *
 * out [a_count][b_count][nblk][n] = normal(seed, stream, a_first + a, b_first + b, i, r), n = 1..16. */
enum { GPMP2MI_RNG_RESTARTS = 1, GPMP2MI_RNG_POSTERIOR = 2 };
int gpmp2mi_normal_fill(uint64_t seed, int stream, int a_first, int a_count, int b_first, int b_count, int nblk, int n,
                        double* out);   /* host out; runs on the device */
int gpmp2mi_normal_fill_dev(uint64_t seed, int stream, int a_first, int a_count, int b_first, int b_count, int nblk,
                            int n, double* out, void* hip_stream);
/* Restarts from the GP prior.  Problem j = first + row (row < M) gets
 *     init_j = mean_j + scale * L^-T z_j,     z_j[i][r] = normal(seed, GPMP2MI_RNG_RESTARTS, j, 0, i, r),
 * H_seed = L L^T the block-tridiagonal precision of the plan's LINEAR PRIOR GRAPH: the PriorFactors on x_0, v_0, x_N, v_N
 * (conf_prior_sigma, vel_prior_sigma) and the N GaussianProcessPriorLinear factors (Qc, delta_t = total_time / N).
 * Both end priors are always in it; end_conf_prior_off, obstacle, limit, workspace and self-collision factors are not:
 * it is a proposal (smooth trajectories pinned at both ends, velocities consistent with positions), not the posterior.
 * keep_first != 0: problem j == 0 gets exactly its mean.  mean [M][N+1][2D], or NULL: the straight line of
 * gpmp2::initArmTrajStraightLine from start_conf[row] to end_conf[row] ([M][D]), bit for bit.  init [M][N+1][2D].
 * H_seed does not depend on the problem: it is built on the host, uploaded and factored once per plan at the first
 * seeded call (which therefore waits for its stream once), and kept with the plan -- with the scoring and posterior
 * workspaces the third exception to "nothing is allocated after gpmp2mi_plan_create": 2 (2D)^2 + 512 doubles per state.
 * The queue forms make the M inits on the device and run gpmp2mi_plan_optimize_queue(_dev) on them: the results equal
 * seed_restarts followed by optimize_queue, the refusals are those of optimize_queue; init_out ([M][N+1][2D], NULL ok)
 * receives the inits.  Shard k of a multi plan draws problems first + row_begin_k .., so a multi plan returns what one
 * plan returns.
 * Errors: GPMP2MI_ERR_INVALID for a NULL plan or required pointer (start_conf / end_conf may be NULL for seed_restarts
 * when a mean is given), M < 1, first < 0, a negative or non-finite scale; GPMP2MI_ERR_UNSUPPORTED for 2D > 15 (one
 * 16 x 16 tile per block) and for the Pose2 robot kinds (a bridge in the tangent space is not built);
 * GPMP2MI_ERR_TIMEOUT for a poisoned plan, before anything is enqueued.  The `_dev` forms take device pointers and
 * enqueue on `stream`; seed_restarts_dev returns without a host synchronisation (after the plan's first seeded call). */
int gpmp2mi_plan_seed_restarts(gpmp2mi_plan* p, int M, uint64_t seed, int first, double scale, int keep_first,
                               const double* start_conf, const double* end_conf, const double* mean /*NULL ok*/,
                               double* init);
int gpmp2mi_plan_seed_restarts_dev(gpmp2mi_plan* p, int M, uint64_t seed, int first, double scale, int keep_first,
                                   const double* start_conf, const double* end_conf, const double* mean /*NULL ok*/,
                                   double* init, void* stream);
int gpmp2mi_plan_optimize_queue_seeded(gpmp2mi_plan* p, int M, uint64_t seed, int first, double scale, int keep_first,
                                       const double* start_conf, const double* start_vel, const double* end_conf,
                                       const double* end_vel, const double* mean /*NULL ok*/, double* traj, int* iters,
                                       double* final_error, int* status, double* error_trace,
                                       double* init_out /*NULL ok*/);
int gpmp2mi_plan_optimize_queue_seeded_dev(gpmp2mi_plan* p, int M, uint64_t seed, int first, double scale,
                                           int keep_first, const double* start_conf, const double* start_vel,
                                           const double* end_conf, const double* end_vel, const double* mean /*NULL ok*/,
                                           double* traj, int* iters, double* final_error, int* status,
                                           double* error_trace, double* init_out /*NULL ok*/, void* stream);
int gpmp2mi_multi_plan_optimize_queue_seeded(gpmp2mi_multi_plan* m, int M, uint64_t seed, int first, double scale,
                                             int keep_first, const double* start_conf, const double* start_vel,
                                             const double* end_conf, const double* end_vel,
                                             const double* mean /*NULL ok*/, double* traj, int* iters,
                                             double* final_error, int* status, double* error_trace,
                                             double* init_out /*NULL ok*/);
/* gpmp2mi_plan_sample_posterior with z made in registers: delta [B][K][N+1][2D] = L^-T z at the current estimate,
 * z of (row b, sample s) = normal(seed, GPMP2MI_RNG_POSTERIOR, row_first + b, sample_first + s, i, r); one wavefront
 * per (16 samples, row).  ok [B] may be NULL.  Errors as above, and GPMP2MI_ERR_INVALID for K < 1, negative row_first /
 * sample_first, or before gpmp2mi_plan_set_problem.  The optimizer's state is not touched. */
int gpmp2mi_plan_sample_posterior_seeded(gpmp2mi_plan* p, int K, uint64_t seed, int row_first, int sample_first,
                                         double* delta, int* ok);
int gpmp2mi_plan_sample_posterior_seeded_dev(gpmp2mi_plan* p, int K, uint64_t seed, int row_first, int sample_first,
                                             double* delta, int* ok, void* stream);

/* ---- sampled clearance: the collision probability of a plan from posterior samples, on the device ------------
 * gpmp2mi_plan_risk answers with a first-order number, clearance - kappa sigma, pair by pair.  These calls draw K whole
 * trajectories per row from the posterior ON THE EXECUTED TIMELINE, put each through the collision check of "scoring",
 * and count: how likely is the trajectory as a whole to come closer to an obstacle than required_clearance?
 *
 * Setting: that of "posterior on the executed timeline": vector-space robots with 2D <= 15, state [x; v],
 * Delta = delta_t, J = inter_step, 0 <= J <= 63, Md = N (J+1) + 1 checked states; state m has interval i = m / (J+1),
 * sub-step j = m % (J+1) and tau_j = j (Delta / (J+1)).
 *  - Indices.  Row b and sample s of a call have the global indices r = row_first + b and q = sample_first + s.
 *  - Support sample.  delta [N+1][2D] = L^-T z with z[i][rho] = normal(seed, GPMP2MI_RNG_POSTERIOR, r, q, i, rho): exactly
 *    the delta of gpmp2mi_plan_sample_posterior_seeded (the stand-alone call takes delta from the caller).
 *    zeta_i = est_i + delta_i, one rounded addition per coordinate.
 *  - Sampled configuration x_s(m) [D]: the configuration half of gpmp2mi_interpolate_traj(inter_step = J) applied to zeta,
 *    with the arithmetic of "scoring" (zeta is rounded, then interpolated); for bridge != 0 and j > 0, plus eps(i, j).
 *  - Bridge noise.  A sample between support states is not the interpolation of a support sample: it also carries the
 *    noise of the prior bridge, jointly over the sub-steps of an interval.
 *        eps(i, j) = sum_{j' = 1..j} Lp[j][j'] (C xi_{i,j'}),
 *        xi_{i,j'}[d] = normal(seed, GPMP2MI_RNG_BRIDGE, r, q, i (J+1) + j', d),  d < D.
 *    C is the lower Cholesky factor of Qc ([D][D] row-major, SPD, NULL = identity; a plan uses its setting's Qc) and Lp
 *    the lower Cholesky factor of the J x J matrix P: for s = tau_a <= t = tau_b,
 *        P[a][b] = P[b][a] = s^2 (Delta - t)^2 (3 t Delta - s Delta - 2 s t) / (6 Delta^3),
 *    the position-position part of K0(s,t) - K0(s,Delta) Q(Delta)^-1 K0(Delta,t) with K0(s,t) = Q(s) Phi(t-s)^T; at a = b
 *    it is t^3 (Delta-t)^3 / (3 Delta^3) = Q_c(tau)[0][0] of "posterior on the executed timeline".  Both factors are
 *    formed on the host in fp64 by row-wise Cholesky without pivoting -- for each row a and b = 0..a:
 *    s = A[a][b] - sum_{k<b} L[a][k] L[b][k], L[a][b] = s / L[b][b] below the diagonal and sqrt(s) on it -- and uploaded
 *    once per key (Qc, delta_t, J); a plan or robot handle keeps the factors of its last 4 keys, and only a call with a
 *    new key waits for the copy.  A new key takes the place of the oldest one with a copy on the calling stream: calls on
 *    one handle must be in stream order (as for the records, see Memory), or a kernel still queued on another stream
 *    could read a block while it is replaced.  eps of
 *    different intervals, rows or samples are independent, and eps is independent of delta.
 *  - Law of the samples.  The x_s(.) of one sample are a joint draw of the configurations on the executed timeline from
 *    the Gaussian posterior; the marginal covariance of x_s(m) is the Sigma_xx(m) of gpmp2mi_plan_marginals_dense.
 *    Velocities are not sampled.
 *  - Per sample: clearance_s(m, sphere) as in "scoring" at x_s(m) (in-range rule, planar fields and non-finite centres
 *    as there); state_clearance [B][K][Md] = its minimum over the in-range spheres, +inf if none; clearance [B][K] = c_s =
 *    the minimum over m; worst [B][K][2] the (m, sphere) attaining it with the ties of "scoring", (-1, -1) if none.
 *  - Per row: hits [B] = #{s : c_s < required_clearance}, an exact integer; probability [B] = hits / K, one fp64 division;
 *    state_hits [B][Md] = #{s : state_clearance[s][m] < required_clearance}; oor_samples [B] = #{s with at least one
 *    out-of-range pair}.  conf [B][K][Md][D] receives the sampled configurations.
 *  - bridge = 0, or J = 0: c_s and worst[s] are bit for bit the min_clearance and worst of gpmp2mi_score_traj on zeta.
 *  - Rows with ok[b] == 0: hits = state_hits = oor_samples = -1, probability = clearance = state_clearance = conf = NaN,
 *    worst = (-1, -1).
 *  - Determinism: every output of (row, sample) is a function of the row's estimate and factorisation, the robot, the
 *    field, Delta, J, bridge, seed, r and q alone -- not of B, K, the chunking below, the entry point or the device.
 *    Counts are integers, so hits and state_hits of a sample range are the sums over any split of it.  No floating-point
 *    atomics.
 * Every output may be NULL.  The `_dev` forms take device pointers (ok included; Qc stays a HOST array, read before the
 * call returns) and a stream, enqueue, and return.
 * Errors, before any device work: GPMP2MI_ERR_INVALID for a NULL handle or required input, K < 1, B < 0 (B == 0 is fine
 * and does nothing), total_step < 1, delta_t <= 0, inter_step < 0, a negative first index or overflow of first + count, a
 * required_clearance that is NaN, a plan without a problem, a Qc that is not SPD; GPMP2MI_ERR_UNSUPPORTED, the limit in
 * the message, for inter_step > 63, 2D > 15 and the Pose2 robot kinds; GPMP2MI_ERR_TIMEOUT for a poisoned plan.  The
 * stand-alone call takes at most 524 280 samples per call (one launch); the plan forms have no such limit.
 * Memory: the plan forms run linearize -> export -> the factor-only posterior sweep, then, chunk after chunk on the one
 * stream, the seeded back-substitution into a delta workspace and the kernels of this section.  The chunk is the largest
 * multiple of 16 samples whose delta fits 256 MiB; that workspace (delta chunk, one 32-byte record per sample and 64
 * checked states, the factors Lp and C) is taken at the first call and kept: with the scoring, posterior, seeding and
 * band workspaces the fifth exception to "nothing is allocated after gpmp2mi_plan_create".  The optimizer's records,
 * factors and estimate are not touched.  gpmp2mi_sampled_clearance_traj_dev keeps its records and factors with the robot
 * handle, in the block gpmp2mi_score_traj_dev uses and under its rule. */
enum { GPMP2MI_RNG_BRIDGE = 3 };
/* caller's trajectories and support samples (e.g. from gpmp2mi_block_tridiag_sample or
 * gpmp2mi_plan_sample_posterior_seeded): traj [B][N+1][2D], delta [B][K][N+1][2D], ok [B] or NULL */
int gpmp2mi_sampled_clearance_traj(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, const double* Qc, double delta_t,
                                   int inter_step, int B, int total_step, int K, const double* traj, const double* delta,
                                   const int* ok, uint64_t seed, int row_first, int sample_first, int bridge,
                                   double required_clearance, int* hits, double* probability, double* clearance,
                                   int* worst, double* state_clearance, int* state_hits, int* oor_samples, double* conf);
int gpmp2mi_sampled_clearance_traj_dev(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, const double* Qc,
                                       double delta_t, int inter_step, int B, int total_step, int K, const double* traj,
                                       const double* delta, const int* ok, uint64_t seed, int row_first,
                                       int sample_first, int bridge, double required_clearance, int* hits,
                                       double* probability, double* clearance, int* worst, double* state_clearance,
                                       int* state_hits, int* oor_samples, double* conf, void* stream);
/* the plan at its current estimate, state rules of gpmp2mi_plan_sample_posterior_seeded; ok [B] as there */
int gpmp2mi_plan_collision_probability(gpmp2mi_plan* p, int inter_step, int K, uint64_t seed, int row_first,
                                       int sample_first, int bridge, double required_clearance, int* hits,
                                       double* probability, double* clearance, int* worst, double* state_clearance,
                                       int* state_hits, int* oor_samples, int* ok);
int gpmp2mi_plan_collision_probability_dev(gpmp2mi_plan* p, int inter_step, int K, uint64_t seed, int row_first,
                                           int sample_first, int bridge, double required_clearance, int* hits,
                                           double* probability, double* clearance, int* worst, double* state_clearance,
                                           int* state_hits, int* oor_samples, int* ok, void* stream);
/* the sampled configurations alone: conf [B][K][Md][D] */
int gpmp2mi_plan_sample_dense_seeded(gpmp2mi_plan* p, int inter_step, int K, uint64_t seed, int row_first,
                                     int sample_first, int bridge, double* conf, int* ok);
int gpmp2mi_plan_sample_dense_seeded_dev(gpmp2mi_plan* p, int inter_step, int K, uint64_t seed, int row_first,
                                         int sample_first, int bridge, double* conf, int* ok, void* stream);

/* ---- goal configurations: batched inverse kinematics from a workspace pose, on the device -----------------------------
 * gpmp2mi_plan_set_problem wants end configurations; a manipulation task knows the pose of the hand.  These calls turn
 * G poses into joint configurations by damped least squares from M seeds each, and (gpmp2mi_ik_goals) keep the distinct
 * collision-free answers: the IK branches of a pose (elbow up / down, wrist flips, a redundant arm's null space) are
 * the goals to spread restarts over, and gpmp2mi_plan_select_distinct chooses among what they lead to.
 *
 * Definitions.  One problem = one pose g (des_pose [G][16], row-major 4x4) and one seed row m (seeds [G][M][D]).
 *  1. q = clamp(seed) into [pos_down, pos_up] (min(max(x, down), up) per coordinate; both NULL: no limits);
 *     lambda = lambda_initial, it = 0.
 *  2. (e, H) are the rows of gpmp2mi_workspace_prior_factor(mode, link, des_pose[g]) at q, by the arithmetic of that
 *     entry point (the kernels share one copy of the log maps).  e^, H^ are e, H with the omega rows multiplied by
 *     rot_weight: rows 0..2 for POSE, all rows for ORIENTATION, none for POSITION.  c = sum of e^_r^2, ascending r.
 *  3. converged: POSITION |e| <= pos_tol; ORIENTATION |e| <= rot_tol; POSE |e[0:3]| <= rot_tol && |e[3:6]| <= pos_tol
 *     (|.| = the root of the sum of squares in ascending order, unscaled rows).
 *  4. A non-finite seed or e stops with GPMP2MI_IK_INVALID, conf = the clamped seed.  Otherwise, if converged, stop
 *     with GPMP2MI_IK_CONVERGED.
 *  5. While it < max_iter: A = H^ H^T + lambda I (r x r, r = 3 or 6: the dual form, whatever the dof); Cholesky of A,
 *     y = A^-1 e^, dq = -H^T y, q' = clamp(q + dq); (e', c') at q'; it += 1.  A non-positive or NaN pivot, or a c'
 *     that is not finite, counts as a rejection.  If c' < c: accept (q = q'), lambda = max(lambda / lambda_factor,
 *     lambda_lower), and stop with CONVERGED if converged.  Else lambda = min(lambda * lambda_factor, lambda_upper).
 *  6. Stop with GPMP2MI_IK_MAX_ITER_REACHED.
 *  - Outputs per row: conf [G][M][D] the last accepted q (always inside the limits: the clamp is exact); residual
 *    [G][M][2] = (|omega rows|, |translation rows|) of e there, unscaled, 0 for a part the mode does not have; iters
 *    [G][M] = it; status [G][M].  Any output may be NULL.
 *  - Seeded forms.  Coordinate d of seed row first + m of pose g is down[d] + u * (up[d] - down[d]), the difference,
 *    the product and the sum each rounded once, where u = x * 2^-53 in [0, 1) and x is the hi53 (d & 4 clear) or lo53
 *    (d & 4 set) word of the block that normal(seed, GPMP2MI_RNG_IK, g, first + m, 0, d) of "seeding" reads.  They
 *    need finite limits.
 *  - Goal stage (gpmp2mi_ik_goals): IK as above (seeds given, or drawn when seeds == NULL), then per row
 *      clearance, out_of_range: min_clearance and the count of spheres outside the field of "scoring" for the single
 *        configuration conf; +inf / 0 when sdf == NULL;
 *      eligible = status == CONVERGED && (no field || (clearance >= required_clearance &&
 *                                                       (!require_in_range || out_of_range == 0)));
 *      score = sqrt(sum_d w_d (conf[d] - near[d])^2), or (double)m when near == NULL;
 *      dist(m, m') = sqrt(sum_d w_d (conf_m[d] - conf_m'[d])^2),
 *    both sums by the roundings of s_i in "distinct alternatives" (that section's pair kernel computes dist).  Then
 *    the leader rule of "distinct alternatives" per pose, by that section's rule kernel, over (score, eligible, dist
 *    <= radius).  Per pose: n_goals = number of modes (all of them, also beyond max_goals), n_converged, n_eligible;
 *    goal_conf [G][max_goals][D], goal_seed [G][max_goals] (the leader's m), goal_score, goal_clearance
 *    [G][max_goals] for the first min(n_goals, max_goals) leaders in leader order; beyond that goal_seed = -1 and the
 *    doubles are untouched.  mode [G][M] as in "distinct alternatives".  No angle is wrapped in score or dist.
 *  - Determinism: a row's IK outputs are a function of the robot, the options, its pose and its seed row alone:
 *    bit-identical alone, at any position of any G x M, through the seeded or the given-seed form, through host or
 *    _dev.  One lane per problem, no cross-lane arithmetic, no atomics.
 * Errors, before any device work (a refused call writes nothing): GPMP2MI_ERR_INVALID for a NULL robot / opts /
 * des_pose / seeds, G or M < 0 (0 is fine and does nothing), a tolerance, rot_weight or lambda that is <= 0 or NaN,
 * lambda_lower > lambda_upper, max_iter outside 1..GPMP2MI_IK_MAX_ITER, an unknown mode, a link outside the robot's,
 * one of pos_down / pos_up alone, down > up or a NaN limit, first < 0, infinite or no limits in a seeded form, a
 * negative or NaN radius, a non-finite near, a negative or non-finite weight, a required_clearance that is NaN, max_goals
 * outside 1..GPMP2MI_MAX_ALTERNATIVES, a field whose dimension does not fit.  GPMP2MI_ERR_UNSUPPORTED, the limit in
 * the message, for a robot that is not a GPMP2MI_ROBOT_ARM of dof 1..7 (the Pose2 kinds need a retraction on the base)
 * and, for gpmp2mi_ik_goals, M > GPMP2MI_MAX_GROUP_ROWS.
 * Memory: opts, pos_down / pos_up, near and weights are HOST data in every form, read before the call returns.
 * gpmp2mi_ik_solve*_dev allocate nothing and enqueue one kernel.  gpmp2mi_ik_goals_dev has no handle to keep a
 * workspace with: as gpmp2mi_group_traj_dev it allocates one block (the staged configurations, the bit matrices, a
 * few [G][M] arrays) and waits for `stream` before it frees it -- ONE synchronising allocation per call.  It enqueues
 * the IK kernel, one row kernel, then per pose one launch of the pair kernel and one of the rule kernel (the rule
 * kernel has no batched form), then one copy kernel.
 * Not here: the Pose2 robot kinds and arms of more than 7 joints, angle wrapping in the distances, null-space
 * objectives, self-collision in the eligibility, gpmp2mi_multi_plan_* twins. */
#define GPMP2MI_IK_MAX_ITER 1000
enum { GPMP2MI_IK_CONVERGED = 0, GPMP2MI_IK_MAX_ITER_REACHED = 1, GPMP2MI_IK_INVALID = 2 };
enum { GPMP2MI_RNG_IK = 4 };
typedef struct gpmp2mi_ik_opts {
  int mode;                 /* GPMP2MI_WORKSPACE_POSITION / _ORIENTATION / _POSE */
  int link;                 /* as gpmp2mi_workspace_factor::link */
  double pos_tol, rot_tol;  /* > 0 */
  double rot_weight;        /* > 0: the omega rows are multiplied by it (metres per radian) */
  int max_iter;             /* 1..GPMP2MI_IK_MAX_ITER */
  double lambda_initial, lambda_factor, lambda_lower, lambda_upper;
  const double *pos_down, *pos_up;   /* HOST [dof]; both NULL = unlimited (then the seeded forms are refused) */
} gpmp2mi_ik_opts;
/* POSE, link = 0 (the caller fills in the last link), 1e-6, 1e-6, 1, 100, 1e-2, 4, 1e-9, 1e6, NULL, NULL; NULL: no-op */
void gpmp2mi_ik_opts_default(gpmp2mi_ik_opts* o);
/* des_pose [G][16], seeds [G][M][D] -> conf [G][M][D], residual [G][M][2], iters [G][M], status [G][M] */
int gpmp2mi_ik_solve(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, int G, const double* des_pose, int M,
                     const double* seeds, double* conf, double* residual, int* iters, int* status);
int gpmp2mi_ik_solve_dev(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, int G, const double* des_pose, int M,
                         const double* seeds, double* conf, double* residual, int* iters, int* status, void* stream);
int gpmp2mi_ik_solve_seeded(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, int G, const double* des_pose, int M,
                            uint64_t seed, int first, double* conf, double* residual, int* iters, int* status);
int gpmp2mi_ik_solve_seeded_dev(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, int G, const double* des_pose, int M,
                                uint64_t seed, int first, double* conf, double* residual, int* iters, int* status,
                                void* stream);
/* seeds [G][M][D] or NULL (then drawn from seed / first); sdf may be NULL; near [D], weights [D]: HOST or NULL.
 * Per row: conf, status, clearance, out_of_range, mode [G][M](..[D]); per pose: n_goals, n_converged, n_eligible [G],
 * goal_conf [G][max_goals][D], goal_seed / goal_score / goal_clearance [G][max_goals].  Any output may be NULL. */
int gpmp2mi_ik_goals(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, const gpmp2mi_sdf* sdf, int G,
                     const double* des_pose, int M, const double* seeds, uint64_t seed, int first,
                     double required_clearance, int require_in_range, const double* near_conf, const double* weights,
                     double radius, int max_goals, double* conf, int* status, double* clearance, int* out_of_range,
                     int* mode, int* n_goals, int* n_converged, int* n_eligible, double* goal_conf, int* goal_seed,
                     double* goal_score, double* goal_clearance);
int gpmp2mi_ik_goals_dev(const gpmp2mi_robot* r, const gpmp2mi_ik_opts* o, const gpmp2mi_sdf* sdf, int G,
                         const double* des_pose, int M, const double* seeds, uint64_t seed, int first,
                         double required_clearance, int require_in_range, const double* near_conf, const double* weights,
                         double radius, int max_goals, double* conf, int* status, double* clearance, int* out_of_range,
                         int* mode, int* n_goals, int* n_converged, int* n_eligible, double* goal_conf, int* goal_seed,
                         double* goal_score, double* goal_clearance, void* stream);

/* ---- misc ---------------------------------------------------------------------------------- */
const char* gpmp2mi_last_error(void);  /* thread-local message of the last failing call */
int gpmp2mi_device_count(void);
int gpmp2mi_version(void);
/* Per-kernel timing of the last gpmp2mi_plan_optimize when enabled (HIP events on the plan's
 * stream): names[i] / ms[i] / launches[i] for i < *n.  Used by bench.py for the roofline line. */
int gpmp2mi_plan_enable_timing(gpmp2mi_plan* p, int enable);
int gpmp2mi_plan_get_timing(gpmp2mi_plan* p, int* n, const char** names, double* ms, int* launches);
/* Diagnostic and test entry points (forced kernel forms, failure injection, solver read-outs): gpmp2mi_debug.h */

#ifdef __cplusplus
}
#endif
#endif /* GPMP2MI_H */
