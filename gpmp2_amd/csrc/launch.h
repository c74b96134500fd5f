// launch.h -- host-callable launchers implemented in the .hip translation units.
#pragma once
#include <cstdint>

#include "common.h"

namespace g2 {

// sdf_kernels.hip
constexpr int EDT_INF = 0x3fffffff;   // "no cell of the target set" in the two int32 volumes of squared distances
int launch_sdf_from_occupancy(int nx, int ny, int nz, const double* occ, double cell, int* wa, int* wb,
                              double* field, hipStream_t st);
// the steps of launch_sdf_from_occupancy behind its seed: the three axis passes over two seeded volumes, and
// field = (sqrt(wa) - sqrt(wb)) * cell.  edt_check_axes: the axis limits of the passes, without a launch.
int edt_check_axes(int nx, int ny, int nz);
int launch_edt_passes(int nx, int ny, int nz, int* wa, int* wb, hipStream_t st);
int launch_edt_finish(size_t n, const int* wa, const int* wb, double cell, double* field, hipStream_t st);
// map_kernels.hip (include/gpmp2mi.h "live map"): seeds that take the place of the occupancy seed
// occ [n] -> the two volumes and the obstacle set as one byte per cell
int launch_map_seed_occ(size_t n, const double* occ, int* wa, int* wb, unsigned char* mask, hipStream_t st);
// mask [n] (null: every cell free) -> the two volumes
int launch_map_seed(size_t n, const unsigned char* mask, int* wa, int* wb, hipStream_t st);
// arguments of k_map_mark: M points classified and the kept ones stored into the two volumes
struct MapMark {
  int dim, nx, ny, nz, M, S;
  double ox, oy, oz, cell, margin;
  const double* pts;   // [M][dim]
  const RobotDev* R;   // null: no self filter
  const double* cen;   // [S][3] in the caller's sphere order (launch_sphere_centers, M = 1)
  int *wa, *wb;
  int* cnt;            // [4]: kept, non-finite, self, outside; zeroed by the caller
};
int launch_map_mark(const MapMark& a, hipStream_t st);
// sensor_kernels.hip (include/gpmp2mi.h "sensor map"): the rays of a frame, their walk, and evidence -> seeds
struct SensorGrid {
  int dim, nx, ny, nz;   // nz == 1 for a planar grid
  double ox, oy, oz, cell;
};
// arguments of k_sensor_rays: M rays classified; cell coordinates of the end points and classes to the ray records
struct SensorRays {
  SensorGrid g;
  int M, S;
  double o[3];              // the sensor origin in the world (the unused axis of a planar grid: 0)
  double margin;
  const double* pts;        // [M][dim], the points form
  const float* depth;       // [height][width], the depth form (null: the points form)
  int width;
  double fx, fy, cx, cy, depth_min, depth_max, pose[12];
  const RobotDev* R;        // null: no self filter
  const double* cen;        // [S][3] in the caller's sphere order (launch_sphere_centers, M = 1)
  double* rb;               // [M][3] cell coordinates of the end point
  int* rcls;                // [M] class: hit, invalid, max_range, self, outside
  int* cnt;                 // [5] in that order; zeroed by the caller
};
int launch_sensor_rays(const SensorRays& a, hipStream_t st);
// arguments of k_sensor_walk: the rays of k_sensor_rays walked into the two byte volumes of marks
struct SensorWalk {
  SensorGrid g;
  int M;
  double o[3];
  const double* rb;
  const int* rcls;
  unsigned char *miss, *hit;   // [n] each, all 0 between two calls
};
int launch_sensor_walk(const SensorWalk& a, hipStream_t st);
// arguments of k_sensor_apply: marks -> evidence (marks cleared), the occupied cells counted, the two volumes seeded
struct SensorApply {
  size_t n;
  int hit, miss, lo, hi, occupied_at;
  short* E;                           // [n]
  unsigned char *miss_marks, *hit_marks;
  const unsigned char* mask;          // the base (null: none)
  int *wa, *wb;                       // null: the evidence only
  int* cnt;                           // one word, zeroed by the caller: cells with E' >= occupied_at
};
int launch_sensor_apply(const SensorApply& a, hipStream_t st);
// scene_kernels.hip (include/gpmp2mi.h "scene"): known geometry rasterised into the two seeded volumes or a byte mask.
// A hit stores (0, EDT_INF) into its cell of wa / wb when `mask` is null, else 1 into its byte of `mask`.
constexpr int SCENE_BOX = 0, SCENE_SPHERE = 1, SCENE_CYLINDER = 2, SCENE_MESH = 3;
constexpr int SCENE_PRIM_BATCH = 8;   // primitives of one launch: their records travel as kernel arguments
struct ScenePrim {
  int kind, obj;        // obj: the entry of `cells` the hits are counted in
  int lo[3], n[3];      // the cell box the lanes run over, inside the grid
  double R[9], t[3];    // object -> world, as given
  double s[3];          // size + inflate
};
struct ScenePrims {
  SensorGrid g;
  int count;
  ScenePrim p[SCENE_PRIM_BATCH];
  int *wa, *wb;
  unsigned char* mask;
  int* cells;           // [K], zeroed by the caller
};
int launch_scene_prims(const ScenePrims& a, hipStream_t st);
// one mesh: k_scene_quantize, k_scene_cross, k_scene_fill on `st`
struct SceneMesh {
  SensorGrid g;
  int obj, V, T;
  const double* verts;  // [V][3], object frame
  const int* tris;      // [T][3]
  int* q;               // [V][3] fixed-point grid coordinates of this call
  double pose[12];
  int* flag;            // one word, zeroed by the caller: a vertex is out of range
  unsigned* bits;       // [nz][ny][W] crossing bits, all 0 between two meshes
  int W;                // words per row: nx rounded up to 32 bits
  int *wa, *wb;
  unsigned char* mask;
  int* cells;           // [K]
};
int launch_scene_mesh(const SceneMesh& a, hipStream_t st);
// factor_kernels.hip
int launch_sdf_pack(const SdfDev& s, double* cells, hipStream_t st);
int launch_sdf_query(const SdfDev& s, int M, const double* pts, double* dist, double* grad, int* inr,
                     hipStream_t st);
// ld: leading dimension of conf (0 = dof; 2 dof reads the configurations out of trajectory states)
int launch_sphere_centers(const RobotDev& h, const RobotDev* R, int M, const double* conf, double* c,
                          double* J, hipStream_t st, int ld = 0);
int launch_fk(const RobotDev& h, const RobotDev* R, int M, const double* conf, double* poses, double* J,
              hipStream_t st, int ld = 0);
int launch_obstacle(const RobotDev& h, const RobotDev* R, const SdfDev& s, double eps, int M,
                    const double* conf, double* err, double* H1, hipStream_t st);
int launch_obstacle_gp(const RobotDev& h, const RobotDev* R, const SdfDev& s, double eps, const GpCoef& gc,
                       int M, const double* c1, const double* v1, const double* c2, const double* v2,
                       double* err, double* H1, double* H2, double* H3, double* H4, hipStream_t st);
int launch_gp_prior_linear(int D, double dt, int M, const double* c1, const double* v1, const double* c2,
                           const double* v2, double* err, double* H1, double* H2, double* H3, double* H4,
                           hipStream_t st);
int launch_gp_interp_linear(int D, const GpCoef& gc, int M, const double* c1, const double* v1,
                            const double* c2, const double* v2, double* conf, double* vel, hipStream_t st);
int launch_gp_prior_lie(int D, double dt, int M, const double* c1, const double* v1, const double* c2,
                        const double* v2, double* err, double* H1, double* H2, double* H3, double* H4,
                        hipStream_t st);
int launch_interpolate_traj(int D, bool lie, double dt, int inter, int B, int N, int start, int Mo,
                            const double* traj, double* out, hipStream_t st);
int launch_vehicle_dynamics(int D, int lie, int M, const double* conf, const double* vel, double* err, double* Hp,
                            double* Hv, hipStream_t st);
int launch_workspace_prior(int mode, int joint, int L, int D, int M, const double* des, const double* poses,
                           const double* Jp, double* err, double* H, hipStream_t st);
int launch_self_collision(int n, int S, int D, int M, const double* data, const double* radius, const double* c,
                          const double* Jc, double* err, double* H, hipStream_t st);
int launch_gp_interp_lie(int D, const GpCoef& gc, int M, const double* c1, const double* v1, const double* c2,
                         const double* v2, double* conf, double* vel, hipStream_t st);
int launch_joint_limit(int D, const double* down, const double* up, const double* th, int M,
                       const double* x, double* err, double* Hd, hipStream_t st);

// score_kernels.hip
constexpr int SCORE_TILE = 64;   // checked states per workgroup of k_score: fixes the summation order
// what one workgroup of k_score leaves for k_score_finish; k = s = INT_MAX: no pair of the tile was in range
struct ScoreRec {
  double support, dense, clearance;
  int k, s, oor, pad;
};
// arguments of k_score_finish; every output may be null
struct ScoreFinish {
  int B, N, D, lie, inter, Md, nblk;
  double dt;
  const ScoreRec* recs;              // [B][nblk], or null: selection over in_clearance / in_oor
  const double* in_clearance;
  const int* in_oor;
  double *support, *dense, *clearance;
  int *worst, *oor;
  int select, require_in_range;      // select: one workgroup applies the rule over the B rows
  double required_clearance;
  const double* ferr;
  const int* status;
  int *best, *n_eligible;
  double* best_err;                  // final_error of the chosen row (left alone when none is)
  const double* traj;                // [B][N+1][2D]: the rows traj_best / dense_best are taken from
  double *traj_best, *dense_best;
};
int score_blocks(int Md);   // records per row
int launch_score(const RobotDev& h, const RobotDev* R, const SdfDev& s, double dt, int inter, int B, int N,
                 const double* traj, ScoreRec* recs, hipStream_t st);
int launch_score_finish(const ScoreFinish& a, hipStream_t st);

// self_clearance_kernels.hip (include/gpmp2mi.h "self-collision check")
// one row of a pair table on the device: sorted-order sphere indices and radius_A + radius_B + epsilon.  16 bytes.
struct SelfPair {
  double total_eps;
  int a, b;
};
// Checked states per workgroup of k_self_clearance: LDS holds 24 S bytes per state, so the tile shrinks as the sphere
// model grows.  A function of S alone (it fixes the summation order); a power of two <= 64.
inline int self_tile(int S) { return S <= 32 ? 64 : S <= 64 ? 32 : 16; }
inline int self_blocks(int Md, int S) { return (Md + self_tile(S) - 1) / self_tile(S); }   // records per row
// arguments of k_self_finish.  The records of k_self_clearance are ScoreRecs: s is the row of the caller's pair table,
// oor the number of invalid (state, pair)s.  `sel` carries the selection (sel.select) with the records of k_score for
// the same rows (sel.recs, sel.nblk) and the shape of the trajectories; its per-row outputs are not written.
struct SelfFinish {
  ScoreFinish sel;
  const ScoreRec* recs;   // [B][nblk]
  int nblk;
  double *support, *dense, *clearance;
  int *worst, *invalid;
  double required_self_clearance;
};
int launch_self_clearance(const RobotDev& h, const RobotDev* R, const SelfPair* pairs, int P, double dt, int inter, int B,
                          int N, const double* traj, ScoreRec* recs, hipStream_t st);
int launch_self_finish(const SelfFinish& a, hipStream_t st);

// motion_kernels.hip (include/gpmp2mi.h "motion limits")
// the limits as k_motion reads them, a kernel argument: +-inf where there is none
struct MotionLimitsDev {
  double down[GPMP2MI_MAX_DOF], up[GPMP2MI_MAX_DOF], vel[GPMP2MI_MAX_DOF], acc[GPMP2MI_MAX_DOF];
};
// What one workgroup of k_motion leaves for k_motion_finish: the four extrema of its tile of SCORE_TILE checked states,
// each with its two indices, and the count of non-finite quantities.  v[0]: the smallest position margin; v[1..3]: MINUS
// the largest velocity ratio, acceleration ratio and point speed, so that all four are minima under key_less
// (score_select.h) and exact ties go to the lowest indices.  ij = INT_MAX: none.  72 bytes.
struct MotionRec {
  double v[4];
  int ij[4][2];
  int invalid, pad;
};
// arguments of k_motion_finish; every output may be null.  `sel` carries the selection (sel.select) and the shape of the
// trajectories; the rule reads the per-row scores the existing stages left: clearance / oor (k_score_finish) and, when
// self_clearance is given, self_clearance / self_invalid (k_self_finish).
struct MotionFinish {
  ScoreFinish sel;
  const MotionRec* recs;   // [B][nblk]
  int nblk;
  double limit_point_speed;
  double *pos_margin, *vel_ratio, *acc_ratio, *point_speed, *time_scale;
  int *worst, *invalid;    // [B][4][2], [B]
  const double *clearance, *self_clearance;
  const int *oor, *self_invalid;
  double required_self_clearance, required_pos_margin, max_time_scale;
  double* time_scale_best;
};
// records per row: score_blocks
int launch_motion(const RobotDev& h, const RobotDev* R, const MotionLimitsDev& lim, double dt, int inter, int B, int N,
                  const double* traj, MotionRec* recs, hipStream_t st);
int launch_motion_finish(const MotionFinish& a, hipStream_t st);

// retime_kernels.hip (include/gpmp2mi.h "re-timing")
// ps [B][Md]: the largest sphere speed of every checked state (NaN where one is not finite); fixed-base kinds only
int launch_retime_caps(const RobotDev& h, const RobotDev* R, double dt, int inter, int B, int N, const double* traj,
                       double* ps, hipStream_t st);
// arguments of k_retime.  The trajectory form reads traj / ps and the limits vel / point_speed; the path form reads the
// caller's qd / ql / qr [B][Md][D] and cap [B][Md].  acc / vel: +inf where there is no limit.  X [B][Md] and K [B][Md][2]
// are workspace; sdot, u and stamps [B][Md] are never null (sdot carries x on the way); the other outputs may be.
struct RetimeArgs {
  int B, Md, D, N, inter;
  double dt, h, max_rate, rate_start, rate_end, point_speed;
  double acc[GPMP2MI_MAX_DOF], vel[GPMP2MI_MAX_DOF];
  const double *traj, *ps;
  const double *qd, *ql, *qr, *cap;
  double *X, *K;
  double *sdot, *u, *stamps, *duration, *achieved, *dense;
  int* status;
};
int launch_retime(const RetimeArgs& a, bool traj, hipStream_t st);
// arguments of k_retime_finish (one workgroup): `sel` carries the selection and the shape of the trajectories; the rule
// reads the per-row scores the existing stages left, as MotionFinish does, and what k_retime left.
struct RetimeFinish {
  ScoreFinish sel;
  const double *clearance, *self_clearance, *pos_margin;
  const int *oor, *self_invalid, *motion_invalid;
  const int* rstatus;
  const double *duration, *sdot, *stamps;   // [B], [B][Md], [B][Md]
  double required_self_clearance, required_pos_margin, max_duration;
  double *duration_best, *stamps_best;
};
int launch_retime_finish(const RetimeFinish& a, hipStream_t st);

// torque_kernels.hip (include/gpmp2mi.h "torque limits")
// the inertial table of a fixed-base arm as k_torque reads it: lives in HBM once per dynamics handle, staged into LDS
// by every workgroup as RobotDev is.  Link j carries mass[j], its centre of mass com[3 j ..] in the link frame and
// inertia[6 j ..] = ixx iyy izz ixy ixz iyz about that centre, link frame.
constexpr int TORQUE_MAX_AD = 8;   // k_torque is instantiated for fixed-base arms of 1..8 joints
struct DynDev {
  double mass[TORQUE_MAX_AD], com[TORQUE_MAX_AD * 3], inertia[TORQUE_MAX_AD * 6];
};
// the torque limits and gravity as k_torque reads them, a kernel argument: +inf where there is no limit
struct TorqueLimitsDev {
  double limit[TORQUE_MAX_AD], gravity[3];
};
// What one workgroup of k_torque leaves for k_torque_finish: MINUS the largest |tau| / L, |tau_g| / L and r of its tile
// of SCORE_TILE checked states (minima under key_less, exact ties to the lowest indices), each with its (state, joint),
// and the count of non-finite torques.  ij = INT_MAX: none.  56 bytes.
struct TorqueRec {
  double v[3];
  int ij[3][2];
  int invalid, pad;
};
// arguments of k_torque_finish; every output may be null.  `sel` carries the selection (sel.select) and the shape of the
// trajectories; the rule reads the per-row scores the existing stages left, as RetimeFinish does, and the motion stage's
// time_scale.  tau: what k_torque wrote, [B][Md][D], the source of tau_best.
struct TorqueFinish {
  ScoreFinish sel;
  const TorqueRec* recs;   // [B][nblk]
  int nblk;
  double *torque_ratio, *static_ratio, *time_scale;
  int *worst, *invalid;    // [B][3][2], [B]
  const double *clearance, *self_clearance, *pos_margin, *motion_time_scale;
  const int *oor, *self_invalid, *motion_invalid;
  double required_self_clearance, required_pos_margin, max_time_scale;
  const double* tau;
  double *time_scale_best, *tau_best;
};
// records per row: score_blocks.  tau: [B][Md][D] or null
int launch_torque(const RobotDev& h, const RobotDev* R, const DynDev* dyn, const TorqueLimitsDev& lim, double dt, int inter,
                  int B, int N, const double* traj, TorqueRec* recs, double* tau, hipStream_t st);
int launch_torque_finish(const TorqueFinish& a, hipStream_t st);

// retime_dynamic_kernels.hip (include/gpmp2mi.h "re-timing under torque limits")
constexpr int RETIME_DYN_MAX_ROWS = 8;   // affine rows per state and side: one per joint of k_torque's arms
// coef [B][Md][4][D] = p, m_left, m_right, tau_g of every checked state: tau = p u + m x + tau_g along the path
int launch_retime_coef(const RobotDev& h, const RobotDev* R, const DynDev* dyn, const TorqueLimitsDev& lim, double dt,
                       int inter, int B, int N, const double* traj, double* coef, hipStream_t st);
// arguments of k_retime_rows and k_retime_dynamic: those of k_retime, and R affine rows |cx x + cu u + off| <= bound per
// state.  cxl / cxr / cu / off: element r of state k of row b at [(b Md + k) stride + r] (the caller's arrays: stride R;
// the four blocks of coef: stride 4 D).  rows [B][Md][2 D + 2 R][4] is workspace; tau [B][Md][D] or null (trajectory
// form: the affine rows are the torques).  achieved is [B][6].  nonfinite [B] or null: 1 where one of a row's
// coefficients is not finite, whether its row has a bound or not.
struct RetimeDynArgs {
  RetimeArgs rt;
  int R, stride;
  double bound[RETIME_DYN_MAX_ROWS];
  const double *cxl, *cxr, *cu, *off;
  double *rows, *tau;
  int* nonfinite;
};
int launch_retime_dynamic(const RetimeDynArgs& a, bool traj, hipStream_t st);
// arguments of k_retime_dynamic_finish (one workgroup): RetimeFinish, and the coefficients' flag and the torques of
// every re-timed row, the source of tau_best
struct RetimeDynFinish {
  RetimeFinish rt;
  const int* nonfinite;   // [B]
  const double* tau;      // [B][Md][D]
  double* tau_best;
};
int launch_retime_dynamic_finish(const RetimeDynFinish& a, hipStream_t st);

// moving_kernels.hip (include/gpmp2mi.h "moving obstacles"; the in-plan factor's launcher is in plan.h)
// the factor on M evaluations: cen / Jc from launch_sphere_centers, robot_radius [S] in the caller's sphere order,
// centers [M][K][3] -> err [M][S][K], H [M][S][K][D] or null
int launch_moving_factor(int S, int D, int K, int M, const double* robot_radius, const double* radius, double eps,
                         const double* centers, const double* cen, const double* Jc, double* err, double* H,
                         hipStream_t st);
// arguments of k_moving_finish.  The records of k_moving_clearance are ScoreRecs by the tiling of k_self_clearance
// (self_tile, self_blocks): s is the pair index sphere * K + moving sphere, oor the number of invalid pairs.  `sel`
// carries the selection (sel.select) and the shape of the trajectories; the rule reads the per-row scores the existing
// stages left, as MotionFinish does.
struct MovingFinish {
  ScoreFinish sel;
  const ScoreRec* recs;   // [B][nblk]
  int nblk, K;
  double *support, *dense, *min_clearance;
  int *worst, *invalid;   // [B][3], [B]
  const double *clearance, *self_clearance;
  const int *oor, *self_invalid;
  double required_self_clearance, required_moving_clearance;
};
// radius [K], centers [K][N+1][3]
int launch_moving_clearance(const RobotDev& h, const RobotDev* R, int K, const double* radius, const double* centers,
                            double eps, double dt, int inter, int B, int N, const double* traj, ScoreRec* recs,
                            hipStream_t st);
int launch_moving_finish(const MovingFinish& a, hipStream_t st);

// carried_kernels.hip (include/gpmp2mi.h "carried object"; the in-plan factor's launcher is in plan.h)
// the factor on M evaluations: radius [A], centers [A][3] in the frame of `link`, conf [M][D] -> err [M][A],
// H [M][A][D] or null
int launch_carried_factor(const RobotDev& h, const RobotDev* R, const SdfDev& s, int link, int A, const double* radius,
                          const double* centers, double eps, int M, const double* conf, double* err, double* H,
                          hipStream_t st);
// arguments of k_carried_finish.  The records of k_carried_clearance are ScoreRecs by the tiling of k_score
// (score_blocks): s is the carried sphere, oor the number of out-of-range (state, sphere)s.  `sel` carries the selection
// (sel.select) and the shape of the trajectories; the rule reads the per-row scores the existing stages left, as
// MovingFinish does (obs_oor: the obstacle stage's out-of-range count).
struct CarriedFinish {
  ScoreFinish sel;
  const ScoreRec* recs;   // [B][nblk]
  int nblk;
  double *support, *dense, *min_clearance;
  int *worst, *oor;       // [B][2], [B]
  const double *clearance, *self_clearance;
  const int *obs_oor, *self_invalid;
  double required_self_clearance, required_carried_clearance;
};
int launch_carried_clearance(const RobotDev& h, const RobotDev* R, const SdfDev& s, int link, int A, const double* radius,
                             const double* centers, double dt, int inter, int B, int N, const double* traj,
                             ScoreRec* recs, hipStream_t st);
int launch_carried_finish(const CarriedFinish& a, hipStream_t st);

// path_kernels.hip (include/gpmp2mi.h "workspace path"; the in-plan factor's launcher is in plan.h)
// the factor on M evaluations, one target per evaluation: conf [M][D], des [M][16] -> err [M][rows], H [M][rows][D] or
// null (rows = 6 for the POSE mode, else 3)
int launch_path_factor(const RobotDev& h, const RobotDev* R, int mode, int link, int M, const double* conf,
                       const double* des, double* err, double* H, hipStream_t st);
// sigma [N+1] -> the states with a finite sigma, ascending, and their count
int launch_path_list(int N, const double* sigma, int* list, int* count, hipStream_t st);
// what one workgroup of k_path_deviation (64 checked states) leaves for k_path_finish; kp / kr = INT_MAX: no state of
// the tile was checked for that deviation
struct PathRec {
  double support, dense, pos, rot;
  int kp, kr, inv, pad;
};
// arguments of k_path_finish; every output may be null.  `sel` carries the selection (sel.select) and the shape of the
// trajectories; the rule reads the per-row scores the obstacle stage left, as MovingFinish does.
struct PathFinish {
  ScoreFinish sel;
  const PathRec* recs;   // [B][nblk]
  int nblk;
  double *max_pos, *max_rot, *support, *dense;
  int *worst, *invalid;   // [B][2], [B]
  const double* clearance;
  const int* oor;
  double allowed_pos, allowed_rot;
};
int path_blocks(int Md);   // records per row
// des [N+1][16], sigma [N+1]
int launch_path_deviation(const RobotDev& h, const RobotDev* R, int mode, int link, const double* des, const double* sigma,
                          double dt, int inter, int B, int N, const double* traj, PathRec* recs, hipStream_t st);
int launch_path_finish(const PathFinish& a, hipStream_t st);

// group_kernels.hip (include/gpmp2mi.h "distinct alternatives")
constexpr int GROUP_TILE = 64;         // k_traj_pairs: one workgroup per 64 x 64 tile of pairs
constexpr int GROUP_CHUNK_ELEMS = 32;   // configuration doubles of a row staged through LDS at a time
// support states per LDS chunk: whole states only, so that s_i closes inside a chunk
constexpr int group_chunk_states(int D) { return D >= GROUP_CHUNK_ELEMS ? 1 : GROUP_CHUNK_ELEMS / D; }
// arguments of k_traj_pairs; dist [B][B] and bits [B][ceil(B/64)] are both optional
struct PairArgs {
  int B, N, D, metric;
  const double* traj;           // [B][N+1][2D]
  double w[GPMP2MI_MAX_DOF];    // the weights, 1 where the caller gave none
  double radius;
  double* dist;
  unsigned long long* bits;
};
int launch_traj_pairs(const PairArgs& a, hipStream_t st);
// arguments of k_group_rule (one workgroup).  Adjacency: `bits`, or dist <= radius for a given matrix.  Eligibility:
// `eligible` (null: all 1), or with `plan_rule` the rule of "scoring" over status / ferr (= score) / clearance / oor,
// extended by the self scores when self_clearance is given.  Every output may be null.
struct GroupRule {
  int B, plan_rule, require_in_range;
  double radius, required_clearance, required_self_clearance;
  const double* dist;
  const unsigned long long* bits;
  const double* score;
  const int* eligible;
  const int* status;
  const double* clearance;
  const int* oor;
  const double* self_clearance;
  const int* self_invalid;
  int *mode, *leaders, *sizes, *n_modes, *n_eligible;
};
int launch_group_rule(const GroupRule& a, hipStream_t st);
// arguments of k_group_copy: one workgroup per alternative, reading what k_group_rule left
struct GroupCopy {
  int N, D, lie, inter, Md, max_alt;
  double dt;
  const double* traj;   // [B][N+1][2D]
  const double* ferr;
  const int *leaders, *sizes, *n_modes, *n_eligible;
  int *out_n_modes, *out_n_eligible;   // the caller's copies of the two counts
  int *alt, *alt_size;
  double *alt_error, *traj_alt, *dense_alt;
};
int launch_group_copy(const GroupCopy& a, hipStream_t st);

// ik_kernels.hip (include/gpmp2mi.h "goal configurations")
constexpr int IK_MAX_DOF = 7;   // k_ik is instantiated for fixed-base arms of 1..7 joints
// arguments of k_ik: G * M problems, one lane each.  seeds == null: the seed rows are drawn (seed, first).
struct IkArgs {
  int G, M, mode, link, max_iter, first;
  double pos_tol, rot_tol, rot_weight, lam0, lam_factor, lam_lo, lam_hi;
  double down[IK_MAX_DOF], up[IK_MAX_DOF];   // -inf / +inf: no limit
  uint64_t seed;
  const double* des;     // [G][16]
  const double* seeds;   // [G][M][D] or null
  double *conf, *residual;
  int *iters, *status;
};
int launch_ik(const RobotDev& h, const RobotDev* R, const IkArgs& a, hipStream_t st);
// arguments of k_ik_rows (one lane per row: clearance of conf, eligibility, score, the row staged as a one-state
// trajectory for k_traj_pairs) and k_ik_goal_copy (one workgroup per pose, reading what k_group_rule left)
struct IkRows {
  int G, M, has_near, require_in_range;
  double required_clearance;
  double near_conf[IK_MAX_DOF], w[IK_MAX_DOF];
  const double* conf;    // [G][M][D]
  const int* status;
  double *clearance, *score, *stage;   // [G][M], [G][M], [G][M][2D]
  int *oor, *eligible;
};
int launch_ik_rows(const RobotDev& h, const RobotDev* R, const SdfDev* s, const IkRows& a, hipStream_t st);
struct IkGoalCopy {
  int M, D, max_goals;
  const double *conf, *score, *clearance;
  const int *status, *leaders, *n_modes, *n_eligible;   // leaders [G][M], n_modes / n_eligible [G]
  int *n_goals, *n_converged, *out_n_eligible, *goal_seed;
  double *goal_conf, *goal_score, *goal_clearance;
};
int launch_ik_goal_copy(const IkGoalCopy& a, int G, hipStream_t st);

// risk_kernels.hip
// what one workgroup of k_risk leaves for k_risk_finish; k = s = INT_MAX: no pair of the tile was in range
struct RiskRec {
  double c, sigma;   // the smallest clearance - kappa sigma of the tile, and sigma at that pair
  int k, s, oor, pad;
};
// arguments of k_risk_finish; every output may be null
struct RiskFinish {
  int B, nblk;
  const RiskRec* recs;   // [B][nblk]
  const int* ok;         // null: every row is fine
  double *robust, *sigma_worst;
  int *worst, *oor;
};
// Sd [B][N+1][n][n], So [B][N][n][n] -> cov [B][N (inter + 1) + 1][n][n], n = 2 D; Qc [D][D] or null (identity)
int launch_gp_interp_cov(int D, const double* Qc, double dt, int inter, int B, int N, const double* Sd, const double* So,
                         double* cov, hipStream_t st);
// records per row: score_blocks.  sigma: [B][Md][S] or null
int launch_risk(const RobotDev& h, const RobotDev* R, const SdfDev& s, const double* Qc, double dt, int inter, int B,
                int N, double kappa, const double* traj, const double* Sd, const double* So, const int* ok, double* sigma,
                RiskRec* recs, hipStream_t st);
int launch_risk_finish(const RiskFinish& a, hipStream_t st);

// sample_clearance_kernels.hip (include/gpmp2mi.h "sampled clearance")
constexpr int SAMPLED_MAX_INTER = 63;                 // inter_step limit: Lp is (J + 1) J / 2 <= 2 016 doubles of LDS
#ifndef G2_SAMPLED_PER_WG
#define G2_SAMPLED_PER_WG 8                           // -DG2_SAMPLED_PER_WG=4 / 16: the builds scripts/sampled_throughput.py compares
#endif
constexpr int SAMPLED_PER_WG = G2_SAMPLED_PER_WG;     // samples a workgroup of k_sampled_clearance loops over (4, 8 and 16
                                                      // measured: profiles/sampled_throughput.json)
constexpr size_t SAMPLED_CHUNK_BYTES = 256ull << 20;  // byte budget of a plan's delta chunk (host/sampled.hip)
// what one wavefront of k_sampled_clearance leaves for k_sampled_finish per (row, sample, tile); k = s = INT_MAX: no
// pair of the tile was in range.  32 bytes.
struct SampledRec {
  double c;
  int k, s, oor, pad0, pad1, pad2;   // oor: 1 when a pair of the tile was out of range
};
// arguments of k_sampled_clearance: one chunk of `cnt` samples, s0 .. s0 + cnt - 1 of the call's K.  Outputs may be null.
struct SampledArgs {
  double dt, required;
  uint64_t seed;
  int inter, B, N, Md, nblk;
  int K, s0, cnt;                    // K: the call's samples = the sample stride of the outputs
  int row_first, sample_first, bridge;
  const double* est;                 // [B][N+1][2D]
  const double* delta;               // [B][cnt][N+1][2D]
  const int* ok;                     // [B] or null
  const double *Lp, *C;              // packed lower factor of the bridge (row j, column j' at (j-1) j / 2 + j' - 1); [D][D]
  SampledRec* recs;                  // [B][cnt][nblk]
  double* state_clearance;           // [B][K][Md]
  int* state_hits;                   // [B][Md], zeroed ahead of the first chunk
  double* conf;                      // [B][K][Md][D]
};
// arguments of k_sampled_finish for the same chunk; first / last: the call's first / last chunk
struct SampledFinish {
  int B, Md, nblk, K, s0, cnt, first, last;
  double required;
  const SampledRec* recs;
  const int* ok;
  int* acc;                          // [B][2]: hits and oor_samples so far
  int *hits, *worst, *state_hits, *oor_samples;
  double *probability, *clearance;
};
int launch_sampled_clearance(const RobotDev& h, const RobotDev* R, const SdfDev& s, const SampledArgs& a, hipStream_t st);
int launch_sampled_finish(const SampledFinish& a, hipStream_t st);

}  // namespace g2
