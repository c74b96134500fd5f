// launch.h -- host-callable launchers implemented in the .hip translation units.
#pragma once
#include "common.h"

namespace g2 {

// sdf_kernels.hip
int launch_sdf_from_occupancy(int nx, int ny, int nz, const double* occ, double cell, int* wa, int* wb,
                              double* field, hipStream_t st);
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

}  // namespace g2
