// path_kernels.hip -- workspace path (include/gpmp2mi.h "workspace path"): one target pose and one sigma per support
// state, the rows of GaussianPriorWorkspace{Position,Orientation,Pose} against it.
//
//   k_path_factor      the factor on M evaluations (gpmp2mi_workspace_path_factor): one wavefront per evaluation, the
//                      device functions of k_path_accumulate, rows to err / H.
//   k_path_list        the constrained states (finite sigma) of a path set from device buffers, ascending, and their count.
//   k_path_accumulate  the factor inside a plan.  One wavefront per (trajectory, constrained state).  Every lane walks
//                      the chain to the link (the walk is uniform over the wavefront, so it costs what one lane's walk
//                      costs); lane k < D forms column k of the link's body Jacobian and of the <= 6 rows, and leaves it
//                      in LDS beside the residual.  Every lane then adds the rows, in ascending order, to the record
//                      entries it owns (RecAcc, record_entries.h) and writes them once.  No poses, no Jacobians and no
//                      rows reach memory.
//   k_path_deviation   the check of the executed trajectory: a lane is a checked state (checked_config, score_select.h),
//                      ONE record per workgroup of 64.
//   k_path_finish      reduces a row's records in index order to the outputs and, when asked, applies the selection rule
//                      over the per-row scores of the obstacle stage.
//
// Determinism: a state's contribution is a function of (D, mode, link) and its own data: one accumulator per record
// entry, rows in ascending order, no atomics.  The check sums in an order fixed by (N, inter_step).
#include <climits>

#include "device_math.h"
#include "dispatch.h"
#include "launch.h"
#include "lie_log.h"
#include "link_frame.h"
#include "plan.h"
#include "record_entries.h"
#include "score_select.h"

namespace g2 {

namespace {

__device__ __forceinline__ void pose_rt(const double* T, double (&Rm)[9], double (&t)[3]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) Rm[i * 3 + j] = T[i * 4 + j];
    t[i] = T[i * 4 + 3];
  }
}
// between(des, pose): Rrel = Rd^T Rm, trel = Rd^T (t - td)
__device__ __forceinline__ void pose_between(const double (&Rd)[9], const double (&td)[3], const double (&Rm)[9],
                                             const double (&t)[3], double (&Rrel)[9], double (&trel)[3]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double a = 0;
#pragma unroll
      for (int c = 0; c < 3; c++) a += Rd[c * 3 + i] * Rm[c * 3 + j];
      Rrel[i * 3 + j] = a;
    }
    trel[i] = Rd[i] * (t[0] - td[0]) + Rd[3 + i] * (t[1] - td[1]) + Rd[6 + i] * (t[2] - td[2]);
  }
}

// The rows of k_workspace_prior (factor_kernels.hip) for the link frame F against `des` (row-major 4x4): the residual
// e [rows] and, for one column `col` of the link's body Jacobian, that column h [rows] of the rows' Jacobian.  The
// entries past `rows` are zero.  jac = false: e only.
__device__ __forceinline__ void path_rows(int mode, const Frame& F, const double* des, const double (&col)[6], bool jac,
                                          double (&e)[6], double (&h)[6]) {
  double Rm[9], t[3], Rd[9], td[3];
  frame_rt(F, Rm, t);
  pose_rt(des, Rd, td);
#pragma unroll
  for (int i = 0; i < 6; i++) e[i] = h[i] = 0.0;
  if (mode == GPMP2MI_WORKSPACE_POSITION) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
      e[i] = t[i] - td[i];
      double a = 0;
#pragma unroll
      for (int c = 0; c < 3; c++) a += Rm[i * 3 + c] * col[3 + c];   // Pose3::translation(H) = [0 R]
      h[i] = a;
    }
    return;
  }
  double Rrel[9], trel[3];
  pose_between(Rd, td, Rm, t, Rrel, trel);
  if (mode == GPMP2MI_WORKSPACE_ORIENTATION) {
    double w[3], Her[9];
    rot3_logmap(Rrel, w);
#pragma unroll
    for (int i = 0; i < 3; i++) e[i] = w[i];
    if (!jac) return;
    rot3_logmap_derivative(w, Her);   // Pose3::rotation(H) = [I 0]
#pragma unroll
    for (int i = 0; i < 3; i++) {
      double a = 0;
#pragma unroll
      for (int c = 0; c < 3; c++) a += Her[i * 3 + c] * col[c];
      h[i] = a;
    }
    return;
  }
  double xi[6];
  pose3_logmap(Rrel, trel, xi);
#pragma unroll
  for (int i = 0; i < 6; i++) e[i] = xi[i];
  if (!jac) return;
  double Hep[36];
  pose3_logmap_derivative(xi, Hep);
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double a = 0;
#pragma unroll
    for (int c = 0; c < 6; c++) a += Hep[i * 6 + c] * col[c];
    h[i] = a;
  }
}

// (max deviation, state): the larger deviation, on exact ties the lower state; "none" is (-inf, INT_MAX)
__device__ __forceinline__ bool dev_greater(double a, int ka, double b, int kb) { return a > b || (a == b && ka < kb); }

}  // namespace

template <int KIND, int AD, int AD2>
__global__ __launch_bounds__(64) void k_path_factor(const RobotDev* __restrict__ Rg, int mode, int link, int M,
                                                     const double* __restrict__ conf, const double* __restrict__ des,
                                                     double* __restrict__ err, double* __restrict__ H) {
  using Kn = Kin<KIND, AD, AD2>;
  constexpr int D = Kn::DOF;
  __shared__ RobotDev R;
  stage_robot(&R, Rg);
  const size_t m = blockIdx.x;   // grid = M
  const int lane = threadIdx.x, rows = mode == GPMP2MI_WORKSPACE_POSE ? 6 : 3;
  double q[D];
#pragma unroll
  for (int k = 0; k < D; k++) q[k] = conf[m * D + k];
  typename Kn::Axes A;
  Frame F;
  int nc, first;
  link_frame<KIND, AD, AD2>(R, q, link, A, F, nc, first);
  double col[6], e[6], h[6];
  link_twist<KIND, AD, AD2>(A, F, nc, first, lane, col);
  path_rows(mode, F, des + m * 16, col, H != nullptr, e, h);
#pragma unroll
  for (int r = 0; r < 6; r++) {
    if (r >= rows) break;
    if (lane == 0) err[m * rows + r] = e[r];
    if (H && lane < D) H[(m * rows + r) * D + lane] = h[r];
  }
}

__global__ void k_path_list(int N, const double* __restrict__ sigma, int* __restrict__ list, int* __restrict__ count) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int n = 0;
  for (int i = 0; i <= N; i++)
    if (isfinite(sigma[i])) list[n++] = i;
  *count = n;
}

constexpr int WP_LD = MAXD + 2;   // an LDS row: h [D], then r

template <int KIND, int AD, int AD2>
__global__ __launch_bounds__(64) void k_path_accumulate(const RobotDev* __restrict__ Rg, const PlanParams* __restrict__ pp,
                                                         PlanBuffers pb, PlanExtras ex, const double* __restrict__ traj,
                                                         int bufsel, const int* __restrict__ active) {
  using Kn = Kin<KIND, AD, AD2>;
  constexpr int D = Kn::DOF;
  __shared__ RobotDev R;
  __shared__ double rows[6][WP_LD];
  stage_robot(&R, Rg);
  const PlanParams& P = *pp;
  const int N = P.N;
  const int nst = ex.wp_n;   // wavefronts per trajectory: the entries of wp_list this launch may look at
  const int b = blockIdx.x / nst, jl = blockIdx.x % nst;
  if (jl >= *ex.wp_count) return;   // after the _dev setter the count is known to the device only
  if (active && !active[b]) return;
  const int i = ex.wp_list[jl];
  const int lane = threadIdx.x, nrow = ex.wp_mode == GPMP2MI_WORKSPACE_POSE ? 6 : 3;
  const double sg = ex.wp_sigma[i], w = 1.0 / (sg * sg);
  double q[D];
  const double* x = traj + ((size_t)b * (N + 1) + i) * 2 * D;
#pragma unroll
  for (int k = 0; k < D; k++) q[k] = x[k];
  typename Kn::Axes A;
  Frame F;
  int nc, first;
  link_frame<KIND, AD, AD2>(R, q, ex.wp_link, A, F, nc, first);
  double col[6], e[6], h[6];
  link_twist<KIND, AD, AD2>(A, F, nc, first, lane, col);
  path_rows(ex.wp_mode, F, ex.wp_des + (size_t)i * 16, col, true, e, h);
#pragma unroll
  for (int r = 0; r < 6; r++) {
    if (lane < D) rows[r][lane] = h[r];
    if (lane == D) rows[r][D] = e[r];   // e is the same in every lane
  }
  RecAcc acc(D, P.NG);
  __syncthreads();
  for (int r = 0; r < nrow; r++) acc.add(w, rows[r]);   // rows in ascending order
  acc.store(pb, b, i, bufsel, P);
}

template <int KIND, int AD, int AD2>
__global__ __launch_bounds__(64) void k_path_deviation(const RobotDev* __restrict__ Rg, int mode, int link,
                                                        const double* __restrict__ des, const double* __restrict__ sigma,
                                                        double dt, int inter, int N, int Md, int nblk,
                                                        const double* __restrict__ traj, PathRec* __restrict__ recs) {
  using Kn = Kin<KIND, AD, AD2>;
  constexpr int D = Kn::DOF;
  __shared__ RobotDev R;
  stage_robot(&R, Rg);
  const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int lane = threadIdx.x;
  const int m = blk * 64 + lane;   // checked state of this lane
  const int seg = m / (inter + 1), j = m % (inter + 1);
  const double tau = (double)j / (double)(inter + 1);
  // a support state is checked if its sigma is finite, a sub-step if both ends are
  bool chk = m < Md && sigma != nullptr;   // no sigma: no path, nothing is checked
  double sg = 0.0;
  if (chk) {
    sg = sigma[seg];
    chk = isfinite(sg);
    if (j > 0) {   // seg < N here
      const double s1 = sigma[seg + 1];
      chk = chk && isfinite(s1);
      sg = sg + tau * (s1 - sg);
    }
  }
  double sup = 0.0, dense = 0.0, pos = -HUGE_VAL, rot = -HUGE_VAL;
  int kp = INT_MAX, kr = INT_MAX, inv = 0;
  if (chk) {
    const double* s0 = traj + ((size_t)b * (N + 1) + seg) * 2 * D;
    double q[D];
    checked_config<Kn>(s0, dt, inter, j, q);
    typename Kn::Axes A;   // filled by the walk, never read here
    Frame F;
    int nc, first;
    link_frame<KIND, AD, AD2>(R, q, link, A, F, nc, first);
    double Rm[9], t[3], Rt[9], tt[3];
    frame_rt(F, Rm, t);
    pose_rt(des + (size_t)seg * 16, Rt, tt);
    if (j > 0) {   // the target between two support states: positions on the chord, rotations on the geodesic
      double R1[9], t1[3];
      pose_rt(des + (size_t)(seg + 1) * 16, R1, t1);
      if (mode != GPMP2MI_WORKSPACE_POSITION) {
        double Rrel[9], trel[3], wl[3], E[9], R0[9];
        pose_between(Rt, tt, R1, t1, Rrel, trel);
        rot3_logmap(Rrel, wl);
#pragma unroll
        for (int k = 0; k < 3; k++) wl[k] *= tau;
        rot3_expmap(wl, E);
#pragma unroll
        for (int k = 0; k < 9; k++) R0[k] = Rt[k];
        mat3_mul(R0, E, Rt);
      }
#pragma unroll
      for (int k = 0; k < 3; k++) tt[k] = tt[k] + tau * (t1[k] - tt[k]);
    }
    double Rrel[9], trel[3], pd = 0.0, rd = 0.0, r2;
    pose_between(Rt, tt, Rm, t, Rrel, trel);
    const double dx = t[0] - tt[0], dy = t[1] - tt[1], dz = t[2] - tt[2];
    if (mode == GPMP2MI_WORKSPACE_POSITION) {
      r2 = dx * dx + dy * dy + dz * dz;
      pd = sqrt(r2);
    } else {
      double xi[6];
      if (mode == GPMP2MI_WORKSPACE_POSE) {
        pose3_logmap(Rrel, trel, xi);
        pd = sqrt(dx * dx + dy * dy + dz * dz);
        r2 = ((((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]) + xi[3] * xi[3]) + xi[4] * xi[4]) + xi[5] * xi[5];
      } else {
        rot3_logmap(Rrel, xi);
        r2 = xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2];
      }
      rd = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
    }
    if (!(isfinite(pd) && isfinite(rd))) {   // invalid: counted, enters no sum and no maximum
      inv = 1;
    } else {
      dense = r2 / (sg * sg);
      sup = j == 0 ? dense : 0.0;
      if (mode != GPMP2MI_WORKSPACE_ORIENTATION) { pos = pd; kp = m; }
      if (mode != GPMP2MI_WORKSPACE_POSITION) { rot = rd; kr = m; }
    }
  }
  // butterfly: both partners add the same two numbers, so all 64 lanes end with the same bits
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    sup += __shfl_xor(sup, off);
    dense += __shfl_xor(dense, off);
    inv += __shfl_xor(inv, off);
    const double op = __shfl_xor(pos, off), orr = __shfl_xor(rot, off);
    const int okp = __shfl_xor(kp, off), okr = __shfl_xor(kr, off);
    if (dev_greater(op, okp, pos, kp)) { pos = op; kp = okp; }
    if (dev_greater(orr, okr, rot, kr)) { rot = orr; kr = okr; }
  }
  if (lane == 0) recs[blockIdx.x] = PathRec{sup, dense, pos, rot, kp, kr, inv, 0};
}

// Second stage: rows are taken by thread (RowPick, score_select.h).  With a.sel.select the grid is one workgroup and
// the rule reads, besides this stage's own results, the per-row scores k_score_finish left.
__global__ __launch_bounds__(256) void k_path_finish(PathFinish a) {
  const ScoreFinish& f = a.sel;
  RowPick mine;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < f.B; b += gridDim.x * blockDim.x) {
    PathRec t = a.recs[(size_t)b * a.nblk];
    for (int i = 1; i < a.nblk; i++) {   // records in index order
      const PathRec& r = a.recs[(size_t)b * a.nblk + i];
      t.support += r.support;
      t.dense += r.dense;
      t.inv += r.inv;
      if (dev_greater(r.pos, r.kp, t.pos, t.kp)) { t.pos = r.pos; t.kp = r.kp; }
      if (dev_greater(r.rot, r.kr, t.rot, t.kr)) { t.rot = r.rot; t.kr = r.kr; }
    }
    // nothing checked (or the mode does not constrain it): deviation 0, state -1
    const double mp = t.kp == INT_MAX ? 0.0 : t.pos, mr = t.kr == INT_MAX ? 0.0 : t.rot;
    if (a.max_pos) a.max_pos[b] = mp;
    if (a.max_rot) a.max_rot[b] = mr;
    if (a.worst) {
      a.worst[2 * b] = t.kp == INT_MAX ? -1 : t.kp;
      a.worst[2 * b + 1] = t.kr == INT_MAX ? -1 : t.kr;
    }
    if (a.support) a.support[b] = t.support;
    if (a.dense) a.dense[b] = t.dense;
    if (a.invalid) a.invalid[b] = t.inv;
    if (!f.select) continue;
    const double fe = f.ferr[b];
    const bool ok = row_eligible(f, b, fe, a.clearance[b], a.oor[b]) && t.inv == 0 && mp <= a.allowed_pos && mr <= a.allowed_rot;
    if (ok) mine.take(fe, b);
  }
  if (!f.select) return;
  select_finish(f, mine);
}

int launch_path_factor(const RobotDev& h, const RobotDev* R, int mode, int link, int M, const double* conf,
                       const double* des, double* err, double* H, hipStream_t st) {
  if (M == 0) return GPMP2MI_OK;
  G2_DISPATCH_ROBOT_H(h, (k_path_factor<KIND_, AD_, AD2_><<<dim3((unsigned)M), dim3(64), 0, st>>>(R, mode, link, M, conf, des,
                                                                                                 err, H)));
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_path_list(int N, const double* sigma, int* list, int* count, hipStream_t st) {
  k_path_list<<<dim3(1), dim3(64), 0, st>>>(N, sigma, list, count);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_path_accumulate(const RobotDev& h, const RobotDev* R, const PlanParams& hp, const PlanBuffers& pb,
                           const PlanExtras& ex, const double* traj, int bufsel, const int* active, hipStream_t st) {
  if (ex.wp_n <= 0) return GPMP2MI_OK;   // no path, or no constrained state: nothing is launched
  if (ex.wp_n > hp.N + 1 || hp.D != h.dof || hp.D > MAXD || hp.NG + hp.D + 1 > 192 || ex.wp_link < 0 ||
      ex.wp_link >= h.nr_links) {
    set_error("k_path_accumulate: a path longer than the plan, a link out of range, or a record wider than 192 entries");
    return GPMP2MI_ERR_INVALID;
  }
  const dim3 grid((unsigned)(hp.B * ex.wp_n));
  G2_DISPATCH_ROBOT_H(h, (k_path_accumulate<KIND_, AD_, AD2_><<<grid, dim3(64), 0, st>>>(R, pb.params, pb, ex, traj, bufsel,
                                                                                       active)));
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int path_blocks(int Md) { return (Md + 63) / 64; }

int launch_path_deviation(const RobotDev& h, const RobotDev* R, int mode, int link, const double* des, const double* sigma,
                          double dt, int inter, int B, int N, const double* traj, PathRec* recs, hipStream_t st) {
  int Md, nblk;
  if (const int rc = checked_grid(N, inter, 64, B, 1, Md, nblk)) return rc;
  const dim3 grid((unsigned)(nblk * B));
  G2_DISPATCH_ROBOT_H(h, (k_path_deviation<KIND_, AD_, AD2_><<<grid, dim3(64), 0, st>>>(R, mode, link, des, sigma, dt, inter, N,
                                                                                      Md, nblk, traj, recs)));
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_path_finish(const PathFinish& a, hipStream_t st) {
  return launch_finish(k_path_finish, a, a.sel.select, a.sel.B, st);
}

}  // namespace g2
