// motion_kernels.hip -- the motion limits of the executed trajectory behind gpmp2mi_motion_score_traj /
// gpmp2mi_plan_motion_score / gpmp2mi_plan_select_feasible (include/gpmp2mi.h "motion limits"): does the robot stay
// inside its joint ranges, joint speeds, joint accelerations and a Cartesian speed at every state that is executed, and by
// which factor must the duration be stretched if not?
//
//   k_motion         tiled as k_score is (checked_grid, score_select.h): a lane is a checked state, a workgroup covers
//                    SCORE_TILE consecutive states of one trajectory, its `nsub` wavefronts share the spheres (s % nsub).
//                    Every lane up-samples BOTH halves of its state (score_dense_coord: the velocity is needed here);
//                    wavefront 0 does the coordinate checks (position margin, velocity ratio) once per state, and its
//                    lanes on a support state that opens an interval the two acceleration ends of that interval; then
//                    every wavefront walks the chain and contracts each sphere's Jacobian with the velocity column by
//                    column (Kin::jacobian_times: no J[D][3] in registers).  Four (value, i, j) keys and the count of
//                    non-finite quantities per lane -> keyed butterflies -> wavefronts in index order through LDS -> ONE
//                    record per workgroup.
//   k_motion_finish  reduces a row's records in index order and writes the outputs; when asked, applies the extended
//                    selection rule over the per-row scores the existing stages left and copies the chosen row
//                    (select_finish, score_select.h).
//
// Determinism: every output is an extremum with an index key (key_less: exact ties go to the lowest indices) or an
// integer count; no sums of floating-point numbers, no atomics.  A row's results do not depend on the batch, its position
// in it or the entry point.
#include <climits>

#include "device_math.h"
#include "dispatch.h"
#include "launch.h"
#include "score_select.h"

namespace g2 {

namespace {

// a quantity joins the extremum of its kind, or the count of the non-finite ones
__device__ __forceinline__ void motion_take(ScoreKey& best, int& invalid, double value, int i, int j) {
  if (!isfinite(value)) {
    invalid++;
    return;
  }
  const ScoreKey key{value, i, j};
  if (key_less(key, best)) best = key;
}

// The acceleration of the interpolated mean at the two ends of an interval (include/gpmp2mi.h "motion limits"), every
// operation rounded once in the order written (no fused multiply-add): straight lines and mirrored trajectories give
// exact ties between intervals, and those must not depend on what the compiler contracts.
__device__ __forceinline__ void motion_acc_ends(double dt, double dx, double v0, double v1, double& a0, double& a1) {
#pragma clang fp contract(off)
  const double w = 6.0 / (dt * dt);
  const double wx = w * dx;
  a0 = wx - (4.0 * v0 + 2.0 * v1) / dt;
  a1 = -wx + (2.0 * v0 + 4.0 * v1) / dt;
}

__device__ __forceinline__ void motion_merge(ScoreKey& best, const ScoreKey& o) {
  if (key_less(o, best)) best = o;
}

}  // namespace

template <int KIND, int AD, int AD2>
__global__ __launch_bounds__(256) void k_motion(const RobotDev* __restrict__ Rg, MotionLimitsDev lim, double dt, int inter,
                                                int N, int Md, int nblk, const double* __restrict__ traj,
                                                MotionRec* __restrict__ recs) {
  using K = Kin<KIND, AD, AD2>;
  constexpr int D = K::DOF;
  constexpr int FREE = K::BASE;   // Pose2 coordinates: no position and no acceleration limit
  __shared__ RobotDev R;
  __shared__ double w_v[4][4];
  __shared__ int w_i[4][4], w_j[4][4], w_inv[4];
  stage_robot(&R, Rg);
  const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6, nsub = blockDim.x >> 6;
  const int m = blk * SCORE_TILE + lane;   // checked state of this lane
  // 0: position margin; 1 .. 3: minus the velocity ratio, the acceleration ratio, the point speed
  ScoreKey best[4];
#pragma unroll
  for (int c = 0; c < 4; c++) best[c] = ScoreKey{HUGE_VAL, INT_MAX, INT_MAX};
  int invalid = 0;
  if (m < Md) {
    const int seg = m / (inter + 1), j = m % (inter + 1);
    const double* s0 = traj + ((size_t)b * (N + 1) + seg) * 2 * D;
    double x[2 * D];   // q, then v
#pragma unroll
    for (int k = 0; k < D; k++) score_dense_coord(K::MOBILE, dt, inter, D, j, k, s0, x);
    if (sub == 0) {
#pragma unroll
      for (int d = 0; d < D; d++) {
        if (d >= FREE && (isfinite(lim.down[d]) || isfinite(lim.up[d]))) {
          const double lo = isfinite(lim.down[d]) ? x[d] - lim.down[d] : HUGE_VAL;
          const double hi = isfinite(lim.up[d]) ? lim.up[d] - x[d] : HUGE_VAL;
          motion_take(best[0], invalid, isfinite(x[d]) ? (lo < hi ? lo : hi) : x[d] - x[d], m, d);
        }
        if (isfinite(lim.vel[d])) motion_take(best[1], invalid, -(fabs(x[D + d]) / lim.vel[d]), m, d);
      }
      if (j == 0 && seg < N) {
        const double* s1 = s0 + 2 * D;
#pragma unroll
        for (int d = FREE; d < D; d++) {
          if (!isfinite(lim.acc[d])) continue;
          double a0, a1;
          motion_acc_ends(dt, s1[d] - s0[d], s0[D + d], s1[D + d], a0, a1);
          motion_take(best[2], invalid, -(fabs(a0) / lim.acc[d]), 2 * seg, d);
          motion_take(best[2], invalid, -(fabs(a1) / lim.acc[d]), 2 * seg + 1, d);
        }
      }
    }
    double q[D], v[D];
#pragma unroll
    for (int k = 0; k < D; k++) { q[k] = x[k]; v[k] = x[D + k]; }
    typename K::Axes A;
    K::walk(R, q, A, [&](int s, const double (&p)[3], auto tag) {
      double u[3];
      K::jacobian_times(A, p, tag, v, u);
      motion_take(best[3], invalid, -sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), m, R.sph_orig[s]);
    }, sub, nsub);
  }
  // wavefront: keyed butterflies (both partners keep the same key, so all 64 lanes end with the same bits)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    invalid += __shfl_xor(invalid, off);
#pragma unroll
    for (int c = 0; c < 4; c++)
      motion_merge(best[c], ScoreKey{__shfl_xor(best[c].c, off), __shfl_xor(best[c].k, off), __shfl_xor(best[c].s, off)});
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 4; c++) { w_v[sub][c] = best[c].c; w_i[sub][c] = best[c].k; w_j[sub][c] = best[c].s; }
    w_inv[sub] = invalid;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    MotionRec r;
    r.invalid = 0;
    r.pad = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      ScoreKey t{w_v[0][c], w_i[0][c], w_j[0][c]};
      for (int w = 1; w < nsub; w++) motion_merge(t, ScoreKey{w_v[w][c], w_i[w][c], w_j[w][c]});   // wavefronts in index order
      r.v[c] = t.c; r.ij[c][0] = t.k; r.ij[c][1] = t.s;
    }
    for (int w = 0; w < nsub; w++) r.invalid += w_inv[w];
    recs[blockIdx.x] = r;
  }
}

namespace {

// the outputs of one row: its records in index order
struct MotionRow {
  double pos_margin, vel_ratio, acc_ratio, point_speed, time_scale;
  int worst[4][2], invalid;
};
__device__ __forceinline__ MotionRow motion_row(const MotionFinish& a, int b) {
  const MotionRec* r = a.recs + (size_t)b * a.nblk;
  MotionRec t = r[0];
  for (int i = 1; i < a.nblk; i++) {   // records in index order
    t.invalid += r[i].invalid;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const ScoreKey x{r[i].v[c], r[i].ij[c][0], r[i].ij[c][1]}, cur{t.v[c], t.ij[c][0], t.ij[c][1]};
      if (key_less(x, cur)) { t.v[c] = x.c; t.ij[c][0] = x.k; t.ij[c][1] = x.s; }
    }
  }
  MotionRow o;
  double val[4];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const bool none = t.ij[c][0] == INT_MAX;
    o.worst[c][0] = none ? -1 : t.ij[c][0];
    o.worst[c][1] = none ? -1 : t.ij[c][1];
    val[c] = c == 0 ? (none ? HUGE_VAL : t.v[0]) : (none ? 0.0 : -t.v[c]);
  }
  o.pos_margin = val[0];
  o.vel_ratio = val[1];
  o.acc_ratio = val[2];
  o.point_speed = val[3];
  const double ra = sqrt(o.acc_ratio), rp = o.point_speed / a.limit_point_speed;
  double s = o.vel_ratio;
  if (ra > s) s = ra;
  if (rp > s) s = rp;
  o.time_scale = s;
  o.invalid = t.invalid;
  return o;
}

}  // namespace

// Second stage: rows are taken by thread (RowPick, score_select.h).  With a.sel.select the grid is one workgroup
// and the rule reads, besides this stage's own results, the per-row scores k_score_finish and k_self_finish left.
__global__ __launch_bounds__(256) void k_motion_finish(MotionFinish a) {
  const ScoreFinish& f = a.sel;
  RowPick mine;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < f.B; b += gridDim.x * blockDim.x) {
    const MotionRow o = motion_row(a, b);
    if (a.pos_margin) a.pos_margin[b] = o.pos_margin;
    if (a.vel_ratio) a.vel_ratio[b] = o.vel_ratio;
    if (a.acc_ratio) a.acc_ratio[b] = o.acc_ratio;
    if (a.point_speed) a.point_speed[b] = o.point_speed;
    if (a.time_scale) a.time_scale[b] = o.time_scale;
    if (a.worst) {
#pragma unroll
      for (int c = 0; c < 4; c++) {
        a.worst[8 * b + 2 * c] = o.worst[c][0];
        a.worst[8 * b + 2 * c + 1] = o.worst[c][1];
      }
    }
    if (a.invalid) a.invalid[b] = o.invalid;
    if (!f.select) continue;
    const double fe = f.ferr[b];
    bool ok = row_eligible(f, b, fe, a.clearance[b], a.oor[b]);
    if (a.self_clearance) ok = ok && a.self_invalid[b] == 0 && a.self_clearance[b] >= a.required_self_clearance;
    ok = ok && o.invalid == 0 && o.pos_margin >= a.required_pos_margin && o.time_scale <= a.max_time_scale;
    if (ok) mine.take(fe, b);
  }
  if (!f.select) return;
  select_finish(f, mine);   // f.best is never null here (launch_motion_finish)
  if (threadIdx.x == 0 && a.time_scale_best) {
    const int best = *f.best;   // written by this thread
    if (best >= 0) *a.time_scale_best = motion_row(a, best).time_scale;
  }
}

int launch_motion(const RobotDev& h, const RobotDev* R, const MotionLimitsDev& lim, double dt, int inter, int B, int N,
                  const double* traj, MotionRec* recs, hipStream_t st) {
  int Md, nblk;
  if (const int rc = checked_grid(N, inter, SCORE_TILE, B, 1, Md, nblk)) return rc;
  const dim3 grid((unsigned)(nblk * B)), block(64 * score_waves(h.nr_spheres));
  G2_DISPATCH_ROBOT_H(h, (k_motion<KIND_, AD_, AD2_><<<grid, block, 0, st>>>(R, lim, dt, inter, N, Md, nblk, traj, recs)));
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_motion_finish(const MotionFinish& a, hipStream_t st) {
  if (a.sel.select && !a.sel.best) {
    set_error("k_motion_finish: the selection needs a place for `best`");
    return GPMP2MI_ERR_INVALID;
  }
  return launch_finish(k_motion_finish, a, a.sel.select, a.sel.B, st);
}

}  // namespace g2
