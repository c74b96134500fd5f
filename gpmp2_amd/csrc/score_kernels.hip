// score_kernels.hip -- the score-and-select stage behind gpmp2mi_score_traj / gpmp2mi_plan_score / gpmp2mi_plan_select
// (include/gpmp2mi.h "scoring"): which of these trajectories is executed, and is it collision-free between its
// support states as well?
//
//   k_score         one lane per checked state of a trajectory: GP up-sampling -> value-only walk of the kinematic
//                   chain -> field lookup per sphere -> hinge sum, minimum clearance with its (state, sphere) and the
//                   out-of-range count; the up-sampled states never reach memory.  A workgroup covers SCORE_TILE
//                   consecutive states; its `nsub` wavefronts share the spheres of those states (s % nsub).  ONE record
//                   per workgroup (block_score_record, score_select.h).  The up-sampling is the text of checked_config
//                   (score_select.h) written out: called from here, the same expressions are scheduled with up to ten
//                   more VGPRs, which costs the 7- and 8-joint arm in a planar field a wavefront of occupancy.
//   k_score_finish  reduces the records of every row in index order to the five per-row outputs, applies the
//                   selection rule when asked and copies the chosen row and its up-sampled form.
//
// Determinism: the tile and nsub depend on (N, inter_step, S) only, every sum is taken in a fixed order (lane
// butterfly, wavefronts in index order, records in index order) and no floating-point atomic is used, so a row's
// results do not depend on the batch, its position in it or the device.
#include <climits>

#include "device_math.h"
#include "dispatch.h"
#include "launch.h"
#include "score_select.h"

namespace g2 {

template <int KIND, int AD, int AD2, int SDIM>
__global__ __launch_bounds__(256) void k_score(const RobotDev* __restrict__ Rg, SdfDev sdf, double dt, int inter, int N,
                                               int Md, int nblk, const double* __restrict__ traj,
                                               ScoreRec* __restrict__ recs) {
  using K = Kin<KIND, AD, AD2>;
  constexpr int D = K::DOF;
  __shared__ RobotDev R;
  stage_robot(&R, Rg);
  const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6, nsub = blockDim.x >> 6;
  const int m = blk * SCORE_TILE + lane;   // checked state of this lane
  double dense = 0.0;
  int oor = 0;
  ScoreKey best{HUGE_VAL, INT_MAX, INT_MAX};
  bool support = false;
  if (m < Md) {
    const int seg = m / (inter + 1), j = m % (inter + 1);
    support = j == 0;
    const double* s0 = traj + ((size_t)b * (N + 1) + seg) * 2 * D;
    double q[D];
    if (j == 0) {   // checked_config, written out (see above)
#pragma unroll
      for (int k = 0; k < D; k++) q[k] = s0[k];
    } else {
      const double* s1 = s0 + 2 * D;
      const GpCoef gc = gp_coef_dev(dt, (double)j * (dt / (double)(inter + 1)));
      if constexpr (K::MOBILE) {
        // GaussianProcessInterpolatorPose2Vector: the Pose2 part through lie_interpolate, the rest as it does
        double x0[3], w0[3], x1[3], w1[3], qp[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { x0[k] = s0[k]; w0[k] = s0[D + k]; x1[k] = s1[k]; w1[k] = s1[D + k]; }
        lie_interpolate<3>(gc, x0, w0, x1, w1, qp, nullptr);
#pragma unroll
        for (int k = 0; k < 3; k++) q[k] = qp[k];
#pragma unroll
        for (int k = 3; k < D; k++) q[k] = s0[k] + (gc.l12 * s0[D + k] + gc.p11 * (s1[k] - s0[k]) + gc.p12 * s1[D + k]);
      } else {
#pragma unroll
        for (int k = 0; k < D; k++) q[k] = gc.l11 * s0[k] + gc.l12 * s0[D + k] + gc.p11 * s1[k] + gc.p12 * s1[D + k];
      }
    }
    typename K::Axes A;   // filled by the walk, never read here: the Jacobian work is dead code
    K::walk(R, q, A, [&](int s, const double (&p)[3], auto) {
      // negated conjunction: a NaN centre fails every comparison and counts as out of range
      bool in = p[0] >= sdf.ox && p[0] <= sdf.hix && p[1] >= sdf.oy && p[1] <= sdf.hiy;
      if (SDIM == 3) in = in && p[2] >= sdf.oz && p[2] <= sdf.hiz;
      if (!in) {
        oor++;
        return;
      }
      double d, gx, gy, gz;
      if (SDIM == 3) (void)sdf3_lookup(sdf, p[0], p[1], p[2], d, gx, gy, gz);
      else (void)sdf2_lookup(sdf, p[0], p[1], d, gx, gy);
      const double r = R.sph_r[s];
      dense += d > r ? 0.0 : r - d;
      const ScoreKey key{d - r, m, R.sph_orig[s]};
      if (key_less(key, best)) best = key;
    }, sub, nsub);
  }
  block_score_record(support ? dense : 0.0, dense, oor, best, recs);
}

// Second stage.  Rows are taken by thread (row = thread id + multiple of the thread count): a row's records are summed
// in index order.  With a.select the grid is one workgroup: every thread keeps the best (final_error, row) of its rows,
// the workgroup reduces them through LDS, then all its threads copy the chosen row (select_finish, score_select.h).
// a.recs == nullptr: selection over given scores (gpmp2mi_select_best_dev).
__global__ __launch_bounds__(256) void k_score_finish(ScoreFinish a) {
  RowPick mine;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < a.B; b += gridDim.x * blockDim.x) {
    double clr;
    int oor;
    if (a.recs) {
      const ScoreRec t = reduce_records(a.recs + (size_t)b * a.nblk, a.nblk);
      const bool none = t.k == INT_MAX;
      if (a.support) a.support[b] = t.support;
      if (a.dense) a.dense[b] = t.dense;
      if (a.clearance) a.clearance[b] = t.clearance;
      if (a.worst) {
        a.worst[2 * b] = none ? -1 : t.k;
        a.worst[2 * b + 1] = none ? -1 : t.s;
      }
      if (a.oor) a.oor[b] = t.oor;
      clr = t.clearance;
      oor = t.oor;
    } else {
      clr = a.in_clearance[b];
      oor = a.in_oor ? a.in_oor[b] : 0;
    }
    if (!a.select) continue;
    const double fe = a.ferr[b];
    if (row_eligible(a, b, fe, clr, oor)) mine.take(fe, b);
  }
  if (!a.select) return;
  select_finish(a, mine);
}

int score_blocks(int Md) { return (Md + SCORE_TILE - 1) / SCORE_TILE; }

int launch_score(const RobotDev& h, const RobotDev* R, const SdfDev& s, double dt, int inter, int B, int N,
                 const double* traj, ScoreRec* recs, hipStream_t st) {
  int Md, nblk;
  if (const int rc = checked_grid(N, inter, SCORE_TILE, B, 1, Md, nblk)) return rc;
  const dim3 grid((unsigned)(nblk * B)), block(64 * score_waves(h.nr_spheres));
  if (s.dim == 3) {
    G2_DISPATCH_ROBOT_H(h, (k_score<KIND_, AD_, AD2_, 3><<<grid, block, 0, st>>>(R, s, dt, inter, N, Md, nblk, traj, recs)));
  } else {
    G2_DISPATCH_ROBOT_H(h, (k_score<KIND_, AD_, AD2_, 2><<<grid, block, 0, st>>>(R, s, dt, inter, N, Md, nblk, traj, recs)));
  }
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_score_finish(const ScoreFinish& a, hipStream_t st) {
  return launch_finish(k_score_finish, a, a.select, a.B, st);
}

}  // namespace g2
