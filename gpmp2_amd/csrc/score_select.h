// score_select.h -- what the finish kernels of the score-and-select stage share (score_kernels.hip: k_score_finish,
// self_clearance_kernels.hip: k_self_finish): the (clearance, state, index) key and its order, the reduction of a row's
// records, one coordinate of the chosen row's up-sampled form, and the selection over the rows of one workgroup.
#pragma once
#include <climits>

#include "device_math.h"
#include "launch.h"

namespace g2 {

// (clearance, state, sphere) compared lexicographically: the minimum and where it occurs travel together, exact ties
// go to the lowest state, then the lowest sphere.  "none" is (+inf, INT_MAX, INT_MAX).  The self-collision check keys
// by (clearance, state, pair) with the same order.
struct ScoreKey {
  double c;
  int k, s;
};
__device__ __forceinline__ bool key_less(const ScoreKey& a, const ScoreKey& b) {
  return a.c < b.c || (a.c == b.c && (a.k < b.k || (a.k == b.k && a.s < b.s)));
}

// eligible(b) of "scoring" (include/gpmp2mi.h) for one row; status_ok: status[b] != GPMP2MI_TRAJ_NOT_SPD, or no status
__device__ __forceinline__ bool score_eligible(bool status_ok, double final_error, double clearance,
                                               double required_clearance, int require_in_range, int oor) {
  return status_ok && isfinite(final_error) && clearance >= required_clearance && (!require_in_range || oor == 0);
}

// the nblk records of one row, in index order
__device__ __forceinline__ ScoreRec reduce_records(const ScoreRec* r, int nblk) {
  ScoreRec t = r[0];
  for (int i = 1; i < nblk; i++) {   // records in index order
    t.support += r[i].support;
    t.dense += r[i].dense;
    t.oor += r[i].oor;
    const ScoreKey x{r[i].clearance, r[i].k, r[i].s}, c{t.clearance, t.k, t.s};
    if (key_less(x, c)) { t.clearance = x.c; t.k = x.k; t.s = x.s; }
  }
  return t;
}

// One output state of interpolateArmTraj / interpolatePose2MobileArmTraj, coordinate k: the expressions of
// k_interpolate_traj (factor_kernels.hip) element by element.  s0 / s1: the support states around it.
__device__ __forceinline__ void score_dense_coord(bool lie, double dt, int inter, int D, int j, int k, const double* s0,
                                                  double* o) {
  if (j == 0) {
    o[k] = s0[k];
    o[D + k] = s0[D + k];
    return;
  }
  const double* s1 = s0 + 2 * D;
  const GpCoef gc = gp_coef_dev(dt, (double)j * (dt / (double)(inter + 1)));
  if (lie) {
    double r, qk;
    if (k < 3) {
      double x0[3], w0[3], x1[3], w1[3], qp[3], lg[3];
#pragma unroll
      for (int i = 0; i < 3; i++) { x0[i] = s0[i]; w0[i] = s0[D + i]; x1[i] = s1[i]; w1[i] = s1[D + i]; }
      lie_interpolate<3>(gc, x0, w0, x1, w1, qp, nullptr);
      pose2_logmap(pose2_between(P2{x0[0], x0[1], x0[2]}, P2{x1[0], x1[1], x1[2]}), lg);
      qk = k == 0 ? qp[0] : k == 1 ? qp[1] : qp[2];
      r = k == 0 ? lg[0] : k == 1 ? lg[1] : lg[2];
    } else {
      qk = s0[k] + (gc.l12 * s0[D + k] + gc.p11 * (s1[k] - s0[k]) + gc.p12 * s1[D + k]);
      r = s1[k] - s0[k];
    }
    o[k] = qk;
    o[D + k] = gc.l22 * s0[D + k] + gc.p21 * r + gc.p22 * s1[D + k];
  } else {
    o[k] = gc.l11 * s0[k] + gc.l12 * s0[D + k] + gc.p11 * s1[k] + gc.p12 * s1[D + k];
    o[D + k] = gc.l21 * s0[k] + gc.l22 * s0[D + k] + gc.p21 * s1[k] + gc.p22 * s1[D + k];
  }
}

// The selection over the rows of ONE workgroup of 256 threads: every thread brings the best (final_error, row) of its
// eligible rows (rows ascending within a thread) and their count; the workgroup reduces them through LDS, writes best /
// n_eligible / best_err, then all its threads copy the chosen row and its up-sampled form.  Every thread must call it.
__device__ __forceinline__ void select_finish(const ScoreFinish& a, double my_err, int my_row, int my_cnt) {
  __shared__ double s_err[256];
  __shared__ int s_row[256], s_cnt[256];
  s_err[threadIdx.x] = my_err;
  s_row[threadIdx.x] = my_row;
  s_cnt[threadIdx.x] = my_cnt;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) {
      const int o = threadIdx.x + h;
      if (s_err[o] < s_err[threadIdx.x] || (s_err[o] == s_err[threadIdx.x] && s_row[o] < s_row[threadIdx.x])) {
        s_err[threadIdx.x] = s_err[o];
        s_row[threadIdx.x] = s_row[o];
      }
      s_cnt[threadIdx.x] += s_cnt[o];
    }
    __syncthreads();
  }
  const int best = s_row[0] == INT_MAX ? -1 : s_row[0];
  if (threadIdx.x == 0) {
    if (a.best) *a.best = best;
    if (a.n_eligible) *a.n_eligible = s_cnt[0];
  }
  if (best < 0) return;   // the trajectory outputs are left untouched
  if (threadIdx.x == 0 && a.best_err) *a.best_err = s_err[0];
  const size_t trow = (size_t)(a.N + 1) * 2 * a.D;
  const double* row = a.traj + (size_t)best * trow;
  if (a.traj_best)
    for (size_t i = threadIdx.x; i < trow; i += blockDim.x) a.traj_best[i] = row[i];
  if (a.dense_best)
    for (int e = threadIdx.x; e < a.Md * a.D; e += blockDim.x) {
      const int m = e / a.D, k = e % a.D;
      const int seg = m / (a.inter + 1), j = m % (a.inter + 1);
      score_dense_coord(a.lie != 0, a.dt, a.inter, a.D, j, k, row + (size_t)seg * 2 * a.D, a.dense_best + (size_t)m * 2 * a.D);
    }
}

}  // namespace g2
