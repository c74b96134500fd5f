// score_select.h -- the one copy of every stage the checks of the executed trajectory share (score_kernels.hip,
// self_clearance_kernels.hip, motion_kernels.hip, moving_kernels.hip, path_kernels.hip, retime_kernels.hip,
// torque_kernels.hip):
//
//   first stage    checked_config: the configuration of checked state m; score_dense_coord: one coordinate of its
//                  up-sampled form with the velocity.  ScoreKey / key_less: the (clearance, state, index) key and its
//                  order.  block_score_record: lane butterfly -> LDS -> ONE ScoreRec per workgroup.
//   finish kernel  reduce_records: a row's records in index order.  row_eligible: the rule's common prefix.  RowPick: the
//                  best (final_error, row) of a thread's rows.  select_finish: the selection over one workgroup.
//   launchers      checked_grid / score_waves: the grid of a first stage and its guards; launch_finish.
//
// Not folded into checked_config, because their expressions differ: k_motion and k_retime_caps need the velocities
// (score_dense_coord); k_sampled_clearance interpolates the rounded sums estimate + delta and adds the bridge; k_risk
// carries the coefficients of its band with the interpolation's.  k_score has the text of checked_config written out
// (score_kernels.hip says why); a change to one must be made to the other.
#pragma once
#include <algorithm>
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
// ... of row b under the selection f, with the obstacle clearance and out-of-range count of that row: the part of the
// rule every finish kernel applies before its own conditions
__device__ __forceinline__ bool row_eligible(const ScoreFinish& f, int b, double final_error, double clearance, int oor) {
  return score_eligible(!f.status || f.status[b] != GPMP2MI_TRAJ_NOT_SPD, final_error, clearance, f.required_clearance,
                        f.require_in_range, oor);
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

// the interpolation coefficients of sub-step j (1 .. inter) of an interval, as k_interpolate_traj forms them
__device__ __forceinline__ GpCoef sub_step_coef(double dt, int inter, int j) {
  return gp_coef_dev(dt, (double)j * (dt / (double)(inter + 1)));
}

// The configuration of a checked state: sub-step j of the interval that starts at support state s0 (j == 0: s0 itself).
// The expressions of k_interpolate_traj (factor_kernels.hip) without the velocity half.
template <class Kn>
__device__ __forceinline__ void checked_config(const double* s0, double dt, int inter, int j, double (&q)[Kn::DOF]) {
  constexpr int D = Kn::DOF;
  if (j == 0) {
#pragma unroll
    for (int k = 0; k < D; k++) q[k] = s0[k];
    return;
  }
  const double* s1 = s0 + 2 * D;
  const GpCoef gc = sub_step_coef(dt, inter, j);
  if constexpr (Kn::MOBILE) {
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
  const GpCoef gc = sub_step_coef(dt, inter, j);
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

// The end of a first stage whose workgroup leaves a ScoreRec: every lane brings its hinge sums (sup: support states
// only), its count (out-of-range spheres, invalid pairs) and its key.  Wavefront butterfly -> LDS -> thread 0 merges the
// wavefronts in index order and writes recs[blockIdx.x].  Every thread must call it.
__device__ __forceinline__ void block_score_record(double sup, double dense, int cnt, ScoreKey best,
                                                   ScoreRec* __restrict__ recs) {
  __shared__ double w_sup[4], w_den[4], w_clr[4];
  __shared__ int w_k[4], w_s[4], w_cnt[4];
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6, nsub = blockDim.x >> 6;
  // wavefront: butterfly (both partners add the same two numbers, so all 64 lanes end with the same bits)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    sup += __shfl_xor(sup, off);
    dense += __shfl_xor(dense, off);
    cnt += __shfl_xor(cnt, off);
    const ScoreKey o{__shfl_xor(best.c, off), __shfl_xor(best.k, off), __shfl_xor(best.s, off)};
    if (key_less(o, best)) best = o;
  }
  if (lane == 0) {
    w_sup[sub] = sup; w_den[sub] = dense; w_clr[sub] = best.c;
    w_k[sub] = best.k; w_s[sub] = best.s; w_cnt[sub] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ScoreRec r{w_sup[0], w_den[0], w_clr[0], w_k[0], w_s[0], w_cnt[0], 0};
    for (int w = 1; w < nsub; w++) {   // wavefronts in index order
      r.support += w_sup[w];
      r.dense += w_den[w];
      r.oor += w_cnt[w];
      const ScoreKey a{w_clr[w], w_k[w], w_s[w]}, c{r.clearance, r.k, r.s};
      if (key_less(a, c)) { r.clearance = a.c; r.k = a.k; r.s = a.s; }
    }
    recs[blockIdx.x] = r;
  }
}

// What a thread of a finish kernel keeps of its eligible rows: the best (final_error, row) and their count
struct RowPick {
  double my_err = HUGE_VAL;
  int my_row = INT_MAX, my_cnt = 0;
  __device__ __forceinline__ void take(double fe, int b) {
    my_cnt++;
    if (fe < my_err) {   // rows ascend within a thread: a tie keeps the lower row
      my_err = fe;
      my_row = b;
    }
  }
};

// The selection over the rows of ONE workgroup of 256 threads: every thread brings the pick of its eligible rows (rows
// ascending within a thread); the workgroup reduces them through LDS, writes best / n_eligible / best_err, then all its
// threads copy the chosen row and its up-sampled form.  Every thread must call it.
__device__ __forceinline__ void select_finish(const ScoreFinish& a, const RowPick& mine) {
  __shared__ double s_err[256];
  __shared__ int s_row[256], s_cnt[256];
  s_err[threadIdx.x] = mine.my_err;
  s_row[threadIdx.x] = mine.my_row;
  s_cnt[threadIdx.x] = mine.my_cnt;
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

// A finish kernel takes its rows by thread; with a selection the grid is the one workgroup of select_finish.
template <class Args>
int launch_finish(void (*kernel)(Args), const Args& a, int select, int B, hipStream_t st) {
  const int grid = select ? 1 : (B + 255) / 256;
  kernel<<<dim3(grid), dim3(256), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

// The grid of a first stage: Md checked states of each of B rows in tiles of `tile`, nblk tiles (records) per row.
// per_state: the most (state, index) pairs of one state that a kernel numbers in an int.  Every product a kernel forms
// from these stays below 2^31.
inline int checked_grid(int N, int inter, int tile, int B, long long per_state, int& Md, int& nblk) {
  const long long md = (long long)N * (inter + 1) + 1;
  const long long nb = (md + tile - 1) / tile;
  if (md >= (1ll << 31) / GPMP2MI_MAX_DOF || nb * B >= (1ll << 31) || md * std::max(per_state, 1ll) >= (1ll << 31)) {
    set_error("too many checked states for one launch");
    return GPMP2MI_ERR_INVALID;
  }
  Md = (int)md;
  nblk = (int)nb;
  return GPMP2MI_OK;
}
// wavefronts that share the spheres (and the pairs) of a tile: a function of the sphere count alone
inline int score_waves(int S) { return S >= 8 ? 4 : 1; }

}  // namespace g2
