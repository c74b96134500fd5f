// retime_kernels.hip -- the speed profile of the executed trajectory behind gpmp2mi_retime_path / gpmp2mi_retime_traj /
// gpmp2mi_plan_retime / gpmp2mi_plan_select_retimed (include/gpmp2mi.h "re-timing"): along the unchanged path, the rate
// sdot_k of planned against executed time at every checked state that makes the duration as short as the joint speeds,
// joint accelerations and the Cartesian sphere speed allow.  The rule is retime_rule.h; these kernels spread it.
//
//   k_retime_caps    tiled as k_motion is (checked_grid, score_select.h): a lane is a checked state, a workgroup covers
//                    SCORE_TILE consecutive states of one trajectory, its `nsub` wavefronts share the spheres.  Writes
//                    ps_k, the largest sphere speed of the state (NaN when one of them is not finite).
//   k_retime         one wavefront per row; its stages are retime_chain.h's, shared with k_retime_dynamic
//                    (retime_dynamic_kernels.hip).  Caps X_k and the finiteness of the row, a lane per state.  Then the chain:
//                    per stage, lanes < 2 D form the rows from the two support states of the interval (TRAJ) or from the
//                    caller's arrays, lane 2 D the row of the next set; the (2 D + 1)^2 pairs are strided over the lanes
//                    and the two ends reduced by butterflies.  K goes to the workspace.  The forward pass takes the
//                    smallest upper bound of the same rows.  Then, a lane per state or per (stage, joint): `achieved`,
//                    the rates, the stage times; the stamps are one sum in index order.
//   k_retime_finish  the selection of gpmp2mi_plan_select_retimed over the per-row scores the existing stages left, by
//                    select_finish (score_select.h); the chosen row's velocities are multiplied by its rates.
//
// Determinism: set ends and rates are extrema of singly rounded quotients, `achieved` is four maxima, the stamps are
// summed in index order by every lane alike.  A row's results do not depend on the batch or the entry point.
#include <climits>

#include "device_math.h"
#include "dispatch.h"
#include "launch.h"
#include "retime_chain.h"
#include "score_select.h"

namespace g2 {

static_assert(2 * GPMP2MI_MAX_DOF + 1 <= 64, "the rows of a stage are one per lane");

template <int KIND, int AD, int AD2>
__global__ __launch_bounds__(256) void k_retime_caps(const RobotDev* __restrict__ Rg, double dt, int inter, int N, int Md,
                                                     int nblk, const double* __restrict__ traj, double* __restrict__ ps) {
  using K = Kin<KIND, AD, AD2>;
  constexpr int D = K::DOF;
  __shared__ RobotDev R;
  __shared__ double w_ps[4][SCORE_TILE];
  __shared__ int w_bad[4][SCORE_TILE];
  stage_robot(&R, Rg);
  const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6, nsub = blockDim.x >> 6;
  const int m = blk * SCORE_TILE + lane;   // checked state of this lane
  double mx = 0.0;
  int bad = 0;
  if (m < Md) {
    const int seg = m / (inter + 1), j = m % (inter + 1);
    const double* s0 = traj + ((size_t)b * (N + 1) + seg) * 2 * D;
    double x[2 * D], q[D], v[D];
#pragma unroll
    for (int k = 0; k < D; k++) score_dense_coord(K::MOBILE, dt, inter, D, j, k, s0, x);
#pragma unroll
    for (int k = 0; k < D; k++) { q[k] = x[k]; v[k] = x[D + k]; }
    typename K::Axes A;
    K::walk(R, q, A, [&](int s, const double (&p)[3], auto tag) {
      double u[3];
      K::jacobian_times(A, p, tag, v, u);
      const double sp = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
      if (!isfinite(sp)) bad = 1;
      else if (sp > mx) mx = sp;
    }, sub, nsub);
  }
  w_ps[sub][lane] = mx;
  w_bad[sub][lane] = bad;
  __syncthreads();
  if (sub == 0 && m < Md) {
    for (int w = 1; w < nsub; w++) {   // a maximum: the order does not matter
      if (w_ps[w][lane] > mx) mx = w_ps[w][lane];
      bad |= w_bad[w][lane];
    }
    ps[(size_t)b * Md + m] = bad ? nan("") : mx;
  }
}

namespace {

// row `lane` of stage k: lanes < D the start rows, < 2 D the end rows, 2 D the next set [lo, hi]; the others nothing
template <bool TRAJ>
__device__ __forceinline__ RetimeRow retime_lane_row(const RetimeArgs& a, const double* s_acc, int b, int k, int lane,
                                                     double lo, double hi, double h2) {
  const int D = a.D;
  double v, qL, qR;
  if (lane < D) {
    retime_state<TRAJ>(a, b, k, lane, v, qL, qR);
    return retime_row_start(qR, v, s_acc[lane]);
  }
  if (lane < 2 * D) {
    retime_state<TRAJ>(a, b, k + 1, lane - D, v, qL, qR);
    return retime_row_end(qL, v, s_acc[lane - D], h2);
  }
  if (lane == 2 * D) return retime_row_next(lo, hi, h2);
  return RetimeRow{-HUGE_VAL, HUGE_VAL, 0.0, HUGE_VAL};
}

}  // namespace

template <bool TRAJ>
__global__ __launch_bounds__(64) void k_retime(RetimeArgs a) {
#pragma clang fp contract(off)   // what is written out here joins the rule: rounded once, as retime_rule.h
  __shared__ double s_acc[GPMP2MI_MAX_DOF], s_vel[GPMP2MI_MAX_DOF];
  __shared__ double s_pl[64], s_pu[64], s_r[64];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int D = a.D, Md = a.Md, n = 2 * D + 1;
  const double h2 = 2.0 * a.h;
#pragma unroll
  for (int d = 0; d < GPMP2MI_MAX_DOF; d++)   // static indices into the kernel argument
    if (lane == d) { s_acc[d] = a.acc[d]; s_vel[d] = a.vel[d]; }
  __syncthreads();
  const RetimeMem w = retime_mem(a, b);
  int status = RETIME_OK;

  // caps and finiteness, a lane per state
  if (__any(retime_caps_pass<TRAJ>(a, s_vel, w, b, lane, [](int) { return 0; }))) status = RETIME_INVALID;
  __syncthreads();

  // backward: the controllable sets; forward: greedy.  Both form the rows of a stage in its lanes.
  const auto rowfn = [&](int k, double klo, double khi) { return retime_lane_row<TRAJ>(a, s_acc, b, k, lane, klo, khi, h2); };
  double lo, hi;
  retime_backward(a, w, s_pl, s_pu, s_r, n, lane, status, lo, hi, rowfn);
  __syncthreads();   // K is read below by every lane
  retime_forward(a, w, lane, status, lo, hi, h2, rowfn);
  __syncthreads();   // x and u are read below by every lane

  double duration = HUGE_VAL;
  double ach[4] = {0.0, 0.0, 0.0, 0.0};
  if (status == RETIME_OK) {
    retime_achieved_acc<TRAJ>(a, s_acc, w, b, lane, h2, ach);
    __syncthreads();   // x is read; the rates take its place
    retime_rates<TRAJ>(a, s_vel, w, b, lane, ach);
#pragma unroll
    for (int c = 0; c < 4; c++) ach[c] = wave_max(ach[c]);
    __syncthreads();   // the rates are read by the neighbouring lanes
    if (retime_stage_times(Md, w, lane, h2)) status = RETIME_EMPTY;
  }
  __syncthreads();
  if (status == RETIME_OK) {
    duration = retime_stamp_sum(Md, w.stamps, lane);
  } else {
    const double nn = nan("");
    for (int k = lane; k < Md; k += 64) w.x[k] = w.u[k] = w.stamps[k] = nn;
#pragma unroll
    for (int c = 0; c < 4; c++) ach[c] = nn;
  }
  if (lane == 0) {
    if (a.status) a.status[b] = status;
    if (a.duration) a.duration[b] = duration;
    if (a.achieved)
      for (int c = 0; c < 4; c++) a.achieved[4 * b + c] = ach[c];
  }
  retime_dense<TRAJ>(a, w.x, b, lane);
}

// The selection of gpmp2mi_plan_select_retimed: one workgroup, rows by thread.
__global__ __launch_bounds__(256) void k_retime_finish(RetimeFinish a) {
  const ScoreFinish& f = a.sel;
  RowPick mine;
  for (int b = threadIdx.x; b < f.B; b += blockDim.x) {
    const double fe = f.ferr[b];
    if (retime_row_ok(a, f, b, fe)) mine.take(fe, b);
  }
  select_finish(f, mine);   // f.best is never null here (launch_retime_finish)
  __syncthreads();   // best, and dense_best as interpolated
  const int best = *f.best;
  if (best < 0) return;
  retime_copy_best(a, f, best);
}

int launch_retime_caps(const RobotDev& h, const RobotDev* R, double dt, int inter, int B, int N, const double* traj,
                       double* ps, hipStream_t st) {
  int Md, nblk;
  if (const int rc = checked_grid(N, inter, SCORE_TILE, B, 1, Md, nblk)) return rc;
  const dim3 grid((unsigned)(nblk * B)), block(64 * score_waves(h.nr_spheres));
  if (h.kind == GPMP2MI_ROBOT_POINT) {
    k_retime_caps<GPMP2MI_ROBOT_POINT, 0, 0><<<grid, block, 0, st>>>(R, dt, inter, N, Md, nblk, traj, ps);
  } else if (h.kind == GPMP2MI_ROBOT_ARM) {
    G2_DISPATCH_ROBOT_ARM_ONLY(h.arm_dof, (k_retime_caps<GPMP2MI_ROBOT_ARM, AD_, 0><<<grid, block, 0, st>>>(
                                              R, dt, inter, N, Md, nblk, traj, ps)));
  } else {
    set_error("re-timing is not built for the Pose2 kinds: the acceleration of the tangent-space interpolation is missing");
    return GPMP2MI_ERR_UNSUPPORTED;
  }
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_retime(const RetimeArgs& a, bool traj, hipStream_t st) {
  if (a.D < 1 || a.D > GPMP2MI_MAX_DOF || a.Md < 2) {
    set_error("k_retime: dof outside 1..GPMP2MI_MAX_DOF or fewer than two states");
    return GPMP2MI_ERR_INVALID;
  }
  if (traj) k_retime<true><<<dim3(a.B), dim3(64), 0, st>>>(a);
  else k_retime<false><<<dim3(a.B), dim3(64), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_retime_finish(const RetimeFinish& a, hipStream_t st) {
  if (!a.sel.select || !a.sel.best) {
    set_error("k_retime_finish: the selection needs a place for `best`");
    return GPMP2MI_ERR_INVALID;
  }
  return launch_finish(k_retime_finish, a, 1, a.sel.B, st);
}

}  // namespace g2
