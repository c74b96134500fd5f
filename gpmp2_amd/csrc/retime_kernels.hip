// retime_kernels.hip -- the speed profile of the executed trajectory behind gpmp2mi_retime_path / gpmp2mi_retime_traj /
// gpmp2mi_plan_retime / gpmp2mi_plan_select_retimed (include/gpmp2mi.h "re-timing"): along the unchanged path, the rate
// sdot_k of planned against executed time at every checked state that makes the duration as short as the joint speeds,
// joint accelerations and the Cartesian sphere speed allow.  The rule is retime_rule.h; these kernels spread it.
//
//   k_retime_caps    tiled as k_motion is (checked_grid, score_select.h): a lane is a checked state, a workgroup covers
//                    SCORE_TILE consecutive states of one trajectory, its `nsub` wavefronts share the spheres.  Writes
//                    ps_k, the largest sphere speed of the state (NaN when one of them is not finite).
//   k_retime         one wavefront per row.  Caps X_k and the finiteness of the row, a lane per state.  Then the chain:
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
#include "retime_rule.h"
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

// q'_k, q''_{k-} and q''_{k+} of coordinate d at checked state k of row b (qL: k > 0, qR: k < Md - 1; else 0)
template <bool TRAJ>
__device__ __forceinline__ void retime_state(const RetimeArgs& a, int b, int k, int d, double& v, double& qL, double& qR) {
  const int D = a.D;
  if constexpr (!TRAJ) {
    const size_t at = ((size_t)b * a.Md + k) * D + d;
    v = a.qd[at];
    qL = k > 0 ? a.ql[at] : 0.0;
    qR = k < a.Md - 1 ? a.qr[at] : 0.0;
  } else {
    const int J1 = a.inter + 1, seg = k / J1, j = k % J1;
    const double* s0 = a.traj + ((size_t)b * (a.N + 1) + seg) * 2 * D;
    qL = qR = 0.0;
    if (j == 0) {
      v = s0[D + d];
    } else {   // the velocity half of score_dense_coord (score_select.h), vector coordinates
      const double* s1 = s0 + 2 * D;
      const GpCoef gc = gp_coef_dev(a.dt, (double)j * (a.dt / (double)J1));
      v = gc.l21 * s0[d] + gc.l22 * s0[D + d] + gc.p21 * s1[d] + gc.p22 * s1[D + d];
    }
    if (seg < a.N) {
      const double* s1 = s0 + 2 * D;
      double a0, a1;
      retime_acc_ends(a.dt, s1[d] - s0[d], s0[D + d], s1[D + d], a0, a1);
      qR = retime_acc_at(a0, a1, j, J1);
      if (j > 0) qL = qR;
    }
    if (j == 0 && seg > 0) {
      const double* sp = s0 - 2 * D;
      double a0, a1;
      retime_acc_ends(a.dt, s0[d] - sp[d], sp[D + d], s0[D + d], a0, a1);
      qL = a1;
    }
  }
}

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

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_xor(v, off);
    if (o < v) v = o;
  }
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_xor(v, off);
    if (o > v) v = o;
  }
  return v;
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
  double* X = a.X + (size_t)b * Md;
  double* Kw = a.K + (size_t)b * Md * 2;
  double* x = a.sdot + (size_t)b * Md;   // x_k until the rates replace it
  double* u = a.u + (size_t)b * Md;
  double* stamps = a.stamps + (size_t)b * Md;
  int status = RETIME_OK;

  // caps and finiteness, a lane per state
  {
    const double X0 = a.max_rate * a.max_rate;
    int bad = 0;
    for (int k = lane; k < Md; k += 64) {
      double c = X0;
      for (int d = 0; d < D; d++) {
        double v, qL, qR;
        retime_state<TRAJ>(a, b, k, d, v, qL, qR);
        bad |= !isfinite(v) || !isfinite(qL) || !isfinite(qR);
        if constexpr (TRAJ) {
          const double cv = retime_cap(s_vel[d], v);
          if (cv < c) c = cv;
        }
      }
      if constexpr (TRAJ) {
        const double p = a.ps[(size_t)b * Md + k];
        bad |= !isfinite(p);
        const double cp = retime_cap(a.point_speed, p);
        if (cp < c) c = cp;
      } else {
        const double cc = a.cap[(size_t)b * Md + k];
        bad |= !(cc >= 0.0);
        if (cc < c) c = cc;
      }
      X[k] = c;
    }
    if (__any(bad)) status = RETIME_INVALID;
  }
  __syncthreads();

  // backward: the controllable sets
  double lo = 0.0, hi = 0.0;
  if (status == RETIME_OK) {
    hi = X[Md - 1];
    if (a.rate_end >= 0.0) {
      lo = a.rate_end * a.rate_end;
      if (lo > hi) status = RETIME_BOUNDARY;
      hi = lo;
    }
  }
  if (status == RETIME_OK) {
    if (lane == 0) { Kw[2 * (Md - 1)] = lo; Kw[2 * (Md - 1) + 1] = hi; }
    const int q64 = 64 / n, r64 = 64 % n;
    for (int k = Md - 2; k >= 0; k--) {
      const RetimeRow row = retime_lane_row<TRAJ>(a, s_acc, b, k, lane, lo, hi, h2);
      s_pl[lane] = row.pl;
      s_pu[lane] = row.pu;
      s_r[lane] = row.r;
      __syncthreads();
      double l = 0.0, t = X[k];
      if (row.xcap < t) t = row.xcap;
      int empty = 0;
      int i = lane / n, j = lane % n;
      for (int p = lane; p < n * n; p += 64) {
        retime_pair(RetimeRow{s_pl[i], 0.0, s_r[i], 0.0}, RetimeRow{0.0, s_pu[j], s_r[j], 0.0}, l, t, empty);
        i += q64;
        j += r64;
        if (j >= n) { j -= n; i++; }
      }
      __syncthreads();   // the rows of this stage are read
      l = wave_max(l);
      t = wave_min(t);
      if (__any(empty) || l > t) {
        status = RETIME_EMPTY;
        break;
      }
      lo = l;
      hi = t;
      if (lane == 0) { Kw[2 * k] = lo; Kw[2 * k + 1] = hi; }
    }
  }
  __syncthreads();   // K is read below by every lane

  // forward: greedy
  double xk = hi;
  if (status == RETIME_OK && a.rate_start >= 0.0) {
    xk = a.rate_start * a.rate_start;
    if (xk < lo || xk > hi) status = RETIME_BOUNDARY;
  }
  if (status == RETIME_OK) {
    if (lane == 0) x[0] = xk;
    for (int k = 0; k < Md - 1; k++) {
      const double nlo = Kw[2 * k + 2], nhi = Kw[2 * k + 3];
      const RetimeRow row = retime_lane_row<TRAJ>(a, s_acc, b, k, lane, nlo, nhi, h2);
      const double uh = wave_min(retime_upper_at(row, xk));
      double x1, uk;
      retime_step(xk, uh, nlo, nhi, h2, x1, uk);
      if (lane == 0) { x[k + 1] = x1; u[k] = uk; }
      xk = x1;
    }
    if (lane == 0) u[Md - 1] = 0.0;
  }
  __syncthreads();   // x and u are read below by every lane

  double duration = HUGE_VAL;
  double ach[4] = {0.0, 0.0, 0.0, 0.0};
  if (status == RETIME_OK) {
    // achieved: the accelerations, a lane per (stage, joint)
    for (int e = lane; e < (Md - 1) * D; e += 64) {
      const int k = e / D, d = e % D;
      double v0, v1, l0, r0, l1, r1;
      retime_state<TRAJ>(a, b, k, d, v0, l0, r0);
      retime_state<TRAJ>(a, b, k + 1, d, v1, l1, r1);
      const double xs = x[k], us = u[k], A = s_acc[d];
      const double e0 = retime_acc_ratio(r0, v0, xs, us, A);
      const double e1 = retime_acc_ratio(l1, retime_end_b(l1, v1, h2), xs, us, A);
      const double m = retime_mid_ratio(v0, r0, l1, xs, us, a.h, A);
      if (e0 > ach[1]) ach[1] = e0;
      if (e1 > ach[1]) ach[1] = e1;
      if (m > ach[2]) ach[2] = m;
    }
    __syncthreads();   // x is read; the rates take its place
    for (int k = lane; k < Md; k += 64) {
      const double s = sqrt(x[k]);
      x[k] = s;
      if constexpr (TRAJ) {
        for (int d = 0; d < D; d++) {
          if (!(s_vel[d] < HUGE_VAL)) continue;
          double v, qL, qR;
          retime_state<TRAJ>(a, b, k, d, v, qL, qR);
          const double r = fabs(v) * s / s_vel[d];
          if (r > ach[0]) ach[0] = r;
        }
        if (a.point_speed < HUGE_VAL) {
          const double r = a.ps[(size_t)b * Md + k] * s / a.point_speed;
          if (r > ach[3]) ach[3] = r;
        }
      } else {
        const double c = a.cap[(size_t)b * Md + k];
        if (c < HUGE_VAL && c > 0.0) {
          const double r = s / sqrt(c);
          if (r > ach[0]) ach[0] = r;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 4; c++) ach[c] = wave_max(ach[c]);
    __syncthreads();   // the rates are read by the neighbouring lanes
    // the stage times, a lane per stage; then one sum in index order, the same in every lane
    int zero = 0;
    for (int k = lane; k < Md - 1; k += 64) {
      const double s0 = x[k], s1 = x[k + 1];
      zero |= s0 + s1 == 0.0;
      stamps[k + 1] = retime_stage_time(s0, s1, h2);
    }
    if (__any(zero)) status = RETIME_EMPTY;
  }
  __syncthreads();
  if (status == RETIME_OK) {
    double t = 0.0;
    if (lane == 0) stamps[0] = 0.0;
    for (int base = 0; base < Md - 1; base += 64) {
      const int k = base + lane;
      const double v = k < Md - 1 ? stamps[k + 1] : 0.0;
      double mine = 0.0;
#pragma unroll
      for (int i = 0; i < 64; i++) {
        t = t + __shfl(v, i);   // t + 0 behind the last stage leaves t as it is
        if (lane == i) mine = t;
      }
      if (k < Md - 1) stamps[k + 1] = mine;
    }
    duration = t;
  } else {
    const double nn = nan("");
    for (int k = lane; k < Md; k += 64) x[k] = u[k] = stamps[k] = nn;
#pragma unroll
    for (int c = 0; c < 4; c++) ach[c] = nn;
  }
  if (lane == 0) {
    if (a.status) a.status[b] = status;
    if (a.duration) a.duration[b] = duration;
    if (a.achieved)
      for (int c = 0; c < 4; c++) a.achieved[4 * b + c] = ach[c];
  }
  if constexpr (TRAJ) {
    if (a.dense) {
      __syncthreads();   // the rates (or the NaNs) of every state
      double* out = a.dense + (size_t)b * Md * 2 * D;
      const double* row = a.traj + (size_t)b * (a.N + 1) * 2 * D;
      for (int e = lane; e < Md * D; e += 64) {
        const int m = e / D, k = e % D;
        double* o = out + (size_t)m * 2 * D;
        score_dense_coord(false, a.dt, a.inter, D, m % (a.inter + 1), k, row + (size_t)(m / (a.inter + 1)) * 2 * D, o);
        o[D + k] = o[D + k] * x[m];
      }
    }
  }
}

// The selection of gpmp2mi_plan_select_retimed: one workgroup, rows by thread.
__global__ __launch_bounds__(256) void k_retime_finish(RetimeFinish a) {
  const ScoreFinish& f = a.sel;
  RowPick mine;
  for (int b = threadIdx.x; b < f.B; b += blockDim.x) {
    const double fe = f.ferr[b];
    bool ok = row_eligible(f, b, fe, a.clearance[b], a.oor[b]);
    if (a.self_clearance) ok = ok && a.self_invalid[b] == 0 && a.self_clearance[b] >= a.required_self_clearance;
    ok = ok && a.motion_invalid[b] == 0 && a.pos_margin[b] >= a.required_pos_margin;
    ok = ok && a.rstatus[b] == RETIME_OK && a.duration[b] <= a.max_duration;
    if (ok) mine.take(fe, b);
  }
  select_finish(f, mine);   // f.best is never null here (launch_retime_finish)
  __syncthreads();   // best, and dense_best as interpolated
  const int best = *f.best;
  if (best < 0) return;
  const double* sd = a.sdot + (size_t)best * f.Md;
  if (threadIdx.x == 0 && a.duration_best) *a.duration_best = a.duration[best];
  if (a.stamps_best)
    for (int m = threadIdx.x; m < f.Md; m += blockDim.x) a.stamps_best[m] = a.stamps[(size_t)best * f.Md + m];
  if (f.dense_best)
    for (int e = threadIdx.x; e < f.Md * f.D; e += blockDim.x) {   // the elements this thread wrote in select_finish
      const int m = e / f.D, k = e % f.D;
      double* o = f.dense_best + (size_t)m * 2 * f.D + f.D + k;
      *o = *o * sd[m];
    }
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
