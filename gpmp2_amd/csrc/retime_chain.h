// retime_chain.h -- the one chain of re-timing, shared by k_retime (retime_kernels.hip) and k_retime_dynamic
// (retime_dynamic_kernels.hip): one wavefront per row; the stages below in this order, the kernels' barriers between
// them.  The two kernels differ in where a stage's rows come from (`rowfn`: formed per lane, or read from the workspace
// k_retime_rows left), in what is tested per state beside the caps (`extra`), and in what the dynamic kernel has of
// its own (the affine `achieved`, tau_retimed).  Also the two stages the finish kernels share.
//
// Every function that rounds anything opens with G2_RETIME_EXACT: the pragma is scoped to a compound statement, and
// what is written out here joins the rule, rounded once as retime_rule.h.  retime_state is the exception, as it always
// was a function of its own: its values are the rule's inputs, not part of it.
#pragma once

#include "device_math.h"
#include "launch.h"
#include "retime_rule.h"
#include "score_select.h"

namespace g2 {

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

// the arrays of row b: the caps and the sets in the workspace, x_k (until the rates replace it), u and the stamps
struct RetimeMem {
  double *X, *Kw, *x, *u, *stamps;
};
__device__ __forceinline__ RetimeMem retime_mem(const RetimeArgs& a, int b) {
  return RetimeMem{a.X + (size_t)b * a.Md, a.K + (size_t)b * a.Md * 2, a.sdot + (size_t)b * a.Md, a.u + (size_t)b * a.Md,
                   a.stamps + (size_t)b * a.Md};
}

// Caps X_k and finiteness, a lane per state.  extra(k): what else is tested at state k; nonzero where the state makes
// the row invalid.  Returns this lane's flag.
template <bool TRAJ, class Extra>
__device__ __forceinline__ int retime_caps_pass(const RetimeArgs& a, const double* s_vel, const RetimeMem& w, int b, int lane,
                                                Extra extra) {
  G2_RETIME_EXACT
  const int D = a.D, Md = a.Md;
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
    bad |= extra(k);
    w.X[k] = c;
  }
  return bad;
}

// Backward: the controllable sets K_k = [lo, hi] into the workspace; lo, hi leave as K_0.  rowfn(k, lo, hi) is row
// `lane` of stage k, of n <= 64 rows, the last the next set; s_pl, s_pu, s_r hold one row per lane.  The n^2 pairs are
// strided over the lanes.  Every lane takes the same path: status is uniform (__any), and so is the break.
template <class RowFn>
__device__ __forceinline__ void retime_backward(const RetimeArgs& a, const RetimeMem& w, double* s_pl, double* s_pu,
                                                double* s_r, int n, int lane, int& status, double& lo, double& hi,
                                                RowFn rowfn) {
  G2_RETIME_EXACT
  const int Md = a.Md;
  lo = hi = 0.0;
  if (status == RETIME_OK) {
    hi = w.X[Md - 1];
    if (a.rate_end >= 0.0) {
      lo = a.rate_end * a.rate_end;
      if (lo > hi) status = RETIME_BOUNDARY;
      hi = lo;
    }
  }
  if (status == RETIME_OK) {
    if (lane == 0) { w.Kw[2 * (Md - 1)] = lo; w.Kw[2 * (Md - 1) + 1] = hi; }
    const int q64 = 64 / n, r64 = 64 % n;
    for (int k = Md - 2; k >= 0; k--) {
      const RetimeRow row = rowfn(k, lo, hi);
      s_pl[lane] = row.pl;
      s_pu[lane] = row.pu;
      s_r[lane] = row.r;
      __syncthreads();
      double l = 0.0, t = w.X[k];
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
      if (lane == 0) { w.Kw[2 * k] = lo; w.Kw[2 * k + 1] = hi; }
    }
  }
}

// Forward: greedy, from K_0 = [lo, hi]; every stage takes the smallest upper bound of the rows of the backward pass.
template <class RowFn>
__device__ __forceinline__ void retime_forward(const RetimeArgs& a, const RetimeMem& w, int lane, int& status, double lo,
                                               double hi, double h2, RowFn rowfn) {
  G2_RETIME_EXACT
  const int Md = a.Md;
  double xk = hi;
  if (status == RETIME_OK && a.rate_start >= 0.0) {
    xk = a.rate_start * a.rate_start;
    if (xk < lo || xk > hi) status = RETIME_BOUNDARY;
  }
  if (status == RETIME_OK) {
    if (lane == 0) w.x[0] = xk;
    for (int k = 0; k < Md - 1; k++) {
      const double nlo = w.Kw[2 * k + 2], nhi = w.Kw[2 * k + 3];
      const RetimeRow row = rowfn(k, nlo, nhi);
      const double uh = wave_min(retime_upper_at(row, xk));
      double x1, uk;
      retime_step(xk, uh, nlo, nhi, h2, x1, uk);
      if (lane == 0) { w.x[k + 1] = x1; w.u[k] = uk; }
      xk = x1;
    }
    if (lane == 0) w.u[Md - 1] = 0.0;
  }
}

// achieved[1], [2]: the accelerations at the stage ends and middles, a lane per (stage, joint)
template <bool TRAJ, int NA>
__device__ __forceinline__ void retime_achieved_acc(const RetimeArgs& a, const double* s_acc, const RetimeMem& w, int b,
                                                    int lane, double h2, double (&ach)[NA]) {
  G2_RETIME_EXACT
  const int D = a.D;
  for (int e = lane; e < (a.Md - 1) * D; e += 64) {
    const int k = e / D, d = e % D;
    double v0, v1, l0, r0, l1, r1;
    retime_state<TRAJ>(a, b, k, d, v0, l0, r0);
    retime_state<TRAJ>(a, b, k + 1, d, v1, l1, r1);
    const double xs = w.x[k], us = w.u[k], A = s_acc[d];
    const double e0 = retime_acc_ratio(r0, v0, xs, us, A);
    const double e1 = retime_acc_ratio(l1, retime_end_b(l1, v1, h2), xs, us, A);
    const double m = retime_mid_ratio(v0, r0, l1, xs, us, a.h, A);
    if (e0 > ach[1]) ach[1] = e0;
    if (e1 > ach[1]) ach[1] = e1;
    if (m > ach[2]) ach[2] = m;
  }
}

// the rates take the place of x, a lane per state; achieved[0], [3]: the joint speeds (path form: the cap) and the
// point speed
template <bool TRAJ, int NA>
__device__ __forceinline__ void retime_rates(const RetimeArgs& a, const double* s_vel, const RetimeMem& w, int b, int lane,
                                             double (&ach)[NA]) {
  G2_RETIME_EXACT
  const int D = a.D, Md = a.Md;
  for (int k = lane; k < Md; k += 64) {
    const double s = sqrt(w.x[k]);
    w.x[k] = s;
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
}

// the stage times, a lane per stage, at the stamps' places; true where a stage stands still (both rates zero)
__device__ __forceinline__ bool retime_stage_times(int Md, const RetimeMem& w, int lane, double h2) {
  G2_RETIME_EXACT
  int zero = 0;
  for (int k = lane; k < Md - 1; k += 64) {
    const double s0 = w.x[k], s1 = w.x[k + 1];
    zero |= s0 + s1 == 0.0;
    w.stamps[k + 1] = retime_stage_time(s0, s1, h2);
  }
  return __any(zero);
}

// the stamps: one sum of the stage times in index order, the same in every lane; returns the duration
__device__ __forceinline__ double retime_stamp_sum(int Md, double* stamps, int lane) {
  G2_RETIME_EXACT
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
  return t;
}

// dense_retimed: the checked states with their velocities multiplied by the rates x (or the NaNs) of every state
template <bool TRAJ>
__device__ __forceinline__ void retime_dense(const RetimeArgs& a, const double* x, int b, int lane) {
  G2_RETIME_EXACT
  if constexpr (TRAJ) {
    if (a.dense) {
      __syncthreads();   // the rates (or the NaNs) of every state
      const int D = a.D, Md = a.Md;
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

// ---- the finish kernels ------------------------------------------------------------------------------------------

// is row b eligible: the rule of the existing stages, a re-timed row and a duration within the bound
__device__ __forceinline__ bool retime_row_ok(const RetimeFinish& a, const ScoreFinish& f, int b, double fe) {
  bool ok = row_eligible(f, b, fe, a.clearance[b], a.oor[b]);
  if (a.self_clearance) ok = ok && a.self_invalid[b] == 0 && a.self_clearance[b] >= a.required_self_clearance;
  ok = ok && a.motion_invalid[b] == 0 && a.pos_margin[b] >= a.required_pos_margin;
  return ok && a.rstatus[b] == RETIME_OK && a.duration[b] <= a.max_duration;
}

// the chosen row's duration and stamps; the velocities of dense_best, as select_finish interpolated them, times its rates
__device__ __forceinline__ void retime_copy_best(const RetimeFinish& a, const ScoreFinish& f, int best) {
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

}  // namespace g2
