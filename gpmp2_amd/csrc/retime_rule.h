// retime_rule.h -- the rule of include/gpmp2mi.h "re-timing", stated once for the kernels (retime_kernels.hip) and for a
// host compiler (tests/cpp/retime_shim.cpp): time-optimal path parameterisation by reachability for box limits on joint
// speed, joint acceleration and a per-state cap.  Plain C++.  Every operation is rounded once in the order written (no
// fused multiply-add): the ends of the controllable sets and the squared rates are minima and maxima of such quotients,
// so they do not depend on the order in which rows and pairs are visited, and the kernels, which spread them over the
// lanes of a wavefront, give the bits of the serial pass at the end of this file.
//
// One row: x_k = sdot_k^2 at the Md checked states, u_k constant over stage k = 0 .. Md-2, x_{k+1} = x_k + 2 h u_k.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define G2_RETIME_HD __host__ __device__ inline
#else
#define G2_RETIME_HD inline
#endif
#if defined(__clang__)
#define G2_RETIME_EXACT _Pragma("clang fp contract(off)")
#else
#define G2_RETIME_EXACT   // a host compiler is given -ffp-contract=off
#endif

namespace g2 {

// the values of GPMP2MI_RETIME_* (include/gpmp2mi.h)
constexpr int RETIME_OK = 0, RETIME_BOUNDARY = 1, RETIME_EMPTY = 2, RETIME_INVALID = 3;

// The acceleration of the interpolated mean at the two ends of an interval: the expressions of "motion limits".
G2_RETIME_HD void retime_acc_ends(double dt, double dx, double v0, double v1, double& a0, double& a1) {
  G2_RETIME_EXACT
  const double w = 6.0 / (dt * dt);
  const double wx = w * dx;
  a0 = wx - (4.0 * v0 + 2.0 * v1) / dt;
  a1 = -wx + (2.0 * v0 + 4.0 * v1) / dt;
}
// q'' at sub-state j of J1 = inter_step + 1 inside an interval: linear between its ends, the ends themselves exact
G2_RETIME_HD double retime_acc_at(double a0, double a1, int j, int J1) {
  G2_RETIME_EXACT
  if (j == 0) return a0;
  if (j == J1) return a1;
  return a0 + (a1 - a0) * ((double)j / (double)J1);
}

// (limit / |denom|)^2, the cap a rate limit puts on x; a zero denominator or an infinite limit caps nothing
G2_RETIME_HD double retime_cap(double limit, double denom) {
  G2_RETIME_EXACT
  const double a = std::fabs(denom);
  if (a == 0.0 || !(limit < HUGE_VAL)) return HUGE_VAL;
  const double r = limit / a;
  return r * r;
}

// What one row leaves: the lower bound u >= pl + r x, the upper bound u <= pu + r x (the same slope), and a cap on x.
// A row that bounds nothing is (-inf, +inf, 0, +inf): it passes through every step below without an effect.
struct RetimeRow {
  double pl, pu, r, xcap;
};
// the two-sided row |a x + b u| <= A
G2_RETIME_HD RetimeRow retime_row(double a, double b, double A) {
  G2_RETIME_EXACT
  RetimeRow o{-HUGE_VAL, HUGE_VAL, 0.0, HUGE_VAL};
  if (!(A < HUGE_VAL)) return o;
  if (b == 0.0) {
    if (a != 0.0) o.xcap = A / std::fabs(a);
    return o;
  }
  o.pu = A / std::fabs(b);
  o.pl = -o.pu;
  o.r = -a / b;
  return o;
}
// the two rows of joint d in stage k: at its start from (q''_{k+}, q'_k), at its end from (q''_{(k+1)-}, q'_{k+1})
G2_RETIME_HD RetimeRow retime_row_start(double qdd_right, double qd, double A) { return retime_row(qdd_right, qd, A); }
G2_RETIME_HD double retime_end_b(double qdd_left, double qd, double h2) {
  G2_RETIME_EXACT
  return qd + h2 * qdd_left;
}
G2_RETIME_HD RetimeRow retime_row_end(double qdd_left, double qd, double A, double h2) {
  return retime_row(qdd_left, retime_end_b(qdd_left, qd, h2), A);
}
// the next set K_{k+1} = [lo, hi] as a row: (lo - x) / 2h <= u <= (hi - x) / 2h
G2_RETIME_HD RetimeRow retime_row_next(double lo, double hi, double h2) {
  G2_RETIME_EXACT
  return RetimeRow{lo / h2, hi / h2, -1.0 / h2, HUGE_VAL};
}

// One (lower i, upper j) pair of the elimination of u: (r_i - r_j) x <= pu_j - pl_i
G2_RETIME_HD void retime_pair(const RetimeRow& lower, const RetimeRow& upper, double& lo, double& hi, int& empty) {
  G2_RETIME_EXACT
  const double al = lower.r - upper.r, be = upper.pu - lower.pl;
  if (al > 0.0) {
    const double q = be / al;
    if (q < hi) hi = q;
  } else if (al < 0.0) {
    const double q = be / al;
    if (q > lo) lo = q;
  } else if (be < 0.0) {
    empty = 1;
  }
}
// the upper bound of a row on u at x
G2_RETIME_HD double retime_upper_at(const RetimeRow& row, double x) {
  G2_RETIME_EXACT
  return row.pu + row.r * x;
}
// one greedy step: u_hi is the smallest upper bound at x; -> x_{k+1} clamped into [lo, hi] and the reported u
G2_RETIME_HD void retime_step(double x, double u_hi, double lo, double hi, double h2, double& x1, double& u) {
  G2_RETIME_EXACT
  double y = x + h2 * u_hi;
  if (y < lo) y = lo;
  if (y > hi) y = hi;
  x1 = y;
  u = (y - x) / h2;
}
// the executed time of stage k
G2_RETIME_HD double retime_stage_time(double sdot0, double sdot1, double h2) {
  G2_RETIME_EXACT
  return h2 / (sdot0 + sdot1);
}

// achieved: the acceleration of one row (a x + b u) against A, and of joint d at the middle of stage k, where
// x = x_k + h u_k, q'' = (q''_{k+} + q''_{(k+1)-}) / 2 and q' = q'_k + (h/2) q''_{k+} + (h/8) (q''_{(k+1)-} - q''_{k+})
G2_RETIME_HD double retime_acc_ratio(double a, double b, double x, double u, double A) {
  G2_RETIME_EXACT
  if (!(A < HUGE_VAL)) return 0.0;
  return std::fabs(a * x + b * u) / A;
}
G2_RETIME_HD double retime_mid_ratio(double qd, double qdd_right, double qdd_left1, double x, double u, double h, double A) {
  G2_RETIME_EXACT
  if (!(A < HUGE_VAL)) return 0.0;
  const double am = 0.5 * (qdd_right + qdd_left1);
  const double vm = qd + (0.5 * h) * qdd_right + (0.125 * h) * (qdd_left1 - qdd_right);
  const double xm = x + h * u;
  return std::fabs(am * xm + vm * u) / A;
}

// ---- the serial pass over one row given as arrays: the host side of gpmp2mi_retime_path ------------------------------
// qd, qdd_left, qdd_right [Md][D], cap [Md] (a bound on x, +inf: none), acc [D]; rate_start / rate_end < 0: free.
// K [Md][2], sdot, u, stamps [Md], achieved [4].  Returns the status; a row that is not OK has duration = +inf and NaN in
// sdot, u, stamps and achieved (K keeps what the backward pass reached).
inline int retime_path_row(int Md, int D, const double* qd, const double* qdd_left, const double* qdd_right,
                           const double* cap, const double* acc, double h, double max_rate, double rate_start,
                           double rate_end, double* K, double* sdot, double* u, double* stamps, double* duration,
                           double* achieved) {
  G2_RETIME_EXACT
  const double h2 = 2.0 * h, X0 = max_rate * max_rate;
  const double nan = std::nan("");
  auto fail = [&](int status) {
    for (int k = 0; k < Md; k++) sdot[k] = u[k] = stamps[k] = nan;
    for (int c = 0; c < 4; c++) achieved[c] = nan;
    *duration = HUGE_VAL;
    return status;
  };
  auto X = [&](int k) { return cap[k] < X0 ? cap[k] : X0; };
  for (int k = 0; k < Md; k++) {
    bool bad = !(cap[k] >= 0.0);
    for (int d = 0; d < D; d++) {
      bad = bad || !std::isfinite(qd[k * D + d]);
      if (k > 0) bad = bad || !std::isfinite(qdd_left[k * D + d]);
      if (k < Md - 1) bad = bad || !std::isfinite(qdd_right[k * D + d]);
    }
    if (bad) return fail(RETIME_INVALID);
  }
  for (int k = 0; k < 2 * Md; k++) K[k] = nan;
  // backward: the controllable sets
  double lo = 0.0, hi = X(Md - 1);
  if (rate_end >= 0.0) {
    lo = rate_end * rate_end;
    if (lo > hi) return fail(RETIME_BOUNDARY);
    hi = lo;
  }
  K[2 * (Md - 1)] = lo;
  K[2 * (Md - 1) + 1] = hi;
  auto stage_row = [&](int k, int r, double nlo, double nhi) {
    if (r < D) return retime_row_start(qdd_right[k * D + r], qd[k * D + r], acc[r]);
    if (r < 2 * D) return retime_row_end(qdd_left[(k + 1) * D + r - D], qd[(k + 1) * D + r - D], acc[r - D], h2);
    return retime_row_next(nlo, nhi, h2);
  };
  const int n = 2 * D + 1;
  for (int k = Md - 2; k >= 0; k--) {
    double l = 0.0, t = X(k);
    int empty = 0;
    for (int i = 0; i < n; i++) {
      const RetimeRow ri = stage_row(k, i, lo, hi);
      if (ri.xcap < t) t = ri.xcap;
      for (int j = 0; j < n; j++) retime_pair(ri, stage_row(k, j, lo, hi), l, t, empty);
    }
    if (empty || l > t) return fail(RETIME_EMPTY);
    lo = K[2 * k] = l;
    hi = K[2 * k + 1] = t;
  }
  // forward: greedy
  double x = hi;
  if (rate_start >= 0.0) {
    x = rate_start * rate_start;
    if (x < lo || x > hi) return fail(RETIME_BOUNDARY);
  }
  sdot[0] = x;
  for (int k = 0; k < Md - 1; k++) {
    double uh = HUGE_VAL;
    for (int i = 0; i < n; i++) {
      const double v = retime_upper_at(stage_row(k, i, K[2 * k + 2], K[2 * k + 3]), x);
      if (v < uh) uh = v;
    }
    double x1;
    retime_step(x, uh, K[2 * k + 2], K[2 * k + 3], h2, x1, u[k]);
    sdot[k + 1] = x = x1;
  }
  u[Md - 1] = 0.0;
  // achieved, from x and the reported u
  double av = 0.0, ae = 0.0, am = 0.0;
  for (int k = 0; k < Md - 1; k++)
    for (int d = 0; d < D; d++) {
      const double q0 = qd[k * D + d], q1 = qd[(k + 1) * D + d];
      const double aR = qdd_right[k * D + d], aL = qdd_left[(k + 1) * D + d];
      const double e0 = retime_acc_ratio(aR, q0, sdot[k], u[k], acc[d]);
      const double e1 = retime_acc_ratio(aL, retime_end_b(aL, q1, h2), sdot[k], u[k], acc[d]);
      const double m = retime_mid_ratio(q0, aR, aL, sdot[k], u[k], h, acc[d]);
      if (e0 > ae) ae = e0;
      if (e1 > ae) ae = e1;
      if (m > am) am = m;
    }
  for (int k = 0; k < Md; k++) {
    sdot[k] = std::sqrt(sdot[k]);
    if (cap[k] < HUGE_VAL && cap[k] > 0.0) {
      const double r = sdot[k] / std::sqrt(cap[k]);
      if (r > av) av = r;
    }
  }
  // the stamps, summed in index order
  stamps[0] = 0.0;
  for (int k = 0; k < Md - 1; k++) {
    if (sdot[k] + sdot[k + 1] == 0.0) return fail(RETIME_EMPTY);
    stamps[k + 1] = stamps[k] + retime_stage_time(sdot[k], sdot[k + 1], h2);
  }
  *duration = stamps[Md - 1];
  achieved[0] = av;
  achieved[1] = ae;
  achieved[2] = am;
  achieved[3] = 0.0;
  return RETIME_OK;
}

}  // namespace g2
