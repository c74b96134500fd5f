// retime_affine_rule.h -- the rule of include/gpmp2mi.h "re-timing under torque limits", stated once for the kernels
// (retime_dynamic_kernels.hip) and for a host compiler (tests/cpp/retime_affine_shim.cpp): the re-timing rule of
// retime_rule.h with rows that carry an offset, |cx x + cu u + off| <= A.  Along a fixed path the joint torque is such a
// row: tau = p u + m x + tau_g with p = M(q) q', m = ID(q, q', q'') without gravity, x = sdot^2, u = sddot.  The row
// type, the elimination, the greedy step and the stamps are retime_rule.h's, which never assume pl == -pu; what is new is
// one row constructor, one status and two entries of `achieved`.  Plain C++, every operation rounded once in the order
// written, as there.
#pragma once
#include "retime_rule.h"

namespace g2 {

// the value of GPMP2MI_RETIME_STATIC (include/gpmp2mi.h): |off| >= A at a checked state, no timing helps
constexpr int RETIME_STATIC = 4;
// the widest stage: the rows of retime_rule.h and R <= RETIME_MAX_EXTRA affine rows at either end
constexpr int RETIME_MAX_EXTRA = 8;

// the row |cx x + cu u + off| <= A, that is -A - off <= cx x + cu u <= A - off.  off == 0: the bits of
// retime_row(cx, cu, A).
G2_RETIME_HD RetimeRow retime_row_affine(double cx, double cu, double off, double A) {
  G2_RETIME_EXACT
  RetimeRow o{-HUGE_VAL, HUGE_VAL, 0.0, HUGE_VAL};
  if (!(A < HUGE_VAL)) return o;
  const double lo = -A - off, hi = A - off;
  if (cu > 0.0) {
    o.pu = hi / cu;
    o.pl = lo / cu;
    o.r = -cx / cu;
  } else if (cu < 0.0) {
    o.pu = lo / cu;
    o.pl = hi / cu;
    o.r = -cx / cu;
  } else if (cx > 0.0) {   // bounds no u; with |off| < A the cap is > 0
    o.xcap = hi / cx;
  } else if (cx < 0.0) {
    o.xcap = lo / cx;
  }
  return o;
}
// the two rows of an affine constraint in stage k: at its start from (cx_{k+}, cu_k, off_k), at its end from
// (cx_{(k+1)-}, cu_{k+1}, off_{k+1}) written in (x_k, u_k), as retime_row_end writes the accelerations
G2_RETIME_HD RetimeRow retime_row_affine_start(double cx_right, double cu, double off, double A) {
  return retime_row_affine(cx_right, cu, off, A);
}
G2_RETIME_HD RetimeRow retime_row_affine_end(double cx_left, double cu, double off, double A, double h2) {
  return retime_row_affine(cx_left, retime_end_b(cx_left, cu, h2), off, A);
}
// achieved: one affine row at (x, u) against its bound, and what the offset alone takes of it
G2_RETIME_HD double retime_affine_value(double cx, double cu, double off, double x, double u) {
  G2_RETIME_EXACT
  return cx * x + cu * u + off;
}
G2_RETIME_HD double retime_affine_ratio(double cx, double cu, double off, double x, double u, double A) {
  G2_RETIME_EXACT
  if (!(A < HUGE_VAL)) return 0.0;
  return std::fabs(retime_affine_value(cx, cu, off, x, u)) / A;
}
G2_RETIME_HD double retime_static_ratio(double off, double A) {
  G2_RETIME_EXACT
  if (!(A < HUGE_VAL)) return 0.0;
  return std::fabs(off) / A;
}
// what a state's coefficients of one affine row say before any pass: 0 fine, 1 not finite (INVALID), 2 static.  A row
// without a bound is not looked at: it passes through every step without an effect, whatever it holds.
G2_RETIME_HD int retime_affine_check(bool has_left, double cx_left, bool has_right, double cx_right, double cu, double off,
                                     double A) {
  if (!(A < HUGE_VAL)) return 0;
  if (!std::isfinite(cu) || !std::isfinite(off) || (has_left && !std::isfinite(cx_left)) ||
      (has_right && !std::isfinite(cx_right)))
    return 1;
  return std::fabs(off) >= A ? 2 : 0;
}

// ---- the serial pass over one row given as arrays: the host side of gpmp2mi_retime_path_affine ------------------------
// The arguments of retime_path_row, and R affine rows per state: cx_left, cx_right, cu, off [Md][R] (cx_left of state 0
// and cx_right of state Md-1 are not read), bound [R] (+inf: none).  achieved [6]: [0..3] as retime_path_row, [4] the
// largest |cx x_k + cu u_k + off| / bound over the start and end rows of every stage, [5] the largest |off| / bound over
// the states.  With R == 0 or every bound +inf all outputs have the bits of retime_path_row.
inline int retime_affine_row(int Md, int D, int R, const double* qd, const double* qdd_left, const double* qdd_right,
                             const double* cap, const double* acc, const double* cx_left, const double* cx_right,
                             const double* cu, const double* off, const double* bound, double h, double max_rate,
                             double rate_start, double rate_end, double* K, double* sdot, double* u, double* stamps,
                             double* duration, double* achieved) {
  G2_RETIME_EXACT
  const double h2 = 2.0 * h, X0 = max_rate * max_rate;
  const double nan = std::nan("");
  auto fail = [&](int status) {
    for (int k = 0; k < Md; k++) sdot[k] = u[k] = stamps[k] = nan;
    for (int c = 0; c < 6; c++) achieved[c] = nan;
    *duration = HUGE_VAL;
    return status;
  };
  auto X = [&](int k) { return cap[k] < X0 ? cap[k] : X0; };
  int stat = 0;
  for (int k = 0; k < Md; k++) {
    bool bad = !(cap[k] >= 0.0);
    for (int d = 0; d < D; d++) {
      bad = bad || !std::isfinite(qd[k * D + d]);
      if (k > 0) bad = bad || !std::isfinite(qdd_left[k * D + d]);
      if (k < Md - 1) bad = bad || !std::isfinite(qdd_right[k * D + d]);
    }
    for (int r = 0; r < R; r++) {
      const int e = k * R + r;
      const int c = retime_affine_check(k > 0, cx_left[e], k < Md - 1, cx_right[e], cu[e], off[e], bound[r]);
      bad = bad || c == 1;
      stat |= c == 2;
    }
    if (bad) return fail(RETIME_INVALID);
  }
  for (int k = 0; k < 2 * Md; k++) K[k] = nan;
  if (stat) return fail(RETIME_STATIC);
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
    r -= 2 * D;
    if (r < R) return retime_row_affine_start(cx_right[k * R + r], cu[k * R + r], off[k * R + r], bound[r]);
    if (r < 2 * R) {
      const int e = (k + 1) * R + r - R;
      return retime_row_affine_end(cx_left[e], cu[e], off[e], bound[r - R], h2);
    }
    return retime_row_next(nlo, nhi, h2);
  };
  const int n = 2 * D + 2 * R + 1;
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
  double av = 0.0, ae = 0.0, am = 0.0, at = 0.0, as = 0.0;
  for (int k = 0; k < Md - 1; k++) {
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
    for (int r = 0; r < R; r++) {
      const int e0 = k * R + r, e1 = (k + 1) * R + r;
      const double t0 = retime_affine_ratio(cx_right[e0], cu[e0], off[e0], sdot[k], u[k], bound[r]);
      const double t1 =
          retime_affine_ratio(cx_left[e1], retime_end_b(cx_left[e1], cu[e1], h2), off[e1], sdot[k], u[k], bound[r]);
      if (t0 > at) at = t0;
      if (t1 > at) at = t1;
    }
  }
  for (int k = 0; k < Md; k++) {
    sdot[k] = std::sqrt(sdot[k]);
    if (cap[k] < HUGE_VAL && cap[k] > 0.0) {
      const double r = sdot[k] / std::sqrt(cap[k]);
      if (r > av) av = r;
    }
    for (int r = 0; r < R; r++) {
      const double s = retime_static_ratio(off[k * R + r], bound[r]);
      if (s > as) as = s;
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
  achieved[4] = at;
  achieved[5] = as;
  return RETIME_OK;
}

}  // namespace g2
