// step_control.h -- the optimizer's step control as pure functions of a trajectory's scalars: the do/while of
// gpmp2::optimize (planner/BatchTrajOptimizer.cpp:248-307), LevenbergMarquardtOptimizer::tryLambda and
// DoglegOptimizerImpl::Iterate / ComputeDoglegPoint (GTSAM semantics restated from upstream).
// No buffer, no pointer into HBM, no thread index: the kernels load the scalars, call these, and store what changed;
// a plain host compiler builds the same text for the CPU tests (tests/cpp/control_shim.cpp).
#pragma once
#include <cmath>

#include "../../include/gpmp2mi.h"

#ifndef G2_PURE
#ifdef __HIPCC__
#define G2_PURE __host__ __device__ __forceinline__
#else
#define G2_PURE inline
#endif
#endif

namespace g2 {

// what the rules below read of a plan's settings (PlanParams::rules)
struct StepRules {
  int opt_type, max_iter, no_increase, fixed_iters;
  double rel_thresh, abs_tol, err_tol;
  double lm_lambda0, lm_factor, lm_upper, lm_lower, lm_min_fidelity, dl_delta0;
};

// gtsam::checkConvergence
G2_PURE bool check_convergence(double rel, double abs_, double err_tol, double cur, double nw) {
  if (nw <= err_tol) return true;
  const double abs_dec = cur - nw;
  const double rel_dec = abs_dec / cur;
  return (rel != 0.0 && rel_dec <= rel) || (abs_dec <= abs_);
}

// =============================================================================== outer loop
// Both return 0 iterate, 1 stop with the current values, 2 stop with the values before the last step (no-increase
// rollback); `status` is meaningful when the trajectory stops.
// The early exits before the loop (:248-268), on the error `err` of the initial values.
G2_PURE int first_decide(const StepRules& R, double err, int& status) {
  status = GPMP2MI_TRAJ_MAX_ITER;
  if (R.fixed_iters > 0) return 0;
  if (err <= R.err_tol) { status = GPMP2MI_TRAJ_ALREADY_OPTIMAL; return 1; }
  return R.max_iter <= 0 ? 1 : 0;
}
// The do/while test (:273-307) after a call to iterate() that returned: `it` iterations so far (this one included when
// it `counted`: an LM call that gives up does not), `prev` the error the last comparison kept (currentError),
// `err_after` the error of the values iterate() left.  A fixed-iteration round stops at its count or at the first
// call that did not count.
G2_PURE int loop_decide(const StepRules& R, int it, bool counted, double prev, double err_after, int& status) {
  status = GPMP2MI_TRAJ_MAX_ITER;
  if (R.fixed_iters > 0) return (it >= R.fixed_iters || !counted) ? 1 : 0;
  const bool conv = check_convergence(R.rel_thresh, R.abs_tol, R.err_tol, prev, err_after);
  if (it < R.max_iter && !conv) return 0;
  if (err_after > prev && R.no_increase) { status = GPMP2MI_TRAJ_ROLLED_BACK; return 2; }
  if (conv) status = GPMP2MI_TRAJ_CONVERGED;
  return 1;
}
// The Gauss-Newton fast path evaluates a trajectory once per pass: it == 0 is the first evaluation of a problem (pass 0
// of a plain run; a queue run loads problems at later passes), every later one follows a step that counted.
// k_assemble and k_gn_step_cr both call it on the same inputs, which only earlier kernels wrote, so they agree by
// construction.
G2_PURE int gn_decide(const StepRules& R, int it, double prev, double new_err, int& status) {
  return it == 0 ? first_decide(R, new_err, status) : loop_decide(R, it, true, prev, new_err, status);
}

// =============================================================================== one call to iterate()
// Outcome of a trial step.  `param` is the optimizer's own scalar afterwards (LM lambda, Dogleg trust radius).
struct TrialOutcome {
  double param;
  bool returned;   // GTSAM's iterate() returned
  bool moved;      // ... with new values (the trial point)
  bool retry;      // Dogleg: another trial point from the same linearization
  bool not_spd;    // the solve failed and the optimizer has no answer to that: stop with GPMP2MI_TRAJ_NOT_SPD
};

// GaussNewtonOptimizer::iterate: always accept
G2_PURE TrialOutcome gn_iterate(bool failed) { return TrialOutcome{0.0, !failed, !failed, false, failed}; }

// LevenbergMarquardtOptimizer::tryLambda: model fidelity test on gd = g.delta, dd = |delta|^2, lambda /= or *= factor,
// give up at lm_upper.  A failed solve counts as a bad step.
G2_PURE TrialOutcome lm_try_lambda(const StepRules& R, double lambda, double cur_err, double new_err, double gd,
                                   double dd, bool failed) {
  bool step_ok = false, stop = false;
  if (!failed) {
    const double old_lin = cur_err;
    const double lin_change = -(0.5 * gd - 0.5 * lambda * dd);
    if (lin_change >= 0) {
      const double cost_change = cur_err - new_err;
      if (lin_change > 2.220446049250313e-16 * old_lin) step_ok = (cost_change / lin_change) > R.lm_min_fidelity;
      if (fabs(cost_change) < R.rel_thresh * cur_err) stop = true;
    }
  }
  TrialOutcome o{lambda, false, false, false, false};
  if (step_ok) {
    o.returned = o.moved = true;
    lambda = fmax(R.lm_lower, lambda / R.lm_factor);
  } else if (!stop) {
    lambda *= R.lm_factor;
    if (lambda >= R.lm_upper) o.returned = true;  // give up: state unchanged
  } else {
    o.returned = true;                            // relative cost change tiny: state unchanged
  }
  o.param = lambda;
  return o;
}

// DoglegOptimizerImpl::Iterate(ONE_STEP_PER_ITERATION): gain ratio rho of the trial point with model decrease q and
// length xnorm, trust radius update
G2_PURE TrialOutcome dogleg_iterate(double Delta, double cur_err, double new_err, double q, double xnorm, bool failed) {
  TrialOutcome o{Delta, false, false, false, failed};
  if (failed) return o;
  const double f_error = cur_err, M_error = cur_err, new_M = M_error + q;
  const double rho = (fabs(f_error - new_err) < 1e-15 || fabs(M_error - new_M) < 1e-15)
                         ? 0.5 : (f_error - new_err) / (M_error - new_M);
  if (rho >= 0.75) { Delta = fmax(Delta, 3.0 * xnorm); o.returned = o.moved = true; }
  else if (rho >= 0.25) { o.returned = o.moved = true; }
  else if (rho >= 0.0) { if (Delta > 1e-5) Delta = 0.5 * Delta; o.returned = o.moved = true; }
  else if (Delta > 1e-5) { Delta *= 0.5; o.retry = true; }            // retry, same linearization
  else { o.returned = true; }                                         // zero step
  o.param = Delta;
  return o;
}

// Powell dogleg point for trust radius Delta (DoglegOptimizerImpl::ComputeDoglegPoint / ComputeBlend):
// dx_d = cu * g + cn * dx_n with model decrease q(dx_d), from g.g, g^T H g, g.dx_n and |dx_n|^2
G2_PURE void dogleg_blend(double gg, double gHg, double gn, double nn, double Delta, double& cu, double& cn,
                          double& q) {
  const double step = -gg / gHg;          // dx_u = step * g   (optimizeGradientSearch)
  const double uu = step * step * gg, un = step * gn;
  const double DeltaSq = Delta * Delta;
  if (DeltaSq < uu) {
    const double k = sqrt(DeltaSq / uu);
    cu = k * step;
    cn = 0.0;
    q = cu * gg + 0.5 * cu * cu * gHg;
  } else if (DeltaSq < nn) {
    const double a = uu - 2. * un + nn, bq = 2. * (un - uu), cq = uu - Delta * Delta;
    const double sq = sqrt(bq * bq - 4 * a * cq);
    const double tau1 = (-bq + sq) / (2. * a), tau2 = (-bq - sq) / (2. * a);
    const double tau = (0.0 <= tau1 && tau1 <= 1.0) ? tau1 : tau2;
    cu = (1. - tau) * step;
    cn = tau;
    // g^T x + 0.5 x^T H x with H dx_n = -g
    q = cu * gg + cn * gn + 0.5 * (cu * cu * gHg - 2.0 * cu * cn * gg - cn * cn * gn);
  } else {
    cu = 0.0;
    cn = 1.0;
    q = 0.5 * gn;
  }
}

}  // namespace g2
