// lie_log.h -- the SO(3) / SE(3) log maps and their derivatives, one copy for the workspace priors (k_workspace_prior,
// factor_kernels.hip), the inverse kinematics built on them (k_ik, ik_kernels.hip) and the workspace path
// (path_kernels.hip), whose check also needs the SO(3) exponential.
#pragma once
#include "device_math.h"

namespace g2 {

// --------------------------------------------------------------------------- SO(3) / SE(3) logs
// GTSAM 4.0 semantics (upstream, restated) in WHAT is computed: SO3::Logmap / LogmapDerivative, Pose3::Logmap /
// LogmapDerivative with Barfoot's Q matrix, tangent order [omega; u].  HOW is no longer GTSAM's (DESIGN.md section 5,
// tests/test_gpu_lie3_maps.py): the log takes its angle from atan2 and, beyond 2 pi / 3, its axis from the symmetric part
// (no trace-based branches, no first-order branch at pi); Pose3's log keeps -w x T / 2 at every angle; the inverse
// Jacobian keeps [w]x / 2 at every angle and its [w]x^2 coefficient in half-angle form; Q's c1, c2, c3 come from their
// series below LIE_Q_SERIES_BELOW (and, in the limit, with the signs of the closed forms, which GTSAM 4.0's
// small-angle constants do not have).
__device__ __forceinline__ void skew3(const double* w, double* W) {
  W[0] = 0; W[1] = -w[2]; W[2] = w[1];
  W[3] = w[2]; W[4] = 0; W[5] = -w[0];
  W[6] = -w[1]; W[7] = w[0]; W[8] = 0;
}
// The axis of a rotation by more than 2 pi / 3 from its symmetric part (R + R^T) / 2 = c I + (1 - c) a a^T, through the
// largest diagonal entry (a_i^2 >= 1/3, so R_ii - c >= 1/2: nothing cancels), its sign such that a . v >= 0 for the skew
// part v; returns omega = theta a.  Written with selects, no indexed array: R, v and w stay in registers (an out-of-line
// copy or R[i * 4] would put them into scratch in every kernel that includes this).
__device__ __forceinline__ void rot3_log_far(const double* R, const double* v, double c, double theta, double* w) {
  const bool b1 = R[4] > R[0];                    // on equal entries the first: as the oracle's index loop
  const double m01 = b1 ? R[4] : R[0];
  const bool b2 = R[8] > m01;
  const double d = 1.0 - c;
  const double ai = sqrt(((b2 ? R[8] : m01) - c) / d), f = 1.0 / (2.0 * d * ai);
  const double s01 = (R[1] + R[3]) * f, s02 = (R[2] + R[6]) * f, s12 = (R[5] + R[7]) * f;
  const double a0 = b2 ? s02 : (b1 ? s01 : ai), a1 = b2 ? s12 : (b1 ? ai : s01), a2 = b2 ? ai : (b1 ? s12 : s02);
  if ((a0 * v[0] + a1 * v[1]) + a2 * v[2] < 0.0) theta = -theta;
  w[0] = theta * a0; w[1] = theta * a1; w[2] = theta * a2;
}
// omega of R (row-major): v = vee(R - R^T) / 2 has length sin(theta), c = (tr - 1) / 2 = cos(theta), theta = atan2 of
// the two (well conditioned at every angle; an R that is not quite a rotation gives no NaN).  While c > -1/2 the axis
// is v / |v|; beyond, v shrinks to nothing at pi and the axis comes from rot3_log_far.
__device__ __forceinline__ void rot3_logmap(const double* R, double* w) {
  const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
  const double s = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  const double c = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
  const double theta = atan2(s, c);
  if (c > -0.5) {
    const double m = s > 0.0 ? theta / s : 1.0;
    w[0] = m * v[0]; w[1] = m * v[1]; w[2] = m * v[2];
  } else {
    rot3_log_far(R, v, c, theta, w);
  }
}
// k = (1 - (t / 2) cot(t / 2)) / t^2, the coefficient of [w]x^2 in the inverse right Jacobian and in Pose3's log
// (GTSAM writes it 1 / t^2 - (1 + cos t) / (2 t sin t), which is 0 / 0 in doubles next to pi).  Its two terms cancel to
// eps / t^2, which [w]x^2 = O(t^2) brings back to eps: no series.  At t^2 <= 2.22e-16 the limit 1/12; the first omitted
// term there is t^2 / 720 <= 3.1e-19.
__device__ __forceinline__ double so3_k(double theta2) {
  if (theta2 <= 2.220446049250313e-16) return 1.0 / 12.0;
  const double theta = sqrt(theta2), h = 0.5 * theta;
  double sh, ch;
  sincos(h, &sh, &ch);   // one argument reduction: fewer registers than cos and sin apart, which k_ik is short of
  return (1.0 - h * ch / sh) / theta2;
}
__device__ __forceinline__ void rot3_logmap_derivative(const double* w, double* H) {
  const double theta2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double W[9], WW[9];
  skew3(w, W);
  mat3_mul(W, W, WW);
  const double k = so3_k(theta2);
  for (int i = 0; i < 9; i++) H[i] = ((i % 4 == 0) ? 1.0 : 0.0) + (0.5 * W[i] + k * WW[i]);
}
// SO3::Expmap by Rodrigues' formula, R row-major; theta^2 at or below 2.22e-16 takes the first-order branch I + [w]x
// (the omitted [w]x^2 / 2 is at most 1.1e-16).  Used by the workspace-path check (path_kernels.hip) between two targets.
__device__ __forceinline__ void rot3_expmap(const double* w, double* R) {
  const double theta2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double W[9];
  skew3(w, W);
  for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + W[i];
  if (theta2 <= 2.220446049250313e-16) return;
  const double theta = sqrt(theta2);
  double WW[9];
  mat3_mul(W, W, WW);
  const double a = sin(theta) / theta, b = (1.0 - cos(theta)) / theta2;
  for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + (a * W[i] + b * WW[i]);
}
// xi = [omega; u], u = V(omega)^-1 T = T - w x T / 2 + k w x (w x T), at every angle
__device__ __forceinline__ void pose3_logmap(const double* R, const double* T, double* xi) {
  double w[3];
  rot3_logmap(R, w);
  xi[0] = w[0]; xi[1] = w[1]; xi[2] = w[2];
  const double k = so3_k(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double WT[3] = {w[1] * T[2] - w[2] * T[1], w[2] * T[0] - w[0] * T[2], w[0] * T[1] - w[1] * T[0]};
  const double WWT[3] = {w[1] * WT[2] - w[2] * WT[1], w[2] * WT[0] - w[0] * WT[2], w[0] * WT[1] - w[1] * WT[0]};
  for (int i = 0; i < 3; i++) xi[3 + i] = T[i] - 0.5 * WT[i] + k * WWT[i];
}
// Barfoot's coefficients of Q:  c1 = (p - sin p) / p^3,  c2 = (1 - p^2 / 2 - cos p) / p^4,
// c3 = -(c2 - 3 (p - sin p - p^3 / 6) / p^5) / 2.  Every numerator cancels: what reaches Q is eps / p (c1, c3) and
// eps / p^2 (c2) for a unit u, 3e-11 at p = 1e-3.  Below LIE_Q_SERIES_BELOW each comes from five terms of its series in
// p^2; the first omitted term, p^10 / 13! (c1), p^10 / 14! (c2), p^10 / 15! (d), is below 1.6e-16 there, and the closed
// forms measure below 1e-15 from there on.
constexpr double LIE_Q_SERIES_BELOW = 0.25;
__device__ __forceinline__ void pose3_q_coefficients(double phi, double& c1, double& c2, double& c3) {
  const double x = phi * phi;
  if (phi < LIE_Q_SERIES_BELOW) {
    c1 = 1.0 / 6.0 - x * (1.0 / 120.0 - x * (1.0 / 5040.0 - x * (1.0 / 362880.0 - x * (1.0 / 39916800.0))));
    c2 = -(1.0 / 24.0 - x * (1.0 / 720.0 - x * (1.0 / 40320.0 - x * (1.0 / 3628800.0 - x * (1.0 / 479001600.0)))));
    const double d = -(1.0 / 120.0 - x * (1.0 / 5040.0 - x * (1.0 / 362880.0 - x * (1.0 / 39916800.0 - x * (1.0 / 6227020800.0)))));
    c3 = -0.5 * (c2 - 3.0 * d);
  } else {
    const double sn = sin(phi), c = cos(phi);
    const double phi3 = x * phi, phi4 = x * x, phi5 = phi4 * phi;
    c1 = (phi - sn) / phi3;
    c2 = (1.0 - x / 2.0 - c) / phi4;
    c3 = -0.5 * (c2 - 3.0 * (phi - sn - phi3 / 6.0) / phi5);
  }
}
// d Log / d pose [6][6] at xi = pose3_logmap(R, T), which every caller has in hand already
__device__ __forceinline__ void pose3_logmap_derivative(const double* xi, double* H) {
  double Jw[9], Q[9], Q2[9];
  rot3_logmap_derivative(xi, Jw);
  {
    double V[9], W[9], WV[9], VW[9], WVW[9], WW[9], WWV[9], VWW[9], WVWW[9], WWVW[9];
    skew3(xi + 3, V);
    skew3(xi, W);
    mat3_mul(W, V, WV);
    mat3_mul(V, W, VW);
    mat3_mul(WV, W, WVW);
    mat3_mul(W, W, WW);
    mat3_mul(WW, V, WWV);
    mat3_mul(VW, W, VWW);
    mat3_mul(WVW, W, WVWW);
    mat3_mul(W, WVW, WWVW);
    const double phi = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
    double c1, c2, c3;
    pose3_q_coefficients(phi, c1, c2, c3);
    for (int i = 0; i < 9; i++)
      Q[i] = -0.5 * V[i] + c1 * (WV[i] + VW[i] - WVW[i]) + c2 * (WWV[i] + VWW[i] - 3.0 * WVW[i]) + c3 * (WVWW[i] + WWVW[i]);
  }
  mat3_mul(Jw, Q, Q2);
  double Q3[9];
  mat3_mul(Q2, Jw, Q3);
  for (int i = 0; i < 36; i++) H[i] = 0.0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      H[i * 6 + j] = Jw[i * 3 + j];
      H[(3 + i) * 6 + 3 + j] = Jw[i * 3 + j];
      H[(3 + i) * 6 + j] = -Q3[i * 3 + j];
    }
}

}  // namespace g2
