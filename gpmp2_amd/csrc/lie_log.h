// lie_log.h -- the SO(3) / SE(3) log maps and their derivatives, one copy for the workspace priors (k_workspace_prior,
// factor_kernels.hip), the inverse kinematics built on them (k_ik, ik_kernels.hip) and the workspace path
// (path_kernels.hip), whose check also needs the SO(3) exponential.
#pragma once
#include "device_math.h"

namespace g2 {

// --------------------------------------------------------------------------- SO(3) / SE(3) logs
// GTSAM 4.0 semantics (upstream, restated): SO3::Logmap / LogmapDerivative, Pose3::Logmap /
// LogmapDerivative with Barfoot's Q matrix.  Used by the workspace priors below.
__device__ __forceinline__ void skew3(const double* w, double* W) {
  W[0] = 0; W[1] = -w[2]; W[2] = w[1];
  W[3] = w[2]; W[4] = 0; W[5] = -w[0];
  W[6] = -w[1]; W[7] = w[0]; W[8] = 0;
}
__device__ __forceinline__ void rot3_logmap(const double* R, double* w) {
  const double R11 = R[0], R12 = R[1], R13 = R[2], R21 = R[3], R22 = R[4], R23 = R[5], R31 = R[6], R32 = R[7], R33 = R[8];
  const double tr = R11 + R22 + R33;
  constexpr double kPi = 3.14159265358979323846;
  if (fabs(tr + 1.0) < 1e-10) {
    if (fabs(R33 + 1.0) > 1e-10) {
      const double k = kPi / sqrt(2.0 + 2.0 * R33);
      w[0] = k * R13; w[1] = k * R23; w[2] = k * (1.0 + R33);
    } else if (fabs(R22 + 1.0) > 1e-10) {
      const double k = kPi / sqrt(2.0 + 2.0 * R22);
      w[0] = k * R12; w[1] = k * (1.0 + R22); w[2] = k * R32;
    } else {
      const double k = kPi / sqrt(2.0 + 2.0 * R11);
      w[0] = k * (1.0 + R11); w[1] = k * R21; w[2] = k * R31;
    }
  } else {
    double magnitude;
    const double tr_3 = tr - 3.0;
    if (tr_3 < -1e-7) {
      const double theta = acos((tr - 1.0) / 2.0);
      magnitude = theta / (2.0 * sin(theta));
    } else {
      magnitude = 0.5 - tr_3 * tr_3 / 12.0;
    }
    w[0] = magnitude * (R32 - R23);
    w[1] = magnitude * (R13 - R31);
    w[2] = magnitude * (R21 - R12);
  }
}
__device__ __forceinline__ void rot3_logmap_derivative(const double* w, double* H) {
  const double theta2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  for (int i = 0; i < 9; i++) H[i] = (i % 4 == 0) ? 1.0 : 0.0;
  if (theta2 <= 2.220446049250313e-16) return;
  const double theta = sqrt(theta2);
  double W[9], WW[9];
  skew3(w, W);
  mat3_mul(W, W, WW);
  const double k = 1.0 / (theta * theta) - (1.0 + cos(theta)) / (2.0 * theta * sin(theta));
  for (int i = 0; i < 9; i++) H[i] += 0.5 * W[i] + k * WW[i];
}
// SO3::Expmap by Rodrigues' formula, R row-major; theta^2 at or below the threshold of rot3_logmap_derivative takes
// the first-order branch I + [w]x.  Used by the workspace-path check (path_kernels.hip) between two targets.
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
__device__ __forceinline__ void pose3_logmap(const double* R, const double* T, double* xi) {
  double w[3];
  rot3_logmap(R, w);
  const double t = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  xi[0] = w[0]; xi[1] = w[1]; xi[2] = w[2];
  if (t < 1e-10) {
    xi[3] = T[0]; xi[4] = T[1]; xi[5] = T[2];
    return;
  }
  const double wn[3] = {w[0] / t, w[1] / t, w[2] / t};
  double W[9], WT[3], WWT[3];
  skew3(wn, W);
  const double Tan = tan(0.5 * t);
  for (int i = 0; i < 3; i++) WT[i] = W[i * 3] * T[0] + W[i * 3 + 1] * T[1] + W[i * 3 + 2] * T[2];
  for (int i = 0; i < 3; i++) WWT[i] = W[i * 3] * WT[0] + W[i * 3 + 1] * WT[1] + W[i * 3 + 2] * WT[2];
  for (int i = 0; i < 3; i++) xi[3 + i] = T[i] - (0.5 * t) * WT[i] + (1.0 - t / (2.0 * Tan)) * WWT[i];
}
__device__ __forceinline__ void pose3_logmap_derivative(const double* R, const double* T, double* H) {
  double xi[6], Jw[9], Q[9], Q2[9];
  pose3_logmap(R, T, xi);
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
    if (fabs(phi) > 1e-5) {
      const double sn = sin(phi), c = cos(phi);
      const double phi2 = phi * phi, phi3 = phi2 * phi, phi4 = phi3 * phi, phi5 = phi4 * phi;
      c1 = (phi - sn) / phi3;
      c2 = (1.0 - phi2 / 2.0 - c) / phi4;
      c3 = -0.5 * ((1.0 - phi2 / 2.0 - c) / phi4 - 3.0 * (phi - sn - phi3 / 6.0) / phi5);
    } else {
      c1 = 1.0 / 6.0;
      c2 = 1.0 / 24.0;
      c3 = -0.5 * (1.0 / 24.0 + 3.0 / 120.0);
    }
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
