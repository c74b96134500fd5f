// dyn_walk.h -- what the two outward walks of inverse dynamics along a fixed-base arm share: k_torque
// (torque_kernels.hip, NS = 2 sides) and k_retime_coef (retime_dynamic_kernels.hip, NS = 3).  A lane is a checked state
// and walks the chain once.  Shared: the vector products, the staging of the inertial table and the LDS columns.  The
// loop over the links stands in each kernel: both units are compiled with the compiler's default contraction, and a
// loop moved into one function is optimised on its own before it is inlined, which changes which products fuse and so
// the bits of tau and coef ("re-timing under torque limits").
//
// The walk: inverse dynamics in the world frame during one outward pass, without a backward pass.  It carries the
// angular velocity w, the angular acceleration wd and the acceleration ao of the current joint origin.  When link i is
// reached it forms the link's force f = m a(c) and moment n = I wd + w x I w about its centre of mass c (I = R Ibar R^T,
// applied in the link frame), and adds z_k . (n + (c - o_k) x f) to the torque of every joint k <= i at once: O(AD^2)
// small products, and nothing per link is kept but the joint axes and origins and the torque vectors.  The motion part
// m = ID(q, v, a) with gravity off and the gravity part tau_g = ID(q, 0, 0) are accumulated apart (the dynamics are
// affine in gravity, tau = tau_g + m): a row at rest has m == 0 exactly, and m is what a stretch of the duration scales.
//
// Sides: side 0 is the acceleration in the interval the state opens or lies in (the last state: the one it closes);
// a support state between two intervals has a side 1, the end of the interval before it.  k_retime_coef has a side 2,
// the walk of (0, q'): it has no velocity terms (neither the centripetal nor the gyroscopic part) and gives
// p = M(q) q', every term of it a product with a q'.
//
// Where the per-joint state lives: in LDS, one column per lane (DynLds), and the walk is a loop, not an unrolled
// chain as Kin::walk_links is.  Unrolled with everything in registers (6 AD doubles of axes, 3 AD of torques, the state
// of the joints still ahead) the compiler needed 100 VGPRs per joint and spilled from five joints on, whatever the
// register budget and however the links were fenced (profiles/torque_resources.txt has the table).  A lane's column is
// its own: no barrier, and [slot][lane] has no bank conflict.
#pragma once

#include "launch.h"
#include "retime_rule.h"
#include "score_select.h"

namespace g2 {

__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// the inertial table into LDS, by words; stage_robot's barrier closes this copy as well
__device__ __forceinline__ void stage_dyn(DynDev* lds, const DynDev* g) {
  const int* s = reinterpret_cast<const int*>(g);
  int* d = reinterpret_cast<int*>(lds);
  for (int i = threadIdx.x; i < (int)(sizeof(DynDev) / 4); i += blockDim.x) d[i] = s[i];
}

// per lane (column): the axis and the origin of every joint reached so far, and per joint NS + 1 torque slots: slot
// s < NS the motion torque of side s, slot NS tau_g
template <int AD, int NS>
struct DynLds {
  double ax[6 * AD][SCORE_TILE], tq[(NS + 1) * AD][SCORE_TILE];
};

}  // namespace g2
