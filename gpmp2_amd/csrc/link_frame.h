// link_frame.h -- the frame of one link and its body Jacobian, column by column, for the kernels that follow a single
// link without storing poses or Jacobians (path_kernels.hip, carried_kernels.hip): the one device copy of that stage.
#pragma once
#include "device_math.h"
#include "dispatch.h"

namespace g2 {

// World frame F of `link` at q and the columns its tag covers (nc, first: ColTag); A as walk_links leaves it.
template <int KIND, int AD, int AD2>
__device__ __forceinline__ void link_frame(const RobotDev& R, const double (&q)[Kin<KIND, AD, AD2>::DOF], int link,
                                           typename Kin<KIND, AD, AD2>::Axes& A, Frame& F, int& nc, int& first) {
  using Kn = Kin<KIND, AD, AD2>;
  nc = first = 0;
  if constexpr (KIND == GPMP2MI_ROBOT_POINT) {   // the one frame of k_fk's point robot
    F.c0[0] = 1; F.c0[1] = 0; F.c0[2] = 0; F.c1[0] = 0; F.c1[1] = 1; F.c1[2] = 0;
    F.c2[0] = 0; F.c2[1] = 0; F.c2[2] = 1; F.t[0] = q[0]; F.t[1] = q[1]; F.t[2] = 0;
    nc = 2;
  } else {
    Kn::walk_links(R, q, A, [&](int l, const Frame& Fr, auto tag) {
      if (l == link) {
        F = Fr;
        nc = decltype(tag)::value;
        first = decltype(tag)::first;
      }
    });
  }
}

// Column `k` of the link's body Jacobian [omega; v] as k_fk forms it (factor_kernels.hip, put_col); zero for a column
// the link's tag does not cover and for k >= D.
template <int KIND, int AD, int AD2>
__device__ __forceinline__ void link_twist(const typename Kin<KIND, AD, AD2>::Axes& A, const Frame& F, int nc, int first,
                                           int k, double (&col)[6]) {
  using Kn = Kin<KIND, AD, AD2>;
  double w[3] = {0, 0, 0}, o[3] = {0, 0, 0};
  int trans = 0, on = 0;   // ints: as bools the two flags of the base-only kind are kept in scratch, one byte each
  static_for<0, Kn::DOF>([&](auto kc) {   // a chain of selects: the axes stay in registers
    constexpr int c = decltype(kc)::value;
    if (k != c) return;
    if constexpr (KIND == GPMP2MI_ROBOT_POINT) {
      w[c] = 1.0;
      trans = on = 1;
    } else if constexpr (Kn::MOBILE && c < 2) {
#pragma unroll
      for (int i = 0; i < 3; i++) w[i] = c == 0 ? A.bx[i] : A.by[i];
      trans = on = 1;
    } else if constexpr (Kn::MOBILE && c == 2) {
      w[2] = 1.0;
#pragma unroll
      for (int i = 0; i < 3; i++) o[i] = A.vt[i];
      on = 1;
    } else if constexpr (Kn::LIFT == 1 && c == 3) {
      w[2] = A.lift_sign;
      trans = 1;
      on = nc > 3;
    } else {
      constexpr int j = c - Kn::NB;
#pragma unroll
      for (int i = 0; i < 3; i++) {
        w[i] = A.zax[j][i];
        o[i] = A.org[j][i];
      }
      on = c >= first && c < nc;
    }
  });
  double om[3] = {0, 0, 0}, v[3];
  if (trans) {
    v[0] = w[0]; v[1] = w[1]; v[2] = w[2];
  } else {
    om[0] = w[0]; om[1] = w[1]; om[2] = w[2];
    const double rx = F.t[0] - o[0], ry = F.t[1] - o[1], rz = F.t[2] - o[2];
    v[0] = w[1] * rz - w[2] * ry;
    v[1] = w[2] * rx - w[0] * rz;
    v[2] = w[0] * ry - w[1] * rx;
  }
  col[0] = F.c0[0] * om[0] + F.c0[1] * om[1] + F.c0[2] * om[2];
  col[1] = F.c1[0] * om[0] + F.c1[1] * om[1] + F.c1[2] * om[2];
  col[2] = F.c2[0] * om[0] + F.c2[1] * om[1] + F.c2[2] * om[2];
  col[3] = F.c0[0] * v[0] + F.c0[1] * v[1] + F.c0[2] * v[2];
  col[4] = F.c1[0] * v[0] + F.c1[1] * v[1] + F.c1[2] * v[2];
  col[5] = F.c2[0] * v[0] + F.c2[1] * v[1] + F.c2[2] * v[2];
  if (!on)
#pragma unroll
    for (int i = 0; i < 6; i++) col[i] = 0.0;
}

__device__ __forceinline__ void frame_rt(const Frame& F, double (&Rm)[9], double (&t)[3]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    Rm[i * 3] = F.c0[i];
    Rm[i * 3 + 1] = F.c1[i];
    Rm[i * 3 + 2] = F.c2[i];
    t[i] = F.t[i];
  }
}

}  // namespace g2
