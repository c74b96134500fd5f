// scene_rule.h -- the integer rule of include/gpmp2mi.h "scene" for closed meshes, stated once for the kernels
// (scene_kernels.hip) and for a host compiler (tests/cpp/scene_shim.cpp): the fixed point of a vertex, the orientation
// of a triangle, the edge test with its ownership of points on an edge or a vertex, and the first flipped cell of a
// crossing.  Plain C++.  Vertices are within +-2^29, so differences have 31 bits and every product below is exact in
// 64-bit integers; the only floating point is the crossing abscissa, evaluated as the header writes it.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define G2_SCENE_HD __host__ __device__ inline
#else
#define G2_SCENE_HD inline
#endif

namespace g2 {

constexpr double SCENE_FIXED_ONE = 1024.0;        // fixed-point units per cell
constexpr double SCENE_FIXED_MAX = 536870912.0;   // 2^29: the whole-mesh guard on |g * 1024|

// q = rint(g * 1024), ties to even; false when g is not finite or |g * 1024| > 2^29 (q is then left alone)
G2_SCENE_HD bool scene_quantize(double g, int64_t* q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double s = g * SCENE_FIXED_ONE;
  if (!std::isfinite(g) || !(std::fabs(s) <= SCENE_FIXED_MAX)) return false;
  *q = (int64_t)std::rint(s);
  return true;
}

// floor(v / 1024) and ceil(v / 1024) of a signed fixed-point value
G2_SCENE_HD int64_t scene_floor_cell(int64_t v) { return (v >= 0 ? v : v - 1023) / 1024; }
G2_SCENE_HD int64_t scene_ceil_cell(int64_t v) { return -scene_floor_cell(-v); }

struct SceneTri {
  int64_t p[3][3];   // fixed-point vertices P0, P1, P2 as (x, y, z)
  int64_t a;         // twice the area of the projection on the y-z plane, > 0 after scene_orient
};

// step 5 of the rule: a of the projection; false for a = 0 (the triangle is skipped); a < 0 swaps P1 and P2
G2_SCENE_HD bool scene_orient(SceneTri& t) {
  int64_t a = (t.p[1][1] - t.p[0][1]) * (t.p[2][2] - t.p[0][2]) - (t.p[1][2] - t.p[0][2]) * (t.p[2][1] - t.p[0][1]);
  if (a == 0) return false;
  if (a < 0) {
    for (int c = 0; c < 3; c++) {
      const int64_t s = t.p[1][c];
      t.p[1][c] = t.p[2][c];
      t.p[2][c] = s;
    }
    a = -a;
  }
  t.a = a;
  return true;
}

// step 6: the edge function of (A, B) at the column (Y, Z), and whether the edge passes: a point exactly on the edge
// belongs to the triangle on one fixed side of it
G2_SCENE_HD int64_t scene_edge(const int64_t* A, const int64_t* B, int64_t Y, int64_t Z) {
  return (B[1] - A[1]) * (Z - A[2]) - (B[2] - A[2]) * (Y - A[1]);
}
G2_SCENE_HD bool scene_edge_passes(int64_t e, int64_t dy, int64_t dz) {
  return e > 0 || (e == 0 && (dy > 0 || (dy == 0 && dz > 0)));
}

// the column (Y, Z) crosses the oriented triangle: e[n] is the edge function opposite P_n, e0 + e1 + e2 = a
G2_SCENE_HD bool scene_column_crosses(const SceneTri& t, int64_t Y, int64_t Z, int64_t e[3]) {
  bool all = true;
  for (int n = 0; n < 3; n++) {
    const int64_t* A = t.p[(n + 1) % 3];
    const int64_t* B = t.p[(n + 2) % 3];
    e[n] = scene_edge(A, B, Y, Z);
    all = all && scene_edge_passes(e[n], B[1] - A[1], B[2] - A[2]);
  }
  return all;
}

// steps 7 and 8: first = ceil(x) of the crossing abscissa in cells, a double; the crossing flips the cells i >= first
G2_SCENE_HD double scene_first(const SceneTri& t, const int64_t e[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double X0 = (double)t.p[0][0] / SCENE_FIXED_ONE, X1 = (double)t.p[1][0] / SCENE_FIXED_ONE,
               X2 = (double)t.p[2][0] / SCENE_FIXED_ONE;
  const double x = (((double)e[0] * X0 + (double)e[1] * X1) + (double)e[2] * X2) / (double)t.a;
  return std::ceil(x);
}

}  // namespace g2
