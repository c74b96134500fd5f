// sensor_kernels.hip -- sensor map (include/gpmp2mi.h "sensor map"): an int16 evidence value per cell of a field handle,
// raised where the rays of a frame end and lowered where they pass; the field is rebuilt from the cells whose evidence
// reaches a threshold by the seeds written here and the axis passes, the finish and the pack the constructors run.
//
//   k_sensor_rays    one lane per ray: the end point (a pixel deprojected, or a given point), its cell coordinates and
//                    its class -- hit / invalid / max_range / self / outside -- by the header's rules in their order.
//                    [M][3] cell coordinates and [M] classes go to the handle's ray records.  The five counts as
//                    k_map_mark: ballot + popcount per wavefront, LDS per workgroup, one integer atomic per class.
//   k_sensor_walk    one lane per ray: the voxel walk of the header from the sensor's cell to the end cell, one cell per
//                    step, the axis chosen by the smallest (first + j) * inv recomputed from the integer j.  Every cell
//                    but the last stores 1 into the byte volume of the miss marks, the last cell of a hit ray stores 1
//                    into the byte volume of the hit marks: plain stores of one value, so the marks depend on the set of
//                    rays alone.  Lanes of a wavefront walk rays of different lengths; the loop body is short and
//                    branch-free up to the store, and a lane whose ray has left the grid for good returns.
//   k_sensor_apply   four cells a lane: E' = clamp(E + (hit ? +hit : miss ? -miss : 0), lo, hi), the marks cleared where
//                    they were set, the cells with E' >= occupied_at counted (shuffle per wavefront, LDS per workgroup,
//                    one integer atomic per workgroup) and, when the field is to be rebuilt, the two int32 volumes
//                    seeded from E' united with the base mask in the same pass.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "launch.h"

namespace g2 {

enum { SENSOR_HIT = 0, SENSOR_INVALID = 1, SENSOR_MAX_RANGE = 2, SENSOR_SELF = 3, SENSOR_OUTSIDE = 4 };
constexpr double SENSOR_MAX_SPAN = 1048576.0;

// u = (p - origin) / cell + 0.5 per axis, a true division; the unused axis of a planar grid sits in the middle of cell 0
__device__ __forceinline__ void sensor_cell_coordinate(const SensorGrid& g, const double (&p)[3], double (&u)[3]) {
#pragma clang fp contract(off)
  u[0] = (p[0] - g.ox) / g.cell + 0.5;
  u[1] = (p[1] - g.oy) / g.cell + 0.5;
  u[2] = g.dim == 3 ? (p[2] - g.oz) / g.cell + 0.5 : 0.5;
}

// |b - a| >= 2^20 on some axis; a difference that is not a number counts as such
__device__ __forceinline__ bool sensor_span_too_long(const double (&a)[3], const double (&b)[3]) {
#pragma clang fp contract(off)
  bool bad = false;
  for (int k = 0; k < 3; k++) bad = bad || !(fabs(b[k] - a[k]) < SENSOR_MAX_SPAN);
  return bad;
}

// p_i = ((P[i][0] xc + P[i][1] yc) + P[i][2] z) + P[i][3] with xc = ((u - cx) / fx) z, yc = ((v - cy) / fy) z
__device__ __forceinline__ void sensor_deproject(const SensorRays& r, int u, int v, double z, double (&p)[3]) {
#pragma clang fp contract(off)
  const double xc = (((double)u - r.cx) / r.fx) * z, yc = (((double)v - r.cy) / r.fy) * z;
  for (int i = 0; i < 3; i++)
    p[i] = ((r.pose[4 * i] * xc + r.pose[4 * i + 1] * yc) + r.pose[4 * i + 2] * z) + r.pose[4 * i + 3];
}

__global__ void __launch_bounds__(256) k_sensor_rays(SensorRays r) {
#pragma clang fp contract(off)
  __shared__ double cs[MAXS * 3];   // sphere centres, the caller's order
  __shared__ double rs[MAXS];       // radius + margin, the same order
  const int S = r.R ? r.S : 0;      // uniform over the grid
  if (S > 0) {
    for (int s = threadIdx.x; s < S; s += blockDim.x) rs[r.R->sph_orig[s]] = r.R->sph_r[s] + r.margin;
    for (int e = threadIdx.x; e < 3 * S; e += blockDim.x) cs[e] = r.cen[e];
    __syncthreads();
  }
  const SensorGrid& g = r.g;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  int cls = -1;
  if (i < (size_t)r.M) {
    const double o[3] = {r.o[0], r.o[1], r.o[2]};
    double p[3] = {0.0, 0.0, 0.0}, a[3], b[3] = {0.5, 0.5, 0.5};
    sensor_cell_coordinate(g, o, a);
    double z = 0.0;
    int u = 0, v = 0;
    cls = SENSOR_HIT;
    if (r.depth) {
      u = (int)(i % (size_t)r.width);
      v = (int)(i / (size_t)r.width);
      z = (double)r.depth[i];
      if (!isfinite(z) || z <= 0.0 || z < r.depth_min) cls = SENSOR_INVALID;
      else sensor_deproject(r, u, v, z, p);
    } else {
      for (int k = 0; k < g.dim; k++) {
        p[k] = r.pts[i * g.dim + k];
        if (!isfinite(p[k])) cls = SENSOR_INVALID;
      }
    }
    if (cls != SENSOR_INVALID) {
      sensor_cell_coordinate(g, p, b);
      if (sensor_span_too_long(a, b)) cls = SENSOR_INVALID;
    }
    if (cls != SENSOR_INVALID && r.depth && z > r.depth_max) {   // the ray carves up to depth_max and marks no end
      sensor_deproject(r, u, v, r.depth_max, p);
      sensor_cell_coordinate(g, p, b);
      cls = sensor_span_too_long(a, b) ? SENSOR_INVALID : SENSOR_MAX_RANGE;
    }
    if (cls == SENSOR_HIT) {
      for (int s = 0; s < S; s++) {   // the rule of map_classify, on the same centres
        const double dx = p[0] - cs[3 * s], dy = p[1] - cs[3 * s + 1];
        double d2 = dx * dx + dy * dy;
        if (g.dim == 3) {
          const double dz = p[2] - cs[3 * s + 2];
          d2 = d2 + dz * dz;
        }
        if (sqrt(d2) <= rs[s]) cls = SENSOR_SELF;
      }
    }
    if (cls == SENSOR_HIT) {
      const bool in = b[0] >= 0.0 && b[0] < (double)g.nx && b[1] >= 0.0 && b[1] < (double)g.ny &&
                      (g.dim == 2 || (b[2] >= 0.0 && b[2] < (double)g.nz));
      if (!in) cls = SENSOR_OUTSIDE;
    }
    r.rb[3 * i] = b[0];
    r.rb[3 * i + 1] = b[1];
    r.rb[3 * i + 2] = b[2];
    r.rcls[i] = cls;
  }
  __shared__ int part[4][5];        // [wavefront][class]
  for (int c = 0; c < 5; c++) {
    const unsigned long long vote = __ballot(cls == c);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][c] = __popcll(vote);
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    const int sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (sum) atomicAdd(&r.cnt[threadIdx.x], sum);
  }
}

// One ray per lane.  No barrier in this kernel: a lane returns when its ray is done or cannot reach the grid any more.
__global__ void __launch_bounds__(256) k_sensor_walk(SensorWalk w) {
#pragma clang fp contract(off)
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= (size_t)w.M) return;
  const int cls = w.rcls[i];
  if (cls == SENSOR_INVALID) return;
  const SensorGrid& g = w.g;
  const double o[3] = {w.o[0], w.o[1], w.o[2]};
  double a[3];
  sensor_cell_coordinate(g, o, a);
  const double b[3] = {w.rb[3 * i], w.rb[3 * i + 1], w.rb[3 * i + 2]};
  const int n[3] = {g.nx, g.ny, g.nz};
  int c[3], left[3], step[3];
  double first[3], inv[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {   // unrolled: every index below is a constant
    const double ck = floor(a[k]), ek = floor(b[k]);
    // an axis on which neither end of the walk, nor anything between them, is in the grid: no cell is ever marked.
    // What passes has |c| < 2^20 + n + 2, so the integers below hold it.
    if (fmax(ck, ek) < 0.0 || fmin(ck, ek) >= (double)n[k]) return;
    c[k] = (int)ck;
    left[k] = (int)fabs(ek - ck);
    step[k] = ek > ck ? 1 : (ek < ck ? -1 : 0);
    inv[k] = left[k] > 0 ? 1.0 / fabs(b[k] - a[k]) : 0.0;
    first[k] = step[k] > 0 ? (ck + 1.0) - a[k] : a[k] - ck;
  }
  int jx = 0, jy = 0, jz = 0;
  const int total = left[0] + left[1] + left[2];
  for (int s = 0; s < total; s++) {
    const bool in = (unsigned)c[0] < (unsigned)n[0] && (unsigned)c[1] < (unsigned)n[1] && (unsigned)c[2] < (unsigned)n[2];
    const bool ax = jx < left[0], ay = jy < left[1], az = jz < left[2];
    if (in) {
      w.miss[((size_t)c[2] * n[1] + c[1]) * n[0] + c[0]] = 1;
    } else {
      // beyond the grid on an axis whose remaining motion is away from it or none: the ray does not come back
      const bool gone = (c[0] < 0 && (step[0] < 0 || !ax)) || (c[0] >= n[0] && (step[0] > 0 || !ax)) ||
                        (c[1] < 0 && (step[1] < 0 || !ay)) || (c[1] >= n[1] && (step[1] > 0 || !ay)) ||
                        (c[2] < 0 && (step[2] < 0 || !az)) || (c[2] >= n[2] && (step[2] > 0 || !az));
      if (gone) return;
    }
    const double tx = (first[0] + (double)jx) * inv[0], ty = (first[1] + (double)jy) * inv[1],
                 tz = (first[2] + (double)jz) * inv[2];
    // the smallest t among the axes with steps left; ties to x, then y, then z
    const bool px = ax && (!ay || tx <= ty) && (!az || tx <= tz);
    const bool py = !px && ay && (!az || ty <= tz);
    const bool pz = !px && !py;
    c[0] += px ? step[0] : 0;
    c[1] += py ? step[1] : 0;
    c[2] += pz ? step[2] : 0;
    jx += px;
    jy += py;
    jz += pz;
  }
  // c == floor(b) now.  A hit ray's end point is in the grid by its class; the comparison keeps the store in bounds
  // whatever the records hold.
  if (cls == SENSOR_HIT && (unsigned)c[0] < (unsigned)n[0] && (unsigned)c[1] < (unsigned)n[1] &&
      (unsigned)c[2] < (unsigned)n[2])
    w.hit[((size_t)c[2] * n[1] + c[1]) * n[0] + c[0]] = 1;
}

__device__ __forceinline__ int sensor_apply_cell(const SensorApply& p, int e, unsigned miss, unsigned hit) {
  e += hit ? p.hit : (miss ? -p.miss : 0);
  return min(max(e, p.lo), p.hi);
}

// E, the two mark volumes, the mask and the two int32 volumes start at workspace boundaries (256 B): the four-cell
// accesses are aligned
__global__ void __launch_bounds__(256) k_sensor_apply(SensorApply p) {
  const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = p.n / 4;
  int occupied = 0;
  for (size_t i = tid; i < n4; i += stride) {
    const unsigned mm = reinterpret_cast<const unsigned*>(p.miss_marks)[i];
    const unsigned hm = reinterpret_cast<const unsigned*>(p.hit_marks)[i];
    const uint2 ev = reinterpret_cast<const uint2*>(p.E)[i];
    const unsigned bm = p.mask ? reinterpret_cast<const unsigned*>(p.mask)[i] : 0u;
    int e[4] = {(short)(ev.x & 0xffffu), (short)(ev.x >> 16), (short)(ev.y & 0xffffu), (short)(ev.y >> 16)};
    bool obst[4];
    for (int k = 0; k < 4; k++) {
      e[k] = sensor_apply_cell(p, e[k], (mm >> (8 * k)) & 0xffu, (hm >> (8 * k)) & 0xffu);
      const bool occ = e[k] >= p.occupied_at;
      occupied += occ;
      obst[k] = occ || ((bm >> (8 * k)) & 0xffu);
    }
    uint2 out;
    out.x = ((unsigned)e[0] & 0xffffu) | ((unsigned)e[1] << 16);
    out.y = ((unsigned)e[2] & 0xffffu) | ((unsigned)e[3] << 16);
    if (out.x != ev.x || out.y != ev.y) reinterpret_cast<uint2*>(p.E)[i] = out;   // most cells of a frame are untouched
    if (mm) reinterpret_cast<unsigned*>(p.miss_marks)[i] = 0u;
    if (hm) reinterpret_cast<unsigned*>(p.hit_marks)[i] = 0u;
    if (p.wa) {
      reinterpret_cast<int4*>(p.wa)[i] = make_int4(obst[0] ? 0 : EDT_INF, obst[1] ? 0 : EDT_INF, obst[2] ? 0 : EDT_INF,
                                                    obst[3] ? 0 : EDT_INF);
      reinterpret_cast<int4*>(p.wb)[i] = make_int4(obst[0] ? EDT_INF : 0, obst[1] ? EDT_INF : 0, obst[2] ? EDT_INF : 0,
                                                    obst[3] ? EDT_INF : 0);
    }
  }
  for (size_t i = n4 * 4 + tid; i < p.n; i += stride) {   // the last n % 4 cells
    const unsigned mm = p.miss_marks[i], hm = p.hit_marks[i];
    const int e = sensor_apply_cell(p, p.E[i], mm, hm);
    p.E[i] = (short)e;
    if (mm) p.miss_marks[i] = 0;
    if (hm) p.hit_marks[i] = 0;
    const bool occ = e >= p.occupied_at;
    occupied += occ;
    const bool obst = occ || (p.mask && p.mask[i]);
    if (p.wa) {
      p.wa[i] = obst ? 0 : EDT_INF;
      p.wb[i] = obst ? EDT_INF : 0;
    }
  }
  for (int d = 32; d > 0; d >>= 1) occupied += __shfl_xor(occupied, d);
  __shared__ int part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = occupied;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int sum = part[0] + part[1] + part[2] + part[3];
    if (sum) atomicAdd(p.cnt, sum);
  }
}

int launch_sensor_rays(const SensorRays& a, hipStream_t st) {
  if (a.M <= 0) return GPMP2MI_OK;
  k_sensor_rays<<<dim3((unsigned)(((size_t)a.M + 255) / 256)), dim3(256), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_sensor_walk(const SensorWalk& a, hipStream_t st) {
  if (a.M <= 0) return GPMP2MI_OK;
  k_sensor_walk<<<dim3((unsigned)(((size_t)a.M + 255) / 256)), dim3(256), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_sensor_apply(const SensorApply& a, hipStream_t st) {
  const size_t lanes = (a.n + 3) / 4;
  k_sensor_apply<<<dim3((unsigned)std::max<size_t>(1, std::min<size_t>((lanes + 255) / 256, 256 * 16))), dim3(256), 0,
                   st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

}  // namespace g2
