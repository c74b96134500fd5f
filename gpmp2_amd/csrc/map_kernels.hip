// map_kernels.hip -- live map (include/gpmp2mi.h "live map"): the seeds that take the place of k_edt_seed when a field
// handle is updated in place from an occupancy grid or a point cloud.  The axis passes, the finish and the pack that
// follow are the existing kernels (sdf_kernels.hip, factor_kernels.hip), so the field is what the constructor from the
// same obstacle set gives, bit for bit.
//
//   k_map_seed_occ   k_edt_seed's rule (occ > 0.75) into the two int32 volumes, and the obstacle set as one byte per
//                    cell: the handle's base.  8 B read, 9 B written per cell.
//   k_map_seed       the two volumes from that byte mask, or all free: 1 B read, 8 B written per cell, four cells a
//                    lane.  The point path never holds an fp64 occupancy volume.
//   k_map_mark       one lane per point: non-finite / inside a body sphere / outside the grid / kept.  The sphere centres
//                    are the output of k_sphere_centers for the one configuration, staged in LDS with radius + margin
//                    beside them.  A kept point stores 0 and EDT_INF into its cell of the two volumes: plain stores,
//                    every racing lane stores the same two values, so the volumes depend on the set of points alone.
//                    The four counts: ballot + popcount per wavefront, summed per workgroup in LDS, one integer atomic
//                    per workgroup and class.  (One atomic per wavefront was measured first: 4 800 wavefronts adding to
//                    the same four words took 0.15 ms of a 1.8 ms update at 307 200 points.)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "launch.h"

namespace g2 {

__global__ void k_map_seed_occ(size_t n, const double* __restrict__ occ, int* __restrict__ a, int* __restrict__ b,
                               unsigned char* __restrict__ mask) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const bool obst = occ[i] > 0.75;   // the rule of k_edt_seed
    a[i] = obst ? 0 : EDT_INF;
    b[i] = obst ? EDT_INF : 0;
    mask[i] = obst ? 1 : 0;
  }
}

// a, b and mask start at hipMalloc / workspace boundaries (256 B), so the four-cell accesses are aligned
__global__ void k_map_seed(size_t n, const unsigned char* __restrict__ mask, int* __restrict__ a, int* __restrict__ b) {
  const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = n / 4;
  for (size_t i = tid; i < n4; i += stride) {
    const unsigned m = mask ? reinterpret_cast<const unsigned*>(mask)[i] : 0u;
    const bool o0 = m & 0xffu, o1 = m & 0xff00u, o2 = m & 0xff0000u, o3 = m & 0xff000000u;
    reinterpret_cast<int4*>(a)[i] = make_int4(o0 ? 0 : EDT_INF, o1 ? 0 : EDT_INF, o2 ? 0 : EDT_INF, o3 ? 0 : EDT_INF);
    reinterpret_cast<int4*>(b)[i] = make_int4(o0 ? EDT_INF : 0, o1 ? EDT_INF : 0, o2 ? EDT_INF : 0, o3 ? EDT_INF : 0);
  }
  for (size_t i = n4 * 4 + tid; i < n; i += stride) {   // the last n % 4 cells
    const bool obst = mask && mask[i];
    a[i] = obst ? 0 : EDT_INF;
    b[i] = obst ? EDT_INF : 0;
  }
}

enum { MAP_KEPT = 0, MAP_NONFINITE = 1, MAP_SELF = 2, MAP_OUTSIDE = 3 };

// The class of point p and, for a kept point, its cell.  Every expression is evaluated as written (no fused
// multiply-add), so the verdicts are those of the same expressions in IEEE double anywhere else.
__device__ __forceinline__ int map_classify(const MapMark& m, const double (&p)[3], const double* cs, const double* rs,
                                            int S, size_t* cell) {
#pragma clang fp contract(off)
  for (int a = 0; a < m.dim; a++)
    if (!isfinite(p[a])) return MAP_NONFINITE;
  for (int s = 0; s < S; s++) {
    const double dx = p[0] - cs[3 * s], dy = p[1] - cs[3 * s + 1];
    double d2 = dx * dx + dy * dy;
    if (m.dim == 3) {
      const double dz = p[2] - cs[3 * s + 2];
      d2 = d2 + dz * dz;
    }
    if (sqrt(d2) <= rs[s]) return MAP_SELF;
  }
  // u = (p - origin) / cell + 0.5: a true division; in the grid iff 0 <= u < n, decided in double
  const double ux = (p[0] - m.ox) / m.cell + 0.5, uy = (p[1] - m.oy) / m.cell + 0.5;
  if (!(ux >= 0.0 && ux < (double)m.nx && uy >= 0.0 && uy < (double)m.ny)) return MAP_OUTSIDE;
  size_t iz = 0;
  if (m.dim == 3) {
    const double uz = (p[2] - m.oz) / m.cell + 0.5;
    if (!(uz >= 0.0 && uz < (double)m.nz)) return MAP_OUTSIDE;
    iz = (size_t)floor(uz);
  }
  *cell = (iz * m.ny + (size_t)floor(uy)) * m.nx + (size_t)floor(ux);
  return MAP_KEPT;
}

__global__ void __launch_bounds__(256) k_map_mark(MapMark m) {
  __shared__ double cs[MAXS * 3];   // sphere centres, the caller's order
  __shared__ double rs[MAXS];       // radius + margin, the same order
  const int S = m.R ? m.S : 0;      // uniform over the grid
  if (S > 0) {
    for (int s = threadIdx.x; s < S; s += blockDim.x) rs[m.R->sph_orig[s]] = m.R->sph_r[s] + m.margin;
    for (int e = threadIdx.x; e < 3 * S; e += blockDim.x) cs[e] = m.cen[e];
    __syncthreads();
  }
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  int cls = -1;
  if (i < (size_t)m.M) {
    double p[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < m.dim; a++) p[a] = m.pts[i * m.dim + a];
    size_t cell = 0;
    cls = map_classify(m, p, cs, rs, S, &cell);
    if (cls == MAP_KEPT) {   // cell < nx ny nz: each index is floor(u) with 0 <= u < n
      m.wa[cell] = 0;
      m.wb[cell] = EDT_INF;
    }
  }
  // the counts: ballot + popcount per wavefront, summed over the workgroup's four wavefronts in LDS, then one integer
  // atomic per class that occurs (all workgroups add to the same four words: fewer, larger adds)
  __shared__ int part[4][4];        // [wavefront][class]
  for (int c = 0; c < 4; c++) {
    const unsigned long long vote = __ballot(cls == c);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][c] = __popcll(vote);
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (sum) atomicAdd(&m.cnt[threadIdx.x], sum);
  }
}

static int map_sweep(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 256 * 16); }

int launch_map_seed_occ(size_t n, const double* occ, int* wa, int* wb, unsigned char* mask, hipStream_t st) {
  k_map_seed_occ<<<dim3(map_sweep(n)), dim3(256), 0, st>>>(n, occ, wa, wb, mask);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_map_seed(size_t n, const unsigned char* mask, int* wa, int* wb, hipStream_t st) {
  k_map_seed<<<dim3(map_sweep((n + 3) / 4)), dim3(256), 0, st>>>(n, mask, wa, wb);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_map_mark(const MapMark& a, hipStream_t st) {
  if (a.M <= 0) return GPMP2MI_OK;
  k_map_mark<<<dim3((unsigned)(((size_t)a.M + 255) / 256)), dim3(256), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

}  // namespace g2
