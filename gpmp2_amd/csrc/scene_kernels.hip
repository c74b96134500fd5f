// scene_kernels.hip -- scene (include/gpmp2mi.h "scene"): boxes, spheres, cylinders and closed triangle meshes rasterised
// on the grid of a field handle.  A hit stores 0 and EDT_INF into its cell of the two seeded volumes (plain stores of
// one value, as k_map_mark), or 1 into a byte mask; the axis passes, the finish and the pack that follow are the existing
// ones.  No floating-point atomic anywhere; the integer atomics are the crossing bits (XOR commutes) and the counts.
//
//   k_scene_prims     up to SCENE_PRIM_BATCH primitives a launch (blockIdx.y), their records in the kernel arguments.
//                     Lanes run over the cells of the primitive's cell box; the header's test in double, no contraction.
//                     The count: shuffle per wavefront, LDS per workgroup, one integer atomic per workgroup.
//   k_scene_quantize  one lane per vertex: world, grid, fixed point (scene_rule.h); an out-of-range vertex ORs the mesh's
//                     flag, and the two kernels behind it leave without writing when it is set.
//   k_scene_cross     one wavefront per triangle and z-slab (blockIdx.y): lanes run over the columns (j, k) of the
//                     triangle's projected box clipped to the grid, the three 64-bit edge functions evaluated directly.
//                     A crossing column does ONE atomicXor of bit max(first, 0) of its row -- not a flip of the row's
//                     tail, which at 200 cells a row would be seven atomics for one.
//   k_scene_fill      one wavefront per row: lanes hold the words of the row, the prefix XOR inside a word by shifts, the
//                     carry across the words by a wavefront scan of the word parities (rows longer than 2048 cells carry
//                     on in a register).  Fused with the stores of the seeds / mask bytes (two words, 64 consecutive
//                     cells, per store instruction), with the count, and with clearing the bits for the next mesh.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "launch.h"
#include "scene_rule.h"

namespace g2 {

// sum over the workgroup's four wavefronts, then one atomic
__device__ __forceinline__ void scene_count(int count, int* dst) {
  for (int d = 32; d > 0; d >>= 1) count += __shfl_xor(count, d);
  __shared__ int part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int sum = part[0] + part[1] + part[2] + part[3];
    if (sum) atomicAdd(dst, sum);
  }
}

__device__ __forceinline__ void scene_store(int* wa, int* wb, unsigned char* mask, size_t cell) {
  if (mask) {
    mask[cell] = 1;
  } else {
    wa[cell] = 0;
    wb[cell] = EDT_INF;
  }
}

// the header's test of a cell centre c against primitive p, every operation rounded once
__device__ __forceinline__ bool scene_prim_hit(const ScenePrim& p, const double (&c)[3]) {
#pragma clang fp contract(off)
  const double d0 = c[0] - p.t[0], d1 = c[1] - p.t[1], d2 = c[2] - p.t[2];
  if (p.kind == SCENE_SPHERE) return sqrt((d0 * d0 + d1 * d1) + d2 * d2) <= p.s[0];
  double l[3];
  for (int m = 0; m < 3; m++) l[m] = (p.R[m] * d0 + p.R[3 + m] * d1) + p.R[6 + m] * d2;
  if (p.kind == SCENE_BOX) return fabs(l[0]) <= p.s[0] && fabs(l[1]) <= p.s[1] && fabs(l[2]) <= p.s[2];
  return sqrt(l[0] * l[0] + l[1] * l[1]) <= p.s[0] && fabs(l[2]) <= p.s[1];
}

__global__ void __launch_bounds__(256) k_scene_prims(ScenePrims a) {
#pragma clang fp contract(off)
  const ScenePrim& p = a.p[blockIdx.y];
  const SensorGrid& g = a.g;
  const size_t bx = (size_t)p.n[0], by = (size_t)p.n[1], total = bx * by * (size_t)p.n[2];
  int count = 0;
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < total; c += (size_t)gridDim.x * blockDim.x) {
    // lo + n <= grid size on every axis (the host clips the box), so the cell is inside the volumes
    const int i = p.lo[0] + (int)(c % bx), j = p.lo[1] + (int)((c / bx) % by), k = p.lo[2] + (int)(c / (bx * by));
    const double cc[3] = {g.ox + (double)i * g.cell, g.oy + (double)j * g.cell,
                          g.dim == 3 ? g.oz + (double)k * g.cell : 0.0};
    if (scene_prim_hit(p, cc)) {
      count++;
      scene_store(a.wa, a.wb, a.mask, ((size_t)k * g.ny + j) * g.nx + i);
    }
  }
  scene_count(count, &a.cells[p.obj]);
}

__global__ void __launch_bounds__(256) k_scene_quantize(SceneMesh m) {
#pragma clang fp contract(off)
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (v < m.V) {
    const double x0 = m.verts[3 * (size_t)v], x1 = m.verts[3 * (size_t)v + 1], x2 = m.verts[3 * (size_t)v + 2];
    const double o[3] = {m.g.ox, m.g.oy, m.g.dim == 3 ? m.g.oz : 0.0};
    for (int a = 0; a < 3; a++) {
      const double w = ((m.pose[4 * a] * x0 + m.pose[4 * a + 1] * x1) + m.pose[4 * a + 2] * x2) + m.pose[4 * a + 3];
      const double gc = (w - o[a]) / m.g.cell;
      int64_t q = 0;
      if (!scene_quantize(gc, &q)) bad = true;
      m.q[3 * (size_t)v + a] = (int)q;   // |q| <= 2^29
    }
  }
  if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(m.flag, 1);
}

__global__ void __launch_bounds__(256) k_scene_cross(SceneMesh m) {
  if (*m.flag) return;   // the whole mesh marks nothing
  const int tri = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (tri >= m.T) return;   // no barrier in this kernel
  SceneTri t;
  for (int n = 0; n < 3; n++) {
    const int v = m.tris[3 * (size_t)tri + n];   // 0 <= v < V: checked when the scene was made
    for (int c = 0; c < 3; c++) t.p[n][c] = m.q[3 * (size_t)v + c];
  }
  if (!scene_orient(t)) return;
  const int ny = m.g.ny, nz = m.g.nz;
  // the z-slab of this wavefront, and inside it the columns whose (Y, Z) can lie in the projected triangle
  const int slab = (nz + (int)gridDim.y - 1) / (int)gridDim.y;
  const int64_t ylo = min(t.p[0][1], min(t.p[1][1], t.p[2][1])), yhi = max(t.p[0][1], max(t.p[1][1], t.p[2][1]));
  const int64_t zlo = min(t.p[0][2], min(t.p[1][2], t.p[2][2])), zhi = max(t.p[0][2], max(t.p[1][2], t.p[2][2]));
  const int64_t j0 = max(scene_ceil_cell(ylo), (int64_t)0), j1 = min(scene_floor_cell(yhi), (int64_t)ny - 1);
  const int64_t k0 = max(scene_ceil_cell(zlo), (int64_t)blockIdx.y * slab);
  const int64_t k1 = min(scene_floor_cell(zhi), min((int64_t)(blockIdx.y + 1) * slab, (int64_t)nz) - 1);
  if (j0 > j1 || k0 > k1) return;
  const int64_t nj = j1 - j0 + 1, total = nj * (k1 - k0 + 1);
  for (int64_t c = lane; c < total; c += 64) {
    const int64_t j = j0 + c % nj, k = k0 + c / nj;   // 0 <= j < ny, 0 <= k < nz
    int64_t e[3];
    if (!scene_column_crosses(t, 1024 * j, 1024 * k, e)) continue;
    const double first = scene_first(t, e);
    if (!(first < (double)m.g.nx)) continue;          // nothing of the row is flipped
    const int f = first <= 0.0 ? 0 : (int)first;      // 0 <= f < nx: the word is inside the row
    atomicXor(&m.bits[((size_t)k * ny + (size_t)j) * m.W + (f >> 5)], 1u << (f & 31));
  }
}

__global__ void __launch_bounds__(256) k_scene_fill(SceneMesh m) {
  if (*m.flag) {   // uniform over the grid
    if (blockIdx.x == 0 && threadIdx.x == 0) m.cells[m.obj] = -1;
    return;
  }
  const int lane = threadIdx.x & 63, nx = m.g.nx, W = m.W;
  const size_t rows = (size_t)m.g.ny * m.g.nz;
  int count = 0;
  for (size_t row = blockIdx.x * (size_t)4 + (threadIdx.x >> 6); row < rows; row += (size_t)gridDim.x * 4) {
    unsigned* rb = m.bits + row * W;
    unsigned carry = 0;   // the parity that enters this chunk of 64 words; uniform over the wavefront
    for (int w0 = 0; w0 < W; w0 += 64) {
      const int wi = w0 + lane;
      const unsigned raw = wi < W ? rb[wi] : 0u;
      if (__ballot(raw != 0u) == 0ull && !carry) continue;   // nothing set up to here: the cells stay free
      if (raw) rb[wi] = 0u;                                  // all 0 again for the next mesh
      unsigned w = raw;
      w ^= w << 1;
      w ^= w << 2;
      w ^= w << 4;
      w ^= w << 8;
      w ^= w << 16;
      const unsigned par = w >> 31;   // the parity of the whole word
      unsigned inc = par;
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(inc, d);
        if (lane >= d) inc ^= up;
      }
      if ((inc ^ par ^ carry) & 1u) w = ~w;   // the parity of the words before this one
      carry ^= __shfl(inc, 63);
      if (wi >= W) w = 0u;
      else if (wi == W - 1 && (nx & 31)) w &= (1u << (nx & 31)) - 1u;   // bits past the end of the row
      count += __popc(w);
      for (int s = 0; s < 64 && w0 + s < W; s += 2) {
        const int src = s + (lane >> 5);
        const unsigned ww = __shfl(w, src);
        if ((ww >> (lane & 31)) & 1u)   // the bit is inside the row, so the cell is inside the volumes
          scene_store(m.wa, m.wb, m.mask, row * nx + (size_t)(w0 + src) * 32 + (lane & 31));
      }
    }
  }
  scene_count(count, &m.cells[m.obj]);
}

int launch_scene_prims(const ScenePrims& a, hipStream_t st) {
  if (a.count <= 0) return GPMP2MI_OK;
  size_t most = 1;
  for (int k = 0; k < a.count; k++) most = std::max(most, (size_t)a.p[k].n[0] * a.p[k].n[1] * a.p[k].n[2]);
  const unsigned blocks = (unsigned)std::min<size_t>((most + 255) / 256, 4096);
  k_scene_prims<<<dim3(blocks, (unsigned)a.count), dim3(256), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_scene_mesh(const SceneMesh& a, hipStream_t st) {
  k_scene_quantize<<<dim3((unsigned)((a.V + 255) / 256)), dim3(256), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  const unsigned slabs = (unsigned)std::min(8, std::max(1, (a.g.nz + 31) / 32));
  k_scene_cross<<<dim3((unsigned)((a.T + 3) / 4), slabs), dim3(256), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  const size_t rows = (size_t)a.g.ny * a.g.nz;
  k_scene_fill<<<dim3((unsigned)std::min<size_t>((rows + 3) / 4, 65536)), dim3(256), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

}  // namespace g2
