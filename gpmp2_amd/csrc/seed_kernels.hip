// seed_kernels.hip -- seeding on the device (include/gpmp2mi.h "seeding"): standard normals from the counter function
// of rng.h, and samples delta = L^-T z whose z never exists in memory.
//
//   k_normal_fill          out[a_count][b_count][nblk][n] = normal(seed, stream, a_first + a, b_first + b, i, r).  Four
//                          threads per row (a, b, i): thread g computes the pairs {g, g + 4} and {g + 8, g + 12} of
//                          rng.h and stores the members below n, so the four threads of a row fill its n doubles and a
//                          wavefront a contiguous run of 16 rows.
//   k_sample_seeded<n, SHARED>   one wavefront per (tile of 16 sample columns, system).  The factor tiles V_i = R_i^-T
//                          and W_i are the ones k_posterior leaves in its factor scratch (512 doubles a block, V at +0,
//                          W at +TILE_DBL) after a factor-only launch (K = 0, no marginals); the back-substitution is
//                          the sample section of k_posterior on the matrix cores:
//                              Delta_N = V_N^T Z_N,   Delta_i = V_i^T (Z_i - W_i Delta_{i+1})
//                          with Z_i made in registers: lane (g, c) holds rows g, g + 4, g + 8, g + 12 of column c, which
//                          are exactly two pairs of rng.h.  A column's result depends on its own z and the factors
//                          alone, not on the tile it rides in.
//     SHARED = true        restarts: every column is a problem j = first + column and uses system 0's factors (the prior
//                          precision H_seed does not depend on the problem); z = normal(seed, stream, j, 0, i, r); the
//                          epilogue writes out = mean + scale Delta, mean a caller array or the straight line of
//                          trajutils.initArmTrajStraightLine computed here.
//     SHARED = false       a plan's posterior: per-system factors, z = normal(seed, stream, a_first + system,
//                          b_first + column, i, r); the epilogue writes Delta.
//   Columns past `count` and rows >= n write nothing.
#include "plan.h"
#include "rng.h"
#include "tiles.h"

namespace g2 {

__global__ __launch_bounds__(256) void k_normal_fill(NormalFillArgs a) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t row = t >> 2, rows = (size_t)a.a_count * a.b_count * a.nblk;
  const int g = (int)(t & 3);
  if (row >= rows || g >= a.n) return;
  const uint32_t i = (uint32_t)(row % a.nblk);
  const size_t ab = row / a.nblk;
  const uint32_t pa = (uint32_t)a.a_first + (uint32_t)(ab / a.b_count), pb = (uint32_t)a.b_first + (uint32_t)(ab % a.b_count);
  double* out = a.out + row * a.n;
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const int r = g + 8 * q;
    if (r >= a.n) break;
    double zc, zs;
    normal_pair(a.seed, a.stream, pa, pb, i, g + 4 * q, zc, zs);
    out[r] = zc;
    if (r + 4 < a.n) out[r + 4] = zs;
  }
}

// W^T of a tile through the matrix cores: tile_atb(W, I) (exact), as k_posterior does
__device__ __forceinline__ Tile seed_identity(int lane) {
  Tile T;
#pragma unroll
  for (int k = 0; k < 4; k++) T.r[k] = ((lane >> 4) + 4 * k == (lane & 15)) ? 1.0 : 0.0;
  return T;
}

// gpmp2::initArmTrajStraightLine(start, end, N) as trajutils.py evaluates it: the velocity rows hold (end - start) / N,
// a configuration row two rounded products and a rounded sum with r = i / N, the end points exact.  Contraction is
// switched off for these bodies: the compiler's default would fuse a product into the sum (the __dmul_rn / __dadd_rn
// intrinsics are plain operators to it and do not prevent that).
__device__ __forceinline__ double line_velocity(double sc, double ec, int N) {
#pragma clang fp contract(off)
  return (ec - sc) / (double)N;
}
__device__ __forceinline__ double line_conf(double sc, double ec, double r, int i, int N) {
#pragma clang fp contract(off)
  if (i == 0) return sc;
  if (i == N) return ec;
  const double pe = r * ec, ps = (1.0 - r) * sc;
  return pe + ps;
}

template <int n, bool SHARED>
__global__ __launch_bounds__(64) void k_sample_seeded(SeedSampleArgs a) {
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const int sys = SHARED ? 0 : blockIdx.y, nblk = a.nblk;
  const int s = blockIdx.x * 16 + c;          // column: sample of the system, or restart
  const bool live = s < a.count;
  const uint32_t pa = (uint32_t)a.a_first + (uint32_t)(SHARED ? s : sys);
  const uint32_t pb = SHARED ? 0u : (uint32_t)a.b_first + (uint32_t)s;
  const double* fac = a.fac + (size_t)sys * nblk * 512;
  const size_t row = ((size_t)sys * a.count + s) * nblk;   // out, mean [systems][count][nblk][n]
  const bool keep = SHARED && a.keep_first && pa == 0u;     // problem 0 stays on its mean
  const Tile I = seed_identity(lane);
  // no mean given: the straight line.  The end points of this lane's rows are read once, ahead of the chain; a velocity
  // row (rho >= D) keeps its constant in ls.
  const bool line = SHARED && !a.mean;
  double ls[4] = {0.0, 0.0, 0.0, 0.0}, le[4] = {0.0, 0.0, 0.0, 0.0};
  if (line && live) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int rho = g + 4 * k;
      if (rho >= n) continue;
      const size_t d = (size_t)s * a.D + (rho >= a.D ? rho - a.D : rho);
      ls[k] = a.start_conf[d];
      le[k] = a.end_conf[d];
      if (rho >= a.D) ls[k] = line_velocity(ls[k], le[k], nblk - 1);
    }
  }
  Tile Dn = tile_zero();
  for (int i = nblk - 1; i >= 0; i--) {
    const Tile V = tile_load(fac + (size_t)i * 512, lane);
    Tile Z = tile_zero();
    if (live && g < n) {
      double zc, zs;
      normal_pair(a.seed, a.stream, pa, pb, (uint32_t)i, g, zc, zs);
      Z.r[0] = zc;
      Z.r[1] = (g + 4 < n) ? zs : 0.0;
      if (n > 8 && g + 8 < n) {
        normal_pair(a.seed, a.stream, pa, pb, (uint32_t)i, g + 4, zc, zs);
        Z.r[2] = zc;
        Z.r[3] = (g + 12 < n) ? zs : 0.0;
      }
    }
    if (i + 1 < nblk) {
      const Tile W = tile_load(fac + (size_t)i * 512 + TILE_DBL, lane);
      const Tile Y = tile_atb(tile_atb(W, I), Dn);   // W_i Delta_{i+1}
#pragma unroll
      for (int k = 0; k < 4; k++) Z.r[k] -= Y.r[k];
    }
    Dn = tile_atb(V, Z);
    const double r = line ? (double)i / (double)(nblk - 1) : 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int rho = g + 4 * k;
      if (!live || rho >= n) continue;
      const size_t at = (row + i) * n + rho;
      if (SHARED) {
        const double m = !line ? a.mean[at] : rho >= a.D ? ls[k] : line_conf(ls[k], le[k], r, i, nblk - 1);
        a.out[at] = keep ? m : fma(a.scale, Dn.r[k], m);
      } else {
        a.out[at] = Dn.r[k];
      }
    }
  }
}

int launch_normal_fill(const NormalFillArgs& a, hipStream_t st) {
  const size_t threads = (size_t)a.a_count * a.b_count * a.nblk * 4;
  if (threads == 0) return GPMP2MI_OK;
  k_normal_fill<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_sample_seeded(int systems, int n, bool shared, const SeedSampleArgs& a, hipStream_t st) {
  const dim3 grid((a.count + 15) / 16, shared ? 1 : systems), block(64);
  switch (n) {
#define G2_SEED_CASE(NN)                                                     \
  case NN:                                                                   \
    if (shared) k_sample_seeded<NN, true><<<grid, block, 0, st>>>(a);        \
    else k_sample_seeded<NN, false><<<grid, block, 0, st>>>(a);              \
    break;
    G2_SEED_CASE(1) G2_SEED_CASE(2) G2_SEED_CASE(3) G2_SEED_CASE(4) G2_SEED_CASE(5) G2_SEED_CASE(6)
    G2_SEED_CASE(7) G2_SEED_CASE(8) G2_SEED_CASE(9) G2_SEED_CASE(10) G2_SEED_CASE(11) G2_SEED_CASE(12)
    G2_SEED_CASE(13) G2_SEED_CASE(14) G2_SEED_CASE(15)
#undef G2_SEED_CASE
    default:
      set_error("seeding: block size must be 1..15 (one 16 x 16 tile per block; dof <= 7 for a plan)");
      return GPMP2MI_ERR_UNSUPPORTED;
  }
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

}  // namespace g2
