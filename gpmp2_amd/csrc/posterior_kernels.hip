// posterior_kernels.hip -- the Gaussian posterior of a block-tridiagonal SPD system H (include/gpmp2mi.h "posterior"):
// the blocks of Sigma = H^-1 on the tridiagonal band, and samples delta = L^-T z (H = L L^T, so cov(delta) = Sigma).
//
//   k_posterior<n>  one wavefront per system, tiles in the MFMA accumulator layout of tiles.h.
//     forward   the elimination of chain_solve<n>: S_0 = H_00, S_i = R_i^T R_i, W_i = R_i^-T H_{i,i+1},
//               S_{i+1} = H_{i+1,i+1} - W_i^T W_i.  V_i = R_i^-T and W_i go to the factor scratch, 512 doubles a block.
//     marginals backward (Rauch-Tung-Striebel), with Gt_i = W_i^T V_i = (R_i^-1 W_i)^T:
//                 Sigma_NN       = V_N^T V_N
//                 Sigma_{i+1,i}  = -Sigma_{i+1,i+1} Gt_i                      (the block Soff stores)
//                 Sigma_ii       = V_i^T V_i - Sigma_{i+1,i}^T Gt_i           (a sum of two positive semi-definite terms)
//               Every product is tile_atb (A^T B on the matrix cores); Sigma_ii is made symmetric in registers from its
//               upper triangle (the transpose is tile_atb(Sigma, I), exact), so memory and the next block see one value.
//     samples   16 right-hand sides ride as the columns of one tile:  Delta_N = V_N^T Z_N,
//               Delta_i = V_i^T (Z_i - W_i Delta_{i+1}), with W_i^T = tile_atb(W_i, I).
// There is no right-hand side here: column RHSCOL of the factor tiles is zero (n <= 15), and in a sample tile it is
// sample 15 like any other column.  Rows and columns >= n of every tile are zero throughout.
#include "plan.h"
#include "tiles.h"

namespace g2 {

__device__ __forceinline__ Tile tile_identity(int lane) {
  Tile T;
#pragma unroll
  for (int k = 0; k < 4; k++) T.r[k] = ((lane >> 4) + 4 * k == (lane & 15)) ? 1.0 : 0.0;
  return T;
}

template <int n>
__global__ __launch_bounds__(64) void k_posterior(PosteriorArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const int nblk = a.nblk;
  const double* D_ = a.Hd + (size_t)b * nblk * n * n;
  const double* O_ = a.Ho + (size_t)b * (nblk - 1) * n * n;
  double* fac = a.fac + (size_t)b * nblk * 512;
  // ---- forward elimination
  Tile Wprev = tile_zero();
  bool ok = true;
  for (int i = 0; i < nblk; i++) {
    Tile S, W, V;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int rho = g + 4 * k;
      const bool in = rho < n && c < n;
      S.r[k] = in ? D_[((size_t)i * n + rho) * n + c] : 0.0;
      W.r[k] = (in && i + 1 < nblk) ? O_[((size_t)i * n + c) * n + rho] : 0.0;   // block (i, i+1) = (i+1, i)^T
      V.r[k] = (rho == c && c < n) ? 1.0 : 0.0;
    }
    if (i > 0) {
      const Tile T = tile_atb(Wprev, Wprev);   // zero outside n x n, as W is
#pragma unroll
      for (int k = 0; k < 4; k++) S.r[k] -= T.r[k];
    }
    ok = tile_eliminate<n>(S, W, V, lane) && ok;
    tile_store(fac + (size_t)i * 512, V, lane);
    tile_store(fac + (size_t)i * 512 + TILE_DBL, W, lane);
    Wprev = W;
  }
  if (lane == 0 && a.ok) a.ok[b] = ok ? 1 : 0;
  const Tile I = tile_identity(lane);
  // ---- marginals
  if (a.Sd || a.So) {
    double* Sd = a.Sd ? a.Sd + (size_t)b * nblk * n * n : nullptr;
    double* So = a.So ? a.So + (size_t)b * (nblk - 1) * n * n : nullptr;
    Tile Sn = tile_zero();   // Sigma_{i+1,i+1}
    for (int i = nblk - 1; i >= 0; i--) {
      const Tile V = tile_load(fac + (size_t)i * 512, lane);
      Tile Sg = tile_atb(V, V);
      if (i + 1 < nblk) {
        const Tile W = tile_load(fac + (size_t)i * 512 + TILE_DBL, lane);
        const Tile Gt = tile_atb(W, V);
        const Tile A = tile_atb(Sn, Gt);   // Sigma_{i+1,i+1} G_i^T = -Sigma_{i+1,i}  (Sn is symmetric)
        const Tile Q = tile_atb(A, Gt);    // G_i Sigma_{i+1,i+1} G_i^T
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int rho = g + 4 * k;
          Sg.r[k] += Q.r[k];
          if (So && rho < n && c < n) So[((size_t)i * n + rho) * n + c] = -A.r[k];
        }
      }
      const Tile St = tile_atb(Sg, I);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int rho = g + 4 * k;
        Sg.r[k] = (rho <= c) ? Sg.r[k] : St.r[k];
        if (Sd && rho < n && c < n) Sd[((size_t)i * n + rho) * n + c] = Sg.r[k];
      }
      Sn = Sg;
    }
  }
  // ---- samples: tile t carries samples 16 t .. 16 t + 15 in its columns
  const int K = a.K;
  for (int s0 = 0; s0 < K; s0 += 16) {
    const int s = s0 + c;
    const size_t row = ((size_t)b * K + s) * nblk;   // z, delta [B][K][nblk][n]
    Tile Dn = tile_zero();
    for (int i = nblk - 1; i >= 0; i--) {
      const Tile V = tile_load(fac + (size_t)i * 512, lane);
      Tile Z;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int rho = g + 4 * k;
        Z.r[k] = (s < K && rho < n) ? a.z[(row + i) * n + rho] : 0.0;
      }
      if (i + 1 < nblk) {
        const Tile W = tile_load(fac + (size_t)i * 512 + TILE_DBL, lane);
        const Tile Y = tile_atb(tile_atb(W, I), Dn);   // W_i Delta_{i+1}
#pragma unroll
        for (int k = 0; k < 4; k++) Z.r[k] -= Y.r[k];
      }
      Dn = tile_atb(V, Z);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int rho = g + 4 * k;
        if (s < K && rho < n) a.delta[(row + i) * n + rho] = Dn.r[k];
      }
    }
  }
}

int launch_posterior(int B, int n, const PosteriorArgs& a, hipStream_t st) {
  const dim3 grid(B), block(64);
  switch (n) {
#define G2_POST_CASE(NN) \
  case NN: k_posterior<NN><<<grid, block, 0, st>>>(a); break;
    G2_POST_CASE(1) G2_POST_CASE(2) G2_POST_CASE(3) G2_POST_CASE(4) G2_POST_CASE(5) G2_POST_CASE(6)
    G2_POST_CASE(7) G2_POST_CASE(8) G2_POST_CASE(9) G2_POST_CASE(10) G2_POST_CASE(11) G2_POST_CASE(12)
    G2_POST_CASE(13) G2_POST_CASE(14) G2_POST_CASE(15)
#undef G2_POST_CASE
    default:
      set_error("posterior: block size must be 1..15 (one 16 x 16 tile per block; dof <= 7 for a plan)");
      return GPMP2MI_ERR_UNSUPPORTED;
  }
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

}  // namespace g2
