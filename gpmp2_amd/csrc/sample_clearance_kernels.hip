// sample_clearance_kernels.hip -- the sampled clearance of a trajectory (include/gpmp2mi.h "sampled clearance"): K joint
// draws of the configurations on the executed timeline per row, each put through the collision check of k_score, behind
// gpmp2mi_sampled_clearance_traj / gpmp2mi_plan_collision_probability / gpmp2mi_plan_sample_dense_seeded.
//
//   k_sampled_clearance  the tiling of k_score (score_kernels.hip): a lane is a checked state of a tile of SCORE_TILE
//                        consecutive states.  The parallelism is K, so a WAVEFRONT IS ONE SAMPLE: the wavefronts of a
//                        workgroup take different samples of the same (row, tile) and loop over a block of
//                        SAMPLED_PER_WG samples.  They share through LDS the staged RobotDev, the estimate's support
//                        states of the tile, Lp and C; a lane's interpolation scalars depend on its state alone and
//                        stay in its registers over the sample loop.  Per sample a lane
//                          1. reads its two delta blocks from the chunk workspace and forms zeta = est + delta,
//                          2. interpolates with the expression of k_score,
//                          3. forms eta_m = C xi_m for its own state into the wavefront's LDS rows (min(D, 4) Philox
//                             blocks, each normal made once per wavefront; a halo of at most J - 1 states covers the
//                             interval that starts before the tile),
//                          4. after a wavefront-local wait sums  sum_j' Lp[j][j'] eta  over its interval,
//                          5. walks the spheres value-only with the range test of k_score and keeps its state's minimum,
//                          6. adds 1 to the LDS counter of its state when that minimum is below required_clearance.
//                        The lane minima go through the butterfly to ONE 32-byte record per (row, sample, tile); the
//                        workgroup issues one integer atomic per state for state_hits and writes the optional maps
//                        (state_clearance, conf) directly.
//   k_sampled_finish     one row per workgroup: the records of a sample in tile order give c_s and worst, an integer
//                        reduction over the samples gives hits and oor_samples; chunk after chunk on one stream the
//                        counts are carried in two words per row, and the last chunk writes them, the probability and
//                        the outputs of a row with ok == 0.
//
// Determinism: a (row, sample)'s numbers are a function of the row's estimate and delta, the robot, the field, Delta, J,
// bridge, the seed and the global indices alone: no sum crosses samples except the integer counts, and no floating-point
// atomic is used.  SAMPLED_PER_WG and the number of wavefronts only decide which wavefront computes a sample.
#include <climits>

#include "device_math.h"
#include "dispatch.h"
#include "launch.h"
#include "rng.h"

namespace g2 {

namespace {

// (clearance, state, sphere) compared as the ScoreKey of k_score: exact ties go to the lowest state, then sphere
struct SampledKey {
  double c;
  int k, s;
};
__device__ __forceinline__ bool sampled_less(const SampledKey& a, const SampledKey& b) {
  return a.c < b.c || (a.c == b.c && (a.k < b.k || (a.k == b.k && a.s < b.s)));
}

// what a lane wrote to LDS is read by the other lanes of its own wavefront only
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int SAMPLED_WAVES = 4;                                      // wavefronts of a workgroup
constexpr int SAMPLED_ETA = SCORE_TILE + SAMPLED_MAX_INTER - 1;       // the tile's states and the halo in front of them

}  // namespace

template <int KIND, int AD, int AD2, int SDIM>
__global__ __launch_bounds__(64 * SAMPLED_WAVES) void k_sampled_clearance(const RobotDev* __restrict__ Rg, SdfDev sdf,
                                                                          SampledArgs a) {
  using K = Kin<KIND, AD, AD2>;
  static_assert(!K::MOBILE, "k_sampled_clearance: vector-space kinds only");
  constexpr int D = K::DOF, n = 2 * D, NP = D < 4 ? D : 4;   // NP: the pairs of rng.h that hold coordinates 0 .. D - 1
  static_assert(D <= 8, "k_sampled_clearance: the pairing below covers coordinates 0 .. 7");
  __shared__ RobotDev R;
  __shared__ double est[(SCORE_TILE + 1) * n];   // the support states the tile touches, from state seg0 on
  __shared__ double lp[SAMPLED_MAX_INTER * (SAMPLED_MAX_INTER + 1) / 2];   // row j, column j' at (j - 1) j / 2 + j' - 1
  __shared__ double cf[D * D];
  __shared__ double eta[SAMPLED_WAVES][SAMPLED_ETA][D];
  __shared__ int hit_cnt[SCORE_TILE];
  stage_robot(&R, Rg);
  const int N = a.N, Md = a.Md, J1 = a.inter + 1;
  const int b = blockIdx.x / a.nblk, blk = blockIdx.x % a.nblk;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = blk * SCORE_TILE, m = m0 + lane;   // checked state of this lane
  const int seg0 = m0 / J1;
  const bool bridge = a.bridge && a.inter > 0;
  {
    const int mlast = min(m0 + SCORE_TILE - 1, Md - 1);
    const int nst = min(mlast / J1 + 1, N) - seg0 + 1;   // <= SCORE_TILE + 1
    const double* src = a.est + ((size_t)b * (N + 1) + seg0) * n;
    for (int e = threadIdx.x; e < nst * n; e += blockDim.x) est[e] = src[e];
    if (bridge) {
      for (int e = threadIdx.x; e < a.inter * J1 / 2; e += blockDim.x) lp[e] = a.Lp[e];
      for (int e = threadIdx.x; e < D * D; e += blockDim.x) cf[e] = a.C[e];
    }
    if (threadIdx.x < SCORE_TILE) hit_cnt[threadIdx.x] = 0;
  }
  __syncthreads();
  const bool bad = a.ok && a.ok[b] == 0;   // a row that is not SPD: its samples are unspecified
  const bool have = m < Md;
  const int seg = m / J1, j = m % J1;
  GpCoef gc{};
  if (have && j > 0) gc = gp_coef_dev(a.dt, (double)j * (a.dt / (double)J1));
  // the halo: sub-steps 1 .. j0 - 1 of the interval the tile starts in, j0 the sub-step of the tile's first state
  const int j0 = m0 % J1, halo = (bridge && j0 > 1) ? j0 - 1 : 0;
  const uint32_t pr = (uint32_t)a.row_first + (uint32_t)b;
  const int send = min((int)(blockIdx.y + 1) * SAMPLED_PER_WG, a.cnt);
  for (int sl = blockIdx.y * SAMPLED_PER_WG + wave; sl < send; sl += SAMPLED_WAVES) {
    const uint32_t pq = (uint32_t)a.sample_first + (uint32_t)(a.s0 + sl);
    const size_t srow = (size_t)b * a.K + a.s0 + sl;   // this sample's row of the outputs
    if (bridge) {
      for (int e = lane; e < SCORE_TILE + halo; e += 64) {
        const int mm = m0 - halo + e;
        if (mm >= Md || mm % J1 == 0) continue;
        double xi[D];
#pragma unroll
        for (int p = 0; p < NP; p++) {
          double zc, zs;
          normal_pair(a.seed, GPMP2MI_RNG_BRIDGE, pr, pq, (uint32_t)mm, p, zc, zs);
          xi[p] = zc;
          if (p + 4 < D) xi[p + 4] = zs;
        }
#pragma unroll
        for (int d = 0; d < D; d++) {
          double s = 0.0;
#pragma unroll
          for (int k = 0; k <= d; k++) s += cf[d * D + k] * xi[k];
          eta[wave][e][d] = s;
        }
      }
      wave_sync();
    }
    int oor = 0;
    SampledKey best{HUGE_VAL, INT_MAX, INT_MAX};
    if (have) {
      const double* e0 = est + (seg - seg0) * n;
      const double* d0 = a.delta + (((size_t)b * a.cnt + sl) * (N + 1) + seg) * n;
      double q[D];
      if (j == 0) {
#pragma unroll
        for (int k = 0; k < D; k++) q[k] = e0[k] + d0[k];
      } else {
        // zeta is rounded, then interpolated: the expression of k_score on the four rounded sums
#pragma unroll
        for (int k = 0; k < D; k++) {
          const double z0 = e0[k] + d0[k], w0 = e0[D + k] + d0[D + k];
          const double z1 = e0[n + k] + d0[n + k], w1 = e0[n + D + k] + d0[n + D + k];
          q[k] = gc.l11 * z0 + gc.l12 * w0 + gc.p11 * z1 + gc.p12 * w1;
        }
        if (bridge) {
          double eps[D];
#pragma unroll
          for (int k = 0; k < D; k++) eps[k] = 0.0;
          const double* lrow = lp + (j - 1) * j / 2;
          const int e1 = lane + halo - j;   // eta row of sub-step j' at e1 + j'
          for (int jp = 1; jp <= j; jp++) {
            const double l = lrow[jp - 1];
#pragma unroll
            for (int k = 0; k < D; k++) eps[k] += l * eta[wave][e1 + jp][k];
          }
#pragma unroll
          for (int k = 0; k < D; k++) q[k] += eps[k];
        }
      }
      if (a.conf) {
        double* o = a.conf + (srow * Md + m) * D;
#pragma unroll
        for (int k = 0; k < D; k++) o[k] = bad ? NAN : q[k];
      }
      typename K::Axes A;   // filled by the walk, never read here: the Jacobian work is dead code
      K::walk(R, q, A, [&](int s, const double (&p)[3], auto) {
        // negated conjunction: a NaN centre fails every comparison and counts as out of range
        bool in = p[0] >= sdf.ox && p[0] <= sdf.hix && p[1] >= sdf.oy && p[1] <= sdf.hiy;
        if (SDIM == 3) in = in && p[2] >= sdf.oz && p[2] <= sdf.hiz;
        if (!in) {
          oor++;
          return;
        }
        double d, gx, gy, gz;
        if (SDIM == 3) (void)sdf3_lookup(sdf, p[0], p[1], p[2], d, gx, gy, gz);
        else (void)sdf2_lookup(sdf, p[0], p[1], d, gx, gy);
        const SampledKey key{d - R.sph_r[s], m, R.sph_orig[s]};
        if (sampled_less(key, best)) best = key;
      });
      if (a.state_clearance) a.state_clearance[srow * Md + m] = bad ? NAN : best.c;
      if (!bad && best.c < a.required) atomicAdd(&hit_cnt[lane], 1);
    }
    // wavefront butterfly: the partners compare the same two keys, so all 64 lanes end with the same one
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      oor += __shfl_xor(oor, off);
      const SampledKey o{__shfl_xor(best.c, off), __shfl_xor(best.k, off), __shfl_xor(best.s, off)};
      if (sampled_less(o, best)) best = o;
    }
    if (lane == 0) a.recs[((size_t)b * a.cnt + sl) * a.nblk + blk] = SampledRec{best.c, best.k, best.s, oor > 0 ? 1 : 0, 0, 0, 0};
    // the next sample's eta rows are written behind this sample's reads: LDS operations of a wavefront stay in order
    if (bridge) wave_sync();
  }
  __syncthreads();
  if (a.state_hits && threadIdx.x < SCORE_TILE && m0 + (int)threadIdx.x < Md && hit_cnt[threadIdx.x] > 0)
    atomicAdd(a.state_hits + (size_t)b * Md + m0 + threadIdx.x, hit_cnt[threadIdx.x]);
}

// One row per workgroup.  A thread takes samples (thread id + multiple of the thread count) of the chunk, a sample's
// records in tile order; the counts of the chunk are reduced through LDS and added to the row's two carried words.
__global__ __launch_bounds__(256) void k_sampled_finish(SampledFinish a) {
  __shared__ int s_hit[256], s_oor[256];
  const int b = blockIdx.x;
  const bool bad = a.ok && a.ok[b] == 0;
  int hit = 0, oors = 0;
  for (int sl = threadIdx.x; sl < a.cnt; sl += blockDim.x) {
    const SampledRec* r = a.recs + ((size_t)b * a.cnt + sl) * a.nblk;
    SampledKey t{r[0].c, r[0].k, r[0].s};
    int oor = r[0].oor;
    for (int i = 1; i < a.nblk; i++) {   // records in tile order
      oor |= r[i].oor;
      const SampledKey x{r[i].c, r[i].k, r[i].s};
      if (sampled_less(x, t)) t = x;
    }
    const bool none = bad || t.k == INT_MAX;
    const size_t srow = (size_t)b * a.K + a.s0 + sl;
    if (a.clearance) a.clearance[srow] = bad ? NAN : t.c;
    if (a.worst) {
      a.worst[2 * srow] = none ? -1 : t.k;
      a.worst[2 * srow + 1] = none ? -1 : t.s;
    }
    hit += t.c < a.required;
    oors += oor != 0;
  }
  s_hit[threadIdx.x] = hit;
  s_oor[threadIdx.x] = oors;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) {
      s_hit[threadIdx.x] += s_hit[threadIdx.x + h];
      s_oor[threadIdx.x] += s_oor[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int th = (a.first ? 0 : a.acc[2 * b]) + s_hit[0], to = (a.first ? 0 : a.acc[2 * b + 1]) + s_oor[0];
    a.acc[2 * b] = th;
    a.acc[2 * b + 1] = to;
    if (a.last) {
      if (a.hits) a.hits[b] = bad ? -1 : th;
      if (a.probability) a.probability[b] = bad ? NAN : (double)th / (double)a.K;
      if (a.oor_samples) a.oor_samples[b] = bad ? -1 : to;
    }
  }
  if (a.last && bad && a.state_hits)
    for (int e = threadIdx.x; e < a.Md; e += blockDim.x) a.state_hits[(size_t)b * a.Md + e] = -1;
}

// the vector-space kinds of dispatch.h with blocks of one tile (the posterior's limit): the arm up to 7 joints, the point
#define G2_SAMPLED_CASE(K, A, SD)                                                           \
  if (!done && h.kind == (K) && h.arm_dof == (A) && s.dim == (SD)) {                        \
    k_sampled_clearance<K, A, 0, SD><<<grid, block, 0, st>>>(R, s, a);                      \
    done = true;                                                                            \
  }

int launch_sampled_clearance(const RobotDev& h, const RobotDev* R, const SdfDev& s, const SampledArgs& a, hipStream_t st) {
  const long long groups = (a.cnt + SAMPLED_PER_WG - 1) / SAMPLED_PER_WG;
  if ((long long)a.nblk * a.B >= (1ll << 31) || groups > 65535) {
    set_error("too many checked states or samples for one launch");
    return GPMP2MI_ERR_INVALID;
  }
  const dim3 grid((unsigned)(a.nblk * a.B), (unsigned)groups), block(64 * SAMPLED_WAVES);
  bool done = false;
  G2_SAMPLED_CASE(GPMP2MI_ROBOT_ARM, 1, 2) G2_SAMPLED_CASE(GPMP2MI_ROBOT_ARM, 1, 3)
  G2_SAMPLED_CASE(GPMP2MI_ROBOT_ARM, 2, 2) G2_SAMPLED_CASE(GPMP2MI_ROBOT_ARM, 2, 3)
  G2_SAMPLED_CASE(GPMP2MI_ROBOT_ARM, 3, 2) G2_SAMPLED_CASE(GPMP2MI_ROBOT_ARM, 3, 3)
  G2_SAMPLED_CASE(GPMP2MI_ROBOT_ARM, 4, 2) G2_SAMPLED_CASE(GPMP2MI_ROBOT_ARM, 4, 3)
  G2_SAMPLED_CASE(GPMP2MI_ROBOT_ARM, 5, 2) G2_SAMPLED_CASE(GPMP2MI_ROBOT_ARM, 5, 3)
  G2_SAMPLED_CASE(GPMP2MI_ROBOT_ARM, 6, 2) G2_SAMPLED_CASE(GPMP2MI_ROBOT_ARM, 6, 3)
  G2_SAMPLED_CASE(GPMP2MI_ROBOT_ARM, 7, 2) G2_SAMPLED_CASE(GPMP2MI_ROBOT_ARM, 7, 3)
  G2_SAMPLED_CASE(GPMP2MI_ROBOT_POINT, 0, 2) G2_SAMPLED_CASE(GPMP2MI_ROBOT_POINT, 0, 3)
  if (!done) {
    set_error("sampled clearance: robot kind / dof combination is not instantiated");
    return GPMP2MI_ERR_UNSUPPORTED;
  }
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_sampled_finish(const SampledFinish& a, hipStream_t st) {
  k_sampled_finish<<<dim3((unsigned)a.B), dim3(256), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

}  // namespace g2
