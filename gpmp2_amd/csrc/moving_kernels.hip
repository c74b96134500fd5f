// moving_kernels.hip -- moving obstacles (include/gpmp2mi.h "moving obstacles"): K spheres whose centres are indexed by
// the support time, against every body sphere of the robot.
//
//   k_moving_factor      the factor on M evaluations (gpmp2mi_moving_sphere_factor): one lane per (evaluation, sphere,
//                        moving sphere), rows to err / H.
//   k_moving_accumulate  the factor inside a plan.  One wavefront per (trajectory, support state of the range).  The
//                        S K pairs, formed from the centres / Jacobians k_sphere_centers left (PlanExtras::cen, Jc), go
//                        through accumulate_sphere_rows (record_entries.h): chunks of 64, the active rows [h | r | w]
//                        through LDS into the record entries a lane owns (RecAcc).  The S K x D rows never reach memory.
//   k_moving_clearance   the check of the executed trajectory, tiled as k_self_clearance is (self_tile, checked_grid): a
//                        lane is a checked state (checked_config, score_select.h); phase 1 leaves the sphere centres of
//                        the tile in LDS (caller's sphere order), phase 2 deals the S K pairs to the wavefronts (and
//                        slots); ONE record per workgroup (block_score_record).
//   k_moving_finish      reduces a row's records in index order to the five outputs and, when asked, applies the
//                        selection rule over the per-row scores of the existing stages.
//
// Determinism: a pair that is not active adds an exact zero, so skipping it changes no bit; the active rows of a state
// are added in pair order, one accumulator per record entry, without atomics: the contribution of a state is a function
// of (S, K, D) and its own data.  The check sums in an order fixed by (N, inter_step, S, K), as k_self_clearance does.
#include <climits>

#include "device_math.h"
#include "dispatch.h"
#include "launch.h"
#include "plan.h"
#include "record_entries.h"
#include "score_select.h"

namespace g2 {

__global__ __launch_bounds__(64) void k_moving_factor(int S, int D, int K, int M, const double* __restrict__ rr,
                                                       const double* __restrict__ radius, double eps,
                                                       const double* __restrict__ centers, const double* __restrict__ cen,
                                                       const double* __restrict__ Jc, double* __restrict__ err,
                                                       double* __restrict__ H) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)M * S * K) return;
  const int k = (int)(t % K), s = (int)((t / K) % S);
  const size_t m = (size_t)(t / ((long long)K * S));
  const double* c = cen + (m * S + s) * 3;
  const double* o = centers + (m * K + k) * 3;
  const SphereHinge hg = sphere_hinge(c[0] - o[0], c[1] - o[1], c[2] - o[2], (rr[s] + radius[k]) + eps);
  err[t] = hg.err;
  if (!H) return;
  const double* J = Jc + (m * S + s) * 3 * D;
  for (int d = 0; d < D; d++) H[(size_t)t * D + d] = -(hg.n[0] * J[d] + hg.n[1] * J[D + d] + hg.n[2] * J[2 * D + d]);
}

constexpr int MV_LD = MAXD + 2;   // an LDS row: h [D], r, w

namespace {

// pair p of a support state for accumulate_sphere_rows: body sphere p / K against moving sphere p % K at that state's time
struct MovingPairs {
  const PlanExtras& ex;
  const double *cen, *Jc;   // of the state
  int N, D, K, i;
  struct Pair {
    int s;
    double w;
  };
  __device__ __forceinline__ SphereHinge hinge(int p, Pair& pr) const {
    const int s = p / K, k = p - s * K;
    pr.s = s;
    pr.w = ex.mv_w;
    const double* o = ex.mv_centers + ((size_t)k * (N + 1) + i) * 3;
    return sphere_hinge(cen[s * 3] - o[0], cen[s * 3 + 1] - o[1], cen[s * 3 + 2] - o[2],
                        (ex.radius[s] + ex.mv_radius[k]) + ex.mv_eps);
  }
  __device__ __forceinline__ void row(const Pair& pr, const SphereHinge& hg, double* h) const {
    const double* J = Jc + (size_t)pr.s * 3 * D;
    for (int d = 0; d < D; d++) h[d] = -(hg.n[0] * J[d] + hg.n[1] * J[D + d] + hg.n[2] * J[2 * D + d]);
  }
};

}  // namespace

__global__ __launch_bounds__(64) void k_moving_accumulate(const PlanParams* __restrict__ pp, PlanBuffers pb, PlanExtras ex,
                                                           int S, int bufsel, const int* __restrict__ active) {
  __shared__ double rows[64][MV_LD];
  const PlanParams& P = *pp;
  const int N = P.N, D = P.D, K = ex.mv_K;
  const int nst = ex.mv_last - ex.mv_first + 1;
  const int b = blockIdx.x / nst, i = ex.mv_first + blockIdx.x % nst;
  if (active && !active[b]) return;
  const size_t m = (size_t)b * (N + 1) + i;
  RecAcc acc(D, P.NG);
  const MovingPairs pairs{ex, ex.cen + m * S * 3, ex.Jc + m * S * 3 * D, N, D, K, i};
  if (accumulate_sphere_rows(rows, D, S * K, pairs, acc)) acc.store(pb, b, i, bufsel, P);
}

template <int KIND, int AD, int AD2>
__global__ __launch_bounds__(256) void k_moving_clearance(const RobotDev* __restrict__ Rg, int K,
                                                          const double* __restrict__ radius,
                                                          const double* __restrict__ centers, double eps, int tile,
                                                          double dt, int inter, int N, int Md, int nblk,
                                                          const double* __restrict__ traj, ScoreRec* __restrict__ recs) {
  using Kn = Kin<KIND, AD, AD2>;
  constexpr int D = Kn::DOF;
  extern __shared__ __attribute__((aligned(16))) double ctr[];   // [3][S][tile], caller's sphere order
  __shared__ RobotDev R;
  __shared__ double rad[MAXS];
  stage_robot(&R, Rg);
  const int S = R.nr_spheres, P = S * K;
  for (int s = threadIdx.x; s < S; s += blockDim.x) rad[R.sph_orig[s]] = R.sph_r[s];
  const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6, nsub = blockDim.x >> 6;
  // a tile narrower than the wavefront: `slots` lanes share a state and split its spheres, then its pairs
  const int slots = 64 / tile, slot = lane / tile, tl = lane % tile;
  const int m = blk * tile + tl;   // checked state of this lane
  const bool live = m < Md;
  const int seg = m / (inter + 1), j = m % (inter + 1);
  if (live && P > 0) {
    const double* s0 = traj + ((size_t)b * (N + 1) + seg) * 2 * D;
    double q[D];
    checked_config<Kn>(s0, dt, inter, j, q);
    typename Kn::Axes A;   // filled by the walk, never read here: the Jacobian work is dead code
    Kn::walk(R, q, A, [&](int s, const double (&p)[3], auto) {
      const int so = R.sph_orig[s];
#pragma unroll
      for (int i = 0; i < 3; i++) ctr[(i * S + so) * tile + tl] = p[i];
    }, sub * slots + slot, nsub * slots);
  }
  __syncthreads();
  double dense = 0.0;
  int inv = 0;
  ScoreKey best{HUGE_VAL, INT_MAX, INT_MAX};
  if (live) {
    const double tau = (double)j / (double)(inter + 1);
    for (int p = sub * slots + slot; p < P; p += nsub * slots) {
      const int s = p / K, k = p - s * K;
      const double* o = centers + ((size_t)k * (N + 1) + seg) * 3;   // j > 0 only below the last support state
      double ox = o[0], oy = o[1], oz = o[2];
      if (j > 0) {
        ox = o[0] + tau * (o[3] - o[0]);
        oy = o[1] + tau * (o[4] - o[1]);
        oz = o[2] + tau * (o[5] - o[2]);
      }
      const double dx = ctr[s * tile + tl] - ox, dy = ctr[(S + s) * tile + tl] - oy, dz = ctr[(2 * S + s) * tile + tl] - oz;
      const double dist = sqrt(dx * dx + dy * dy + dz * dz);
      if (!isfinite(dist)) {   // invalid: counted, adds nothing
        inv++;
        continue;
      }
      const double te = (rad[s] + radius[k]) + eps;
      dense += dist > te ? 0.0 : te - dist;
      const ScoreKey key{dist - te, m, p};
      if (key_less(key, best)) best = key;
    }
  }
  block_score_record((live && j == 0) ? dense : 0.0, dense, inv, best, recs);
}

// Second stage: rows are taken by thread (RowPick, score_select.h).  With a.sel.select the grid is one workgroup
// and the rule reads, besides this stage's own results, the per-row scores k_score_finish and k_self_finish left.
__global__ __launch_bounds__(256) void k_moving_finish(MovingFinish a) {
  const ScoreFinish& f = a.sel;
  RowPick mine;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < f.B; b += gridDim.x * blockDim.x) {
    const ScoreRec t = reduce_records(a.recs + (size_t)b * a.nblk, a.nblk);
    const bool none = t.k == INT_MAX;
    if (a.support) a.support[b] = t.support;
    if (a.dense) a.dense[b] = t.dense;
    if (a.min_clearance) a.min_clearance[b] = t.clearance;
    if (a.worst) {
      a.worst[3 * b] = none ? -1 : t.k;
      a.worst[3 * b + 1] = none ? -1 : t.s / a.K;
      a.worst[3 * b + 2] = none ? -1 : t.s % a.K;
    }
    if (a.invalid) a.invalid[b] = t.oor;
    if (!f.select) continue;
    const double fe = f.ferr[b];
    bool ok = row_eligible(f, b, fe, a.clearance[b], a.oor[b]);
    if (a.self_clearance) ok = ok && a.self_invalid[b] == 0 && a.self_clearance[b] >= a.required_self_clearance;
    ok = ok && t.oor == 0 && t.clearance >= a.required_moving_clearance;
    if (ok) mine.take(fe, b);
  }
  if (!f.select) return;
  select_finish(f, mine);
}

int launch_moving_factor(int S, int D, int K, int M, const double* robot_radius, const double* radius, double eps,
                         const double* centers, const double* cen, const double* Jc, double* err, double* H,
                         hipStream_t st) {
  const long long T = (long long)M * S * K;
  if ((T + 63) / 64 >= (1ll << 31)) {
    set_error("too many (evaluation, sphere, moving sphere) rows for one launch");
    return GPMP2MI_ERR_INVALID;
  }
  if (T == 0) return GPMP2MI_OK;
  k_moving_factor<<<dim3((unsigned)((T + 63) / 64)), dim3(64), 0, st>>>(S, D, K, M, robot_radius, radius, eps, centers, cen,
                                                                       Jc, err, H);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_moving_accumulate(const PlanParams& hp, const PlanBuffers& pb, const PlanExtras& ex, int S, int bufsel,
                             const int* active, hipStream_t st) {
  if (ex.mv_K <= 0 || S <= 0) return GPMP2MI_OK;   // an empty set launches nothing
  if (ex.mv_K > ex.mv_cap || hp.D > MAXD || hp.NG + hp.D + 1 > 192) {
    set_error("k_moving_accumulate: set larger than the capacity, or a record wider than 192 entries");
    return GPMP2MI_ERR_INVALID;
  }
  const int nst = ex.mv_last - ex.mv_first + 1;
  k_moving_accumulate<<<dim3((unsigned)(hp.B * nst)), dim3(64), 0, st>>>(pb.params, pb, ex, S, bufsel, active);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_moving_clearance(const RobotDev& h, const RobotDev* R, int K, const double* radius, const double* centers,
                            double eps, double dt, int inter, int B, int N, const double* traj, ScoreRec* recs,
                            hipStream_t st) {
  const int S = h.nr_spheres, tile = self_tile(S);
  int Md, nblk;
  if (const int rc = checked_grid(N, inter, tile, B, S * K, Md, nblk)) return rc;
  const size_t lds = (size_t)3 * std::max(S, 1) * tile * sizeof(double);   // <= 48 KB by self_tile
  const dim3 grid((unsigned)(nblk * B)), block(64 * score_waves(S));
  G2_DISPATCH_ROBOT_H(h, (k_moving_clearance<KIND_, AD_, AD2_><<<grid, block, lds, st>>>(
                             R, K, radius, centers, eps, tile, dt, inter, N, Md, nblk, traj, recs)));
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_moving_finish(const MovingFinish& a, hipStream_t st) {
  return launch_finish(k_moving_finish, a, a.sel.select, a.sel.B, st);
}

}  // namespace g2
