// moving_kernels.hip -- moving obstacles (include/gpmp2mi.h "moving obstacles"): K spheres whose centres are indexed by
// the support time, against every body sphere of the robot.
//
//   k_moving_factor      the factor on M evaluations (gpmp2mi_moving_sphere_factor): one lane per (evaluation, sphere,
//                        moving sphere), rows to err / H.
//   k_moving_accumulate  the factor inside a plan.  One wavefront per (trajectory, support state of the range).  The
//                        S K pairs are taken in chunks of 64, one pair per lane, from the centres / Jacobians
//                        k_sphere_centers left (PlanExtras::cen, Jc).  A chunk without an active pair (ballot) is
//                        skipped; an active one leaves its rows [h | r] in LDS, and every lane adds the active rows, in
//                        ascending pair order, to the record entries it owns (entry e = lane, lane + 64, lane + 128 of
//                        the D (D + 1) / 2 + D + 1 <= 190 packed entries G | g | e).  The S K x D rows never reach memory.
//   k_moving_clearance   the check of the executed trajectory, by the tiling of k_self_clearance: a lane is a checked
//                        state; phase 1 leaves the sphere centres of the tile in LDS (caller's sphere order), phase 2
//                        deals the S K pairs to the wavefronts (and slots); ONE record per workgroup.
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
#include "score_select.h"

namespace g2 {

namespace {

// SelfCollision.h:114-127 with one sphere outside the robot: (dx, dy, dz) = c_s - o_k.  active: the hinge is on (a NaN
// distance keeps it on, as k_self_collision does); n: the direction, zero when dist == 0 (no NaN is made)
struct MovingHinge {
  double err, n[3];
  bool active;
};
__device__ __forceinline__ MovingHinge moving_hinge(double dx, double dy, double dz, double total_eps) {
  MovingHinge o;
  const double dist = sqrt(dx * dx + dy * dy + dz * dz);
  o.active = !(dist > total_eps);
  o.err = o.active ? total_eps - dist : 0.0;
  const bool dir = o.active && dist != 0.0;
  o.n[0] = dir ? dx / dist : 0.0;
  o.n[1] = dir ? dy / dist : 0.0;
  o.n[2] = dir ? dz / dist : 0.0;
  return o;
}

}  // namespace

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
  const MovingHinge hg = moving_hinge(c[0] - o[0], c[1] - o[1], c[2] - o[2], (rr[s] + radius[k]) + eps);
  err[t] = hg.err;
  if (!H) return;
  const double* J = Jc + (m * S + s) * 3 * D;
  for (int d = 0; d < D; d++) H[(size_t)t * D + d] = -(hg.n[0] * J[d] + hg.n[1] * J[D + d] + hg.n[2] * J[2 * D + d]);
}

constexpr int MV_LD = MAXD + 2;   // an LDS row: h [D], then r

__global__ __launch_bounds__(64) void k_moving_accumulate(const PlanParams* __restrict__ pp, PlanBuffers pb, PlanExtras ex,
                                                           int S, int bufsel, const int* __restrict__ active) {
  __shared__ double rows[64][MV_LD];
  const PlanParams& P = *pp;
  const int N = P.N, D = P.D, K = ex.mv_K;
  const int nst = ex.mv_last - ex.mv_first + 1;
  const int b = blockIdx.x / nst, i = ex.mv_first + blockIdx.x % nst;
  if (active && !active[b]) return;
  const int lane = threadIdx.x;
  const size_t m = (size_t)b * (N + 1) + i;
  const double* cen = ex.cen + m * S * 3;
  const double* Jc = ex.Jc + m * S * 3 * D;
  // the record entries of this lane as products rows[.][ea] * rows[.][eb]: G (k, k2) packed upper, g_k = h_k r, e = r r
  const int NE = P.NG + D + 1;
  int ea[3], eb[3];
  double acc[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const int e = lane + 64 * j;
    int k = 0, rem = e;
    while (k < D && rem >= D - k) {
      rem -= D - k;
      k++;
    }
    ea[j] = e < P.NG ? k : e < P.NG + D ? e - P.NG : D;
    eb[j] = e < P.NG ? k + rem : D;
    if (e >= NE) ea[j] = eb[j] = 0;   // not an entry: reads stay inside the row, nothing is stored
    acc[j] = 0.0;
  }
  const int SK = S * K;
  bool any = false;
  for (int c0 = 0; c0 < SK; c0 += 64) {
    const int p = c0 + lane;
    MovingHinge hg;
    hg.active = false;
    int s = 0;
    if (p < SK) {
      s = p / K;
      const int k = p - s * K;
      const double* o = ex.mv_centers + ((size_t)k * (N + 1) + i) * 3;
      hg = moving_hinge(cen[s * 3] - o[0], cen[s * 3 + 1] - o[1], cen[s * 3 + 2] - o[2],
                        (ex.radius[s] + ex.mv_radius[k]) + ex.mv_eps);
    }
    const unsigned long long mask = __ballot(hg.active);
    if (mask == 0) continue;   // wavefront-uniform
    any = true;
    if (hg.active) {
      const double* J = Jc + (size_t)s * 3 * D;
      for (int d = 0; d < D; d++) rows[lane][d] = -(hg.n[0] * J[d] + hg.n[1] * J[D + d] + hg.n[2] * J[2 * D + d]);
      rows[lane][D] = hg.err;
    }
    __syncthreads();
    for (unsigned long long mm = mask; mm; mm &= mm - 1) {   // active rows in ascending pair order
      const int l = __ffsll((long long)mm) - 1;
#pragma unroll
      for (int j = 0; j < 3; j++) acc[j] += ex.mv_w * rows[l][ea[j]] * rows[l][eb[j]];
    }
    __syncthreads();
  }
  if (!any) return;
  double* rec = rec_of(pb, pb.which[b], bufsel) + ((size_t)b * P.Ppad + (size_t)i * (P.I + 1)) * P.RECS;
#pragma unroll
  for (int j = 0; j < 3; j++)
    if (lane + 64 * j < NE) rec[lane + 64 * j] += acc[j];
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
  __shared__ double w_sup[4], w_den[4], w_clr[4];
  __shared__ int w_k[4], w_p[4], w_inv[4];
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
    if (j == 0) {
#pragma unroll
      for (int k = 0; k < D; k++) q[k] = s0[k];
    } else {   // the arithmetic of k_score / k_self_clearance
      const double* s1 = s0 + 2 * D;
      const GpCoef gc = gp_coef_dev(dt, (double)j * (dt / (double)(inter + 1)));
      if constexpr (Kn::MOBILE) {
        double x0[3], w0[3], x1[3], w1[3], qp[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { x0[k] = s0[k]; w0[k] = s0[D + k]; x1[k] = s1[k]; w1[k] = s1[D + k]; }
        lie_interpolate<3>(gc, x0, w0, x1, w1, qp, nullptr);
#pragma unroll
        for (int k = 0; k < 3; k++) q[k] = qp[k];
#pragma unroll
        for (int k = 3; k < D; k++) q[k] = s0[k] + (gc.l12 * s0[D + k] + gc.p11 * (s1[k] - s0[k]) + gc.p12 * s1[D + k]);
      } else {
#pragma unroll
        for (int k = 0; k < D; k++) q[k] = gc.l11 * s0[k] + gc.l12 * s0[D + k] + gc.p11 * s1[k] + gc.p12 * s1[D + k];
      }
    }
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
  double sup = (live && j == 0) ? dense : 0.0;
  // wavefront: butterfly (both partners add the same two numbers, so all 64 lanes end with the same bits)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    sup += __shfl_xor(sup, off);
    dense += __shfl_xor(dense, off);
    inv += __shfl_xor(inv, off);
    const ScoreKey o{__shfl_xor(best.c, off), __shfl_xor(best.k, off), __shfl_xor(best.s, off)};
    if (key_less(o, best)) best = o;
  }
  if (lane == 0) {
    w_sup[sub] = sup; w_den[sub] = dense; w_clr[sub] = best.c;
    w_k[sub] = best.k; w_p[sub] = best.s; w_inv[sub] = inv;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ScoreRec r{w_sup[0], w_den[0], w_clr[0], w_k[0], w_p[0], w_inv[0], 0};
    for (int w = 1; w < nsub; w++) {   // wavefronts in index order
      r.support += w_sup[w];
      r.dense += w_den[w];
      r.oor += w_inv[w];
      const ScoreKey a{w_clr[w], w_k[w], w_p[w]}, c{r.clearance, r.k, r.s};
      if (key_less(a, c)) { r.clearance = a.c; r.k = a.k; r.s = a.s; }
    }
    recs[blockIdx.x] = r;
  }
}

// Second stage, by the pattern of k_motion_finish: rows are taken by thread.  With a.sel.select the grid is one workgroup
// and the rule reads, besides this stage's own results, the per-row scores k_score_finish and k_self_finish left.
__global__ __launch_bounds__(256) void k_moving_finish(MovingFinish a) {
  const ScoreFinish& f = a.sel;
  double my_err = HUGE_VAL;
  int my_row = INT_MAX, my_cnt = 0;
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
    bool ok = score_eligible(!f.status || f.status[b] != GPMP2MI_TRAJ_NOT_SPD, fe, a.clearance[b], f.required_clearance,
                             f.require_in_range, a.oor[b]);
    if (a.self_clearance) ok = ok && a.self_invalid[b] == 0 && a.self_clearance[b] >= a.required_self_clearance;
    ok = ok && t.oor == 0 && t.clearance >= a.required_moving_clearance;
    if (!ok) continue;
    my_cnt++;
    if (fe < my_err) {   // rows ascend within a thread: a tie keeps the lower row
      my_err = fe;
      my_row = b;
    }
  }
  if (!f.select) return;
  select_finish(f, my_err, my_row, my_cnt);
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
  const long long Md = (long long)N * (inter + 1) + 1;
  const long long nblk = (Md + tile - 1) / tile;
  if (Md >= (1ll << 31) / GPMP2MI_MAX_DOF || nblk * B >= (1ll << 31) || Md * std::max(S * K, 1) >= (1ll << 31)) {
    set_error("too many checked states for one launch");
    return GPMP2MI_ERR_INVALID;
  }
  // wavefronts that share the spheres and the pairs of a tile: a function of the sphere count alone
  const int nsub = S >= 8 ? 4 : 1;
  const size_t lds = (size_t)3 * std::max(S, 1) * tile * sizeof(double);   // <= 48 KB by self_tile
  const dim3 grid((unsigned)(nblk * B)), block(64 * nsub);
  G2_DISPATCH_ROBOT_H(h, (k_moving_clearance<KIND_, AD_, AD2_><<<grid, block, lds, st>>>(
                             R, K, radius, centers, eps, tile, dt, inter, N, (int)Md, (int)nblk, traj, recs)));
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_moving_finish(const MovingFinish& a, hipStream_t st) {
  const int grid = a.sel.select ? 1 : (a.sel.B + 255) / 256;
  k_moving_finish<<<dim3(grid), dim3(256), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

}  // namespace g2
