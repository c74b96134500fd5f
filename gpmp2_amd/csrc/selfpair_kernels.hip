// selfpair_kernels.hip -- the self-collision table of a plan (include/gpmp2mi.h "self-collision table in a plan"): P
// pairs of the robot's own spheres, each with its epsilon and sigma, as a factor on the support states of a range.
//
//   k_selfpair_accumulate  One wavefront per (trajectory, support state of the range), by the scheme of
//                          k_moving_accumulate.  The P pairs are taken in chunks of 64, one pair per lane, from the
//                          plan's records (PlanExtras::sp_rec) and the centres / Jacobians k_sphere_centers left
//                          (PlanExtras::cen, Jc).  A chunk without an active pair (ballot) is skipped; an active one
//                          leaves its rows [h | r | w] in LDS -- the Jacobian difference is formed by the active lanes
//                          only -- and every lane adds the active rows, in ascending table order, to the record entries
//                          it owns (entry e = lane, lane + 64, lane + 128 of the D (D + 1) / 2 + D + 1 <= 190 packed
//                          entries G | g | e).  The P x D rows never reach memory.
//
// LDS: a row is MAXD + 3 = 21 doubles, an odd number, so the lanes that fill their own rows hit distinct banks within
// each group of 16 lanes a 64-bit store is served in (42 dwords mod 32 banks); in the accumulation all lanes read the
// same row (<= 21 distinct words, the rest broadcast).
// Determinism: a pair that is not active adds an exact zero, so skipping it changes no bit; the active rows of a state
// are added in table order, one accumulator per record entry, without atomics: the contribution of a state is a
// function of (P, D), the table and its own data.
#include "device_math.h"
#include "launch.h"
#include "plan.h"

namespace g2 {

namespace {

// SelfCollision.h:114-127 on (dx, dy, dz) = c_A - c_B, with the dist == 0 rule of moving_hinge (moving_kernels.hip).
// active: the hinge is on (a NaN distance keeps it on); n: the direction, zero when dist == 0 (no NaN is made)
struct PairHinge {
  double err, n[3];
  bool active;
};
__device__ __forceinline__ PairHinge pair_hinge(double dx, double dy, double dz, double total_eps) {
  PairHinge o;
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

constexpr int SP_LD = MAXD + 3;   // an LDS row: h [D], r, w; odd, see above

__global__ __launch_bounds__(64) void k_selfpair_accumulate(const PlanParams* __restrict__ pp, PlanBuffers pb,
                                                             PlanExtras ex, int S, int bufsel,
                                                             const int* __restrict__ active) {
  __shared__ double rows[64][SP_LD];
  const PlanParams& P = *pp;
  const int N = P.N, D = P.D, NP = ex.sp_P;
  const int nst = ex.sp_last - ex.sp_first + 1;
  const int b = blockIdx.x / nst, i = ex.sp_first + blockIdx.x % nst;
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
  bool any = false;
  for (int c0 = 0; c0 < NP; c0 += 64) {
    const int p = c0 + lane;
    PairHinge hg;
    hg.active = false;
    int sa = 0, sb = 0;
    double w = 0.0;
    if (p < NP) {
      const SelfPairRec r = ex.sp_rec[p];
      sa = r.a;
      sb = r.b;
      w = r.w;
      hg = pair_hinge(cen[sa * 3] - cen[sb * 3], cen[sa * 3 + 1] - cen[sb * 3 + 1], cen[sa * 3 + 2] - cen[sb * 3 + 2],
                      r.total_eps);
    }
    const unsigned long long mask = __ballot(hg.active);
    if (mask == 0) continue;   // wavefront-uniform
    any = true;
    if (hg.active) {
      const double* Ja = Jc + (size_t)sa * 3 * D;
      const double* Jb = Jc + (size_t)sb * 3 * D;
      for (int d = 0; d < D; d++)
        rows[lane][d] = -(hg.n[0] * (Ja[d] - Jb[d]) + hg.n[1] * (Ja[D + d] - Jb[D + d]) + hg.n[2] * (Ja[2 * D + d] - Jb[2 * D + d]));
      rows[lane][D] = hg.err;
      rows[lane][D + 1] = w;
    }
    __syncthreads();
    for (unsigned long long mm = mask; mm; mm &= mm - 1) {   // active rows in ascending table order
      const int l = __ffsll((long long)mm) - 1;
      const double wl = rows[l][D + 1];
#pragma unroll
      for (int j = 0; j < 3; j++) acc[j] += wl * rows[l][ea[j]] * rows[l][eb[j]];
    }
    __syncthreads();
  }
  if (!any) return;
  double* rec = rec_of(pb, pb.which[b], bufsel) + ((size_t)b * P.Ppad + (size_t)i * (P.I + 1)) * P.RECS;
#pragma unroll
  for (int j = 0; j < 3; j++)
    if (lane + 64 * j < NE) rec[lane + 64 * j] += acc[j];
}

int launch_selfpair_accumulate(const PlanParams& hp, const PlanBuffers& pb, const PlanExtras& ex, int S, int bufsel,
                               const int* active, hipStream_t st) {
  if (ex.sp_P <= 0 || S <= 0) return GPMP2MI_OK;   // an empty table launches nothing
  if (ex.sp_P > ex.sp_cap || hp.D > MAXD || hp.NG + hp.D + 1 > 192) {
    set_error("k_selfpair_accumulate: table larger than the capacity, or a record wider than 192 entries");
    return GPMP2MI_ERR_INVALID;
  }
  const int nst = ex.sp_last - ex.sp_first + 1;
  k_selfpair_accumulate<<<dim3((unsigned)(hp.B * nst)), dim3(64), 0, st>>>(pb.params, pb, ex, S, bufsel, active);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

}  // namespace g2
