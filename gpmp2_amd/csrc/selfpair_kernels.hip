// selfpair_kernels.hip -- the self-collision table of a plan (include/gpmp2mi.h "self-collision table in a plan"): P
// pairs of the robot's own spheres, each with its epsilon and sigma, as a factor on the support states of a range.
//
//   k_selfpair_accumulate  One wavefront per (trajectory, support state of the range).  The P pairs, formed from the
//                          plan's records (PlanExtras::sp_rec) and the centres / Jacobians k_sphere_centers left
//                          (PlanExtras::cen, Jc), go through accumulate_sphere_rows (record_entries.h): chunks of 64,
//                          the active rows [h | r | w] through LDS -- the Jacobian difference is formed by the active
//                          lanes only -- into the record entries a lane owns (RecAcc).  The P x D rows never reach memory.
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
#include "record_entries.h"

namespace g2 {

constexpr int SP_LD = MAXD + 3;   // an LDS row: h [D], r, w; odd, see above

namespace {

// pair p of the table for accumulate_sphere_rows
struct TablePairs {
  const SelfPairRec* rec;
  const double *cen, *Jc;   // of the state
  int D;
  struct Pair {
    int sa, sb;
    double w;
  };
  __device__ __forceinline__ SphereHinge hinge(int p, Pair& pr) const {
    const SelfPairRec r = rec[p];
    pr.sa = r.a;
    pr.sb = r.b;
    pr.w = r.w;
    return sphere_hinge(cen[r.a * 3] - cen[r.b * 3], cen[r.a * 3 + 1] - cen[r.b * 3 + 1],
                        cen[r.a * 3 + 2] - cen[r.b * 3 + 2], r.total_eps);
  }
  __device__ __forceinline__ void row(const Pair& pr, const SphereHinge& hg, double* h) const {
    const double* Ja = Jc + (size_t)pr.sa * 3 * D;
    const double* Jb = Jc + (size_t)pr.sb * 3 * D;
    for (int d = 0; d < D; d++)
      h[d] = -(hg.n[0] * (Ja[d] - Jb[d]) + hg.n[1] * (Ja[D + d] - Jb[D + d]) + hg.n[2] * (Ja[2 * D + d] - Jb[2 * D + d]));
  }
};

}  // namespace

__global__ __launch_bounds__(64) void k_selfpair_accumulate(const PlanParams* __restrict__ pp, PlanBuffers pb,
                                                             PlanExtras ex, int S, int bufsel,
                                                             const int* __restrict__ active) {
  __shared__ double rows[64][SP_LD];
  const PlanParams& P = *pp;
  const int N = P.N, D = P.D;
  const int nst = ex.sp_last - ex.sp_first + 1;
  const int b = blockIdx.x / nst, i = ex.sp_first + blockIdx.x % nst;
  if (active && !active[b]) return;
  const size_t m = (size_t)b * (N + 1) + i;
  RecAcc acc(D, P.NG);
  const TablePairs pairs{ex.sp_rec, ex.cen + m * S * 3, ex.Jc + m * S * 3 * D, D};
  if (accumulate_sphere_rows(rows, D, ex.sp_P, pairs, acc)) acc.store(pb, b, i, bufsel, P);
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
