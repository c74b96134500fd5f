// record_entries.h -- the packed unary record G | g | e of a support state as a sum of row products, for the factors that
// add rows [h | r] (weight w) straight into it: k_moving_accumulate, k_selfpair_accumulate, k_path_accumulate, k_carried_accumulate.
//
// The map from an entry to its two row positions is a pure function: no buffer, no thread index, and a plain host
// compiler builds the same text for the CPU tests (tests/cpp/record_entries_shim.cpp), which run every D up to MAXD.
// The device part below it (RecAcc, accumulate_sphere_rows) is seen by the kernel units only.
#pragma once

#ifndef G2_PURE
#ifdef __HIPCC__
#define G2_PURE __host__ __device__ __forceinline__
#else
#define G2_PURE inline
#endif
#endif

namespace g2 {

// entries of the record of a D-dof state: NG = D (D + 1) / 2 of G (upper triangle, packed by rows), D of g, one of e
G2_PURE int record_entries(int D, int NG) { return NG + D + 1; }

// Entry e is the sum over the rows of  w * row[ea] * row[eb],  a row being h [D] then r at position D: G (k, k2) =
// h_k h_k2, g_k = h_k r, e = r r.  e past the last entry gives (0, 0): reads stay inside the row, nothing is stored.
G2_PURE void record_entry(int D, int NG, int e, int& ea, int& eb) {
  int k = 0, rem = e;
  while (k < D && rem >= D - k) {
    rem -= D - k;
    k++;
  }
  ea = e < NG ? k : e < NG + D ? e - NG : D;
  eb = e < NG ? k + rem : D;
  if (e >= record_entries(D, NG)) ea = eb = 0;
}

// entries a lane of the one wavefront per state owns: lane, lane + 64, lane + 128.  The launchers refuse a record wider
// than 64 * REC_SLOTS entries.
constexpr int REC_SLOTS = 3;

}  // namespace g2

#ifdef __HIPCC__
#include "device_math.h"
#include "plan.h"

namespace g2 {

// The entries of one lane and their accumulators, one per entry: rows are added in the order add() is called, without
// atomics, so a state's contribution is a function of its own data.
struct RecAcc {
  int NE, ea[REC_SLOTS], eb[REC_SLOTS];
  double acc[REC_SLOTS];
  __device__ __forceinline__ RecAcc(int D, int NG) : NE(record_entries(D, NG)) {
#pragma unroll
    for (int j = 0; j < REC_SLOTS; j++) {
      record_entry(D, NG, threadIdx.x + 64 * j, ea[j], eb[j]);
      acc[j] = 0.0;
    }
  }
  __device__ __forceinline__ void add(double w, const double* row) {
#pragma unroll
    for (int j = 0; j < REC_SLOTS; j++) acc[j] += w * row[ea[j]] * row[eb[j]];
  }
  // into the unary record of support state i of trajectory b
  __device__ __forceinline__ void store(const PlanBuffers& pb, int b, int i, int bufsel, const PlanParams& P) const {
    double* rec = rec_of(pb, pb.which[b], bufsel) + ((size_t)b * P.Ppad + (size_t)i * (P.I + 1)) * P.RECS;
#pragma unroll
    for (int j = 0; j < REC_SLOTS; j++)
      if ((int)threadIdx.x + 64 * j < NE) rec[threadIdx.x + 64 * j] += acc[j];
  }
};

// The sphere-pair factors of one state, one wavefront: the n pairs are taken in chunks of 64, one pair per lane.  A
// chunk without an active pair (ballot) is skipped; an active one leaves its rows [h | r | w] in LDS -- the Jacobian row
// is formed by the active lanes only -- and every lane adds the active rows, in ascending pair order, to its entries.
// `pairs` supplies, for pair p:  SphereHinge hinge(p, Pair&)  (which also fills the Pair: what row() needs, and the
// weight w) and  row(pair, hinge, h)  writing h [D].  Returns whether any pair was active.  A pair that is not active
// would add an exact zero, so skipping it changes no bit.
template <int LD, class Pairs>
__device__ __forceinline__ bool accumulate_sphere_rows(double (&rows)[64][LD], int D, int n, const Pairs& pairs,
                                                       RecAcc& acc) {
  static_assert(LD >= MAXD + 2, "an LDS row holds h [D], r and w");
  const int lane = threadIdx.x;
  bool any = false;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int p = c0 + lane;
    SphereHinge hg;
    hg.active = false;
    typename Pairs::Pair pr{};
    if (p < n) hg = pairs.hinge(p, pr);
    const unsigned long long mask = __ballot(hg.active);
    if (mask == 0) continue;   // wavefront-uniform
    any = true;
    if (hg.active) {
      pairs.row(pr, hg, rows[lane]);
      rows[lane][D] = hg.err;
      rows[lane][D + 1] = pr.w;
    }
    __syncthreads();
    for (unsigned long long mm = mask; mm; mm &= mm - 1) {   // active rows in ascending pair order
      const int l = __ffsll((long long)mm) - 1;
      acc.add(rows[l][D + 1], rows[l]);
    }
    __syncthreads();
  }
  return any;
}

}  // namespace g2
#endif
