// cr_schedule.h -- which block the tasks of a cyclic-reduction level work on, for every kernel that walks the tree
// (cr_kernels.hip, wide_cr.h, dense_kernels.hip) and for the launchers that size their grids.  Integers only; a plain
// host compiler builds the same text for the CPU tests (tests/cpp/control_shim.cpp).
//
// Blocks 0 .. N.  Forward level h = 1, 2, 4, ..: the blocks still in the tree are the multiples of h; each absorbs the
// Schur complements of its neighbours j -+ h/2 (eliminated one level below), the odd multiples are then eliminated
// (E tasks) and the even multiples store their updated block (U tasks).  The final level is the first h > N: block 0
// is alone.  Backward level h solves the blocks eliminated at level h from x_{j-h}, x_{j+h}.
#pragma once

#ifndef G2_PURE
#ifdef __HIPCC__
#define G2_PURE __host__ __device__ __forceinline__
#else
#define G2_PURE inline
#endif
#endif

namespace g2 {

// the final level: the first power of two above N.  Every function below asks for it, inside the kernels' level and
// task loops, so it is three scalar instructions and not a loop.
G2_PURE int cr_hfinal(int N) { return N < 1 ? 1 : 1 << (32 - __builtin_clz((unsigned)N)); }

// One forward level: tasks 0 .. countE - 1 are the E tasks, the U tasks follow.
struct CrLevel {
  int h, countE, countU;
  bool final;
  G2_PURE int tasks() const { return countE + countU; }
  G2_PURE bool elim(int idx) const { return idx < countE; }
  G2_PURE int block(int idx) const { return elim(idx) ? (final ? 0 : h * (2 * idx + 1)) : 2 * h * (idx - countE); }
};
// updates = false: the level has no U tasks (nothing to absorb yet, or the caller defers them to the next level)
G2_PURE CrLevel cr_level(int N, int h, bool updates = true) {
  const bool final = (h == cr_hfinal(N));
  const int countE = final ? 1 : ((N / h) + 1) / 2;
  const int countU = (final || !updates) ? 0 : (N / (2 * h)) + 1;  // multiples of 2h in [0, N]
  return CrLevel{h, countE, countU, final};
}

// backward level h: its tasks and the block of task idx
G2_PURE int cr_back_count(int N, int h) { return (h == cr_hfinal(N)) ? 1 : ((N / h) + 1) / 2; }
G2_PURE int cr_back_block(int N, int h, int idx) { return (h == cr_hfinal(N)) ? 0 : h * (2 * idx + 1); }

}  // namespace g2
