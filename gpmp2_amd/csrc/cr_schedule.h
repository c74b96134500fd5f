// cr_schedule.h -- which block the tasks of a cyclic-reduction level work on, for every kernel that walks the tree
// (cr_kernels.hip, wide_cr.h, dense_kernels.hip) and for the launchers that size their grids.  Integers only; a plain
// host compiler builds the same text for the CPU tests (tests/cpp/control_shim.cpp).
//
// Blocks 0 .. N.  Forward level h = 1, 2, 4, ..: the blocks still in the tree are the multiples of h; each absorbs the
// Schur complements of its neighbours j -+ h/2 (eliminated one level below), the odd multiples are then eliminated
// (E tasks) and the even multiples store their updated block (U tasks).  The final level is the first h > N: block 0
// is alone.  Backward level h solves the blocks eliminated at level h from x_{j-h}, x_{j+h}.  (The 2 x 2-tile and
// dense paths: wide_cr.h, dense_kernels.hip.)
//
// The ROOTED schedule (crr_*; the one-tile path, cr_kernels.hip and the fused finish of linearize_kernels.hip) numbers the
// same blocks v = j + 1 = 1 .. N + 1 and there is no block v = 0.  A block belongs to the level of the lowest set bit
// of v: level h eliminates the odd multiples of h in [1, N + 1], the even multiples are its U tasks.  A coupling to
// v - h = 0 or to v + h > N + 1 does not exist, so the first E block of every level has no left coupling, and the top
// level -- the largest power of two <= N + 1 -- is a single block without couplings: the root lies INSIDE the chain
// and the tree has floor(log2(N + 1)) + 1 levels, one fewer than above whenever N + 1 is no power of two (block 0 of
// the schedule above has no set bit, outlives every level and needs a level of its own).  Per-block storage stays
// addressed by the state j = v - 1.
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

// ---- rooted schedule: tree index v = j + 1 in [1, N + 1]
G2_PURE int crr_top(int N) { return 1 << (31 - __builtin_clz((unsigned)(N + 1))); }     // N >= 0
G2_PURE int crr_levels(int N) { return 32 - __builtin_clz((unsigned)(N + 1)); }
// One forward level, tasks ordered as in CrLevel; block() is the tree index v.  At the top level countE = 1, countU = 0.
struct CrrLevel {
  int h, countE, countU;
  G2_PURE int tasks() const { return countE + countU; }
  G2_PURE bool elim(int idx) const { return idx < countE; }
  G2_PURE int block(int idx) const { return elim(idx) ? h * (2 * idx + 1) : 2 * h * (idx - countE + 1); }
};
G2_PURE CrrLevel crr_level(int N, int h, bool updates = true) {
  const int m = (N + 1) / h;                       // multiples of h in [1, N + 1]
  return CrrLevel{h, (m + 1) / 2, updates ? m / 2 : 0};
}
G2_PURE int crr_back_count(int N, int h) { return ((N + 1) / h + 1) / 2; }
G2_PURE int crr_back_block(int, int h, int idx) { return h * (2 * idx + 1); }
// workgroups that take the tree indices g q .. g q + g - 1 (g = 4: k_assemble, g = 8: the finish kernels): v = 0 opens
// the first group, so that every group is aligned with the tree
G2_PURE int crr_groups(int N, int g) { return (N + 1) / g + 1; }

constexpr int ZNS = 24, FXS = 40;   // states a chunk of 64 evaluation points may read; slots of its step window
// the most states a chunk reads with I sub-steps per interval: 63 / (I + 1) + 2 that its points belong to, and the one before
G2_PURE constexpr int chunk_states(int I) { return 63 / (I + 1) + 3; }

// The blocks a workgroup must back-substitute itself (levels 4, 2, 1) to know the step of the states s0 .. s1, once the
// solve kernel has handed over the multiples of 8 (fused finish, k_linearize_arm): bit k of a mask is the tree index
// v = w0 + k, w0 the multiple of 8 at or below s0 + 1.  A block of level h needs its neighbours at distance h, which
// belong to higher levels; need8 are the handed-over blocks to fetch.  s1 - s0 < ZNS: every bit lies below w0 + 33, and
// `span` (<= 64; FXS in the kernel) is the number of window slots the caller has.
struct CrrWindow {
  int w0;
  unsigned long long need1, need2, need4, need8;
};
G2_PURE unsigned long long crr_bits(int lo, int hi) {   // bits lo .. hi, hi <= 63; empty when hi < lo
  return (hi < lo) ? 0ull : ((~0ull >> (63 - (hi - lo))) << lo);
}
G2_PURE CrrWindow crr_window(int N, int s0, int s1, int span) {
  typedef unsigned long long u64;
  const int w0 = (s0 + 1) & ~7, last = N + 1 - w0;
  const u64 valid = crr_bits(w0 == 0 ? 1 : 0, last < span - 1 ? last : span - 1), inr = crr_bits(s0 + 1 - w0, s1 + 1 - w0);
  const u64 L1 = 0xAAAAAAAAAAAAAAAAull, L2 = 0x4444444444444444ull, L4 = 0x1010101010101010ull, L8 = 0x0101010101010101ull;
  const u64 need1 = inr & L1 & valid, nb1 = (need1 << 1) | (need1 >> 1);
  const u64 need2 = (inr | nb1) & L2 & valid, nb2 = (need2 << 2) | (need2 >> 2);
  const u64 need4 = (inr | nb1 | nb2) & L4 & valid, nb4 = (need4 << 4) | (need4 >> 4);
  const u64 need8 = (inr | nb1 | nb2 | nb4) & L8 & valid;
  return CrrWindow{w0, need1, need2, need4, need8};
}

}  // namespace g2
