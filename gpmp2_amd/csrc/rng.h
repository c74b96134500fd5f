// rng.h -- the library's random function, stated once (include/gpmp2mi.h "seeding"): a counter-based standard normal
//     z = normal(seed, stream, a, b, i, r)
// that is a pure function of its arguments.  No state, no buffer, no thread index: a kernel that needs coordinate r of
// block i of problem (a, b) computes it where it needs it, so a problem's numbers depend on (seed, indices) alone and
// never on the batch, the slot, the shard or the entry point that asked.  A plain host compiler builds the same text
// for the CPU tests (tests/cpp/rng_shim.cpp), as step_control.h and cr_schedule.h.
//
// Generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) with the
// Random123 constants: multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85.
//
// Packing (how the arguments become the 128-bit counter and the 64-bit key):
//     key     = (seed low word, seed high word)
//     counter = (a, b, i, stream << 8 | pair)          stream < 2^24, i >= 0, pair = 0..7
// Every argument owns its own bits, so two different (stream, a, b, i, pair) never share a counter and therefore never
// read the same block output.
//
// Pairing (which two coordinates share one block): coordinates r and r + 4 with bit 2 of r clear,
//     pair = (r & 3) + 4 (r >> 3):   {0,4} {1,5} {2,6} {3,7} {8,12} {9,13} {10,14} {11,15}
// the cosine member is r, the sine member r + 4.  In the tile layout of tiles.h a lane holds rows g, g + 4, g + 8, g + 12
// of its column: registers (0, 1) are one pair and (2, 3) the other, so a lane computes two blocks and keeps all four
// normals (normal_pair below); nothing is computed to be thrown away.  r = 0..15.
//
// Block to normals: o[0..3] the block output,
//     hi53 = o[0] << 21 | o[1] >> 11,   lo53 = o[2] << 21 | o[3] >> 11          (the top 53 bits of each half)
//     u1 = (hi53 + 1) 2^-53 in (0, 1],  u2 = lo53 2^-53 in [0, 1)
//     (sqrt(-2 ln u1) cos 2 pi u2, sqrt(-2 ln u1) sin 2 pi u2)                   Box-Muller, fp64 throughout
// Every output is finite, and |z| <= sqrt(106 ln 2) ~ 8.57 by construction.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/gpmp2mi.h"

#ifndef G2_PURE
#ifdef __HIPCC__
#define G2_PURE __host__ __device__ __forceinline__
#else
#define G2_PURE inline
#endif
#endif

namespace g2 {

// the uses of the function: one stream each, so that restarts and posterior samples of one seed are independent
enum { RNG_STREAM_RESTARTS = GPMP2MI_RNG_RESTARTS, RNG_STREAM_POSTERIOR = GPMP2MI_RNG_POSTERIOR };
constexpr uint32_t RNG_STREAM_MAX = (1u << 24) - 1;

struct RngBlock {
  uint32_t o[4];
};

G2_PURE RngBlock philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int round = 0; round < 10; round++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return RngBlock{{c0, c1, c2, c3}};
}

G2_PURE int rng_pair_of(int r) { return (r & 3) + 4 * (r >> 3); }
G2_PURE int rng_is_sine(int r) { return (r >> 2) & 1; }

// the counter of pair `pair` of block i of problem (a, b): the packing stated above
G2_PURE RngBlock rng_counter(uint32_t stream, uint32_t a, uint32_t b, uint32_t i, int pair) {
  return RngBlock{{a, b, i, (stream << 8) | (uint32_t)pair}};
}
// ... and the block it holds
G2_PURE RngBlock rng_block(uint64_t seed, uint32_t stream, uint32_t a, uint32_t b, uint32_t i, int pair) {
  const RngBlock c = rng_counter(stream, a, b, i, pair);
  return philox4x32_10(c.o[0], c.o[1], c.o[2], c.o[3], (uint32_t)seed, (uint32_t)(seed >> 32));
}

// Box-Muller on one block: zc the cosine member, zs the sine member
G2_PURE void rng_box_muller(const RngBlock& k, double& zc, double& zs) {
  const uint64_t hi53 = ((uint64_t)k.o[0] << 21) | (k.o[1] >> 11), lo53 = ((uint64_t)k.o[2] << 21) | (k.o[3] >> 11);
  const double two53 = 1.0 / 9007199254740992.0;
  const double u1 = (double)(hi53 + 1) * two53, u2 = (double)lo53 * two53;
  const double rad = sqrt(-2.0 * log(u1)), ang = 6.283185307179586476925286766559 * u2;
  zc = rad * cos(ang);
  zs = rad * sin(ang);
}

// both members of a pair: coordinates r = (pair & 3) + 8 (pair >> 2) (cosine) and r + 4 (sine)
G2_PURE void normal_pair(uint64_t seed, uint32_t stream, uint32_t a, uint32_t b, uint32_t i, int pair, double& zc,
                         double& zs) {
  rng_box_muller(rng_block(seed, stream, a, b, i, pair), zc, zs);
}

// The uniform of coordinate r (include/gpmp2mi.h "goal configurations"): x 2^-53 in [0, 1), x the hi53 word of r's
// block for a cosine member and the lo53 word for a sine member -- the words Box-Muller reads, without the + 1.
G2_PURE double uniform(uint64_t seed, uint32_t stream, uint32_t a, uint32_t b, uint32_t i, int r) {
  const RngBlock k = rng_block(seed, stream, a, b, i, rng_pair_of(r));
  const uint64_t hi53 = ((uint64_t)k.o[0] << 21) | (k.o[1] >> 11), lo53 = ((uint64_t)k.o[2] << 21) | (k.o[3] >> 11);
  return (double)(rng_is_sine(r) ? lo53 : hi53) * (1.0 / 9007199254740992.0);
}

G2_PURE double normal(uint64_t seed, uint32_t stream, uint32_t a, uint32_t b, uint32_t i, int r) {
  double zc, zs;
  normal_pair(seed, stream, a, b, i, rng_pair_of(r), zc, zs);
  return rng_is_sine(r) ? zs : zc;
}

}  // namespace g2
