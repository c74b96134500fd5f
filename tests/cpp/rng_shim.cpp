// rng_shim.cpp -- gpmp2_amd/csrc/rng.h built by the host compiler behind C entry points, so that the CPU tests
// (tests/test_rng_cpu.py) run the kernels' own text.
#include "rng.h"

extern "C" {

void shim_philox(const uint32_t* c, const uint32_t* k, uint32_t* out) {
  const g2::RngBlock o = g2::philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1]);
  for (int t = 0; t < 4; t++) out[t] = o.o[t];
}

// n tuples: the counter and the block that coordinate r[t] of block i[t] of problem (a[t], b[t]) reads, and the normal
void shim_tuples(int n, const uint64_t* seed, const uint32_t* stream, const uint32_t* a, const uint32_t* b,
                 const uint32_t* i, const int* r, uint32_t* counter, uint32_t* block, double* z) {
  for (int t = 0; t < n; t++) {
    const int pair = g2::rng_pair_of(r[t]);
    const g2::RngBlock c = g2::rng_counter(stream[t], a[t], b[t], i[t], pair);
    const g2::RngBlock o = g2::rng_block(seed[t], stream[t], a[t], b[t], i[t], pair);
    for (int w = 0; w < 4; w++) {
      counter[4 * t + w] = c.o[w];
      block[4 * t + w] = o.o[w];
    }
    z[t] = g2::normal(seed[t], stream[t], a[t], b[t], i[t], r[t]);
  }
}

}  // extern "C"
