// C entry points around gpmp2_amd/csrc/pass_counter.h for the CPU test (tests/test_pass_counter_cpu.py): the kernels'
// own text, built by the host compiler.  Nothing else lives here.
#include <cstdint>

#include "pass_counter.h"

using namespace g2;

extern "C" {

uint64_t shim_pass_arrival(int continues) { return pass_arrival(continues); }
int shim_pass_arrivals_before(uint64_t before) { return pass_arrivals_before(before); }
int shim_pass_arrived_last(uint64_t before, int grid) { return pass_arrived_last(before, grid) ? 1 : 0; }
int shim_pass_count(uint64_t before, int continues) { return pass_count(before, continues); }

// The `grid` workgroups arrive in the order `order` (a permutation of 0 .. grid - 1), workgroup w adding its
// continues[w] the way publish_pass_count does: word += pass_arrival(c), looking at the value the add found.
// Returns how many arrivals reported "last"; *who = the position in `order` of the (last) one that did, *count = what
// it decoded, *word_out = the word afterwards.
int shim_pass_run(int grid, const int* order, const int* continues, int* who, int* count, uint64_t* word_out) {
  uint64_t word = 0;
  int lasts = 0;
  *who = -1;
  *count = -1;
  for (int k = 0; k < grid; k++) {
    const int c = continues[order[k]];
    const uint64_t before = word;   // what the atomic add returns
    word += pass_arrival(c);
    if (pass_arrived_last(before, grid)) {
      lasts++;
      *who = k;
      *count = pass_count(before, c);
    }
  }
  *word_out = word;
  return lasts;
}

}  // extern "C"
