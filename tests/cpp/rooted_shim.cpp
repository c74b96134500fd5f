// C entry points around the rooted cyclic-reduction schedule of gpmp2_amd/csrc/cr_schedule.h (crr_*) for the CPU tests
// (tests/rooted_shim.py): the product's own text, built by the host compiler.  Nothing else lives here.
#include "cr_schedule.h"

using namespace g2;

extern "C" {

int shim_crr_top(int N) { return crr_top(N); }
int shim_crr_levels(int N) { return crr_levels(N); }
int shim_cr_hfinal(int N) { return cr_hfinal(N); }
// one forward level: elim[idx], block[idx] (tree index v) of its tasks (room for N + 2 each); returns their number;
// counts = {countE, countU}
int shim_crr_level(int N, int h, int updates, int* elim, int* block, int* counts) {
  const CrrLevel level = crr_level(N, h, updates != 0);
  for (int idx = 0; idx < level.tasks(); idx++) {
    elim[idx] = level.elim(idx) ? 1 : 0;
    block[idx] = level.block(idx);
  }
  counts[0] = level.countE;
  counts[1] = level.countU;
  return level.tasks();
}
int shim_crr_back_count(int N, int h) { return crr_back_count(N, h); }
int shim_crr_back_block(int N, int h, int idx) { return crr_back_block(N, h, idx); }
int shim_crr_groups(int N, int g) { return crr_groups(N, g); }
// the fused finish's bounds: states per chunk, slots of the step window; the most states a chunk reads
int shim_zns() { return ZNS; }
int shim_fxs() { return FXS; }
int shim_chunk_states(int I) { return chunk_states(I); }
// out = {need1, need2, need4, need8}; returns w0
int shim_crr_window(int N, int s0, int s1, int span, unsigned long long* out) {
  const CrrWindow w = crr_window(N, s0, s1, span);
  out[0] = w.need1;
  out[1] = w.need2;
  out[2] = w.need4;
  out[3] = w.need8;
  return w.w0;
}

}  // extern "C"
