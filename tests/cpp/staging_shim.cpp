// C entry points around gpmp2_amd/csrc/host/staging.h for the CPU tests (tests/test_staging_cpu.py): the host driver's
// own carver, staging rule and stage layouts, built by the host compiler alone.  Nothing else lives here.
#include "host/staging.h"

using namespace g2;

extern "C" {

// n pieces of sizes[i] bytes carved from `base` as one row list: offsets[i] from the base, *total the bytes carved
void shim_carve_rows(int n, const size_t* sizes, char* base, size_t* offsets, size_t* total) {
  RowOut rows[16];
  for (int i = 0; i < n; i++) rows[i] = RowOut{nullptr, 1, sizes[i]};
  Carver c{base};
  carve_rows(c, rows, n, 1);
  for (int i = 0; i < n; i++) offsets[i] = (size_t)((uintptr_t)rows[i].staged - (uintptr_t)base);
  *total = c.off;
}

void* shim_staging_rule(int host, void* caller, void* staged) { return staging_rule(host != 0, caller, staged); }

// The bytes of a plan's workspace of stage `stage` (0 score, 1 self check, 2 motion limits, 3 moving obstacles,
// 4 workspace path, 5 re-timing, 6 distinct alternatives) by the stage's own output list and layout; rec / rec2: the bytes
// of its record sets (group: the words of a bit-matrix row, and the slots of alternatives kept)
size_t shim_stage_bytes(int stage, size_t B, size_t N, size_t D, size_t inter, size_t rec, size_t rec2, size_t max_alt) {
  const Shape s{B, N, D, N * (inter + 1) + 1};
  RowOut rows[8];
  switch (stage) {
    case 0: rows_of(ScoreOut{}, SCORE_WORST, rows); return carve_score(nullptr, rec, rows, s).bytes;
    case 1: rows_of(ScoreOut{}, SELF_WORST, rows); return carve_self(nullptr, rec, rec2, rows, s).bytes;
    case 2: rows_of(MotionOut{}, rows); return carve_motion(nullptr, rec, rows, s).bytes;
    case 3: rows_of(ScoreOut{}, MOVING_WORST, rows); return carve_moving(nullptr, rec, rows, s).bytes;
    case 4: rows_of(PathOut{}, rows); return carve_path(nullptr, rec, rows, s).bytes;
    case 5: rows_of(RetimeOut{}, s.Md, D, rows); return carve_retime(nullptr, rows, s).bytes;
    case 6: return carve_group(nullptr, s, rec, rec2, max_alt).bytes;
  }
  return 0;
}

}  // extern "C"
