// C entry points around gpmp2_amd/csrc/scene_rule.h for the CPU tests (tests/scene_shim.py): the kernels' own text of
// the mesh rule, built by the host compiler.  Nothing else lives here.
#include "scene_rule.h"

using namespace g2;

extern "C" {

// 1 and *q for an accepted coordinate, 0 when the whole-mesh guard fires
int shim_scene_quantize(double g, long long* q) {
  int64_t v = 0;
  if (!scene_quantize(g, &v)) return 0;
  *q = v;
  return 1;
}

// One triangle (fixed-point vertices [3][3]) against the column (Y, Z): -1 the triangle is skipped (a == 0), 0 the column
// does not cross it, 1 it does; then *first = ceil(x), e[3] the edge functions and *a the oriented area.
int shim_scene_column(const long long* p, long long Y, long long Z, double* first, long long* e, long long* a) {
  SceneTri t;
  for (int n = 0; n < 3; n++)
    for (int c = 0; c < 3; c++) t.p[n][c] = p[3 * n + c];
  if (!scene_orient(t)) return -1;
  *a = t.a;
  int64_t ee[3];
  const bool crosses = scene_column_crosses(t, Y, Z, ee);
  for (int n = 0; n < 3; n++) e[n] = ee[n];
  if (!crosses) return 0;
  *first = scene_first(t, ee);
  return 1;
}

long long shim_scene_floor_cell(long long v) { return scene_floor_cell(v); }
long long shim_scene_ceil_cell(long long v) { return scene_ceil_cell(v); }

}  // extern "C"
