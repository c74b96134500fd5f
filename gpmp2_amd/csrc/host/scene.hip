// scene.hip -- scene (include/gpmp2mi.h "scene"): boxes, spheres, cylinders and closed meshes as one more source of a
// field handle's obstacle set.  The seeds of the base and of the evidence are the existing ones (launch_map_seed, the
// seed-writing form of k_sensor_apply through evidence_seed); the objects are marked on top (scene_kernels.hip), and the
// transform behind the seeds is map.hip's (map_transform), so the field is what the occupancy constructor gives for the
// same obstacle set.
#include <climits>
#include <cmath>
#include <cstring>

#include "host.h"

using namespace g2;

namespace {

int check_pose(const double* pose) {
  for (int k = 0; k < 12; k++) G2_CHECK(std::isfinite(pose[k]), GPMP2MI_ERR_INVALID, "an object's pose is not finite");
  return GPMP2MI_OK;
}

// a closed mesh: every undirected edge, as a pair of vertex indices, occurs in an even number of triangles
bool mesh_is_closed(int T, const int* tri) {
  std::vector<uint64_t> edges;
  edges.reserve((size_t)T * 3);
  for (int t = 0; t < T; t++)
    for (int n = 0; n < 3; n++) {
      const uint64_t a = (uint64_t)tri[3 * (size_t)t + n], b = (uint64_t)tri[3 * (size_t)t + (n + 1) % 3];
      edges.push_back(a < b ? (a << 32) | b : (b << 32) | a);
    }
  std::sort(edges.begin(), edges.end());
  for (size_t i = 0; i < edges.size();) {
    size_t j = i;
    while (j < edges.size() && edges[j] == edges[i]) j++;
    if ((j - i) & 1) return false;
    i = j;
  }
  return true;
}

int check_object(const gpmp2mi_scene_object& o) {
  G2_CHECK(o.kind >= GPMP2MI_SCENE_BOX && o.kind <= GPMP2MI_SCENE_MESH, GPMP2MI_ERR_INVALID, "unknown object kind");
  G2_TRY(check_pose(o.pose));
  G2_CHECK(std::isfinite(o.inflate), GPMP2MI_ERR_INVALID, "an object's inflate is not finite");
  G2_CHECK(o.inflate >= 0.0, GPMP2MI_ERR_INVALID, "an object's inflate is negative");
  if (o.kind != GPMP2MI_SCENE_MESH) {
    const int used = o.kind == GPMP2MI_SCENE_BOX ? 3 : (o.kind == GPMP2MI_SCENE_SPHERE ? 1 : 2);
    for (int n = 0; n < used; n++) {
      G2_CHECK(std::isfinite(o.size[n]), GPMP2MI_ERR_INVALID, "an object's size is not finite");
      G2_CHECK(o.size[n] >= 0.0, GPMP2MI_ERR_INVALID, "an object's size is negative");
    }
    return GPMP2MI_OK;
  }
  G2_CHECK(o.inflate == 0.0, GPMP2MI_ERR_INVALID, "a mesh cannot be inflated: inflate must be 0");
  G2_CHECK(o.n_vertices >= 4 && o.n_triangles >= 4, GPMP2MI_ERR_INVALID,
           "a mesh needs at least 4 vertices and 4 triangles");
  G2_CHECK(o.vertices && o.triangles, GPMP2MI_ERR_INVALID, "null vertices or triangles of a mesh");
  G2_CHECK(o.n_triangles <= GPMP2MI_MAX_SCENE_TRIANGLES, GPMP2MI_ERR_UNSUPPORTED,
           "a mesh has more than 2^20 triangles");
  for (int t = 0; t < o.n_triangles; t++) {
    const int* v = o.triangles + 3 * (size_t)t;
    for (int n = 0; n < 3; n++)
      G2_CHECK(v[n] >= 0 && v[n] < o.n_vertices, GPMP2MI_ERR_INVALID, "a triangle's vertex index is outside 0 .. V-1");
    G2_CHECK(v[0] != v[1] && v[1] != v[2] && v[0] != v[2], GPMP2MI_ERR_INVALID, "a triangle has a repeated index");
  }
  G2_CHECK(mesh_is_closed(o.n_triangles, o.triangles), GPMP2MI_ERR_INVALID,
           "a mesh is not closed: some edge occurs in an odd number of triangles");
  return GPMP2MI_OK;
}

int check_range(const gpmp2mi_scene* sc, int first, int count, const void* data, const char* what) {
  G2_CHECK(sc, GPMP2MI_ERR_INVALID, "null scene handle");
  G2_CHECK(first >= 0 && count >= 0 && (long long)first + count <= (long long)sc->obj.size(), GPMP2MI_ERR_INVALID,
           "first / count are outside the scene");
  G2_CHECK(data || count == 0, GPMP2MI_ERR_INVALID, what);
  return GPMP2MI_OK;
}

int check_grid(int dim, const double* origin, double cell, int nx, int ny, int nz) {
  G2_CHECK(origin, GPMP2MI_ERR_INVALID, "null origin");
  G2_CHECK(dim == 2 || dim == 3, GPMP2MI_ERR_INVALID, "dim must be 2 or 3");
  G2_CHECK(nx >= 1 && ny >= 1 && nz >= 1, GPMP2MI_ERR_INVALID, "the grid sizes nx, ny, nz must be >= 1");
  G2_CHECK(dim == 3 || nz == 1, GPMP2MI_ERR_INVALID, "a planar grid has nz = 1");
  G2_CHECK(std::isfinite(cell) && cell > 0.0, GPMP2MI_ERR_INVALID, "cell_size must be finite and > 0");
  for (int k = 0; k < dim; k++) G2_CHECK(std::isfinite(origin[k]), GPMP2MI_ERR_INVALID, "the grid origin is not finite");
  return GPMP2MI_OK;
}

size_t bits_bytes_for(int nx, int ny, int nz) { return (size_t)ny * nz * ((nx + 31) / 32) * sizeof(unsigned); }

// once the arguments are accepted: the scene's device current, and the bit volume for the grid (all 0)
int scene_ready(const gpmp2mi_scene* sc, int nx, int ny, int nz) {
  G2_TRY(ensure_device());
  int cur = -1;
  G2_HIP(hipGetDevice(&cur));
  G2_CHECK(cur == sc->device, GPMP2MI_ERR_INVALID, "the scene handle lives on another device than the current one");
  const size_t need = bits_bytes_for(nx, ny, nz);
  if (need > sc->bits.bytes) {
    G2_TRY(sc->bits.reserve(need));
    G2_HIP(hipMemsetAsync(sc->bits.p, 0, need, nullptr));
    G2_HIP(hipStreamSynchronize(nullptr));   // the first `_dev` call may come on any stream
  }
  return GPMP2MI_OK;
}

// The cell box the lanes of a primitive run over: a ball around t that holds the object when R is orthonormal, grown by a
// cell; the whole grid when R is anything else (R is used as given, so the object may be any parallelepiped).  False:
// the box holds no cell.
bool prim_box(const gpmp2mi_scene::Object& o, const SensorGrid& g, ScenePrim* p) {
  const double* P = o.pose;
  double r = o.s[0];
  bool whole = false;
  if (o.kind != SCENE_SPHERE) {
    r = o.kind == SCENE_BOX ? std::sqrt(o.s[0] * o.s[0] + o.s[1] * o.s[1] + o.s[2] * o.s[2])
                            : std::sqrt(o.s[0] * o.s[0] + o.s[1] * o.s[1]);
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) {
        const double dot = P[a] * P[b] + P[4 + a] * P[4 + b] + P[8 + a] * P[8 + b];
        if (!(std::fabs(dot - (a == b ? 1.0 : 0.0)) <= 1e-9)) whole = true;
      }
    r *= 1.0 + 1e-6;
  }
  const int n[3] = {g.nx, g.ny, g.nz};
  const double org[3] = {g.ox, g.oy, g.dim == 3 ? g.oz : 0.0};
  for (int a = 0; a < 3; a++) {
    const double t = P[4 * a + 3];
    // comparisons that a NaN or an infinity fails leave the whole axis
    const double lo = whole ? 0.0 : std::floor((t - r - org[a]) / g.cell) - 1.0;
    const double hi = whole ? (double)n[a] : std::ceil((t + r - org[a]) / g.cell) + 1.0;
    const int l = lo > 0.0 ? (lo < (double)n[a] ? (int)lo : n[a]) : 0;
    const int h = hi < (double)(n[a] - 1) ? (hi > -1.0 ? (int)hi : -1) : n[a] - 1;
    if (h < l) return false;
    p->lo[a] = l;
    p->n[a] = h - l + 1;
  }
  p->kind = o.kind;
  for (int a = 0; a < 3; a++) {
    for (int b = 0; b < 3; b++) p->R[3 * a + b] = P[4 * a + b];
    p->t[a] = P[4 * a + 3];
    p->s[a] = o.s[a];
  }
  return true;
}

void mark_scene(const gpmp2mi_scene* sc, int k, hipStream_t st) {
  if (sc->timing) (void)hipEventRecord(sc->ev[k], st);
}

// The enabled objects into the two volumes (mask null) or the byte mask, the counts into the scene's own [K] on `st`
int raster(const gpmp2mi_scene* sc, const SensorGrid& g, int* wa, int* wb, unsigned char* mask, hipStream_t st) {
  const int K = (int)sc->obj.size();
  G2_HIP(hipMemsetAsync(sc->counts, 0, 2 * (size_t)K * sizeof(int), st));
  mark_scene(sc, 0, st);
  ScenePrims b{};
  b.g = g;
  b.wa = wa; b.wb = wb; b.mask = mask;
  b.cells = sc->counts;
  for (int k = 0; k < K; k++) {
    const auto& o = sc->obj[k];
    if (!o.enabled || o.kind == SCENE_MESH) continue;
    if (!prim_box(o, g, &b.p[b.count])) continue;
    b.p[b.count++].obj = k;
    if (b.count == SCENE_PRIM_BATCH) {
      G2_TRY(launch_scene_prims(b, st));
      b.count = 0;
    }
  }
  G2_TRY(launch_scene_prims(b, st));
  mark_scene(sc, 1, st);
  for (int k = 0; k < K; k++) {
    const auto& o = sc->obj[k];
    if (!o.enabled || o.kind != SCENE_MESH) continue;
    SceneMesh m{};
    m.g = g;
    m.obj = k;
    m.V = o.V; m.T = o.T;
    m.verts = (const double*)(sc->geo + o.vert_off);
    m.tris = (const int*)(sc->geo + o.tri_off);
    m.q = (int*)(sc->geo + o.q_off);
    std::memcpy(m.pose, o.pose, sizeof(m.pose));
    m.flag = sc->counts + K + k;
    m.bits = (unsigned*)sc->bits.p;
    m.W = (g.nx + 31) / 32;
    m.wa = wa; m.wb = wb; m.mask = mask;
    m.cells = sc->counts;
    G2_TRY(launch_scene_mesh(m, st));
  }
  mark_scene(sc, 2, st);
  return GPMP2MI_OK;
}

int check_rasterize_args(const gpmp2mi_scene* sc, int dim, const double* origin, double cell, int nx, int ny, int nz,
                         const unsigned char* mask) {
  G2_CHECK(sc, GPMP2MI_ERR_INVALID, "null scene handle");
  G2_CHECK(mask, GPMP2MI_ERR_INVALID, "null mask");
  return check_grid(dim, origin, cell, nx, ny, nz);
}

int rasterize(const gpmp2mi_scene* sc, int dim, const double* origin, double cell, int nx, int ny, int nz,
              unsigned char* d_mask, int* d_cells, hipStream_t st) {
  SensorGrid g{};
  g.dim = dim; g.nx = nx; g.ny = ny; g.nz = nz;
  g.ox = origin[0]; g.oy = origin[1]; g.oz = dim == 3 ? origin[2] : 0.0;
  g.cell = cell;
  G2_HIP(hipMemsetAsync(d_mask, 0, (size_t)nx * ny * nz, st));
  G2_TRY(raster(sc, g, nullptr, nullptr, d_mask, st));
  if (d_cells)
    G2_HIP(hipMemcpyAsync(d_cells, sc->counts, sc->obj.size() * sizeof(int), hipMemcpyDeviceToDevice, st));
  return GPMP2MI_OK;
}

int check_update_args(const gpmp2mi_sdf* s, const gpmp2mi_scene* sc, int use_base, int use_evidence, int occupied_at) {
  G2_CHECK(s, GPMP2MI_ERR_INVALID, "null field handle");
  G2_CHECK(sc, GPMP2MI_ERR_INVALID, "null scene handle");
  G2_CHECK(occupied_at >= -32768 && occupied_at <= 32767, GPMP2MI_ERR_INVALID, "occupied_at must be in -32768 .. 32767");
  G2_CHECK(!use_base || s->has_base, GPMP2MI_ERR_INVALID,
           "use_base on a handle without a base: call gpmp2mi_sdf_update_from_occupancy first");
  G2_CHECK(!use_evidence || s->ev_ws, GPMP2MI_ERR_INVALID,
           "use_evidence on a handle without evidence: integrate a frame or call gpmp2mi_sdf_reserve_evidence first");
  G2_CHECK(sc->device == s->device, GPMP2MI_ERR_INVALID, "the scene handle lives on another device than the field");
  return GPMP2MI_OK;
}

int update_from_scene(gpmp2mi_sdf* s, const gpmp2mi_scene* sc, int use_base, int use_evidence, int occupied_at,
                      int* d_cells, hipStream_t st) {
  const MapWs w = map_ws_layout((char*)s->map_ws, cells_of(s));
  SensorGrid g{};
  g.dim = s->h.dim; g.nx = s->h.nx; g.ny = s->h.ny; g.nz = s->h.dim == 3 ? s->h.nz : 1;
  g.ox = s->h.ox; g.oy = s->h.oy; g.oz = s->h.dim == 3 ? s->h.oz : 0.0;
  g.cell = s->h.cell;
  mark_stage(s, 0, st);
  if (use_evidence) G2_TRY(evidence_seed(s, occupied_at, use_base, st));
  else G2_TRY(launch_map_seed(cells_of(s), use_base ? w.mask : nullptr, w.wa, w.wb, st));
  G2_TRY(raster(sc, g, w.wa, w.wb, nullptr, st));
  G2_TRY(map_transform(s, w, st));
  if (d_cells)
    G2_HIP(hipMemcpyAsync(d_cells, sc->counts, sc->obj.size() * sizeof(int), hipMemcpyDeviceToDevice, st));
  return GPMP2MI_OK;
}

// what both forms of the update do once the arguments are accepted
int update_ready(gpmp2mi_sdf* s, const gpmp2mi_scene* sc) {
  G2_TRY(map_ready(s, true));
  return scene_ready(sc, s->h.nx, s->h.ny, s->h.dim == 3 ? s->h.nz : 1);
}

}  // namespace

extern "C" {

int gpmp2mi_scene_create(int K, const gpmp2mi_scene_object* objs, gpmp2mi_scene** out) {
  G2_CHECK(objs && out, GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK(K >= 1 && K <= GPMP2MI_MAX_SCENE_OBJECTS, GPMP2MI_ERR_INVALID, "K must be in 1 .. GPMP2MI_MAX_SCENE_OBJECTS");
  for (int k = 0; k < K; k++) G2_TRY(check_object(objs[k]));
  G2_TRY(ensure_device());
  auto sc = std::make_unique<gpmp2mi_scene>();
  G2_HIP(hipGetDevice(&sc->device));
  sc->obj.resize(K);
  size_t off = 0;
  for (int k = 0; k < K; k++) {
    auto& o = sc->obj[k];
    const gpmp2mi_scene_object& in = objs[k];
    o.kind = in.kind;
    o.enabled = in.enabled != 0;
    std::memcpy(o.pose, in.pose, sizeof(o.pose));
    if (in.kind == GPMP2MI_SCENE_MESH) {
      o.V = in.n_vertices;
      o.T = in.n_triangles;
      o.vert_off = off;
      off += ws_round((size_t)o.V * 3 * sizeof(double));
      o.tri_off = off;
      off += ws_round((size_t)o.T * 3 * sizeof(int));
      o.q_off = off;
      off += ws_round((size_t)o.V * 3 * sizeof(int));
    } else {
      for (int n = 0; n < 3; n++) o.s[n] = in.size[n] + in.inflate;
    }
  }
  if (off) G2_TRY(dev_malloc((void**)&sc->geo, off));
  G2_TRY(dev_malloc((void**)&sc->counts, 2 * (size_t)K * sizeof(int)));
  for (int k = 0; k < K; k++) {
    const auto& o = sc->obj[k];
    if (o.kind != GPMP2MI_SCENE_MESH) continue;
    G2_HIP(hipMemcpy(sc->geo + o.vert_off, objs[k].vertices, (size_t)o.V * 3 * sizeof(double), hipMemcpyHostToDevice));
    G2_HIP(hipMemcpy(sc->geo + o.tri_off, objs[k].triangles, (size_t)o.T * 3 * sizeof(int), hipMemcpyHostToDevice));
  }
  *out = sc.release();
  return GPMP2MI_OK;
}

void gpmp2mi_scene_destroy(gpmp2mi_scene* sc) { delete sc; }

int gpmp2mi_scene_count(const gpmp2mi_scene* sc) { return sc ? (int)sc->obj.size() : -1; }

int gpmp2mi_scene_set_poses(gpmp2mi_scene* sc, int first, int count, const double* poses) {
  G2_TRY(check_range(sc, first, count, poses, "null poses with count > 0"));
  for (int k = 0; k < count; k++) G2_TRY(check_pose(poses + 12 * (size_t)k));
  for (int k = 0; k < count; k++) std::memcpy(sc->obj[first + k].pose, poses + 12 * (size_t)k, 12 * sizeof(double));
  return GPMP2MI_OK;
}

int gpmp2mi_scene_set_enabled(gpmp2mi_scene* sc, int first, int count, const int* enabled) {
  G2_TRY(check_range(sc, first, count, enabled, "null enabled with count > 0"));
  for (int k = 0; k < count; k++) sc->obj[first + k].enabled = enabled[k] != 0;
  return GPMP2MI_OK;
}

int gpmp2mi_scene_reserve(gpmp2mi_scene* sc, int nx, int ny, int nz) {
  G2_CHECK(sc, GPMP2MI_ERR_INVALID, "null scene handle");
  G2_CHECK(nx >= 1 && ny >= 1 && nz >= 1, GPMP2MI_ERR_INVALID, "the grid sizes nx, ny, nz must be >= 1");
  return scene_ready(sc, nx, ny, nz);
}

int gpmp2mi_scene_rasterize(const gpmp2mi_scene* sc, int dim, const double origin[3], double cell_size, int nx, int ny,
                            int nz, unsigned char* mask, int* cells) {
  G2_TRY(check_rasterize_args(sc, dim, origin, cell_size, nx, ny, nz, mask));
  G2_TRY(scene_ready(sc, nx, ny, nz));
  DevBuf<unsigned char> d_mask;
  G2_TRY(d_mask.out(mask, (size_t)nx * ny * nz));
  G2_TRY(rasterize(sc, dim, origin, cell_size, nx, ny, nz, d_mask.p, nullptr, nullptr));
  G2_TRY(fetch_all(d_mask));
  if (cells) G2_HIP(hipMemcpy(cells, sc->counts, sc->obj.size() * sizeof(int), hipMemcpyDeviceToHost));
  return GPMP2MI_OK;
}

int gpmp2mi_scene_rasterize_dev(const gpmp2mi_scene* sc, int dim, const double origin[3], double cell_size, int nx,
                                int ny, int nz, unsigned char* mask, int* cells, void* stream) {
  G2_TRY(check_rasterize_args(sc, dim, origin, cell_size, nx, ny, nz, mask));
  G2_TRY(scene_ready(sc, nx, ny, nz));
  return rasterize(sc, dim, origin, cell_size, nx, ny, nz, mask, cells, (hipStream_t)stream);
}

int gpmp2mi_sdf_update_from_scene(gpmp2mi_sdf* s, const gpmp2mi_scene* sc, int use_base, int use_evidence,
                                  int occupied_at, int* cells) {
  G2_TRY(check_update_args(s, sc, use_base, use_evidence, occupied_at));
  G2_TRY(update_ready(s, sc));
  G2_TRY(update_from_scene(s, sc, use_base, use_evidence, occupied_at, nullptr, nullptr));
  G2_HIP(hipStreamSynchronize(nullptr));
  if (cells) G2_HIP(hipMemcpy(cells, sc->counts, sc->obj.size() * sizeof(int), hipMemcpyDeviceToHost));
  return GPMP2MI_OK;
}

int gpmp2mi_sdf_update_from_scene_dev(gpmp2mi_sdf* s, const gpmp2mi_scene* sc, int use_base, int use_evidence,
                                      int occupied_at, int* cells, void* stream) {
  G2_TRY(check_update_args(s, sc, use_base, use_evidence, occupied_at));
  G2_TRY(update_ready(s, sc));
  return update_from_scene(s, sc, use_base, use_evidence, occupied_at, cells, (hipStream_t)stream);
}

int gpmp2mi_debug_scene_timing(gpmp2mi_scene* sc, int on, double* ms2) {
  G2_CHECK(sc, GPMP2MI_ERR_INVALID, "null scene handle");
  if (ms2) {
    G2_CHECK(sc->timing, GPMP2MI_ERR_INVALID, "stage timing is not switched on for this scene");
    G2_HIP(hipEventSynchronize(sc->ev[2]));
    for (int k = 0; k < 2; k++) {
      float ms = 0.0f;
      G2_HIP(hipEventElapsedTime(&ms, sc->ev[k], sc->ev[k + 1]));
      ms2[k] = ms;
    }
  }
  if (on && !sc->ev[0])
    for (hipEvent_t& e : sc->ev) G2_HIP(hipEventCreate(&e));
  sc->timing = on != 0;
  return GPMP2MI_OK;
}

}  // extern "C"
