// map.hip -- live map (include/gpmp2mi.h "live map"): a field handle's voxels rewritten in place from a field, an
// occupancy grid or a point cloud.  The geometry and the addresses of `plain` and `cells` stay, so every plan bound to
// the handle reads the new map in the calls that follow in stream order.  Kernels: map_kernels.hip for the seeds and the
// point classification; the axis passes, the finish (sdf_kernels.hip) and the pack (factor_kernels.hip) are the ones the
// constructors run.  The multi plan's refresh of its replicas is in multi_plan.hip.
#include <cmath>

#include "host.h"

using namespace g2;

// shared with the sensor map (sensor.hip), declared in host.h: the workspace, the stage marks and the transform
namespace g2 {

MapWs map_ws_layout(char* base, size_t n) {
  MapWs w{};
  Carver take{base};
  w.wa = (int*)take(n * sizeof(int));
  w.wb = (int*)take(n * sizeof(int));
  w.mask = (unsigned char*)take(n);
  w.cen = (double*)take((size_t)MAXS * 3 * sizeof(double));
  w.cnt = (int*)take(4 * sizeof(int));
  w.bytes = take.off;
  return w;
}
// what every update does once its arguments are accepted: a device, the handle's device current, the workspace
int map_ready(gpmp2mi_sdf* s, bool transform) {
  G2_TRY(ensure_device());
  int cur = -1;
  G2_HIP(hipGetDevice(&cur));
  G2_CHECK(cur == s->device, GPMP2MI_ERR_INVALID, "the field handle lives on another device than the current one");
  if (transform) G2_TRY(edt_check_axes(s->h.nx, s->h.ny, s->h.nz));
  if (!s->map_ws) G2_TRY(dev_malloc(&s->map_ws, map_ws_layout(nullptr, cells_of(s)).bytes));
  return GPMP2MI_OK;
}

static int check_layout(int layout) {
  G2_CHECK(layout == GPMP2MI_SDF_LAYOUT_ZYX || layout == GPMP2MI_SDF_LAYOUT_GTSAM, GPMP2MI_ERR_INVALID,
           "unknown voxel layout");
  return GPMP2MI_OK;
}

void mark_stage(gpmp2mi_sdf* s, int k, hipStream_t st) {
  if (s->map_timing) (void)hipEventRecord(s->map_ev[k], st);
}

// the two seeded volumes -> plain -> cells on `st`
int map_transform(gpmp2mi_sdf* s, const MapWs& w, hipStream_t st) {
  mark_stage(s, 1, st);
  G2_TRY(launch_edt_passes(s->h.nx, s->h.ny, s->h.nz, w.wa, w.wb, st));
  mark_stage(s, 2, st);
  G2_TRY(launch_edt_finish(cells_of(s), w.wa, w.wb, s->h.cell, s->plain, st));
  mark_stage(s, 3, st);
  G2_TRY(launch_sdf_pack(s->h, s->cells, st));
  mark_stage(s, 4, st);
  return GPMP2MI_OK;
}

}  // namespace g2

namespace {

int update_from_occupancy(gpmp2mi_sdf* s, const double* d_occ, hipStream_t st) {
  const MapWs w = map_ws_layout((char*)s->map_ws, cells_of(s));
  mark_stage(s, 0, st);
  G2_TRY(launch_map_seed_occ(cells_of(s), d_occ, w.wa, w.wb, w.mask, st));
  s->has_base = true;
  return map_transform(s, w, st);
}

// the argument rules of the point forms that need no look at a handle, then those that do
int check_points_args(const gpmp2mi_sdf* s, int M, const double* points, int use_base, const gpmp2mi_robot* robot,
                      const double* conf, double margin) {
  G2_CHECK(s, GPMP2MI_ERR_INVALID, "null field handle");
  G2_CHECK(M >= 0, GPMP2MI_ERR_INVALID, "M must be >= 0");
  G2_CHECK(M == 0 || points, GPMP2MI_ERR_INVALID, "null points with M > 0");
  G2_CHECK(!std::isnan(margin), GPMP2MI_ERR_INVALID, "margin is NaN");
  G2_CHECK(!robot || conf, GPMP2MI_ERR_INVALID, "a robot for the self filter, but a null conf");
  G2_CHECK(!use_base || s->has_base, GPMP2MI_ERR_INVALID,
           "use_base on a handle without a base: call gpmp2mi_sdf_update_from_occupancy first");
  G2_CHECK(!robot || robot->device == s->device, GPMP2MI_ERR_INVALID, "the robot handle lives on another device than the field");
  return GPMP2MI_OK;
}

// points, conf, stats: device pointers (stats may be null); everything on `st`, no host synchronisation
int update_from_points(gpmp2mi_sdf* s, int M, const double* d_points, int use_base, const gpmp2mi_robot* robot,
                       const double* d_conf, double margin, int* d_stats, hipStream_t st) {
  const MapWs w = map_ws_layout((char*)s->map_ws, cells_of(s));
  const SdfDev& g = s->h;
  mark_stage(s, 0, st);
  G2_HIP(hipMemsetAsync(w.cnt, 0, 4 * sizeof(int), st));
  if (robot && M > 0) G2_TRY(launch_sphere_centers(robot->h, robot->d, 1, d_conf, w.cen, nullptr, st));
  G2_TRY(launch_map_seed(cells_of(s), use_base ? w.mask : nullptr, w.wa, w.wb, st));
  MapMark a{};
  a.dim = g.dim; a.nx = g.nx; a.ny = g.ny; a.nz = g.nz;
  a.M = M;
  a.S = robot ? robot->h.nr_spheres : 0;
  a.ox = g.ox; a.oy = g.oy; a.oz = g.oz; a.cell = g.cell;
  a.margin = margin;
  a.pts = d_points;
  a.R = robot ? robot->d : nullptr;
  a.cen = w.cen;
  a.wa = w.wa; a.wb = w.wb;
  a.cnt = w.cnt;
  G2_TRY(launch_map_mark(a, st));
  G2_TRY(map_transform(s, w, st));
  if (d_stats) G2_HIP(hipMemcpyAsync(d_stats, w.cnt, 4 * sizeof(int), hipMemcpyDeviceToDevice, st));
  return GPMP2MI_OK;
}

}  // namespace

extern "C" {

int gpmp2mi_sdf_reserve_update(gpmp2mi_sdf* s) {
  G2_CHECK(s, GPMP2MI_ERR_INVALID, "null field handle");
  return map_ready(s, false);
}

int gpmp2mi_sdf_update(gpmp2mi_sdf* s, const double* voxels, int layout) {
  G2_CHECK(s && voxels, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_layout(layout));
  G2_TRY(map_ready(s, false));
  std::vector<double> tmp;
  const double* src = to_zyx(voxels, layout, s->h.nx, s->h.ny, s->h.nz, tmp);
  G2_HIP(hipMemcpy(s->plain, src, cells_of(s) * sizeof(double), hipMemcpyHostToDevice));
  s->has_base = false;
  G2_TRY(launch_sdf_pack(s->h, s->cells, nullptr));
  G2_HIP(hipStreamSynchronize(nullptr));
  return GPMP2MI_OK;
}

int gpmp2mi_sdf_update_dev(gpmp2mi_sdf* s, const double* voxels_zyx, void* stream) {
  G2_CHECK(s && voxels_zyx, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(map_ready(s, false));
  hipStream_t st = (hipStream_t)stream;
  G2_HIP(hipMemcpyAsync(s->plain, voxels_zyx, cells_of(s) * sizeof(double), hipMemcpyDeviceToDevice, st));
  s->has_base = false;
  return launch_sdf_pack(s->h, s->cells, st);
}

int gpmp2mi_sdf_update_from_occupancy(gpmp2mi_sdf* s, const double* occ, int layout) {
  G2_CHECK(s && occ, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_layout(layout));
  G2_TRY(map_ready(s, true));
  std::vector<double> tmp;
  DevBuf<double> d_occ;
  G2_TRY(d_occ.upload(to_zyx(occ, layout, s->h.nx, s->h.ny, s->h.nz, tmp), cells_of(s)));
  G2_TRY(update_from_occupancy(s, d_occ.p, nullptr));
  G2_HIP(hipStreamSynchronize(nullptr));
  return GPMP2MI_OK;
}

int gpmp2mi_sdf_update_from_occupancy_dev(gpmp2mi_sdf* s, const double* occ_zyx, void* stream) {
  G2_CHECK(s && occ_zyx, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(map_ready(s, true));
  return update_from_occupancy(s, occ_zyx, (hipStream_t)stream);
}

int gpmp2mi_sdf_update_from_points(gpmp2mi_sdf* s, int M, const double* points, int use_base, const gpmp2mi_robot* robot,
                                   const double* conf, double margin, int* stats) {
  G2_TRY(check_points_args(s, M, points, use_base, robot, conf, margin));
  G2_TRY(map_ready(s, true));
  DevBuf<double> d_pts, d_conf;
  G2_TRY(d_pts.upload(points, (size_t)M * s->h.dim));
  if (robot) G2_TRY(d_conf.upload(conf, robot->h.dof));
  G2_TRY(update_from_points(s, M, d_pts.p, use_base, robot, d_conf.p, margin, nullptr, nullptr));
  G2_HIP(hipStreamSynchronize(nullptr));
  if (stats)
    G2_HIP(hipMemcpy(stats, map_ws_layout((char*)s->map_ws, cells_of(s)).cnt, 4 * sizeof(int), hipMemcpyDeviceToHost));
  return GPMP2MI_OK;
}

int gpmp2mi_sdf_update_from_points_dev(gpmp2mi_sdf* s, int M, const double* points, int use_base,
                                       const gpmp2mi_robot* robot, const double* conf, double margin, int* stats,
                                       void* stream) {
  G2_TRY(check_points_args(s, M, points, use_base, robot, conf, margin));
  G2_TRY(map_ready(s, true));
  return update_from_points(s, M, points, use_base, robot, conf, margin, stats, (hipStream_t)stream);
}

int gpmp2mi_debug_sdf_update_timing(gpmp2mi_sdf* s, int on, double* ms4) {
  G2_CHECK(s, GPMP2MI_ERR_INVALID, "null field handle");
  if (ms4) {
    G2_CHECK(s->map_timing, GPMP2MI_ERR_INVALID, "stage timing is not switched on for this handle");
    G2_HIP(hipEventSynchronize(s->map_ev[4]));
    for (int k = 0; k < 4; k++) {
      float ms = 0.0f;
      G2_HIP(hipEventElapsedTime(&ms, s->map_ev[k], s->map_ev[k + 1]));
      ms4[k] = ms;
    }
  }
  if (on && !s->map_ev[0])
    for (hipEvent_t& e : s->map_ev) G2_HIP(hipEventCreate(&e));
  s->map_timing = on != 0;
  return GPMP2MI_OK;
}

}  // extern "C"
