// sensor.hip -- sensor map (include/gpmp2mi.h "sensor map"): an int16 evidence value per cell kept on a field handle,
// raised where the rays of a frame end and lowered where they pass, and the field rebuilt from it in place.  Kernels:
// sensor_kernels.hip for the rays, the walk and the apply-and-seed pass; the transform behind the seeds is map.hip's
// (map_transform), so the field is what the occupancy constructor gives for the same obstacle set.
#include <climits>
#include <cmath>
#include <cstring>

#include "host.h"

using namespace g2;

namespace {

// the handle's evidence workspace for n cells
struct EvWs {
  short* E;                    // [n]
  unsigned char *miss, *hit;   // [n] each: the marks of the call in flight, all 0 between two calls
  int* cnt;                    // [6] hit, invalid, max_range, self, outside; cells with E >= occupied_at
  size_t bytes;
};
EvWs ev_ws_layout(char* base, size_t n) {
  EvWs w{};
  Carver take{base};
  w.E = (short*)take(n * sizeof(short));
  w.miss = (unsigned char*)take(n);
  w.hit = (unsigned char*)take(n);
  w.cnt = (int*)take(6 * sizeof(int));
  w.bytes = take.off;
  return w;
}
size_t ray_bytes(int M) { return ws_round((size_t)M * 3 * sizeof(double)) + ws_round((size_t)M * sizeof(int)); }

// once the arguments are accepted: the live map's workspace (the rebuild runs in it), the evidence all 0, M ray records
int evidence_ready(gpmp2mi_sdf* s, int M) {
  G2_TRY(map_ready(s, true));
  if (!s->ev_ws) {
    const size_t bytes = ev_ws_layout(nullptr, cells_of(s)).bytes;
    G2_TRY(dev_malloc(&s->ev_ws, bytes));
    G2_HIP(hipMemsetAsync(s->ev_ws, 0, bytes, nullptr));
    G2_HIP(hipStreamSynchronize(nullptr));   // the first `_dev` call may come on any stream
  }
  if (M > 0) G2_TRY(s->ray_ws.reserve(ray_bytes(M)));
  return GPMP2MI_OK;
}

int check_opts(const gpmp2mi_evidence_opts* o) {
  G2_CHECK(o, GPMP2MI_ERR_INVALID, "null opts");
  G2_CHECK(o->hit >= 0 && o->hit <= 65535, GPMP2MI_ERR_INVALID, "opts.hit must be in 0 .. 65535");
  G2_CHECK(o->miss >= 0 && o->miss <= 65535, GPMP2MI_ERR_INVALID, "opts.miss must be in 0 .. 65535");
  G2_CHECK(o->lo >= -32768 && o->lo <= 0, GPMP2MI_ERR_INVALID, "opts.lo must be in -32768 .. 0");
  G2_CHECK(o->hi >= 0 && o->hi <= 32767, GPMP2MI_ERR_INVALID, "opts.hi must be in 0 .. 32767");
  G2_CHECK(o->occupied_at > o->lo && o->occupied_at <= o->hi, GPMP2MI_ERR_INVALID,
           "opts.occupied_at must be in lo + 1 .. hi");
  return GPMP2MI_OK;
}

// the argument rules that need no look at a handle, then (check_handle) those that do
int check_common(const gpmp2mi_sdf* s, const gpmp2mi_robot* robot, const double* conf, double margin,
                 const gpmp2mi_evidence_opts* opts) {
  G2_CHECK(s, GPMP2MI_ERR_INVALID, "null field handle");
  G2_TRY(check_opts(opts));
  G2_CHECK(!std::isnan(margin), GPMP2MI_ERR_INVALID, "margin is NaN");
  G2_CHECK(!robot || conf, GPMP2MI_ERR_INVALID, "a robot for the self filter, but a null conf");
  return GPMP2MI_OK;
}
int check_handle(const gpmp2mi_sdf* s, int use_base, const gpmp2mi_robot* robot) {
  G2_CHECK(!use_base || s->has_base, GPMP2MI_ERR_INVALID,
           "use_base on a handle without a base: call gpmp2mi_sdf_update_from_occupancy first");
  G2_CHECK(!robot || robot->device == s->device, GPMP2MI_ERR_INVALID,
           "the robot handle lives on another device than the field");
  return GPMP2MI_OK;
}

int check_points_args(const gpmp2mi_sdf* s, int M, const double* points, const double* origin,
                      const gpmp2mi_robot* robot, const double* conf, double margin,
                      const gpmp2mi_evidence_opts* opts) {
  G2_TRY(check_common(s, robot, conf, margin, opts));
  G2_CHECK(M >= 0, GPMP2MI_ERR_INVALID, "M must be >= 0");
  G2_CHECK(M == 0 || points, GPMP2MI_ERR_INVALID, "null points with M > 0");
  G2_CHECK(origin, GPMP2MI_ERR_INVALID, "null sensor_origin");
  for (int k = 0; k < s->h.dim; k++)
    G2_CHECK(std::isfinite(origin[k]), GPMP2MI_ERR_INVALID, "sensor_origin is not finite");
  return check_handle(s, opts->use_base, robot);
}

int check_depth_args(const gpmp2mi_sdf* s, const gpmp2mi_depth_camera* cam, const float* depth,
                     const gpmp2mi_robot* robot, const double* conf, double margin, const gpmp2mi_evidence_opts* opts) {
  G2_TRY(check_common(s, robot, conf, margin, opts));
  G2_CHECK(cam, GPMP2MI_ERR_INVALID, "null camera");
  G2_CHECK(cam->width >= 0 && cam->height >= 0, GPMP2MI_ERR_INVALID, "camera width and height must be >= 0");
  G2_CHECK((long long)cam->width * cam->height <= INT_MAX, GPMP2MI_ERR_INVALID, "camera width * height exceeds INT_MAX");
  G2_CHECK(cam->width * cam->height == 0 || depth, GPMP2MI_ERR_INVALID, "null depth with width * height > 0");
  G2_CHECK(std::isfinite(cam->fx) && std::isfinite(cam->fy) && std::isfinite(cam->cx) && std::isfinite(cam->cy),
           GPMP2MI_ERR_INVALID, "camera intrinsics fx, fy, cx, cy must be finite");
  G2_CHECK(cam->fx != 0.0 && cam->fy != 0.0, GPMP2MI_ERR_INVALID, "camera fx and fy must not be 0");
  G2_CHECK(std::isfinite(cam->depth_min) && std::isfinite(cam->depth_max) && cam->depth_min >= 0.0 &&
               cam->depth_min < cam->depth_max,
           GPMP2MI_ERR_INVALID, "camera depth range must be 0 <= depth_min < depth_max, both finite");
  for (double v : cam->pose) G2_CHECK(std::isfinite(v), GPMP2MI_ERR_INVALID, "camera pose is not finite");
  G2_CHECK(s->h.dim == 3, GPMP2MI_ERR_INVALID, "the depth form needs a 3-D field handle");
  return check_handle(s, opts->use_base, robot);
}

SensorGrid grid_of(const gpmp2mi_sdf* s) {
  const SdfDev& g = s->h;
  SensorGrid q{};
  q.dim = g.dim; q.nx = g.nx; q.ny = g.ny; q.nz = g.dim == 3 ? g.nz : 1;
  q.ox = g.ox; q.oy = g.oy; q.oz = g.oz; q.cell = g.cell;
  return q;
}

void mark_sensor(gpmp2mi_sdf* s, int k, hipStream_t st) {
  if (s->map_timing && s->sensor_ev[0]) (void)hipEventRecord(s->sensor_ev[k], st);
}

// marks -> evidence, the occupied count, and (seed) the two seeded volumes
int apply_and_seed(gpmp2mi_sdf* s, const EvWs& e, const MapWs& w, int hit, int miss, int lo, int hi, int occupied_at,
                   int use_base, bool seed, hipStream_t st) {
  SensorApply a{};
  a.n = cells_of(s);
  a.hit = hit; a.miss = miss; a.lo = lo; a.hi = hi; a.occupied_at = occupied_at;
  a.E = e.E;
  a.miss_marks = e.miss; a.hit_marks = e.hit;
  a.mask = use_base ? w.mask : nullptr;
  a.wa = seed ? w.wa : nullptr;
  a.wb = seed ? w.wb : nullptr;
  a.cnt = e.cnt + 5;
  return launch_sensor_apply(a, st);
}

// the same, and (refresh) the transform behind the seeds
int apply_and_refresh(gpmp2mi_sdf* s, const EvWs& e, int hit, int miss, int lo, int hi, int occupied_at, int use_base,
                      bool refresh, hipStream_t st) {
  const MapWs w = map_ws_layout((char*)s->map_ws, cells_of(s));
  G2_TRY(apply_and_seed(s, e, w, hit, miss, lo, hi, occupied_at, use_base, refresh, st));
  return refresh ? map_transform(s, w, st) : GPMP2MI_OK;
}

// d_points or d_depth (with cam), d_conf, d_stats: device pointers; everything on `st`, no host synchronisation
int integrate(gpmp2mi_sdf* s, int M, const double* d_points, const float* d_depth, const gpmp2mi_depth_camera* cam,
              const double* origin, const gpmp2mi_robot* robot, const double* d_conf, double margin,
              const gpmp2mi_evidence_opts& o, int* d_stats, hipStream_t st) {
  const size_t n = cells_of(s);
  const EvWs e = ev_ws_layout((char*)s->ev_ws, n);
  const MapWs w = map_ws_layout((char*)s->map_ws, n);
  double* rb = (double*)s->ray_ws.p;
  int* rcls = (int*)((char*)s->ray_ws.p + ws_round((size_t)M * 3 * sizeof(double)));
  mark_stage(s, 0, st);
  mark_sensor(s, 0, st);
  G2_HIP(hipMemsetAsync(e.cnt, 0, 6 * sizeof(int), st));
  if (robot && M > 0) G2_TRY(launch_sphere_centers(robot->h, robot->d, 1, d_conf, w.cen, nullptr, st));
  SensorRays r{};
  r.g = grid_of(s);
  r.M = M;
  r.S = robot ? robot->h.nr_spheres : 0;
  for (int k = 0; k < 3; k++) r.o[k] = k < r.g.dim ? origin[k] : 0.0;
  r.margin = margin;
  r.pts = d_points;
  r.depth = d_depth;
  if (cam) {
    r.width = cam->width;
    r.fx = cam->fx; r.fy = cam->fy; r.cx = cam->cx; r.cy = cam->cy;
    r.depth_min = cam->depth_min; r.depth_max = cam->depth_max;
    std::memcpy(r.pose, cam->pose, sizeof(r.pose));
  }
  r.R = robot ? robot->d : nullptr;
  r.cen = w.cen;
  r.rb = rb; r.rcls = rcls;
  r.cnt = e.cnt;
  G2_TRY(launch_sensor_rays(r, st));
  mark_sensor(s, 1, st);
  SensorWalk k{};
  k.g = r.g;
  k.M = M;
  for (int a = 0; a < 3; a++) k.o[a] = r.o[a];
  k.rb = rb; k.rcls = rcls;
  k.miss = e.miss; k.hit = e.hit;
  G2_TRY(launch_sensor_walk(k, st));
  mark_sensor(s, 2, st);
  G2_TRY(apply_and_refresh(s, e, o.hit, o.miss, o.lo, o.hi, o.occupied_at, o.use_base, o.refresh != 0, st));
  if (d_stats) G2_HIP(hipMemcpyAsync(d_stats, e.cnt, 6 * sizeof(int), hipMemcpyDeviceToDevice, st));
  return GPMP2MI_OK;
}

// the closing step of a host form: wait, then the six counts
int finish_host(gpmp2mi_sdf* s, int* stats) {
  G2_HIP(hipStreamSynchronize(nullptr));
  if (stats)
    G2_HIP(hipMemcpy(stats, ev_ws_layout((char*)s->ev_ws, cells_of(s)).cnt, 6 * sizeof(int), hipMemcpyDeviceToHost));
  return GPMP2MI_OK;
}

int check_refresh_args(const gpmp2mi_sdf* s, int occupied_at, int use_base) {
  G2_CHECK(s, GPMP2MI_ERR_INVALID, "null field handle");
  G2_CHECK(occupied_at >= -32768 && occupied_at <= 32767, GPMP2MI_ERR_INVALID, "occupied_at must be in -32768 .. 32767");
  return check_handle(s, use_base, nullptr);
}

int refresh_from_evidence(gpmp2mi_sdf* s, int occupied_at, int use_base, hipStream_t st) {
  const EvWs e = ev_ws_layout((char*)s->ev_ws, cells_of(s));
  mark_stage(s, 0, st);
  G2_HIP(hipMemsetAsync(e.cnt + 5, 0, sizeof(int), st));
  // no marks are set between two calls: E stays as it is, only the seeds are written
  return apply_and_refresh(s, e, 0, 0, -32768, 32767, occupied_at, use_base, true, st);
}

}  // namespace

namespace g2 {
// for scene.hip: the seeds of {E >= occupied_at} (and the base) without the transform.  No marks are set between two
// calls, so E stays as it is; only the count of occupied cells (stats entry 5 of a later call is zeroed first) moves.
int evidence_seed(gpmp2mi_sdf* s, int occupied_at, int use_base, hipStream_t st) {
  const EvWs e = ev_ws_layout((char*)s->ev_ws, cells_of(s));
  const MapWs w = map_ws_layout((char*)s->map_ws, cells_of(s));
  G2_HIP(hipMemsetAsync(e.cnt + 5, 0, sizeof(int), st));
  return apply_and_seed(s, e, w, 0, 0, -32768, 32767, occupied_at, use_base, true, st);
}
}  // namespace g2

extern "C" {

void gpmp2mi_evidence_opts_default(gpmp2mi_evidence_opts* o) {
  if (!o) return;
  o->hit = 2;
  o->miss = 1;
  o->lo = -4;
  o->hi = 8;
  o->occupied_at = 1;
  o->use_base = 0;
  o->refresh = 1;
}

int gpmp2mi_sdf_reserve_evidence(gpmp2mi_sdf* s) {
  G2_CHECK(s, GPMP2MI_ERR_INVALID, "null field handle");
  return evidence_ready(s, 0);
}

int gpmp2mi_sdf_integrate_points(gpmp2mi_sdf* s, int M, const double* points, const double* sensor_origin,
                                 const gpmp2mi_robot* robot, const double* conf, double margin,
                                 const gpmp2mi_evidence_opts* opts, int* stats) {
  G2_TRY(check_points_args(s, M, points, sensor_origin, robot, conf, margin, opts));
  G2_TRY(evidence_ready(s, M));
  DevBuf<double> d_pts, d_conf;
  G2_TRY(d_pts.upload(points, (size_t)M * s->h.dim));
  if (robot) G2_TRY(d_conf.upload(conf, robot->h.dof));
  G2_TRY(integrate(s, M, d_pts.p, nullptr, nullptr, sensor_origin, robot, d_conf.p, margin, *opts, nullptr, nullptr));
  return finish_host(s, stats);
}

int gpmp2mi_sdf_integrate_points_dev(gpmp2mi_sdf* s, int M, const double* points, const double* sensor_origin,
                                     const gpmp2mi_robot* robot, const double* conf, double margin,
                                     const gpmp2mi_evidence_opts* opts, int* stats, void* stream) {
  G2_TRY(check_points_args(s, M, points, sensor_origin, robot, conf, margin, opts));
  G2_TRY(evidence_ready(s, M));
  return integrate(s, M, points, nullptr, nullptr, sensor_origin, robot, conf, margin, *opts, stats, (hipStream_t)stream);
}

int gpmp2mi_sdf_integrate_depth(gpmp2mi_sdf* s, const gpmp2mi_depth_camera* cam, const float* depth,
                                const gpmp2mi_robot* robot, const double* conf, double margin,
                                const gpmp2mi_evidence_opts* opts, int* stats) {
  G2_TRY(check_depth_args(s, cam, depth, robot, conf, margin, opts));
  const int M = cam->width * cam->height;
  G2_TRY(evidence_ready(s, M));
  DevBuf<float> d_depth;
  DevBuf<double> d_conf;
  G2_TRY(d_depth.upload(depth, (size_t)M));
  if (robot) G2_TRY(d_conf.upload(conf, robot->h.dof));
  const double origin[3] = {cam->pose[3], cam->pose[7], cam->pose[11]};
  G2_TRY(integrate(s, M, nullptr, d_depth.p, cam, origin, robot, d_conf.p, margin, *opts, nullptr, nullptr));
  return finish_host(s, stats);
}

int gpmp2mi_sdf_integrate_depth_dev(gpmp2mi_sdf* s, const gpmp2mi_depth_camera* cam, const float* depth,
                                    const gpmp2mi_robot* robot, const double* conf, double margin,
                                    const gpmp2mi_evidence_opts* opts, int* stats, void* stream) {
  G2_TRY(check_depth_args(s, cam, depth, robot, conf, margin, opts));
  const int M = cam->width * cam->height;
  G2_TRY(evidence_ready(s, M));
  const double origin[3] = {cam->pose[3], cam->pose[7], cam->pose[11]};
  return integrate(s, M, nullptr, depth, cam, origin, robot, conf, margin, *opts, stats, (hipStream_t)stream);
}

int gpmp2mi_sdf_refresh_from_evidence(gpmp2mi_sdf* s, int occupied_at, int use_base) {
  G2_TRY(check_refresh_args(s, occupied_at, use_base));
  G2_TRY(evidence_ready(s, 0));
  G2_TRY(refresh_from_evidence(s, occupied_at, use_base, nullptr));
  G2_HIP(hipStreamSynchronize(nullptr));
  return GPMP2MI_OK;
}

int gpmp2mi_sdf_refresh_from_evidence_dev(gpmp2mi_sdf* s, int occupied_at, int use_base, void* stream) {
  G2_TRY(check_refresh_args(s, occupied_at, use_base));
  G2_TRY(evidence_ready(s, 0));
  return refresh_from_evidence(s, occupied_at, use_base, (hipStream_t)stream);
}

int gpmp2mi_sdf_evidence_reset(gpmp2mi_sdf* s) {
  G2_TRY(gpmp2mi_sdf_evidence_reset_dev(s, nullptr));
  G2_HIP(hipStreamSynchronize(nullptr));
  return GPMP2MI_OK;
}

int gpmp2mi_sdf_evidence_reset_dev(gpmp2mi_sdf* s, void* stream) {
  G2_CHECK(s, GPMP2MI_ERR_INVALID, "null field handle");
  G2_TRY(evidence_ready(s, 0));
  const size_t n = cells_of(s);
  G2_HIP(hipMemsetAsync(ev_ws_layout((char*)s->ev_ws, n).E, 0, n * sizeof(short), (hipStream_t)stream));
  return GPMP2MI_OK;
}

int gpmp2mi_sdf_get_evidence(const gpmp2mi_sdf* s, int16_t* E) {
  G2_CHECK(s, GPMP2MI_ERR_INVALID, "null field handle");
  G2_CHECK(E, GPMP2MI_ERR_INVALID, "null E");
  const size_t n = cells_of(s);
  if (!s->ev_ws) {   // never allocated: all 0, as it would be
    std::memset(E, 0, n * sizeof(int16_t));
    return GPMP2MI_OK;
  }
  G2_HIP(hipMemcpy(E, ev_ws_layout((char*)s->ev_ws, n).E, n * sizeof(int16_t), hipMemcpyDeviceToHost));
  return GPMP2MI_OK;
}

int gpmp2mi_debug_sdf_integrate_timing(gpmp2mi_sdf* s, int on, double* ms6) {
  G2_CHECK(s, GPMP2MI_ERR_INVALID, "null field handle");
  if (ms6) {
    G2_CHECK(s->map_timing && s->sensor_ev[0], GPMP2MI_ERR_INVALID, "stage timing is not switched on for this handle");
    G2_HIP(hipEventSynchronize(s->map_ev[4]));
    hipEvent_t ev[7] = {s->sensor_ev[0], s->sensor_ev[1], s->sensor_ev[2], s->map_ev[1], s->map_ev[2], s->map_ev[3],
                        s->map_ev[4]};
    for (int k = 0; k < 6; k++) {
      float ms = 0.0f;
      G2_HIP(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
      ms6[k] = ms;
    }
  }
  if (on && !s->sensor_ev[0])
    for (hipEvent_t& e : s->sensor_ev) G2_HIP(hipEventCreate(&e));
  return gpmp2mi_debug_sdf_update_timing(s, on, nullptr);
}

}  // extern "C"
