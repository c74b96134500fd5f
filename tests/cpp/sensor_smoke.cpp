// Builds against include/gpmp2mi_planner.hpp with plain g++ and links the product library.  A field needs the GPU:
// without one the constructor must throw (no silent fallback); with one a free 10^3 field takes a frame of nine rays that
// end on a 3 x 3 plate (the distance at the plate's centre changes sign), then two frames that pass through the plate and
// end behind it (the plate is carved away again), then a depth image after the evidence was reset.
#include <cstdio>

#include "gpmp2mi_planner.hpp"

using namespace gpmp2mi;

static Vector plate(double x) {
  Vector pts;
  for (double y : {0.4, 0.5, 0.6})
    for (double z : {0.4, 0.5, 0.6})
      for (double v : {x, y, z}) pts.push_back(v);
  return pts;
}

int main() {
  try {
    const std::size_t n = 10;
    const double cell = 0.1;
    SignedDistanceField sdf({0.0, 0.0, 0.0}, cell, n, n, n, Vector(n * n * n, 0.5));
    const std::array<double, 3> q{0.7, 0.5, 0.5};   // the centre of the plate's middle cell (7, 5, 5)
    const Vector sensor{0.0, 0.5, 0.5};
    double before = 0.0, hit = 0.0, after = 0.0;
    if (!sdf.getSignedDistance(q, before)) return 10;
    EvidenceOptions opts;
    if (opts.hit != 2 || opts.miss != 1 || opts.lo != -4 || opts.hi != 8 || opts.occupied_at != 1 || opts.use_base != 0 ||
        opts.refresh != 1)
      return 11;
    bool threw = false;
    try {
      EvidenceOptions with_base;
      with_base.use_base = 1;
      sdf.integratePoints(plate(0.7), sensor, with_base);   // no base yet
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (!threw) return 12;
    EvidenceStats st = sdf.integratePoints(plate(0.7), sensor);
    if (st.hit != 9 || st.invalid != 0 || st.max_range != 0 || st.self != 0 || st.outside != 0 || st.occupied != 9) return 13;
    if (!sdf.getSignedDistance(q, hit)) return 14;
    int twos = 0, negative = 0;
    for (int16_t e : sdf.evidence()) {
      twos += e == 2;
      negative += e < 0;
    }
    if (twos != 9 || negative == 0) return 15;
    for (int frame = 0; frame < 2; frame++) st = sdf.integratePoints(plate(0.9), sensor);   // through the plate: 2 -> 1 -> 0
    if (st.hit != 9 || st.occupied != 9) return 16;
    if (!sdf.getSignedDistance(q, after)) return 17;
    std::printf("CARVED before=%.3f hit=%.3f after=%.3f occupied=%d\n", before, hit, after, st.occupied);
    if (!(before > 0.0) || !(hit < 0.0) || !(after > 0.0)) return 18;
    // a depth image: a camera at the middle of the z = 0 face looking along +z, a wall 0.7 m away
    sdf.resetEvidence();
    DepthCamera cam{};
    cam.width = cam.height = 3;
    cam.fx = cam.fy = 10.0;
    cam.cx = cam.cy = 1.0;
    cam.depth_min = 0.05;
    cam.depth_max = 2.0;
    const double pose[12] = {1, 0, 0, 0.5, 0, 1, 0, 0.5, 0, 0, 1, 0.0};
    for (int i = 0; i < 12; i++) cam.pose[i] = pose[i];
    std::vector<float> depth(9, 0.7f);
    depth[4] = 5.0f;   // beyond depth_max: carves, marks nothing
    st = sdf.integrateDepth(cam, depth);
    if (st.hit != 8 || st.max_range != 1 || st.occupied != 8) return 19;
    EvidenceOptions quiet;
    quiet.refresh = 0;
    st = sdf.integrateDepth(cam, depth, quiet);
    double unchanged = 0.0, again = 0.0;
    if (!sdf.getSignedDistance(q, unchanged)) return 20;
    sdf.refreshFromEvidence(5);   // nothing has reached 5 yet: the empty map
    if (!sdf.getSignedDistance(q, again) || again != 1000.0) return 21;
    std::printf("OK depth hit=%d max_range=%d occupied=%d\n", st.hit, st.max_range, st.occupied);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
