// Builds against include/gpmp2mi_planner.hpp with plain g++ and links the product library.  A field needs the GPU:
// without one the constructor must throw (no silent fallback); with one a free 10^3 field is updated in place from a
// cloud that fills a 3^3 block of cells, and the distance queried at the block's centre changes sign.
#include <cstdio>

#include "gpmp2mi_planner.hpp"

using namespace gpmp2mi;

int main() {
  try {
    const std::size_t n = 10;
    const double cell = 0.1;
    SignedDistanceField sdf({0.0, 0.0, 0.0}, cell, n, n, n, Vector(n * n * n, 0.5));
    const std::array<double, 3> q{0.5, 0.5, 0.5};   // the centre of cell (5, 5, 5)
    double before = 0.0, after = 0.0, again = 0.0;
    if (!sdf.getSignedDistance(q, before)) return 10;
    Vector cloud;
    for (int z = 4; z <= 6; z++)
      for (int y = 4; y <= 6; y++)
        for (int x = 4; x <= 6; x++)
          for (double v : {x * cell, y * cell, z * cell}) cloud.push_back(v);
    cloud.insert(cloud.end(), {5.0, 0.5, 0.5});   // one point outside the grid
    bool threw = false;
    try {
      sdf.updateFromPoints(cloud, true);   // no base yet
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (!threw) return 11;
    const MapUpdateStats st = sdf.updateFromPoints(cloud, false);
    if (st.kept != 27 || st.outside != 1 || st.non_finite != 0 || st.self != 0) return 12;
    if (!sdf.getSignedDistance(q, after)) return 13;
    std::printf("CHANGED before=%.3f after=%.3f kept=%d outside=%d\n", before, after, st.kept, st.outside);
    if (!(before > 0.0) || !(after < 0.0)) return 14;
    // an empty occupancy grid is the base now; the cloud on top of it gives the same field
    sdf.updateFromOccupancy(Vector(n * n * n, 0.0));
    sdf.updateFromPoints(cloud);
    if (!sdf.getSignedDistance(q, again) || again != after) return 15;
    std::printf("OK after=%.3f\n", again);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
