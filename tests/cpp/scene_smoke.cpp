// Builds against include/gpmp2mi_planner.hpp with plain g++ and links the product library.  A scene needs the GPU:
// without one the first use must throw (no silent fallback); with one a box, a sphere, a cylinder and a closed cube mesh
// are rasterised on a 10^3 grid (known counts), the field is rebuilt from them, the mesh moves and the field follows.
#include <cstdio>

#include "gpmp2mi_planner.hpp"

using namespace gpmp2mi;

int main() {
  try {
    const std::size_t n = 10;
    const double cell = 0.1;
    Scene scene;
    const std::size_t box = scene.addBox({0.15, 0.15, 0.15}, Scene::translation(0.5, 0.5, 0.5));
    const std::size_t sphere = scene.addSphere(0.12, {0.2, 0.2, 0.2});
    const std::size_t cyl = scene.addCylinder(0.12, 0.25, Scene::translation(0.8, 0.2, 0.5));
    // a unit cube scaled to three cells, its corners on cell centres once it is placed at (0.1, 0.6, 0.1)
    Vector v;
    for (int c = 0; c < 8; c++)
      for (int a = 0; a < 3; a++) v.push_back(((c >> a) & 1) ? 0.3 : 0.0);
    const std::vector<int> t{0, 2, 3, 0, 3, 1, 4, 5, 7, 4, 7, 6, 0, 1, 5, 0, 5, 4, 2, 6, 7, 2, 7, 3, 0, 4, 6, 0, 6, 2, 1, 3, 7, 1, 7, 5};
    const std::size_t mesh = scene.addMesh(v, t, Scene::translation(0.1, 0.6, 0.1));
    if (scene.size() != 4 || box != 0 || sphere != 1 || cyl != 2 || mesh != 3) return 10;
    std::vector<int> cells;
    const std::vector<unsigned char> mask = scene.rasterize({0.0, 0.0, 0.0}, cell, n, n, n, &cells);   // throws without a GPU
    int total = 0;
    for (unsigned char m : mask) total += m;
    std::printf("CELLS box=%d sphere=%d cylinder=%d mesh=%d total=%d\n", cells[0], cells[1], cells[2], cells[3], total);
    if (cells[0] != 27 || cells[1] != 7 || cells[2] != 25 || cells[3] != 27 || total != 86) return 11;
    SignedDistanceField sdf({0.0, 0.0, 0.0}, cell, n, n, n, Vector(n * n * n, 0.5));
    const std::array<double, 3> in_box{0.5, 0.5, 0.5}, in_mesh{0.2, 0.7, 0.2}, moved_to{0.2, 0.7, 0.7};
    double d_box = 0.0, d_mesh = 0.0, d_free = 0.0, d_left = 0.0, d_new = 0.0;
    if (sdf.updateFromScene(scene) != cells) return 12;
    if (!sdf.getSignedDistance(in_box, d_box) || !sdf.getSignedDistance(in_mesh, d_mesh) ||
        !sdf.getSignedDistance(moved_to, d_free))
      return 13;
    if (!(d_box < 0.0) || !(d_mesh < 0.0) || !(d_free > 0.0)) return 14;
    scene.setPose(mesh, Scene::translation(0.1, 0.6, 0.6));   // the mesh moves up by five cells
    scene.setEnabled(sphere, false);
    const std::vector<int> after = sdf.updateFromScene(scene);
    if (after[0] != 27 || after[1] != 0 || after[2] != 25 || after[3] != 27) return 15;
    if (!sdf.getSignedDistance(in_mesh, d_left) || !sdf.getSignedDistance(moved_to, d_new)) return 16;
    if (!(d_left > 0.0) || !(d_new < 0.0)) return 17;
    bool threw = false;
    try {
      sdf.updateFromScene(scene, /*use_base=*/true);   // no base on this handle
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (!threw) return 18;
    PlanarSDF planar({0.0, 0.0}, cell, n, n, Vector(n * n, 0.5));
    scene.setPose(mesh, Scene::translation(0.1, 0.6, -0.1));
    const std::vector<int> flat = planar.updateFromScene(scene);   // the scene cut by the plane z = 0: only the cube reaches it
    if (flat[0] != 0 || flat[1] != 0 || flat[2] != 0 || flat[3] != 9) return 19;
    std::printf("OK moved mesh=%d sphere=%d planar=%d,%d,%d,%d\n", after[3], after[1], flat[0], flat[1], flat[2], flat[3]);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
