// Builds against include/gpmp2mi_planner.hpp with plain g++ and links the product library.  Seeds restarts of a 2-link
// problem through the facade (SeedRestarts, BatchTrajOptimizeSeeded, TrajectoryPosteriorSamples, NormalFill) and prints
// (hex floats, exact) what it got for tests/test_cpp_seed.py to compare with the Python binding.  Needs the GPU: without
// one it must throw.
#include <cmath>
#include <cstdio>

#include "gpmp2mi_planner.hpp"

using namespace gpmp2mi;

static void print(const char* tag, std::size_t i, const Vector& v) {
  std::printf("%s %zu", tag, i);
  for (double x : v) std::printf(" %a", x);
  std::printf("\n");
}

int main() {
  try {
    Arm arm(2, {1.0, 1.0}, {0.0, 0.0}, {0.0, 0.0}, Pose3::Translation(0.0, 0.0, 0.0));
    BodySphereVector spheres;
    for (int l = 0; l < 2; l++)
      for (double x : {-0.75, -0.25}) spheres.emplace_back(l, 0.1, std::array<double, 3>{x, 0.0, 0.0});
    ArmModel model(arm, spheres);
    const int cells = 60;
    Vector field(cells * cells);  // distance to a disc of radius 0.4 at (1.2, 1.0); column-major (row = y, col = x)
    for (int x = 0; x < cells; x++)
      for (int y = 0; y < cells; y++)
        field[x * cells + y] = std::hypot(-3.0 + 0.1 * x - 1.2, -3.0 + 0.1 * y - 1.0) - 0.4;
    PlanarSDF sdf({-3.0, -3.0}, 0.1, cells, cells, field);
    const std::size_t N = 10, M = 5;
    const std::uint64_t seed = 77;
    TrajOptimizerSetting setting(2);
    setting.set_total_step(N);
    setting.set_total_time(2.0);
    setting.set_obs_check_inter(2);
    setting.set_cost_sigma(0.1);
    setting.set_epsilon(0.2);
    setting.setGaussNewton();
    const Vector start{0.0, 0.0}, end{1.5, 0.5}, zero{0.0, 0.0};
    const std::vector<Trajectory> init = SeedRestarts(model, sdf, start, end, setting, M, seed, 0.5, true);
    if (init.size() != M) return 10;
    const Trajectory line = initArmTrajStraightLine(start, end, N);
    if (init[0].data != line.data) return 11;          // keep_first: restart 0 is the straight line, bit for bit
    if (init[1].data == line.data) return 12;
    const SeededRestarts res = BatchTrajOptimizeSeeded(model, sdf, start, zero, end, zero, setting, M, 2, seed, 0.5, true, true);
    if (res.traj.size() != M || res.init.size() != M || res.iterations.size() != M) return 13;
    for (std::size_t m = 0; m < M; m++) {
      if (res.init[m].data != init[m].data) return 14;  // the queue's inits are those of SeedRestarts
      print("INIT", m, init[m].data);
      print("TRAJ", m, res.traj[m].data);
    }
    const std::vector<Trajectory> delta = TrajectoryPosteriorSamples(model, sdf, res.traj[0], start, zero, end, zero, setting, 3, seed);
    if (delta.size() != 3) return 15;
    for (std::size_t k = 0; k < 3; k++) print("DELTA", k, delta[k].data);
    const Vector z = NormalFill(seed, GPMP2MI_RNG_POSTERIOR, 0, 1, 0, 3, static_cast<int>(N + 1), 4);
    if (z.size() != 3 * (N + 1) * 4) return 16;
    print("Z", 0, z);
    std::printf("OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
