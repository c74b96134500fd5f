// Builds against include/gpmp2mi_planner.hpp with plain g++ and links the product library.  On a box without a GPU the
// planner must throw (no silent fallback); on a GPU box it solves six 2-link problems sharded over devices {0, 0} and
// checks each against the one-problem BatchTrajOptimize2DArm call.
#include <cmath>
#include <cstdio>

#include "gpmp2mi_planner.hpp"

using namespace gpmp2mi;

int main() {
  try {
    Arm arm(2, {1.0, 1.0}, {0.0, 0.0}, {0.0, 0.0}, Pose3::Translation(0.0, 0.0, 0.0));
    BodySphereVector spheres;
    for (int l = 0; l < 2; l++)
      for (double x : {-0.75, -0.25}) spheres.emplace_back(l, 0.1, std::array<double, 3>{x, 0.0, 0.0});
    ArmModel model(arm, spheres);
    const int n = 60;
    Vector field(n * n);  // distance to a disc of radius 0.4 at (1.2, 1.0); column-major (row = y, col = x)
    for (int x = 0; x < n; x++)
      for (int y = 0; y < n; y++)
        field[x * n + y] = std::hypot(-3.0 + 0.1 * x - 1.2, -3.0 + 0.1 * y - 1.0) - 0.4;
    PlanarSDF sdf({-3.0, -3.0}, 0.1, n, n, field);
    TrajOptimizerSetting setting(2);
    setting.set_total_step(10);
    setting.set_total_time(2.0);
    setting.set_obs_check_inter(2);
    setting.set_cost_sigma(0.1);
    setting.set_epsilon(0.2);
    setting.setGaussNewton();
    const std::size_t B = 6;
    const Vector zero{0.0, 0.0};
    std::vector<Vector> sc, sv, ec, ev;
    std::vector<Trajectory> init;
    for (std::size_t b = 0; b < B; b++) {
      const Vector start{0.0, 0.1 * b}, end{1.5 - 0.05 * b, 0.5};
      sc.push_back(start), sv.push_back(zero), ec.push_back(end), ev.push_back(zero);
      init.push_back(initArmTrajStraightLine(start, end, 10));
    }
    MultiDeviceBatchPlanner planner(model, sdf, setting, B, {0, 0});
    const std::vector<int> rb = planner.row_begin();
    if (planner.devices() != std::vector<int>{0, 0} || rb != std::vector<int>{0, 3, 6}) return 4;
    const std::vector<Trajectory> out = planner.optimize(sc, sv, ec, ev, init);
    double worst = 0.0;
    for (std::size_t b = 0; b < B; b++) {
      int iters = 0;
      const Trajectory one = BatchTrajOptimize2DArm(model, sdf, sc[b], sv[b], ec[b], ev[b], init[b], setting, &iters);
      if (iters != planner.iterations()[b]) return 5;
      for (std::size_t i = 0; i < one.data.size(); i++) worst = std::fmax(worst, std::fabs(one.data[i] - out[b].data[i]));
    }
    std::printf("OK shards=2 iterations=%d..%d max|multi - single|=%.1e\n", planner.iterations()[0],
                planner.iterations()[B - 1], worst);
    if (worst > 0.0) return 6;
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
