// Builds against include/gpmp2mi_planner.hpp with plain g++ and links the product library.  Plans the 2-link problem of
// risk_smoke.cpp through ISAM2TrajOptimizer2DArm, then prints (hex floats, exact) the estimate and what SampledClearance
// returns for it, for tests/test_cpp_sampled.py to compare with Plan.collision_probability().  Needs the GPU: without one
// it must throw.
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
    const std::size_t N = 10, J = 3, K = 24;
    const double required = 0.05;
    TrajOptimizerSetting setting(2);
    setting.set_total_step(N);
    setting.set_total_time(2.0);
    setting.set_obs_check_inter(2);
    setting.set_cost_sigma(0.1);
    setting.set_epsilon(0.2);
    setting.setGaussNewton();
    const Vector start{0.0, 0.0}, end{1.5, 0.5}, zero{0.0, 0.0};
    ISAM2TrajOptimizer2DArm isam(model, sdf, setting);
    isam.initFactorGraph(start, zero, end, zero);
    isam.initValues(initArmTrajStraightLine(start, end, N));
    for (int k = 0; k < 3; k++) isam.update();
    const Trajectory est = isam.values();
    print("TRAJ", 0, est.data);
    const auto sc = SampledClearance(model, sdf, est, start, zero, end, zero, setting, J, K, 77u, required, true, 2, 5);
    if (sc.checked_states != N * (J + 1) + 1 || sc.samples != K || sc.clearance.size() != K || sc.worst.size() != 2 * K ||
        sc.state_hits.size() != sc.checked_states)
      return 10;
    int hits = 0;
    for (double c : sc.clearance) hits += c < required;
    if (hits != sc.hits || sc.probability != double(sc.hits) / double(K)) return 11;
    print("COUNTS", 0, Vector{double(sc.hits), sc.probability, double(sc.oor_samples)});
    print("CLEARANCE", 0, sc.clearance);
    print("WORST", 0, Vector(sc.worst.begin(), sc.worst.end()));
    print("STATEHITS", 0, Vector(sc.state_hits.begin(), sc.state_hits.end()));
    bool threw = false;
    try {
      SampledClearance(model, sdf, est, start, zero, end, zero, setting, 64, K, 77u, required);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (!threw) return 12;
    std::printf("OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
