// Builds against include/gpmp2mi_planner.hpp with plain g++ and links the product library.  Plans a 2-link problem
// through ISAM2TrajOptimizer2DArm, then prints (hex floats, exact) the estimate and the covariance blocks the facade
// returns for it -- jointMarginalCovariance / marginalCovariance of the class and TrajectoryMarginals at the same
// values -- for tests/test_cpp_posterior.py to compare with Plan.marginals().  Needs the GPU: without one it must throw.
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
    const std::size_t N = 10;
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
    const TrajectoryCovariance batch = TrajectoryMarginals(model, sdf, est, start, zero, end, zero, setting);
    if (batch.diag.size() != (N + 1) * 16 || batch.off.size() != N * 16) return 10;
    for (std::size_t i : {std::size_t(0), std::size_t(4), N}) {
      const Vector J = isam.jointMarginalCovariance(i), X = isam.marginalCovariance(i), V = isam.marginalCovariance(i, true);
      if (J.size() != 16 || X.size() != 4 || V.size() != 4) return 11;
      for (int r = 0; r < 2; r++)
        for (int c = 0; c < 2; c++)
          if (X[r * 2 + c] != J[r * 4 + c] || V[r * 2 + c] != J[(2 + r) * 4 + 2 + c]) return 12;
      for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++)
          if (J[r * 4 + c] != J[c * 4 + r]) return 13;
      if (!(J[0] > 0.0) || !(J[15] > 0.0)) return 14;
      print("JOINT", i, J);
      print("BATCH", i, batch.joint(i));
    }
    print("OFF", 4, Vector(batch.off.begin() + 4 * 16, batch.off.begin() + 5 * 16));
    bool threw = false;
    try {
      isam.jointMarginalCovariance(N + 1);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (!threw) return 15;
    std::printf("OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
