// Builds against include/gpmp2mi_planner.hpp with plain g++ and links the product library.  GroupRows is host code and
// runs everywhere; GroupTrajectories and BatchTrajOptimizeDistinct need the GPU: without one they must throw (no silent
// fallback), with one they find the two bundles of a hand-made batch and hand over one representative of each.
#include <cmath>
#include <cstdio>
#include <limits>

#include "gpmp2mi_planner.hpp"

using namespace gpmp2mi;

int main() {
  try {
    // the chain: a-b and b-c are within 1.5, a-c is not
    const Vector chain{0.0, 1.0, 2.0, 1.0, 0.0, 1.0, 2.0, 1.0, 0.0};
    TrajectoryGroups g = GroupRows(chain, {2.0, 1.0, 3.0}, {}, 1.5);      // b first: one mode of three
    if (g.n_modes != 1 || g.mode != std::vector<int>{0, 0, 0} || g.leaders != std::vector<int>{1} || g.sizes != std::vector<int>{3}) return 10;
    g = GroupRows(chain, {1.0, 2.0, 3.0}, {}, 1.5);                       // a first: {a, b} and {c}
    if (g.n_modes != 2 || g.mode != std::vector<int>{0, 0, 1} || g.leaders != std::vector<int>{0, 2} || g.sizes != std::vector<int>{2, 1}) return 11;
    g = GroupRows(chain, {1.0, 1.0, 1.0}, {1, 0, 1}, 1.5);                // ties to the lowest row; b does not take part
    if (g.n_modes != 2 || g.mode != std::vector<int>{0, -1, 1} || g.leaders != std::vector<int>{0, 2}) return 12;
    g = GroupRows(chain, {1.0, std::nan(""), 3.0}, {}, std::numeric_limits<double>::infinity());
    if (g.n_modes != 1 || g.mode != std::vector<int>{0, -1, 0} || g.sizes != std::vector<int>{2}) return 13;
    bool threw = false;
    try {
      GroupRows(chain, {1.0, 2.0, 3.0}, {}, -1.0);
    } catch (const std::exception&) {
      threw = true;
    }
    if (!threw) return 14;
    std::printf("RULE OK\n");

    // two bundles of straight lines in joint space, 0.01 apart inside a bundle and 1 apart between them
    std::vector<Trajectory> rows;
    for (double off : {0.0, 1.0, 0.01, 1.01, 0.02})
      rows.push_back(initArmTrajStraightLine({0.1 + off, 0.2, -0.1}, {0.6 + off, -0.2, 0.3}, 6));
    const Vector score{3.0, 1.0, 2.0, 5.0, 4.0};
    g = GroupTrajectories(rows, score, {}, 0.1);
    std::printf("GROUPS n=%zu leaders=%d,%d sizes=%d,%d\n", g.n_modes, g.n_modes > 0 ? g.leaders[0] : -1,
                g.n_modes > 1 ? g.leaders[1] : -1, g.n_modes > 0 ? g.sizes[0] : 0, g.n_modes > 1 ? g.sizes[1] : 0);
    if (g.n_modes != 2 || g.mode != std::vector<int>{1, 0, 1, 0, 1} || g.leaders != std::vector<int>{1, 2} || g.sizes != std::vector<int>{2, 3}) return 20;
    if (GroupTrajectories(rows, score, {}, 0.1, GPMP2MI_DIST_RMS).mode != g.mode) return 21;
    if (GroupTrajectories(rows, score, {}, 0.1, GPMP2MI_DIST_MAX_STATE, {0.0, 1.0, 1.0}).n_modes != 1) return 22;   // joint 0 ignored
    if (GroupTrajectories(rows, score, {1, 0, 1, 1, 1}, 0.1).leaders != std::vector<int>{2, 3}) return 23;

    // the plan form: a 3-link arm in an empty field, restarts from the two bundles
    Arm arm(3, {0.5, 0.5, 0.5}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, Pose3::Translation(0.0, 0.0, 0.0));
    BodySphereVector spheres;
    for (int l = 0; l < 3; l++) spheres.emplace_back(l, 0.05, std::array<double, 3>{-0.25, 0.0, 0.0});
    ArmModel model(arm, spheres);
    const std::vector<double> field(20 * 20 * 20, 5.0);
    SignedDistanceField sdf({-2.0, -2.0, -2.0}, 0.2, 20, 20, 20, field);
    TrajOptimizerSetting setting(3);
    setting.set_total_step(6);
    setting.set_total_time(1.2);
    setting.setGaussNewton();
    const Vector start{0.1, 0.2, -0.1}, end{0.6, -0.2, 0.3}, zero{0.0, 0.0, 0.0};
    const DistinctAlternatives d = BatchTrajOptimizeDistinct(model, sdf, start, zero, end, zero, rows, setting, 2, 0.05, 4);
    std::printf("DISTINCT modes=%zu eligible=%zu alt0=%d\n", d.n_modes, d.n_eligible, d.alt.empty() ? -1 : d.alt[0]);
    // one optimum in an empty field: every restart ends on it
    if (d.n_eligible != 5 || d.n_modes != 1 || d.alt.size() != 1 || d.alt_size[0] != 5 || d.traj.size() != 1 || d.dense.size() != 1) return 30;
    if (d.traj[0].total_step != 6 || d.dense[0].total_step != 18 || d.mode != std::vector<int>{0, 0, 0, 0, 0}) return 31;
    for (std::size_t i = 0; i <= 6; i++)
      for (std::size_t k = 0; k < 6; k++)
        if (d.dense[0].data[3 * i * 6 + k] != d.traj[0].data[i * 6 + k]) return 32;   // support states are copied
    std::printf("OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
