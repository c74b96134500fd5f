// Builds against include/gpmp2mi_planner.hpp with plain g++ and links the product library.  The selection overload that
// takes the self scores is host code and runs everywhere; the pair table and the scores need the GPU: without one they
// must throw (no silent fallback), with one a 3-link arm folded onto itself is told from the same arm stretched out.
#include <cmath>
#include <cstdio>
#include <limits>

#include "gpmp2mi_planner.hpp"

using namespace gpmp2mi;

static TrajectoryScore score(double clearance, int out_of_range) {
  TrajectoryScore s;
  s.min_clearance = clearance;
  s.out_of_range = out_of_range;
  return s;
}
static TrajectorySelfScore self_score(double clearance, int invalid) {
  TrajectorySelfScore s;
  s.min_clearance = clearance;
  s.invalid = invalid;
  return s;
}

int main() {
  try {
    // the rule alone: row 1 is the cheapest but touches itself, row 2 has an invalid pair, rows 3 and 4 tie
    const double inf = std::numeric_limits<double>::infinity();
    const Vector fe{5.0, 1.0, 2.0, 3.0, 3.0, 0.5};
    const std::vector<int> status{0, 0, 0, 0, 1, GPMP2MI_TRAJ_NOT_SPD};
    const std::vector<TrajectoryScore> sc{score(0.1, 0), score(0.1, 0), score(0.1, 0), score(0.05, 3), score(0.2, 0), score(0.3, 0)};
    const std::vector<TrajectorySelfScore> ss{self_score(0.3, 0), self_score(-0.02, 0), self_score(inf, 4), self_score(0.2, 0),
                                              self_score(0.01, 0), self_score(0.3, 0)};
    std::size_t n = 99;
    if (SelectBestTrajectory(fe, status, sc, 0.0, false, &n) != 1 || n != 5) return 10;        // without the self scores
    if (SelectBestTrajectory(fe, status, sc, ss, 0.0, false, &n) != 3 || n != 3) return 11;
    if (SelectBestTrajectory(fe, status, sc, ss, 0.0, true, &n) != 4 || n != 2) return 12;
    if (SelectBestTrajectory(fe, status, sc, ss, -inf, false, &n) != 1 || n != 4) return 13;   // invalid stays out
    if (SelectBestTrajectory(fe, status, sc, ss, 0.04, false, &n) != 3 || n != 2) return 14;   // the smaller of the two
    if (SelectBestTrajectory(fe, status, sc, ss, 1.0, false, &n) != -1 || n != 0) return 15;
    std::printf("SELECT OK\n");

    Arm arm(3, {0.5, 0.5, 0.5}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, Pose3::Translation(0.0, 0.0, 0.0));
    BodySphereVector spheres;
    for (int l = 0; l < 3; l++)
      for (double x : {-0.375, -0.125}) spheres.emplace_back(l, 0.06, std::array<double, 3>{x, 0.0, 0.0});
    ArmModel model(arm, spheres);
    const SelfCollisionPairs pairs = SelfCollisionPairs::Generate(model, 2, Vector{0.0, 0.0, 0.0});
    if (pairs.size() != 4 || pairs.data().size() != 16) return 20;                              // link 0 against link 2
    const SelfCollisionPairs one(model, Vector{5.0, 0.0, 0.01, 1.0});
    if (one.size() != 1) return 21;
    TrajOptimizerSetting setting(3);
    setting.set_total_step(8);
    setting.set_total_time(2.0);
    const Trajectory folded = initArmTrajStraightLine({0.10, M_PI - 0.05, M_PI + 0.03}, {0.25, M_PI + 0.04, M_PI - 0.06}, 8);
    const Trajectory open = initArmTrajStraightLine({0.2, 0.1, -0.1}, {0.5, -0.2, 0.3}, 8);
    const TrajectorySelfScore f0 = SelfScoreTrajectory(model, pairs, folded, setting, 0), f4 = SelfScoreTrajectory(model, pairs, folded, setting, 4);
    const TrajectorySelfScore o4 = SelfScoreTrajectory(model, pairs, open, setting, 4);
    std::printf("FOLDED support=%.4f dense=%.4f clearance=%.4f at (%d, %d)\nOPEN dense=%.4f clearance=%.4f\n", f4.support_cost,
                f4.dense_cost, f4.min_clearance, f4.worst_state, f4.worst_pair, o4.dense_cost, o4.min_clearance);
    if (f0.dense_cost != f0.support_cost || f4.support_cost != f0.support_cost || f4.dense_cost < f4.support_cost) return 22;
    if (!(f4.min_clearance < -0.05) || f4.min_clearance > f0.min_clearance || f4.worst_state < 0 || f4.worst_state > 40 ||
        f4.worst_pair < 0 || f4.worst_pair > 3 || f4.invalid != 0)
      return 23;
    if (!(o4.min_clearance > 0.05) || o4.dense_cost != 0.0 || o4.invalid != 0) return 24;
    const TrajectorySelfScore e = SelfScoreTrajectory(model, SelfCollisionPairs(model, Vector{}), folded, setting, 4);
    if (e.dense_cost != 0.0 || e.min_clearance != inf || e.worst_state != -1 || e.worst_pair != -1) return 25;
    // the folded result is the cheaper one, and is not chosen
    const std::vector<TrajectoryScore> clear{score(0.5, 0), score(0.5, 0)};
    const int best = SelectBestTrajectory({1.0, 2.0}, {}, clear, {f4, o4}, 0.0, false, &n);
    if (best != 1 || n != 1) return 26;
    std::printf("OK best=%d of %zu eligible\n", best, n);
    return 0;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION %s\n", e.what());
    return 3;
  }
}
