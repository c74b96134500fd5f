// Workspace path through the plain C header (include/gpmp2mi.h "workspace path"): a planar two-link arm in free space
// plans from one tool position to another twice, with a straight POSITION line of the tool as the plan's path and with
// the path cleared; the check and the selection run on the resident results.  Builds with plain g++ against the C ABI.
#include <cmath>
#include <cstdio>
#include <vector>

#include "gpmp2mi.h"

#define CK(call)                                                                   \
  do {                                                                             \
    int rc_ = (call);                                                              \
    if (rc_ != GPMP2MI_OK) {                                                       \
      std::printf("EXCEPTION %s -> %d: %s\n", #call, rc_, gpmp2mi_last_error());   \
      return 3;                                                                    \
    }                                                                              \
  } while (0)

static void tip(const double* q, double* t) {   // two unit links in the plane
  t[0] = std::cos(q[0]) + std::cos(q[0] + q[1]);
  t[1] = std::sin(q[0]) + std::sin(q[0] + q[1]);
  t[2] = 0.0;
}

int main() {
  const int D = 2, N = 10, B = 2;
  const double a[2] = {1.0, 1.0}, zero[2] = {0.0, 0.0};
  const int sph_link[2] = {0, 1};
  const double sph_r[2] = {0.05, 0.05}, sph_c[6] = {-0.5, 0, 0, -0.5, 0, 0};
  gpmp2mi_robot_desc rd{};
  rd.kind = GPMP2MI_ROBOT_ARM;
  rd.dof = rd.arm_dof = D;
  rd.a = a; rd.alpha = zero; rd.d = zero; rd.theta_bias = nullptr;
  for (int i = 0; i < 4; i++) rd.base_pose[5 * i] = rd.base_pose2[5 * i] = rd.base_pose3[5 * i] = 1.0;
  rd.nr_spheres = 2;
  rd.sphere_link = sph_link; rd.sphere_radius = sph_r; rd.sphere_center = sph_c;
  gpmp2mi_robot* robot = nullptr;
  CK(gpmp2mi_robot_create(&rd, &robot));
  const int G = 12;   // free space: the field is 10 everywhere
  const double origin[3] = {-3.0, -3.0, -3.0};
  std::vector<double> vox((size_t)G * G * G, 10.0);
  gpmp2mi_sdf* sdf = nullptr;
  CK(gpmp2mi_sdf_create(3, origin, 0.5, G, G, G, vox.data(), GPMP2MI_SDF_LAYOUT_ZYX, &sdf));
  gpmp2mi_settings st;
  gpmp2mi_settings_default(&st, D);
  st.total_step = N;
  st.total_time = 2.0;
  st.conf_prior_sigma = st.vel_prior_sigma = 1e-4;
  st.epsilon = 0.1;
  st.cost_sigma = 0.05;
  st.obs_check_inter = 2;
  st.opt_type = GPMP2MI_OPT_LM;
  st.max_iter = 200;
  st.rel_thresh = 1e-7;   // run to the optimum: the deviations below are compared with each other
  gpmp2mi_graph_opts go;
  gpmp2mi_graph_opts_default(&go);
  go.workspace_path = 1;
  go.workspace_path_mode = GPMP2MI_WORKSPACE_POSITION;
  go.workspace_path_link = 1;
  gpmp2mi_plan* plan = nullptr;
  CK(gpmp2mi_plan_create(robot, sdf, &st, &go, B, &plan));

  const double qs[2] = {0.3, 1.2}, qe[2] = {1.4, 0.6};
  double ts[3], te[3];
  tip(qs, ts);
  tip(qe, te);
  std::vector<double> des((size_t)(N + 1) * 16, 0.0), sigma(N + 1, 0.0005);
  for (int i = 0; i <= N; i++) {
    double* T = &des[(size_t)i * 16];
    T[0] = T[5] = T[10] = T[15] = 1.0;
    for (int k = 0; k < 3; k++) T[4 * k + 3] = ts[k] + (double)i / N * (te[k] - ts[k]);
  }
  // (the factor acts on the support states, and the deviations below are those of the support states, inter_step 0:
  // between two of them the tool follows the GP interpolation of the joints, 2.5 cm off this line at N = 10, which the
  // selection's allowance of 5 cm at inter_step 4 admits)
  std::vector<double> sc, ec, z((size_t)B * D, 0.0), init((size_t)B * (N + 1) * 2 * D);
  for (int b = 0; b < B; b++) {
    sc.insert(sc.end(), qs, qs + D);
    ec.insert(ec.end(), qe, qe + D);
    for (int i = 0; i <= N; i++)
      for (int k = 0; k < D; k++) {
        const double bump = b * 0.2 * std::sin(M_PI * i / N);   // row 1 starts off the straight line
        init[((size_t)b * (N + 1) + i) * 2 * D + k] = qs[k] + (double)i / N * (qe[k] - qs[k]) + bump;
        init[((size_t)b * (N + 1) + i) * 2 * D + D + k] = (qe[k] - qs[k]) / st.total_time;
      }
  }
  double dev_with[2], dev_without[2], dense[2];
  int worst[4], invalid[2], best = -9, n = -9;
  std::vector<double> traj_best((size_t)(N + 1) * 2 * D);
  // a refused path changes nothing: a sigma of zero
  sigma[3] = 0.0;
  if (gpmp2mi_plan_set_workspace_path(plan, des.data(), sigma.data()) != GPMP2MI_ERR_INVALID) {
    std::printf("FAIL a zero sigma was accepted\n");
    return 1;
  }
  sigma[3] = 0.0005;
  CK(gpmp2mi_plan_set_workspace_path(plan, des.data(), sigma.data()));
  CK(gpmp2mi_plan_set_problem(plan, sc.data(), z.data(), ec.data(), z.data(), init.data()));
  CK(gpmp2mi_plan_optimize(plan, nullptr));
  CK(gpmp2mi_plan_path_score(plan, 0, dev_with, nullptr, worst, nullptr, dense, invalid));
  CK(gpmp2mi_plan_select_path(plan, 4, -1e300, 0, 0.05, INFINITY, &best, &n, traj_best.data(), nullptr));
  int iters[2], status[2];
  CK(gpmp2mi_plan_get_result(plan, nullptr, iters, nullptr, status, nullptr));
  std::printf("WITH max_pos_dev %.4f %.4f invalid %d %d iterations %d %d status %d %d best %d of %d\n", dev_with[0],
              dev_with[1], invalid[0], invalid[1], iters[0], iters[1], status[0], status[1], best, n);
  if (best < 0 || n != 2 || invalid[0] || invalid[1] || !(dense[0] > 0)) {
    std::printf("FAIL the rows should both follow the line\n");
    return 1;
  }
  // the same plan without the path, scored against the same line through the trajectory form
  CK(gpmp2mi_plan_set_workspace_path(plan, nullptr, nullptr));
  CK(gpmp2mi_plan_set_problem(plan, sc.data(), z.data(), ec.data(), z.data(), init.data()));
  CK(gpmp2mi_plan_optimize(plan, nullptr));
  std::vector<double> traj((size_t)B * (N + 1) * 2 * D);
  CK(gpmp2mi_plan_get_result(plan, traj.data(), nullptr, nullptr, nullptr, nullptr));
  CK(gpmp2mi_path_score_traj(robot, GPMP2MI_WORKSPACE_POSITION, 1, des.data(), sigma.data(), st.total_time / N, 0, B, N,
                             traj.data(), dev_without, nullptr, nullptr, nullptr, nullptr, nullptr));
  CK(gpmp2mi_plan_select_path(plan, 4, -1e300, 0, 0.05, INFINITY, &best, &n, nullptr, nullptr));
  std::printf("WITHOUT max_pos_dev %.4f %.4f best %d of %d\n", dev_without[0], dev_without[1], best, n);
  if (!(10.0 * dev_with[0] <= dev_without[0]) || n != 2) {   // no path: nothing is checked, both rows stay eligible
    std::printf("FAIL the path should bind\n");
    return 1;
  }
  gpmp2mi_plan_destroy(plan);
  gpmp2mi_sdf_destroy(sdf);
  gpmp2mi_robot_destroy(robot);
  std::printf("OK path\n");
  return 0;
}
