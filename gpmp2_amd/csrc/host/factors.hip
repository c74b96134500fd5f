// factors.hip -- the factor-level entry points and the other one-call evaluations: host arrays in, one or two kernels
// on the null stream, host arrays out.
#include "host.h"

using namespace g2;

extern "C" {

int gpmp2mi_forward_kinematics(const gpmp2mi_robot* r, int M, const double* conf, double* poses, double* J) {
  G2_CHECK(r && conf && poses && M >= 0, GPMP2MI_ERR_INVALID, "null argument");
  if (M == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const int D = r->h.dof, L = r->h.nr_links;
  DevBuf<double> dq, dp, dj;
  G2_TRY(dq.upload(conf, (size_t)M * D));
  G2_TRY(dp.out(poses, (size_t)M * L * 16));
  if (J) G2_TRY(dj.out(J, (size_t)M * L * 6 * D));
  G2_TRY(launch_fk(r->h, r->d, M, dq.p, dp.p, dj.p, nullptr));
  return fetch_all(dp, dj);
}

int gpmp2mi_sphere_centers(const gpmp2mi_robot* r, int M, const double* conf, double* centers, double* J) {
  G2_CHECK(r && conf && centers && M >= 0, GPMP2MI_ERR_INVALID, "null argument");
  if (M == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const int D = r->h.dof, S = r->h.nr_spheres;
  DevBuf<double> dq, dc, dj;
  G2_TRY(dq.upload(conf, (size_t)M * D));
  G2_TRY(dc.out(centers, (size_t)M * S * 3));
  if (J) G2_TRY(dj.out(J, (size_t)M * S * 3 * D));
  G2_TRY(launch_sphere_centers(r->h, r->d, M, dq.p, dc.p, dj.p, nullptr));
  return fetch_all(dc, dj);
}

int gpmp2mi_workspace_prior_factor(const gpmp2mi_robot* r, int mode, int joint, const double des_pose[16], int M,
                                   const double* conf, double* err, double* H) {
  G2_CHECK(r && des_pose && conf && err && M >= 0, GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK(mode >= GPMP2MI_WORKSPACE_POSITION && mode <= GPMP2MI_WORKSPACE_POSE, GPMP2MI_ERR_INVALID, "unknown mode");
  G2_CHECK(joint >= 0 && joint < r->h.nr_links, GPMP2MI_ERR_INVALID, "joint out of range");
  if (M == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const int D = r->h.dof, L = r->h.nr_links, rows = mode == GPMP2MI_WORKSPACE_POSE ? 6 : 3;
  DevBuf<double> dq, dp, dj, dd, de, dh;
  G2_TRY(dq.upload(conf, (size_t)M * D));
  G2_TRY(dd.upload(des_pose, 16));
  G2_TRY(dp.alloc((size_t)M * L * 16));
  if (H) G2_TRY(dj.alloc((size_t)M * L * 6 * D));
  G2_TRY(de.out(err, (size_t)M * rows));
  if (H) G2_TRY(dh.out(H, (size_t)M * rows * D));
  G2_TRY(launch_fk(r->h, r->d, M, dq.p, dp.p, dj.p, nullptr));
  G2_TRY(launch_workspace_prior(mode, joint, L, D, M, dd.p, dp.p, dj.p, de.p, dh.p, nullptr));
  return fetch_all(de, dh);
}

int gpmp2mi_goal_factor_arm(const gpmp2mi_robot* r, const double dest_point[3], int M, const double* conf, double* err,
                            double* H) {
  G2_CHECK(r && dest_point, GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK(r->h.kind == GPMP2MI_ROBOT_ARM, GPMP2MI_ERR_INVALID, "GoalFactorArm needs an Arm");
  const double des[16] = {1, 0, 0, dest_point[0], 0, 1, 0, dest_point[1], 0, 0, 1, dest_point[2], 0, 0, 0, 1};
  return gpmp2mi_workspace_prior_factor(r, GPMP2MI_WORKSPACE_POSITION, r->h.arm_dof - 1, des, M, conf, err, H);
}

int gpmp2mi_self_collision_factor(const gpmp2mi_robot* r, int n_pairs, const double* data, int M, const double* conf,
                                  double* err, double* H) {
  G2_CHECK(r && data && conf && err && M >= 0 && n_pairs >= 0, GPMP2MI_ERR_INVALID, "null argument");
  const int D = r->h.dof, S = r->h.nr_spheres;
  for (int i = 0; i < n_pairs; i++) {
    const double a = data[i * 4], b = data[i * 4 + 1];
    G2_CHECK(a >= 0 && a < S && b >= 0 && b < S, GPMP2MI_ERR_INVALID, "sphere id out of range");
  }
  if (M == 0 || n_pairs == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  std::vector<double> radius(S);
  for (int s = 0; s < S; s++) radius[r->h.sph_orig[s]] = r->h.sph_r[s];
  DevBuf<double> dq, dc, dj, dd, dr, de, dh;
  G2_TRY(dq.upload(conf, (size_t)M * D));
  G2_TRY(dd.upload(data, (size_t)n_pairs * 4));
  G2_TRY(dr.upload(radius.data(), S));
  G2_TRY(dc.alloc((size_t)M * S * 3));
  if (H) G2_TRY(dj.alloc((size_t)M * S * 3 * D));
  G2_TRY(de.out(err, (size_t)M * n_pairs));
  if (H) G2_TRY(dh.out(H, (size_t)M * n_pairs * D));
  G2_TRY(launch_sphere_centers(r->h, r->d, M, dq.p, dc.p, dj.p, nullptr));
  G2_TRY(launch_self_collision(n_pairs, S, D, M, dd.p, dr.p, dc.p, dj.p, de.p, dh.p, nullptr));
  return fetch_all(de, dh);
}

int gpmp2mi_obstacle_factor(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, double eps, int M,
                            const double* conf, double* err, double* H1) {
  G2_CHECK(r && s && conf && err && M >= 0, GPMP2MI_ERR_INVALID, "null argument");
  if (M == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const int D = r->h.dof, S = r->h.nr_spheres;
  DevBuf<double> dq, de, dh;
  G2_TRY(dq.upload(conf, (size_t)M * D));
  G2_TRY(de.out(err, (size_t)M * S));
  if (H1) G2_TRY(dh.out(H1, (size_t)M * S * D));
  G2_TRY(launch_obstacle(r->h, r->d, s->h, eps, M, dq.p, de.p, dh.p, nullptr));
  return fetch_all(de, dh);
}

int gpmp2mi_obstacle_gp_factor(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, double eps, const double* Qc,
                               double delta_t, double tau, int M, const double* c1, const double* v1,
                               const double* c2, const double* v2, double* err, double* H1, double* H2,
                               double* H3, double* H4) {
  (void)Qc;  // Lambda / Psi do not depend on Qc (pinned by tests/test_oracle_known_answers.py)
  G2_CHECK(r && s && c1 && v1 && c2 && v2 && err && M >= 0, GPMP2MI_ERR_INVALID, "null argument");
  const bool jac = H1 || H2 || H3 || H4;
  G2_CHECK(!jac || (H1 && H2 && H3 && H4), GPMP2MI_ERR_INVALID, "pass all four Jacobians or none");
  if (M == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const int D = r->h.dof, S = r->h.nr_spheres;
  DevBuf<double> a, b, c, d, de, h1, h2, h3, h4;
  G2_TRY(a.upload(c1, (size_t)M * D));
  G2_TRY(b.upload(v1, (size_t)M * D));
  G2_TRY(c.upload(c2, (size_t)M * D));
  G2_TRY(d.upload(v2, (size_t)M * D));
  G2_TRY(de.out(err, (size_t)M * S));
  if (jac) {
    G2_TRY(h1.out(H1, (size_t)M * S * D));
    G2_TRY(h2.out(H2, (size_t)M * S * D));
    G2_TRY(h3.out(H3, (size_t)M * S * D));
    G2_TRY(h4.out(H4, (size_t)M * S * D));
  }
  const GpCoef gc = gp_coef(delta_t, tau);
  G2_TRY(launch_obstacle_gp(r->h, r->d, s->h, eps, gc, M, a.p, b.p, c.p, d.p, de.p, h1.p, h2.p, h3.p, h4.p, nullptr));
  return fetch_all(de, h1, h2, h3, h4);
}

int gpmp2mi_gp_prior_factor(int D, int lie, double dt, int M, const double* c1, const double* v1,
                            const double* c2, const double* v2, double* err, double* H1, double* H2,
                            double* H3, double* H4) {
  G2_CHECK(c1 && v1 && c2 && v2 && err && M >= 0 && D > 0, GPMP2MI_ERR_INVALID, "null argument");
  const bool jac = H1 || H2 || H3 || H4;
  G2_CHECK(!jac || (H1 && H2 && H3 && H4), GPMP2MI_ERR_INVALID, "pass all four Jacobians or none");
  if (M == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  DevBuf<double> a, b, c, d, de, h1, h2, h3, h4;
  G2_TRY(a.upload(c1, (size_t)M * D));
  G2_TRY(b.upload(v1, (size_t)M * D));
  G2_TRY(c.upload(c2, (size_t)M * D));
  G2_TRY(d.upload(v2, (size_t)M * D));
  G2_TRY(de.out(err, (size_t)M * 2 * D));
  if (jac) {
    G2_TRY(h1.out(H1, (size_t)M * 2 * D * D));
    G2_TRY(h2.out(H2, (size_t)M * 2 * D * D));
    G2_TRY(h3.out(H3, (size_t)M * 2 * D * D));
    G2_TRY(h4.out(H4, (size_t)M * 2 * D * D));
  }
  if (lie) G2_TRY(launch_gp_prior_lie(D, dt, M, a.p, b.p, c.p, d.p, de.p, h1.p, h2.p, h3.p, h4.p, nullptr));
  else G2_TRY(launch_gp_prior_linear(D, dt, M, a.p, b.p, c.p, d.p, de.p, h1.p, h2.p, h3.p, h4.p, nullptr));
  return fetch_all(de, h1, h2, h3, h4);
}

int gpmp2mi_gp_interpolate(int D, int lie, const double* Qc, double dt, double tau, int M, const double* c1,
                           const double* v1, const double* c2, const double* v2, double* conf, double* vel) {
  (void)Qc;
  G2_CHECK(c1 && v1 && c2 && v2 && M >= 0 && D > 0, GPMP2MI_ERR_INVALID, "null argument");
  if (M == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  DevBuf<double> a, b, c, d, oc, ov;
  G2_TRY(a.upload(c1, (size_t)M * D));
  G2_TRY(b.upload(v1, (size_t)M * D));
  G2_TRY(c.upload(c2, (size_t)M * D));
  G2_TRY(d.upload(v2, (size_t)M * D));
  if (conf) G2_TRY(oc.out(conf, (size_t)M * D));
  if (vel) G2_TRY(ov.out(vel, (size_t)M * D));
  if (lie) G2_TRY(launch_gp_interp_lie(D, gp_coef(dt, tau), M, a.p, b.p, c.p, d.p, oc.p, ov.p, nullptr));
  else G2_TRY(launch_gp_interp_linear(D, gp_coef(dt, tau), M, a.p, b.p, c.p, d.p, oc.p, ov.p, nullptr));
  return fetch_all(oc, ov);
}

int gpmp2mi_interpolate_traj_dev(int D, int lie, double dt, int inter, int B, int N, int start, int end,
                                 const double* traj, double* out, void* stream) {
  G2_CHECK(traj && out && B >= 0 && D > 0 && inter >= 0 && dt > 0, GPMP2MI_ERR_INVALID, "bad argument");
  G2_CHECK(start >= 0 && start < end && end <= N, GPMP2MI_ERR_INVALID, "need 0 <= start_index < end_index <= total_step");
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const long long Mo = (long long)(end - start) * (inter + 1) + 1;
  G2_CHECK(Mo * B < (1ll << 31), GPMP2MI_ERR_INVALID, "too many output states for one launch");
  return launch_interpolate_traj(D, lie != 0, dt, inter, B, N, start, (int)Mo, traj, out, (hipStream_t)stream);
}

int gpmp2mi_interpolate_traj(int D, int lie, const double* Qc, double dt, int inter, int B, int N, int start,
                             int end, const double* traj, double* out) {
  (void)Qc;
  G2_CHECK(traj && out && B >= 0 && D > 0 && inter >= 0, GPMP2MI_ERR_INVALID, "bad argument");
  G2_CHECK(start >= 0 && start < end && end <= N, GPMP2MI_ERR_INVALID, "need 0 <= start_index < end_index <= total_step");
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const size_t Mo = (size_t)(end - start) * (inter + 1) + 1;
  DevBuf<double> a, o;
  G2_TRY(a.upload(traj, (size_t)B * (N + 1) * 2 * D));
  G2_TRY(o.out(out, (size_t)B * Mo * 2 * D));
  G2_TRY(gpmp2mi_interpolate_traj_dev(D, lie, dt, inter, B, N, start, end, a.p, o.p, nullptr));
  return fetch_all(o);
}

int gpmp2mi_vehicle_dynamics_factor(int D, int lie, int M, const double* conf, const double* vel, double* err, double* Hp,
                                    double* Hv) {
  G2_CHECK(conf && vel && err && M >= 0 && D >= 3, GPMP2MI_ERR_INVALID, "null argument or dof < 3");
  if (M == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  DevBuf<double> dc, dv, de, dp, dh;
  G2_TRY(dc.upload(conf, (size_t)M * D));
  G2_TRY(dv.upload(vel, (size_t)M * D));
  G2_TRY(de.out(err, M));
  if (Hp) G2_TRY(dp.out(Hp, (size_t)M * D));
  if (Hv) G2_TRY(dh.out(Hv, (size_t)M * D));
  G2_TRY(launch_vehicle_dynamics(D, lie, M, dc.p, dv.p, de.p, dp.p, dh.p, nullptr));
  return fetch_all(de, dp, dh);
}

int gpmp2mi_joint_limit_factor(int D, const double* down, const double* up, const double* th, int M,
                               const double* x, double* err, double* Hd) {
  G2_CHECK(down && up && th && x && err && M >= 0 && D > 0, GPMP2MI_ERR_INVALID, "null argument");
  if (M == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  DevBuf<double> a, b, c, dx, de, dh;
  G2_TRY(a.upload(down, D));
  G2_TRY(b.upload(up, D));
  G2_TRY(c.upload(th, D));
  G2_TRY(dx.upload(x, (size_t)M * D));
  G2_TRY(de.out(err, (size_t)M * D));
  if (Hd) G2_TRY(dh.out(Hd, (size_t)M * D));
  G2_TRY(launch_joint_limit(D, a.p, b.p, c.p, M, dx.p, de.p, dh.p, nullptr));
  return fetch_all(de, dh);
}

int gpmp2mi_block_tridiag_solve(int B, int nblk, int n, const double* Hd, const double* Ho, const double* b,
                                double* x, int* ok) {
  G2_CHECK(Hd && b && x && B >= 0 && nblk > 0 && n > 0, GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK(nblk == 1 || Ho, GPMP2MI_ERR_INVALID, "null argument");
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  DevBuf<double> dd, dob, db, dx, ds;
  DevBuf<int> dk;
  G2_TRY(dd.upload(Hd, (size_t)B * nblk * n * n));
  G2_TRY(dob.upload(Ho, (size_t)B * (nblk - 1) * n * n));
  G2_TRY(db.upload(b, (size_t)B * nblk * n));
  G2_TRY(dx.out(x, (size_t)B * nblk * n));
  G2_TRY(ds.alloc((size_t)B * nblk * 512));
  G2_TRY(dk.out(ok, B));
  G2_TRY(launch_block_tridiag_solve(B, nblk, n, dd.p, dob.p, db.p, dx.p, dk.p, ds.p, nullptr));
  return fetch_all(dx, dk);
}

int gpmp2mi_collision_cost(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, int total_step, int B,
                           const double* traj, double* cost) {
  // internal::CollisionCost planner/BatchTrajOptimizer-inl.h:87-100: unary obstacle error with
  // epsilon = 0 summed over all states; evaluated on device, summed on the host.
  G2_CHECK(r && s && traj && cost && B >= 0 && total_step >= 0, GPMP2MI_ERR_INVALID, "null argument");
  const int D = r->h.dof, S = r->h.nr_spheres, M = B * (total_step + 1);
  std::vector<double> conf((size_t)M * D), err((size_t)M * S);
  for (int m = 0; m < M; m++)
    for (int k = 0; k < D; k++) conf[(size_t)m * D + k] = traj[(size_t)m * 2 * D + k];
  G2_TRY(gpmp2mi_obstacle_factor(r, s, 0.0, M, conf.data(), err.data(), nullptr));
  for (int b = 0; b < B; b++) {
    double c = 0.0;
    for (int i = 0; i <= total_step; i++)
      for (int k = 0; k < S; k++) c += err[((size_t)b * (total_step + 1) + i) * S + k];
    cost[b] = c;
  }
  return GPMP2MI_OK;
}

}  // extern "C"
