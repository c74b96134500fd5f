// risk.hip -- the posterior on the executed timeline (include/gpmp2mi.h): the covariance of every checked state from the
// band of Sigma at the support states, and the k-sigma clearance of the executed trajectory, for caller buffers and for
// a plan at its current estimate.  The plan forms run linearize -> export -> k_posterior through plan_posterior_band
// into a band workspace the plan owns, then the kernels of risk_kernels.hip; the optimizer's records, factors and
// estimate are not touched.  The `_dev` forms enqueue and return.
#include <cmath>

#include "host.h"

using namespace g2;

namespace {

constexpr int RISK_MAX_N = TILE - 1;   // the limit of k_posterior: one tile per block

int check_timeline_args(int inter, int B, int total_step, double delta_t) {
  G2_CHECK(inter >= 0, GPMP2MI_ERR_INVALID, "inter_step must be >= 0");
  G2_CHECK(B >= 0, GPMP2MI_ERR_INVALID, "B must be >= 0");
  G2_CHECK(total_step >= 1, GPMP2MI_ERR_INVALID, "total_step must be >= 1");
  G2_CHECK(delta_t > 0, GPMP2MI_ERR_INVALID, "delta_t must be > 0");
  const long long Md = (long long)total_step * (inter + 1) + 1;
  G2_CHECK(Md < (1ll << 31) / GPMP2MI_MAX_DOF && (long long)score_blocks((int)Md) * std::max(B, 1) < (1ll << 31) &&
               (long long)total_step * std::max(B, 1) < (1ll << 31),
           GPMP2MI_ERR_INVALID, "too many checked states for one launch");
  return GPMP2MI_OK;
}
int check_kappa(double kappa) {
  G2_CHECK(std::isfinite(kappa) && kappa >= 0.0, GPMP2MI_ERR_INVALID, "kappa must be finite and >= 0");
  return GPMP2MI_OK;
}
// the robot kinds k_risk is instantiated for; refused before dispatch
int check_risk_robot(const RobotDev& h) {
  G2_CHECK(h.kind < GPMP2MI_ROBOT_POSE2_MOBILE_BASE, GPMP2MI_ERR_UNSUPPORTED,
           "risk: vector-space robots only (arm, point robot); the Pose2 robot kinds would need the covariance of the "
           "tangent-space interpolation");
  if (2 * h.dof > RISK_MAX_N) {
    set_error("posterior: built for blocks of one tile, 2 dof <= 15 (dof <= 7); this robot has dof " +
              std::to_string(h.dof));
    return GPMP2MI_ERR_UNSUPPORTED;
  }
  return GPMP2MI_OK;
}

struct RiskOut {
  double *robust = nullptr, *sigma_worst = nullptr, *sigma = nullptr;
  int *worst = nullptr, *oor = nullptr;
};

// k_risk over `traj` and the band into `recs`, then k_risk_finish with the outputs of `o`; device pointers
int enqueue_risk(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, const double* Qc, double dt, int inter, int B, int N,
                 const double* traj, const double* Sd, const double* So, const int* ok, double kappa, const RiskOut& o,
                 RiskRec* recs, hipStream_t st) {
  const int Md = N * (inter + 1) + 1;
  G2_TRY(launch_risk(r->h, r->d, s->h, Qc, dt, inter, B, N, kappa, traj, Sd, So, ok, o.sigma, recs, st));
  const RiskFinish f{B, score_blocks(Md), recs, ok, o.robust, o.sigma_worst, o.worst, o.oor};
  return launch_risk_finish(f, st);
}

// a plan's workspace for (B, N, n, inter): the band, ok, then the records
struct PlanRiskWs {
  double *Sd, *So;
  int* ok;
  RiskRec* recs;
  size_t bytes;
};
PlanRiskWs risk_ws_layout(char* base, const PlanParams& P, int inter) {
  const size_t nn = (size_t)P.n * P.n, Md = (size_t)P.N * (inter + 1) + 1;
  PlanRiskWs w{};
  Carver take{base};
  w.Sd = (double*)take((size_t)P.B * (P.N + 1) * nn * sizeof(double));
  w.So = (double*)take((size_t)P.B * P.N * nn * sizeof(double));
  w.ok = (int*)take(P.B * sizeof(int));
  w.recs = (RiskRec*)take((size_t)P.B * score_blocks((int)Md) * sizeof(RiskRec));
  w.bytes = take.off;
  return w;
}

// what every plan call of this unit checks first; nothing is enqueued before it passes
int check_risk_plan(gpmp2mi_plan* p, int inter) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_CHECK(inter >= 0, GPMP2MI_ERR_INVALID, "inter_step must be >= 0");
  G2_TRY(plan_posterior_check(p));
  G2_CHECK(!p->hp.lie, GPMP2MI_ERR_UNSUPPORTED,
           "risk: vector-space robots only (arm, point robot); the Pose2 robot kinds would need the covariance of the "
           "tangent-space interpolation");
  G2_TRY(check_timeline_args(inter, p->hp.B, p->hp.N, p->hp.delta_t));
  G2_CHECK(p->robot->h.dof == p->hp.D, GPMP2MI_ERR_INVALID, "robot dof does not fit the plan");
  return GPMP2MI_OK;
}

// the band of Sigma at the plan's current estimate into its workspace on `st`; Qc on the device at the first call
int plan_band(gpmp2mi_plan* p, int inter, PlanRiskWs* w, int* ok_out, hipStream_t st) {
  const PlanParams& P = p->hp;
  if (!p->risk_qc) {
    G2_TRY(dev_malloc((void**)&p->risk_qc, p->Qc.size() * sizeof(double)));
    G2_HIP(hipMemcpy(p->risk_qc, p->Qc.data(), p->Qc.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  G2_TRY(p->ws[p->WS_RISK].reserve(risk_ws_layout(nullptr, P, inter).bytes));
  *w = risk_ws_layout((char*)p->ws[p->WS_RISK].p, P, inter);
  G2_TRY(plan_posterior_band(p, w->Sd, w->So, w->ok, st));   // marks `st` dirty
  if (ok_out) G2_HIP(hipMemcpyAsync(ok_out, w->ok, P.B * sizeof(int), hipMemcpyDeviceToDevice, st));
  return GPMP2MI_OK;
}

int plan_dense_dev(gpmp2mi_plan* p, int inter, double* cov, int* ok, hipStream_t st) {
  const PlanParams& P = p->hp;
  PlanRiskWs w;
  G2_TRY(plan_band(p, inter, &w, ok, st));
  if (!cov) return GPMP2MI_OK;
  return launch_gp_interp_cov(P.D, p->risk_qc, P.delta_t, inter, P.B, P.N, w.Sd, w.So, cov, st);
}

int plan_risk_dev(gpmp2mi_plan* p, int inter, double kappa, const RiskOut& o, int* ok, hipStream_t st) {
  const PlanParams& P = p->hp;
  PlanRiskWs w;
  G2_TRY(plan_band(p, inter, &w, ok, st));
  const double* traj = p->optimized ? p->pb.result : p->pb.init;
  return enqueue_risk(p->robot, p->sdf, p->risk_qc, P.delta_t, inter, P.B, P.N, traj, w.Sd, w.So, w.ok, kappa, o, w.recs,
                      st);
}

}  // namespace

extern "C" {

int gpmp2mi_gp_interpolate_cov_dev(int dof, const double* Qc, double delta_t, int inter_step, int B, int total_step,
                                   const double* Sdiag, const double* Soff, double* cov, void* stream) {
  G2_CHECK(dof >= 1 && dof <= GPMP2MI_MAX_DOF, GPMP2MI_ERR_INVALID, "dof must be 1..GPMP2MI_MAX_DOF");
  G2_CHECK(Sdiag && Soff, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_timeline_args(inter_step, B, total_step, delta_t));
  if (B == 0 || !cov) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  return launch_gp_interp_cov(dof, Qc, delta_t, inter_step, B, total_step, Sdiag, Soff, cov, (hipStream_t)stream);
}

int gpmp2mi_gp_interpolate_cov(int dof, const double* Qc, double delta_t, int inter_step, int B, int total_step,
                               const double* Sdiag, const double* Soff, double* cov) {
  G2_CHECK(dof >= 1 && dof <= GPMP2MI_MAX_DOF, GPMP2MI_ERR_INVALID, "dof must be 1..GPMP2MI_MAX_DOF");
  G2_CHECK(Sdiag && Soff, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_timeline_args(inter_step, B, total_step, delta_t));
  if (B == 0 || !cov) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const size_t nn = (size_t)4 * dof * dof, Md = (size_t)total_step * (inter_step + 1) + 1;
  DevBuf<double> dq, dsd, dso, dc;
  if (Qc) G2_TRY(dq.upload(Qc, (size_t)dof * dof));
  G2_TRY(dsd.upload(Sdiag, (size_t)B * (total_step + 1) * nn));
  G2_TRY(dso.upload(Soff, (size_t)B * total_step * nn));
  G2_TRY(dc.out(cov, (size_t)B * Md * nn));
  G2_TRY(launch_gp_interp_cov(dof, dq.p, delta_t, inter_step, B, total_step, dsd.p, dso.p, dc.p, nullptr));
  return fetch_all(dc);
}

int gpmp2mi_risk_traj_dev(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, const double* Qc, double delta_t, int inter_step,
                          int B, int total_step, const double* traj, const double* Sdiag, const double* Soff,
                          const int* ok, double kappa, double* robust_clearance, int* worst, double* sigma_worst,
                          int* out_of_range, double* sigma, void* stream) {
  G2_CHECK(r && s && traj && Sdiag && Soff, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_timeline_args(inter_step, B, total_step, delta_t));
  G2_TRY(check_kappa(kappa));
  G2_TRY(check_risk_robot(r->h));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  int cur = -1;
  G2_HIP(hipGetDevice(&cur));
  G2_CHECK(cur == r->device, GPMP2MI_ERR_INVALID, "the robot handle lives on another device than the current one");
  const size_t Md = (size_t)total_step * (inter_step + 1) + 1;
  // the records share the robot handle's workspace with gpmp2mi_score_traj_dev, under its rule: calls in stream order
  std::lock_guard<std::mutex> lk(r->score_mu);
  G2_TRY(r->score_ws.reserve((size_t)B * score_blocks((int)Md) * sizeof(RiskRec)));
  RiskOut o;
  o.robust = robust_clearance; o.worst = worst; o.sigma_worst = sigma_worst; o.oor = out_of_range; o.sigma = sigma;
  return enqueue_risk(r, s, Qc, delta_t, inter_step, B, total_step, traj, Sdiag, Soff, ok, kappa, o,
                      (RiskRec*)r->score_ws.p, (hipStream_t)stream);
}

int gpmp2mi_risk_traj(const gpmp2mi_robot* r, const gpmp2mi_sdf* s, const double* Qc, double delta_t, int inter_step,
                      int B, int total_step, const double* traj, const double* Sdiag, const double* Soff, const int* ok,
                      double kappa, double* robust_clearance, int* worst, double* sigma_worst, int* out_of_range,
                      double* sigma) {
  G2_CHECK(r && s && traj && Sdiag && Soff, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(check_timeline_args(inter_step, B, total_step, delta_t));
  G2_TRY(check_kappa(kappa));
  G2_TRY(check_risk_robot(r->h));
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const int D = r->h.dof;
  const size_t nn = (size_t)4 * D * D, Md = (size_t)total_step * (inter_step + 1) + 1;
  DevBuf<double> dq, dt, dsd, dso, dc, dsw, dsg;
  DevBuf<int> dk, dw, dr;
  if (Qc) G2_TRY(dq.upload(Qc, (size_t)D * D));
  G2_TRY(dt.upload(traj, (size_t)B * (total_step + 1) * 2 * D));
  G2_TRY(dsd.upload(Sdiag, (size_t)B * (total_step + 1) * nn));
  G2_TRY(dso.upload(Soff, (size_t)B * total_step * nn));
  if (ok) G2_TRY(dk.upload(ok, B));
  if (robust_clearance) G2_TRY(dc.out(robust_clearance, B));
  if (worst) G2_TRY(dw.out(worst, (size_t)2 * B));
  if (sigma_worst) G2_TRY(dsw.out(sigma_worst, B));
  if (out_of_range) G2_TRY(dr.out(out_of_range, B));
  if (sigma) G2_TRY(dsg.out(sigma, (size_t)B * Md * r->h.nr_spheres));
  G2_TRY(gpmp2mi_risk_traj_dev(r, s, dq.p, delta_t, inter_step, B, total_step, dt.p, dsd.p, dso.p, dk.p, kappa, dc.p,
                               dw.p, dsw.p, dr.p, dsg.p, nullptr));
  return fetch_all(dc, dw, dsw, dr, dsg);
}

int gpmp2mi_plan_marginals_dense_dev(gpmp2mi_plan* p, int inter_step, double* cov, int* ok, void* stream) {
  G2_TRY(check_risk_plan(p, inter_step));
  return plan_dense_dev(p, inter_step, cov, ok, (hipStream_t)stream);
}

int gpmp2mi_plan_marginals_dense(gpmp2mi_plan* p, int inter_step, double* cov, int* ok) {
  G2_TRY(check_risk_plan(p, inter_step));
  const PlanParams& P = p->hp;
  const size_t nn = (size_t)P.n * P.n, Md = (size_t)P.N * (inter_step + 1) + 1;
  DevBuf<double> dc;
  DevBuf<int> dk;
  if (cov) G2_TRY(dc.out(cov, (size_t)P.B * Md * nn));
  if (ok) G2_TRY(dk.out(ok, P.B));
  G2_TRY(plan_dense_dev(p, inter_step, dc.p, dk.p, nullptr));
  G2_TRY(fetch_all(dc, dk));
  p->mark_clean(nullptr);
  return GPMP2MI_OK;
}

int gpmp2mi_plan_risk_dev(gpmp2mi_plan* p, int inter_step, double kappa, double* robust_clearance, int* worst,
                          double* sigma_worst, int* out_of_range, double* sigma, int* ok, void* stream) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_TRY(check_kappa(kappa));
  G2_TRY(check_risk_plan(p, inter_step));
  RiskOut o;
  o.robust = robust_clearance; o.worst = worst; o.sigma_worst = sigma_worst; o.oor = out_of_range; o.sigma = sigma;
  return plan_risk_dev(p, inter_step, kappa, o, ok, (hipStream_t)stream);
}

int gpmp2mi_plan_risk(gpmp2mi_plan* p, int inter_step, double kappa, double* robust_clearance, int* worst,
                      double* sigma_worst, int* out_of_range, double* sigma, int* ok) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_TRY(check_kappa(kappa));
  G2_TRY(check_risk_plan(p, inter_step));
  const PlanParams& P = p->hp;
  const size_t Md = (size_t)P.N * (inter_step + 1) + 1;
  DevBuf<double> dc, dsw, dsg;
  DevBuf<int> dw, dr, dk;
  RiskOut o;
  if (robust_clearance) G2_TRY(dc.out(robust_clearance, P.B));
  if (worst) G2_TRY(dw.out(worst, (size_t)2 * P.B));
  if (sigma_worst) G2_TRY(dsw.out(sigma_worst, P.B));
  if (out_of_range) G2_TRY(dr.out(out_of_range, P.B));
  if (sigma) G2_TRY(dsg.out(sigma, (size_t)P.B * Md * p->robot->h.nr_spheres));
  if (ok) G2_TRY(dk.out(ok, P.B));
  o.robust = dc.p; o.worst = dw.p; o.sigma_worst = dsw.p; o.oor = dr.p; o.sigma = dsg.p;
  G2_TRY(plan_risk_dev(p, inter_step, kappa, o, dk.p, nullptr));
  G2_TRY(fetch_all(dc, dw, dsw, dr, dsg, dk));
  p->mark_clean(nullptr);
  return GPMP2MI_OK;
}

}  // extern "C"
