// posterior.hip -- the posterior of a solved plan (include/gpmp2mi.h "posterior"): marginal covariances and samples, for
// caller systems and for a plan's graph at its estimate.  One launch of k_posterior (posterior_kernels.hip) per call;
// the plan forms put a linearization into the spare record buffer and its export in front of it, so the optimizer's
// state (the records at `cur`, its factors, its estimate) is not touched.  The `_dev` forms enqueue and return.
#include "host.h"

using namespace g2;

namespace {

constexpr int POST_MAX_N = TILE - 1;   // one tile per block, as launch_block_tridiag_solve

int check_chain_args(int B, int nblk, int n, const double* Hd, const double* Ho) {
  G2_CHECK(B >= 0 && nblk > 0 && n > 0, GPMP2MI_ERR_INVALID, "B must be >= 0, nblk and n positive");
  G2_CHECK(Hd && (nblk == 1 || Ho), GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK(n <= POST_MAX_N, GPMP2MI_ERR_UNSUPPORTED, "posterior: block size must be 1..15 (one 16 x 16 tile per block)");
  return GPMP2MI_OK;
}

// host systems in, host results out: the shared body of the two stand-alone calls
int chain_posterior(int B, int nblk, int n, int K, const double* Hd, const double* Ho, const double* z, double* Sd,
                    double* So, double* delta, int* ok) {
  if (B == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  const size_t nb = (size_t)B * nblk, no = (size_t)B * (nblk - 1);
  DevBuf<double> dd, dob, dz, dsd, dso, dde, dfac;
  DevBuf<int> dk;
  G2_TRY(dd.upload(Hd, nb * n * n));
  G2_TRY(dob.upload(Ho, no * n * n));
  if (K) G2_TRY(dz.upload(z, (size_t)K * nb * n));
  if (Sd) G2_TRY(dsd.out(Sd, nb * n * n));
  if (So) G2_TRY(dso.out(So, no * n * n));
  if (K) G2_TRY(dde.out(delta, (size_t)K * nb * n));
  if (ok) G2_TRY(dk.out(ok, B));
  G2_TRY(dfac.alloc(nb * 512));
  const PosteriorArgs a{nblk, K, dd.p, dob.p, dz.p, dsd.p, dso.p, dde.p, dk.p, dfac.p};
  G2_TRY(launch_posterior(B, n, a, nullptr));
  return fetch_all(dsd, dso, dde, dk);
}

// a plan's posterior workspace: the exported normal equations, then the factor scratch
struct PlanPostWs {
  double *Hd, *Ho, *fac;
  size_t bytes;
};
PlanPostWs post_ws_layout(char* base, const PlanParams& P) {
  const size_t nb = (size_t)P.B * (P.N + 1), nn = (size_t)P.n * P.n;
  PlanPostWs w{};
  size_t off = 0;
  auto take = [&](size_t count) {
    double* q = (double*)(base + off);
    off += ws_round(count * sizeof(double));
    return q;
  };
  w.Hd = take(nb * nn);
  w.Ho = take((size_t)P.B * P.N * nn);
  w.fac = take(nb * 512);
  w.bytes = off;
  return w;
}

int check_plan(gpmp2mi_plan* p) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_PLAN_LIVE(p);   // before anything is enqueued
  G2_CHECK(p->problem_set, GPMP2MI_ERR_INVALID, "call gpmp2mi_plan_set_problem first");
  if (p->hp.n > POST_MAX_N) {
    set_error("posterior: built for blocks of one tile, 2 dof <= 15 (dof <= 7); this plan has dof " +
              std::to_string(p->hp.D));
    return GPMP2MI_ERR_UNSUPPORTED;
  }
  return GPMP2MI_OK;
}

// `traj` (device) or, null, the plan's current estimate: linearize -> export -> k_posterior on `st`.  Outputs and z are
// device pointers.
int plan_posterior_dev(gpmp2mi_plan* p, const double* traj, int K, const double* z, double* Sd, double* So,
                       double* delta, int* ok, hipStream_t st) {
  const PlanParams& P = p->hp;
  if (!traj) traj = p->optimized ? p->pb.result : p->pb.init;
  G2_TRY(p->ws[p->WS_POST].reserve(post_ws_layout(nullptr, P).bytes));
  const PlanPostWs w = post_ws_layout((char*)p->ws[p->WS_POST].p, P);
  p->mark_dirty(st);
  // into the spare record buffer (the one that does not hold the linearization at `cur`), as gpmp2mi_plan_linearize
  G2_TRY(plan_linearize(p, traj, 1, nullptr, st));
  G2_TRY(launch_export_normal_eq(P, p->pb, traj, 1, w.Hd, w.Ho, nullptr, st));
  const PosteriorArgs a{P.N + 1, K, w.Hd, w.Ho, z, Sd, So, delta, ok, w.fac};
  return launch_posterior(P.B, P.n, a, st);
}

// host arrays: staged in DevBufs, the null stream, one synchronisation at the end
int plan_posterior_host(gpmp2mi_plan* p, const double* traj, int K, const double* z, double* Sd, double* So,
                        double* delta, int* ok) {
  const PlanParams& P = p->hp;
  const size_t nb = (size_t)P.B * (P.N + 1), nn = (size_t)P.n * P.n;
  DevBuf<double> dt, dz, dsd, dso, dde;
  DevBuf<int> dk;
  if (traj) G2_TRY(dt.upload(traj, p->tsz()));
  if (K) G2_TRY(dz.upload(z, (size_t)K * nb * P.n));
  if (Sd) G2_TRY(dsd.out(Sd, nb * nn));
  if (So) G2_TRY(dso.out(So, (size_t)P.B * P.N * nn));
  if (K) G2_TRY(dde.out(delta, (size_t)K * nb * P.n));
  if (ok) G2_TRY(dk.out(ok, P.B));
  G2_TRY(plan_posterior_dev(p, dt.p, K, dz.p, dsd.p, dso.p, dde.p, dk.p, nullptr));
  G2_TRY(fetch_all(dsd, dso, dde, dk));
  p->mark_clean(nullptr);
  return GPMP2MI_OK;
}

}  // namespace

int g2::plan_posterior_factor(gpmp2mi_plan* p, int* ok, const double** fac, hipStream_t st) {
  G2_TRY(plan_posterior_dev(p, nullptr, 0, nullptr, nullptr, nullptr, nullptr, ok, st));
  *fac = post_ws_layout((char*)p->ws[p->WS_POST].p, p->hp).fac;
  return GPMP2MI_OK;
}

int g2::plan_posterior_check(gpmp2mi_plan* p) { return check_plan(p); }
int g2::plan_posterior_band(gpmp2mi_plan* p, double* Sd, double* So, int* ok, hipStream_t st) {
  return plan_posterior_dev(p, nullptr, 0, nullptr, Sd, So, nullptr, ok, st);
}

extern "C" {

int gpmp2mi_block_tridiag_marginals(int B, int nblk, int n, const double* Hdiag, const double* Hoff, double* Sdiag,
                                    double* Soff, int* ok) {
  G2_TRY(check_chain_args(B, nblk, n, Hdiag, Hoff));
  return chain_posterior(B, nblk, n, 0, Hdiag, Hoff, nullptr, Sdiag, Soff, nullptr, ok);
}

int gpmp2mi_block_tridiag_sample(int B, int nblk, int n, int K, const double* Hdiag, const double* Hoff,
                                 const double* z, double* delta, int* ok) {
  G2_CHECK(K > 0 && z && delta, GPMP2MI_ERR_INVALID, "K must be > 0, z and delta not null");
  G2_TRY(check_chain_args(B, nblk, n, Hdiag, Hoff));
  return chain_posterior(B, nblk, n, K, Hdiag, Hoff, z, nullptr, nullptr, delta, ok);
}

int gpmp2mi_plan_marginals(gpmp2mi_plan* p, const double* traj, double* Sdiag, double* Soff, int* ok) {
  G2_TRY(check_plan(p));
  return plan_posterior_host(p, traj, 0, nullptr, Sdiag, Soff, nullptr, ok);
}
int gpmp2mi_plan_marginals_dev(gpmp2mi_plan* p, double* Sdiag, double* Soff, int* ok, void* stream) {
  G2_TRY(check_plan(p));
  return plan_posterior_dev(p, nullptr, 0, nullptr, Sdiag, Soff, nullptr, ok, (hipStream_t)stream);
}

int gpmp2mi_plan_sample_posterior(gpmp2mi_plan* p, int K, const double* z, double* delta, int* ok) {
  G2_CHECK(K > 0 && z && delta, GPMP2MI_ERR_INVALID, "K must be > 0, z and delta not null");
  G2_TRY(check_plan(p));
  return plan_posterior_host(p, nullptr, K, z, nullptr, nullptr, delta, ok);
}
int gpmp2mi_plan_sample_posterior_dev(gpmp2mi_plan* p, int K, const double* z, double* delta, int* ok, void* stream) {
  G2_CHECK(K > 0 && z && delta, GPMP2MI_ERR_INVALID, "K must be > 0, z and delta not null");
  G2_TRY(check_plan(p));
  return plan_posterior_dev(p, nullptr, K, z, nullptr, nullptr, delta, ok, (hipStream_t)stream);
}

}  // extern "C"
