// plan_device.h -- device helpers shared by the plan kernels: graph-error terms, the Dogleg retry test and the tail of
// a trial step.  The step-control rules themselves are in step_control.h.
#pragma once
#include "device_math.h"
#include "pass_counter.h"
#include "plan.h"
#include "tiles.h"

namespace g2 {

// =============================================================================== error terms
// prior + limit + vehicle-dynamics error of one trajectory (0.5 * whitened squared residuals),
// wave-reduced.  PriorFactor (planner/BatchTrajOptimizer-inl.h:41-48), JointLimitFactorVector,
// VelocityLimitFactorVector (:50-59), VehicleDynamicsFactor (dynamics/VehicleDynamics.h:19-27).
// One entry of that sum: `acc` plus the terms of coordinate rho of state i (start / goal prior, replanner state priors,
// position / velocity limit, vehicle dynamics).  zs: the state's 2D values; nxp = pb.xp_n[b].  Every caller that sums
// these terms goes through here: misc_error_partial below and the per-chunk shares of k_linearize_arm.
// MAYBE_LIE = false: the caller knows the robot has no Pose2 base (fixed-base arms), and the chart code is left out.
template <bool MAYBE_LIE = true>
__device__ __forceinline__ double misc_entry_add(double acc, const PlanParams& P, const PlanBuffers& pb, int b, int nxp,
                                                 int i, int rho, const double* __restrict__ zs) {
  const int D = P.D, n = P.n, N = P.N;
  const bool lie = MAYBE_LIE && P.lie;
  const int a = rho >= D, k = rho - a * D;
  const double z = zs[rho];
  if (i == 0 || (i == N && pb.goal_on[b] && (a || !P.end_conf_prior_off))) {
    const double* tg = (i == 0) ? (a ? pb.start_vel : pb.start_conf) : (a ? pb.end_vel : pb.end_conf);
    tg += (size_t)b * D;
    double d = z - tg[k];
    if (lie && !a && k < 3) {  // -Local(x, prior) of PriorFactor<Pose2Vector>
      const P2 bt = pose2_between(P2{zs[0], zs[1], zs[2]}, P2{tg[0], tg[1], tg[2]});
      d = -(k == 0 ? bt.x : k == 1 ? bt.y : bt.th);
    }
    acc += (a ? P.vel_prior_w : P.conf_prior_w) * d * d;
  }
  for (int e = 0; e < nxp; e++) {  // replanner state priors: r^T W r, row k's share
    const size_t xe = (size_t)b * XP_MAX + e;
    if (pb.xp_state[xe] != i || (a && !pb.xp_has_vel[xe])) continue;
    const double* Wm = pb.xp_info + (xe * 2 + a) * D * D + (size_t)k * D;
    const double* tg = pb.xp_target + xe * n + a * D;
    double wr = 0.0, rk = 0.0;
    for (int cc = 0; cc < D; cc++) {
      double rc = zs[a * D + cc] - tg[cc];
      if (lie && !a && cc < 3) {
        const P2 bt = pose2_between(P2{zs[0], zs[1], zs[2]}, P2{tg[0], tg[1], tg[2]});
        rc = -(cc == 0 ? bt.x : cc == 1 ? bt.y : bt.th);
      }
      wr = fma(Wm[cc], rc, wr);
      if (cc == k) rk = rc;
    }
    acc += wr * rk;
  }
  double H;
  if (!a && P.flag_pos_limit && !(lie && k < 3)) {
    const double e = hinge_limit(z, P.pos_lo[k], P.pos_hi[k], P.pos_th[k], H);
    acc += P.pos_w[k] * e * e;
  }
  if (a && P.flag_vel_limit) {
    const double e = hinge_limit(z, -P.vel_lim[k], P.vel_lim[k], P.vel_th[k], H);
    acc += P.vel_w[k] * e * e;
  }
  if (a && k == 1 && P.vdyn_w > 0.0) acc += P.vdyn_w * z * z;
  return acc;
}
// without limit / dynamics factors and replanner priors only the first and the last state carry terms
__device__ __forceinline__ bool misc_every_state(const PlanParams& P, int nxp) {
  return P.flag_pos_limit || P.flag_vel_limit || P.vdyn_w > 0.0 || nxp > 0;
}
// this thread's share when `nthr` threads split the entries (not yet reduced)
__device__ __forceinline__ double misc_error_partial(const PlanParams& P, const PlanBuffers& pb, int b,
                                                     const double* __restrict__ tr, int tid, int nthr) {
  const int n = P.n, N = P.N;
  double acc = 0.0;
  const int nxp = pb.xp_n[b];
  const bool every_state = misc_every_state(P, nxp);
  const int count = every_state ? (N + 1) * n : (N > 0 ? 2 * n : n);
  for (int q = tid; q < count; q += nthr) {
    const int idx = (every_state || q < n) ? q : N * n + (q - n);
    const int i = idx / n, rho = idx - i * n;
    acc = misc_entry_add(acc, P, pb, b, nxp, i, rho, tr + (size_t)i * n);
  }
  return acc;
}
__device__ __forceinline__ double misc_error(const PlanParams& P, const PlanBuffers& pb, int b,
                                             const double* __restrict__ tr, int lane) {
  return wave_sum(misc_error_partial(P, pb, b, tr, lane, 64));
}

// total graph error of trajectory b from its point records: 0.5 * (sum e_p + sum gp energy + misc)
__device__ __forceinline__ double total_error(const PlanParams& P, const PlanBuffers& pb, int b,
                                              const double* __restrict__ tr,
                                              const double* __restrict__ rec,
                                              const double* __restrict__ gpu, int lane) {
  const double* eb = rec + (size_t)b * P.Ppad * P.RECS + (P.NG + P.D);
  double acc = 0.0;
  for (int p = lane; p < P.P; p += 64) acc += eb[(size_t)p * P.RECS];
  const double* gb = gpu + (size_t)b * P.Npad * P.GPS + P.n;
  for (int i = 1 + lane; i <= P.N; i += 64) acc += gb[(size_t)i * P.GPS];
  return 0.5 * (wave_sum(acc) + misc_error(P, pb, b, tr, lane));
}

// the same with the work split over the `nthr` threads of a workgroup: this thread's share of
// sum e_p + sum gp energy + misc (the caller reduces and halves)
__device__ __forceinline__ double total_error_partial(const PlanParams& P, const PlanBuffers& pb, int b,
                                                      const double* __restrict__ tr, const double* __restrict__ rec,
                                                      const double* __restrict__ gpu, int tid, int nthr) {
  const double* eb = rec + (size_t)b * P.Ppad * P.RECS + (P.NG + P.D);
  double acc = 0.0;
  for (int p = tid; p < P.P; p += nthr) acc += eb[(size_t)p * P.RECS];
  const double* gb = gpu + (size_t)b * P.Npad * P.GPS + P.n;
  for (int i = 1 + tid; i <= P.N; i += nthr) acc += gb[(size_t)i * P.GPS];
  return acc + misc_error_partial(P, pb, b, tr, tid, nthr);
}

// Dogleg only: the trial point in the making is a retry from the linearization already factorised (a smaller trust
// radius after a rejected point), so everything up to the solve is skipped.  LM counts its calls in the same word.
__device__ __forceinline__ bool dogleg_retry(const PlanParams& P, const PlanBuffers& pb, int b) {
  return P.rules.opt_type == GPMP2MI_OPT_DOGLEG && pb.phase[b] != 0;
}

// End of the batch of loads at the head of a pass kernel.  The loads written above this line are issued above it (the
// compiler may not sink a load past what might be a store), and the uniform words named here pass through this point
// together: every use of one of them comes after the arrival of all, so the batch costs one round trip and one wait,
// whatever order the tests below come in.  (Left to itself the scheduler put the test of `active`, and with it a wait,
// in front of the request for `which`.)  No instruction of its own.
__device__ __forceinline__ void head_batch_end(int& a, int& b, int& c) {
  asm volatile("" : "+s"(a), "+s"(b), "+s"(c)::"memory");
}
__device__ __forceinline__ void head_batch_end(int& a, int& b, int& c, int& d) {
  asm volatile("" : "+s"(a), "+s"(b), "+s"(c), "+s"(d)::"memory");
}

// Graph error of trajectory b from the per-chunk shares k_linearize_arm left (pb.cshare): chunks in ascending order,
// (obstacle + GP) + misc of each, halved -- acc = 0; acc += t_q for q = 0 .. nchunk - 1.  In two halves, for the head of a
// pass kernel.  shares_request: lane q of the calling wavefront asks for the three shares of chunk q -- one batch of
// vector loads, issued together with the trajectory's other scalars and before any of them is tested.  (As uniform
// loads in one batch the row took 60 scalar registers and pushed k_gn_step_cr into scratch; as the loop it was before, a
// chain of dependent loads behind `active`.)  error_from_shares forms t_q in lane q and adds the lanes' values in that
// order, so every lane holds the same value, with the bits of the plain loop: no barrier.  Chunks past the 64th finish
// from memory.
struct ShareHead {
  double a, g, m;
};
__device__ __forceinline__ ShareHead shares_request(const PlanBuffers& pb, int b, int nchunk, int lane) {
  const double* __restrict__ cs = pb.cshare + ((size_t)b * nchunk + lane) * 3;
  ShareHead h{0.0, 0.0, 0.0};
  if (lane < nchunk) {
    h.a = cs[0];
    h.g = cs[1];
    h.m = cs[2];
  }
  return h;
}
__device__ __forceinline__ double error_from_shares(const ShareHead& h, const PlanBuffers& pb, int b, int nchunk) {
  const double t = (h.a + h.g) + h.m;
  const int lo = __double2loint(t), hi = __double2hiint(t);
  double acc = 0.0;
  const int nq = min(nchunk, 64);
  for (int q = 0; q < nq; q++)
    acc += __hiloint2double(__builtin_amdgcn_readlane(hi, q), __builtin_amdgcn_readlane(lo, q));
  const double* __restrict__ cs = pb.cshare + (size_t)b * nchunk * 3;
  for (int q = 64; q < nchunk; q++) acc += (cs[3 * q] + cs[3 * q + 1]) + cs[3 * q + 2];
  return 0.5 * acc;
}

// block-wide deterministic sum over the WAVES wavefronts of a workgroup (a wave sum, then the per-wave partials in
// wave order); every thread returns the total.  red: WAVES doubles of LDS.
template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
  v = wave_sum(v);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int k = 0; k < WAVES; k++) t += red[k];
  return t;
}

// =============================================================================== trial-step tail
// The end of a trial step, shared by the block solvers (k_solve_step of both tile forms, k_dense_tail); all nthr
// threads (WAVES wavefronts) of the trajectory's workgroup call it.  The solution x of the linearization is read from
// xsrc and the gradient from gv, block i at offset i * X (X = 0: packed at stride n, and x is staged into xs on the
// way).  xs (LDS) holds the step the trial point is retracted along; red: WAVES doubles of LDS.
//   resolve (all but a Dogleg retry): delta = x and the step-control sums SC_GD, SC_DD, SC_GG, SC_GN, SC_NN (GN, NN:
//            of the Newton step)
//   LM / GN: trial = cur (+) x                           (LevenbergMarquardtOptimizer::tryLambda up to the retract)
//   Dogleg : xs = dogleg point of g and delta for the trust radius pb.lambda[b] (SC_GHG must be set),
//            trial = cur (+) xs, SC_Q, SC_XNORM
template <int WAVES, int X>
__device__ __forceinline__ void trial_step_tail(const PlanParams& P, const PlanBuffers& pb, int b, int n, int D,
                                                bool resolve, const double* xsrc, double* xs, const double* gv,
                                                double* red, int tid, int nthr) {
  const size_t tsz = (size_t)(P.N + 1) * n;
  const double* cur = pb.cur + b * tsz;
  double* trial = pb.trial + b * tsz;
  double* delta = pb.delta + b * tsz;
  double* sc = pb.scal + (size_t)b * SC_COUNT;
  const int xstride = X ? X : n;
  auto off = [&](size_t k) -> size_t {   // entry k = i n + rho of the trajectory in xsrc / xs / gv
    if constexpr (X == 0) {
      return k;
    } else {
      const int i = (int)(k / n), rho = (int)(k - (size_t)i * n);
      return i * X + rho;
    }
  };
  if (resolve) {
    double gd = 0.0, dd = 0.0, gg = 0.0;
    for (size_t k = tid; k < tsz; k += nthr) {
      const size_t o = off(k);
      const double x = xsrc[o], gk = gv[o];
      if constexpr (X == 0) xs[o] = x;
      delta[k] = x;
      gd = fma(gk, x, gd);
      dd = fma(x, x, dd);
      gg = fma(gk, gk, gg);
    }
    gd = block_sum<WAVES>(gd, red, tid);
    dd = block_sum<WAVES>(dd, red, tid);
    gg = block_sum<WAVES>(gg, red, tid);
    if (tid == 0) {
      sc[SC_GD] = gd;
      sc[SC_DD] = dd;
      sc[SC_GG] = gg;
      sc[SC_GN] = gd;
      sc[SC_NN] = dd;
    }
    __syncthreads();
  }
  const bool dogleg = P.rules.opt_type == GPMP2MI_OPT_DOGLEG;
  double q = 0.0, xn = 0.0;
  if (dogleg) {
    double cu, cn;
    dogleg_blend(sc[SC_GG], sc[SC_GHG], sc[SC_GN], sc[SC_NN], pb.lambda[b], cu, cn, q);
    __syncthreads();
    for (size_t k = tid; k < tsz; k += nthr) {
      const size_t o = off(k);
      const double x = cu * gv[o] + cn * delta[k];
      xs[o] = x;
      xn = fma(x, x, xn);
    }
    __syncthreads();
  }
  for (size_t k = tid; k < tsz; k += nthr) {
    const int i = (int)(k / n), rho = (int)(k - (size_t)i * n);
    const double* zs = cur + (size_t)i * n;
    const double* dz = xs + i * xstride;
    trial[k] = (rho < D) ? retract_coord(P.lie != 0, rho, zs, dz) : zs[rho] + dz[rho];
  }
  if (!dogleg) return;
  xn = block_sum<WAVES>(xn, red, tid);
  if (tid == 0) {
    sc[SC_Q] = q;
    sc[SC_XNORM] = sqrt(xn);
  }
}

// Called by one thread of every workgroup of the kernel that closes a pass, after its own work: the last
// workgroup to arrive publishes the pass's active count to the host-mapped flag array, so the host
// driver learns it without a copy command or an event in the stream.  `continues`: 1 when the workgroup's trajectory
// keeps iterating.
// Arrival and count travel in one word (pass_counter.h), added to with one relaxed device-scope atomic: the add that
// returns grid - 1 earlier arrivals also returns their counts, so there is a single location and nothing to order --
// no fence in any workgroup.  The flag store is system scope because the host polls it, but it releases no data: the
// host uses the count only to decide what to enqueue next on the same stream, where stream order makes this kernel's
// writes visible to the next one, and it reads results only after hipStreamSynchronize.
__device__ __forceinline__ void publish_pass_count(const PlanBuffers& pb, int pass, int continues) {
  const unsigned long long before = __hip_atomic_fetch_add(pb.pass_word + pass, (unsigned long long)pass_arrival(continues),
                                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (pass_arrived_last(before, (int)gridDim.x)) {
    const int v = pass_count(before, continues);
    pb.n_active[pass] = v;
    __hip_atomic_store(pb.host_flags + pass, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace g2
