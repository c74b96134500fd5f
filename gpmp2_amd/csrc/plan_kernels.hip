// plan_kernels.hip -- the small kernels of a plan's pass around the linearization (linearize_kernels.hip), the assembly
// and the solve (cr_kernels.hip, dense_kernels.hip), with their launchers:
//   extra factors : k_extra_accumulate adds workspace-prior / goal / self-collision rows to the records of their states
//   error         : k_error_reduce (whole graph error), k_error_parts (closing pass of a fixed-iteration run)
//   run state     : k_set_mode, k_plan_reset
//   step control  : k_decide -- the gpmp2::optimize / gtsam::checkConvergence control flow on the trial point
//                   (planner/BatchTrajOptimizer.cpp:273-307; rules: step_control.h), k_finalize_unfinished
//   queue runs    : k_queue_reset / first / scan / refill
//   parity        : k_export_normal_eq (dense H, g from the records), k_block_tridiag_solve (generic block solve)
#include "device_math.h"
#include "dispatch.h"
#include "plan.h"
#include "tiles.h"
#include "assembler.h"
#include "cr_schedule.h"
#include "plan_device.h"

namespace g2 {

// =============================================================================== extra factors
// One lane per (trajectory, support state): adds the whitened normal-equation terms of the workspace priors /
// goal factor / self-collision rows of that state to the record of its unary evaluation point
// (p = i (I + 1)): G += H^T H / sigma^2, g += H^T r / sigma^2, e += r^T r / sigma^2.  The residuals and Jacobians come
// from the factor kernels (k_fk + k_workspace_prior, k_sphere_centers + k_self_collision) run on the states.
__global__ __launch_bounds__(64) void k_extra_accumulate(const PlanParams* __restrict__ pp, PlanBuffers pb, PlanExtras ex,
                                                          int bufsel, const int* __restrict__ active) {
  const PlanParams& P = *pp;
  const int N = P.N, D = P.D, M = P.B * (N + 1);
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const int b = m / (N + 1), i = m - b * (N + 1);
  if (active && !active[b]) return;
  double* rec = rec_of(pb, pb.which[b], bufsel) + ((size_t)b * P.Ppad + (size_t)i * (P.I + 1)) * P.RECS;
  auto add_rows = [&](const double* err, const double* H, int rows, const double* w, double wu) {
    // rows x D Jacobian H (row-major), residual err; weight w[r] per row (or the uniform wu when w == nullptr)
    double e = 0.0;
    for (int r = 0; r < rows; r++) e += (w ? w[r] : wu) * err[r] * err[r];
    rec[P.NG + D] += e;
    for (int k = 0; k < D; k++) {
      double g = 0.0;
      for (int r = 0; r < rows; r++) g += (w ? w[r] : wu) * H[r * D + k] * err[r];
      rec[P.NG + k] += g;
      for (int k2 = k; k2 < D; k2++) {
        double a = 0.0;
        for (int r = 0; r < rows; r++) a += (w ? w[r] : wu) * H[r * D + k] * H[r * D + k2];
        rec[k * D - (k * (k - 1)) / 2 + (k2 - k)] += a;
      }
    }
  };
  for (int f = 0; f < ex.n_ws; f++) {
    if (i < ex.ws_first[f] || i > ex.ws_last[f]) continue;
    const int rows = ex.ws_mode[f] == GPMP2MI_WORKSPACE_POSE ? 6 : 3;
    // (k_workspace_prior packs `rows` per state; every factor owns a slice sized for 6)
    add_rows(ex.ws_err + (size_t)f * M * 6 + (size_t)m * rows, ex.ws_H + ((size_t)f * M * 6 + (size_t)m * rows) * D, rows,
             nullptr, ex.ws_w[f]);
  }
  if (ex.n_sc > 0 && i >= ex.sc_first && i <= ex.sc_last)
    add_rows(ex.sc_err + (size_t)m * ex.n_sc, ex.sc_H + (size_t)m * ex.n_sc * D, ex.n_sc, ex.sc_w, 0.0);
}

int launch_extra_accumulate(const PlanParams& hp, const PlanBuffers& pb, const PlanExtras& ex, int L, int S, int bufsel,
                            const int* active, hipStream_t st) {
  const int M = hp.B * (hp.N + 1);
  k_extra_accumulate<<<dim3((M + 63) / 64), dim3(64), 0, st>>>(pb.params, pb, ex, bufsel, active);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

__global__ __launch_bounds__(64) void k_error_reduce(const PlanParams* __restrict__ pp, PlanBuffers pb,
                                                      const double* __restrict__ traj, int bufsel,
                                                      double* __restrict__ err) {
  const PlanParams& P = *pp;
  const int b = blockIdx.x, lane = threadIdx.x;
  const double e = total_error(P, pb, b, traj + (size_t)b * (P.N + 1) * P.n, rec_of(pb, pb.which[b], bufsel),
                               gpu_of(pb, pb.which[b], bufsel), lane);
  if (lane == 0) err[b] = e;
}

int launch_error_reduce(const PlanParams& hp, const PlanBuffers& pb, const double* traj, int bufsel,
                        double* err, hipStream_t st) {
  k_error_reduce<<<dim3(hp.B), dim3(64), 0, st>>>(pb.params, pb, traj, bufsel, err);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}


// The closing pass of a run with a fixed number of iterations only evaluates the error of the final values (every
// trajectory stops in the step kernel before it factorises anything): instead of k_assemble, which would build and
// eliminate all blocks for nothing, this kernel leaves the graph error of each active trajectory where the step kernel
// looks for it -- the whole sum in the share of block 0, zeros in the others.  Only plans whose step control reads
// pb.epart launch it: with the early stop (per-chunk shares of k_linearize_arm in pb.cshare) the closing pass runs
// nothing between the linearization and the step kernel.
__global__ __launch_bounds__(256) void k_error_parts(const PlanParams* __restrict__ pp, PlanBuffers pb,
                                                      const double* __restrict__ traj, int bufsel,
                                                      const int* __restrict__ active) {
  const PlanParams& P = *pp;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (active && !active[b]) return;
  __shared__ double red[4];
  const double part = total_error_partial(P, pb, b, traj + (size_t)b * (P.N + 1) * P.n, rec_of(pb, pb.which[b], bufsel),
                                          gpu_of(pb, pb.which[b], bufsel), tid, 256);
  const double ws = wave_sum(part);
  if ((tid & 63) == 0) red[tid >> 6] = ws;
  __syncthreads();
  const double e = 0.5 * (((red[0] + red[1]) + red[2]) + red[3]);   // the fixed-order sum of k_decide
  for (int i = tid; i <= P.N; i += 256) pb.epart[(size_t)b * P.Npad + i] = (i == 0) ? e : 0.0;
}

int launch_error_parts(const PlanParams& hp, const PlanBuffers& pb, const double* traj, int bufsel, const int* active,
                       hipStream_t st) {
  k_error_parts<<<dim3(hp.B), dim3(256), 0, st>>>(pb.params, pb, traj, bufsel, active);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

// gpmp2mi_plan_update switches the resident parameter block to `iterations` fixed Gauss-Newton steps and back: two
// words, written in stream order by this kernel instead of re-uploading the block from pageable host memory twice
__global__ void k_set_mode(PlanParams* pp, int opt_type, int fixed_iters) {
  pp->rules.opt_type = opt_type;
  pp->rules.fixed_iters = fixed_iters;
}
int launch_set_mode(const PlanBuffers& pb, int opt_type, int fixed_iters, hipStream_t st) {
  k_set_mode<<<dim3(1), dim3(1), 0, st>>>(pb.params, opt_type, fixed_iters);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

// the per-trajectory scalars of a fresh run (k_plan_reset; k_queue_refill when it loads a slot)
__device__ __forceinline__ void reset_slot(const PlanParams& P, const PlanBuffers& pb, size_t b) {
  pb.iters[b] = 0;
  pb.status[b] = GPMP2MI_TRAJ_MAX_ITER;
  pb.active[b] = 1;
  pb.phase[b] = 0;
  pb.which[b] = 0;
  pb.stepped[b] = 0;
  pb.notspd[b] = 0;
  pb.cur_err[b] = pb.prev_err[b] = pb.last_err[b] = pb.final_err[b] = 0.0;
  pb.lambda[b] = (P.rules.opt_type == GPMP2MI_OPT_DOGLEG) ? P.rules.dl_delta0 : P.rules.lm_lambda0;
}

// reset the optimizer state before a run and load the starting values: cur = start (no separate copy command in
// the stream); grid-stride over the flat index ranges so that no thread writes a long serial run
__global__ __launch_bounds__(256) void k_plan_reset(const PlanParams* __restrict__ pp, PlanBuffers pb,
                                                    const double* __restrict__ start) {
  const PlanParams& P = *pp;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  const size_t B = P.B;
  if (start) {
    const size_t tot = B * (size_t)(P.N + 1) * P.n;
    for (size_t k = tid; k < tot; k += nth) pb.cur[k] = start[k];
  }
  for (size_t k = tid; k < (size_t)P.max_pass; k += nth) {
    pb.n_active[k] = 0;
    pb.pass_word[k] = 0;
  }
  for (size_t k = tid; k < B * SC_COUNT; k += nth) pb.scal[k] = 0.0;
  for (size_t k = tid; k < B * (size_t)(P.rules.max_iter + 1); k += nth) pb.trace[k] = __longlong_as_double(0x7ff8000000000000LL);
  for (size_t b = tid; b < B; b += nth) reset_slot(P, pb, b);
}

int launch_plan_reset(const PlanParams& hp, const PlanBuffers& pb, const double* start, hipStream_t st) {
  const size_t tot = (size_t)hp.B * (hp.N + 1) * hp.n;
  const int blocks = (int)std::min<size_t>(1024, std::max<size_t>(1, (tot + 1023) / 1024));
  k_plan_reset<<<dim3(blocks), dim3(256), 0, st>>>(pb.params, pb, start);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

// =============================================================================== step control
// One wavefront per trajectory.  `init`: error of the initial values + the early exits of
// gpmp2::optimize (planner/BatchTrajOptimizer.cpp:248-268).  Otherwise: the trial point produced by
// k_solve_step has been linearized into the spare record buffer; compute its graph error and apply
//   GaussNewtonOptimizer::iterate      (always accept)
//   LevenbergMarquardtOptimizer::tryLambda  (model fidelity test, lambda *= / /= 10, give up at 1e5)
//   DoglegOptimizerImpl::Iterate(ONE_STEP_PER_ITERATION)  (gain ratio rho, trust radius update)
// followed by the do/while of gpmp2::optimize (checkConvergence, max_iter, no-increase rollback).
// The rules themselves are the pure functions of step_control.h; the first lane loads the trajectory's scalars, calls
// them and stores what changed.
// Returns 1 when the trajectory keeps iterating (uniform over the workgroup): its share of the pass's count.
__device__ __forceinline__ int decide_body(const PlanParams& P, const PlanBuffers& pb, int pass, int init) {
  // 4 wavefronts: all of them sum the graph error of the point in question (fixed-order block reduction),
  // the first thread takes the decision, all four wavefronts then move the trajectories
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const bool w0 = tid < 64;
  __shared__ int dec[2];
  __shared__ double red[4];
  if (!pb.active[b]) return 0;
  const int N = P.N, n = P.n;
  const size_t tsz = (size_t)(N + 1) * n;
  double* cur = pb.cur + b * tsz;
  double* last = pb.last + b * tsz;
  double* trial = pb.trial + b * tsz;
  double* result = pb.result + b * tsz;
  double* sc = pb.scal + (size_t)b * SC_COUNT;
  double* tr = pb.trace + (size_t)b * (P.rules.max_iter + 1);
  const int wh = pb.which[b];
  // action: 0 keep iterating, 1 finish with cur, 2 finish with last; accept: copy trial -> cur
  int action = 0, accept = 0;

  // The trajectory moves at the end (last = cur, cur = trial, result = ...) read cur and trial; requested here, they
  // arrive while the error is being summed instead of one dependent load-store pair after another behind the decision.
  constexpr int PF = 10;   // prefetched elements per thread and array (covers (N + 1) n <= 2560)
  double pf_cur[PF], pf_trial[PF];
#pragma unroll
  for (int m = 0; m < PF; m++) {
    const size_t k = tid + (size_t)m * 256;
    pf_cur[m] = (k < tsz) ? cur[k] : 0.0;
    pf_trial[m] = (!init && k < tsz) ? trial[k] : 0.0;
  }

  const bool failed = !init && pb.notspd[b] != 0;
  double err_sum = 0.0;
  if (!failed) {
    const double part = init ? total_error_partial(P, pb, b, cur, rec_of(pb, wh, 0), gpu_of(pb, wh, 0), tid, blockDim.x)
                             : total_error_partial(P, pb, b, trial, rec_of(pb, wh, 1), gpu_of(pb, wh, 1), tid, blockDim.x);
    const double ws = wave_sum(part);
    if (lane == 0) red[tid >> 6] = ws;
  }
  __syncthreads();
  if (!failed) err_sum = 0.5 * (((red[0] + red[1]) + red[2]) + red[3]);
  if (w0 && init) {
    const double err = err_sum;
    if (lane == 0) {
      pb.cur_err[b] = pb.prev_err[b] = err;
      tr[0] = err;
      int status;
      action = first_decide(P.rules, err, status);
      if (action) {
        pb.status[b] = status;
        pb.final_err[b] = err;
      }
    }
  } else if (w0) {
    const double new_err = err_sum;
    const int opt = P.rules.opt_type;
    // LM / GN split form: g.delta, |delta|^2, |g|^2 arrive as per-group shares of k_finish_trial (fixed-order wave sums)
    double sp_gd = 0.0, sp_dd = 0.0, sp_gg = 0.0;
    if (P.split_back && opt == GPMP2MI_OPT_LM && !failed) {
      const int groups = P.spart_groups;
      const double* sp = pb.spart + (size_t)b * groups * 3;
      for (int qq = lane; qq < groups; qq += 64) {
        sp_gd += sp[3 * qq];
        sp_dd += sp[3 * qq + 1];
        sp_gg += sp[3 * qq + 2];
      }
      sp_gd = wave_sum(sp_gd);
      sp_dd = wave_sum(sp_dd);
      sp_gg = wave_sum(sp_gg);
    }
    if (lane == 0) {
      pb.notspd[b] = 0;
      const double cur_err = pb.cur_err[b];
      // one call to the optimizer's iterate() (step_control.h) ...
      TrialOutcome o;
      if (opt == GPMP2MI_OPT_GAUSS_NEWTON) {
        o = gn_iterate(failed);
      } else if (opt == GPMP2MI_OPT_LM) {
        if (P.split_back && !failed) {   // per-group shares of k_finish_trial, summed by wavefront 0 above
          sc[SC_GD] = sp_gd;
          sc[SC_DD] = sp_dd;
          sc[SC_GG] = sp_gg;
        }
        o = lm_try_lambda(P.rules, pb.lambda[b], cur_err, new_err, sc[SC_GD], sc[SC_DD], failed);
        pb.lambda[b] = o.param;
      } else {
        o = dogleg_iterate(pb.lambda[b], cur_err, new_err, sc[SC_Q], sc[SC_XNORM], failed);
        if (!failed) {
          pb.lambda[b] = o.param;
          pb.phase[b] = o.retry ? 1 : 0;
        }
      }
      if (o.not_spd) {
        action = 1;
        pb.status[b] = GPMP2MI_TRAJ_NOT_SPD;
        pb.final_err[b] = cur_err;
      }
      // ... and, once it has returned, the do/while of gpmp2::optimize
      if (o.returned) {
        const double err_after = o.moved ? new_err : cur_err;
        const bool counted = o.moved || opt == GPMP2MI_OPT_DOGLEG;  // LM give-up does not count
        const int it = pb.iters[b] + (counted ? 1 : 0);
        pb.iters[b] = it;
        if (o.moved) accept = 1;
        // trace = error after every call to iterate() (an LM call that gives up repeats the value);
        // LM keeps its call counter in `phase`, which only Dogleg uses otherwise
        const int call = (opt == GPMP2MI_OPT_LM) ? ++pb.phase[b] : it;
        if (call <= P.rules.max_iter) tr[call] = err_after;
        const double prev = pb.prev_err[b];
        int status;
        action = loop_decide(P.rules, it, counted, prev, err_after, status);
        if (action) {
          pb.status[b] = status;
          pb.final_err[b] = (action == 2) ? prev : err_after;
        } else if (P.rules.fixed_iters == 0) {
          pb.prev_err[b] = err_after;   // currentError of the next comparison
        }
        pb.cur_err[b] = err_after;
      }
    }
  }
  if (tid == 0) {
    dec[0] = action;
    dec[1] = accept;
  }
  __syncthreads();
  action = dec[0];
  accept = dec[1];
  // (pf_cur / pf_trial hold the first PF * 256 elements; longer trajectories finish with plain loads)
  if (accept) {
    if (action == 2) {
      // rollback: the result is the pre-step `cur`; nothing else reads cur afterwards
#pragma unroll
      for (int m = 0; m < PF; m++) {
        const size_t k = tid + (size_t)m * 256;
        if (k < tsz) result[k] = pf_cur[m];
      }
      for (size_t k = tid + (size_t)PF * 256; k < tsz; k += 256) result[k] = cur[k];
    } else {
#pragma unroll
      for (int m = 0; m < PF; m++) {
        const size_t k = tid + (size_t)m * 256;
        if (k < tsz) {
          last[k] = pf_cur[m];
          cur[k] = pf_trial[m];
          if (action == 1) result[k] = pf_trial[m];
        }
      }
      for (size_t k = tid + (size_t)PF * 256; k < tsz; k += 256) {
        const double t = trial[k];
        last[k] = cur[k];
        cur[k] = t;
        if (action == 1) result[k] = t;
      }
      if (tid == 0) pb.which[b] = wh ^ 1;  // the trial linearization is now the one at cur
    }
  } else if (action == 1) {
#pragma unroll
    for (int m = 0; m < PF; m++) {
      const size_t k = tid + (size_t)m * 256;
      if (k < tsz) result[k] = pf_cur[m];
    }
    for (size_t k = tid + (size_t)PF * 256; k < tsz; k += 256) result[k] = cur[k];
  } else if (action == 2) {
    for (size_t k = tid; k < tsz; k += blockDim.x) result[k] = last[k];
  }
  if (tid == 0 && action != 0) pb.active[b] = 0;
  return action == 0;
}
__global__ __launch_bounds__(256) void k_decide(const PlanParams* __restrict__ pp, PlanBuffers pb, int pass, int init) {
  const int continues = decide_body(*pp, pb, pass, init);
  if (threadIdx.x == 0) publish_pass_count(pb, pass, continues);
}

int launch_decide(const PlanParams& hp, const PlanBuffers& pb, int pass, bool init, hipStream_t st) {
  k_decide<<<dim3(hp.B), dim3(256), 0, st>>>(pb.params, pb, pass, init ? 1 : 0);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

// Trajectories that are still iterating when the trial-step driver has spent its pass budget: finish them with
// their current values (status MAX_ITER) so that `result` is never stale.  One workgroup per trajectory.
__global__ __launch_bounds__(256) void k_finalize_unfinished(const PlanParams* __restrict__ pp, PlanBuffers pb) {
  const PlanParams& P = *pp;
  const int b = blockIdx.x;
  if (!pb.active[b]) return;
  const size_t tsz = (size_t)(P.N + 1) * P.n;
  for (size_t k = threadIdx.x; k < tsz; k += blockDim.x) pb.result[b * tsz + k] = pb.cur[b * tsz + k];
  if (threadIdx.x == 0) {
    pb.status[b] = GPMP2MI_TRAJ_MAX_ITER;
    pb.final_err[b] = pb.cur_err[b];
    pb.active[b] = 0;
  }
}
int launch_finalize_unfinished(const PlanParams& hp, const PlanBuffers& pb, hipStream_t st) {
  k_finalize_unfinished<<<dim3(hp.B), dim3(256), 0, st>>>(pb.params, pb);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

// =============================================================================== queue runs
// Before the first pass: no slot holds a problem, slot b < M is handed problem b (k_queue_refill loads it).
__global__ __launch_bounds__(256) void k_queue_reset(const PlanParams* __restrict__ pp, PlanBuffers pb, QueueRun q) {
  const int B = pp->B;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    q.job[b] = -1;
    q.act[b] = 0;
    q.next[b] = b < q.M ? b : -1;
    q.fresh[b] = 0;
    q.qpass[b] = 0;
    pb.active[b] = 0;
  }
  if (threadIdx.x == 0) {
    *q.head = min(q.M, B);
    *q.busy = 0;
  }
}
int launch_queue_reset(const PlanParams& hp, const PlanBuffers& pb, const QueueRun& q, hipStream_t st) {
  k_queue_reset<<<dim3(1), dim3(256), 0, st>>>(pb.params, pb, q);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

// Trial-step path: the decide-init of a plain run's pass 0 (error of the initial values, early exits) for the slots
// loaded at the last boundary, after their own first linearization.
__global__ __launch_bounds__(256) void k_queue_first(const PlanParams* __restrict__ pp, PlanBuffers pb,
                                                     const int* __restrict__ fresh, int pass) {
  if (!fresh[blockIdx.x]) return;
  decide_body(*pp, pb, pass, 1);
}
int launch_queue_first(const PlanParams& hp, const PlanBuffers& pb, const QueueRun& q, int pass, hipStream_t st) {
  k_queue_first<<<dim3(hp.B), dim3(256), 0, st>>>(pb.params, pb, q.fresh, pass);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

// After the kernel that closes a pass: which slots finished (act), and which problem each slot takes next.  The slots
// that finished (and those without a problem) take the next problems in ascending slot order: rank = exclusive scan
// of that predicate over the slots.  `load` = 0 holds the new problems back (fixed-iteration plans refill only at the
// boundary that closes a round, so that the slots stay in lockstep).  Publishes the active slots after the refill plus
// the problems not loaded yet; zero ends the run.  One workgroup; thread t owns the slots [t per, (t + 1) per).
__global__ __launch_bounds__(256) void k_queue_scan(const PlanParams* __restrict__ pp, PlanBuffers pb, QueueRun q, int pass,
                                                    int load) {
  constexpr int NT = 256;
  const int B = pp->B, tid = threadIdx.x;
  const int per = (B + NT - 1) / NT, b0 = min(B, tid * per), b1 = min(B, b0 + per);
  const int head = *q.head;
  int elig = 0, still = 0, busy = 0;
  for (int b = b0; b < b1; b++) {
    const int j = q.job[b];
    int a = 0;
    if (j >= 0) {
      busy++;
      if (!pb.active[b]) {
        a = 1;
      } else if (q.budget > 0) {
        const int qp = q.qpass[b] + 1;
        q.qpass[b] = qp;
        if (qp >= q.budget) a = 2;
      }
      if (!a) still++;
    }
    q.act[b] = a;
    if (a || j < 0) elig++;
  }
  __shared__ int scan[NT];
  __shared__ int sums[2];
  if (tid == 0) sums[0] = sums[1] = 0;
  scan[tid] = elig;
  __syncthreads();
  if (still) atomicAdd(&sums[0], still);
  if (busy) atomicAdd(&sums[1], busy);
  for (int d = 1; d < NT; d *= 2) {   // inclusive scan (Hillis-Steele)
    const int v = (tid >= d) ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  int r = scan[tid] - elig;
  for (int b = b0; b < b1; b++) {
    int nj = -1;
    if (q.act[b] || q.job[b] < 0) {
      if (load && head + r < q.M) nj = head + r;
      r++;
    }
    q.next[b] = nj;
  }
  if (tid == 0) {
    const int loaded = load ? min(scan[NT - 1], q.M - head) : 0;
    *q.head = head + loaded;
    *q.busy += sums[1];
    __hip_atomic_store(q.flags + pass, sums[0] + loaded + (q.M - head - loaded), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
int launch_queue_scan(const PlanParams& hp, const PlanBuffers& pb, const QueueRun& q, int pass, bool load, hipStream_t st) {
  k_queue_scan<<<dim3(1), dim3(256), 0, st>>>(pb.params, pb, q, pass, load ? 1 : 0);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

// One workgroup per slot, after k_queue_scan.  A finished problem's result, iterations, status, final error and trace
// row go to its output rows (act 2: the pass budget ran out, and the values are what k_finalize_unfinished would
// leave).  A slot handed a new problem loads its start / end rows and its initial values into `states`, the buffer the
// next pass's first kernel reads (pb.cur; on the fused Gauss-Newton path the states of the pass just closed, which
// k_linearize_arm copies forward for a slot that did not step), and takes the per-trajectory state of a fresh run.
__global__ __launch_bounds__(256) void k_queue_refill(const PlanParams* __restrict__ pp, PlanBuffers pb, QueueRun q,
                                                      double* __restrict__ states) {
  const PlanParams& P = *pp;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int a = q.act[b], nj = q.next[b];
  if (!a && nj < 0) {
    if (tid == 0) q.fresh[b] = 0;
    return;
  }
  const int D = P.D, T = P.rules.max_iter + 1;
  const size_t tsz = (size_t)(P.N + 1) * P.n;
  if (a) {
    const size_t j = q.job[b];
    const double* src = (a == 2 ? pb.cur : pb.result) + b * tsz;
    if (q.traj)
      for (size_t k = tid; k < tsz; k += blockDim.x) q.traj[j * tsz + k] = src[k];
    if (q.trace)
      for (int k = tid; k < T; k += blockDim.x) q.trace[j * T + k] = pb.trace[(size_t)b * T + k];
    if (tid == 0) {
      if (q.iters) q.iters[j] = pb.iters[b];
      if (q.status) q.status[j] = (a == 2) ? GPMP2MI_TRAJ_MAX_ITER : pb.status[b];
      if (q.final_err) q.final_err[j] = (a == 2) ? pb.cur_err[b] : pb.final_err[b];
      pb.active[b] = 0;
    }
    __syncthreads();   // the slot's rows are read before the next problem overwrites them
  }
  if (nj < 0) {
    if (tid == 0) {
      q.job[b] = -1;
      q.fresh[b] = 0;
    }
    return;
  }
  const size_t jn = nj;
  if (tid < D) {
    pb.start_conf[(size_t)b * D + tid] = q.start_conf[jn * D + tid];
    pb.start_vel[(size_t)b * D + tid] = q.start_vel[jn * D + tid];
    pb.end_conf[(size_t)b * D + tid] = q.end_conf[jn * D + tid];
    pb.end_vel[(size_t)b * D + tid] = q.end_vel[jn * D + tid];
  }
  for (size_t k = tid; k < tsz; k += blockDim.x) states[b * tsz + k] = q.init[jn * tsz + k];
  for (int k = tid; k < SC_COUNT; k += blockDim.x) pb.scal[(size_t)b * SC_COUNT + k] = 0.0;
  for (int k = tid; k < T; k += blockDim.x) pb.trace[(size_t)b * T + k] = __longlong_as_double(0x7ff8000000000000LL);
  if (tid == 0) {
    reset_slot(P, pb, b);
    q.job[b] = nj;
    q.fresh[b] = 1;
    q.qpass[b] = 0;
  }
}
int launch_queue_refill(const PlanParams& hp, const PlanBuffers& pb, const QueueRun& q, double* states, hipStream_t st) {
  k_queue_refill<<<dim3(hp.B), dim3(256), 0, st>>>(pb.params, pb, q, states);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

// =============================================================================== export H, g
template <int D, bool LIE>
__global__ __launch_bounds__(64) void k_export_normal_eq(const PlanParams* __restrict__ pp, PlanBuffers pb,
                                                          const double* __restrict__ traj, int bufsel,
                                                          double* __restrict__ Hd, double* __restrict__ Ho,
                                                          double* __restrict__ gout, const int* __restrict__ active) {
  constexpr int n = 2 * D;
  using Asm = Assembler<D, LIE>;
  const PlanParams& P = *pp;
  const int N = P.N;
  const int b = blockIdx.x / (N + 1), i = blockIdx.x - b * (N + 1);
  // optimizer use (wide path): finished trajectories and Dogleg retries keep their last system
  if (active && (!active[b] || dogleg_retry(P, pb, b))) return;
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  extern __shared__ __attribute__((aligned(16))) double asm_smem[];
  Asm as(P, pb, rec_of(pb, pb.which[b], bufsel), gpu_of(pb, pb.which[b], bufsel), b, lane);
  const typename Asm::Slot slot0 = as.make_slot(asm_smem, 0), slot1 = as.make_slot(asm_smem, 1);
  as.stage2(i, slot0, slot1);
  __syncthreads();
  // blocks wider than one tile (2 dof > 15) are walked as 2x2 (3x3 for 2 dof > 31) tiles; the right-hand side
  // rides in the last column of the tile grid
  constexpr int T = (n <= 15) ? 1 : (n <= 31) ? 2 : 3, RC = 16 * T - 1;
  const double* zi = traj + ((size_t)b * (N + 1) + i) * n;
  for (int ti = 0; ti < T; ti++)
    for (int tj = 0; tj < T; tj++) {
      Asm at(P, pb, rec_of(pb, pb.which[b], bufsel), gpu_of(pb, pb.which[b], bufsel), b, lane, 16 * ti, 16 * tj, RC);
      Tile S, Cl, Cr;
      at.build_tiles(i, slot0, slot1, zi, S, Cl, Cr, true);
      const int cc = 16 * tj + c;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int rho = 16 * ti + g + 4 * k;
        if (rho < n && cc < n) {
          if (Hd) Hd[(((size_t)b * (N + 1) + i) * n + rho) * n + cc] = S.r[k];
          // the ABI exports block (i+1, i) = H_{i,i+1}^T
          if (Ho && i < N) Ho[(((size_t)b * N + i) * n + cc) * n + rho] = Cr.r[k];
        }
        if (rho < n && cc == RC && gout) gout[((size_t)b * (N + 1) + i) * n + rho] = -S.r[k];
      }
    }
}

int launch_export_normal_eq(const PlanParams& hp, const PlanBuffers& pb, const double* traj, int bufsel,
                            double* Hd, double* Ho, double* g, hipStream_t st, const int* active) {
  const dim3 grid(hp.B * (hp.N + 1)), block(64);
  const size_t shmem = 2 * (size_t)((hp.I + 1) * hp.RECS + hp.GPS + 24 * hp.I) * sizeof(double);
  switch (hp.D) {
#define G2_EXP_CASE(DD) \
  case DD:                                                                                          \
    if (hp.lie) k_export_normal_eq<DD, true><<<grid, block, shmem, st>>>(pb.params, pb, traj, bufsel, Hd, Ho, g, active); \
    else k_export_normal_eq<DD, false><<<grid, block, shmem, st>>>(pb.params, pb, traj, bufsel, Hd, Ho, g, active);       \
    break;
    G2_EXP_CASE(1) G2_EXP_CASE(2) G2_EXP_CASE(3) G2_EXP_CASE(4) G2_EXP_CASE(5) G2_EXP_CASE(6) G2_EXP_CASE(7)
    G2_EXP_CASE(8) G2_EXP_CASE(9) G2_EXP_CASE(10) G2_EXP_CASE(11) G2_EXP_CASE(17) G2_EXP_CASE(18)
#undef G2_EXP_CASE
    default:
      set_error("normal equations are instantiated for dof <= 11 and 17, 18");
      return GPMP2MI_ERR_UNSUPPORTED;
  }
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

// =============================================================================== generic solve
// gpmp2mi_block_tridiag_solve: dense blocks in, x out; same chain solver.
template <int n>
__global__ __launch_bounds__(64) void k_block_tridiag_solve(int nblk, const double* __restrict__ Hd,
                                                             const double* __restrict__ Ho,
                                                             const double* __restrict__ rhs,
                                                             double* __restrict__ x, int* __restrict__ okf,
                                                             double* __restrict__ scratch) {
  const int b = blockIdx.x, lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const double* D_ = Hd + (size_t)b * nblk * n * n;
  const double* O_ = Ho + (size_t)b * (nblk - 1) * n * n;
  const double* r_ = rhs + (size_t)b * nblk * n;
  const bool ok = chain_solve<n>(
      nblk,
      [&](int i, Tile& Dt, Tile& Wt) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int rho = g + 4 * k;
          double d = 0.0, h = 0.0;
          if (rho < n && c < n) {
            d = D_[((size_t)i * n + rho) * n + c];
            if (i + 1 < nblk) h = O_[((size_t)i * n + c) * n + rho];  // block (i,i+1) = (i+1,i)^T
          }
          if (rho < n && c == RHSCOL) h = r_[(size_t)i * n + rho];
          Dt.r[k] = d;
          Wt.r[k] = h;
        }
      },
      scratch + (size_t)b * nblk * 512, x + (size_t)b * nblk * n, lane);
  if (lane == 0 && okf) okf[b] = ok ? 1 : 0;
}

int launch_block_tridiag_solve(int B, int nblk, int n, const double* Hd, const double* Ho, const double* b,
                               double* x, int* ok, double* scratch, hipStream_t st) {
  const dim3 grid(B), block(64);
  switch (n) {
#define G2_SOLVE_CASE(NN) \
  case NN: k_block_tridiag_solve<NN><<<grid, block, 0, st>>>(nblk, Hd, Ho, b, x, ok, scratch); break;
    G2_SOLVE_CASE(1) G2_SOLVE_CASE(2) G2_SOLVE_CASE(3) G2_SOLVE_CASE(4) G2_SOLVE_CASE(5) G2_SOLVE_CASE(6)
    G2_SOLVE_CASE(7) G2_SOLVE_CASE(8) G2_SOLVE_CASE(9) G2_SOLVE_CASE(10) G2_SOLVE_CASE(11) G2_SOLVE_CASE(12)
    G2_SOLVE_CASE(13) G2_SOLVE_CASE(14) G2_SOLVE_CASE(15)
#undef G2_SOLVE_CASE
    default:
      set_error("block size must be 1..15");
      return GPMP2MI_ERR_UNSUPPORTED;
  }
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

}  // namespace g2
