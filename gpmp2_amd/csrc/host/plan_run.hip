// plan_run.hip -- what a plan does once it exists: set_problem, the pass drivers (plain and queue) with the flag wait,
// get_result, the evaluation calls, replanning and plan_update, the one-shot call, timing.
#include <chrono>
#include <cstdlib>

#include "host.h"

using namespace g2;

// linearize `traj` into record buffer `bufsel` of every (active) trajectory: the fused obstacle / GP-prior kernel,
// then -- only for plans that carry extra factors -- the workspace / self-collision factor kernels on the support
// states and their accumulation into the unary records, and the moving-sphere factor of a non-empty resident set
// (moving_kernels.hip), the self-collision factor of a non-empty resident pair table (selfpair_kernels.hip) and the
// workspace-path factor of a resident path (path_kernels.hip) and the carried-object factor of a non-empty resident set
// (carried_kernels.hip), which add their terms to the same records without storing rows
// dst / pass: fused finish (launch_linearize); the extra-factor kernels then run on the NEW states in dst
int g2::plan_linearize(gpmp2mi_plan* p, const double* traj, int bufsel, const int* active, hipStream_t st, double* dst,
                       int pass, bool trial) {
  const PlanParams& P = p->hp;
  G2_TRY(launch_linearize(p->robot->h, p->robot->d, p->sdf->h, P, p->pb, traj, bufsel, active, st, dst, pass, trial));
  if (!p->has_extras) return GPMP2MI_OK;
  if (dst) traj = dst;
  const PlanExtras& ex = p->ex;
  const RobotDev& h = p->robot->h;
  const int M = P.B * (P.N + 1), D = P.D, L = h.nr_links, S = h.nr_spheres;
  if (ex.n_ws > 0) {
    G2_TRY(launch_fk(h, p->robot->d, M, traj, ex.poses, ex.Jp, st, 2 * D));
    for (int f = 0; f < ex.n_ws; f++)
      G2_TRY(launch_workspace_prior(ex.ws_mode[f], ex.ws_link[f], L, D, M, ex.des + 16 * f, ex.poses, ex.Jp,
                                    ex.ws_err + (size_t)f * M * 6, ex.ws_H + (size_t)f * M * 6 * D, st));
  }
  // the sphere centres and their Jacobians: once, for the self-collision rows, the moving spheres and the pair table
  if (ex.n_sc > 0 || ex.mv_K > 0 || ex.sp_P > 0)
    G2_TRY(launch_sphere_centers(h, p->robot->d, M, traj, ex.cen, ex.Jc, st, 2 * D));
  if (ex.n_sc > 0)
    G2_TRY(launch_self_collision(ex.n_sc, S, D, M, ex.sc_data, ex.radius, ex.cen, ex.Jc, ex.sc_err, ex.sc_H, st));
  // the accumulations follow each other on the stream: no two of them touch a record concurrently
  if (ex.n_ws > 0 || ex.n_sc > 0) G2_TRY(launch_extra_accumulate(P, p->pb, ex, L, S, bufsel, active, st));
  G2_TRY(launch_moving_accumulate(P, p->pb, ex, S, bufsel, active, st));   // nothing for an empty set
  G2_TRY(launch_selfpair_accumulate(P, p->pb, ex, S, bufsel, active, st));   // nothing for an empty table
  // the workspace path (path_kernels.hip): nothing without a constrained state
  G2_TRY(launch_path_accumulate(h, p->robot->d, P, p->pb, ex, traj, bufsel, active, st));
  // the carried object (carried_kernels.hip), last: nothing for an empty set
  return launch_carried_accumulate(h, p->robot->d, p->sdf->h, P, p->pb, ex, traj, bufsel, active, st);
}

// Active-trajectory count of a finished pass.  The closing kernel of every pass publishes it to a pinned,
// device-mapped flag (publish_pass_count), so there is no copy command or event in the stream; the host spins
// on the flag, falls back to the stream state if the flag never arrives (a faulted kernel) and gives up after a
// wall-clock limit (GPMP2MI_WAIT_TIMEOUT_MS, default 5000) so that a hung kernel cannot hang the caller.
static double wait_timeout_seconds() {
  const char* e = getenv("GPMP2MI_WAIT_TIMEOUT_MS");
  const double ms = e ? atof(e) : 5000.0;
  return (ms > 0 ? ms : 5000.0) * 1e-3;
}
// `st_valid` false: no stream to query (the host-only test hook gpmp2mi_debug_wait_flag)
int g2::spin_wait_flag(const volatile int* flag, bool st_valid, hipStream_t st, double timeout_s, int* count) {
  const auto t0 = std::chrono::steady_clock::now();
  double next_query = 2e-3;
  for (long spin = 0;; spin++) {
    const int v = __atomic_load_n(flag, __ATOMIC_ACQUIRE);
    if (v >= 0) {
      *count = v;
      return GPMP2MI_OK;
    }
    if ((spin & 0xfff) == 0xfff) {
      const double el0 = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      // A stream query is not free on the device side: with work pending the runtime answers it through a marker
      // packet (barrier + completion signal) at the tail of the queue, i.e. between this pass and the next one
      // (rocprofv3 trace: 5.6 us of idle queue per pass boundary when the query ran on every check).  The query only
      // serves to notice a faulted stream early, so it starts after 2 ms of waiting and then runs every 2 ms.
      if (st_valid && el0 >= next_query) {
        next_query = el0 + 2e-3;
        const hipError_t e = hipStreamQuery(st);
        if (e == hipSuccess) {  // everything enqueued has run: the flag must be there now
          const int w = __atomic_load_n(flag, __ATOMIC_ACQUIRE);
          G2_CHECK(w >= 0, GPMP2MI_ERR_HIP, "pass count was never published");
          *count = w;
          return GPMP2MI_OK;
        }
        if (e != hipErrorNotReady) G2_HIP(e);
      }
      const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (el > timeout_s) {
        set_error("timed out after " + std::to_string((int)(el * 1e3)) +
                  " ms waiting for a pass to finish (kernel hung?); GPMP2MI_WAIT_TIMEOUT_MS raises the limit");
        return GPMP2MI_ERR_TIMEOUT;
      }
    }
  }
}
// `flags`: the host-mapped counts of the run (plain: gpmp2mi_plan::h_flags, queue: qflags)
static int wait_pass_count(const int* flags, int pass, hipStream_t st, int* count) {
  return spin_wait_flag(flags + pass, true, st, wait_timeout_seconds(), count);
}

// ---- the pass bodies shared by the plain driver (plan_run_impl) and the queue driver (plan_queue_impl); `pb` is the
// plan's buffers, or a copy whose pass-indexed arrays point elsewhere (queue runs)
// Gauss-Newton fast path, one pass: assemble, the step kernel (step control + solve), and k_finish_step on the split
// path without the fused finish.  `states`: the states of the pass.  The closing pass of a fixed-iteration round solves
// nothing: it only needs the error of the final values, which the linearization's shares already hold (early stop:
// nothing is launched in front of the step kernel) or k_error_parts sums.
static int enqueue_gn_pass(gpmp2mi_plan* p, const PlanBuffers& pb, int pass, double* states, hipStream_t st) {
  const PlanParams& P = p->hp;
  const PlanForms& F = p->forms;
  const bool early = F.early_stop(p->has_extras);
  if (P.rules.fixed_iters > 0 && pass % (P.rules.fixed_iters + 1) == P.rules.fixed_iters) {
    if (!early) {
      p->timer.begin("final_error", st);
      G2_TRY(launch_error_parts(P, pb, states, 0, pb.active, st));
    }
  } else {
    p->timer.begin("assemble", st);
    G2_TRY(launch_assemble(P, pb, states, 0, pb.active, st, early));
  }
  p->timer.begin("gn_step_cr", st);
  G2_TRY(launch_gn_step_cr(P, pb, pass, st, early));
  if (F.split_back && !F.fuse_finish) {
    p->timer.begin("finish_step", st);
    G2_TRY(launch_finish_step(P, pb, pass, st));
  }
  return GPMP2MI_OK;
}

// trial-step path, one pass up to the decision: assemble (+ g^T H g) -> solve + trial point -> linearize(trial) into
// the spare buffer
static int enqueue_trial_pass(gpmp2mi_plan* p, const PlanBuffers& pb, hipStream_t st) {
  const PlanParams& P = p->hp;
  const PlanForms& F = p->forms;
  if (F.dense) {
    // dof 12..18, or forced for 8..11: dense normal equations + cyclic reduction over dense blocks
    p->timer.begin("export_dense", st);
    G2_TRY(launch_export_normal_eq(P, pb, pb.cur, 0, pb.wHd, pb.wHo, pb.wg, st, pb.active));
    p->timer.begin("solve_dense", st);
    G2_TRY(launch_solve_dense(P, pb, st));
  } else if (F.wide) {
    // blocks wider than one tile (8 <= dof <= 11): the same cyclic reduction on 2x2 tiles
    p->timer.begin("assemble_wide", st);
    G2_TRY(launch_assemble_wide(P, pb, pb.cur, 0, pb.active, st));
    if (P.rules.opt_type == GPMP2MI_OPT_DOGLEG) {
      p->timer.begin("ghg_wide", st);
      G2_TRY(launch_ghg_wide(P, pb, st));
    }
    for (int h = 2; h < P.wide_h0; h *= 2) {
      p->timer.begin(h == 2 ? "cr_level2_wide" : "cr_level4_wide", st);
      G2_TRY(launch_cr_level_wide(P, pb, h, st));
    }
    p->timer.begin("solve_step_wide", st);
    G2_TRY(launch_solve_step_wide(P, pb, st));
    if (F.finish_trial(P.rules.opt_type)) {   // levels 4, 2, 1, step and trial point chip-wide
      p->timer.begin("finish_trial_wide", st);
      G2_TRY(launch_finish_trial_wide(P, pb, st));
    }
  } else {
    p->timer.begin("assemble", st);
    G2_TRY(launch_assemble(P, pb, pb.cur, 0, pb.active, st));
    if (P.rules.opt_type == GPMP2MI_OPT_DOGLEG) {
      p->timer.begin("ghg", st);
      G2_TRY(launch_ghg(P, pb, st));
    }
    p->timer.begin("solve_step", st);
    G2_TRY(launch_solve_step(P, pb, st));
    if (F.finish_trial(P.rules.opt_type)) {   // levels 2, 1, step and trial point chip-wide
      p->timer.begin("finish_trial", st);
      G2_TRY(launch_finish_trial(P, pb, st));
    }
  }
  p->timer.begin("linearize", st);
  if (F.trial_lin_steps(P.rules.opt_type)) {
    // fused finish: the linearization forms the trial point cur (+) delta itself (k_linearize_arm, `trial`)
    return plan_linearize(p, pb.cur, 1, pb.active, st, pb.trial, 1, true);
  }
  return plan_linearize(p, pb.trial, 1, pb.active, st);
}

// Fused finish (F.fuse_finish): there is no k_finish_step; the linearization of pass k applies the step of pass k - 1
// itself, reading the states of pass k - 1 from one of the plan's two state buffers and writing those of pass k to
// the other -- cur / last swap roles every pass, the step kernel picks them by the parity of its pass number.
static double* states_of(const gpmp2mi_plan* p, int pass) {
  return (p->forms.fuse_finish && (pass & 1)) ? p->pb.last : p->pb.cur;
}
// the linearization that opens Gauss-Newton pass `pass` (fast path)
static int enqueue_gn_lin(gpmp2mi_plan* p, int pass, hipStream_t st) {
  p->timer.begin("linearize", st);
  if (p->forms.fuse_finish && pass > 0)
    return plan_linearize(p, states_of(p, pass - 1), 0, p->pb.active, st, states_of(p, pass), pass);
  return plan_linearize(p, p->pb.cur, 0, p->pb.active, st);
}

// the optimizer driver: `cur` holds the starting values; `update`: gpmp2mi_plan_update's fixed Gauss-Newton steps
static int plan_run_impl(gpmp2mi_plan* p, hipStream_t st, const double* start, bool update) {
  const PlanParams& P = p->hp;
  const PlanForms& F = p->forms;
  PlanBuffers& pb = p->pb;
  p->timer.reset();
  for (int k = 0; k < p->n_active_len; k++) p->h_flags[k] = -1;  // the previous run has drained (stream sync below)
  G2_TRY(launch_plan_reset(P, pb, start, st));
  const int iter_cap = (P.rules.fixed_iters > 0 ? P.rules.fixed_iters : P.rules.max_iter);
  if (P.rules.opt_type == GPMP2MI_OPT_GAUSS_NEWTON && F.gn_fast(update)) {
    // ---- Gauss-Newton fast path: 3 launches per pass, step control fused into the solve kernel.
    // Software-pipelined driver: the linearization of pass k+1 is enqueued before the host looks at the active count of
    // pass k, which it learns while the GPU still has the finish kernel of pass k and that linearization (~23 us) to run,
    // so the GPU never waits for the host.  When pass k finished every trajectory, the enqueued linearization is a no-op
    // (all workgroups exit on active[b] == 0).
    const int max_pass = iter_cap + 1;
    G2_TRY(enqueue_gn_lin(p, 0, st));
    for (int pass = 0; pass < max_pass; pass++) {
      G2_TRY(enqueue_gn_pass(p, pb, pass, states_of(p, pass), st));
      if (pass + 1 == max_pass) break;
      G2_TRY(enqueue_gn_lin(p, pass + 1, st));   // ahead of the count
      p->timer.close(st);
      int cnt = 0;
      G2_TRY(wait_pass_count(p->h_flags, pass, st, &cnt));
      if (cnt == 0) break;
    }
    p->timer.close(st);
  } else {
    // ---- generic trial-step path (LM, Dogleg; GN on wide plans or when forced): per pass
    //   assemble (+ g^T H g) -> solve + trial point -> linearize(trial) into the spare buffer -> decide
    // LM may retry an iterate with a larger lambda, Dogleg with a smaller radius, hence the cap.
    const int max_pass = p->n_active_len - 1;
    p->timer.begin("linearize", st);
    G2_TRY(plan_linearize(p, pb.cur, 0, pb.active, st));
    p->timer.begin("decide", st);
    G2_TRY(launch_decide(P, pb, 0, true, st));
    p->timer.close(st);
    for (int pass = 1; pass < max_pass; pass++) {
      G2_TRY(enqueue_trial_pass(p, pb, st));
      p->timer.begin("decide", st);
      G2_TRY(launch_decide(P, pb, pass, false, st));
      p->timer.close(st);
      if (pass >= 2) {
        int cnt = 0;
        G2_TRY(wait_pass_count(p->h_flags, pass - 1, st, &cnt));
        if (cnt == 0) break;
      }
    }
    // pass budget spent with trajectories still iterating (many consecutive rejected trial steps): they
    // finish with their current values and status MAX_ITER instead of returning a stale `result`
    G2_TRY(launch_finalize_unfinished(P, pb, st));
  }
  G2_HIP(hipStreamSynchronize(st));
  if (p->timer.enabled) p->timer.collect();
  p->optimized = true;
  return GPMP2MI_OK;
}
// The wrapper of both drivers: `driver` enqueues on `st` and follows the passes.  `stage` (queue runs from host arrays):
// staging a hung kernel may still write, leaked with the plan.
template <class Driver>
static int guarded_run(gpmp2mi_plan* p, hipStream_t st, QueueStage* stage, Driver driver) {
  p->mark_dirty(st);
  const int rc = driver();
  if (rc == GPMP2MI_ERR_TIMEOUT) {
    // The stream may hold a kernel that never finishes: waiting for it here (or in gpmp2mi_plan_destroy) would hang
    // the caller after all.  The plan is poisoned instead: no further runs, no wait and no recycling at destroy.
    p->poisoned = true;
    if (stage) stage->leak();
    return rc;
  }
  // any other error: the next run resets the host flags assuming the stream has drained
  if (rc != GPMP2MI_OK) (void)hipStreamSynchronize(st);
  p->mark_clean(st);   // both drivers end with a stream synchronisation as well
  return rc;
}
static int plan_run(gpmp2mi_plan* p, hipStream_t st, const double* start, bool update) {
  G2_PLAN_LIVE(p);
  return guarded_run(p, st, nullptr, [&] { return plan_run_impl(p, st, start, update); });
}

// ---- queue runs (gpmp2mi_plan_optimize_queue): M problems through the B slots.  The passes are those of
// plan_run_impl, on a copy of the plan's buffers whose pass-indexed arrays are sized for the run; after the kernel that
// closes a pass, k_queue_scan and k_queue_refill harvest the finished slots and load the next problems, and the host
// follows the count k_queue_scan publishes (active slots + problems not loaded yet) instead of the step kernels'.
static int plan_queue_impl(gpmp2mi_plan* p, hipStream_t st, QueueRun q, int* passes_out) {
  const PlanParams& P = p->hp;
  const PlanForms& F = p->forms;
  const int B = P.B;
  const bool gn = P.rules.opt_type == GPMP2MI_OPT_GAUSS_NEWTON && F.gn_fast(false);
  const int iter_cap = (P.rules.fixed_iters > 0 ? P.rules.fixed_iters : P.rules.max_iter);
  // passes one problem may take: the fast path ends every trajectory by pass iter_cap; the trial-step path gives each
  // problem the plain run's budget of n_active_len - 2 iterative passes (its first one shares a pass with the initial
  // evaluation), then finishes it as k_finalize_unfinished does
  q.budget = gn ? 0 : p->n_active_len - 2;
  const long per = gn ? iter_cap + 1 : q.budget;
  // while problems wait, every slot is busy, so that phase takes at most M per / B passes; the last problems then
  // take at most `per` more (fixed-iteration rounds: ceil(M / B) (iter_cap + 1))
  const long cap_l = ((long)q.M * per + B - 1) / B + per + 2;
  G2_CHECK(cap_l <= (1L << 26), GPMP2MI_ERR_UNSUPPORTED, "too many problems for one queue run");
  const int cap = (int)cap_l;

  // workspace: busy counter, job / next / act / fresh / qpass [B], head, then (from the next 8-byte boundary) the step
  // kernels' pass_word [cap] (64-bit words), n_active / host_flags [cap] (device memory: the host reads k_queue_scan's
  // counts instead)
  const size_t slot_ints = (5 * (size_t)B + 1 + 1) & ~(size_t)1;
  const size_t bytes = sizeof(long long) + slot_ints * sizeof(int) + (size_t)cap * (sizeof(unsigned long long) + 2 * sizeof(int));
  G2_TRY(p->ws[p->WS_QUEUE].reserve(bytes));
  if (p->qflags.cap < cap) {
    flags_release(p->qflags);
    p->qflags = FlagBuf{};
    G2_TRY(flags_acquire(cap, &p->qflags));
  }
  q.busy = (long long*)p->ws[p->WS_QUEUE].p;
  int* w = (int*)(q.busy + 1);
  q.job = w;
  q.next = w + B;
  q.act = w + 2 * B;
  q.fresh = w + 3 * B;
  q.qpass = w + 4 * B;
  q.head = w + 5 * B;
  PlanBuffers qb = p->pb;
  qb.pass_word = (unsigned long long*)(w + slot_ints);
  qb.n_active = (int*)(qb.pass_word + cap);
  qb.host_flags = qb.n_active + cap;
  q.flags = p->qflags.dev;
  for (int k = 0; k < cap; k++) p->qflags.host[k] = -1;   // the previous run has drained
  G2_HIP(hipMemsetAsync(qb.pass_word, 0, (size_t)cap * (sizeof(unsigned long long) + 2 * sizeof(int)), st));

  const PlanBuffers& pb = p->pb;
  p->timer.reset();
  G2_TRY(launch_queue_reset(P, qb, q, st));
  G2_TRY(launch_queue_refill(P, qb, q, pb.cur, st));   // slots 0 .. min(M, B) - 1 take problems 0 ..
  auto refill = [&](int pass, bool load, double* states) -> int {
    p->timer.begin("queue_scan", st);
    G2_TRY(launch_queue_scan(P, qb, q, pass, load, st));
    p->timer.begin("queue_refill", st);
    return launch_queue_refill(P, qb, q, states, st);
  };
  int passes = 0;
  if (gn) {
    // Gauss-Newton fast path: a fresh slot's first evaluation is the step kernel's iters == 0 branch.  A new problem's
    // initial values go where the next pass's linearization reads the states (states_of(pass)).  Fixed-iteration plans
    // load only at the boundary that closes a round.
    G2_TRY(enqueue_gn_lin(p, 0, st));
    for (int pass = 0;; pass++) {
      G2_CHECK(pass < cap, GPMP2MI_ERR_HIP, "queue run exceeded its pass bound");
      G2_TRY(enqueue_gn_pass(p, qb, pass, states_of(p, pass), st));
      const bool load = P.rules.fixed_iters == 0 || pass % (P.rules.fixed_iters + 1) == P.rules.fixed_iters;
      G2_TRY(refill(pass, load, states_of(p, pass)));
      G2_TRY(enqueue_gn_lin(p, pass + 1, st));   // ahead of the count
      p->timer.close(st);
      passes = pass + 1;
      int cnt = 0;
      G2_TRY(wait_pass_count(p->qflags.host, pass, st, &cnt));
      if (cnt == 0) break;
    }
  } else {
    // trial-step path: the slots loaded at the last boundary (fresh) get the plain run's pass 0 -- linearization at
    // the initial values and the decide-init -- at the head of the pass, then join its trial step
    for (int pass = 0;; pass++) {
      G2_CHECK(pass < cap, GPMP2MI_ERR_HIP, "queue run exceeded its pass bound");
      p->timer.begin("linearize_fresh", st);
      G2_TRY(plan_linearize(p, pb.cur, 0, q.fresh, st));
      p->timer.begin("decide_fresh", st);
      G2_TRY(launch_queue_first(P, qb, q, pass, st));
      G2_TRY(enqueue_trial_pass(p, qb, st));
      p->timer.begin("decide", st);
      G2_TRY(launch_decide(P, qb, pass, false, st));
      G2_TRY(refill(pass, true, pb.cur));
      p->timer.close(st);
      passes = pass + 1;
      if (pass >= 1) {
        int cnt = 0;
        G2_TRY(wait_pass_count(p->qflags.host, pass - 1, st, &cnt));
        if (cnt == 0) {
          passes = pass;   // this pass found nothing to do
          break;
        }
      }
    }
  }
  G2_HIP(hipStreamSynchronize(st));
  if (p->timer.enabled) p->timer.collect();
  *passes_out = passes;
  return GPMP2MI_OK;
}

void KernelTimer::collect() {
  names.clear();
  ms.clear();
  launches.clear();
  for (size_t i = 0; i + 1 < recs.size(); i++) {
    if (!recs[i].name) continue;
    float t = 0;
    if (hipEventElapsedTime(&t, recs[i].ev, recs[i + 1].ev) != hipSuccess) continue;
    size_t k = 0;
    for (; k < names.size(); k++)
      if (names[k] == recs[i].name) break;
    if (k == names.size()) {
      names.push_back(recs[i].name);
      ms.push_back(0.0);
      launches.push_back(0);
    }
    ms[k] += t;
    launches[k] += 1;
  }
  cnames.clear();
  for (auto& s : names) cnames.push_back(s.c_str());
}

int QueueStage::alloc(int M, const QueueRun& io, int D_, size_t trow, int T_) {
  D = D_, tr = trow, T = T_;
  const size_t m = M, md = m * D, mt = m * tr;
  const size_t nd = 4 * md + mt + (io.traj ? mt : 0) + (io.final_err ? m : 0) + (io.trace ? m * T : 0);
  const size_t ni = (io.iters ? m : 0) + (io.status ? m : 0);
  G2_TRY(dev_malloc(&base, nd * sizeof(double) + ni * sizeof(int)));
  double* d = (double*)base;
  auto take = [&](size_t cnt) { double* r = d; d += cnt; return r; };
  q.M = M;
  q.start_conf = take(md); q.start_vel = take(md); q.end_conf = take(md); q.end_vel = take(md); q.init = take(mt);
  if (io.traj) q.traj = take(mt);
  if (io.final_err) q.final_err = take(m);
  if (io.trace) q.trace = take(m * T);
  int* i = (int*)d;
  if (io.iters) q.iters = i, i += m;
  if (io.status) q.status = i;
  return GPMP2MI_OK;
}
int QueueStage::upload(const QueueRun& io, size_t j, hipStream_t st, bool with_init) const {
  const size_t md = (size_t)q.M * D * sizeof(double);
  G2_HIP(hipMemcpyAsync((void*)q.start_conf, io.start_conf + j * D, md, hipMemcpyHostToDevice, st));
  G2_HIP(hipMemcpyAsync((void*)q.start_vel, io.start_vel + j * D, md, hipMemcpyHostToDevice, st));
  G2_HIP(hipMemcpyAsync((void*)q.end_conf, io.end_conf + j * D, md, hipMemcpyHostToDevice, st));
  G2_HIP(hipMemcpyAsync((void*)q.end_vel, io.end_vel + j * D, md, hipMemcpyHostToDevice, st));
  if (with_init) G2_HIP(hipMemcpyAsync((void*)q.init, io.init + j * tr, q.M * tr * sizeof(double), hipMemcpyHostToDevice, st));
  return GPMP2MI_OK;
}
int QueueStage::download(const QueueRun& io, size_t j, hipStream_t st) const {
  const size_t m = q.M;
  if (q.traj) G2_HIP(hipMemcpyAsync(io.traj + j * tr, q.traj, m * tr * sizeof(double), hipMemcpyDeviceToHost, st));
  if (q.iters) G2_HIP(hipMemcpyAsync(io.iters + j, q.iters, m * sizeof(int), hipMemcpyDeviceToHost, st));
  if (q.final_err) G2_HIP(hipMemcpyAsync(io.final_err + j, q.final_err, m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (q.status) G2_HIP(hipMemcpyAsync(io.status + j, q.status, m * sizeof(int), hipMemcpyDeviceToHost, st));
  if (q.trace) G2_HIP(hipMemcpyAsync(io.trace + j * T, q.trace, m * T * sizeof(double), hipMemcpyDeviceToHost, st));
  return GPMP2MI_OK;
}

int g2::plan_set_problem(gpmp2mi_plan* p, const double* sc, const double* sv, const double* ec, const double* ev,
                         const double* init, hipMemcpyKind kind, hipStream_t st) {
  G2_CHECK(p && sc && sv && ec && ev && init, GPMP2MI_ERR_INVALID, "null argument");
  G2_PLAN_LIVE(p);
  const size_t bd = (size_t)p->hp.B * p->hp.D * sizeof(double);
  G2_HIP(hipMemcpyAsync(p->pb.start_conf, sc, bd, kind, st));
  G2_HIP(hipMemcpyAsync(p->pb.start_vel, sv, bd, kind, st));
  G2_HIP(hipMemcpyAsync(p->pb.end_conf, ec, bd, kind, st));
  G2_HIP(hipMemcpyAsync(p->pb.end_vel, ev, bd, kind, st));
  G2_HIP(hipMemcpyAsync(p->pb.init, init, p->tsz() * sizeof(double), kind, st));
  G2_TRY(p->close_copies(kind, st));
  p->problem_set = true;
  p->optimized = false;
  return GPMP2MI_OK;
}

int g2::plan_optimize_queue(gpmp2mi_plan* p, QueueRun io, bool host, hipStream_t st) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_CHECK(io.M >= 1, GPMP2MI_ERR_INVALID, "queue: M must be >= 1");
  G2_CHECK(io.start_conf && io.start_vel && io.end_conf && io.end_vel && io.init, GPMP2MI_ERR_INVALID, "queue: null input");
  G2_PLAN_LIVE(p);
  const PlanParams& P = p->hp;
  for (int b = 0; b < P.B; b++) {
    G2_CHECK(p->h_xp_n[b] == 0, GPMP2MI_ERR_INVALID,
             "queue: slot " + std::to_string(b) + " carries state priors (fix_state / add_state_estimate): clear them with "
             "gpmp2mi_plan_clear_state_priors first");
    G2_CHECK(!p->goal_removed[b], GPMP2MI_ERR_INVALID,
             "queue: the goal of slot " + std::to_string(b) + " was removed (remove_goal): restore it with "
             "gpmp2mi_plan_change_goal first");
  }
  QueueStage stage;
  if (host) {
    // host variant: the M problems are staged once, the results come back once
    G2_TRY(stage.alloc(io.M, io, P.D, (size_t)(P.N + 1) * P.n, P.rules.max_iter + 1));
    G2_TRY(stage.upload(io, 0, st));   // if it fails half-way, ~QueueStage's hipFree waits for the copies in flight
  }
  const QueueRun q = host ? stage.q : io;
  // the resident problem is overwritten slot by slot
  p->problem_set = false;
  p->optimized = false;
  p->queue_ran = false;
  int passes = 0;
  G2_TRY(guarded_run(p, st, host ? &stage : nullptr, [&] { return plan_queue_impl(p, st, q, &passes); }));
  p->qstats.passes = passes;
  p->qstats.slot_passes = (long)P.B * passes;
  G2_HIP(hipMemcpy(&p->qstats.busy_slot_passes, p->ws[p->WS_QUEUE].p, sizeof(long long), hipMemcpyDeviceToHost));
  p->queue_ran = true;
  if (host) {
    G2_TRY(stage.download(io, 0, st));   // (the same on a failure here)
    G2_HIP(hipStreamSynchronize(st));
  }
  return GPMP2MI_OK;
}

int g2::plan_get_result(gpmp2mi_plan* p, double* traj, int* iters, double* ferr, int* status, double* trace,
                        hipMemcpyKind kind, hipStream_t st) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_PLAN_LIVE(p);
  G2_CHECK(p->optimized, GPMP2MI_ERR_INVALID, "plan has not been optimized");
  const int B = p->hp.B;
  if (traj) G2_HIP(hipMemcpyAsync(traj, p->pb.result, p->tsz() * sizeof(double), kind, st));
  if (iters) G2_HIP(hipMemcpyAsync(iters, p->pb.iters, B * sizeof(int), kind, st));
  if (ferr) G2_HIP(hipMemcpyAsync(ferr, p->pb.final_err, B * sizeof(double), kind, st));
  if (status) G2_HIP(hipMemcpyAsync(status, p->pb.status, B * sizeof(int), kind, st));
  if (trace)
    G2_HIP(hipMemcpyAsync(trace, p->pb.trace, (size_t)B * (p->hp.rules.max_iter + 1) * sizeof(double), kind, st));
  return p->close_copies(kind, st);
}

static int plan_add_prior(gpmp2mi_plan* p, int b, int state, const double* conf, const double* Wc, const double* vel,
                          const double* Wv) {
  G2_CHECK(p && conf && Wc, GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK(b >= 0 && b < p->hp.B && state >= 0 && state <= p->hp.N, GPMP2MI_ERR_INVALID, "index out of range");
  G2_CHECK(p->h_xp_n[b] < XP_MAX, GPMP2MI_ERR_UNSUPPORTED, "too many state priors on this trajectory");
  const int D = p->hp.D, n = p->hp.n, e = p->h_xp_n[b];
  const size_t xe = (size_t)b * XP_MAX + e;
  std::vector<double> tg(n, 0.0), info(2 * D * D, 0.0);
  std::copy(conf, conf + D, tg.begin());
  std::copy(Wc, Wc + D * D, info.begin());
  const int has_vel = (vel && Wv) ? 1 : 0;
  if (has_vel) {
    std::copy(vel, vel + D, tg.begin() + D);
    std::copy(Wv, Wv + D * D, info.begin() + D * D);
  }
  G2_HIP(hipMemcpy(p->pb.xp_target + xe * n, tg.data(), n * sizeof(double), hipMemcpyHostToDevice));
  G2_HIP(hipMemcpy(p->pb.xp_info + xe * 2 * D * D, info.data(), info.size() * sizeof(double), hipMemcpyHostToDevice));
  G2_HIP(hipMemcpy(p->pb.xp_state + xe, &state, sizeof(int), hipMemcpyHostToDevice));
  G2_HIP(hipMemcpy(p->pb.xp_has_vel + xe, &has_vel, sizeof(int), hipMemcpyHostToDevice));
  p->h_xp_n[b] = e + 1;
  G2_HIP(hipMemcpy(p->pb.xp_n + b, &p->h_xp_n[b], sizeof(int), hipMemcpyHostToDevice));
  return GPMP2MI_OK;
}

extern "C" {

int gpmp2mi_plan_set_problem(gpmp2mi_plan* p, const double* sc, const double* sv, const double* ec,
                             const double* ev, const double* init) {
  return plan_set_problem(p, sc, sv, ec, ev, init, hipMemcpyHostToDevice, nullptr);
}
int gpmp2mi_plan_set_problem_dev(gpmp2mi_plan* p, const double* sc, const double* sv, const double* ec,
                                 const double* ev, const double* init, void* stream) {
  return plan_set_problem(p, sc, sv, ec, ev, init, hipMemcpyDeviceToDevice, (hipStream_t)stream);
}

int gpmp2mi_plan_optimize(gpmp2mi_plan* p, void* stream) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  G2_CHECK(p->problem_set, GPMP2MI_ERR_INVALID, "call gpmp2mi_plan_set_problem first");
  return plan_run(p, (hipStream_t)stream, p->pb.init, false);   // cur = init is part of the reset kernel
}
int gpmp2mi_plan_get_result(gpmp2mi_plan* p, double* traj, int* iters, double* ferr, int* status, double* trace) {
  return plan_get_result(p, traj, iters, ferr, status, trace, hipMemcpyDeviceToHost, nullptr);
}
int gpmp2mi_plan_get_result_dev(gpmp2mi_plan* p, double* traj, int* iters, double* ferr, int* status, void* stream) {
  return plan_get_result(p, traj, iters, ferr, status, nullptr, hipMemcpyDeviceToDevice, (hipStream_t)stream);
}
const double* gpmp2mi_plan_traj_dev(const gpmp2mi_plan* p) { return p ? p->pb.result : nullptr; }

int gpmp2mi_plan_optimize_queue(gpmp2mi_plan* p, int M, const double* start_conf, const double* start_vel,
                                const double* end_conf, const double* end_vel, const double* init, double* traj,
                                int* iters, double* final_error, int* status, double* error_trace) {
  const QueueRun io{M, 0, start_conf, start_vel, end_conf, end_vel, init, traj, iters, final_error, status, error_trace};
  return plan_optimize_queue(p, io, true, nullptr);
}
int gpmp2mi_plan_optimize_queue_dev(gpmp2mi_plan* p, int M, const double* start_conf, const double* start_vel,
                                    const double* end_conf, const double* end_vel, const double* init, double* traj,
                                    int* iters, double* final_error, int* status, double* error_trace, void* stream) {
  const QueueRun io{M, 0, start_conf, start_vel, end_conf, end_vel, init, traj, iters, final_error, status, error_trace};
  return plan_optimize_queue(p, io, false, (hipStream_t)stream);
}
int gpmp2mi_plan_queue_stats(const gpmp2mi_plan* p, gpmp2mi_queue_stats* out) {
  G2_CHECK(p && out, GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK(p->queue_ran, GPMP2MI_ERR_INVALID, "no queue run on this plan yet");
  *out = p->qstats;
  return GPMP2MI_OK;
}

int gpmp2mi_plan_graph_error(gpmp2mi_plan* p, const double* traj, double* err) {
  G2_CHECK(p && traj && err, GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK(p->problem_set, GPMP2MI_ERR_INVALID, "call gpmp2mi_plan_set_problem first");
  DevBuf<double> dt, de;
  G2_TRY(dt.upload(traj, p->tsz()));
  G2_TRY(de.out(err, p->hp.B));
  G2_TRY(plan_linearize(p, dt.p, 1, nullptr, nullptr));
  G2_TRY(launch_error_reduce(p->hp, p->pb, dt.p, 1, de.p, nullptr));
  return fetch_all(de);
}

int gpmp2mi_plan_linearize(gpmp2mi_plan* p, const double* traj, double* Hdiag, double* Hoff, double* g, double* err) {
  G2_CHECK(p && traj, GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK(p->problem_set, GPMP2MI_ERR_INVALID, "call gpmp2mi_plan_set_problem first");
  const PlanParams& P = p->hp;
  const size_t nb = (size_t)P.B * (P.N + 1), n = P.n;
  DevBuf<double> dt, dd, dob, dg, de;
  G2_TRY(dt.upload(traj, p->tsz()));
  if (Hdiag) G2_TRY(dd.out(Hdiag, nb * n * n));
  if (Hoff) G2_TRY(dob.out(Hoff, (size_t)P.B * P.N * n * n));
  if (g) G2_TRY(dg.out(g, nb * n));
  if (err) G2_TRY(de.out(err, P.B));
  // evaluate into the spare record buffer (the one that does not hold the linearization at `cur`)
  const PlanBuffers& pb = p->pb;
  G2_TRY(plan_linearize(p, dt.p, 1, nullptr, nullptr));
  G2_TRY(launch_export_normal_eq(P, pb, dt.p, 1, dd.p, dob.p, dg.p, nullptr));
  if (err) G2_TRY(launch_error_reduce(P, pb, dt.p, 1, de.p, nullptr));
  return fetch_all(dd, dob, dg, de);
}

// -------------------------------------------------------------------------------------------- replanning
int gpmp2mi_plan_fix_state(gpmp2mi_plan* p, int b, int state_idx, const double* conf, const double* vel) {
  G2_CHECK(p && conf && vel, GPMP2MI_ERR_INVALID, "null argument");
  const int D = p->hp.D;
  std::vector<double> Wc(D * D, 0.0), Wv(D * D, 0.0);
  for (int k = 0; k < D; k++) {
    Wc[k * D + k] = p->hp.conf_prior_w;
    Wv[k * D + k] = p->hp.vel_prior_w;
  }
  return plan_add_prior(p, b, state_idx, conf, Wc.data(), vel, Wv.data());
}

int gpmp2mi_plan_add_state_estimate(gpmp2mi_plan* p, int b, int state_idx, const double* conf, const double* conf_cov,
                                    const double* vel, const double* vel_cov) {
  G2_CHECK(p && conf && conf_cov, GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK((vel == nullptr) == (vel_cov == nullptr), GPMP2MI_ERR_INVALID, "pass vel and vel_cov together");
  const int D = p->hp.D;
  std::vector<double> Wc(D * D), Wv(D * D);
  G2_CHECK(invert_small(D, conf_cov, Wc.data()), GPMP2MI_ERR_INVALID, "pose covariance is singular");
  if (vel) G2_CHECK(invert_small(D, vel_cov, Wv.data()), GPMP2MI_ERR_INVALID, "velocity covariance is singular");
  return plan_add_prior(p, b, state_idx, conf, Wc.data(), vel, vel ? Wv.data() : nullptr);
}

int gpmp2mi_plan_change_goal(gpmp2mi_plan* p, int b, const double* goal_conf, const double* goal_vel) {
  G2_CHECK(p && goal_conf && goal_vel && b >= 0 && b < p->hp.B, GPMP2MI_ERR_INVALID, "bad argument");
  const int D = p->hp.D, one = 1;
  G2_HIP(hipMemcpy(p->pb.end_conf + (size_t)b * D, goal_conf, D * sizeof(double), hipMemcpyHostToDevice));
  G2_HIP(hipMemcpy(p->pb.end_vel + (size_t)b * D, goal_vel, D * sizeof(double), hipMemcpyHostToDevice));
  G2_HIP(hipMemcpy(p->pb.goal_on + b, &one, sizeof(int), hipMemcpyHostToDevice));
  p->goal_removed[b] = 0;
  return GPMP2MI_OK;
}

int gpmp2mi_plan_remove_goal(gpmp2mi_plan* p, int b) {
  G2_CHECK(p && b >= 0 && b < p->hp.B, GPMP2MI_ERR_INVALID, "bad argument");
  const int zero = 0;
  G2_HIP(hipMemcpy(p->pb.goal_on + b, &zero, sizeof(int), hipMemcpyHostToDevice));
  p->goal_removed[b] = 1;
  return GPMP2MI_OK;
}

int gpmp2mi_plan_clear_state_priors(gpmp2mi_plan* p, int b) {
  G2_CHECK(p && b >= 0 && b < p->hp.B, GPMP2MI_ERR_INVALID, "bad argument");
  p->h_xp_n[b] = 0;
  G2_HIP(hipMemcpy(p->pb.xp_n + b, &p->h_xp_n[b], sizeof(int), hipMemcpyHostToDevice));
  return GPMP2MI_OK;
}

int gpmp2mi_plan_update(gpmp2mi_plan* p, int iterations, void* stream) {
  G2_CHECK(p && iterations > 0, GPMP2MI_ERR_INVALID, "bad argument");
  G2_CHECK(p->problem_set, GPMP2MI_ERR_INVALID, "call gpmp2mi_plan_set_problem first");
  G2_CHECK(iterations <= p->hp.rules.max_iter, GPMP2MI_ERR_INVALID, "iterations exceeds max_iter");
  G2_CHECK(iterations + 3 <= p->n_active_len, GPMP2MI_ERR_INVALID, "iterations exceeds the plan's pass budget");
  hipStream_t st = (hipStream_t)stream;
  // warm start: the previous estimate becomes the initial values of this run
  const double* from = p->optimized ? p->pb.result : p->pb.init;
  // temporarily switch the resident parameters to `iterations` fixed Gauss-Newton steps
  PlanParams saved = p->hp;
  p->hp.rules.opt_type = GPMP2MI_OPT_GAUSS_NEWTON;
  p->hp.rules.fixed_iters = iterations;
  if (const int rc0 = launch_set_mode(p->pb, p->hp.rules.opt_type, p->hp.rules.fixed_iters, st)) {
    p->hp = saved;
    return rc0;
  }
  const int rc = plan_run(p, st, from, true);
  p->hp = saved;
  G2_TRY(launch_set_mode(p->pb, p->hp.rules.opt_type, p->hp.rules.fixed_iters, st));
  G2_HIP(hipStreamSynchronize(st));
  return rc;
}

int gpmp2mi_batch_optimize(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, const gpmp2mi_settings* s,
                           const gpmp2mi_graph_opts* o, int B, const double* sc, const double* sv,
                           const double* ec, const double* ev, const double* init, double* traj_out,
                           int* iters, double* ferr, int* status) {
  gpmp2mi_plan* p = nullptr;
  int rc = gpmp2mi_plan_create(robot, sdf, s, o, B, &p);
  if (rc) return rc;
  rc = gpmp2mi_plan_set_problem(p, sc, sv, ec, ev, init);
  if (!rc) rc = gpmp2mi_plan_optimize(p, nullptr);
  if (!rc) rc = gpmp2mi_plan_get_result(p, traj_out, iters, ferr, status, nullptr);
  gpmp2mi_plan_destroy(p);
  return rc;
}

int gpmp2mi_plan_enable_timing(gpmp2mi_plan* p, int enable) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  p->timer.enabled = enable != 0;
  return GPMP2MI_OK;
}
int gpmp2mi_plan_get_timing(gpmp2mi_plan* p, int* n, const char** names, double* ms, int* launches) {
  G2_CHECK(p && n, GPMP2MI_ERR_INVALID, "null argument");
  const int cap = *n;
  const int have = (int)p->timer.names.size();
  *n = have;
  for (int i = 0; i < std::min(cap, have); i++) {
    if (names) names[i] = p->timer.cnames[i];
    if (ms) ms[i] = p->timer.ms[i];
    if (launches) launches[i] = p->timer.launches[i];
  }
  return GPMP2MI_OK;
}

}  // extern "C"
