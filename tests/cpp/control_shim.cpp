// C entry points around gpmp2_amd/csrc/step_control.h and cr_schedule.h for the CPU tests (tests/control_shim.py):
// the product's own text, built by the host compiler.  Nothing else lives here.
#include "cr_schedule.h"
#include "step_control.h"

using namespace g2;

namespace {
// returned | moved << 1 | retry << 2 | not_spd << 3
int flags_of(const TrialOutcome& o) { return (o.returned ? 1 : 0) | (o.moved ? 2 : 0) | (o.retry ? 4 : 0) | (o.not_spd ? 8 : 0); }
}  // namespace

extern "C" {

int shim_check_convergence(double rel, double abs_, double err_tol, double cur, double nw) {
  return check_convergence(rel, abs_, err_tol, cur, nw) ? 1 : 0;
}
int shim_first_decide(const StepRules* R, double err, int* status) { return first_decide(*R, err, *status); }
int shim_loop_decide(const StepRules* R, int it, int counted, double prev, double err_after, int* status) {
  return loop_decide(*R, it, counted != 0, prev, err_after, *status);
}
int shim_gn_decide(const StepRules* R, int it, double prev, double new_err, int* status) {
  return gn_decide(*R, it, prev, new_err, *status);
}
int shim_gn_iterate(int failed) { return flags_of(gn_iterate(failed != 0)); }
int shim_lm_try_lambda(const StepRules* R, double lambda, double cur_err, double new_err, double gd, double dd, int failed,
                       double* lambda_out) {
  const TrialOutcome o = lm_try_lambda(*R, lambda, cur_err, new_err, gd, dd, failed != 0);
  *lambda_out = o.param;
  return flags_of(o);
}
int shim_dogleg_iterate(double Delta, double cur_err, double new_err, double q, double xnorm, int failed,
                        double* Delta_out) {
  const TrialOutcome o = dogleg_iterate(Delta, cur_err, new_err, q, xnorm, failed != 0);
  *Delta_out = o.param;
  return flags_of(o);
}
// out = {cu, cn, q}
void shim_dogleg_blend(double gg, double gHg, double gn, double nn, double Delta, double* out) {
  dogleg_blend(gg, gHg, gn, nn, Delta, out[0], out[1], out[2]);
}

int shim_cr_hfinal(int N) { return cr_hfinal(N); }
// one forward level: elim[idx], block[idx] of its tasks (room for N + 2 each); returns their number; counts = {countE,
// countU, final}
int shim_cr_level(int N, int h, int updates, int* elim, int* block, int* counts) {
  const CrLevel level = cr_level(N, h, updates != 0);
  for (int idx = 0; idx < level.tasks(); idx++) {
    elim[idx] = level.elim(idx) ? 1 : 0;
    block[idx] = level.block(idx);
  }
  counts[0] = level.countE;
  counts[1] = level.countU;
  counts[2] = level.final ? 1 : 0;
  return level.tasks();
}
int shim_cr_back_count(int N, int h) { return cr_back_count(N, h); }
int shim_cr_back_block(int N, int h, int idx) { return cr_back_block(N, h, idx); }

}  // extern "C"
