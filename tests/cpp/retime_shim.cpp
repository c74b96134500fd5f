// C entry point around gpmp2_amd/csrc/retime_rule.h for the CPU tests (tests/retime_shim.py): the kernels' own text of
// the re-timing rule, built by the host compiler with -ffp-contract=off.  Nothing else lives here.
#include "retime_rule.h"

extern "C" {

// One row of gpmp2mi_retime_path on the host; K [Md][2] are the controllable sets.  Returns the status.
int shim_retime_path(int Md, int D, const double* qd, const double* qdd_left, const double* qdd_right, const double* cap,
                     const double* acc, double h, double max_rate, double rate_start, double rate_end, double* K,
                     double* sdot, double* u, double* stamps, double* duration, double* achieved) {
  return g2::retime_path_row(Md, D, qd, qdd_left, qdd_right, cap, acc, h, max_rate, rate_start, rate_end, K, sdot, u,
                             stamps, duration, achieved);
}

}  // extern "C"
