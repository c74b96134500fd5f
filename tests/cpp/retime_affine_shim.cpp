// C entry points around gpmp2_amd/csrc/retime_affine_rule.h for the CPU tests (tests/retime_affine_shim.py): the kernels'
// own text of the re-timing rule with affine rows, built by the host compiler with -ffp-contract=off.  Nothing else
// lives here.
#include "retime_affine_rule.h"

extern "C" {

// One row of gpmp2mi_retime_path_affine on the host; K [Md][2] are the controllable sets.  Returns the status.
int shim_retime_affine(int Md, int D, int R, const double* qd, const double* qdd_left, const double* qdd_right,
                       const double* cap, const double* acc, const double* cx_left, const double* cx_right,
                       const double* cu, const double* off, const double* bound, double h, double max_rate,
                       double rate_start, double rate_end, double* K, double* sdot, double* u, double* stamps,
                       double* duration, double* achieved) {
  return g2::retime_affine_row(Md, D, R, qd, qdd_left, qdd_right, cap, acc, cx_left, cx_right, cu, off, bound, h,
                               max_rate, rate_start, rate_end, K, sdot, u, stamps, duration, achieved);
}

// (pl, pu, r, xcap) of the row |cx x + cu u + off| <= A, and of the two-sided row |a x + b u| <= A of retime_rule.h
void shim_row_affine(double cx, double cu, double off, double A, double* out) {
  const g2::RetimeRow o = g2::retime_row_affine(cx, cu, off, A);
  out[0] = o.pl, out[1] = o.pu, out[2] = o.r, out[3] = o.xcap;
}
void shim_row(double a, double b, double A, double* out) {
  const g2::RetimeRow o = g2::retime_row(a, b, A);
  out[0] = o.pl, out[1] = o.pu, out[2] = o.r, out[3] = o.xcap;
}

}  // extern "C"
