// retime_dynamic_kernels.hip -- the speed profile of the executed trajectory under joint torque limits, behind
// gpmp2mi_retime_path_affine / gpmp2mi_retime_dynamic_traj (include/gpmp2mi.h "re-timing under torque limits"): the rule
// of retime_kernels.hip with rows that carry an offset, |cx x + cu u + off| <= A.  Along the fixed path the torque of
// joint d is such a row, tau = p u + m x + tau_g with x = sdot^2 and u = sddot.  The rule is retime_affine_rule.h; these
// kernels spread it.  ps comes from k_retime_caps (retime_kernels.hip), unchanged.
//
//   k_retime_coef     tiled as k_torque is: one wavefront, a lane per checked state, SCORE_TILE states per workgroup.
//                     One outward walk in the world frame (the walk of k_torque, described in dyn_walk.h with what the
//                     two share) with three accelerations per lane: (q', q''_right), (q', q''_left) and (0, q').  The third has
//                     no velocity terms and gives p = M(q) q'.  Writes coef [B][Md][4][D] = p, m_left, m_right, tau_g; a
//                     state with one side carries that side twice.  Where q' == 0 exactly p == 0 exactly (every term of
//                     the third walk is a product with a q'), and where q'' == 0 as well m == 0: the rule branches on
//                     cu == 0, so a rounding-level p at a rest state would be another row.
//   k_retime_rows     a lane per (stage, row): (pl, pu, r, xcap) of the 2 D + 2 R rows of every stage that do not
//                     depend on the chain, into the workspace.  Forming rows inside the chain is what k_retime pays per
//                     dependent stage.
//   k_retime_dynamic  one wavefront per row, the chain of k_retime (the stages of retime_chain.h, which both kernels
//                     call): caps, finiteness and the static test, a lane per
//                     state; the chain reads a stage's rows from the workspace (the next stage's are in flight
//                     meanwhile), lane 2 D + 2 R forms the row of the next set, the n^2 pairs are strided over the
//                     lanes; the forward pass; `achieved` [6], the rates, the stamps in index order, the re-timed
//                     velocities and the torques of the re-timed row.
//   k_retime_dynamic_finish  the selection of gpmp2mi_plan_select_retimed_dynamic over the per-row scores the existing
//                     stages left, by select_finish (score_select.h); the chosen row's stamps and torques are copied
//                     and its velocities multiplied by its rates.
//
// Determinism: as retime_kernels.hip.  Set ends and rates are extrema of singly rounded quotients, `achieved` is six
// maxima, the stamps are summed in index order by every lane alike, coef and tau_retimed are per-state values.  A row's
// results do not depend on the batch or the entry point.  No address is computed from data.
#include <climits>

#include "device_math.h"
#include "dispatch.h"
#include "dyn_walk.h"
#include "launch.h"
#include "retime_affine_rule.h"
#include "retime_chain.h"
#include "score_select.h"

namespace g2 {

static_assert(2 * GPMP2MI_MAX_DOF + 2 * 8 + 1 <= 64, "the rows of a stage are one per lane");
static_assert(RETIME_DYN_MAX_ROWS == RETIME_MAX_EXTRA && TORQUE_MAX_AD <= RETIME_MAX_EXTRA, "one affine row per joint");

template <int AD>
__global__ __launch_bounds__(64) void k_retime_coef(const RobotDev* __restrict__ Rg, const DynDev* __restrict__ Dg,
                                                    TorqueLimitsDev lim, double dt, int inter, int N, int Md, int nblk,
                                                    const double* __restrict__ traj, double* __restrict__ coef) {
  constexpr int D = AD;
  __shared__ RobotDev R;
  __shared__ DynDev Dn;
  __shared__ DynLds<AD, 3> S;   // per joint: m of the right side, m of the left side, p and tau_g
  stage_dyn(&Dn, Dg);
  stage_robot(&R, Rg);   // its barrier closes both copies
  const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int lane = threadIdx.x;
  const int m = blk * SCORE_TILE + lane;   // checked state of this lane
  if (m >= Md) return;                     // nothing is shared behind the staging
  const int seg = m / (inter + 1), j = m % (inter + 1);
  const double* s0 = traj + ((size_t)b * (N + 1) + seg) * 2 * D;
  // side 0: q'' seen from the right (the last state: from the left); side 1: from the left, which differs at a support
  // state between two intervals only; side 2: the walk of (0, q')
  const bool two = j == 0 && seg > 0 && seg < N;
  const double* i0 = seg < N ? s0 : s0 - 2 * D;
  const double* i1 = two ? s0 - 2 * D : i0;
  Frame Fr;
  frame_from_3x4(R.base, Fr);
  double w[3] = {0.0, 0.0, 0.0};
  double wd[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  double ao[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  double op[3] = {Fr.t[0], Fr.t[1], Fr.t[2]};   // the origin of the joint before (joint 0: its own, r = 0)
#pragma unroll 1
  for (int l = 0; l < AD; l++) {   // link l hangs from joint l: axis z through o, the frame in front of it
    double x[D + 1], a0, a1, t1[3], t2[3], t3[3];
    score_dense_coord(false, dt, inter, D, j, 0, s0 + l, x);   // coordinate l: x[0] = q, x[D] = v
    const double ql = x[0], vl = x[D];
    retime_acc_ends(dt, i0[2 * D + l] - i0[l], i0[D + l], i0[3 * D + l], a0, a1);
    const double al0 = seg < N ? retime_acc_at(a0, a1, j, inter + 1) : a1;
    retime_acc_ends(dt, i1[2 * D + l] - i1[l], i1[D + l], i1[3 * D + l], a0, a1);
    const double al1 = two ? a1 : al0;
    const double z[3] = {Fr.c2[0], Fr.c2[1], Fr.c2[2]}, o[3] = {Fr.t[0], Fr.t[1], Fr.t[2]};
#pragma unroll
    for (int i = 0; i < 3; i++) {
      S.ax[6 * l + i][lane] = z[i];
      S.ax[6 * l + 3 + i][lane] = o[i];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) S.tq[4 * l + i][lane] = 0.0;
    // o and the origin before it both ride on link l-1
    const double r[3] = {o[0] - op[0], o[1] - op[1], o[2] - op[2]};
    cross3(w, r, t2);
    cross3(w, t2, t3);
#pragma unroll
    for (int s = 0; s < 3; s++) {
      cross3(wd[s], r, t1);
#pragma unroll
      for (int i = 0; i < 3; i++) ao[s][i] += s < 2 ? t1[i] + t3[i] : t1[i];
    }
    cross3(w, z, t1);   // the velocity product of wd, with w of the link before
#pragma unroll
    for (int i = 0; i < 3; i++) {
      wd[0][i] += z[i] * al0 + t1[i] * vl;
      wd[1][i] += z[i] * al1 + t1[i] * vl;
      wd[2][i] += z[i] * vl;
      w[i] += z[i] * vl;
      op[i] = o[i];
    }
    dh_advance(Fr, ql + R.bias[l], R.a[l], R.d[l], R.ca[l], R.sa[l]);   // as Kin::walk_links advances
    const double* cl = Dn.com + 3 * l;
    double c[3], rc[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      c[i] = Fr.t[i] + Fr.c0[i] * cl[0] + Fr.c1[i] * cl[1] + Fr.c2[i] * cl[2];
      rc[i] = c[i] - o[i];
    }
    cross3(w, rc, t2);
    cross3(w, t2, t3);
    // the gyroscopic moment wl x Ibar wl in the link frame, wl = R^T w
    const double mass = Dn.mass[l];
    const double* I = Dn.inertia + 6 * l;   // ixx iyy izz ixy ixz iyz
    const double wl[3] = {dot3(Fr.c0, w), dot3(Fr.c1, w), dot3(Fr.c2, w)};
    const double Iw[3] = {I[0] * wl[0] + I[3] * wl[1] + I[4] * wl[2], I[3] * wl[0] + I[1] * wl[1] + I[5] * wl[2],
                          I[4] * wl[0] + I[5] * wl[1] + I[2] * wl[2]};
    double gy[3];
    cross3(wl, Iw, gy);
    // per side: f = m a(c), n = R (Ibar wdl + gy), wdl = R^T wd; side 2 has neither the centripetal nor the gyroscopic part
    double f[3][3], n[3][3];
#pragma unroll
    for (int s = 0; s < 3; s++) {
      cross3(wd[s], rc, t1);
      const double wdl[3] = {dot3(Fr.c0, wd[s]), dot3(Fr.c1, wd[s]), dot3(Fr.c2, wd[s])};
      double nl[3] = {I[0] * wdl[0] + I[3] * wdl[1] + I[4] * wdl[2], I[3] * wdl[0] + I[1] * wdl[1] + I[5] * wdl[2],
                      I[4] * wdl[0] + I[5] * wdl[1] + I[2] * wdl[2]};
#pragma unroll
      for (int i = 0; i < 3; i++) {
        if (s < 2) nl[i] += gy[i];
        f[s][i] = mass * (s < 2 ? ao[s][i] + t1[i] + t3[i] : ao[s][i] + t1[i]);
      }
#pragma unroll
      for (int i = 0; i < 3; i++) n[s][i] = Fr.c0[i] * nl[0] + Fr.c1[i] * nl[1] + Fr.c2[i] * nl[2];
    }
    const double fg[3] = {-(mass * lim.gravity[0]), -(mass * lim.gravity[1]), -(mass * lim.gravity[2])};
#pragma unroll 1
    for (int k = 0; k <= l; k++) {
      const double zk[3] = {S.ax[6 * k][lane], S.ax[6 * k + 1][lane], S.ax[6 * k + 2][lane]};
      const double rk[3] = {c[0] - S.ax[6 * k + 3][lane], c[1] - S.ax[6 * k + 4][lane], c[2] - S.ax[6 * k + 5][lane]};
#pragma unroll
      for (int s = 0; s < 3; s++) {
        cross3(rk, f[s], t1);
        S.tq[4 * k + s][lane] += zk[0] * (n[s][0] + t1[0]) + zk[1] * (n[s][1] + t1[1]) + zk[2] * (n[s][2] + t1[2]);
      }
      cross3(rk, fg, t2);
      S.tq[4 * k + 3][lane] += dot3(zk, t2);
    }
  }
  double* out = coef + ((size_t)b * Md + m) * 4 * D;
#pragma unroll
  for (int d = 0; d < D; d++) {
    out[d] = S.tq[4 * d + 2][lane];           // p
    out[D + d] = S.tq[4 * d + 1][lane];       // m_left
    out[2 * D + d] = S.tq[4 * d][lane];       // m_right
    out[3 * D + d] = S.tq[4 * d + 3][lane];   // tau_g
  }
}

namespace {

// the four coefficients of affine row r at checked state k of row b
struct AffineAt {
  double cxl, cxr, cu, off;
};
__device__ __forceinline__ AffineAt affine_at(const RetimeDynArgs& a, int b, int k, int r) {
  const size_t at = ((size_t)b * a.rt.Md + k) * a.stride + r;
  return AffineAt{a.cxl[at], a.cxr[at], a.cu[at], a.off[at]};
}

// row `lane` of stage k as k_retime_rows left it; lanes behind the stored rows hold a row that bounds nothing
__device__ __forceinline__ RetimeRow stored_row(const double* __restrict__ rows, int k, int nr, int lane) {
  if (lane >= nr) return RetimeRow{-HUGE_VAL, HUGE_VAL, 0.0, HUGE_VAL};
  const double* p = rows + ((size_t)k * nr + lane) * 4;
  return RetimeRow{p[0], p[1], p[2], p[3]};
}

}  // namespace

// rows [B][Md][2 D + 2 R][4]: the rows of stage k at state k's place (the last state's place stays unused)
template <bool TRAJ>
__global__ __launch_bounds__(256) void k_retime_rows(RetimeDynArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_acc[GPMP2MI_MAX_DOF], s_bound[RETIME_DYN_MAX_ROWS];
#pragma unroll
  for (int d = 0; d < GPMP2MI_MAX_DOF; d++)   // static indices into the kernel argument
    if (threadIdx.x == d) s_acc[d] = a.rt.acc[d];
#pragma unroll
  for (int r = 0; r < RETIME_DYN_MAX_ROWS; r++)
    if (threadIdx.x == 64 + r) s_bound[r] = a.bound[r];
  __syncthreads();
  const int D = a.rt.D, R = a.R, Md = a.rt.Md, nr = 2 * D + 2 * R;
  const int per = (Md - 1) * nr, nblk = (per + 255) / 256;   // both, and nblk B, < 2^31: launch_retime_dynamic
  const int b = blockIdx.x / nblk, e = (blockIdx.x % nblk) * 256 + threadIdx.x;
  if (e >= per) return;
  const int k = e / nr, i = e % nr;
  const double h2 = 2.0 * a.rt.h;
  RetimeRow row;
  double v, qL, qR;
  if (i < D) {
    retime_state<TRAJ>(a.rt, b, k, i, v, qL, qR);
    row = retime_row_start(qR, v, s_acc[i]);
  } else if (i < 2 * D) {
    retime_state<TRAJ>(a.rt, b, k + 1, i - D, v, qL, qR);
    row = retime_row_end(qL, v, s_acc[i - D], h2);
  } else if (i < 2 * D + R) {
    const AffineAt c = affine_at(a, b, k, i - 2 * D);
    row = retime_row_affine_start(c.cxr, c.cu, c.off, s_bound[i - 2 * D]);
  } else {
    const AffineAt c = affine_at(a, b, k + 1, i - 2 * D - R);
    row = retime_row_affine_end(c.cxl, c.cu, c.off, s_bound[i - 2 * D - R], h2);
  }
  double* o = a.rows + (((size_t)b * Md + k) * nr + i) * 4;
  o[0] = row.pl;
  o[1] = row.pu;
  o[2] = row.r;
  o[3] = row.xcap;
}

template <bool TRAJ>
__global__ __launch_bounds__(64) void k_retime_dynamic(RetimeDynArgs g) {
#pragma clang fp contract(off)   // what is written out here joins the rule: rounded once, as retime_affine_rule.h
  __shared__ double s_acc[GPMP2MI_MAX_DOF], s_vel[GPMP2MI_MAX_DOF], s_bound[RETIME_DYN_MAX_ROWS];
  __shared__ double s_pl[64], s_pu[64], s_r[64];
  const RetimeArgs& a = g.rt;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int D = a.D, R = g.R, Md = a.Md, nr = 2 * D + 2 * R, n = nr + 1;
  const double h2 = 2.0 * a.h;
#pragma unroll
  for (int d = 0; d < GPMP2MI_MAX_DOF; d++)   // static indices into the kernel argument
    if (lane == d) { s_acc[d] = a.acc[d]; s_vel[d] = a.vel[d]; }
#pragma unroll
  for (int r = 0; r < RETIME_DYN_MAX_ROWS; r++)
    if (lane == 32 + r) s_bound[r] = g.bound[r];
  __syncthreads();
  const RetimeMem w = retime_mem(a, b);
  const double* x = w.x;
  const double* u = w.u;
  const double* rows = g.rows + (size_t)b * Md * nr * 4;
  int status = RETIME_OK;
  double ach[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

  // caps, finiteness and what the offsets alone take, a lane per state
  {
    int stat = 0, inf = 0;
    const int bad = retime_caps_pass<TRAJ>(a, s_vel, w, b, lane, [&](int k) {
      int inv = 0;
      for (int r = 0; r < R; r++) {
        const AffineAt q = affine_at(g, b, k, r);
        const int what = retime_affine_check(k > 0, q.cxl, k < Md - 1, q.cxr, q.cu, q.off, s_bound[r]);
        inv |= what == 1;
        stat |= what == 2;
        inf |= retime_affine_check(k > 0, q.cxl, k < Md - 1, q.cxr, q.cu, q.off, 1.0) == 1;
        const double s = retime_static_ratio(q.off, s_bound[r]);
        if (s > ach[5]) ach[5] = s;
      }
      return inv;
    });
    if (__any(bad)) status = RETIME_INVALID;
    else if (__any(stat)) status = RETIME_STATIC;
    inf = __any(inf);
    if (g.nonfinite && lane == 0) g.nonfinite[b] = inf != 0;
  }
  __syncthreads();

  // backward: the controllable sets; forward: greedy.  Both read a stage's rows from the workspace while the next
  // stage's are in flight (`ahead`); lane nr forms the row of the next set.
  RetimeRow ahead;
  double lo, hi;
  if (status == RETIME_OK) ahead = stored_row(rows, Md - 2, nr, lane);
  retime_backward(a, w, s_pl, s_pu, s_r, n, lane, status, lo, hi, [&](int k, double klo, double khi) {
    RetimeRow row = ahead;
    if (k > 0) ahead = stored_row(rows, k - 1, nr, lane);   // in flight while this stage is eliminated
    if (lane == nr) row = retime_row_next(klo, khi, h2);
    return row;
  });
  __syncthreads();   // K is read below by every lane
  if (status == RETIME_OK) ahead = stored_row(rows, 0, nr, lane);
  retime_forward(a, w, lane, status, lo, hi, h2, [&](int k, double nlo, double nhi) {
    RetimeRow row = ahead;
    if (k < Md - 2) ahead = stored_row(rows, k + 1, nr, lane);
    if (lane == nr) row = retime_row_next(nlo, nhi, h2);
    return row;
  });
  __syncthreads();   // x and u are read below by every lane

  double duration = HUGE_VAL;
  if (status == RETIME_OK) {
    // achieved: the accelerations, a lane per (stage, joint), and the affine rows, a lane per (stage, row)
    retime_achieved_acc<TRAJ>(a, s_acc, w, b, lane, h2, ach);
    for (int e = lane; e < (Md - 1) * R; e += 64) {
      const int k = e / R, r = e % R;
      const AffineAt c0 = affine_at(g, b, k, r), c1 = affine_at(g, b, k + 1, r);
      const double xs = x[k], us = u[k], A = s_bound[r];
      const double t0 = retime_affine_ratio(c0.cxr, c0.cu, c0.off, xs, us, A);
      const double t1 = retime_affine_ratio(c1.cxl, retime_end_b(c1.cxl, c1.cu, h2), c1.off, xs, us, A);
      if (t0 > ach[4]) ach[4] = t0;
      if (t1 > ach[4]) ach[4] = t1;
    }
    if constexpr (TRAJ) {
      if (g.tau) {   // the torques of the re-timed row; the last state from the left with the last stage's u
        double* tau = g.tau + (size_t)b * Md * D;
        for (int e = lane; e < Md * D; e += 64) {
          const int k = e / D, d = e % D;
          const AffineAt c = affine_at(g, b, k, d);
          const bool last = k == Md - 1;
          tau[e] = retime_affine_value(last ? c.cxl : c.cxr, c.cu, c.off, x[k], u[last ? k - 1 : k]);
        }
      }
    }
    __syncthreads();   // x is read; the rates take its place
    retime_rates<TRAJ>(a, s_vel, w, b, lane, ach);
#pragma unroll
    for (int c = 0; c < 6; c++) ach[c] = wave_max(ach[c]);
    __syncthreads();   // the rates are read by the neighbouring lanes
    if (retime_stage_times(Md, w, lane, h2)) status = RETIME_EMPTY;
  }
  __syncthreads();
  if (status == RETIME_OK) {
    duration = retime_stamp_sum(Md, w.stamps, lane);
  } else {
    const double nn = nan("");
    for (int k = lane; k < Md; k += 64) w.x[k] = w.u[k] = w.stamps[k] = nn;
#pragma unroll
    for (int c = 0; c < 6; c++) ach[c] = nn;
    if constexpr (TRAJ) {
      if (g.tau)
        for (int e = lane; e < Md * D; e += 64) g.tau[(size_t)b * Md * D + e] = nn;
    }
  }
  if (lane == 0) {
    if (a.status) a.status[b] = status;
    if (a.duration) a.duration[b] = duration;
    if (a.achieved)
      for (int c = 0; c < 6; c++) a.achieved[6 * b + c] = ach[c];
  }
  retime_dense<TRAJ>(a, w.x, b, lane);
}

// The selection of gpmp2mi_plan_select_retimed_dynamic: one workgroup, rows by thread; the rule of k_retime_finish and
// no coefficient that is not finite.
__global__ __launch_bounds__(256) void k_retime_dynamic_finish(RetimeDynFinish g) {
  const RetimeFinish& a = g.rt;
  const ScoreFinish& f = a.sel;
  RowPick mine;
  for (int b = threadIdx.x; b < f.B; b += blockDim.x) {
    const double fe = f.ferr[b];
    if (retime_row_ok(a, f, b, fe) && g.nonfinite[b] == 0) mine.take(fe, b);
  }
  select_finish(f, mine);   // f.best is never null here (launch_retime_dynamic_finish)
  __syncthreads();   // best, and dense_best as interpolated
  const int best = *f.best;
  if (best < 0) return;
  retime_copy_best(a, f, best);
  if (g.tau_best)
    for (int e = threadIdx.x; e < f.Md * f.D; e += blockDim.x) g.tau_best[e] = g.tau[(size_t)best * f.Md * f.D + e];
}

int launch_retime_coef(const RobotDev& h, const RobotDev* R, const DynDev* dyn, const TorqueLimitsDev& lim, double dt,
                       int inter, int B, int N, const double* traj, double* coef, hipStream_t st) {
  int Md, nblk;
  if (const int rc = checked_grid(N, inter, SCORE_TILE, B, 4 * GPMP2MI_MAX_DOF, Md, nblk)) return rc;
  if (h.kind != GPMP2MI_ROBOT_ARM) {
    set_error("torque limits are built for fixed-base arms only");
    return GPMP2MI_ERR_UNSUPPORTED;
  }
  const dim3 grid((unsigned)(nblk * B)), block(64);
  G2_DISPATCH_ROBOT_ARM_ONLY(h.arm_dof,
                             (k_retime_coef<AD_><<<grid, block, 0, st>>>(R, dyn, lim, dt, inter, N, Md, nblk, traj, coef)));
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_retime_dynamic(const RetimeDynArgs& a, bool traj, hipStream_t st) {
  const RetimeArgs& r = a.rt;
  if (r.D < 1 || r.D > GPMP2MI_MAX_DOF || r.Md < 2 || a.R < 0 || a.R > RETIME_DYN_MAX_ROWS) {
    set_error("k_retime_dynamic: dof outside 1..GPMP2MI_MAX_DOF, fewer than two states or more than 8 affine rows");
    return GPMP2MI_ERR_INVALID;
  }
  const long long per = (long long)(r.Md - 1) * (2 * r.D + 2 * a.R);
  const long long nblk = (per + 255) / 256;
  if (per >= (1ll << 31) || nblk * r.B >= (1ll << 31)) {
    set_error("too many checked states or rows for one launch");
    return GPMP2MI_ERR_INVALID;
  }
  const dim3 grid((unsigned)(nblk * r.B));
  if (traj) {
    k_retime_rows<true><<<grid, dim3(256), 0, st>>>(a);
    k_retime_dynamic<true><<<dim3(r.B), dim3(64), 0, st>>>(a);
  } else {
    k_retime_rows<false><<<grid, dim3(256), 0, st>>>(a);
    k_retime_dynamic<false><<<dim3(r.B), dim3(64), 0, st>>>(a);
  }
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_retime_dynamic_finish(const RetimeDynFinish& a, hipStream_t st) {
  if (!a.rt.sel.select || !a.rt.sel.best) {
    set_error("k_retime_dynamic_finish: the selection needs a place for `best`");
    return GPMP2MI_ERR_INVALID;
  }
  return launch_finish(k_retime_dynamic_finish, a, 1, a.rt.sel.B, st);
}

}  // namespace g2
