// retime_dynamic_kernels.hip -- the speed profile of the executed trajectory under joint torque limits, behind
// gpmp2mi_retime_path_affine / gpmp2mi_retime_dynamic_traj (include/gpmp2mi.h "re-timing under torque limits"): the rule
// of retime_kernels.hip with rows that carry an offset, |cx x + cu u + off| <= A.  Along the fixed path the torque of
// joint d is such a row, tau = p u + m x + tau_g with x = sdot^2 and u = sddot.  The rule is retime_affine_rule.h; these
// kernels spread it.  ps comes from k_retime_caps (retime_kernels.hip), unchanged.
//
//   k_retime_coef     tiled as k_torque is: one wavefront, a lane per checked state, SCORE_TILE states per workgroup.
//                     One outward walk in the world frame (the walk of k_torque, torque_kernels.hip, a second copy of
//                     it) with three accelerations per lane: (q', q''_right), (q', q''_left) and (0, q').  The third has
//                     no velocity terms and gives p = M(q) q'.  Writes coef [B][Md][4][D] = p, m_left, m_right, tau_g; a
//                     state with one side carries that side twice.  Where q' == 0 exactly p == 0 exactly (every term of
//                     the third walk is a product with a q'), and where q'' == 0 as well m == 0: the rule branches on
//                     cu == 0, so a rounding-level p at a rest state would be another row.
//   k_retime_rows     a lane per (stage, row): (pl, pu, r, xcap) of the 2 D + 2 R rows of every stage that do not
//                     depend on the chain, into the workspace.  Forming rows inside the chain is what k_retime pays per
//                     dependent stage.
//   k_retime_dynamic  one wavefront per row, the structure of k_retime: caps, finiteness and the static test, a lane per
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
#include "launch.h"
#include "retime_affine_rule.h"
#include "score_select.h"

namespace g2 {

static_assert(2 * GPMP2MI_MAX_DOF + 2 * 8 + 1 <= 64, "the rows of a stage are one per lane");
static_assert(RETIME_DYN_MAX_ROWS == RETIME_MAX_EXTRA && TORQUE_MAX_AD <= RETIME_MAX_EXTRA, "one affine row per joint");

namespace {

__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// per lane (column): the axis and the origin of every joint reached so far, and per joint m of the right side, m of the
// left side, p and tau_g (TorqueLds of torque_kernels.hip with a fourth slot; profiles/torque_resources.txt says why
// not registers)
template <int AD>
struct CoefLds {
  double ax[6 * AD][SCORE_TILE], tq[4 * AD][SCORE_TILE];
};

}  // namespace

template <int AD>
__global__ __launch_bounds__(64) void k_retime_coef(const RobotDev* __restrict__ Rg, const DynDev* __restrict__ Dg,
                                                    TorqueLimitsDev lim, double dt, int inter, int N, int Md, int nblk,
                                                    const double* __restrict__ traj, double* __restrict__ coef) {
  constexpr int D = AD;
  __shared__ RobotDev R;
  __shared__ DynDev Dn;
  __shared__ CoefLds<AD> S;
  {
    const int* s = reinterpret_cast<const int*>(Dg);
    int* d = reinterpret_cast<int*>(&Dn);
    for (int i = threadIdx.x; i < (int)(sizeof(DynDev) / 4); i += blockDim.x) d[i] = s[i];
  }
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

// q'_k, q''_{k-} and q''_{k+} of coordinate d at checked state k of row b (qL: k > 0, qR: k < Md - 1; else 0): the
// expressions of retime_state in retime_kernels.hip, which that unit keeps to itself
template <bool TRAJ>
__device__ __forceinline__ void dyn_state(const RetimeArgs& a, int b, int k, int d, double& v, double& qL, double& qR) {
  const int D = a.D;
  if constexpr (!TRAJ) {
    const size_t at = ((size_t)b * a.Md + k) * D + d;
    v = a.qd[at];
    qL = k > 0 ? a.ql[at] : 0.0;
    qR = k < a.Md - 1 ? a.qr[at] : 0.0;
  } else {
    const int J1 = a.inter + 1, seg = k / J1, j = k % J1;
    const double* s0 = a.traj + ((size_t)b * (a.N + 1) + seg) * 2 * D;
    qL = qR = 0.0;
    if (j == 0) {
      v = s0[D + d];
    } else {   // the velocity half of score_dense_coord (score_select.h), vector coordinates
      const double* s1 = s0 + 2 * D;
      const GpCoef gc = gp_coef_dev(a.dt, (double)j * (a.dt / (double)J1));
      v = gc.l21 * s0[d] + gc.l22 * s0[D + d] + gc.p21 * s1[d] + gc.p22 * s1[D + d];
    }
    if (seg < a.N) {
      const double* s1 = s0 + 2 * D;
      double a0, a1;
      retime_acc_ends(a.dt, s1[d] - s0[d], s0[D + d], s1[D + d], a0, a1);
      qR = retime_acc_at(a0, a1, j, J1);
      if (j > 0) qL = qR;
    }
    if (j == 0 && seg > 0) {
      const double* sp = s0 - 2 * D;
      double a0, a1;
      retime_acc_ends(a.dt, s0[d] - sp[d], sp[D + d], s0[D + d], a0, a1);
      qL = a1;
    }
  }
}

// the four coefficients of affine row r at checked state k of row b
struct AffineAt {
  double cxl, cxr, cu, off;
};
__device__ __forceinline__ AffineAt affine_at(const RetimeDynArgs& a, int b, int k, int r) {
  const size_t at = ((size_t)b * a.rt.Md + k) * a.stride + r;
  return AffineAt{a.cxl[at], a.cxr[at], a.cu[at], a.off[at]};
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_xor(v, off);
    if (o < v) v = o;
  }
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_xor(v, off);
    if (o > v) v = o;
  }
  return v;
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
    dyn_state<TRAJ>(a.rt, b, k, i, v, qL, qR);
    row = retime_row_start(qR, v, s_acc[i]);
  } else if (i < 2 * D) {
    dyn_state<TRAJ>(a.rt, b, k + 1, i - D, v, qL, qR);
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
  double* X = a.X + (size_t)b * Md;
  double* Kw = a.K + (size_t)b * Md * 2;
  double* x = a.sdot + (size_t)b * Md;   // x_k until the rates replace it
  double* u = a.u + (size_t)b * Md;
  double* stamps = a.stamps + (size_t)b * Md;
  const double* rows = g.rows + (size_t)b * Md * nr * 4;
  int status = RETIME_OK;
  double ach[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

  // caps, finiteness and what the offsets alone take, a lane per state
  {
    const double X0 = a.max_rate * a.max_rate;
    int bad = 0, stat = 0, inf = 0;
    for (int k = lane; k < Md; k += 64) {
      double c = X0;
      for (int d = 0; d < D; d++) {
        double v, qL, qR;
        dyn_state<TRAJ>(a, b, k, d, v, qL, qR);
        bad |= !isfinite(v) || !isfinite(qL) || !isfinite(qR);
        if constexpr (TRAJ) {
          const double cv = retime_cap(s_vel[d], v);
          if (cv < c) c = cv;
        }
      }
      if constexpr (TRAJ) {
        const double p = a.ps[(size_t)b * Md + k];
        bad |= !isfinite(p);
        const double cp = retime_cap(a.point_speed, p);
        if (cp < c) c = cp;
      } else {
        const double cc = a.cap[(size_t)b * Md + k];
        bad |= !(cc >= 0.0);
        if (cc < c) c = cc;
      }
      for (int r = 0; r < R; r++) {
        const AffineAt q = affine_at(g, b, k, r);
        const int what = retime_affine_check(k > 0, q.cxl, k < Md - 1, q.cxr, q.cu, q.off, s_bound[r]);
        bad |= what == 1;
        stat |= what == 2;
        inf |= retime_affine_check(k > 0, q.cxl, k < Md - 1, q.cxr, q.cu, q.off, 1.0) == 1;
        const double s = retime_static_ratio(q.off, s_bound[r]);
        if (s > ach[5]) ach[5] = s;
      }
      X[k] = c;
    }
    if (__any(bad)) status = RETIME_INVALID;
    else if (__any(stat)) status = RETIME_STATIC;
    inf = __any(inf);
    if (g.nonfinite && lane == 0) g.nonfinite[b] = inf != 0;
  }
  __syncthreads();

  // backward: the controllable sets
  double lo = 0.0, hi = 0.0;
  if (status == RETIME_OK) {
    hi = X[Md - 1];
    if (a.rate_end >= 0.0) {
      lo = a.rate_end * a.rate_end;
      if (lo > hi) status = RETIME_BOUNDARY;
      hi = lo;
    }
  }
  if (status == RETIME_OK) {
    if (lane == 0) { Kw[2 * (Md - 1)] = lo; Kw[2 * (Md - 1) + 1] = hi; }
    const int q64 = 64 / n, r64 = 64 % n;
    RetimeRow ahead = stored_row(rows, Md - 2, nr, lane);
    for (int k = Md - 2; k >= 0; k--) {
      RetimeRow row = ahead;
      if (k > 0) ahead = stored_row(rows, k - 1, nr, lane);   // in flight while this stage is eliminated
      if (lane == nr) row = retime_row_next(lo, hi, h2);
      s_pl[lane] = row.pl;
      s_pu[lane] = row.pu;
      s_r[lane] = row.r;
      __syncthreads();
      double l = 0.0, t = X[k];
      if (row.xcap < t) t = row.xcap;
      int empty = 0;
      int i = lane / n, j = lane % n;
      for (int p = lane; p < n * n; p += 64) {
        retime_pair(RetimeRow{s_pl[i], 0.0, s_r[i], 0.0}, RetimeRow{0.0, s_pu[j], s_r[j], 0.0}, l, t, empty);
        i += q64;
        j += r64;
        if (j >= n) { j -= n; i++; }
      }
      __syncthreads();   // the rows of this stage are read
      l = wave_max(l);
      t = wave_min(t);
      if (__any(empty) || l > t) {
        status = RETIME_EMPTY;
        break;
      }
      lo = l;
      hi = t;
      if (lane == 0) { Kw[2 * k] = lo; Kw[2 * k + 1] = hi; }
    }
  }
  __syncthreads();   // K is read below by every lane

  // forward: greedy
  double xk = hi;
  if (status == RETIME_OK && a.rate_start >= 0.0) {
    xk = a.rate_start * a.rate_start;
    if (xk < lo || xk > hi) status = RETIME_BOUNDARY;
  }
  if (status == RETIME_OK) {
    if (lane == 0) x[0] = xk;
    RetimeRow ahead = stored_row(rows, 0, nr, lane);
    for (int k = 0; k < Md - 1; k++) {
      const double nlo = Kw[2 * k + 2], nhi = Kw[2 * k + 3];
      RetimeRow row = ahead;
      if (k < Md - 2) ahead = stored_row(rows, k + 1, nr, lane);
      if (lane == nr) row = retime_row_next(nlo, nhi, h2);
      const double uh = wave_min(retime_upper_at(row, xk));
      double x1, uk;
      retime_step(xk, uh, nlo, nhi, h2, x1, uk);
      if (lane == 0) { x[k + 1] = x1; u[k] = uk; }
      xk = x1;
    }
    if (lane == 0) u[Md - 1] = 0.0;
  }
  __syncthreads();   // x and u are read below by every lane

  double duration = HUGE_VAL;
  if (status == RETIME_OK) {
    // achieved: the accelerations, a lane per (stage, joint), and the affine rows, a lane per (stage, row)
    for (int e = lane; e < (Md - 1) * D; e += 64) {
      const int k = e / D, d = e % D;
      double v0, v1, l0, r0, l1, r1;
      dyn_state<TRAJ>(a, b, k, d, v0, l0, r0);
      dyn_state<TRAJ>(a, b, k + 1, d, v1, l1, r1);
      const double xs = x[k], us = u[k], A = s_acc[d];
      const double e0 = retime_acc_ratio(r0, v0, xs, us, A);
      const double e1 = retime_acc_ratio(l1, retime_end_b(l1, v1, h2), xs, us, A);
      const double m = retime_mid_ratio(v0, r0, l1, xs, us, a.h, A);
      if (e0 > ach[1]) ach[1] = e0;
      if (e1 > ach[1]) ach[1] = e1;
      if (m > ach[2]) ach[2] = m;
    }
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
    for (int k = lane; k < Md; k += 64) {
      const double s = sqrt(x[k]);
      x[k] = s;
      if constexpr (TRAJ) {
        for (int d = 0; d < D; d++) {
          if (!(s_vel[d] < HUGE_VAL)) continue;
          double v, qL, qR;
          dyn_state<TRAJ>(a, b, k, d, v, qL, qR);
          const double r = fabs(v) * s / s_vel[d];
          if (r > ach[0]) ach[0] = r;
        }
        if (a.point_speed < HUGE_VAL) {
          const double r = a.ps[(size_t)b * Md + k] * s / a.point_speed;
          if (r > ach[3]) ach[3] = r;
        }
      } else {
        const double c = a.cap[(size_t)b * Md + k];
        if (c < HUGE_VAL && c > 0.0) {
          const double r = s / sqrt(c);
          if (r > ach[0]) ach[0] = r;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 6; c++) ach[c] = wave_max(ach[c]);
    __syncthreads();   // the rates are read by the neighbouring lanes
    // the stage times, a lane per stage; then one sum in index order, the same in every lane
    int zero = 0;
    for (int k = lane; k < Md - 1; k += 64) {
      const double s0 = x[k], s1 = x[k + 1];
      zero |= s0 + s1 == 0.0;
      stamps[k + 1] = retime_stage_time(s0, s1, h2);
    }
    if (__any(zero)) status = RETIME_EMPTY;
  }
  __syncthreads();
  if (status == RETIME_OK) {
    double t = 0.0;
    if (lane == 0) stamps[0] = 0.0;
    for (int base = 0; base < Md - 1; base += 64) {
      const int k = base + lane;
      const double v = k < Md - 1 ? stamps[k + 1] : 0.0;
      double mine = 0.0;
#pragma unroll
      for (int i = 0; i < 64; i++) {
        t = t + __shfl(v, i);   // t + 0 behind the last stage leaves t as it is
        if (lane == i) mine = t;
      }
      if (k < Md - 1) stamps[k + 1] = mine;
    }
    duration = t;
  } else {
    const double nn = nan("");
    for (int k = lane; k < Md; k += 64) x[k] = u[k] = stamps[k] = nn;
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
  if constexpr (TRAJ) {
    if (a.dense) {
      __syncthreads();   // the rates (or the NaNs) of every state
      double* out = a.dense + (size_t)b * Md * 2 * D;
      const double* row = a.traj + (size_t)b * (a.N + 1) * 2 * D;
      for (int e = lane; e < Md * D; e += 64) {
        const int m = e / D, k = e % D;
        double* o = out + (size_t)m * 2 * D;
        score_dense_coord(false, a.dt, a.inter, D, m % (a.inter + 1), k, row + (size_t)(m / (a.inter + 1)) * 2 * D, o);
        o[D + k] = o[D + k] * x[m];
      }
    }
  }
}

// The selection of gpmp2mi_plan_select_retimed_dynamic: one workgroup, rows by thread; the rule of k_retime_finish and
// no coefficient that is not finite.
__global__ __launch_bounds__(256) void k_retime_dynamic_finish(RetimeDynFinish g) {
  const RetimeFinish& a = g.rt;
  const ScoreFinish& f = a.sel;
  RowPick mine;
  for (int b = threadIdx.x; b < f.B; b += blockDim.x) {
    const double fe = f.ferr[b];
    bool ok = row_eligible(f, b, fe, a.clearance[b], a.oor[b]);
    if (a.self_clearance) ok = ok && a.self_invalid[b] == 0 && a.self_clearance[b] >= a.required_self_clearance;
    ok = ok && a.motion_invalid[b] == 0 && a.pos_margin[b] >= a.required_pos_margin;
    ok = ok && a.rstatus[b] == RETIME_OK && g.nonfinite[b] == 0 && a.duration[b] <= a.max_duration;
    if (ok) mine.take(fe, b);
  }
  select_finish(f, mine);   // f.best is never null here (launch_retime_dynamic_finish)
  __syncthreads();   // best, and dense_best as interpolated
  const int best = *f.best;
  if (best < 0) return;
  const double* sd = a.sdot + (size_t)best * f.Md;
  if (threadIdx.x == 0 && a.duration_best) *a.duration_best = a.duration[best];
  if (a.stamps_best)
    for (int m = threadIdx.x; m < f.Md; m += blockDim.x) a.stamps_best[m] = a.stamps[(size_t)best * f.Md + m];
  if (g.tau_best)
    for (int e = threadIdx.x; e < f.Md * f.D; e += blockDim.x) g.tau_best[e] = g.tau[(size_t)best * f.Md * f.D + e];
  if (f.dense_best)
    for (int e = threadIdx.x; e < f.Md * f.D; e += blockDim.x) {   // the elements this thread wrote in select_finish
      const int m = e / f.D, k = e % f.D;
      double* o = f.dense_best + (size_t)m * 2 * f.D + f.D + k;
      *o = *o * sd[m];
    }
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
