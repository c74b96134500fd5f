// torque_kernels.hip -- the torque limits of the executed trajectory behind gpmp2mi_torque_score_traj /
// gpmp2mi_plan_torque_score / gpmp2mi_plan_select_dynamic (include/gpmp2mi.h "torque limits"): which joint torques does
// the trajectory ask of a fixed-base arm at every state that is executed, how much of each limit does gravity alone
// take, and by which factor must the duration be stretched for the drives to follow?
//
//   k_torque         tiled as k_motion is (checked_grid, score_select.h): a lane is a checked state, a workgroup covers
//                    SCORE_TILE consecutive states of one trajectory.  The recursion over the chain is serial in the
//                    links, so there is nothing wavefronts could share the way k_motion's share the spheres: the
//                    workgroup is ONE wavefront.  Every lane walks the chain outward once (the loop in k_torque): at
//                    joint j it up-samples both halves of its state for that joint (score_dense_coord), forms the
//                    acceleration of the interpolated mean there (retime_acc_ends / retime_acc_at; a support state
//                    between two intervals has a left and a right value, and both are carried), advances the frame and
//                    adds link j's force and moment to the torques of the joints below.  Three (value, state, joint)
//                    keys and the count of non-finite torques per lane -> keyed butterflies -> ONE record per workgroup.
//   k_torque_finish  reduces a row's records in index order and writes the outputs; when asked, applies the extended
//                    selection rule over the per-row scores the existing stages left and copies the chosen row
//                    (select_finish, score_select.h) with its torques.
//
// The walk itself and where its per-joint state lives (LDS columns DynLds, not registers) are described in dyn_walk.h,
// which holds what this walk and k_retime_coef's (retime_dynamic_kernels.hip) share; here NS = 2: per joint m of side 0,
// m of side 1 and tau_g.
//
// Determinism: every output is an extremum with an index key (key_less: exact ties go to the lowest indices), an integer
// count, or a per-state value; no sums of floating-point numbers across lanes, no atomics.  A row's results do not depend
// on the batch, its position in it or the entry point.  No address is computed from data.
#include <climits>

#include "device_math.h"
#include "dispatch.h"
#include "dyn_walk.h"

namespace g2 {

namespace {

__device__ __forceinline__ void torque_key(ScoreKey& best, double value, int i, int j) {
  const ScoreKey key{value, i, j};
  if (key_less(key, best)) best = key;
}

// What one evaluation (state m, one side) brings: tau = tau_g + m against the limits.  first: the side that also brings
// the static ratios of the state (tau_g does not depend on the side).
template <int AD>
__device__ __forceinline__ void torque_take(ScoreKey (&best)[3], int& invalid, const TorqueLimitsDev& lim, int m,
                                            const double (&mt)[AD], const double (&tg)[AD], bool first) {
#pragma unroll
  for (int d = 0; d < AD; d++) {
    const double L = lim.limit[d], g = tg[d], mm = mt[d], t = g + mm;
    const bool limited = L < HUGE_VAL;
    if (first && limited && isfinite(g)) torque_key(best[1], -(fabs(g) / L), m, d);
    if (!isfinite(t)) {
      invalid++;
      continue;
    }
    if (!limited) continue;
    torque_key(best[0], -(fabs(t) / L), m, d);
    const double den = mm > 0.0 ? L - g : L + g;   // what gravity leaves of the limit in the direction of m
    if (mm == 0.0) torque_key(best[2], -0.0, m, d);
    else if (den > 0.0) torque_key(best[2], -(fabs(mm) / den), m, d);   // den <= 0: static_ratio >= 1 says it
  }
}

__device__ __forceinline__ void torque_merge(ScoreKey& best, const ScoreKey& o) {
  if (key_less(o, best)) best = o;
}

}  // namespace

template <int AD>
__global__ __launch_bounds__(64) void k_torque(const RobotDev* __restrict__ Rg, const DynDev* __restrict__ Dg,
                                               TorqueLimitsDev lim, double dt, int inter, int N, int Md, int nblk,
                                               const double* __restrict__ traj, TorqueRec* __restrict__ recs,
                                               double* __restrict__ tau) {
  constexpr int D = AD;
  __shared__ RobotDev R;
  __shared__ DynDev Dn;
  __shared__ DynLds<AD, 2> S;
  stage_dyn(&Dn, Dg);
  stage_robot(&R, Rg);   // its barrier closes both copies
  const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int lane = threadIdx.x;
  const int m = blk * SCORE_TILE + lane;   // checked state of this lane
  // MINUS the torque ratio, the static ratio and r
  ScoreKey best[3];
#pragma unroll
  for (int c = 0; c < 3; c++) best[c] = ScoreKey{HUGE_VAL, INT_MAX, INT_MAX};
  int invalid = 0;
  if (m < Md) {
    const int seg = m / (inter + 1), j = m % (inter + 1);
    const double* s0 = traj + ((size_t)b * (N + 1) + seg) * 2 * D;
    // side 0: the acceleration in the interval the state opens or lies in (the last state: the one it closes); a
    // support state between two intervals has a side 1, the end of the interval before it (elsewhere side 1 repeats
    // the end of side 0's interval and is not looked at)
    const bool two = j == 0 && seg > 0 && seg < N;
    const double* i0 = seg < N ? s0 : s0 - 2 * D;
    const double* i1 = two ? s0 - 2 * D : i0;
    Frame Fr;
    frame_from_3x4(R.base, Fr);
    double w[3] = {0.0, 0.0, 0.0}, wd[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    double ao[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    double op[3] = {Fr.t[0], Fr.t[1], Fr.t[2]};   // the origin of the joint before (joint 0: its own, r = 0)
#pragma unroll 1
    for (int l = 0; l < AD; l++) {   // link l hangs from joint l: axis z through o, the frame in front of it
      double x[D + 1], a0, a1, t1[3], t2[3], t3[3];
      score_dense_coord(false, dt, inter, D, j, 0, s0 + l, x);   // coordinate l: x[0] = q, x[D] = v
      const double ql = x[0], vl = x[D];
      retime_acc_ends(dt, i0[2 * D + l] - i0[l], i0[D + l], i0[3 * D + l], a0, a1);
      const double al0 = seg < N ? retime_acc_at(a0, a1, j, inter + 1) : a1;
      retime_acc_ends(dt, i1[2 * D + l] - i1[l], i1[D + l], i1[3 * D + l], a0, a1);
      const double al1 = a1;
      const double z[3] = {Fr.c2[0], Fr.c2[1], Fr.c2[2]}, o[3] = {Fr.t[0], Fr.t[1], Fr.t[2]};
#pragma unroll
      for (int i = 0; i < 3; i++) {
        S.ax[6 * l + i][lane] = z[i];
        S.ax[6 * l + 3 + i][lane] = o[i];
        S.tq[3 * l + i][lane] = 0.0;
      }
      // o and the origin before it both ride on link l-1
      const double r[3] = {o[0] - op[0], o[1] - op[1], o[2] - op[2]};
      cross3(w, r, t2);
      cross3(w, t2, t3);
#pragma unroll
      for (int s = 0; s < 2; s++) {
        cross3(wd[s], r, t1);
#pragma unroll
        for (int i = 0; i < 3; i++) ao[s][i] += t1[i] + t3[i];
      }
      cross3(w, z, t1);   // the velocity product of wd, with w of the link before
#pragma unroll
      for (int i = 0; i < 3; i++) {
        wd[0][i] += z[i] * al0 + t1[i] * vl;
        wd[1][i] += z[i] * al1 + t1[i] * vl;
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
      // per side: f = m a(c), n = R (Ibar wdl + gy), wdl = R^T wd
      double f[2][3], n[2][3];
#pragma unroll
      for (int s = 0; s < 2; s++) {
        cross3(wd[s], rc, t1);
        const double wdl[3] = {dot3(Fr.c0, wd[s]), dot3(Fr.c1, wd[s]), dot3(Fr.c2, wd[s])};
        const double nl[3] = {I[0] * wdl[0] + I[3] * wdl[1] + I[4] * wdl[2] + gy[0],
                              I[3] * wdl[0] + I[1] * wdl[1] + I[5] * wdl[2] + gy[1],
                              I[4] * wdl[0] + I[5] * wdl[1] + I[2] * wdl[2] + gy[2]};
#pragma unroll
        for (int i = 0; i < 3; i++) {
          f[s][i] = mass * (ao[s][i] + t1[i] + t3[i]);
          n[s][i] = Fr.c0[i] * nl[0] + Fr.c1[i] * nl[1] + Fr.c2[i] * nl[2];
        }
      }
      const double fg[3] = {-(mass * lim.gravity[0]), -(mass * lim.gravity[1]), -(mass * lim.gravity[2])};
#pragma unroll 1
      for (int k = 0; k <= l; k++) {
        const double zk[3] = {S.ax[6 * k][lane], S.ax[6 * k + 1][lane], S.ax[6 * k + 2][lane]};
        const double rk[3] = {c[0] - S.ax[6 * k + 3][lane], c[1] - S.ax[6 * k + 4][lane], c[2] - S.ax[6 * k + 5][lane]};
#pragma unroll
        for (int s = 0; s < 2; s++) {
          cross3(rk, f[s], t1);
          S.tq[3 * k + s][lane] += zk[0] * (n[s][0] + t1[0]) + zk[1] * (n[s][1] + t1[1]) + zk[2] * (n[s][2] + t1[2]);
        }
        cross3(rk, fg, t2);
        S.tq[3 * k + 2][lane] += dot3(zk, t2);
      }
    }
    double mt[2][D], tg[D];
#pragma unroll
    for (int d = 0; d < D; d++) {
      mt[0][d] = S.tq[3 * d][lane];
      mt[1][d] = S.tq[3 * d + 1][lane];
      tg[d] = S.tq[3 * d + 2][lane];
    }
    torque_take<AD>(best, invalid, lim, m, mt[0], tg, true);
    if (two) torque_take<AD>(best, invalid, lim, m, mt[1], tg, false);
    if (tau) {
#pragma unroll
      for (int d = 0; d < D; d++) tau[((size_t)b * Md + m) * D + d] = tg[d] + mt[0][d];
    }
  }
  // keyed butterflies (both partners keep the same key, so all 64 lanes end with the same bits)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    invalid += __shfl_xor(invalid, off);
#pragma unroll
    for (int c = 0; c < 3; c++)
      torque_merge(best[c], ScoreKey{__shfl_xor(best[c].c, off), __shfl_xor(best[c].k, off), __shfl_xor(best[c].s, off)});
  }
  if (lane == 0) {   // one wavefront: nothing to merge through LDS
    TorqueRec r;
    r.invalid = invalid;
    r.pad = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) { r.v[c] = best[c].c; r.ij[c][0] = best[c].k; r.ij[c][1] = best[c].s; }
    recs[blockIdx.x] = r;
  }
}

namespace {

// the outputs of one row: its records in index order
struct TorqueRow {
  double torque_ratio, static_ratio, time_scale;
  int worst[3][2], invalid;
};
__device__ __forceinline__ TorqueRow torque_row(const TorqueFinish& a, int b) {
  const TorqueRec* r = a.recs + (size_t)b * a.nblk;
  TorqueRec t = r[0];
  for (int i = 1; i < a.nblk; i++) {   // records in index order
    t.invalid += r[i].invalid;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const ScoreKey x{r[i].v[c], r[i].ij[c][0], r[i].ij[c][1]}, cur{t.v[c], t.ij[c][0], t.ij[c][1]};
      if (key_less(x, cur)) { t.v[c] = x.c; t.ij[c][0] = x.k; t.ij[c][1] = x.s; }
    }
  }
  TorqueRow o;
  double val[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const bool none = t.ij[c][0] == INT_MAX;
    o.worst[c][0] = none ? -1 : t.ij[c][0];
    o.worst[c][1] = none ? -1 : t.ij[c][1];
    val[c] = none ? 0.0 : -t.v[c];
  }
  o.torque_ratio = val[0];
  o.static_ratio = val[1];
  o.time_scale = o.static_ratio >= 1.0 ? HUGE_VAL : sqrt(val[2]);
  o.invalid = t.invalid;
  return o;
}
// the larger of the two stretches a row needs: the motion stage's and this one's
__device__ __forceinline__ double both_scales(double motion, double torque) { return torque > motion ? torque : motion; }

}  // namespace

// Second stage: rows are taken by thread (RowPick, score_select.h).  With a.sel.select the grid is one workgroup and the
// rule reads, besides this stage's own results, the per-row scores the earlier stages left.
__global__ __launch_bounds__(256) void k_torque_finish(TorqueFinish a) {
  const ScoreFinish& f = a.sel;
  RowPick mine;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < f.B; b += gridDim.x * blockDim.x) {
    const TorqueRow o = torque_row(a, b);
    if (a.torque_ratio) a.torque_ratio[b] = o.torque_ratio;
    if (a.static_ratio) a.static_ratio[b] = o.static_ratio;
    if (a.time_scale) a.time_scale[b] = o.time_scale;
    if (a.worst) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        a.worst[6 * b + 2 * c] = o.worst[c][0];
        a.worst[6 * b + 2 * c + 1] = o.worst[c][1];
      }
    }
    if (a.invalid) a.invalid[b] = o.invalid;
    if (!f.select) continue;
    const double fe = f.ferr[b];
    bool ok = row_eligible(f, b, fe, a.clearance[b], a.oor[b]);
    if (a.self_clearance) ok = ok && a.self_invalid[b] == 0 && a.self_clearance[b] >= a.required_self_clearance;
    ok = ok && a.motion_invalid[b] == 0 && a.pos_margin[b] >= a.required_pos_margin && o.invalid == 0;
    ok = ok && both_scales(a.motion_time_scale[b], o.time_scale) <= a.max_time_scale;
    if (ok) mine.take(fe, b);
  }
  if (!f.select) return;
  select_finish(f, mine);   // f.best is never null here (launch_torque_finish)
  __syncthreads();
  const int best = *f.best;
  if (best < 0) return;
  if (threadIdx.x == 0 && a.time_scale_best)
    *a.time_scale_best = both_scales(a.motion_time_scale[best], torque_row(a, best).time_scale);
  if (a.tau_best)
    for (int e = threadIdx.x; e < f.Md * f.D; e += blockDim.x) a.tau_best[e] = a.tau[(size_t)best * f.Md * f.D + e];
}

int launch_torque(const RobotDev& h, const RobotDev* R, const DynDev* dyn, const TorqueLimitsDev& lim, double dt, int inter,
                  int B, int N, const double* traj, TorqueRec* recs, double* tau, hipStream_t st) {
  int Md, nblk;
  if (const int rc = checked_grid(N, inter, SCORE_TILE, B, 1, Md, nblk)) return rc;
  if (h.kind != GPMP2MI_ROBOT_ARM) {
    set_error("torque limits are built for fixed-base arms only");
    return GPMP2MI_ERR_UNSUPPORTED;
  }
  const dim3 grid((unsigned)(nblk * B)), block(64);
  G2_DISPATCH_ROBOT_ARM_ONLY(h.arm_dof,
                             (k_torque<AD_><<<grid, block, 0, st>>>(R, dyn, lim, dt, inter, N, Md, nblk, traj, recs, tau)));
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_torque_finish(const TorqueFinish& a, hipStream_t st) {
  if (a.sel.select && !a.sel.best) {
    set_error("k_torque_finish: the selection needs a place for `best`");
    return GPMP2MI_ERR_INVALID;
  }
  return launch_finish(k_torque_finish, a, a.sel.select, a.sel.B, st);
}

}  // namespace g2
