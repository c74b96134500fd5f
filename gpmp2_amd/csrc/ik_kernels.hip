// ik_kernels.hip -- "goal configurations" (include/gpmp2mi.h): batched inverse kinematics from a workspace pose.
//
//   k_ik            one lane per problem (pose g, seed row m), 64 lanes per workgroup, the robot staged in LDS.  The rule
//                   of the header, literally: damped least squares in the dual form, so the system is ROWS x ROWS (3 or
//                   6) whatever the dof.  q, e, H (ROWS x D, omega rows already scaled) and the packed system stay in
//                   registers; the chain is walked once per pass and the Jacobian is formed only for a step that was
//                   accepted (the test needs e' alone).  In the POSE form its columns wait in LDS while the log-map
//                   derivative has the registers (profiles/ik_resources.txt).  A lane leaves the loop at its own
//                   count; the loop is bounded by max_iter + 1 passes.
//   k_ik_rows       one lane per answer: clearance of the single configuration (the value-only walk and the range-tested
//                   lookups of k_score), eligibility, score, and the row staged as a one-state trajectory for
//                   k_traj_pairs (group_kernels.hip), whose distances and whose rule kernel the goal stage reuses.
//   k_ik_goal_copy  one workgroup per pose: the counts and the leaders' rows.
//
// Determinism: no lane reads another lane's numbers and nothing is accumulated across lanes, so a row's outputs do not
// depend on G, M or its place among them.
#include <climits>

#include "device_math.h"
#include "launch.h"
#include "lie_log.h"
#include "rng.h"

namespace g2 {

namespace {
__device__ __forceinline__ double ik_clamp(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }
__device__ __forceinline__ double ik_norm3(const double* v) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
// lo + u * (hi - lo) with the difference, the product and the sum each rounded once: the compiler must not fuse the
// product into the sum (__dmul_rn / __dadd_rn are plain operators to it and do not prevent that)
__device__ __forceinline__ double ik_draw(double u, double lo, double hi) {
#pragma clang fp contract(off)
  const double span = hi - lo;
  const double prod = u * span;
  return lo + prod;
}
constexpr int ik_tri(int i, int j) { return i * (i + 1) / 2 + j; }   // packed lower triangle, j <= i
}  // namespace

template <int AD, int ROWS>
__global__ __launch_bounds__(64) void k_ik(const RobotDev* __restrict__ Rg, IkArgs a) {
  using K = Kin<GPMP2MI_ROBOT_ARM, AD, 0>;
  constexpr int D = AD, NC = ROWS == 6 ? 6 : 3;
  __shared__ RobotDev R;
  __shared__ double s_J[ROWS == 6 ? 6 * D : 1][64];   // a lane's Jacobian columns, parked (POSE only)
  stage_robot(&R, Rg);
  const long long p = blockIdx.x * 64ll + threadIdx.x;
  if (p >= (long long)a.G * a.M) return;
  const int g = (int)(p / a.M), m = (int)(p % a.M);
  double Rd[9], td[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) Rd[i * 3 + j] = a.des[(size_t)g * 16 + i * 4 + j];
    td[i] = a.des[(size_t)g * 16 + i * 4 + 3];
  }
  const bool orient = ROWS == 3 && a.mode == GPMP2MI_WORKSPACE_ORIENTATION;
  const double sw = a.rot_weight;
  // scale of row r: rot_weight on the omega rows
  auto scale = [&](int r) { return (ROWS == 6 ? r < 3 : orient) ? sw : 1.0; };

  double q[D], qt[D];
  bool fin = true;
#pragma unroll
  for (int k = 0; k < D; k++) {
    double s;
    if (a.seeds) {
      s = a.seeds[(size_t)p * D + k];
    } else {
      const double u = uniform(a.seed, GPMP2MI_RNG_IK, (uint32_t)g, (uint32_t)(a.first + m), 0u, k);
      s = ik_draw(u, a.down[k], a.up[k]);
    }
    fin = fin && isfinite(s);
    qt[k] = ik_clamp(s, a.down[k], a.up[k]);
    if (s != s) qt[k] = s;   // fmin / fmax drop a NaN: the clamped seed of a NaN is a NaN
    q[k] = qt[k];
  }

  double e[ROWS], H[ROWS][D];
#pragma unroll
  for (int r = 0; r < ROWS; r++) {
    e[r] = 0.0;
#pragma unroll
    for (int k = 0; k < D; k++) H[r][k] = 0.0;
  }
  double c = 0.0, lam = a.lam0;
  int it = 0, status = GPMP2MI_IK_MAX_ITER_REACHED;
  bool first = true, bad = false;

  for (int pass = 0; pass <= a.max_iter; pass++) {   // pass 0 evaluates the seed; pass n > 0 the n-th trial point
    typename K::Axes A;
    Frame F;
    K::walk_links(R, qt, A, [&](int l, const Frame& Fr, auto) {
      if (l == a.link) F = Fr;
    });
    // the rows of k_workspace_prior (factor_kernels.hip) at the link's frame
    double Rm[9], Rrel[9], trel[3], et[ROWS];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      Rm[i * 3 + 0] = F.c0[i];
      Rm[i * 3 + 1] = F.c1[i];
      Rm[i * 3 + 2] = F.c2[i];
    }
    const double* t = F.t;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double s = 0;
#pragma unroll
        for (int cc = 0; cc < 3; cc++) s += Rd[cc * 3 + i] * Rm[cc * 3 + j];
        Rrel[i * 3 + j] = s;
      }
      trel[i] = Rd[i] * (t[0] - td[0]) + Rd[3 + i] * (t[1] - td[1]) + Rd[6 + i] * (t[2] - td[2]);
    }
    if constexpr (ROWS == 6) {
      pose3_logmap(Rrel, trel, et);
    } else {
      if (orient) {
        rot3_logmap(Rrel, et);
      } else {
#pragma unroll
        for (int i = 0; i < 3; i++) et[i] = t[i] - td[i];
      }
    }
    double ct = 0.0;
    bool efin = true;
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
      const double x = scale(r) * et[r];
      ct += x * x;
      efin = efin && isfinite(et[r]);
    }
    bool conv;
    if constexpr (ROWS == 6) conv = ik_norm3(et) <= a.rot_tol && ik_norm3(et + 3) <= a.pos_tol;
    else conv = ik_norm3(et) <= (orient ? a.rot_tol : a.pos_tol);

    bool accept = true;
    if (!first) {
      it++;
      accept = !bad && ct < c;   // a NaN or infinite c' fails the comparison
    }
    if (accept) {
#pragma unroll
      for (int k = 0; k < D; k++) q[k] = qt[k];
#pragma unroll
      for (int r = 0; r < ROWS; r++) e[r] = et[r];
      c = ct;
      if (first && !(fin && efin)) {
        status = GPMP2MI_IK_INVALID;
        break;
      }
      if (conv) {
        status = GPMP2MI_IK_CONVERGED;
        break;
      }
      if (!first) lam = fmax(lam / a.lam_factor, a.lam_lo);
      // H^ = scale * (d e / d pose) * J6, J6 the body Jacobian of the link as k_fk forms it: column k from the axis
      // and origin of joint k, zero for the joints beyond the link
      // The columns first, and out to LDS (lane-major: conflict-free 8-byte accesses) while the log-map derivative has
      // the registers: with the axes, the frame or the columns live through it the D = 6, 7 POSE forms spill to scratch.
      double J6[6][D];
      static_for<0, D>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        const double* w = A.zax[k];
        const double* o = A.org[k];
        const double rx = F.t[0] - o[0], ry = F.t[1] - o[1], rz = F.t[2] - o[2];
        const double v[3] = {w[1] * rz - w[2] * ry, w[2] * rx - w[0] * rz, w[0] * ry - w[1] * rx};
        const bool live = k <= a.link;
        J6[0][k] = live ? F.c0[0] * w[0] + F.c0[1] * w[1] + F.c0[2] * w[2] : 0.0;
        J6[1][k] = live ? F.c1[0] * w[0] + F.c1[1] * w[1] + F.c1[2] * w[2] : 0.0;
        J6[2][k] = live ? F.c2[0] * w[0] + F.c2[1] * w[1] + F.c2[2] * w[2] : 0.0;
        J6[3][k] = live ? F.c0[0] * v[0] + F.c0[1] * v[1] + F.c0[2] * v[2] : 0.0;
        J6[4][k] = live ? F.c1[0] * v[0] + F.c1[1] * v[1] + F.c1[2] * v[2] : 0.0;
        J6[5][k] = live ? F.c2[0] * v[0] + F.c2[1] * v[1] + F.c2[2] * v[2] : 0.0;
      });
      double Hm[ROWS][NC];
      if constexpr (ROWS == 6) {
#pragma unroll
        for (int i = 0; i < 6 * D; i++) s_J[i][threadIdx.x] = J6[i / D][i % D];
        double Hep[36];
        pose3_logmap_derivative(e, Hep);   // e == et here: the accepted point's log map
#pragma unroll
        for (int i = 0; i < 36; i++) Hm[i / 6][i % 6] = Hep[i];
#pragma unroll
        for (int i = 0; i < 6 * D; i++) J6[i / D][i % D] = s_J[i][threadIdx.x];
      } else {
        double Her[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (orient) rot3_logmap_derivative(et, Her);   // Pose3::rotation(H) = [I 0]
#pragma unroll
        for (int i = 0; i < 9; i++) Hm[i / 3][i % 3] = orient ? Her[i] : Rm[i];   // Pose3::translation(H) = [0 R]
      }
#pragma unroll
      for (int k = 0; k < D; k++)
#pragma unroll
        for (int i = 0; i < ROWS; i++) {
          double s = 0;
#pragma unroll
          for (int cc = 0; cc < NC; cc++) {
            double x;
            if constexpr (ROWS == 6) x = J6[cc][k];
            else x = orient ? J6[cc][k] : J6[3 + cc][k];
            s += Hm[i][cc] * x;
          }
          H[i][k] = scale(i) * s;
        }
    } else {
      lam = fmin(lam * a.lam_factor, a.lam_hi);
    }
    first = false;
    if (it >= a.max_iter) break;   // status: MAX_ITER_REACHED

    // the step: A = H^ H^T + lambda I, Cholesky, y = A^-1 e^, dq = -H^T y
    double L[ROWS * (ROWS + 1) / 2], y[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; i++)
#pragma unroll
      for (int j = 0; j <= i; j++) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < D; k++) s += H[i][k] * H[j][k];
        L[ik_tri(i, j)] = i == j ? s + lam : s;
      }
    bad = false;
#pragma unroll
    for (int j = 0; j < ROWS; j++) {
      double d = L[ik_tri(j, j)];
#pragma unroll
      for (int k = 0; k < j; k++) d -= L[ik_tri(j, k)] * L[ik_tri(j, k)];
      if (!(d > 0.0)) bad = true;
      const double ljj = sqrt(d);
      L[ik_tri(j, j)] = ljj;
#pragma unroll
      for (int i = j + 1; i < ROWS; i++) {
        double s = L[ik_tri(i, j)];
#pragma unroll
        for (int k = 0; k < j; k++) s -= L[ik_tri(i, k)] * L[ik_tri(j, k)];
        L[ik_tri(i, j)] = s / ljj;
      }
    }
#pragma unroll
    for (int i = 0; i < ROWS; i++) {   // L z = e^
      double s = scale(i) * e[i];
#pragma unroll
      for (int k = 0; k < i; k++) s -= L[ik_tri(i, k)] * y[k];
      y[i] = s / L[ik_tri(i, i)];
    }
#pragma unroll
    for (int i = ROWS - 1; i >= 0; i--) {   // L^T y = z
      double s = y[i];
#pragma unroll
      for (int k = i + 1; k < ROWS; k++) s -= L[ik_tri(k, i)] * y[k];
      y[i] = s / L[ik_tri(i, i)];
    }
#pragma unroll
    for (int k = 0; k < D; k++) {
      double s = 0;
#pragma unroll
      for (int r = 0; r < ROWS; r++) s += H[r][k] * y[r];
      qt[k] = bad ? q[k] : ik_clamp(q[k] - s, a.down[k], a.up[k]);
    }
  }

#pragma unroll
  for (int k = 0; k < D; k++)
    if (a.conf) a.conf[(size_t)p * D + k] = q[k];
  if (a.residual) {
    double rw = 0.0, rt = 0.0;
    if constexpr (ROWS == 6) {
      rw = ik_norm3(e);
      rt = ik_norm3(e + 3);
    } else {
      if (orient) rw = ik_norm3(e);
      else rt = ik_norm3(e);
    }
    a.residual[(size_t)p * 2] = rw;
    a.residual[(size_t)p * 2 + 1] = rt;
  }
  if (a.iters) a.iters[p] = it;
  if (a.status) a.status[p] = status;
}

// SDIM: 2 / 3, or 0 without a field (clearance +inf, out_of_range 0)
template <int AD, int SDIM>
__global__ __launch_bounds__(64) void k_ik_rows(const RobotDev* __restrict__ Rg, SdfDev sdf, IkRows a) {
  using K = Kin<GPMP2MI_ROBOT_ARM, AD, 0>;
  constexpr int D = AD;
  __shared__ RobotDev R;
  stage_robot(&R, Rg);
  const long long p = blockIdx.x * 64ll + threadIdx.x;
  if (p >= (long long)a.G * a.M) return;
  double q[D];
#pragma unroll
  for (int k = 0; k < D; k++) q[k] = a.conf[(size_t)p * D + k];
  double clr = HUGE_VAL;
  int oor = 0;
  if constexpr (SDIM != 0) {
    typename K::Axes A;   // filled by the walk, never read here
    K::walk(R, q, A, [&](int s, const double (&pt)[3], auto) {
      // negated conjunction: a NaN centre fails every comparison and counts as out of range (k_score)
      bool in = pt[0] >= sdf.ox && pt[0] <= sdf.hix && pt[1] >= sdf.oy && pt[1] <= sdf.hiy;
      if (SDIM == 3) in = in && pt[2] >= sdf.oz && pt[2] <= sdf.hiz;
      if (!in) {
        oor++;
        return;
      }
      double d, gx, gy, gz;
      if (SDIM == 3) (void)sdf3_lookup(sdf, pt[0], pt[1], pt[2], d, gx, gy, gz);
      else (void)sdf2_lookup(sdf, pt[0], pt[1], d, gx, gy);
      const double cl = d - R.sph_r[s];
      if (cl < clr) clr = cl;
    });
  }
  bool el = a.status[p] == GPMP2MI_IK_CONVERGED;
  if (SDIM != 0) el = el && clr >= a.required_clearance && (!a.require_in_range || oor == 0);
  double score = (double)(int)(p % a.M);
  if (a.has_near) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < D; k++) {   // the roundings of s_i in k_traj_pairs
      const double df = __dsub_rn(q[k], a.near_conf[k]);
      s = __fma_rn(a.w[k], __dmul_rn(df, df), s);
    }
    score = __dsqrt_rn(s);
  }
  if (a.clearance) a.clearance[p] = clr;
  if (a.oor) a.oor[p] = oor;
  a.score[p] = score;
  a.eligible[p] = el ? 1 : 0;
#pragma unroll
  for (int k = 0; k < D; k++) {
    a.stage[(size_t)p * 2 * D + k] = q[k];
    a.stage[(size_t)p * 2 * D + D + k] = 0.0;
  }
}

__global__ __launch_bounds__(64) void k_ik_goal_copy(IkGoalCopy a) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const int nm = a.n_modes[g];
  int cnt = 0;
  for (int m = tid; m < a.M; m += 64) cnt += a.status[(size_t)g * a.M + m] == GPMP2MI_IK_CONVERGED ? 1 : 0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
  if (tid == 0) {
    if (a.n_goals) a.n_goals[g] = nm;
    if (a.n_converged) a.n_converged[g] = cnt;
    if (a.out_n_eligible) a.out_n_eligible[g] = a.n_eligible[g];
  }
  for (int k = tid; k < a.max_goals; k += 64) {
    const size_t o = (size_t)g * a.max_goals + k;
    if (k >= nm) {
      if (a.goal_seed) a.goal_seed[o] = -1;
      continue;
    }
    const int L = a.leaders[(size_t)g * a.M + k];
    const size_t row = (size_t)g * a.M + L;
    if (a.goal_seed) a.goal_seed[o] = L;
    if (a.goal_score) a.goal_score[o] = a.score[row];
    if (a.goal_clearance) a.goal_clearance[o] = a.clearance[row];
    if (a.goal_conf)
      for (int d = 0; d < a.D; d++) a.goal_conf[o * a.D + d] = a.conf[row * a.D + d];
  }
}

#define G2_IK_DOFS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7)

int launch_ik(const RobotDev& h, const RobotDev* R, const IkArgs& a, hipStream_t st) {
  const long long P = (long long)a.G * a.M;
  if (P <= 0) return GPMP2MI_OK;
  const dim3 grid((unsigned)((P + 63) / 64)), block(64);
  const bool pose = a.mode == GPMP2MI_WORKSPACE_POSE;
  switch (h.dof) {
#define G2_IK_CASE(DD)                                           \
  case DD:                                                       \
    if (pose) k_ik<DD, 6><<<grid, block, 0, st>>>(R, a);         \
    else k_ik<DD, 3><<<grid, block, 0, st>>>(R, a);              \
    break;
    G2_IK_DOFS(G2_IK_CASE)
#undef G2_IK_CASE
    default: set_error("inverse kinematics is instantiated for arms of 1..7 joints"); return GPMP2MI_ERR_UNSUPPORTED;
  }
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_ik_rows(const RobotDev& h, const RobotDev* R, const SdfDev* s, const IkRows& a, hipStream_t st) {
  const long long P = (long long)a.G * a.M;
  if (P <= 0) return GPMP2MI_OK;
  const dim3 grid((unsigned)((P + 63) / 64)), block(64);
  const SdfDev sd = s ? *s : SdfDev{};
  const int sdim = s ? s->dim : 0;
  switch (h.dof) {
#define G2_IK_CASE(DD)                                                          \
  case DD:                                                                      \
    if (sdim == 3) k_ik_rows<DD, 3><<<grid, block, 0, st>>>(R, sd, a);          \
    else if (sdim == 2) k_ik_rows<DD, 2><<<grid, block, 0, st>>>(R, sd, a);     \
    else k_ik_rows<DD, 0><<<grid, block, 0, st>>>(R, sd, a);                    \
    break;
    G2_IK_DOFS(G2_IK_CASE)
#undef G2_IK_CASE
    default: set_error("inverse kinematics is instantiated for arms of 1..7 joints"); return GPMP2MI_ERR_UNSUPPORTED;
  }
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_ik_goal_copy(const IkGoalCopy& a, int G, hipStream_t st) {
  if (G <= 0) return GPMP2MI_OK;
  k_ik_goal_copy<<<dim3(G), dim3(64), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

}  // namespace g2
