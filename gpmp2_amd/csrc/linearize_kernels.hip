// linearize_kernels.hip -- the first launch of every pass: one lane per evaluation point
// (support state or GP-interpolated sub-step) of every trajectory.  interpolate -> FK -> sphere centres -> packed-cell
// SDF lookup -> hinge -> per-point  G = J^T J / sigma^2 (DxD packed), g = J^T r / sigma^2, e = r^T r / sigma^2, plus the
// GP-prior residual of each interval.  (ObstacleSDFFactor / ObstacleSDFFactorGP / GaussianProcessPriorLinear
// evaluateError + NoiseModelFactor::linearize + WhitenSystem.)
//   k_linearize     : every robot; one wavefront per 64 points, or two that split the spheres (fixed-base arms)
//   k_linearize_arm : fixed-base arms; four wavefronts that share one walk of the chain, the fused finish, the error shares
#include "dispatch.h"
#include "device_math.h"
#include "plan.h"
#include "tiles.h"
#include "cr_schedule.h"
#include "rec_pieces.h"
#include "plan_device.h"

namespace g2 {

#ifdef G2_STAMPS
#define G2_LSTAMP(k) do { if (chunk == 1 && threadIdx.x == 0 && pb.iters[b] == G2_STAMP_ITER) pb.stamps[(size_t)b * 64 + 48 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define G2_LSTAMP(k) do {} while (0)
#endif
// NSPLIT = 1: one wavefront per 64 evaluation points.  NSPLIT = 2 (fixed-base arms): a workgroup of two wavefronts per
// 64 points -- both walk the kinematic chain (replicated) but each visits only the body spheres s % 2 == its index,
// so a point's 16 serial lookup / Jacobian steps become 8; the partial records are summed through LDS (w0 += w1),
// wavefront 0 stores the record while wavefront 1 evaluates the GP prior.  Splitting over LANES cannot work (lanes with
// different sphere subsets diverge and take turns); splitting over four wavefronts needs <= 168 VGPRs for all
// workgroups to be resident and spills (measured: 34.8 us against 18.1 us for two and 22.2 us for one at 64
// trajectories).  Register budget: 2 wavefronts per SIMD (<= 256 VGPRs) for arms -- at 1 024 trajectories that alone
// takes the unsplit kernel from 86.7 to 74.2 us, the split one to 69.3 us.
template <int KIND, int AD, int AD2, int SDIM, int NSPLIT>
__global__ __launch_bounds__(64 * NSPLIT, KIND == GPMP2MI_ROBOT_ARM ? 2 : 1) void k_linearize(const RobotDev* __restrict__ Rg, SdfDev sdf,
                                                            const PlanParams* __restrict__ pp,
                                                            PlanBuffers pb, const double* __restrict__ traj,
                                                            int bufsel, const int* __restrict__ active) {
  using K = Kin<KIND, AD, AD2>;
  constexpr int D = K::DOF, n = 2 * D, NG = D * (D + 1) / 2;
  const PlanParams& P = *pp;
  const int nchunk = P.Ppad / 64;
  const int b = blockIdx.x / nchunk, chunk = blockIdx.x - b * nchunk;
  if (active && !active[b]) return;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
#ifdef G2_WGTIMES
  if (threadIdx.x == 0) pb.stamps[(size_t)blockIdx.x * 2] = wall_clock64();
#endif
  double* __restrict__ rec = rec_of(pb, pb.which[b], bufsel);
  double* __restrict__ gpu = gpu_of(pb, pb.which[b], bufsel);
  G2_LSTAMP(0);
  // robot model -> LDS: the global loads are issued first and committed after the state loads and
  // the GP interpolation below, so their latency overlaps
  __shared__ RobotDev R;
  constexpr int NT = 64 * NSPLIT, RN = sizeof(RobotDev) / 4, RPT = (RN + NT - 1) / NT;
  int rtmp[RPT];
#pragma unroll
  for (int u = 0; u < RPT; u++) {
    const int idx = threadIdx.x + NT * u;
    rtmp[u] = idx < RN ? reinterpret_cast<const int*>(Rg)[idx] : 0;
  }
  const int p_raw = chunk * 64 + lane;
  const int p = min(p_raw, P.P - 1);  // tail lanes shadow the last point until the barrier below
  const int N = P.N, I = P.I;
  int i = 0, j = I;
  if (p > 0) {
    const int t = p - 1;
    i = 1 + t / (I + 1);
    j = t - (i - 1) * (I + 1);
  }
  const bool unary = (j == I);
  const double* z1 = traj + ((size_t)b * (N + 1) + i) * n;          // state i
  const double* z0 = (i > 0) ? z1 - n : z1;                          // state i-1 (only used if i > 0)
  double x0[D], v0[D], x1[D], v1[D], q[D];
#pragma unroll
  for (int k = 0; k < D; k++) {
    x1[k] = z1[k];
    v1[k] = z1[D + k];
    x0[k] = (i > 0) ? z0[k] : 0.0;
    v0[k] = (i > 0) ? z0[D + k] : 0.0;
  }
  if (unary) {
#pragma unroll
    for (int k = 0; k < D; k++) q[k] = x1[k];
  } else {
    const GpCoef c = P.coef[j];
    if constexpr (K::BASE == 3) {
      // GaussianProcessInterpolatorPose2Vector: the configuration now, the pose blocks of its four Jacobians when the
      // record is stored (36 doubles that would otherwise stay live across the whole sphere loop)
      lie_interpolate<D>(c, x0, v0, x1, v1, q, nullptr);
    } else {
#pragma unroll
      for (int k = 0; k < D; k++) q[k] = c.l11 * x0[k] + c.l12 * v0[k] + c.p11 * x1[k] + c.p12 * v1[k];
    }
  }

#pragma unroll
  for (int u = 0; u < RPT; u++) {
    const int idx = threadIdx.x + NT * u;
    if (idx < RN) reinterpret_cast<int*>(&R)[idx] = rtmp[u];
  }
  __syncthreads();
  if (NSPLIT == 1 && p_raw >= P.P) return;   // (split form: tail lanes keep shadowing the last point, stores are predicated)
  G2_LSTAMP(1);
  double G[NG], gv[D], e = 0.0;
#pragma unroll
  for (int k = 0; k < NG; k++) G[k] = 0.0;
#pragma unroll
  for (int k = 0; k < D; k++) gv[k] = 0.0;

  if (!(P.obs_skip_first && p == 0)) {
    const double eps = P.eps;
    double hx, hy, hz, r;
    auto accumulate = [&](const double (&Jc)[D][3], auto nc) {
      // columns >= NC of this sphere's Jacobian are zero, and so are the columns [NB, FIRST) of the OTHER arm of a
      // two-arm robot: those entries of g and G are never touched (the arm-A x arm-B block of G stays a compile-time
      // zero and takes no registers)
      constexpr int NC = decltype(nc)::value, FIRST = decltype(nc)::first, NB = K::NB;
      auto live = [](int k) { return !(k >= NB && k < FIRST); };
      double Jr[NC];
#pragma unroll
      for (int k = 0; k < NC; k++)
        Jr[k] = hx * Jc[k][0] + hy * Jc[k][1] + (SDIM == 3 ? hz * Jc[k][2] : 0.0);
      e += r * r;
#pragma unroll
      for (int k = 0; k < NC; k++) {
        if (!live(k)) continue;
        gv[k] += Jr[k] * r;
#pragma unroll
        for (int k2 = k; k2 < NC; k2++)
          if (live(k2)) G[k * D - (k * (k - 1)) / 2 + (k2 - k)] += Jr[k] * Jr[k2];
      }
    };
    K::visit_spheres(
        R, q,
        [&](int s, const double (&pt)[3]) {
          if (s < 11) G2_LSTAMP(2 + s);
          r = hinge_obstacle<SDIM>(sdf, pt[0], pt[1], pt[2], R.sph_r[s] + eps, hx, hy, hz);
          // inactive hinge (or out of the field): zero residual row, nothing to accumulate --
          // and the sphere's Jacobian is never formed
          return !(hx == 0.0 && hy == 0.0 && hz == 0.0 && r == 0.0);
        },
        [&](int, const double (&)[3], const double (&Jc)[D][3], auto nc) { accumulate(Jc, nc); }, wv, NSPLIT);
  }
  if constexpr (NSPLIT > 1) {
    // partial records -> wavefront 0 through LDS: w0 += w1
    static_assert(NSPLIT == 2, "two wavefronts per point set");
    constexpr int RV = NG + D + 1;
    __shared__ double part[RV][64];
    if (wv == 1) {
#pragma unroll
      for (int k = 0; k < NG; k++) part[k][lane] = G[k];
#pragma unroll
      for (int k = 0; k < D; k++) part[NG + k][lane] = gv[k];
      part[NG + D][lane] = e;
    }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
      for (int k = 0; k < NG; k++) G[k] += part[k][lane];
#pragma unroll
      for (int k = 0; k < D; k++) gv[k] += part[NG + k][lane];
      e += part[NG + D][lane];
    }
  }
  const bool store_ok = (NSPLIT == 1) || (p_raw < P.P);
  G2_LSTAMP(13);
  const double w = P.obs_w;
  // point-major record: this lane's REC values are one contiguous run, stored in 16-B pieces (split form: wavefront 0
  // holds the sums; the last wavefront takes the GP prior below, so the two tails run side by side)
  if (NSPLIT == 1 || wv == 0) {
    constexpr int RECL = NG + D + 1 + (K::BASE == 3 ? 36 : 0);
    double rv[RECL + 1];
#pragma unroll
    for (int k = 0; k < NG; k++) rv[k] = G[k] * w;
#pragma unroll
    for (int k = 0; k < D; k++) rv[NG + k] = gv[k] * w;
    rv[NG + D] = e * w;
    if constexpr (K::BASE == 3) {  // pose blocks of the four interpolation Jacobians
      double Mlie[4][9];
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int t = 0; t < 9; t++) Mlie[m][t] = 0.0;
      if (!unary) {
        double a0[D], b0[D], a1[D], b1[D], qq[D];
#pragma unroll
        for (int k = 0; k < D; k++) {
          a1[k] = z1[k];
          b1[k] = z1[D + k];
          a0[k] = z0[k];
          b0[k] = z0[D + k];
        }
        lie_interpolate<D>(P.coef[j], a0, b0, a1, b1, qq, Mlie);
      }
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int t = 0; t < 9; t++) rv[NG + D + 1 + m * 9 + t] = Mlie[m][t];
    }
    rv[RECL] = 0.0;
    double2* rb = reinterpret_cast<double2*>(rec + ((size_t)b * P.Ppad + p) * P.RECS);
    const int nst = P.RECS >> 1;   // REC <= RECL: mobile robots without interpolation store the short record
#pragma unroll
    for (int k = 0; k < (RECL + 1) / 2; k++)
      if (k < nst && store_ok) rb[k] = double2{rv[2 * k], rv[2 * k + 1]};
  }

  G2_LSTAMP(14);
  // GP prior of the interval ending at state i.  Vector spaces: GaussianProcessPriorLinear
  // (gp/GaussianProcessPriorLinear.h:57-83) r = Phi z_{i-1} - z_i.  Pose2 robots:
  // GaussianProcessPriorLie<Pose2Vector> (gp/GaussianProcessPriorLie.h:61-86)
  // r = [Log(x1^-1 x2) - v1 dt ; v2 - v1] plus the pose blocks of its Jacobians.
  // Both: u = Q^-1 r (Q^-1 = B(dt) (x) Qc^-1), energy r^T u.
  if (unary && i > 0 && store_ok && (NSPLIT == 1 || wv == NSPLIT - 1)) {
    double rx[D], rv[D], sx[D], sv[D];
    double* gb = gpu + ((size_t)b * P.Npad + i) * P.GPS;
    if constexpr (NSPLIT > 1) {   // the states were not kept in registers across the sphere loop: fetch them again
#pragma unroll
      for (int k = 0; k < D; k++) {
        x1[k] = z1[k];
        v1[k] = z1[D + k];
        x0[k] = z0[k];
        v0[k] = z0[D + k];
      }
    }
    if constexpr (K::BASE == 3) {
      const P2 p1{x0[0], x0[1], x0[2]}, p2{x1[0], x1[1], x1[2]};
      const P2 bt = pose2_between(p1, p2);
      double lg[3], Hinv[9], Hc1[9], Hlog[9], T[9], J1[9];
      pose2_logmap(bt, lg);
      pose2_adjoint(p1, Hinv);                  // Inverse: H = -Ad(p1)
      pose2_adjoint(pose2_inverse(p2), Hc1);    // Compose(a, b): H1 = Ad(b^-1)
      pose2_logmap_derivative(bt, Hlog);
      mat3_mul(Hlog, Hc1, T);
      mat3_mul(T, Hinv, J1);
#pragma unroll
      for (int k = 0; k < 9; k++) {
        gb[n + 1 + k] = -J1[k];
        gb[n + 1 + 9 + k] = Hlog[k];
      }
#pragma unroll
      for (int k = 0; k < D; k++) {
        const double r = (k < 3) ? lg[k] : (x1[k] - x0[k]);
        rx[k] = r - v0[k] * P.delta_t;
        rv[k] = v1[k] - v0[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < D; k++) {
        rx[k] = x0[k] + P.delta_t * v0[k] - x1[k];
        rv[k] = v0[k] - v1[k];
      }
    }
#pragma unroll
    for (int k = 0; k < D; k++) {
      double ax = 0, av = 0;
#pragma unroll
      for (int m = 0; m < D; m++) {
        ax += P.Qc_inv[k * D + m] * rx[m];
        av += P.Qc_inv[k * D + m] * rv[m];
      }
      sx[k] = ax;
      sv[k] = av;
    }
    double en = 0.0;
#pragma unroll
    for (int k = 0; k < D; k++) {
      const double ux = P.Winv[0] * sx[k] + P.Winv[1] * sv[k];
      const double uv = P.Winv[2] * sx[k] + P.Winv[3] * sv[k];
      gb[k] = ux;
      gb[D + k] = uv;
      en += rx[k] * ux + rv[k] * uv;
    }
    gb[n] = en;
  }
  G2_LSTAMP(15);
#ifdef G2_WGTIMES
  if (threadIdx.x == 0) pb.stamps[(size_t)blockIdx.x * 2 + 1] = wall_clock64();
#endif
}

// k_linearize for fixed-base arms, round 3: NW wavefronts per 64 evaluation points that SHARE one walk of the
// kinematic chain instead of replicating it.
//   phase 1  every wavefront interpolates the point's configuration (replicated: 28 loads, 28 FMAs) and takes the
//            sin / cos of the joints j % NW == its index -> LDS
//   phase 2  wavefront 0 walks the chain once (AD dependent frame advances) and leaves, per link, the columns c0, c2
//            and the origin t of its frame in LDS (9 doubles per lane and link; c1 = c2 x c0 is recomputed where a
//            sphere centre needs it).  Axis and origin of joint k are c2 and t of frame k - 1 (the base frame for k = 0).
//            Meanwhile wavefront 1 forms the prior / limit share and wavefront 2 evaluates the GP prior of the chunk's
//            support states (states in LDS and the plan's constants: nothing of it waits for the chain)
//   phase 3  wavefront w visits the spheres s % NW == w: centre from its link's frame, SDF lookup, hinge, and for the
//            active lanes the Jacobian columns z_k x (p - o_k) of the joints below the link, accumulated as before
//   phase 4  partial records summed over the wavefronts in a fixed tree order (w0 + w2) + (w1 + w3) through LDS (the
//            frames' bytes): wavefronts 0 and 1 leave w0 + w2 and w1 + w3 there, and all four wavefronts form the last
//            add and the scaling and store the chunk's 64 records -- one run of memory -- in 16-B pieces in memory order
//            (rec_pieces.h): 1 KiB per wavefront and store instruction.  (Wavefront 0 alone, each lane its own record at a
//            stride of 288 B, was 18 store instructions of 64 partial-line requests at the very end of the longest
//            wavefront; the GP prior sat behind the last barrier on wavefront 3.  Linearization of passes 1 - 4 of the
//            flagship: 20.9 / 26.3 / 26.0 / 25.6 -> 18.7 / 24.5 / 24.6 / 24.0 us)
// Against the two-wavefront split above (both wavefronts walk the chain and keep all joint axes in registers, 252
// VGPRs, two wavefronts per SIMD) the dependent chain of a wavefront is sin/cos of two joints + 4 spheres instead of
// 7 joints + 8 spheres, and 168 VGPRs leave room for three wavefronts per SIMD: 640 workgroups x 4 wavefronts of the
// 64-restart batch are resident at once.
// Fused finish (Gauss-Newton fast path, `dst` != nullptr): the kernel first APPLIES the step the previous pass solved, what
// k_finish_step did chip-wide in a launch of its own (7 - 8 us).  The step kernel left the solution of the blocks whose
// tree index v = state + 1 (cr_schedule.h, rooted schedule) is a multiple of 8 (pb.xg); every workgroup back-substitutes
// levels 4, 2, 1 for the blocks the 12 - 18 states of its 64 points need (crr_window: bit masks over FXS tree indices from a
// multiple of 8), adds the step to the states it reads from `traj` (the buffer of the previous pass, which nobody writes
// during this kernel), keeps the new states in LDS and writes those whose unary point lies in its chunk to `dst`.  The
// two state buffers of a plan (cur / last) swap roles from pass to pass: `last` is the buffer the step started from.
// Error shares (linearization at `cur`: bufsel == 0, not `trial`): the kernel holds every term of the graph error
// 0.5 (sum of point errors + sum of GP energies + prior / limit terms), so each workgroup leaves its chunk's three sums in
// pb.cshare -- obstacle (wavefront 0, the values that are stored in the records), GP prior (wavefront 2), and the prior /
// limit / state-prior terms of the states it owns (wavefront 1, from the states in LDS, while wavefront 0 walks the chain).
// The Gauss-Newton step control reads them (error_from_shares) instead of a sum over k_assemble's blocks.
template <int AD, int SDIM, int NW>
__global__ __launch_bounds__(64 * NW, 3) void k_linearize_arm(PassConsts pc, const RobotDev* __restrict__ Rg, SdfDev sdf,
                                                               const PlanParams* __restrict__ pp, PlanBuffers pb,
                                                               const double* __restrict__ traj, int bufsel,
                                                               const int* __restrict__ active, double* __restrict__ dst,
                                                               int pass, int trial) {
  static_assert(NW == 4, "tree reduction below");
  constexpr int D = AD, n = 2 * D, NG = D * (D + 1) / 2, RV = NG + D + 1;
  constexpr int FR = 9;                                  // doubles per lane and link: c0, c2, t
  constexpr int ROWS_F = FR * AD, ROWS_SC = 2 * AD;
  constexpr int ROWS_P = (NW / 2) * rec_lds_stride(RV);  // partial records: NW / 2 buffers of 64 points (rec_pieces.h)
  constexpr int ROWS = (ROWS_F + ROWS_SC > ROWS_P) ? ROWS_F + ROWS_SC : ROWS_P;
  const PlanParams& P = *pp;
  // head: the sizes come with the kernel arguments (pc), and the trajectory's own words -- active, which, stepped -- are
  // requested together before `active` is tested; the model, the states and the step stay behind that test
  const int nchunk = pc.Ppad / 64;
  const int b = blockIdx.x / nchunk, chunk = blockIdx.x - b * nchunk;
  int act = (active ? active : pb.active)[b];
  int wh = pb.which[b];
  int stp = pb.stepped[b];
  head_batch_end(act, wh, stp);
  if (active && !act) return;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  double* __restrict__ rec = rec_of(pb, wh, bufsel);
  double* __restrict__ gpu = gpu_of(pb, wh, bufsel);
  G2_LSTAMP(0);
  __shared__ RobotDev R;
  __shared__ double buf[ROWS][64];                       // [0, ROWS_F) frames, [ROWS_F, ROWS_F + ROWS_SC) sin / cos; later the partial records
  constexpr int NT = 64 * NW, RN = sizeof(RobotDev) / 4, RPT = (RN + NT - 1) / NT;
  int rtmp[RPT];
#pragma unroll
  for (int u = 0; u < RPT; u++) {
    const int idx = threadIdx.x + NT * u;
    rtmp[u] = idx < RN ? reinterpret_cast<const int*>(Rg)[idx] : 0;
  }
  const int p_raw = chunk * 64 + lane;
  const int p = min(p_raw, pc.P - 1);  // tail lanes shadow the last point, their stores are predicated
  const int N = pc.N, I = pc.I;
  int i = 0, j = I;
  if (p > 0) {
    const int t = p - 1;
    i = 1 + t / (I + 1);
    j = t - (i - 1) * (I + 1);
  }
  const bool unary = (j == I);
  const bool store_ok = p_raw < pc.P;
  // ---- the states this workgroup reads: [s0, s1]; through LDS (zn), with the pending step applied in the fused form
  double (*fx)[16] = reinterpret_cast<double (*)[16]>(&buf[0][0]);   // step of the blocks w0 .. w0 + 39 (buf is not in use yet)
  static_assert(FXS * 16 <= ROWS * 64, "the step window lives in the frame buffer");
  __shared__ double zn[ZNS][n];       // states s0 .. s0 + ZNS - 1 (ZNS, FXS: cr_schedule.h)
  const int p_lo = chunk * 64, p_hi = min(p_lo + 63, pc.P - 1);
  auto state_of = [&](int pt) { return pt == 0 ? 0 : 1 + (pt - 1) / (I + 1); };
  const int s1 = state_of(p_hi), s0 = max(0, state_of(p_lo) - 1), ns = s1 - s0 + 1;   // ns <= ZNS: launch_linearize checks
  const bool apply = dst != nullptr && stp == pass;
  const bool shares = bufsel == 0 && !trial;
  double* __restrict__ cshare = pb.cshare + ((size_t)b * nchunk + chunk) * 3;
  if (apply) {
    const double* fac = pb.fac + (size_t)b * (N + 1) * 3 * TILE_DBL;
    const double* xg = pb.xg + (size_t)b * (N + 1) * 16;
    // window in tree indices: the states s0 .. s1 are v = s0 + 1 .. s1 + 1 <= w0 + 7 + ZNS, their neighbours at distance 1, 2, 4
    // reach no further than the next multiple of 8, w0 + 32 < FXS
    const int w0 = (s0 + 1) & ~7, M = N + 1, c = lane & 15, g = lane >> 4;
    using u64 = unsigned long long;
    const CrrWindow win = crr_window(N, s0, s1, FXS);   // the blocks of levels 1, 2, 4 to solve here, the multiples of 8 to fetch
    const u64 need1 = win.need1, need2 = win.need2, need4 = win.need4, need8 = win.need8;
    // multiples of 8: solved by the step kernel
    for (u64 m = need8; m; m &= m - 1) {
      const int k = __builtin_ctzll(m);
      if (wv == ((k >> 3) & (NW - 1)) && lane < 16) fx[k][lane] = xg[(size_t)(w0 + k - 1) * 16 + lane];
    }
    __syncthreads();
    // Task t of a level (the t-th needed block) belongs to wavefront t % NW.  (Requesting the factor tiles ahead -- all twelve
    // of a wavefront at once, or one level ahead -- was slower: 21.0 / 20.2 against 19.5 us; 2 560 wavefronts x 21 KB.  Touching
    // one 8-byte word of each of their lines at this point, only when few trajectories are live, was slower as well, down to a
    // plan of 4 trajectories: DESIGN.md section 4.)
    auto level = [&](u64 need, int h) {
      int t = 0;
      for (u64 m = need; m; m &= m - 1, t++) {
        if ((t & (NW - 1)) != wv) continue;
        const int k = __builtin_ctzll(m), vb = w0 + k;
        const double* f = fac + (size_t)(vb - 1) * 3 * TILE_DBL;
        const Tile Wl = tile_load_rows<n>(f, lane), Wr = tile_load_rows<n>(f + TILE_DBL, lane);
        const Tile V = load_v<n>(f + 2 * TILE_DBL, h, N, lane);
        const double xl = (vb - h >= 1) ? fx[k - h][c] : 0.0;         // (k - h < 0 cannot happen: w0 is a multiple of 8)
        const double xr = (vb + h <= M) ? fx[k + h][c] : 0.0;
        const double x = cr_backsolve<n>(Wl, Wr, V, xl, xr, lane);
        if (g == 0) fx[k][c] = (c < n) ? x : 0.0;
      }
      __syncthreads();
    };
    level(need4, 4);
    level(need2, 2);
    level(need1, 1);
  }
  // trial-step path (`trial`): dst is the trial point, the step itself goes to pb.delta, and the workgroup leaves its share
  // of g.delta, |delta|^2, |g|^2 over the states it owns in pb.spart for k_decide (what k_finish_trial did per group of 8)
  double s_gd = 0.0, s_dd = 0.0, s_gg = 0.0;
  for (int e = threadIdx.x; e < ns * n; e += 64 * NW) {
    const int t = e / n, rho = e - t * n, st = s0 + t;
    const size_t k = ((size_t)b * (N + 1) + st) * n + rho;
    double z = traj[k];
    const double x = apply ? fx[st + 1 - ((s0 + 1) & ~7)][rho] : 0.0;
    z += x;                                       // Values::retract of a vector-valued state
    zn[t][rho] = z;
    const int pu = st * (I + 1);                  // the state's unary evaluation point: its owner writes the state
    if (dst != nullptr && pu >= p_lo && pu <= p_lo + 63) {
      dst[k] = z;
      if (trial && apply) {
        const double gk = pb.gvec[((size_t)b * (N + 1) + st) * 16 + rho];
        pb.delta[k] = x;
        s_gd = fma(gk, x, s_gd);
        s_dd = fma(x, x, s_dd);
        s_gg = fma(gk, gk, s_gg);
      }
    }
  }
  if (trial && apply) {   // fixed order: lanes (wave_sum), then wavefronts 0 .. NW - 1
    __shared__ double psum[NW][3];
    s_gd = wave_sum(s_gd);
    s_dd = wave_sum(s_dd);
    s_gg = wave_sum(s_gg);
    if (lane == 0) {
      psum[wv][0] = s_gd;
      psum[wv][1] = s_dd;
      psum[wv][2] = s_gg;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      double a = 0.0;
#pragma unroll
      for (int w = 0; w < NW; w++) a += psum[w][threadIdx.x];
      pb.spart[((size_t)b * nchunk + chunk) * 3 + threadIdx.x] = a;
    }
  }
  __syncthreads();
  const double* z1 = &zn[i - s0][0];                                 // state i
  const double* z0 = (i > 0) ? z1 - n : z1;                          // state i-1 (only used if i > 0)
  {
    double q[D];
    if (unary) {
#pragma unroll
      for (int k = 0; k < D; k++) q[k] = z1[k];
    } else {
      const GpCoef c = P.coef[j];
#pragma unroll
      for (int k = 0; k < D; k++) q[k] = c.l11 * z0[k] + c.l12 * z0[D + k] + c.p11 * z1[k] + c.p12 * z1[D + k];
    }
    // sin / cos of this wavefront's joints (the joint bias straight from the model in HBM: a uniform scalar load)
#pragma unroll
    for (int k = 0; k < AD; k++) {
      if (k % NW != wv) continue;
      double sn, cs;
      sincos(q[k] + Rg->bias[k], &sn, &cs);
      buf[ROWS_F + 2 * k][lane] = sn;
      buf[ROWS_F + 2 * k + 1][lane] = cs;
    }
  }
#pragma unroll
  for (int u = 0; u < RPT; u++) {
    const int idx = threadIdx.x + NT * u;
    if (idx < RN) reinterpret_cast<int*>(&R)[idx] = rtmp[u];
  }
  __syncthreads();
  G2_LSTAMP(1);
  if (wv == 0) {
    Frame F;
    frame_from_3x4(R.base, F);  // world_T_base
    static_for<0, AD>([&](auto jc) {
      constexpr int k = decltype(jc)::value;
      const double sn = buf[ROWS_F + 2 * k][lane], cs = buf[ROWS_F + 2 * k + 1][lane];
      dh_advance_sc(F, sn, cs, R.a[k], R.d[k], R.ca[k], R.sa[k]);
#pragma unroll
      for (int t = 0; t < 3; t++) {
        buf[FR * k + t][lane] = F.c0[t];
        buf[FR * k + 3 + t][lane] = F.c2[t];
        buf[FR * k + 6 + t][lane] = F.t[t];
      }
    });
  } else if (wv == 1 && shares) {
    // misc share: the entries of the states this chunk owns (the test that guards dst[k] = z above), from zn
    const int nxp = pb.xp_n[b];
    const bool every_state = misc_every_state(P, nxp);
    double acc = 0.0;
    for (int e = lane; e < ns * n; e += 64) {
      const int t = e / n, rho = e - t * n, st = s0 + t;
      const int pu = st * (I + 1);
      if (pu < p_lo || pu > p_lo + 63 || !(every_state || st == 0 || st == N)) continue;
      acc = misc_entry_add<false>(acc, P, pb, b, nxp, st, rho, &zn[t][0]);
    }
    acc = wave_sum(acc);
    if (lane == 0) cshare[2] = acc;
  } else if (wv == 2) {
    // GP prior of the interval ending at state i: GaussianProcessPriorLinear (gp/GaussianProcessPriorLinear.h:57-83),
    // r = Phi z_{i-1} - z_i, u = Q^-1 r (Q^-1 = B(dt) (x) Qc^-1), energy r^T u.  It needs the states in LDS and the plan's
    // constants only, so it runs here, while wavefront 0 walks the chain, and not behind the sphere loop
    double en = 0.0;
    if (unary && i > 0 && store_ok) {
      double rx[D], rv[D], sx[D], sv[D];
      double* gb = gpu + ((size_t)b * P.Npad + i) * P.GPS;
#pragma unroll
      for (int k = 0; k < D; k++) {
        rx[k] = z0[k] + P.delta_t * z0[D + k] - z1[k];
        rv[k] = z0[D + k] - z1[D + k];
      }
#pragma unroll
      for (int k = 0; k < D; k++) {
        double ax = 0, av = 0;
#pragma unroll
        for (int m = 0; m < D; m++) {
          ax += P.Qc_inv[k * D + m] * rx[m];
          av += P.Qc_inv[k * D + m] * rv[m];
        }
        sx[k] = ax;
        sv[k] = av;
      }
#pragma unroll
      for (int k = 0; k < D; k++) {
        const double ux = P.Winv[0] * sx[k] + P.Winv[1] * sv[k];
        const double uv = P.Winv[2] * sx[k] + P.Winv[3] * sv[k];
        gb[k] = ux;
        gb[D + k] = uv;
        en += rx[k] * ux + rv[k] * uv;
      }
      gb[n] = en;
    }
    if (shares) {   // GP share: the energies as stored
      const double gs = wave_sum(en);
      if (lane == 0) cshare[1] = gs;
    }
  }
  __syncthreads();
  G2_LSTAMP(2);
  double G[NG], gv[D], e = 0.0;
#pragma unroll
  for (int k = 0; k < NG; k++) G[k] = 0.0;
#pragma unroll
  for (int k = 0; k < D; k++) gv[k] = 0.0;
  if (!(P.obs_skip_first && p == 0)) {
    const double eps = P.eps;
    static_for<0, AD>([&](auto jc) {
      constexpr int L = decltype(jc)::value, NC = L + 1;     // link L: the joints 0 .. L move it
      for (int s = R.link_first[L]; s < R.link_first[L + 1]; s++) {
        if (s % NW != wv) continue;
        double c0[3], c2[3], o[3], pt[3];
#pragma unroll
        for (int t = 0; t < 3; t++) {
          c0[t] = buf[FR * L + t][lane];
          c2[t] = buf[FR * L + 3 + t][lane];
          o[t] = buf[FR * L + 6 + t][lane];
        }
        const double c1[3] = {c2[1] * c0[2] - c2[2] * c0[1], c2[2] * c0[0] - c2[0] * c0[2], c2[0] * c0[1] - c2[1] * c0[0]};
        const double cx = R.sph_c[3 * s], cy = R.sph_c[3 * s + 1], cz = R.sph_c[3 * s + 2];
#pragma unroll
        for (int t = 0; t < 3; t++) pt[t] = o[t] + c0[t] * cx + c1[t] * cy + c2[t] * cz;
        double hx, hy, hz;
        const double r = hinge_obstacle<SDIM>(sdf, pt[0], pt[1], pt[2], R.sph_r[s] + eps, hx, hy, hz);
        // inactive hinge (or out of the field): zero residual row, nothing to accumulate
        if (hx == 0.0 && hy == 0.0 && hz == 0.0 && r == 0.0) continue;
        double Jr[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) {
          double zx, zy, zz, ox, oy, oz;
          if (k == 0) {   // joint 0 sits in the base frame: R.base rows are (c0 c1 c2 t) per coordinate
            zx = R.base[2]; zy = R.base[6]; zz = R.base[10];
            ox = R.base[3]; oy = R.base[7]; oz = R.base[11];
          } else {
            zx = buf[FR * (k - 1) + 3][lane]; zy = buf[FR * (k - 1) + 4][lane]; zz = buf[FR * (k - 1) + 5][lane];
            ox = buf[FR * (k - 1) + 6][lane]; oy = buf[FR * (k - 1) + 7][lane]; oz = buf[FR * (k - 1) + 8][lane];
          }
          const double rx = pt[0] - ox, ry = pt[1] - oy, rz = pt[2] - oz;
          const double Jx = zy * rz - zz * ry, Jy = zz * rx - zx * rz, Jz = zx * ry - zy * rx;   // z_k x (p - o_k)
          Jr[k] = hx * Jx + hy * Jy + (SDIM == 3 ? hz * Jz : 0.0);
        }
        e += r * r;
#pragma unroll
        for (int k = 0; k < NC; k++) {
          gv[k] += Jr[k] * r;
#pragma unroll
          for (int k2 = k; k2 < NC; k2++) G[k * D - (k * (k - 1)) / 2 + (k2 - k)] += Jr[k] * Jr[k2];
        }
      }
    });
  }
  G2_LSTAMP(3);
  // partial records, fixed order: (w0 + w2) + (w1 + w3).  The two slots are point-major with an odd stride (rec_pieces.h)
  __syncthreads();   // every wavefront is done with the frames: their bytes now take the partial records
  constexpr int RECL = RV, RVP = rec_lds_stride(RECL), SLOT = 64 * RVP;
  static_assert(2 * SLOT <= ROWS * 64, "two partial records fit in the frame buffer");
  double* const part = &buf[0][0];
  auto put = [&](int slot) {
    double* q = part + slot * SLOT + lane * RVP;
#pragma unroll
    for (int k = 0; k < NG; k++) q[k] = G[k];
#pragma unroll
    for (int k = 0; k < D; k++) q[NG + k] = gv[k];
    q[NG + D] = e;
  };
  auto add = [&](int slot) {
    const double* q = part + slot * SLOT + lane * RVP;
#pragma unroll
    for (int k = 0; k < NG; k++) G[k] += q[k];
#pragma unroll
    for (int k = 0; k < D; k++) gv[k] += q[NG + k];
    e += q[NG + D];
  };
  if (wv >= 2) put(wv - 2);
  __syncthreads();
  if (wv < 2) {             // w0 + w2 back into slot 0, w1 + w3 into slot 1: each slot is read and rewritten by one wavefront
    add(wv);
    put(wv);
  }
  __syncthreads();
  G2_LSTAMP(13);
  // The record is (slot 0 + slot 1) * obs_w, the last add of the tree and the scaling.  All four wavefronts form and store it,
  // in 16-B pieces in memory order (rec_pieces.h): the chunk's records are one run of memory, a wavefront stores 1 KiB of it
  // per instruction.  (Wavefront 0 alone, each lane its own record, issued 18 stores of 64 separate 16-B requests.)
  const double w = P.obs_w;
  {
    const int npc = rec_piece_count(rec_live_points(P.P, p_lo), RECL);   // points at or beyond P.P are not written
    double* rchunk = rec + ((size_t)b * P.Ppad + p_lo) * P.RECS;
    constexpr int NIT = (64 * rec_npieces(RECL) + 64 * NW - 1) / (64 * NW);
#pragma unroll
    for (int it = 0; it < NIT; it++) {
      const int pe = threadIdx.x + 64 * NW * it;
      if (pe < npc) {
        const RecPiece pc = rec_piece(pe, RECL, P.RECS);
        const double* a = part + pc.src;
        const double v0 = (a[0] + a[SLOT]) * w;
        const double v1 = pc.padded ? 0.0 : (a[1] + a[SLOT + 1]) * w;
        *reinterpret_cast<double2*>(rchunk + pc.dst) = double2{v0, v1};
      }
    }
  }
  if (wv == 0 && shares) {   // obstacle share: the point errors as stored
    const double es = wave_sum(store_ok ? (e + part[SLOT + lane * RVP + NG + D]) * w : 0.0);
    if (lane == 0) cshare[0] = es;
  }
  G2_LSTAMP(14);
  G2_LSTAMP(15);
}

// dst / pass: fused finish of the Gauss-Newton fast path (k_linearize_arm; only with hp.fuse_finish): apply the step of
// pass - 1 to the states in `traj` and write the new states to `dst`; dst = nullptr: linearize `traj` as it is.
// hp.lin_split names the form that runs: 2 and 4 only ever on fixed-base arms (host/plan_create.hip choose_forms)
int launch_linearize(const RobotDev& h, const RobotDev* robot, const SdfDev& sdf, const PlanParams& hp,
                     const PlanBuffers& pb, const double* traj, int bufsel, const int* active,
                     hipStream_t st, double* dst, int pass, bool trial) {
  if (dst != nullptr && !(hp.fuse_finish && hp.lin_split == 4)) {
    set_error("fused finish asked of a plan that was not set up for it");
    return GPMP2MI_ERR_INVALID;
  }
  if (hp.lin_split == 4 && chunk_states(hp.I) > ZNS) {   // states per chunk kept in LDS by k_linearize_arm
    set_error("the four-wavefront linearization needs obs_check_inter >= 2");
    return GPMP2MI_ERR_INVALID;
  }
  // (a variant that kept 4-8 SDF cells in flight per lane was no faster: DESIGN.md section 4)
  const dim3 grid(hp.B * (hp.Ppad / 64));
  if (hp.lin_split == 4) {
    const dim3 block(256);
    if (sdf.dim == 3) {
      G2_DISPATCH_ROBOT_ARM_ONLY(h.arm_dof, (k_linearize_arm<AD_, 3, 4><<<grid, block, 0, st>>>(pass_consts(hp), robot, sdf, pb.params, pb, traj, bufsel, active, dst, pass, trial ? 1 : 0)));
    } else {
      G2_DISPATCH_ROBOT_ARM_ONLY(h.arm_dof, (k_linearize_arm<AD_, 2, 4><<<grid, block, 0, st>>>(pass_consts(hp), robot, sdf, pb.params, pb, traj, bufsel, active, dst, pass, trial ? 1 : 0)));
    }
  } else if (hp.lin_split == 2) {
    const dim3 block(128);
    if (sdf.dim == 3) {
      G2_DISPATCH_ROBOT_ARM_ONLY(h.arm_dof, (k_linearize<GPMP2MI_ROBOT_ARM, AD_, 0, 3, 2><<<grid, block, 0, st>>>(robot, sdf, pb.params, pb, traj, bufsel, active)));
    } else {
      G2_DISPATCH_ROBOT_ARM_ONLY(h.arm_dof, (k_linearize<GPMP2MI_ROBOT_ARM, AD_, 0, 2, 2><<<grid, block, 0, st>>>(robot, sdf, pb.params, pb, traj, bufsel, active)));
    }
  } else {
    const dim3 block(64);
    if (sdf.dim == 3) {
      G2_DISPATCH_ROBOT_H(h, (k_linearize<KIND_, AD_, AD2_, 3, 1><<<grid, block, 0, st>>>(robot, sdf, pb.params, pb, traj, bufsel, active)));
    } else {
      G2_DISPATCH_ROBOT_H(h, (k_linearize<KIND_, AD_, AD2_, 2, 1><<<grid, block, 0, st>>>(robot, sdf, pb.params, pb, traj, bufsel, active)));
    }
  }
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

}  // namespace g2
