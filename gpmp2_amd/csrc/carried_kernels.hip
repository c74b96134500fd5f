// carried_kernels.hip -- carried object (include/gpmp2mi.h "carried object"): A spheres rigidly attached to one link,
// against the static field.
//
//   k_carried_factor      the factor on M evaluations (gpmp2mi_carried_sphere_factor): one wavefront per evaluation, the
//                         device functions of k_carried_accumulate, rows to err / H.
//   k_carried_accumulate  the factor inside a plan.  One wavefront per (trajectory, support state of the range).  Every
//                         lane walks the chain to the link (the walk is uniform over the wavefront, so it costs what one
//                         lane's walk costs); lane k < D leaves column k of the link's body Jacobian in LDS.  The A
//                         spheres go through accumulate_sphere_rows (record_entries.h): chunks of 64, the range test, the
//                         field lookup and the hinge per lane, the active rows [h | r | w] through LDS -- the Jacobian
//                         row is formed by the active lanes only -- into the record entries a lane owns (RecAcc).  No
//                         rows, poses or Jacobians reach memory.
//   k_carried_clearance   the check of the executed trajectory, tiled as k_score is: a lane is a checked state
//                         (checked_config, score_select.h) of a tile of SCORE_TILE; each wavefront of the workgroup walks
//                         to the link, value only, and takes the spheres a % nsub; radii and centres of the set are
//                         staged in LDS once per workgroup; ONE record per workgroup (block_score_record).
//   k_carried_finish      reduces a row's records in index order to the five outputs and, when asked, applies the
//                         selection rule over the per-row scores of the existing stages.
//
// The range test stands in front of every lookup and is the negated conjunction of k_score: a NaN centre fails it,
// counts as out of range and is never turned into a cell index (sdf3_lookup's own test lets a NaN through).
// LDS: a row is MAXD + 3 = 21 doubles, the odd stride of k_selfpair_accumulate (selfpair_kernels.hip says why); with the
// twist columns [MAXD][6] that is 11.6 KB beside the robot model.
// Determinism: a sphere that is not active adds an exact zero, so skipping it changes no bit; the active rows of a state
// are added in sphere order, one accumulator per record entry, without atomics: the contribution of a state is a
// function of (A, D), the set and its own data.  The check sums in an order fixed by (N, inter_step, A).
#include <climits>

#include "device_math.h"
#include "dispatch.h"
#include "launch.h"
#include "link_frame.h"
#include "plan.h"
#include "record_entries.h"
#include "score_select.h"

namespace g2 {

constexpr int CR_LD = MAXD + 3;   // an LDS row: h [D], r, w; odd, see above

namespace {

// c = R o + t
__device__ __forceinline__ void carried_center(const double (&Rm)[9], const double (&t)[3], const double* o,
                                               double (&c)[3]) {
#pragma unroll
  for (int i = 0; i < 3; i++) c[i] = (Rm[i * 3] * o[0] + Rm[i * 3 + 1] * o[1] + Rm[i * 3 + 2] * o[2]) + t[i];
}

// the range test of k_score, a negated conjunction: a NaN centre fails every comparison
template <int SDIM>
__device__ __forceinline__ bool carried_in_range(const SdfDev& sdf, const double (&c)[3]) {
  bool in = c[0] >= sdf.ox && c[0] <= sdf.hix && c[1] >= sdf.oy && c[1] <= sdf.hiy;
  if (SDIM == 3) in = in && c[2] >= sdf.oz && c[2] <= sdf.hiz;
  return in;
}

// sphere a of the set at one configuration, for accumulate_sphere_rows: the link frame (Rm, t) and the columns of its
// body Jacobian tw [D][6] = [omega; v] are the state's; SphereHinge::n carries the field's gradient at the centre
template <int SDIM>
struct CarriedSpheres {
  const SdfDev& sdf;
  const double *radius, *centers;   // [A], [A][3] in the link frame
  const double (&Rm)[9];
  const double (&t)[3];
  const double (*tw)[6];
  double eps, w;
  int D;
  struct Pair {
    double o[3], w;
  };
  __device__ __forceinline__ SphereHinge hinge(int a, Pair& pr) const {
    SphereHinge hg;
    hg.active = false;
    hg.err = 0.0;
    hg.n[0] = hg.n[1] = hg.n[2] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) pr.o[i] = centers[a * 3 + i];
    pr.w = w;
    double c[3];
    carried_center(Rm, t, pr.o, c);
    if (!carried_in_range<SDIM>(sdf, c)) return hg;   // out of range: err 0, a zero row (ObstacleCost.h:31-38)
    double d, gx, gy, gz = 0.0;
    if (SDIM == 3) (void)sdf3_lookup(sdf, c[0], c[1], c[2], d, gx, gy, gz);
    else (void)sdf2_lookup(sdf, c[0], c[1], d, gx, gy);
    const double te = radius[a] + eps;
    hg.active = !(d > te);
    hg.err = hg.active ? te - d : 0.0;
    hg.n[0] = gx;
    hg.n[1] = gy;
    hg.n[2] = gz;
    return hg;
  }
  // h_k = -grad d . R (v_k + omega_k x o)
  __device__ __forceinline__ void row(const Pair& pr, const SphereHinge& hg, double* h) const {
    // grad d in the link frame: R^T n
    const double m0 = Rm[0] * hg.n[0] + Rm[3] * hg.n[1] + Rm[6] * hg.n[2];
    const double m1 = Rm[1] * hg.n[0] + Rm[4] * hg.n[1] + Rm[7] * hg.n[2];
    const double m2 = Rm[2] * hg.n[0] + Rm[5] * hg.n[1] + Rm[8] * hg.n[2];
    for (int k = 0; k < D; k++) {
      const double* col = tw[k];
      const double u0 = col[3] + (col[1] * pr.o[2] - col[2] * pr.o[1]);
      const double u1 = col[4] + (col[2] * pr.o[0] - col[0] * pr.o[2]);
      const double u2 = col[5] + (col[0] * pr.o[1] - col[1] * pr.o[0]);
      h[k] = -(m0 * u0 + m1 * u1 + m2 * u2);
    }
  }
};

// the link frame at q as (Rm, t), and column `lane` of the link's body Jacobian into tw (lanes below D)
template <int KIND, int AD, int AD2>
__device__ __forceinline__ void carried_link(const RobotDev& R, const double (&q)[Kin<KIND, AD, AD2>::DOF], int link,
                                             double (&Rm)[9], double (&t)[3], double (*tw)[6]) {
  using Kn = Kin<KIND, AD, AD2>;
  typename Kn::Axes A;
  Frame F;
  int nc, first;
  link_frame<KIND, AD, AD2>(R, q, link, A, F, nc, first);
  frame_rt(F, Rm, t);
  if (tw) {
    const int lane = threadIdx.x;
    double col[6];
    link_twist<KIND, AD, AD2>(A, F, nc, first, lane, col);
    if (lane < Kn::DOF)
#pragma unroll
      for (int i = 0; i < 6; i++) tw[lane][i] = col[i];
  }
}

}  // namespace

template <int KIND, int AD, int AD2, int SDIM>
__global__ __launch_bounds__(64) void k_carried_factor(const RobotDev* __restrict__ Rg, SdfDev sdf, int link, int A,
                                                        const double* __restrict__ radius,
                                                        const double* __restrict__ centers, double eps, int M,
                                                        const double* __restrict__ conf, double* __restrict__ err,
                                                        double* __restrict__ H) {
  using Kn = Kin<KIND, AD, AD2>;
  constexpr int D = Kn::DOF;
  __shared__ RobotDev R;
  __shared__ double tw[MAXD][6];
  stage_robot(&R, Rg);
  const size_t m = blockIdx.x;   // grid = M
  const int lane = threadIdx.x;
  double q[D];
#pragma unroll
  for (int k = 0; k < D; k++) q[k] = conf[m * D + k];
  double Rm[9], t[3];
  carried_link<KIND, AD, AD2>(R, q, link, Rm, t, tw);
  __syncthreads();
  const CarriedSpheres<SDIM> sph{sdf, radius, centers, Rm, t, tw, eps, 1.0, D};
  for (int a = lane; a < A; a += 64) {
    typename CarriedSpheres<SDIM>::Pair pr;
    const SphereHinge hg = sph.hinge(a, pr);
    err[m * A + a] = hg.err;
    if (!H) continue;
    double* h = H + (m * A + a) * D;
    if (hg.active) sph.row(pr, hg, h);
    else
      for (int k = 0; k < D; k++) h[k] = 0.0;
  }
}

template <int KIND, int AD, int AD2, int SDIM>
__global__ __launch_bounds__(64) void k_carried_accumulate(const RobotDev* __restrict__ Rg, SdfDev sdf,
                                                            const PlanParams* __restrict__ pp, PlanBuffers pb,
                                                            PlanExtras ex, const double* __restrict__ traj, int bufsel,
                                                            const int* __restrict__ active) {
  using Kn = Kin<KIND, AD, AD2>;
  constexpr int D = Kn::DOF;
  __shared__ RobotDev R;
  __shared__ double rows[64][CR_LD];
  __shared__ double tw[MAXD][6];
  stage_robot(&R, Rg);
  const PlanParams& P = *pp;
  const int N = P.N;
  const int nst = ex.cr_last - ex.cr_first + 1;
  const int b = blockIdx.x / nst, i = ex.cr_first + blockIdx.x % nst;
  if (active && !active[b]) return;
  double q[D];
  const double* x = traj + ((size_t)b * (N + 1) + i) * 2 * D;
#pragma unroll
  for (int k = 0; k < D; k++) q[k] = x[k];
  double Rm[9], t[3];
  carried_link<KIND, AD, AD2>(R, q, ex.cr_link, Rm, t, tw);
  __syncthreads();
  RecAcc acc(D, P.NG);
  const CarriedSpheres<SDIM> sph{sdf, ex.cr_radius, ex.cr_centers, Rm, t, tw, ex.cr_eps, ex.cr_w, D};
  if (accumulate_sphere_rows(rows, D, ex.cr_A, sph, acc)) acc.store(pb, b, i, bufsel, P);
}

template <int KIND, int AD, int AD2, int SDIM>
__global__ __launch_bounds__(256) void k_carried_clearance(const RobotDev* __restrict__ Rg, SdfDev sdf, int link, int A,
                                                           const double* __restrict__ radius,
                                                           const double* __restrict__ centers, double dt, int inter,
                                                           int N, int Md, int nblk, const double* __restrict__ traj,
                                                           ScoreRec* __restrict__ recs) {
  using Kn = Kin<KIND, AD, AD2>;
  constexpr int D = Kn::DOF;
  __shared__ RobotDev R;
  __shared__ double srad[GPMP2MI_MAX_CARRIED_SPHERES], sctr[GPMP2MI_MAX_CARRIED_SPHERES * 3];
  for (int a = threadIdx.x; a < A; a += blockDim.x) srad[a] = radius[a];
  for (int a = threadIdx.x; a < 3 * A; a += blockDim.x) sctr[a] = centers[a];
  stage_robot(&R, Rg);   // closes with a barrier
  const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6, nsub = blockDim.x >> 6;
  const int m = blk * SCORE_TILE + lane;   // checked state of this lane
  double dense = 0.0;
  int oor = 0;
  ScoreKey best{HUGE_VAL, INT_MAX, INT_MAX};
  bool support = false;
  if (m < Md && A > 0) {
    const int seg = m / (inter + 1), j = m % (inter + 1);
    support = j == 0;
    const double* s0 = traj + ((size_t)b * (N + 1) + seg) * 2 * D;
    double q[D];
    checked_config<Kn>(s0, dt, inter, j, q);
    double Rm[9], t[3];
    carried_link<KIND, AD, AD2>(R, q, link, Rm, t, nullptr);   // value only: the Jacobian work is dead code
    for (int a = sub; a < A; a += nsub) {
      double c[3];
      carried_center(Rm, t, sctr + a * 3, c);
      if (!carried_in_range<SDIM>(sdf, c)) {
        oor++;
        continue;
      }
      double d, gx, gy, gz;
      if (SDIM == 3) (void)sdf3_lookup(sdf, c[0], c[1], c[2], d, gx, gy, gz);
      else (void)sdf2_lookup(sdf, c[0], c[1], d, gx, gy);
      const double r = srad[a];
      dense += d > r ? 0.0 : r - d;
      const ScoreKey key{d - r, m, a};
      if (key_less(key, best)) best = key;
    }
  }
  block_score_record(support ? dense : 0.0, dense, oor, best, recs);
}

// Second stage: rows are taken by thread (RowPick, score_select.h).  With a.sel.select the grid is one workgroup
// and the rule reads, besides this stage's own results, the per-row scores k_score_finish and k_self_finish left.
__global__ __launch_bounds__(256) void k_carried_finish(CarriedFinish a) {
  const ScoreFinish& f = a.sel;
  RowPick mine;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < f.B; b += gridDim.x * blockDim.x) {
    const ScoreRec t = reduce_records(a.recs + (size_t)b * a.nblk, a.nblk);
    const bool none = t.k == INT_MAX;
    if (a.support) a.support[b] = t.support;
    if (a.dense) a.dense[b] = t.dense;
    if (a.min_clearance) a.min_clearance[b] = t.clearance;
    if (a.worst) {
      a.worst[2 * b] = none ? -1 : t.k;
      a.worst[2 * b + 1] = none ? -1 : t.s;
    }
    if (a.oor) a.oor[b] = t.oor;
    if (!f.select) continue;
    const double fe = f.ferr[b];
    bool ok = row_eligible(f, b, fe, a.clearance[b], a.obs_oor[b]);
    if (a.self_clearance) ok = ok && a.self_invalid[b] == 0 && a.self_clearance[b] >= a.required_self_clearance;
    ok = ok && (!f.require_in_range || t.oor == 0) && t.clearance >= a.required_carried_clearance;
    if (ok) mine.take(fe, b);
  }
  if (!f.select) return;
  select_finish(f, mine);
}

#define G2_CARRIED_DISPATCH(h, s, KERNEL, GRID, BLOCK, ...)                                                      \
  do {                                                                                                           \
    if ((s).dim == 3) {                                                                                          \
      G2_DISPATCH_ROBOT_H(h, (KERNEL<KIND_, AD_, AD2_, 3><<<GRID, BLOCK, 0, st>>>(__VA_ARGS__)));                \
    } else {                                                                                                     \
      G2_DISPATCH_ROBOT_H(h, (KERNEL<KIND_, AD_, AD2_, 2><<<GRID, BLOCK, 0, st>>>(__VA_ARGS__)));                \
    }                                                                                                            \
  } while (0)

int launch_carried_factor(const RobotDev& h, const RobotDev* R, const SdfDev& s, int link, int A, const double* radius,
                          const double* centers, double eps, int M, const double* conf, double* err, double* H,
                          hipStream_t st) {
  if (M == 0 || A == 0) return GPMP2MI_OK;
  if (link < 0 || link >= h.nr_links || A > GPMP2MI_MAX_CARRIED_SPHERES) {
    set_error("k_carried_factor: a link out of range or a set above GPMP2MI_MAX_CARRIED_SPHERES");
    return GPMP2MI_ERR_INVALID;
  }
  const dim3 grid((unsigned)M), block(64);
  G2_CARRIED_DISPATCH(h, s, k_carried_factor, grid, block, R, s, link, A, radius, centers, eps, M, conf, err, H);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_carried_accumulate(const RobotDev& h, const RobotDev* R, const SdfDev& s, const PlanParams& hp,
                              const PlanBuffers& pb, const PlanExtras& ex, const double* traj, int bufsel,
                              const int* active, hipStream_t st) {
  if (ex.cr_A <= 0) return GPMP2MI_OK;   // an empty set launches nothing
  if (ex.cr_A > ex.cr_cap || hp.D != h.dof || hp.D > MAXD || hp.NG + hp.D + 1 > 64 * REC_SLOTS || ex.cr_link < 0 ||
      ex.cr_link >= h.nr_links || ex.cr_first < 0 || ex.cr_last > hp.N || ex.cr_first > ex.cr_last) {
    set_error("k_carried_accumulate: set larger than the capacity, a link or a state range out of range, or a record "
              "wider than 192 entries");
    return GPMP2MI_ERR_INVALID;
  }
  const int nst = ex.cr_last - ex.cr_first + 1;
  const dim3 grid((unsigned)(hp.B * nst)), block(64);
  G2_CARRIED_DISPATCH(h, s, k_carried_accumulate, grid, block, R, s, pb.params, pb, ex, traj, bufsel, active);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_carried_clearance(const RobotDev& h, const RobotDev* R, const SdfDev& s, int link, int A, const double* radius,
                             const double* centers, double dt, int inter, int B, int N, const double* traj,
                             ScoreRec* recs, hipStream_t st) {
  if (link < 0 || link >= h.nr_links || A < 0 || A > GPMP2MI_MAX_CARRIED_SPHERES) {
    set_error("k_carried_clearance: a link out of range or a set above GPMP2MI_MAX_CARRIED_SPHERES");
    return GPMP2MI_ERR_INVALID;
  }
  int Md, nblk;
  if (const int rc = checked_grid(N, inter, SCORE_TILE, B, A, Md, nblk)) return rc;
  const dim3 grid((unsigned)(nblk * B)), block(64 * score_waves(A));
  G2_CARRIED_DISPATCH(h, s, k_carried_clearance, grid, block, R, s, link, A, radius, centers, dt, inter, N, Md, nblk, traj,
                      recs);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_carried_finish(const CarriedFinish& a, hipStream_t st) {
  return launch_finish(k_carried_finish, a, a.sel.select, a.sel.B, st);
}

}  // namespace g2
