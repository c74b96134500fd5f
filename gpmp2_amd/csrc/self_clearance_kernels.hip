// self_clearance_kernels.hip -- the self-collision check of the executed trajectory behind gpmp2mi_self_score_traj /
// gpmp2mi_plan_self_score / gpmp2mi_plan_select_checked (include/gpmp2mi.h "self-collision check"): does the robot
// touch itself at any of the states that are executed, for any pair of a table far larger than the in-plan factor holds?
//
//   k_self_clearance  a lane is a checked state, a workgroup covers self_tile(S) consecutive states of one trajectory
//                     (checked_grid, score_select.h).  Phase 1: GP up-sampling (checked_config) -> value-only walk
//                     of the kinematic chain; the sphere centres go to LDS, lane-minor ([coord][sphere][state]), the
//                     spheres dealt to the wavefronts (and, in a tile narrower than a wavefront, to the 64 / tile lanes
//                     that share a state).  Barrier.  Phase 2: the pairs dealt the same way; per (state, pair) six
//                     doubles from LDS -> distance, hinge, key (clearance, state, pair).  ONE record per workgroup
//                     (block_score_record).
//   k_self_finish     reduces the records of every row in index order to the five per-row outputs; when asked, reduces
//                     the records of k_score for the same rows as well, applies the selection rule with both
//                     clearances and copies the chosen row and its up-sampled form.
//
// Determinism: the tile and nsub depend on S only, every sum is taken in an order fixed by (N, inter_step, S, P) and the
// table's order (a lane's pairs ascending, lane butterfly, wavefronts in index order, records in index order), and no
// floating-point atomic is used, so a row's results do not depend on the batch, its position in it or the entry point.
#include <climits>

#include "device_math.h"
#include "dispatch.h"
#include "launch.h"
#include "score_select.h"

namespace g2 {

template <int KIND, int AD, int AD2>
__global__ __launch_bounds__(256) void k_self_clearance(const RobotDev* __restrict__ Rg,
                                                        const SelfPair* __restrict__ pairs, int P, int tile, double dt,
                                                        int inter, int N, int Md, int nblk,
                                                        const double* __restrict__ traj, ScoreRec* __restrict__ recs) {
  using K = Kin<KIND, AD, AD2>;
  constexpr int D = K::DOF;
  extern __shared__ __attribute__((aligned(16))) double ctr[];   // [3][S][tile]
  __shared__ RobotDev R;
  stage_robot(&R, Rg);
  const int S = R.nr_spheres;
  const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6, nsub = blockDim.x >> 6;
  // a tile narrower than the wavefront: `slots` lanes share a state and split its spheres, then its pairs
  const int slots = 64 / tile, slot = lane / tile, tl = lane % tile;
  const int m = blk * tile + tl;   // checked state of this lane
  const bool live = m < Md;
  if (live && P > 0) {
    const int seg = m / (inter + 1), j = m % (inter + 1);
    const double* s0 = traj + ((size_t)b * (N + 1) + seg) * 2 * D;
    double q[D];
    checked_config<K>(s0, dt, inter, j, q);
    typename K::Axes A;   // filled by the walk, never read here: the Jacobian work is dead code
    K::walk(R, q, A, [&](int s, const double (&p)[3], auto) {
#pragma unroll
      for (int i = 0; i < 3; i++) ctr[(i * S + s) * tile + tl] = p[i];
    }, sub * slots + slot, nsub * slots);
  }
  __syncthreads();
  double dense = 0.0;
  int inv = 0;
  ScoreKey best{HUGE_VAL, INT_MAX, INT_MAX};
  auto pair = [&](int p) {
    const SelfPair pr = pairs[p];
    const double dx = ctr[pr.a * tile + tl] - ctr[pr.b * tile + tl];
    const double dy = ctr[(S + pr.a) * tile + tl] - ctr[(S + pr.b) * tile + tl];
    const double dz = ctr[(2 * S + pr.a) * tile + tl] - ctr[(2 * S + pr.b) * tile + tl];
    const double dist = sqrt(dx * dx + dy * dy + dz * dz);
    if (!isfinite(dist)) {   // invalid: counted, adds nothing
      inv++;
      return;
    }
    dense += dist > pr.total_eps ? 0.0 : pr.total_eps - dist;
    const ScoreKey key{dist - pr.total_eps, m, p};
    if (key_less(key, best)) best = key;
  };
  if (live) {
    if (slots == 1) {
      // the pair index is the same in every lane: the record comes through a scalar load
      const int first = __builtin_amdgcn_readfirstlane(sub), step = __builtin_amdgcn_readfirstlane(nsub);
      for (int p = first; p < P; p += step) pair(p);
    } else {
      for (int p = sub * slots + slot; p < P; p += nsub * slots) pair(p);
    }
  }
  block_score_record((live && m % (inter + 1) == 0) ? dense : 0.0, dense, inv, best, recs);
}

// Second stage: rows are taken by thread, a row's records are summed in index order (RowPick, reduce_records).
// With a.sel.select the grid is one workgroup and the rule reads both clearances of a row: the obstacle records of
// k_score (a.sel.recs) are reduced here too, by the same function k_score_finish uses.
__global__ __launch_bounds__(256) void k_self_finish(SelfFinish a) {
  const ScoreFinish& f = a.sel;
  RowPick mine;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < f.B; b += gridDim.x * blockDim.x) {
    const ScoreRec t = reduce_records(a.recs + (size_t)b * a.nblk, a.nblk);
    const bool none = t.k == INT_MAX;
    if (a.support) a.support[b] = t.support;
    if (a.dense) a.dense[b] = t.dense;
    if (a.clearance) a.clearance[b] = t.clearance;
    if (a.worst) {
      a.worst[2 * b] = none ? -1 : t.k;
      a.worst[2 * b + 1] = none ? -1 : t.s;
    }
    if (a.invalid) a.invalid[b] = t.oor;
    if (!f.select) continue;
    const ScoreRec o = reduce_records(f.recs + (size_t)b * f.nblk, f.nblk);
    const double fe = f.ferr[b];
    const bool ok = row_eligible(f, b, fe, o.clearance, o.oor) && t.oor == 0 && t.clearance >= a.required_self_clearance;
    if (ok) mine.take(fe, b);
  }
  if (!f.select) return;
  select_finish(f, mine);
}

int launch_self_clearance(const RobotDev& h, const RobotDev* R, const SelfPair* pairs, int P, double dt, int inter, int B,
                          int N, const double* traj, ScoreRec* recs, hipStream_t st) {
  const int S = h.nr_spheres, tile = self_tile(S);
  int Md, nblk;
  if (const int rc = checked_grid(N, inter, tile, B, P, Md, nblk)) return rc;
  const size_t lds = (size_t)3 * std::max(S, 1) * tile * sizeof(double);   // <= 48 KB by self_tile
  const dim3 grid((unsigned)(nblk * B)), block(64 * score_waves(S));
  G2_DISPATCH_ROBOT_H(h, (k_self_clearance<KIND_, AD_, AD2_><<<grid, block, lds, st>>>(R, pairs, P, tile, dt, inter, N,
                                                                                      Md, nblk, traj, recs)));
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_self_finish(const SelfFinish& a, hipStream_t st) {
  return launch_finish(k_self_finish, a, a.sel.select, a.sel.B, st);
}

}  // namespace g2
