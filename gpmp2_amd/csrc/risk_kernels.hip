// risk_kernels.hip -- the posterior on the executed timeline (include/gpmp2mi.h "posterior on the executed timeline"):
// the covariance of every checked state from the band of Sigma = H^-1 at the support states, and the k-sigma clearance
// of the executed trajectory behind gpmp2mi_risk_traj / gpmp2mi_plan_risk.
//
//   k_gp_interp_cov  one workgroup per (row, interval): a lane owns a coordinate pair (ka <= kb), loads the 16 support
//                    values of its 2 x 2 [x|v] blocks once and forms that block of all J sub-steps, writing both mirrored
//                    entries; the support states are copied bit for bit.  The per-sub-step scalars (Lambda_2, Psi_2, the
//                    three Q_c entries) are put into an LDS table by the first lanes of the workgroup, once per workgroup.
//   k_risk           the tiling of k_score (score_kernels.hip): one lane per checked state, `nsub` wavefronts share the
//                    spheres -- and the entries of the packed triangle of Sigma_xx(m), which each lane forms straight
//                    from the band into LDS.  A lane forms its configuration as k_score does, walks the chain with
//                    the Jacobian visitor, and per in-range sphere computes
//                    h = grad d . d centre / d x, sigma^2 = h Sigma_xx h^T and the key (clearance - kappa sigma, m, s).
//                    Wavefront butterfly -> LDS -> ONE record per workgroup.
//   k_risk_finish    reduces the records of every row in index order and applies the `ok` rule.
//
// What goes through LDS is the result, not the input: the D (D + 1) / 2 <= 28 doubles of Sigma_xx per state (14 KB per
// tile at D = 7), not the support blocks a tile touches.  Those are ceil(64 / (J + 1)) + 1 intervals of 3 n^2 doubles --
// more than the 160 KB of a CU for J < 5 at n = 14 -- and the lanes of one interval read the same addresses, which the
// cache serves as a broadcast.  Held in registers the triangle spilled from D = 6 on (profiles/risk_resources.txt);
// in LDS the wavefronts also stop forming it four times over.
//
// Determinism: as k_score -- the tile and nsub depend on (N, inter_step, S) only, every sum is taken in a fixed order and
// no floating-point atomic is used.
#include <climits>

#include "device_math.h"
#include "dispatch.h"
#include "launch.h"

namespace g2 {

// Lambda_2 / Psi_2 of gp_coef_dev and the conditional covariance of the prior bridge at tau, in the factored closed
// form (the subtractive form Q(tau) - Psi Q(dt) Psi^T loses two digits)
struct RiskCoef {
  GpCoef g;
  double q00, q01, q11, pad;
};
__device__ __forceinline__ RiskCoef risk_coef_dev(double dt, double tau) {
  RiskCoef c;
  c.g = gp_coef_dev(dt, tau);
  const double r = dt - tau, d3 = dt * dt * dt, tr = tau * r;
  c.q00 = tr * tr * tr / (3.0 * d3);
  c.q01 = tr * tr * (dt - 2.0 * tau) / (2.0 * d3);
  c.q11 = tr * (dt * dt - 3.0 * tau * dt + 3.0 * tau * tau) / d3;
  c.pad = 0.0;
  return c;
}

constexpr int COV_TAB = 64;   // sub-steps per pass of k_gp_interp_cov's LDS table

__global__ __launch_bounds__(256) void k_gp_interp_cov(int D, const double* __restrict__ Qc, double dt, int inter, int N,
                                                       const double* __restrict__ Sd, const double* __restrict__ So,
                                                       double* __restrict__ cov) {
  __shared__ RiskCoef tab[COV_TAB];
  const int n = 2 * D, nn = n * n;
  const int b = blockIdx.x / N, i = blockIdx.x % N;
  const size_t Md = (size_t)N * (inter + 1) + 1;
  const double* A = Sd + ((size_t)b * (N + 1) + i) * nn;   // Sigma_ii
  const double* E = A + nn;                                // Sigma_{i+1,i+1}
  const double* C = So + ((size_t)b * N + i) * nn;         // Sigma_{i+1,i}
  double* out = cov + ((size_t)b * Md + (size_t)i * (inter + 1)) * nn;
  // support states: copies (n^2 is a multiple of 4, so every block keeps the alignment of its array)
  {
    const int last = i == N - 1;   // the last interval also owns state Md - 1
    double* o1 = cov + ((size_t)b * Md + (Md - 1)) * nn;
    if ((((uintptr_t)Sd | (uintptr_t)cov) & 15) == 0) {
      const double2 *a2 = (const double2*)A, *e2 = (const double2*)E;
      double2 *o2 = (double2*)out, *l2 = (double2*)o1;
      for (int e = threadIdx.x; e < nn / 2; e += blockDim.x) {
        o2[e] = a2[e];
        if (last) l2[e] = e2[e];
      }
    } else {
      for (int e = threadIdx.x; e < nn; e += blockDim.x) {
        out[e] = A[e];
        if (last) o1[e] = E[e];
      }
    }
  }
  if (inter == 0) return;
  // this lane's pair: p = ka + kb (kb + 1) / 2, ka <= kb
  const int npair = D * (D + 1) / 2;
  const int p = threadIdx.x;
  int ka = 0, kb = 0;
  double a[2][2], e[2][2], c1[2][2], c2[2][2], qc = 0.0;
  if (p < npair) {
    while ((kb + 1) * (kb + 2) / 2 <= p) kb++;
    ka = p - kb * (kb + 1) / 2;
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
      for (int c = 0; c < 2; c++) {
        a[r][c] = A[(r * D + ka) * n + c * D + kb];
        e[r][c] = E[(r * D + ka) * n + c * D + kb];
        c1[r][c] = C[(r * D + ka) * n + c * D + kb];
        c2[r][c] = C[(r * D + kb) * n + c * D + ka];
      }
    qc = Qc ? Qc[ka * D + kb] : (ka == kb ? 1.0 : 0.0);
  }
  for (int j0 = 1; j0 <= inter; j0 += COV_TAB) {
    const int cnt = min(COV_TAB, inter - j0 + 1);
    __syncthreads();
    if ((int)threadIdx.x < cnt) tab[threadIdx.x] = risk_coef_dev(dt, (double)(j0 + threadIdx.x) * (dt / (double)(inter + 1)));
    __syncthreads();
    if (p >= npair) continue;
    for (int t = 0; t < cnt; t++) {
      const RiskCoef k = tab[t];
      const double L[2][2] = {{k.g.l11, k.g.l12}, {k.g.l21, k.g.l22}}, P[2][2] = {{k.g.p11, k.g.p12}, {k.g.p21, k.g.p22}};
      const double Q[2][2] = {{k.q00, k.q01}, {k.q01, k.q11}};
      double o[2][2];
#pragma unroll
      for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
          // row (r, ka), column (c, kb) of  L A L^T + P E P^T + P C L^T + (P C L^T)^T + Q (x) Qc, in this order
          double s = 0.0;
#pragma unroll
          for (int u = 0; u < 2; u++)
#pragma unroll
            for (int w = 0; w < 2; w++) s += L[r][u] * a[u][w] * L[c][w];
#pragma unroll
          for (int u = 0; u < 2; u++)
#pragma unroll
            for (int w = 0; w < 2; w++) s += P[r][u] * e[u][w] * P[c][w];
          double x = 0.0;
#pragma unroll
          for (int u = 0; u < 2; u++)
#pragma unroll
            for (int w = 0; w < 2; w++) x += P[r][u] * c1[u][w] * L[c][w] + P[c][u] * c2[u][w] * L[r][w];
          o[r][c] = (s + x) + Q[r][c] * qc;
        }
      double* om = out + (size_t)(j0 + t) * nn;
      if (ka == kb) o[1][0] = o[0][1];   // the diagonal pair's block is its own mirror: one value for both
#pragma unroll
      for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
          om[(r * D + ka) * n + c * D + kb] = o[r][c];
          if (ka != kb) om[(c * D + kb) * n + r * D + ka] = o[r][c];
        }
    }
  }
}

// (robust clearance, state, sphere) compared as ScoreKey of k_score; sigma travels with it
struct RiskKey {
  double c, sg;
  int k, s;
};
__device__ __forceinline__ bool risk_less(const RiskKey& a, const RiskKey& b) {
  return a.c < b.c || (a.c == b.c && (a.k < b.k || (a.k == b.k && a.s < b.s)));
}

template <int KIND, int AD, int AD2, int SDIM>
__global__ __launch_bounds__(256) void k_risk(const RobotDev* __restrict__ Rg, SdfDev sdf, const double* __restrict__ Qc,
                                              double dt, int inter, int N, int Md, int nblk, double kappa,
                                              const double* __restrict__ traj, const double* __restrict__ Sd,
                                              const double* __restrict__ So, const int* __restrict__ ok,
                                              double* __restrict__ sigma, RiskRec* __restrict__ recs) {
  using K = Kin<KIND, AD, AD2>;
  static_assert(!K::MOBILE, "k_risk: vector-space kinds only");
  constexpr int D = K::DOF, n = 2 * D, nn = n * n, NT = D * (D + 1) / 2;
  __shared__ RobotDev R;
  __shared__ double sxx[NT][SCORE_TILE];   // packed triangle of Sigma_xx of the tile's states: (ka, kb) at ka + kb (kb + 1) / 2
  __shared__ double w_c[4], w_sg[4];
  __shared__ int w_k[4], w_s[4], w_oor[4];
  stage_robot(&R, Rg);
  const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6, nsub = blockDim.x >> 6;
  const int m = blk * SCORE_TILE + lane;   // checked state of this lane
  const int S = R.nr_spheres;
  const bool bad = ok && ok[b] == 0;       // a row that is not SPD: its band is unspecified
  const int seg = m / (inter + 1), j = m % (inter + 1);
  RiskCoef rc{};
  if (m < Md) {
    // Sigma_xx(m): the wavefronts of the workgroup share the entries of the triangle (t % nsub), each entry is formed by
    // one lane from the band.  Over z = [x_i, v_i, x_{i+1}, v_{i+1}] it is sum_uw c_u c_w M_uw + Q_c[0][0] Qc with
    // c = (l11, l12, p11, p12) and M the 4 x 4 arrangement of the (ka, kb) entries of Sigma_ii, Sigma_{i+1,i+1}, Sigma_{i+1,i}
    const double* A = Sd + ((size_t)b * (N + 1) + seg) * nn;
    if (j > 0) rc = risk_coef_dev(dt, (double)j * (dt / (double)(inter + 1)));
    const double c[4] = {rc.g.l11, rc.g.l12, rc.g.p11, rc.g.p12};
    int ka = 0, kb = 0;
    for (int t = 0; t < NT; t++) {
      if (t % nsub == sub) {
        if (j == 0) {
          sxx[t][lane] = A[ka * n + kb];
        } else {
          const double* E = A + nn;
          const double* C = So + ((size_t)b * N + seg) * nn;
          double sa = 0.0, se = 0.0, sc = 0.0;
#pragma unroll
          for (int u = 0; u < 2; u++)
#pragma unroll
            for (int w = 0; w < 2; w++) {
              sa += c[u] * c[w] * A[(u * D + ka) * n + w * D + kb];
              se += c[2 + u] * c[2 + w] * E[(u * D + ka) * n + w * D + kb];
              sc += c[2 + u] * c[w] * (C[(u * D + ka) * n + w * D + kb] + C[(u * D + kb) * n + w * D + ka]);
            }
          const double qc = Qc ? Qc[ka * D + kb] : (ka == kb ? 1.0 : 0.0);
          sxx[t][lane] = ((sa + se) + sc) + rc.q00 * qc;
        }
      }
      if (++ka > kb) { ka = 0; kb++; }
    }
  }
  __syncthreads();
  int oor = 0;
  RiskKey best{HUGE_VAL, 0.0, INT_MAX, INT_MAX};
  if (m < Md) {
    const double* s0 = traj + ((size_t)b * (N + 1) + seg) * 2 * D;
    double q[D];
    if (j == 0) {
#pragma unroll
      for (int k = 0; k < D; k++) q[k] = s0[k];
    } else {
      const double* s1 = s0 + 2 * D;
      const GpCoef& gc = rc.g;
#pragma unroll
      for (int k = 0; k < D; k++) q[k] = gc.l11 * s0[k] + gc.l12 * s0[D + k] + gc.p11 * s1[k] + gc.p12 * s1[D + k];
    }
    double* smap = sigma ? sigma + ((size_t)b * Md + m) * S : nullptr;
    K::visit_spheres(
        R, q,
        [&](int s, const double (&p)[3]) {
          // negated conjunction: a NaN centre fails every comparison and counts as out of range
          bool in = p[0] >= sdf.ox && p[0] <= sdf.hix && p[1] >= sdf.oy && p[1] <= sdf.hiy;
          if (SDIM == 3) in = in && p[2] >= sdf.oz && p[2] <= sdf.hiz;
          if (!in) {
            oor++;
            if (smap) smap[R.sph_orig[s]] = NAN;
          }
          return in;
        },
        [&](int s, const double (&p)[3], const double (&Jc)[D][3], auto) {
          double d, gx, gy, gz = 0.0;
          if (SDIM == 3) (void)sdf3_lookup(sdf, p[0], p[1], p[2], d, gx, gy, gz);
          else (void)sdf2_lookup(sdf, p[0], p[1], d, gx, gy);
          double h[D];
#pragma unroll
          for (int k = 0; k < D; k++) {
            h[k] = gx * Jc[k][0] + gy * Jc[k][1];
            if (SDIM == 3) h[k] += gz * Jc[k][2];
          }
          // h Sigma_xx h^T over the triangle, columns in order: the diagonal term plus twice the part above it
          double s2 = 0.0;
#pragma unroll
          for (int kb = 0; kb < D; kb++) {
            double t = 0.0;
#pragma unroll
            for (int ka = 0; ka < kb; ka++) t += sxx[ka + kb * (kb + 1) / 2][lane] * h[ka];
            s2 += h[kb] * (sxx[kb + kb * (kb + 1) / 2][lane] * h[kb] + 2.0 * t);
          }
          const double sg = sqrt(fmax(s2, 0.0));
          if (smap) smap[R.sph_orig[s]] = bad ? NAN : sg;
          const RiskKey key{(d - R.sph_r[s]) - kappa * sg, sg, m, R.sph_orig[s]};
          if (risk_less(key, best)) best = key;
        },
        sub, nsub);
  }
  // wavefront butterfly: the partners compare the same two keys, so all 64 lanes end with the same one
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    oor += __shfl_xor(oor, off);
    const RiskKey o{__shfl_xor(best.c, off), __shfl_xor(best.sg, off), __shfl_xor(best.k, off), __shfl_xor(best.s, off)};
    if (risk_less(o, best)) best = o;
  }
  if (lane == 0) {
    w_c[sub] = best.c; w_sg[sub] = best.sg; w_k[sub] = best.k; w_s[sub] = best.s; w_oor[sub] = oor;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    RiskRec r{w_c[0], w_sg[0], w_k[0], w_s[0], w_oor[0], 0};
    for (int w = 1; w < nsub; w++) {   // wavefronts in index order
      r.oor += w_oor[w];
      const RiskKey x{w_c[w], w_sg[w], w_k[w], w_s[w]}, c{r.c, r.sigma, r.k, r.s};
      if (risk_less(x, c)) { r.c = x.c; r.sigma = x.sg; r.k = x.k; r.s = x.s; }
    }
    recs[blockIdx.x] = r;
  }
}

// One thread per row: its records in index order, then the rule for rows that are not SPD
__global__ __launch_bounds__(256) void k_risk_finish(RiskFinish a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  const RiskRec* r = a.recs + (size_t)b * a.nblk;
  RiskRec t = r[0];
  for (int i = 1; i < a.nblk; i++) {
    t.oor += r[i].oor;
    const RiskKey x{r[i].c, r[i].sigma, r[i].k, r[i].s}, c{t.c, t.sigma, t.k, t.s};
    if (risk_less(x, c)) { t.c = x.c; t.sigma = x.sg; t.k = x.k; t.s = x.s; }
  }
  const bool bad = a.ok && a.ok[b] == 0;
  const bool none = bad || t.k == INT_MAX;
  if (a.robust) a.robust[b] = bad ? NAN : t.c;
  if (a.sigma_worst) a.sigma_worst[b] = bad ? NAN : (none ? 0.0 : t.sigma);
  if (a.worst) {
    a.worst[2 * b] = none ? -1 : t.k;
    a.worst[2 * b + 1] = none ? -1 : t.s;
  }
  if (a.oor) a.oor[b] = t.oor;
}

int launch_gp_interp_cov(int D, const double* Qc, double dt, int inter, int B, int N, const double* Sd, const double* So,
                         double* cov, hipStream_t st) {
  if ((long long)B * N >= (1ll << 31)) {
    set_error("too many intervals for one launch");
    return GPMP2MI_ERR_INVALID;
  }
  const int npair = D * (D + 1) / 2;   // a lane per pair: one wavefront up to dof 10, three at dof 18
  k_gp_interp_cov<<<dim3((unsigned)(B * N)), dim3((npair + 63) / 64 * 64), 0, st>>>(D, Qc, dt, inter, N, Sd, So, cov);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

// the vector-space kinds of dispatch.h with blocks of one tile (the posterior's limit): the arm up to 7 joints, the point
#define G2_RISK_CASE(K, A, SD)                                                                                        \
  if (!done && h.kind == (K) && h.arm_dof == (A) && s.dim == (SD)) {                                                  \
    k_risk<K, A, 0, SD><<<grid, block, 0, st>>>(R, s, Qc, dt, inter, N, (int)Md, (int)nblk, kappa, traj, Sd, So, ok, \
                                                sigma, recs);                                                         \
    done = true;                                                                                                      \
  }

int launch_risk(const RobotDev& h, const RobotDev* R, const SdfDev& s, const double* Qc, double dt, int inter, int B,
                int N, double kappa, const double* traj, const double* Sd, const double* So, const int* ok, double* sigma,
                RiskRec* recs, hipStream_t st) {
  const long long Md = (long long)N * (inter + 1) + 1;
  const long long nblk = (Md + SCORE_TILE - 1) / SCORE_TILE;
  if (Md >= (1ll << 31) / GPMP2MI_MAX_DOF || nblk * B >= (1ll << 31)) {
    set_error("too many checked states for one launch");
    return GPMP2MI_ERR_INVALID;
  }
  const int nsub = h.nr_spheres >= 8 ? 4 : 1;   // as k_score
  const dim3 grid((unsigned)(nblk * B)), block(64 * nsub);
  bool done = false;
  G2_RISK_CASE(GPMP2MI_ROBOT_ARM, 1, 2) G2_RISK_CASE(GPMP2MI_ROBOT_ARM, 1, 3)
  G2_RISK_CASE(GPMP2MI_ROBOT_ARM, 2, 2) G2_RISK_CASE(GPMP2MI_ROBOT_ARM, 2, 3)
  G2_RISK_CASE(GPMP2MI_ROBOT_ARM, 3, 2) G2_RISK_CASE(GPMP2MI_ROBOT_ARM, 3, 3)
  G2_RISK_CASE(GPMP2MI_ROBOT_ARM, 4, 2) G2_RISK_CASE(GPMP2MI_ROBOT_ARM, 4, 3)
  G2_RISK_CASE(GPMP2MI_ROBOT_ARM, 5, 2) G2_RISK_CASE(GPMP2MI_ROBOT_ARM, 5, 3)
  G2_RISK_CASE(GPMP2MI_ROBOT_ARM, 6, 2) G2_RISK_CASE(GPMP2MI_ROBOT_ARM, 6, 3)
  G2_RISK_CASE(GPMP2MI_ROBOT_ARM, 7, 2) G2_RISK_CASE(GPMP2MI_ROBOT_ARM, 7, 3)
  G2_RISK_CASE(GPMP2MI_ROBOT_POINT, 0, 2) G2_RISK_CASE(GPMP2MI_ROBOT_POINT, 0, 3)
  if (!done) {
    set_error("risk: robot kind / dof combination is not instantiated");
    return GPMP2MI_ERR_UNSUPPORTED;
  }
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_risk_finish(const RiskFinish& a, hipStream_t st) {
  k_risk_finish<<<dim3((a.B + 255) / 256), dim3(256), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

}  // namespace g2
