// group_kernels.hip -- "distinct alternatives" (include/gpmp2mi.h): the all-pairs trajectory distance (k_traj_pairs), the
// leader rule in rounds (k_group_rule, one workgroup) and the copy of the leaders' rows (k_group_copy).
#include <algorithm>

#include "group_rule.h"
#include "score_select.h"

namespace g2 {

namespace {
constexpr int PAIR_LD = GROUP_CHUNK_ELEMS + 1;   // staged row stride in doubles: odd, so the 16 rows a wavefront reads
                                                 // with one ds_read_b64 fall on 16 different bank pairs
constexpr int RES_LD = GROUP_TILE + 1;           // stride of the result tile, read by rows and by columns
static_assert(2 * GROUP_TILE * PAIR_LD >= GROUP_TILE * RES_LD, "the result tile reuses the staging");
}  // namespace

// One workgroup of 256 threads per 64 x 64 tile of pairs, upper triangle of tiles only: tile (ti, tj), ti <= tj, holds
// rows r0 .. r0 + 63 against rows c0 .. c0 + 63 and stores its result twice, as [r][c] and mirrored as [c][r], so the
// matrix is symmetric by construction.  Thread (ty, tx) keeps the 4 x 4 pairs (ty + 16 i, tx + 16 j): every value read
// from LDS is used four times.  The configuration halves of both row tiles go through LDS in chunks of whole states
// (group_chunk_states); s_i is closed at every state boundary, then folded into the running max / sum.  The arithmetic
// of a pair is written with explicit roundings: it is the same in every tile, batch and entry point.
template <bool RMS>
__global__ __launch_bounds__(256) void k_traj_pairs(PairArgs a) {
  __shared__ double s_buf[2 * GROUP_TILE * PAIR_LD];
  __shared__ double s_w[GPMP2MI_MAX_DOF];
  __shared__ int s_off[GROUP_CHUNK_ELEMS];
  const int T = (a.B + GROUP_TILE - 1) / GROUP_TILE;
  int k = blockIdx.x, ti = 0;
  while (k >= T - ti) {   // row ti of the triangle has T - ti tiles
    k -= T - ti;
    ti++;
  }
  const int tj = ti + k;
  const int r0 = ti * GROUP_TILE, c0 = tj * GROUP_TILE;
  const int D = a.D, n = 2 * D, S = a.N + 1, CH = group_chunk_states(D);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  if (tid < D) s_w[tid] = a.w[tid];
  if (tid < CH * D) s_off[tid] = (tid / D) * n + tid % D;   // element e of a chunk: state e / D, coordinate e % D

  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = 0.0;

  for (int s0 = 0; s0 < S; s0 += CH) {
    const int nst = min(CH, S - s0), ne = nst * D;
    __syncthreads();   // the previous chunk has been read (first pass: s_w / s_off are written)
    for (int idx = tid; idx < 2 * GROUP_TILE * GROUP_CHUNK_ELEMS; idx += 256) {
      const int which = idx / (GROUP_TILE * GROUP_CHUNK_ELEMS), row = (idx / GROUP_CHUNK_ELEMS) % GROUP_TILE;
      const int e = idx % GROUP_CHUNK_ELEMS;
      if (e >= ne) continue;
      const int g = (which ? c0 : r0) + row;
      s_buf[(which * GROUP_TILE + row) * PAIR_LD + e] = g < a.B ? a.traj[((size_t)g * S + s0) * n + s_off[e]] : 0.0;
    }
    __syncthreads();
    const double* A = s_buf + ty * PAIR_LD;
    const double* Bt = s_buf + (GROUP_TILE + tx) * PAIR_LD;
    for (int st = 0; st < nst; st++) {
      double s[4][4];
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) s[i][j] = 0.0;
      for (int d = 0; d < D; d++) {
        const int e = st * D + d;
        const double w = s_w[d];
        double xa[4], xb[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          xa[i] = A[16 * i * PAIR_LD + e];
          xb[i] = Bt[16 * i * PAIR_LD + e];
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const double df = __dsub_rn(xa[i], xb[j]);
            s[i][j] = __fma_rn(w, __dmul_rn(df, df), s[i][j]);   // w * df^2, added in ascending d
          }
      }
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if (RMS) acc[i][j] = __dadd_rn(acc[i][j], s[i][j]);
          else acc[i][j] = (s[i][j] > acc[i][j] || s[i][j] != s[i][j]) ? s[i][j] : acc[i][j];   // a NaN stays
        }
    }
  }
  __syncthreads();   // the staging is free: it becomes the 64 x 64 result tile
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const double v = RMS ? __ddiv_rn(acc[i][j], (double)S) : acc[i][j];
      s_buf[(ty + 16 * i) * RES_LD + tx + 16 * j] = __dsqrt_rn(v);
    }
  __syncthreads();
  // wavefront wv stores 16 rows of the tile, lane = column: coalesced rows, and one ballot per 64-bit word of the bits
  const int wv = tid >> 6, lane = tid & 63, W = group_words(a.B);
  for (int q = 0; q < 16; q++) {
    const int r = wv * 16 + q, gr = r0 + r, gc = c0 + lane;
    const bool live = gr < a.B && gc < a.B;
    const double v = s_buf[r * RES_LD + lane];
    if (a.dist && live) a.dist[(size_t)gr * a.B + gc] = v;
    if (a.bits) {
      const unsigned long long word = __ballot(live && group_within(v, a.radius));
      if (lane == 0 && gr < a.B) a.bits[(size_t)gr * W + tj] = word;
    }
  }
  if (ti == tj) return;
  for (int q = 0; q < 16; q++) {   // mirrored: row c0 + c of the matrix, columns r0 + lane
    const int c = wv * 16 + q, gr = c0 + c, gc = r0 + lane;
    const bool live = gr < a.B && gc < a.B;
    const double v = s_buf[lane * RES_LD + c];
    if (a.dist && live) a.dist[(size_t)gr * a.B + gc] = v;
    if (a.bits) {
      const unsigned long long word = __ballot(live && group_within(v, a.radius));
      if (lane == 0 && gr < a.B) a.bits[(size_t)gr * W + ti] = word;
    }
  }
}

namespace {
constexpr int RULE_THREADS = 1024;
constexpr int RULE_ROWS = GPMP2MI_MAX_GROUP_ROWS / RULE_THREADS;   // rows a thread keeps in registers
static_assert(RULE_ROWS * RULE_THREADS == GPMP2MI_MAX_GROUP_ROWS, "rows are dealt to the threads evenly");
}  // namespace

// The leader rule in rounds (group_rule.h), one workgroup: thread t keeps rows t, t + 1024, ... in registers.  A round
// is an argmin of (score, row) over the undecided rows (wavefront butterfly, then the 16 wavefronts in index order),
// then every undecided row looks up its pair with the new leader.  Two barriers per round, n_modes rounds.
__global__ __launch_bounds__(RULE_THREADS) void k_group_rule(GroupRule a) {
  __shared__ double s_ps[RULE_THREADS / 64];
  __shared__ int s_pr[RULE_THREADS / 64];
  __shared__ int s_cnt[2], s_nel;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, W = group_words(a.B);
  if (tid == 0) s_cnt[0] = s_cnt[1] = s_nel = 0;
  __syncthreads();
  double sc[RULE_ROWS];
  int md[RULE_ROWS];
  int nel = 0;
#pragma unroll
  for (int q = 0; q < RULE_ROWS; q++) {
    const int b = tid + q * RULE_THREADS;
    sc[q] = HUGE_VAL;
    md[q] = -1;
    if (b >= a.B) continue;
    sc[q] = a.score[b];
    int el;
    if (a.plan_rule) {
      el = score_eligible(!a.status || a.status[b] != GPMP2MI_TRAJ_NOT_SPD, sc[q], a.clearance[b], a.required_clearance,
                          a.require_in_range, a.oor[b]);
      if (a.self_clearance) el = el && a.self_invalid[b] == 0 && a.self_clearance[b] >= a.required_self_clearance;
    } else {
      el = a.eligible ? a.eligible[b] : 1;
    }
    if (group_takes_part(sc[q], el)) {
      md[q] = GROUP_UNDECIDED;
      nel++;
    }
  }
  if (nel) atomicAdd(&s_nel, nel);
  int k = 0;
  for (;; k++) {
    double bs = HUGE_VAL;
    int br = INT_MAX;
#pragma unroll
    for (int q = 0; q < RULE_ROWS; q++)   // rows ascend within a thread
      if (md[q] == GROUP_UNDECIDED && group_rank_less(sc[q], tid + q * RULE_THREADS, bs, br)) {
        bs = sc[q];
        br = tid + q * RULE_THREADS;
      }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double os = __shfl_xor(bs, off);
      const int orow = __shfl_xor(br, off);
      if (group_rank_less(os, orow, bs, br)) { bs = os; br = orow; }
    }
    if (lane == 0) { s_ps[wv] = bs; s_pr[wv] = br; }
    __syncthreads();
    bs = s_ps[0];
    br = s_pr[0];
    for (int w = 1; w < RULE_THREADS / 64; w++)
      if (group_rank_less(s_ps[w], s_pr[w], bs, br)) { bs = s_ps[w]; br = s_pr[w]; }
    if (br == INT_MAX) break;   // nothing is undecided: the same in every thread
    int joined = 0;
#pragma unroll
    for (int q = 0; q < RULE_ROWS; q++) {
      const int b = tid + q * RULE_THREADS;
      // every row of the batch looks its pair up, decided or not: the update below is then a plain select.  Keep it a
      // select: the branchy form (`continue` for decided rows, `if (in) { md = k; n++; }`) is miscompiled by hipcc for
      // gfx950 -- members are counted but stay undecided ("A compiler note on k_group_rule")
      bool near = false;
      if (b < a.B) near = a.bits ? group_bit(a.bits, W, br, b) : group_within(a.dist[(size_t)br * a.B + b], a.radius);
      const bool in = md[q] == GROUP_UNDECIDED && (b == br || near);
      md[q] = in ? k : md[q];
      joined += in ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) joined += __shfl_xor(joined, off);
    if (lane == 0 && joined) atomicAdd(&s_cnt[k & 1], joined);
    __syncthreads();
    if (tid == 0) {
      if (a.leaders) a.leaders[k] = br;
      if (a.sizes) a.sizes[k] = s_cnt[k & 1];
      s_cnt[k & 1] = 0;   // round k + 2 adds to it behind two more barriers
    }
  }
  for (int j = k + tid; j < a.B; j += RULE_THREADS) {
    if (a.leaders) a.leaders[j] = -1;
    if (a.sizes) a.sizes[j] = 0;
  }
  if (a.mode)
#pragma unroll
    for (int q = 0; q < RULE_ROWS; q++) {
      const int b = tid + q * RULE_THREADS;
      if (b < a.B) a.mode[b] = md[q];
    }
  if (tid == 0) {
    if (a.n_modes) *a.n_modes = k;
    if (a.n_eligible) *a.n_eligible = s_nel;
  }
}

// Workgroup k: leader, size and final_error of mode k, the leader's row and its up-sampled form, by the expressions
// select_finish (score_select.h) copies the chosen row with.  k >= n_modes: alt = -1, alt_size = 0, the rest untouched.
__global__ __launch_bounds__(256) void k_group_copy(GroupCopy a) {
  const int k = blockIdx.x;
  if (k == 0 && threadIdx.x == 0) {
    if (a.out_n_modes) *a.out_n_modes = *a.n_modes;
    if (a.out_n_eligible) *a.out_n_eligible = *a.n_eligible;
  }
  if (k >= *a.n_modes) {
    if (threadIdx.x == 0) {
      if (a.alt) a.alt[k] = -1;
      if (a.alt_size) a.alt_size[k] = 0;
    }
    return;
  }
  const int L = a.leaders[k];
  if (threadIdx.x == 0) {
    if (a.alt) a.alt[k] = L;
    if (a.alt_size) a.alt_size[k] = a.sizes[k];
    if (a.alt_error) a.alt_error[k] = a.ferr[L];
  }
  const size_t trow = (size_t)(a.N + 1) * 2 * a.D;
  const double* row = a.traj + (size_t)L * trow;
  if (a.traj_alt)
    for (size_t i = threadIdx.x; i < trow; i += blockDim.x) a.traj_alt[(size_t)k * trow + i] = row[i];
  if (a.dense_alt) {
    double* out = a.dense_alt + (size_t)k * a.Md * 2 * a.D;
    for (int e = threadIdx.x; e < a.Md * a.D; e += blockDim.x) {
      const int m = e / a.D, c = e % a.D;
      const int seg = m / (a.inter + 1), j = m % (a.inter + 1);
      score_dense_coord(a.lie != 0, a.dt, a.inter, a.D, j, c, row + (size_t)seg * 2 * a.D, out + (size_t)m * 2 * a.D);
    }
  }
}

int launch_traj_pairs(const PairArgs& a, hipStream_t st) {
  if (a.B <= 0 || (!a.dist && !a.bits)) return GPMP2MI_OK;
  const long long T = (a.B + GROUP_TILE - 1) / GROUP_TILE;
  const dim3 grid((unsigned)(T * (T + 1) / 2)), block(256);
  if (a.metric == GPMP2MI_DIST_RMS) k_traj_pairs<true><<<grid, block, 0, st>>>(a);
  else k_traj_pairs<false><<<grid, block, 0, st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_group_rule(const GroupRule& a, hipStream_t st) {
  if (a.B > GPMP2MI_MAX_GROUP_ROWS) {
    set_error("more rows than GPMP2MI_MAX_GROUP_ROWS");
    return GPMP2MI_ERR_UNSUPPORTED;
  }
  k_group_rule<<<dim3(1), dim3(RULE_THREADS), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

int launch_group_copy(const GroupCopy& a, hipStream_t st) {
  k_group_copy<<<dim3(a.max_alt), dim3(256), 0, st>>>(a);
  G2_HIP(hipGetLastError());
  return GPMP2MI_OK;
}

}  // namespace g2
