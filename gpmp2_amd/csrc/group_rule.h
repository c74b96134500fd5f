// group_rule.h -- the grouping rule of include/gpmp2mi.h "distinct alternatives", stated once for the host form
// (host/group.hip) and the rule kernel (group_kernels.hip); plain C++ so that a host compiler can include it too.
//
// The rule visits the participating rows in rank order and lets each join the first leader within `radius`.  It needs no
// sort: a row that no earlier leader took is, when its turn comes, the best-ranked row nobody has decided yet, and the
// rows it takes are exactly the undecided rows within `radius` of it -- every one of them was refused by all earlier
// leaders, so this leader is their first.  Hence the rounds below: argmin over the undecided rows, make it a leader,
// decide its neighbours; n_modes rounds.
#pragma once
#include <climits>
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define G2_RULE_HD __host__ __device__ inline
#else
#define G2_RULE_HD inline
#endif

namespace g2 {

constexpr int GROUP_UNDECIDED = -2;   // a participating row no leader has taken yet; -1: the row does not take part

G2_RULE_HD bool group_takes_part(double score, int eligible) { return eligible != 0 && std::isfinite(score); }

// rank order: ascending score, the lowest row on ties.  (+inf, INT_MAX) stands for "no row".
G2_RULE_HD bool group_rank_less(double sa, int ra, double sb, int rb) { return sa < sb || (sa == sb && ra < rb); }

// a row joins a leader's mode: false for a NaN distance
G2_RULE_HD bool group_within(double dist, double radius) { return dist <= radius; }

// the bit matrix the pair kernel leaves: row r has group_words(B) 64-bit words, bit c of the row is group_within(dist(r, c))
G2_RULE_HD int group_words(int B) { return (B + 63) / 64; }
G2_RULE_HD bool group_bit(const unsigned long long* bits, int W, int r, int c) {
  return (bits[(size_t)r * W + (c >> 6)] >> (c & 63)) & 1ull;
}

// The rounds on the host.  within(leader, row) is the adjacency; every output may be null.
template <class Within>
inline void group_rule_host(int B, const double* score, const int* eligible, Within within, int* mode, int* leaders,
                            int* sizes, int* n_modes, int* work /*[B]*/) {
  for (int b = 0; b < B; b++)
    work[b] = group_takes_part(score[b], eligible ? eligible[b] : 1) ? GROUP_UNDECIDED : -1;
  int k = 0;
  for (;; k++) {
    double bs = HUGE_VAL;
    int br = INT_MAX;
    for (int b = 0; b < B; b++)
      if (work[b] == GROUP_UNDECIDED && group_rank_less(score[b], b, bs, br)) { bs = score[b]; br = b; }
    if (br == INT_MAX) break;
    int cnt = 0;
    for (int b = 0; b < B; b++)
      if (work[b] == GROUP_UNDECIDED && (b == br || within(br, b))) { work[b] = k; cnt++; }
    if (leaders) leaders[k] = br;
    if (sizes) sizes[k] = cnt;
  }
  for (int j = k; j < B; j++) {
    if (leaders) leaders[j] = -1;
    if (sizes) sizes[j] = 0;
  }
  if (mode)
    for (int b = 0; b < B; b++) mode[b] = work[b];
  if (n_modes) *n_modes = k;
}

}  // namespace g2
