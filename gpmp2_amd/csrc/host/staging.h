// staging.h -- how the host units lay out a device workspace and stage the per-row outputs of a check stage: the carver,
// the descriptor of one per-row output with its staging rule, and the blocks every check stage's workspace is made of.
// No HIP in here: the host compiler alone builds it (tests/cpp/staging_shim.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace g2 {

constexpr size_t WS_ALIGN = 256;
inline size_t ws_round(size_t bytes) { return (bytes + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN; }

// Carves a workspace front to back, every piece rounded up to WS_ALIGN.  A null base gives the sizes alone: `off` is the
// total, and the pointers it hands out are the offsets.
struct Carver {
  char* base;
  size_t off = 0;
  char* operator()(size_t bytes) {
    char* p = (char*)((uintptr_t)base + off);   // no pointer arithmetic on a null base
    off += ws_round(bytes);
    return p;
  }
  template <class T>
  T* take(size_t count) { return (T*)(*this)(count * sizeof(T)); }
};

// One per-row output of a check stage, [B][per_row] of `elem` bytes: the caller's array (host or device, may be null) and
// its room in the stage's workspace once carved.  A stage states its outputs once, as a short array of these; the layout,
// the staging rule and the read-back (finish_host: check_common.hip) all go by that array.
struct RowOut {
  void* caller;
  size_t elem, per_row;
  char* staged = nullptr;
  size_t bytes(size_t B) const { return B * per_row * elem; }
};
template <class T>
RowOut row(T* caller, size_t per_row = 1) { return RowOut{caller, sizeof(T), per_row}; }
inline void carve_rows(Carver& c, RowOut* rows, int n, size_t B) {
  for (int i = 0; i < n; i++) rows[i].staged = c(rows[i].bytes(B));
}
// The staging rule, where a kernel writes an output: a device form writes the caller's array; a host form writes the
// staged one, and computes only what the caller asked for.
inline void* staging_rule(bool host, void* caller, void* staged) { return host ? (caller ? staged : nullptr) : caller; }
template <class T>
T* target(const RowOut& r, bool host) { return (T*)staging_rule(host, r.caller, r.staged); }

// The per-row scores of the earlier stages that a selection rule reads, in a later stage's workspace.  n = 1: the
// obstacle stage; 2: and the self check; 3: and the motion limits.  The doubles come first, then the ints.
struct PriorRows {
  double *clearance = nullptr, *self_clearance = nullptr, *pos_margin = nullptr;
  int *oor = nullptr, *self_invalid = nullptr, *motion_invalid = nullptr;
};
inline PriorRows carve_priors(Carver& c, size_t B, int n) {
  PriorRows w;
  double** d[3] = {&w.clearance, &w.self_clearance, &w.pos_margin};
  int** i[3] = {&w.oor, &w.self_invalid, &w.motion_invalid};
  for (int k = 0; k < n; k++) *d[k] = c.take<double>(B);
  for (int k = 0; k < n; k++) *i[k] = c.take<int>(B);
  return w;
}

// What a selection leaves for the host: best, n_eligible, then (8-byte aligned) the chosen row's final_error and, where
// the stage has one, its extra double, read back in one copy; behind it the chosen row, and the stage's extra array of
// that row where it has one (extra_row_bytes > 0).
struct PickBlock {
  int best, n_eligible;
  double best_err, extra;
};
struct PickRows {
  PickBlock* pick = nullptr;
  double *traj_best = nullptr, *dense_best = nullptr, *extra_row = nullptr;
};
struct Shape {   // B rows of N + 1 support states and Md checked states, D degrees of freedom
  size_t B, N, D, Md;
};
inline PickRows carve_pick(Carver& c, const Shape& s, bool extra, size_t extra_row_bytes = 0) {
  PickRows w;
  w.pick = (PickBlock*)c(sizeof(PickBlock) - (extra ? 0 : sizeof(double)));
  w.traj_best = c.take<double>((s.N + 1) * 2 * s.D);
  w.dense_best = c.take<double>(s.Md * 2 * s.D);
  if (extra_row_bytes) w.extra_row = (double*)c(extra_row_bytes);
  return w;
}

// ---- the per-row outputs of the stages, each stated once: the typed face, its list, and the list resolved by the
// staging rule back into the typed face (what the stage's finish kernel gets)

// score, self check (oor: invalid), moving obstacles (oor: invalid) and the carried object share a face; `worst` is [B][worst_w]
struct ScoreOut {
  double *support = nullptr, *dense = nullptr, *clearance = nullptr;
  int *worst = nullptr, *oor = nullptr;
};
inline ScoreOut make_out(double* support, double* dense, double* clearance, int* worst, int* oor) {
  ScoreOut o;
  o.support = support, o.dense = dense, o.clearance = clearance, o.worst = worst, o.oor = oor;
  return o;
}
constexpr int SCORE_ROWS = 5, SCORE_WORST = 2, SELF_WORST = 2, MOVING_WORST = 3, CARRIED_WORST = 2;
inline void rows_of(const ScoreOut& o, size_t worst_w, RowOut* r) {
  r[0] = row(o.support), r[1] = row(o.dense), r[2] = row(o.clearance), r[3] = row(o.worst, worst_w), r[4] = row(o.oor);
}
inline ScoreOut score_out(const RowOut* r, bool host) {
  ScoreOut o;
  o.support = target<double>(r[0], host), o.dense = target<double>(r[1], host), o.clearance = target<double>(r[2], host);
  o.worst = target<int>(r[3], host), o.oor = target<int>(r[4], host);
  return o;
}

struct MotionOut {
  double *pos_margin = nullptr, *vel_ratio = nullptr, *acc_ratio = nullptr, *point_speed = nullptr, *time_scale = nullptr;
  int *worst = nullptr, *invalid = nullptr;   // worst: [B][4][2]
};
constexpr int MOTION_ROWS = 7;
inline void rows_of(const MotionOut& o, RowOut* r) {
  r[0] = row(o.pos_margin), r[1] = row(o.vel_ratio), r[2] = row(o.acc_ratio), r[3] = row(o.point_speed);
  r[4] = row(o.time_scale), r[5] = row(o.worst, 8), r[6] = row(o.invalid);
}
inline MotionOut motion_out(const RowOut* r, bool host) {
  MotionOut o;
  o.pos_margin = target<double>(r[0], host), o.vel_ratio = target<double>(r[1], host);
  o.acc_ratio = target<double>(r[2], host), o.point_speed = target<double>(r[3], host);
  o.time_scale = target<double>(r[4], host), o.worst = target<int>(r[5], host), o.invalid = target<int>(r[6], host);
  return o;
}

struct PathOut {
  double *max_pos = nullptr, *max_rot = nullptr;
  int* worst = nullptr;   // [B][2]
  double *support = nullptr, *dense = nullptr;
  int* invalid = nullptr;
};
constexpr int PATH_ROWS = 6;
inline void rows_of(const PathOut& o, RowOut* r) {
  r[0] = row(o.max_pos), r[1] = row(o.max_rot), r[2] = row(o.worst, 2), r[3] = row(o.support), r[4] = row(o.dense);
  r[5] = row(o.invalid);
}
inline PathOut path_out(const RowOut* r, bool host) {
  PathOut o;
  o.max_pos = target<double>(r[0], host), o.max_rot = target<double>(r[1], host), o.worst = target<int>(r[2], host);
  o.support = target<double>(r[3], host), o.dense = target<double>(r[4], host), o.invalid = target<int>(r[5], host);
  return o;
}

// re-timing: the first RETIME_CORE_ROWS are the profile itself, which the kernel needs room for whoever asks (a null
// one takes the workspace's: enqueue_retime); a caller's trajectory call carves those alone
struct RetimeOut {
  double *sdot = nullptr, *u = nullptr, *stamps = nullptr, *duration = nullptr, *achieved = nullptr, *dense = nullptr;
  int* status = nullptr;
};
constexpr int RETIME_ROWS = 7, RETIME_CORE_ROWS = 3;
inline void rows_of(const RetimeOut& o, size_t Md, size_t D, RowOut* r) {
  r[0] = row(o.sdot, Md), r[1] = row(o.u, Md), r[2] = row(o.stamps, Md);
  r[3] = row(o.duration), r[4] = row(o.achieved, 4), r[5] = row(o.dense, Md * 2 * D), r[6] = row(o.status);
}
inline RetimeOut retime_out(const RowOut* r, bool host) {
  RetimeOut o;
  o.sdot = target<double>(r[0], host), o.u = target<double>(r[1], host), o.stamps = target<double>(r[2], host);
  o.duration = target<double>(r[3], host), o.achieved = target<double>(r[4], host);
  o.dense = target<double>(r[5], host), o.status = target<int>(r[6], host);
  return o;
}

// ---- the workspace of a plan's check stage, in carve order: the stage's records (one set, or two), the per-row scores
// of the earlier stages, the staged outputs, the pick.  rec_bytes: B rows of the stage's records (launch.h knows them).
struct CheckWs {
  char *recs = nullptr, *recs2 = nullptr;
  PriorRows prior;
  PickRows sel;
  size_t bytes = 0;
};
inline CheckWs carve_check(char* base, size_t rec_bytes, size_t rec2_bytes, int n_prior, RowOut* rows, int n_rows,
                           const Shape& s, bool pick_extra) {
  CheckWs w;
  Carver c{base};
  w.recs = c(rec_bytes);
  if (rec2_bytes) w.recs2 = c(rec2_bytes);
  w.prior = carve_priors(c, s.B, n_prior);
  carve_rows(c, rows, n_rows, s.B);
  w.sel = carve_pick(c, s, pick_extra);
  w.bytes = c.off;
  return w;
}
// the six stages that keep a CheckWs (rows: the stage's rows_of).  The self check keeps the records of k_score for
// select_checked as its second set; motion limits, moving obstacles and the carried object read the obstacle stage and the self check, the
// workspace path the obstacle stage alone; the motion limits carry time_scale in the pick.
inline CheckWs carve_score(char* base, size_t rec_bytes, RowOut* rows, const Shape& s) {
  return carve_check(base, rec_bytes, 0, 0, rows, SCORE_ROWS, s, false);
}
inline CheckWs carve_self(char* base, size_t rec_bytes, size_t obstacle_rec_bytes, RowOut* rows, const Shape& s) {
  return carve_check(base, rec_bytes, obstacle_rec_bytes, 0, rows, SCORE_ROWS, s, false);
}
inline CheckWs carve_motion(char* base, size_t rec_bytes, RowOut* rows, const Shape& s) {
  return carve_check(base, rec_bytes, 0, 2, rows, MOTION_ROWS, s, true);
}
inline CheckWs carve_moving(char* base, size_t rec_bytes, RowOut* rows, const Shape& s) {
  return carve_check(base, rec_bytes, 0, 2, rows, SCORE_ROWS, s, false);
}
inline CheckWs carve_carried(char* base, size_t rec_bytes, RowOut* rows, const Shape& s) {
  return carve_check(base, rec_bytes, 0, 2, rows, SCORE_ROWS, s, false);
}
inline CheckWs carve_path(char* base, size_t rec_bytes, RowOut* rows, const Shape& s) {
  return carve_check(base, rec_bytes, 0, 1, rows, PATH_ROWS, s, false);
}

// re-timing keeps more: ps and X [B][Md] and K [B][Md][2] of k_retime_caps / k_retime in front of its rows, the scores
// of all three earlier stages behind them, and the chosen row's stamps [Md] behind the pick
struct RetimeCore {
  double *ps, *X, *K;
};
inline RetimeCore carve_retime_core(Carver& c, RowOut* rows, size_t B, size_t Md) {
  RetimeCore w;
  w.ps = c.take<double>(B * Md);
  w.X = c.take<double>(B * Md);
  w.K = c.take<double>(2 * B * Md);
  carve_rows(c, rows, RETIME_CORE_ROWS, B);
  return w;
}
struct RetimeWs {
  RetimeCore core;
  PriorRows prior;
  PickRows sel;
  size_t bytes;
};
inline RetimeWs carve_retime(char* base, RowOut* rows, const Shape& s) {
  RetimeWs w;
  Carver c{base};
  w.core = carve_retime_core(c, rows, s.B, s.Md);
  carve_rows(c, rows + RETIME_CORE_ROWS, RETIME_ROWS - RETIME_CORE_ROWS, s.B);
  w.prior = carve_priors(c, s.B, 3);
  w.sel = carve_pick(c, s, true, s.Md * sizeof(double));
  w.bytes = c.off;
  return w;
}

// torque limits: tau [B][Md][D] is the last row, which a selection needs room for whoever asks (the chosen row's torques
// are copied out of it)
struct TorqueOut {
  double *torque_ratio = nullptr, *static_ratio = nullptr, *time_scale = nullptr;
  int *worst = nullptr, *invalid = nullptr;   // worst: [B][3][2]
  double* tau = nullptr;
};
constexpr int TORQUE_ROWS = 6;
inline void rows_of(const TorqueOut& o, size_t Md, size_t D, RowOut* r) {
  r[0] = row(o.torque_ratio), r[1] = row(o.static_ratio), r[2] = row(o.time_scale), r[3] = row(o.worst, 6);
  r[4] = row(o.invalid), r[5] = row(o.tau, Md * D);
}
inline TorqueOut torque_out(const RowOut* r, bool host) {
  TorqueOut o;
  o.torque_ratio = target<double>(r[0], host), o.static_ratio = target<double>(r[1], host);
  o.time_scale = target<double>(r[2], host), o.worst = target<int>(r[3], host), o.invalid = target<int>(r[4], host);
  o.tau = target<double>(r[5], host);
  return o;
}
// the stage's records, the scores of all three earlier stages with the motion stage's time_scale [B] behind them, the
// staged outputs, and the pick with the chosen row's torques [Md][D] behind it
struct TorqueWs {
  char* recs;
  PriorRows prior;
  double* motion_time_scale;
  PickRows sel;
  size_t bytes;
};
inline TorqueWs carve_torque(char* base, size_t rec_bytes, RowOut* rows, const Shape& s) {
  TorqueWs w;
  Carver c{base};
  w.recs = c(rec_bytes);
  w.prior = carve_priors(c, s.B, 3);
  w.motion_time_scale = c.take<double>(s.B);
  carve_rows(c, rows, TORQUE_ROWS, s.B);
  w.sel = carve_pick(c, s, true, s.Md * s.D * sizeof(double));
  w.bytes = c.off;
  return w;
}

// re-timing under torque limits: the outputs of re-timing (achieved is [B][6] here), the torques of the re-timed row
// [B][Md][D] and the coefficients [B][Md][4][D].  The last two have room whoever asks: the chain reads the coefficients,
// and a selection copies the chosen row's torques.
struct RetimeDynOut : RetimeOut {
  double *tau = nullptr, *coef = nullptr;
};
constexpr int RETIME_DYN_ROWS = 9;
inline void rows_of(const RetimeDynOut& o, size_t Md, size_t D, RowOut* r) {
  rows_of(static_cast<const RetimeOut&>(o), Md, D, r);
  r[4] = row(o.achieved, 6);
  r[7] = row(o.tau, Md * D), r[8] = row(o.coef, Md * 4 * D);
}
inline RetimeDynOut retime_dyn_out(const RowOut* r, bool host) {
  RetimeDynOut o;
  static_cast<RetimeOut&>(o) = retime_out(r, host);
  o.tau = target<double>(r[7], host), o.coef = target<double>(r[8], host);
  return o;
}
// what k_retime needs, the rows of k_retime_rows ([B][Md][4 D][4]: 2 D acceleration and 2 D torque rows per stage) and a
// flag per row (a coefficient is not finite); a caller's trajectory call carves this alone
struct RetimeDynCore {
  RetimeCore core;
  double* stage_rows;
  int* nonfinite;
};
inline RetimeDynCore carve_retime_dyn_core(Carver& c, RowOut* rows, size_t B, size_t Md, size_t D) {
  RetimeDynCore w;
  w.core = carve_retime_core(c, rows, B, Md);
  w.stage_rows = c.take<double>(B * Md * 4 * D * 4);
  w.nonfinite = c.take<int>(B);
  carve_rows(c, rows + 7, 2, B);
  return w;
}
// the scores of all three earlier stages behind them, and the chosen row's stamps [Md] and torques [Md][D] behind the pick
struct RetimeDynWs {
  RetimeDynCore core;
  PriorRows prior;
  PickRows sel;
  size_t bytes;
};
inline RetimeDynWs carve_retime_dyn(char* base, RowOut* rows, const Shape& s) {
  RetimeDynWs w;
  Carver c{base};
  w.core = carve_retime_dyn_core(c, rows, s.B, s.Md, s.D);
  carve_rows(c, rows + RETIME_CORE_ROWS, RETIME_ROWS - RETIME_CORE_ROWS, s.B);
  w.prior = carve_priors(c, s.B, 3);
  w.sel = carve_pick(c, s, true, s.Md * (1 + s.D) * sizeof(double));
  w.bytes = c.off;
  return w;
}

// distinct alternatives: the bit matrix of k_traj_pairs ([B][words] 64-bit words), the per-row scores the rule reads,
// what the rule leaves, then the staging of the host form (`alt_cap` slots of indices, sizes and errors; max_alt slabs)
struct GroupWs {
  unsigned long long* bits;
  PriorRows prior;
  int *mode, *leaders, *sizes;
  int* pick;   // n_modes, n_eligible
  int *alt, *alt_size;
  double *alt_error, *traj_alt, *dense_alt;
  size_t bytes;
};
inline GroupWs carve_group(char* base, const Shape& s, size_t words, size_t alt_cap, size_t max_alt) {
  GroupWs w;
  Carver c{base};
  w.bits = c.take<unsigned long long>(s.B * words);
  w.prior = carve_priors(c, s.B, 2);
  w.mode = c.take<int>(s.B);
  w.leaders = c.take<int>(s.B);
  w.sizes = c.take<int>(s.B);
  w.pick = c.take<int>(2);
  w.alt = c.take<int>(alt_cap);
  w.alt_size = c.take<int>(alt_cap);
  w.alt_error = c.take<double>(alt_cap);
  w.traj_alt = c.take<double>(max_alt * (s.N + 1) * 2 * s.D);
  w.dense_alt = c.take<double>(max_alt * s.Md * 2 * s.D);
  w.bytes = c.off;
  return w;
}

}  // namespace g2
