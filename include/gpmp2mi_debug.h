/*
 * gpmp2mi_debug.h -- diagnostic and test entry points of the library behind include/gpmp2mi.h.
 *
 * Nothing here is needed to plan.  These calls exist for the test suite and the probes under scripts/:
 * forcing one of the kernel forms a plan could take, failure injection, and read-outs of solver state.
 * The library reads no environment variable to choose a form; it reads only GPMP2MI_WAIT_TIMEOUT_MS
 * (include/gpmp2mi.h).
 */
#ifndef GPMP2MI_DEBUG_H
#define GPMP2MI_DEBUG_H

#include <stddef.h>

#include "gpmp2mi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Forms a plan would otherwise choose for itself (host/plan_create.hip choose_forms).  The forms agree to rounding, not
 * always bit for bit.  A forced form the plan cannot take is refused with GPMP2MI_ERR_UNSUPPORTED. */
typedef struct gpmp2mi_debug_forms {   /* all zero = the plan's own choice */
  int lin_split;        /* 1, 2, 4: force the fixed-base-arm linearization form (2 and 4: fixed-base arms only;
                           4: obs_check_inter >= 2) */
  int no_fused_finish;  /* 1: k_finish_step / k_finish_trial instead of the fused finish */
  int generic_gn;       /* 1: Gauss-Newton through the trial-step driver (gpmp2mi_plan_update keeps the fast path) */
  int wide_dense;       /* 1: dof 8..11 through the dense block solver */
  int fail_alloc_at;    /* k > 0: the k-th device allocation of this create fails (GPMP2MI_ERR_ALLOC) */
  int no_early_stop;    /* 1: the Gauss-Newton fast driver sums the error behind k_assemble and decides in the step
                           kernel alone, instead of deciding from the linearization's error shares before the build */
} gpmp2mi_debug_forms;
/* gpmp2mi_plan_create with forced forms (forms = NULL: the same call) */
int gpmp2mi_debug_plan_create(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf,
                              const gpmp2mi_settings* setting, const gpmp2mi_graph_opts* opts /*NULL ok*/,
                              int B, const gpmp2mi_debug_forms* forms /*NULL ok*/, gpmp2mi_plan** out);
/* gpmp2mi_multi_plan_create with `forms` forced on every shard's plan; replicate_all = 1 copies the robot and the field
 * to every device in `devices`, the handles' own device included (so that the copy path runs on one GPU) */
int gpmp2mi_debug_multi_plan_create(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf,
                                    const gpmp2mi_settings* setting, const gpmp2mi_graph_opts* opts /*NULL ok*/, int B,
                                    int nshards, const int* devices, const gpmp2mi_debug_forms* forms /*NULL ok*/,
                                    int replicate_all, gpmp2mi_multi_plan** out);
/* Test hook (works without a GPU): robot / field copies owned by live multi plans.  Any pointer may be NULL. */
int gpmp2mi_debug_replica_counts(long* robots, long* sdfs);
/* Test hook: makes set_to (>= 0) the calling thread's current device of the HIP runtime the library uses, then returns
 * that thread's current device in *current (multi-plan calls must leave it as they found it). */
int gpmp2mi_debug_current_device(int set_to, int* current);

/* Test hook: the precision H_seed of the plan's linear prior graph as the plan built it for the seeded calls
 * (include/gpmp2mi.h "seeding"): Hdiag [N+1][2D][2D], Hoff [N][2D][2D] = block (i+1, i).  Either may be NULL. */
int gpmp2mi_debug_plan_seed_prior(gpmp2mi_plan* p, double* Hdiag, double* Hoff);

/* Test hook (works without a GPU): the byte budget of the delta chunk of the plan forms of "sampled clearance"
 * (include/gpmp2mi.h), for every plan of the process; 0 = the default (256 MiB).  A chunk is never smaller than 16 samples,
 * so a small budget lets a test cross chunk borders at small K. */
int gpmp2mi_debug_sampled_chunk_bytes(size_t bytes);

/* Diagnostic (scripts/map_throughput.py): stage times of the updates of "live map" (include/gpmp2mi.h).  With ms4 != NULL
 * it first waits for the last update from occupancy / from points recorded on this handle and returns the device time
 * of its stages in ms: {seed (and mark), the three axis passes, finish, pack}.  Then on = 1 makes the updates that follow
 * record an event between their stages; on = 0 stops that. */
int gpmp2mi_debug_sdf_update_timing(gpmp2mi_sdf* s, int on, double* ms4 /*[4] or NULL*/);
/* Diagnostic (scripts/sensor_throughput.py): the same for the integrate calls of "sensor map" with opts->refresh set.
 * ms6 = {deproject and classify, walk, apply and seed, the three axis passes, finish, pack}.  It switches the timer of
 * gpmp2mi_debug_sdf_update_timing with it: the last four stages are recorded by the same events. */
int gpmp2mi_debug_sdf_integrate_timing(gpmp2mi_sdf* s, int on, double* ms6 /*[6] or NULL*/);
/* Diagnostic (scripts/scene_throughput.py): the rasterisation of a scene (include/gpmp2mi.h "scene"), which in a
 * gpmp2mi_sdf_update_from_scene is part of the first stage of gpmp2mi_debug_sdf_update_timing.  ms2 = {the primitives,
 * the meshes: quantize, cross and fill of each} of the last call recorded on this scene handle. */
int gpmp2mi_debug_scene_timing(gpmp2mi_scene* sc, int on, double* ms2 /*[2] or NULL*/);

/* Diagnostic builds (-DG2_STAMPS) only: 64 raw s_memtime stamps of trajectory b's last solve step. */
int gpmp2mi_plan_debug_stamps(gpmp2mi_plan* p, int b, unsigned long long* out64);
/* Diagnostic: scalars of trajectory b's last LM / Dogleg trial step, out17 = {g.delta, |delta|^2, g.g, g^T H g,
 * g.dx_n, |dx_n|^2, model decrease q, |step|, zero-step flag, -, ..., [16] = current lambda / trust radius}. */
int gpmp2mi_plan_debug_scalars(gpmp2mi_plan* p, int b, double* out17);
/* Test hook, host only (no GPU needed): the wall-clock-bounded spin the pass driver uses on its device-mapped
 * pass flags, run on a caller-owned flag: returns GPMP2MI_OK with *value = *flag once *flag >= 0, or
 * GPMP2MI_ERR_TIMEOUT (gpmp2mi_last_error set) after timeout_ms.  The driver's own limit is 5 s
 * (GPMP2MI_WAIT_TIMEOUT_MS overrides). */
int gpmp2mi_debug_wait_flag(const int* flag, int timeout_ms, int* value);
/* Test hook (works without a GPU: all zeros then): arena chunks / pass-flag buffers owned by live plans, the pooled
 * ones, and the plans leaked because they were poisoned (GPMP2MI_ERR_TIMEOUT).  Any pointer may be NULL. */
int gpmp2mi_debug_resource_counts(long* live_chunks, long* pooled_chunks, long* live_flagbufs, long* pooled_flagbufs,
                                  long* leaked_plans);
/* Test hooks: a one-thread kernel that occupies `stream` until gpmp2mi_debug_stall_release(token) -- or, whatever
 * happens, until max_ms (<= 10000) of device wall clock have passed -- so that the pass driver's timeout path can be
 * driven on a real stream.  release() sets the flag, waits for that stream and frees the token. */
int gpmp2mi_debug_stall_begin(void* stream, int max_ms, void** token);
int gpmp2mi_debug_stream_create(void** stream);   /* a non-blocking stream of the HIP runtime the library uses */
int gpmp2mi_debug_stream_destroy(void* stream);
int gpmp2mi_debug_stall_release(void* token);
/* Test hooks: device memory from the HIP runtime the library uses, for the tests of the `_dev` entry points (a test
 * process must not pull in a second runtime to own a buffer).  alloc fills with `fill_byte`; read / write are blocking
 * copies on the default stream, which does not wait for the non-blocking streams of gpmp2mi_debug_stream_create; free
 * waits for the device. */
int gpmp2mi_debug_device_alloc(size_t bytes, int fill_byte, void** out);
int gpmp2mi_debug_device_read(void* dst_host, const void* src_dev, size_t bytes);
int gpmp2mi_debug_device_write(void* dst_dev, const void* src_host, size_t bytes);
int gpmp2mi_debug_device_free(void* p);
/* Diagnostic: lane semantics of the wave-level moves the solver relies on (tests/test_gpu_plan.py). */
int gpmp2mi_debug_crosslane(const double* in64, double* out512);
/* Diagnostic: raw device-to-host copy of a solver hand-over buffer of the plan (0: diagonal tiles [B][N+1][256],
 * 1: factor tiles [B][N+1][3][256], 2: pending Schur tiles [B][groups][256], 3: level-4 couplings [B][groups][256]). */
int gpmp2mi_plan_debug_read(gpmp2mi_plan* p, int which, double* out, long count);

#ifdef __cplusplus
}
#endif
#endif /* GPMP2MI_DEBUG_H */
