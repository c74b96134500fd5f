// debug.hip -- the diagnostics and test hooks of include/gpmp2mi_debug.h that do not belong to a unit's own state: raw
// reads of a plan's buffers, the flag wait on a caller's word, streams, the stall kernel of the timeout tests.
#include "host.h"

using namespace g2;

// test hook kernel (gpmp2mi_debug_stall_begin): spins on a host-mapped word, bounded by the device's real-time clock
__global__ void k_debug_stall(const int* flag, long long max_ticks) {
  const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
  while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0) {
    if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > max_ticks) break;
    __builtin_amdgcn_s_sleep(64);
  }
}

extern "C" {

// diagnostic: raw s_memtime stamps of the last step kernel (all zero unless built with -DG2_STAMPS)
int gpmp2mi_plan_debug_stamps(gpmp2mi_plan* p, int b, unsigned long long* out64) {
  // rows B .. 2B - 1 hold the per-task stamps of the cyclic reduction (G2_TSTAMP) of trajectory b - B
  G2_CHECK(p && out64 && b >= 0 && b < 2 * p->hp.B, GPMP2MI_ERR_INVALID, "bad argument");
  G2_HIP(hipMemcpy(out64, p->pb.stamps + (size_t)b * 64, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return GPMP2MI_OK;
}

// diagnostic: the scalars of trajectory b's last trial step (PlanBuffers::scal, see plan.h SC_*) and its
// current lambda / trust radius in out[16]
int gpmp2mi_plan_debug_scalars(gpmp2mi_plan* p, int b, double* out17) {
  G2_CHECK(p && out17 && b >= 0 && b < p->hp.B, GPMP2MI_ERR_INVALID, "bad argument");
  G2_HIP(hipMemcpy(out17, p->pb.scal + (size_t)b * SC_COUNT, SC_COUNT * sizeof(double), hipMemcpyDeviceToHost));
  G2_HIP(hipMemcpy(out17 + SC_COUNT, p->pb.lambda + b, sizeof(double), hipMemcpyDeviceToHost));
  return GPMP2MI_OK;
}

// diagnostic: out[8][64] = {bcast_row<0..3>, bcast_in_row<5>, row_sum16, sum_rows, bcast_in_row<13>}(in[64])
int gpmp2mi_debug_crosslane(const double* in64, double* out512) {
  G2_CHECK(in64 && out512, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(ensure_device());
  DevBuf<double> di, dout;
  G2_TRY(di.upload(in64, 64));
  G2_TRY(dout.out(out512, 512));
  G2_TRY(launch_debug_crosslane(di.p, dout.p, nullptr));
  return fetch_all(dout);
}

// test hook (host only, no GPU needed): the bounded spin of the pass driver on a caller-owned flag
int gpmp2mi_debug_wait_flag(const int* flag, int timeout_ms, int* value) {
  G2_CHECK(flag && value && timeout_ms > 0, GPMP2MI_ERR_INVALID, "bad argument");
  return spin_wait_flag(flag, false, nullptr, timeout_ms * 1e-3, value);
}

// diagnostic: raw copy of one of the solver's hand-over buffers (0 tiles, 1 fac, 2 pend, 3 coup) to the host
int gpmp2mi_plan_debug_read(gpmp2mi_plan* p, int which, double* out, long count) {
  G2_CHECK(p && out && count >= 0, GPMP2MI_ERR_INVALID, "bad argument");
  const double* src = which == 0 ? p->pb.tiles : which == 1 ? p->pb.fac : which == 2 ? p->pb.pend : which == 3 ? p->pb.coup : nullptr;
  G2_CHECK(src, GPMP2MI_ERR_INVALID, "unknown buffer");
  G2_HIP(hipMemcpy(out, src, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
  return GPMP2MI_OK;
}

// test hook: a kernel that occupies `stream` until gpmp2mi_debug_stall_release (or, whatever happens, until max_ms
// of device wall clock have passed: every wave reaches that exit), so that the pass driver's timeout path can be driven
// on a real stream.  One thread; polls a host-mapped word.
struct gpmp2mi_stall_token {
  int* host = nullptr;
  int* dev = nullptr;
  hipStream_t st = nullptr;
};
// test hooks: a non-blocking HIP stream from the runtime this library is linked against (a test process must not pull
// in a second HIP runtime just to get a stream)
int gpmp2mi_debug_stream_create(void** stream) {
  G2_CHECK(stream, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(ensure_device());
  hipStream_t st = nullptr;
  G2_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  *stream = st;
  return GPMP2MI_OK;
}
int gpmp2mi_debug_stream_destroy(void* stream) {
  if (stream) G2_HIP(hipStreamDestroy((hipStream_t)stream));
  return GPMP2MI_OK;
}
int gpmp2mi_debug_stall_begin(void* stream, int max_ms, void** token) {
  G2_CHECK(token && max_ms > 0 && max_ms <= 10000, GPMP2MI_ERR_INVALID, "bad argument");
  G2_TRY(ensure_device());
  auto t = std::make_unique<gpmp2mi_stall_token>();
  G2_HIP(hipHostMalloc((void**)&t->host, sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
  *t->host = 0;
  G2_HIP(hipHostGetDevicePointer((void**)&t->dev, t->host, 0));
  t->st = (hipStream_t)stream;
  k_debug_stall<<<dim3(1), dim3(1), 0, t->st>>>(t->dev, (long long)max_ms * 100000LL);   // s_memrealtime: 100 MHz
  G2_HIP(hipGetLastError());
  *token = t.release();
  return GPMP2MI_OK;
}
int gpmp2mi_debug_stall_release(void* token) {
  auto* t = static_cast<gpmp2mi_stall_token*>(token);
  G2_CHECK(t && t->host, GPMP2MI_ERR_INVALID, "null token");
  __atomic_store_n(t->host, 1, __ATOMIC_RELEASE);
  const hipError_t e = hipStreamSynchronize(t->st);
  (void)hipHostFree(t->host);
  delete t;
  G2_HIP(e);
  return GPMP2MI_OK;
}

// test hooks: device buffers for the tests of the `_dev` entry points, from this library's HIP runtime
int gpmp2mi_debug_device_alloc(size_t bytes, int fill_byte, void** out) {
  G2_CHECK(out && bytes > 0, GPMP2MI_ERR_INVALID, "bad argument");
  *out = nullptr;
  G2_TRY(ensure_device());
  void* p = nullptr;
  G2_TRY(dev_malloc(&p, bytes));
  const hipError_t e = hipMemset(p, fill_byte, bytes);
  if (e != hipSuccess) (void)hipFree(p);
  G2_HIP(e);
  G2_HIP(hipStreamSynchronize(nullptr));
  *out = p;
  return GPMP2MI_OK;
}
int gpmp2mi_debug_device_read(void* dst_host, const void* src_dev, size_t bytes) {
  G2_CHECK(dst_host && src_dev && bytes > 0, GPMP2MI_ERR_INVALID, "bad argument");
  G2_TRY(ensure_device());
  G2_HIP(hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost));
  return GPMP2MI_OK;
}
int gpmp2mi_debug_device_write(void* dst_dev, const void* src_host, size_t bytes) {
  G2_CHECK(dst_dev && src_host && bytes > 0, GPMP2MI_ERR_INVALID, "bad argument");
  G2_TRY(ensure_device());
  G2_HIP(hipMemcpy(dst_dev, src_host, bytes, hipMemcpyHostToDevice));
  return GPMP2MI_OK;
}
int gpmp2mi_debug_device_free(void* p) {
  if (p) G2_HIP(hipFree(p));
  return GPMP2MI_OK;
}

int gpmp2mi_debug_current_device(int set_to, int* current) {
  G2_CHECK(current, GPMP2MI_ERR_INVALID, "null argument");
  G2_TRY(ensure_device());
  if (set_to >= 0) G2_HIP(hipSetDevice(set_to));
  G2_HIP(hipGetDevice(current));
  return GPMP2MI_OK;
}

// test hook: robot / field copies owned by live multi plans (works without a GPU: zeros then)
int gpmp2mi_debug_replica_counts(long* robots, long* sdfs) {
  if (robots) *robots = g_robot_replicas.load();
  if (sdfs) *sdfs = g_sdf_replicas.load();
  return GPMP2MI_OK;
}

}  // extern "C"
