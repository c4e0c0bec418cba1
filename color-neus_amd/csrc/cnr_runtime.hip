// What every HIP unit of the library shares at run time: the backend's name, the error latch behind CNR_LAUNCH_CHECK, per-launch event timing,
// named profiler ranges, and the memset / column helpers.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <cstdio>
#include <vector>

#include "cnr_backend.h"
#include "cnr_hip_util.h"

namespace cnr {

hipError_t g_first_error = hipSuccess;
const char* g_first_error_where = "";

const char* be_name() { return "hip-gfx950"; }

// ---- per-launch timing (HIP events recorded on the launch stream) ---------------------------------------------------
struct TimingRec { KernelTiming t; hipEvent_t e0, e1; };
static bool g_timing_on = false;
static std::vector<TimingRec> g_timing;
static std::vector<hipEvent_t> g_event_pool;
static hipEvent_t get_event() {
  if (!g_event_pool.empty()) { hipEvent_t e = g_event_pool.back(); g_event_pool.pop_back(); return e; }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}
void timing_begin(const char* name, int kind, int nt, long P, int N, int K, int pairs, hipStream_t s, double bytes) {
  if (!g_timing_on) return;
  TimingRec r;
  snprintf(r.t.name, sizeof r.t.name, "%s", name);
  r.t.kind = kind; r.t.nt = nt; r.t.P = P; r.t.N = N; r.t.K = K; r.t.pairs = pairs; r.t.ms = 0.f; r.t.bytes = bytes;
  r.e0 = get_event(); r.e1 = get_event();
  (void)hipEventRecord(r.e0, s);
  g_timing.push_back(r);
}
void timing_end(hipStream_t s) {
  if (!g_timing_on || g_timing.empty()) return;
  (void)hipEventRecord(g_timing.back().e1, s);
}
void be_timing_enable(int on) { g_timing_on = on != 0; }
int be_timing_collect(KernelTiming* out, int max_records) {
  int n = 0;
  for (auto& r : g_timing) {
    (void)hipEventSynchronize(r.e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.e0, r.e1);
    r.t.ms = ms;
    if (out && n < max_records) out[n] = r.t;
    ++n;
    g_event_pool.push_back(r.e0);
    g_event_pool.push_back(r.e1);
  }
  g_timing.clear();
  return n;
}

namespace {
struct Roctx {
  int (*push)(const char*) = nullptr; int (*pop)() = nullptr;
  Roctx() {
    if (!debug_flags().roctx) return;
    for (const char* lib : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
      void* h = dlopen(lib, RTLD_LAZY | RTLD_GLOBAL);
      if (!h) continue;
      push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
      pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
      if (push && pop) return;
      push = nullptr; pop = nullptr;
    }
  }
};
Roctx& roctx() { static Roctx r; return r; }
}  // namespace
void be_range_push(const char* name) { if (roctx().push) (void)roctx().push(name); }
void be_range_pop() { if (roctx().pop) (void)roctx().pop(); }

int be_check_last_error(char* msg, size_t n) {
  if (g_first_error == hipSuccess) return 0;
  snprintf(msg, n, "HIP error in %s: %s", g_first_error_where, hipGetErrorString(g_first_error));
  g_first_error = hipSuccess;
  return -1;
}

void device_fill(void* p, int byte, size_t bytes, hipStream_t s, const char* where) {
  hipError_t e = hipMemsetAsync(p, byte, bytes, s);
  if (e != hipSuccess && g_first_error == hipSuccess) { g_first_error = e; g_first_error_where = where; }
}
void be_memset_zero(void* p, size_t bytes, cnr_stream s) { device_fill(p, 0, bytes, s, "memset"); }

__global__ void zero_cols_kernel(float* p, int ld, int c0, int c1, long rows) {
  const int w = c1 - c0;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows * w) p[(i / w) * ld + c0 + (int)(i % w)] = 0.0f;
}
void be_zero_cols(float* p, int ld, int c0, int c1, long rows, cnr_stream s) {
  if (c1 <= c0 || rows <= 0) return;
  const long n = rows * (c1 - c0);
  hipLaunchKernelGGL(zero_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, ld, c0, c1, rows);
  CNR_LAUNCH_CHECK("zero_cols");
}

__global__ __launch_bounds__(256) void copy_cols_kernel(float* dst, int ld_dst, const float* src, int ld_src, int ncols, long rows) {
  const long n = rows * ncols;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / ncols;
    const int c = (int)(i - r * ncols);
    dst[r * ld_dst + c] = src[r * ld_src + c];
  }
}
void be_copy_cols(float* dst, int ld_dst, const float* src, int ld_src, int ncols, long rows, cnr_stream s) {
  if (ncols <= 0 || rows <= 0) return;
  long blocks = (rows * ncols + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(copy_cols_kernel, dim3((unsigned)blocks), dim3(256), 0, s, dst, ld_dst, src, ld_src, ncols, rows);
  CNR_LAUNCH_CHECK("copy_cols");
}

}  // namespace cnr
