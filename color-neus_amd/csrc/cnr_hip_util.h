// shared error bookkeeping of the HIP translation units
#pragma once
#include <hip/hip_runtime.h>
namespace cnr {
extern hipError_t g_first_error;
extern const char* g_first_error_where;
// the one fill of device memory: `byte` into `bytes` bytes at p on the stream; a failure is recorded as the first error under `where`
void device_fill(void* p, int byte, size_t bytes, hipStream_t s, const char* where);
// optional per-launch timing with HIP events on the launch stream (bench / profiling only; off by default)
void timing_begin(const char* name, int kind, int nt, long P, int N, int K, int pairs, hipStream_t s, double bytes);
void timing_end(hipStream_t s);
// hipFuncSetAttribute is a per-device setting: remember per (kernel instantiation, device) that it has been applied.
// (launch_lds below is its user: one opt-in per kernel instantiation and device)
struct DeviceOnce {
  bool done[64] = {};
  bool first() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return true;   // unknown device: just apply the attribute again
    if (done[dev]) return false;
    done[dev] = true;
    return true;
  }
};
// Launch of a kernel that needs more dynamic LDS than the default limit: the opt-in up to `lds_max` bytes, once per kernel instantiation and
// device, then the launch with `lds` bytes.  (A launch record is the caller's: a TimingScope around the call.)
template <auto Kernel, class... Args>
void launch_lds(dim3 grid, dim3 block, size_t lds, size_t lds_max, hipStream_t s, const Args&... args) {
  static DeviceOnce attr_once;
  if (attr_once.first()) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
  hipLaunchKernelGGL(Kernel, grid, block, lds, s, args...);
}
struct TimingScope {
  hipStream_t s;
  TimingScope(const char* name, int kind, int nt, long P, int N, int K, int pairs, hipStream_t st, double bytes = 0.0) : s(st) {
    timing_begin(name, kind, nt, P, N, K, pairs, s, bytes);
  }
  ~TimingScope() { timing_end(s); }
};
}
// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains every outstanding global access of the wave
// (s_waitcnt vmcnt(0) in front of s_barrier): in the streaming GEMM kernels that makes the tile prefetched for a later iteration
// land before EVERY barrier, i.e. the prefetch distance can never exceed one iteration.  Those kernels exchange data between waves
// through LDS only (global data written by a wave is never read by another wave of the same launch), so no global ordering is needed.
__device__ __forceinline__ void cnr_lds_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
}
// 1 / s for a power of two s (every row / operand scale of the split-f16 arithmetic is one, 2^-114 .. 2^114): exponent arithmetic, exact -- the IEEE
// division the compiler emits for `1.0f / s` is ~10 VALU instructions (v_div_scale x 2, v_rcp, 4 fma, v_div_fmas, v_div_fixup) per row and tile
__device__ __forceinline__ float cnr_pow2_rcp(float s) { return __uint_as_float(0x7f000000u - __float_as_uint(s)); }
// max over the 16 lanes of a DPP row (every lane gets it) by four data-parallel-primitive moves (quad_perm xor 1, xor 2, row_half_mirror, row_mirror)
// instead of four __shfl_xor(.., 16), which hipcc lowers to ds_bpermute_b32: an LDS-crossbar round trip each, on the path between a tile's
// arrival and its f16 planes.  max is associative and commutative: bit-identical to the shuffle form.
__device__ __forceinline__ float cnr_max16(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  int v = __float_as_int(x);
  x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false))); v = __float_as_int(x);
  x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false))); v = __float_as_int(x);
  x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false))); v = __float_as_int(x);
  x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false)));
#endif
  return x;
}
// Cross-half and cross-row exchanges as VALU ops (gfx950: v_permlane32_swap_b32 / v_permlane16_swap_b32) instead of __shfl_xor(.., 32) / (.., 16), which hipcc
// lowers to ds_bpermute_b32 (an LDS-crossbar round trip each, and an s_waitcnt on the LDS counter in the middle of an epilogue).  permlane32_swap(x, x) returns
// {(lo, lo), (hi, hi)} (lanes 0-31 | 32-63), permlane16_swap(x, x) {(r0, r0, r2, r2), (r1, r1, r3, r3)} (16-lane rows): the two results hold this lane's value and
// its partner's, so max / min / sum of the pair are one more VALU op -- the same numbers as with the shuffle (max, min exact; a + b commutative).
__device__ __forceinline__ float cnr_pair32_max(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned u = __float_as_uint(x);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  x = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
#endif
  return x;
}
__device__ __forceinline__ float cnr_pair32_sum(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned u = __float_as_uint(x);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  x = __uint_as_float(r[0]) + __uint_as_float(r[1]);
#endif
  return x;
}
__device__ __forceinline__ int cnr_pair32_min(int x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto r = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
  const int a = (int)r[0], b = (int)r[1];
  x = a < b ? a : b;
#endif
  return x;
}
__device__ __forceinline__ int cnr_pair16_min(int x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto r = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);
  const int a = (int)r[0], b = (int)r[1];
  x = a < b ? a : b;
#endif
  return x;
}
// max over the 8 lanes of a half DPP row / min over the 16 lanes of a DPP row by DPP moves (see cnr_max16), and the pair exchanges of two values at once
__device__ __forceinline__ float cnr_max8(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  int v = __float_as_int(x);
  x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false))); v = __float_as_int(x);
  x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false))); v = __float_as_int(x);
  x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false)));
#endif
  return x;
}
__device__ __forceinline__ int cnr_min16(int x) {
#if defined(__HIP_DEVICE_COMPILE__)
  int o;
  o = __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xf, 0xf, false); x = o < x ? o : x;
  o = __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xf, 0xf, false); x = o < x ? o : x;
  o = __builtin_amdgcn_update_dpp(x, x, 0x141, 0xf, 0xf, false); x = o < x ? o : x;
  o = __builtin_amdgcn_update_dpp(x, x, 0x140, 0xf, 0xf, false); x = o < x ? o : x;
#endif
  return x;
}
__device__ __forceinline__ int cnr_ror8_min(int x) {   // min with the lane 8 further in the 16-lane row (lane ^ 8)
#if defined(__HIP_DEVICE_COMPILE__)
  const int o = __builtin_amdgcn_update_dpp(x, x, 0x128, 0xf, 0xf, false);
  x = o < x ? o : x;
#endif
  return x;
}
#define CNR_LAUNCH_CHECK(where)                                   \
  do {                                                            \
    hipError_t e_ = hipGetLastError();                            \
    if (e_ != hipSuccess && cnr::g_first_error == hipSuccess) {   \
      cnr::g_first_error = e_;                                    \
      cnr::g_first_error_where = where;                           \
    }                                                             \
  } while (0)

// The one point-wise launch: a row X(name, parameter struct, body, element count) of a point-wise table (CNR_POINTWISE_KERNELS in cnr_bodies.h,
// CNR_RAYS_KERNELS, CNR_CAMERA_KERNELS, CNR_BG_KERNELS in their family headers) becomes the grid-stride kernel over the body and be_<name>, which
// launches it on the row's element count.  Expanded inside namespace cnr by the unit that holds the table's kernels.
#define CNR_PW_KERNEL(NAME, PARAM, BODY, COUNT)                                              \
  __global__ __launch_bounds__(256) void NAME##_kernel(const PARAM p, long n) {              \
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)   \
      BODY(p, i);                                                                            \
  }                                                                                          \
  void be_##NAME(const PARAM& p, cnr_stream s) {                                             \
    const long n = (COUNT);                                                                  \
    if (n <= 0) return;                                                                      \
    long blocks = (n + 255) / 256;                                                           \
    if (blocks > 8192) blocks = 8192;                                                        \
    TimingScope ts_(#NAME, 2, 0, n, 0, 0, 0, s);                                             \
    hipLaunchKernelGGL(NAME##_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p, n);        \
    CNR_LAUNCH_CHECK(#NAME);                                                                 \
  }

namespace cnr {
// Batched row jobs: ONE launch works through the rows of up to CAP small jobs (a model's layers: each on its own is a latency-bound launch of a few
// microseconds).  Workgroup b works on row b - start[i] of job i, the job whose row range [start[i], start[i + 1]) holds b; the batch travels as the
// kernel's argument block.
template <class JobT, int CAP>
struct RowBatch {
  using Job = JobT;
  static constexpr int kCap = CAP;
  int count; int start[CAP + 1]; Job job[CAP];
  struct At { const Job& job; int row; };
  __device__ __forceinline__ At locate(int block) const {
    const RowBatch& b = *this;
    int i = 0;
    while (i + 1 < b.count && block >= b.start[i + 1]) ++i;
    return {b.job[i], block - b.start[i]};
  }
};
// cuts the job list into batches of Batch::kCap and launches `kernel` (one workgroup of `threads` per row, rows_of(job) rows per job) once per batch,
// each launch under the record `name` with its row count
template <class Batch, class Rows>
void launch_row_batches(void (*kernel)(const Batch), const char* name, const typename Batch::Job* jobs, int count, int threads, hipStream_t s, Rows rows_of) {
  static_assert(sizeof(Batch) <= 4096, "kernel argument block");
  for (int i0 = 0; i0 < count; i0 += Batch::kCap) {
    Batch b;
    b.count = count - i0 < Batch::kCap ? count - i0 : Batch::kCap;
    int rows = 0;
    for (int i = 0; i < b.count; ++i) { b.start[i] = rows; b.job[i] = jobs[i0 + i]; rows += rows_of(jobs[i0 + i]); }
    b.start[b.count] = rows;
    TimingScope ts_(name, 2, 0, rows, 0, 0, 0, s);
    hipLaunchKernelGGL(kernel, dim3(rows), dim3(threads), 0, s, b);
  }
  CNR_LAUNCH_CHECK(name);
}
}  // namespace cnr
