// Per-parameter gradient clip + Adam (cnr_clip_adam).
#include <hip/hip_runtime.h>

#include "cnr_optim.h"
#include "cnr_hip_util.h"
#include "cnr_wave.h"

namespace cnr {

// ------------------------------------------------------------------------------------------------
// per-parameter clip + Adam (53 tensors, 1 M floats): two launches over 4096-element chunks instead of ~150 torch launches.
//   1. per-chunk sum of squared gradient entries (fixed order inside a chunk);
//   2. every chunk's workgroup folds its OWN tensor's chunk sums in chunk order (<= 17 values) -> clip coefficient -> Adam update.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int adam_find_tensor(const AdamArgs& a, int chunk) {
  int lo = 0, hi = a.count - 1;     // last tensor whose first chunk is <= chunk (binary search: 6 dependent scalar loads, not 53)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.t[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__global__ __launch_bounds__(256) void clip_norm_kernel(const AdamArgs a) {
  __shared__ float red[4];
  const int chunk = blockIdx.x;
  const AdamTensor t = a.t[adam_find_tensor(a, chunk)];
  const long i0 = (long)(chunk - t.chunk0) * kAdamChunk;
  float ss = 0.0f;
  for (int j = threadIdx.x; j < kAdamChunk; j += 256) { const long i = i0 + j; if (i < t.n) { const float g = t.g[i]; ss += g * g; } }
  ss = block_sum_256(ss, red);
  if (threadIdx.x == 0) a.partial[chunk] = ss;
}
__global__ __launch_bounds__(256) void clip_adam_kernel(const AdamArgs a) {
  const int chunk = blockIdx.x;
  const AdamTensor t = a.t[adam_find_tensor(a, chunk)];
  float coef = 1.0f;
  if (a.max_norm > 0.0f) {
    // the tensor's chunk sums (<= 17 for the largest layer): one load per lane, folded in a fixed order that is the same in every
    // workgroup of the tensor (a serial loop of dependent loads costs one L2 round trip per chunk)
    __shared__ float coef_s;
    const int nch = (int)((t.n + kAdamChunk - 1) / kAdamChunk);
    if (threadIdx.x < 64) {
      float part = 0.0f;
      for (int c = threadIdx.x; c < nch; c += 64) part += a.partial[t.chunk0 + c];
      part = wave_sum(part);
      if (threadIdx.x == 0) coef_s = adam_clip_coef(part, a.max_norm);
    }
    __syncthreads();
    coef = coef_s;
  }
  const long i0 = (long)(chunk - t.chunk0) * kAdamChunk;
  for (int j = threadIdx.x; j < kAdamChunk; j += 256) {
    const long i = i0 + j;
    if (i < t.n) adam_update1(a, t.w + i, t.g[i] * coef, a.m + t.off + i, a.v + t.off + i);
  }
}
void be_clip_adam(const AdamArgs& a, cnr_stream s) {
  if (a.count <= 0 || a.nchunks <= 0) return;
  TimingScope ts_("clip_adam", 2, 0, a.count, 0, 0, 0, s);
  if (a.max_norm > 0.0f) hipLaunchKernelGGL(clip_norm_kernel, dim3(a.nchunks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(clip_adam_kernel, dim3(a.nchunks), dim3(256), 0, s, a);
  CNR_LAUNCH_CHECK("clip_adam");
}

}  // namespace cnr
