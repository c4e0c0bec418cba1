// Training loss (cnr_loss_*): block partial sums in a fixed order, one block folds the partials; gradients are element-wise.
#include <hip/hip_runtime.h>

#include "cnr_loss.h"
#include "cnr_hip_util.h"
#include "cnr_wave.h"

namespace cnr {

// ================================================================================================
// training loss: block partial sums in a fixed order, then one block folds the partials; gradients are element-wise
// ================================================================================================
__global__ __launch_bounds__(256) void loss_partial_kernel(const LossArgs a, float* partial) {
  __shared__ float red[4];
  const int tid = threadIdx.x, nb = gridDim.x, b = blockIdx.x;
  float s_rgb = 0.f, s_bce = 0.f, s_rel = 0.f;
  const long n_rgb = a.R * 3;
  for (long i = (long)b * 256 + tid; i < n_rgb; i += (long)nb * 256) s_rgb += loss_rgb_term(a.color[i], a.gt[i], a.rgb_l1);
  if (a.mask)
    for (long r = (long)b * 256 + tid; r < a.R; r += (long)nb * 256) s_bce += loss_bce_term(a.wsum[r], a.mask[r]);
  if (a.drel) {
    const long per_ray = a.drel_per_ray ? 1 : (long)a.M * 3, n_rel = a.R * per_ray;
    for (long i = (long)b * 256 + tid; i < n_rel; i += (long)nb * 256) {
      const float m = (a.include_mask && a.mask) ? a.mask[i / per_ray] : 1.0f;
      s_rel += a.drel[i] * m;
    }
  }
  s_rgb = block_sum_256(s_rgb, red);
  s_bce = block_sum_256(s_bce, red);
  s_rel = block_sum_256(s_rel, red);
  if (tid == 0) { partial[b * 4 + 0] = s_rgb; partial[b * 4 + 1] = s_bce; partial[b * 4 + 2] = s_rel; partial[b * 4 + 3] = 0.f; }
}
__global__ __launch_bounds__(256) void loss_fold_kernel(const float* partial, int nb, float* sums) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  float v[3] = {0.f, 0.f, 0.f};
  for (int b = tid; b < nb; b += 256) { v[0] += partial[b * 4]; v[1] += partial[b * 4 + 1]; v[2] += partial[b * 4 + 2]; }
  for (int j = 0; j < 3; ++j) { const float s = block_sum_256(v[j], red); if (tid == 0) sums[j] = s; }
  if (tid == 0) sums[3] = 0.f;
}
void be_loss_sums(const LossArgs& a, float* partial, float* sums, cnr_stream s) {
  TimingScope ts_("loss_sums", 2, 0, a.R, 0, 0, 0, s);
  hipLaunchKernelGGL(loss_partial_kernel, dim3(kLossBlocks), dim3(256), 0, s, a, partial);
  hipLaunchKernelGGL(loss_fold_kernel, dim3(1), dim3(256), 0, s, partial, kLossBlocks, sums);
  CNR_LAUNCH_CHECK("loss_sums");
}
// The whole forward side in ONE launch: every block writes its partial sums, takes a ticket, and the block that draws the last one folds all
// partials in the fixed order of loss_fold_kernel and runs the scalar tail (loss_combine).  Which block is last does not matter: bitwise the same
// sums as the two-launch form.  The ticket counter is a 4-byte slot of the CALLER's scratch (zero before the first use of the buffer; the last
// block leaves it zero): calls on one stream may share a buffer, calls that may overlap (other streams, other threads) bring their own.
// The last block also clears the partial sums it has folded, so an all-zero scratch is all zero again after the call.
// shard != 0 (ray-sharded runs): no scalar tail; the last block writes the rank's statistics for the all-reduce instead:
// stats[0..2] = the three sums, stats[3..4] = the rank's eikonal sums, stats[5] = a second copy of stats[4] that the all-reduce leaves alone.
__global__ __launch_bounds__(256) void loss_forward_kernel(const LossArgs a, float* partial, unsigned* ticket, const LossScalars c, const float* gerr, float* sums,
                                                           float* out6, const int shard, const float* eik_sums) {
  __shared__ float red[4];
  __shared__ int is_last;
  const int tid = threadIdx.x, nb = gridDim.x, b = blockIdx.x;
  float s_rgb = 0.f, s_bce = 0.f, s_rel = 0.f;
  const long n_rgb = a.R * 3;
  for (long i = (long)b * 256 + tid; i < n_rgb; i += (long)nb * 256) s_rgb += loss_rgb_term(a.color[i], a.gt[i], a.rgb_l1);
  if (a.mask)
    for (long r = (long)b * 256 + tid; r < a.R; r += (long)nb * 256) s_bce += loss_bce_term(a.wsum[r], a.mask[r]);
  if (a.drel) {
    const long per_ray = a.drel_per_ray ? 1 : (long)a.M * 3, n_rel = a.R * per_ray;
    for (long i = (long)b * 256 + tid; i < n_rel; i += (long)nb * 256) {
      const float m = (a.include_mask && a.mask) ? a.mask[i / per_ray] : 1.0f;
      s_rel += a.drel[i] * m;
    }
  }
  s_rgb = block_sum_256(s_rgb, red);
  s_bce = block_sum_256(s_bce, red);
  s_rel = block_sum_256(s_rel, red);
  if (tid == 0) {
    partial[b * 4 + 0] = s_rgb; partial[b * 4 + 1] = s_bce; partial[b * 4 + 2] = s_rel; partial[b * 4 + 3] = 0.f;
    __threadfence();                                               // the partials are visible device-wide before the ticket is drawn
    const unsigned t = atomicAdd(ticket, 1u);
    is_last = t == (unsigned)nb - 1u;
  }
  __syncthreads();
  if (!is_last) return;
  __threadfence();
  float v[3] = {0.f, 0.f, 0.f};
  for (int k = tid; k < nb; k += 256) {                            // (device-scope loads: other CUs wrote these)
    v[0] += __hip_atomic_load(partial + k * 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    v[1] += __hip_atomic_load(partial + k * 4 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    v[2] += __hip_atomic_load(partial + k * 4 + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    partial[k * 4] = 0.f; partial[k * 4 + 1] = 0.f; partial[k * 4 + 2] = 0.f;   // (slot 3 was written as 0: the scratch is left all zero)
  }
  __shared__ float tot[4];
  for (int j = 0; j < 3; ++j) { const float sj = block_sum_256(v[j], red); if (tid == 0) tot[j] = sj; }
  if (tid == 0) {
    tot[3] = 0.f;
    if (shard) {
      const float num = eik_sums[0], den = eik_sums[1];
      sums[0] = tot[0]; sums[1] = tot[1]; sums[2] = tot[2]; sums[3] = num; sums[4] = den; sums[5] = den; sums[6] = 0.f; sums[7] = 0.f;
    } else {
      sums[0] = tot[0]; sums[1] = tot[1]; sums[2] = tot[2]; sums[3] = 0.f;
      loss_combine(c, tot, gerr, out6);
    }
    *ticket = 0;
  }
}
void be_loss_forward(const LossArgs& a, float* partial, unsigned* ticket, const LossScalars& c, const float* gerr, float* sums, float* out6, cnr_stream s) {
  TimingScope ts_("loss_forward", 2, 0, a.R, 0, 0, 0, s);
  hipLaunchKernelGGL(loss_forward_kernel, dim3(kLossBlocks), dim3(256), 0, s, a, partial, ticket, c, gerr, sums, out6, 0, (const float*)nullptr);
  CNR_LAUNCH_CHECK("loss_forward");
}
void be_loss_shard_stats(const LossArgs& a, float* partial, unsigned* ticket, const float* eik_sums, float* stats8, cnr_stream s) {
  TimingScope ts_("loss_shard_stats", 2, 0, a.R, 0, 0, 0, s);
  hipLaunchKernelGGL(loss_forward_kernel, dim3(kLossBlocks), dim3(256), 0, s, a, partial, ticket, LossScalars{}, (const float*)nullptr, stats8, (float*)nullptr, 1, eik_sums);
  CNR_LAUNCH_CHECK("loss_shard_stats");
}
__global__ void loss_shard_combine_kernel(const LossScalars c, const float* stats, float* out8) { if (threadIdx.x == 0 && blockIdx.x == 0) loss_shard_combine(c, stats, out8); }
void be_loss_shard_combine(const LossScalars& c, const float* stats8, float* out8, cnr_stream s) {
  TimingScope ts_("loss_shard_combine", 2, 0, 1, 0, 0, 0, s);
  hipLaunchKernelGGL(loss_shard_combine_kernel, dim3(1), dim3(64), 0, s, c, stats8, out8);
  CNR_LAUNCH_CHECK("loss_shard_combine");
}
// ... and the backward side in one: every thread forms the coefficients from the upstream gradient itself (loss_coef: a dozen flops)
__global__ __launch_bounds__(256) void loss_backward_kernel(const LossArgs a, const LossScalars c, const float* g_loss, const float* mean_rel, const float* eik_factor,
                                                            float* coef_out, float* d_color, float* d_wsum, float* d_drel_ray) {
  float coef[4];
  loss_coef(c, g_loss, c.use_relight ? mean_rel : g_loss, eik_factor, coef);
  if (blockIdx.x == 0 && threadIdx.x == 0) { coef_out[0] = coef[0]; coef_out[1] = coef[1]; coef_out[2] = coef[2]; coef_out[3] = coef[3]; }
  const long n_rgb = a.R * 3;
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_rgb; i += stride) d_color[i] = coef[0] * loss_rgb_grad(a.color[i], a.gt[i], a.rgb_l1);
  if (d_wsum)
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < a.R; r += stride) d_wsum[r] = a.mask ? coef[1] * loss_bce_grad(a.wsum[r], a.mask[r]) : 0.0f;
  if (d_drel_ray)   // d mean(delta_relight * mask)^2 / d delta_relight[r][j][c]: one value per ray
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < a.R; r += stride) d_drel_ray[r] = (a.include_mask && a.mask) ? coef[2] * a.mask[r] : coef[2];
}
void be_loss_backward(const LossArgs& a, const LossScalars& c, const float* g_loss, const float* mean_rel, const float* eik_factor, float* coef4, float* d_color,
                      float* d_wsum, float* d_drel_ray, cnr_stream s) {
  TimingScope ts_("loss_backward", 2, 0, a.R, 0, 0, 0, s);
  long blocks = (a.R * 3 + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(loss_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, c, g_loss, mean_rel, eik_factor, coef4, d_color, d_wsum, d_drel_ray);
  CNR_LAUNCH_CHECK("loss_backward");
}
__global__ __launch_bounds__(256) void loss_grads_kernel(const LossArgs a, const float* coef, float* d_color, float* d_wsum, float* d_drel) {
  const float c_rgb = coef[0], c_bce = coef[1], c_rel = coef[2];
  const long n_rgb = a.R * 3, per_ray = (long)a.M * 3, n_rel = a.drel || d_drel ? a.R * per_ray : 0;
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_rgb; i += stride) d_color[i] = c_rgb * loss_rgb_grad(a.color[i], a.gt[i], a.rgb_l1);
  if (d_wsum)
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < a.R; r += stride) d_wsum[r] = a.mask ? c_bce * loss_bce_grad(a.wsum[r], a.mask[r]) : 0.0f;
  if (d_drel)
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_rel; i += stride) d_drel[i] = c_rel * ((a.include_mask && a.mask) ? a.mask[i / per_ray] : 1.0f);
}
__global__ void loss_combine_kernel(const LossScalars c, const float* sums, const float* gerr, float* out) { if (threadIdx.x == 0 && blockIdx.x == 0) loss_combine(c, sums, gerr, out); }
__global__ void loss_coef_kernel(const LossScalars c, const float* g_loss, const float* mean_rel, float* coef) { if (threadIdx.x == 0 && blockIdx.x == 0) loss_coef(c, g_loss, mean_rel, nullptr, coef); }
void be_loss_combine(const LossScalars& c, const float* sums, const float* gerr, float* out6, cnr_stream s) {
  hipLaunchKernelGGL(loss_combine_kernel, dim3(1), dim3(64), 0, s, c, sums, gerr, out6);
  CNR_LAUNCH_CHECK("loss_combine");
}
void be_loss_coef(const LossScalars& c, const float* g_loss, const float* mean_rel, float* coef4, cnr_stream s) {
  hipLaunchKernelGGL(loss_coef_kernel, dim3(1), dim3(64), 0, s, c, g_loss, mean_rel, coef4);
  CNR_LAUNCH_CHECK("loss_coef");
}
void be_loss_grads(const LossArgs& a, const float* coef, float* d_color, float* d_wsum, float* d_drel, cnr_stream s) {
  TimingScope ts_("loss_grads", 2, 0, a.R, 0, 0, 0, s);
  hipLaunchKernelGGL(loss_grads_kernel, dim3(1024), dim3(256), 0, s, a, coef, d_color, d_wsum, d_drel);
  CNR_LAUNCH_CHECK("loss_grads");
}

}  // namespace cnr
