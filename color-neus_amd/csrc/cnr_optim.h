// Per-parameter gradient clip + Adam (cnr_clip_adam): descriptors, the launch, and the per-tensor arithmetic both builds share.
#pragma once
#include "cnr_common.h"

namespace cnr {

// per-parameter gradient clip + Adam over up to kAdamBatch tensors per launch (clip_gradient + torch.optim.Adam, net_utils.py:174-184, :88)
constexpr int kAdamBatch = 64;
constexpr int kAdamChunk = 4096;   // elements per workgroup: a tensor is cut into ceil(n / kAdamChunk) chunks
struct AdamTensor { float* w; const float* g; long off; long n; int chunk0; };   // off: offset of this tensor's moments in the flat m / v buffers; chunk0: its first chunk
struct AdamArgs {
  int count; AdamTensor t[kAdamBatch];
  int nchunks; float* partial;         // [nchunks] per-chunk sums of squared gradient entries (scratch)
  float* m; float* v;                  // flat exp_avg / exp_avg_sq
  float lr, beta1, beta2, eps, max_norm;   // max_norm <= 0: no clipping
  float bc1, bc2_sqrt;                 // 1 - beta1^step, sqrt(1 - beta2^step)
  const float* hyper;                  // device [3] = {lr, bc1, bc2_sqrt} or null: read instead of the three members above (graph replay)
};
// one tensor's update; norm2 = the tensor's sum of squared gradient entries (fixed-order reduction by the caller)
CNR_HD float adam_clip_coef(float norm2, float max_norm) {
  if (!(max_norm > 0.0f)) return 1.0f;
  const float c = max_norm / (sqrtf(norm2) + 1e-6f);    // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
  return c < 1.0f ? c : 1.0f;
}
CNR_HD void adam_update1(const AdamArgs& a, float* w, float g, float* m, float* v) {
  const float m1 = *m + (g - *m) * (1.0f - a.beta1);               // exp_avg.lerp_(grad, 1 - beta1)
  const float v1 = *v * a.beta2 + (1.0f - a.beta2) * g * g;        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
  *m = m1; *v = v1;
  const float lr = a.hyper ? a.hyper[0] : a.lr, bc1 = a.hyper ? a.hyper[1] : a.bc1, bc2_sqrt = a.hyper ? a.hyper[2] : a.bc2_sqrt;
  const float denom = sqrtf(v1) / bc2_sqrt + a.eps;
  *w = *w - (lr / bc1) * (m1 / denom);                         // param.addcdiv_(exp_avg, denom, value = -lr / bias_correction1)
}
void be_clip_adam(const AdamArgs& a, cnr_stream s);   // a.partial must hold a.nchunks floats

}  // namespace cnr
