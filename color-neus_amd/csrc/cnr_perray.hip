// The one-wavefront-per-ray kernels of the render path (4 rays per workgroup, ray state staged in LDS): the sampler (upsample / merge /
// sampler_step), the compositor and its backward, the early-termination compaction, and the ray gradients.  Per-sample arithmetic: cnr_raymath.h.
#include <hip/hip_runtime.h>

#include "cnr_backend.h"
#include "cnr_raymath.h"
#include "cnr_hip_util.h"
#include "cnr_wave.h"

namespace cnr {

// ================================================================================================
// per-ray kernels: one wavefront per ray, 4 rays per workgroup, ray state staged in LDS
// ================================================================================================
// ---- building blocks of the sampler kernels (merge_kernel, upsample_kernel, sampler_step_kernel): one wavefront works on one ray's rows
// in LDS.  None of them holds a barrier: every kernel places its own between the stages.
// slope of the sdf along the ray in every section -> cs
__device__ __forceinline__ void ray_section_slopes(const float* zs, const float* ss, int nsec, float* cs, int lane) {
  for (int i = lane; i < nsec; i += 64) cs[i] = upsample_slope(ss[i], ss[i + 1], zs[i], zs[i + 1]);
}
// section alpha of up_sample from the slopes cs and the radii rs -> as
__device__ __forceinline__ void ray_section_alphas(const float* zs, const float* ss, const float* cs, const float* rs, int nsec, float inv_s, float* as, int lane) {
  for (int i = lane; i < nsec; i += 64) {
    const float c = upsample_cos(i > 0 ? cs[i - 1] : 0.0f, cs[i], rs[i], rs[i + 1]);
    as[i] = upsample_alpha(ss[i], ss[i + 1], zs[i], zs[i + 1], c, inv_s);
  }
}
// as: section alphas -> weights = alpha * exclusive cumprod(1 - alpha + 1e-7), + 1e-5 (sample_pdf); given_w: as already holds the weights.
// Returns their sum
__device__ __forceinline__ float ray_pdf_weights(float* as, int nsec, bool given_w, int lane) {
  float carry = 1.0f, part = 0.0f;
  for (int base = 0; base < nsec; base += 64) {
    const int i = base + lane;
    const bool ok = i < nsec;
    const float a = ok ? as[i] : 0.0f;
    const float T = wave_excl_cumprod(ok ? 1.0f - a + 1e-7f : 1.0f, lane, carry);
    const float w = (given_w ? a : a * T) + 1e-5f;
    if (ok) { as[i] = w; part += w; }
  }
  return wave_sum(part);
}
// cdf of the weights as (nsec + 1 entries, cdf[0] = 0) -> cs
__device__ __forceinline__ void ray_cdf(const float* as, float total, int nsec, float* cs, int lane) {
  float csum = 0.0f;
  for (int base = 0; base < nsec; base += 64) {
    const int i = base + lane;
    const bool ok = i < nsec;
    const float pdf = ok ? as[i] / total : 0.0f;
    const float incl = wave_scan_incl_add(pdf, lane);
    if (ok) cs[i + 1] = csum + incl;
    csum = csum + __shfl(incl, 63);
  }
  if (lane == 0) cs[0] = 0.0f;
}

__global__ __launch_bounds__(256) void upsample_kernel(const UpSample p) {
  __shared__ float sh[4][5][kMaxRaySamples];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long ray = (long)blockIdx.x * 4 + wave;
  const bool active = ray < p.R;
  if (!active) ray = p.R - 1;
  float* zs = sh[wave][0]; float* ss = sh[wave][1]; float* cs = sh[wave][2]; float* rs = sh[wave][3]; float* as = sh[wave][4];
  const int n = p.n, nsec = p.n - 1;
  const bool given_w = p.w_in != nullptr;   // wave-uniform
  if (given_w) {
    for (int i = lane; i < n; i += 64) zs[i] = p.z[ray * p.ldz + i];
    for (int i = lane; i < nsec; i += 64) as[i] = p.w_in[ray * nsec + i];
  } else {
    float o[3], d[3];
    for (int c = 0; c < 3; ++c) { o[c] = p.o[ray * 3 + c]; d[c] = p.d[ray * 3 + c]; }
    for (int i = lane; i < n; i += 64) {
      float z = p.z[ray * p.ldz + i];
      zs[i] = z;
      ss[i] = p.sdf[ray * p.lds + i];
      rs[i] = ray_radius(o, d, z);
    }
  }
  __syncthreads();
  if (!given_w) ray_section_slopes(zs, ss, nsec, cs, lane);
  __syncthreads();
  if (!given_w) ray_section_alphas(zs, ss, cs, rs, nsec, p.inv_s, as, lane);
  __syncthreads();
  const float total = ray_pdf_weights(as, nsec, given_w, lane);
  __syncthreads();
  ray_cdf(as, total, nsec, cs, lane);
  __syncthreads();
  if (lane < p.m && active) {
    const float u = p.u_in ? p.u_in[ray * p.m + lane] : linspace_at(0.5f / (float)p.m, 1.0f - 0.5f / (float)p.m, p.m, lane);
    p.new_z[ray * p.m + lane] = invert_cdf(cs, zs, n, u);
  }
}
void be_upsample(const UpSample& p, cnr_stream s) {
  // algorithmic bytes per ray: z and sdf (or the given weights) in, o / d, the new positions out
  TimingScope ts_("upsample", 2, 0, p.R, 0, 0, 0, s, (double)p.R * (4.0 * p.n + 4.0 * (p.w_in ? p.n - 1 : p.n) + (p.w_in ? 0.0 : 24.0) + 4.0 * p.m));
  hipLaunchKernelGGL(upsample_kernel, dim3((unsigned)((p.R + 3) / 4)), dim3(256), 0, s, p);
  CNR_LAUNCH_CHECK("upsample");
}

__global__ __launch_bounds__(256) void merge_kernel(const MergeZ p) {
  __shared__ float sh[4][2][kMaxRaySamples];
  __shared__ float shn[4][2][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long ray = (long)blockIdx.x * 4 + wave;
  const bool active = ray < p.R;
  if (!active) ray = p.R - 1;
  float* zs = sh[wave][0]; float* ss = sh[wave][1]; float* nz = shn[wave][0]; float* ns = shn[wave][1];
  const bool with_sdf = p.new_sdf != nullptr;
  for (int i = lane; i < p.n; i += 64) { zs[i] = p.z[ray * p.ldz + i]; ss[i] = with_sdf ? p.sdf_in[ray * p.lds_in + i] : 0.0f; }
  for (int j = lane; j < p.m; j += 64) { nz[j] = p.new_z[ray * p.m + j]; ns[j] = with_sdf ? p.new_sdf[ray * p.m + j] : 0.0f; }
  __syncthreads();
  if (active)
    merge_samples(zs, ss, p.n, nz, ns, p.m, lane, 64, [&](int at, float z, float s) {
      p.z[ray * p.ldz + at] = z;
      if (with_sdf) p.sdf_out[ray * p.lds_out + at] = s;
    });
}
// merge (previous iteration) + up_sample + embedding of the new samples for one ray per wavefront: the stages of merge_kernel and
// upsample_kernel and the EmbedZ rows, with the merged row handed over in LDS instead of through three launches
__global__ __launch_bounds__(256) void sampler_step_kernel(const SamplerStep p) {
  __shared__ float sh[4][7][kMaxRaySamples];
  __shared__ float shn[4][2][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long ray = (long)blockIdx.x * 4 + wave;
  const bool active = ray < p.u.R;
  if (!active) ray = p.u.R - 1;
  float* zs = sh[wave][0]; float* ss = sh[wave][1]; float* cs = sh[wave][2]; float* rs = sh[wave][3]; float* as = sh[wave][4];
  float* zo = sh[wave][5]; float* so = sh[wave][6]; float* nz = shn[wave][0]; float* ns = shn[wave][1];
  const UpSample& u = p.u;
  const int n = u.n, nsec = u.n - 1;
  float o[3], d[3];
  for (int c = 0; c < 3; ++c) { o[c] = u.o[ray * 3 + c]; d[c] = u.d[ray * 3 + c]; }
  if (p.do_merge) {
    const MergeZ& g = p.g;   // (with new_sdf: the fused form is only used between two up-sampling iterations)
    for (int i = lane; i < g.n; i += 64) { zo[i] = g.z[ray * g.ldz + i]; so[i] = g.sdf_in[ray * g.lds_in + i]; }
    for (int j = lane; j < g.m; j += 64) { nz[j] = g.new_z[ray * g.m + j]; ns[j] = g.new_sdf[ray * g.m + j]; }
    __syncthreads();
    merge_samples(zo, so, g.n, nz, ns, g.m, lane, 64, [&](int at, float z, float s) { zs[at] = z; ss[at] = s; });
    __syncthreads();
    if (active)
      for (int i = lane; i < n; i += 64) { g.z[ray * g.ldz + i] = zs[i]; g.sdf_out[ray * g.lds_out + i] = ss[i]; }
  } else {
    for (int i = lane; i < n; i += 64) { zs[i] = u.z[ray * u.ldz + i]; ss[i] = u.sdf[ray * u.lds + i]; }
    __syncthreads();
  }
  for (int i = lane; i < n; i += 64) rs[i] = ray_radius(o, d, zs[i]);
  __syncthreads();
  ray_section_slopes(zs, ss, nsec, cs, lane);
  __syncthreads();
  ray_section_alphas(zs, ss, cs, rs, nsec, u.inv_s, as, lane);
  __syncthreads();
  const float total = ray_pdf_weights(as, nsec, false, lane);
  __syncthreads();
  ray_cdf(as, total, nsec, cs, lane);
  __syncthreads();
  if (lane < u.m) {
    const float znew = invert_cdf(cs, zs, n, linspace_at(0.5f / (float)u.m, 1.0f - 0.5f / (float)u.m, u.m, lane));
    nz[lane] = znew;
    if (active) u.new_z[ray * u.m + lane] = znew;
  }
  if (p.do_embed) {
    __syncthreads();
    if (active) {
      // triples of the kEmb-wide rows of the u.m new samples (one contiguous piece of E): triple 0 = x, 1 + 2k = sin(2^k x), 2 + 2k = cos(2^k x)
      const int ntr = kEmb / 3;
      for (int idx = lane; idx < u.m * ntr; idx += 64) {
        const int j = idx / ntr, t = idx - j * ntr;
        const float z = nz[j];
        float v[3];
        const int k = t > 0 ? (t - 1) >> 1 : 0;
        const float f = (float)(1 << k);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float x = (o[c] + d[c] * z) * p.scale;
          float sn, cn;
          sincosf(x * f, &sn, &cn);
          v[c] = t == 0 ? x : (t <= 2 * p.multires ? ((t & 1) ? sn : cn) : 0.0f);
        }
        float* e = p.E + (ray * u.m + j) * kEmb + 3 * t;
        e[0] = v[0]; e[1] = v[1]; e[2] = v[2];
      }
    }
  }
}
void be_sampler_step(const SamplerStep& p, cnr_stream s) {
  TimingScope ts_("sampler_step", 2, 0, p.u.R, 0, 0, 0, s, (double)p.u.R * (8.0 * p.u.n + 24.0 + 4.0 * p.u.m + (p.do_embed ? 4.0 * kEmb * p.u.m : 0.0)));
  hipLaunchKernelGGL(sampler_step_kernel, dim3((unsigned)((p.u.R + 3) / 4)), dim3(256), 0, s, p);
  CNR_LAUNCH_CHECK("sampler_step");
}

void be_merge(const MergeZ& p, cnr_stream s) {
  TimingScope ts_("merge", 2, 0, p.R, 0, 0, 0, s, (double)p.R * (p.new_sdf ? 2.0 : 1.0) * (4.0 * p.n + 4.0 * p.m + 4.0 * (p.n + p.m)));
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)((p.R + 3) / 4)), dim3(256), 0, s, p);
  CNR_LAUNCH_CHECK("merge");
}

constexpr int kRayChunks = kMaxRaySamples / 64;

__global__ __launch_bounds__(256) void composite_fwd_kernel(const CompositeFwd p) {
  __shared__ float shz[4][kMaxRaySamples];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long ray = (long)blockIdx.x * 4 + wave;
  const bool active = ray < p.R;
  if (!active) ray = p.R - 1;
  float* zs = shz[wave];
  const int M = p.M;
  for (int i = lane; i < M; i += 64) zs[i] = p.z[ray * M + i];
  __syncthreads();
  float o[3], d[3];
  for (int c = 0; c < 3; ++c) { o[c] = p.o[ray * 3 + c]; d[c] = p.d[ray * 3 + c]; }
  const float inv_s = inv_s_of(p.variance[0]);

  float carry = 1.0f;
  float wsum = 0.f, wmax = -1.f, dep = 0.f, col[3] = {0.f, 0.f, 0.f}, gcl[3] = {0.f, 0.f, 0.f}, e0 = 0.f, e1 = 0.f, drs = 0.f;
#pragma unroll
  for (int c = 0; c < kRayChunks; ++c) {
    if (c * 64 < M) {
      const int j = c * 64 + lane;
      const long pt = ray * M + j;
      if (p.delta && j < M) drs += (p.delta[pt * 3] + p.delta[pt * 3 + 1]) + p.delta[pt * 3 + 2];
      RaySample q = ray_sample(zs, j, M, p.sample_dist, o, d, p.sdf, p.g, pt, inv_s, p.cos_anneal);
      const float T = wave_excl_cumprod(q.ok ? 1.0f - q.a.alpha + 1e-7f : 1.0f, lane, carry);
      const float w = q.ok ? q.a.alpha * T : 0.0f;
      if (q.ok) {
        wsum += w; wmax = fmaxf(wmax, w); dep += w * q.z;
        if (p.color) for (int k = 0; k < 3; ++k) col[k] += w * p.color[pt * p.ldcolor + k];   // (null: the weights-only pass in front of the compaction)
        if (p.gcolor) for (int k = 0; k < 3; ++k) gcl[k] += w * p.gcolor[pt * p.ldg + k];
        e0 += q.relax * (q.gn - 1.0f) * (q.gn - 1.0f);
        e1 += q.relax;
        if (active) {
          p.weights[pt] = w;
          p.cdf_fine[pt] = q.a.pc;
          p.inside_sphere[pt] = q.inside;
          if (p.sdf_s) p.sdf_s[pt] = p.sdf[pt];
          if (p.color_s && p.color) for (int k = 0; k < 3; ++k) p.color_s[pt * 3 + k] = p.color[pt * p.ldcolor + k];
          if (p.gcolor_s && p.gcolor) for (int k = 0; k < 3; ++k) p.gcolor_s[pt * 3 + k] = p.gcolor[pt * p.ldg + k];
        }
      }
    }
  }
  wsum = wave_sum(wsum); wmax = wave_max(wmax); dep = wave_sum(dep);
  for (int k = 0; k < 3; ++k) { col[k] = wave_sum(col[k]); gcl[k] = wave_sum(gcl[k]); }
  e0 = wave_sum(e0); e1 = wave_sum(e1);
  if (p.delta_ray_sum) { drs = wave_sum(drs); if (lane == 0 && active) p.delta_ray_sum[ray] = drs; }
  if (lane == 0 && active) {
    for (int k = 0; k < 3; ++k) {
      float cc = col[k];
      if (p.background_rgb) cc = cc + p.background_rgb[k] * (1.0f - wsum);
      p.color_fine[ray * 3 + k] = cc;
      if (p.global_color) p.global_color[ray * 3 + k] = gcl[k];
    }
    p.weight_sum[ray] = wsum; p.weight_max[ray] = wmax; p.depth[ray] = dep;
    p.s_val[ray] = 1.0f / inv_s;
    p.eik_partial[ray * 2] = e0; p.eik_partial[ray * 2 + 1] = e1;
  }
}
void be_composite_fwd(const CompositeFwd& p, cnr_stream s) {
  // algorithmic bytes per ray: z, sdf, gradients, colour(s) in; cdf, weights, inside_sphere and the per-ray outputs out
  TimingScope ts_("composite_fwd", 2, 0, p.R, 0, 0, 0, s,
                  (double)p.R * ((4.0 + 4.0 + 12.0 + 12.0 + (p.gcolor ? 12.0 : 0.0)) * p.M + 24.0 + 12.0 * p.M + 52.0));
  hipLaunchKernelGGL(composite_fwd_kernel, dim3((unsigned)((p.R + 3) / 4)), dim3(256), 0, s, p);
  CNR_LAUNCH_CHECK("composite_fwd");
}

__global__ __launch_bounds__(256) void composite_bwd_kernel(const CompositeBwd p) {
  __shared__ float shz[4][kMaxRaySamples];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long ray = (long)blockIdx.x * 4 + wave;
  const bool active = ray < p.R;
  if (!active) ray = p.R - 1;
  float* zs = shz[wave];
  const int M = p.M;
  for (int i = lane; i < M; i += 64) zs[i] = p.z[ray * M + i];
  __syncthreads();
  float o[3], d[3];
  for (int c = 0; c < 3; ++c) { o[c] = p.o[ray * 3 + c]; d[c] = p.d[ray * 3 + c]; }
  const float inv_s = inv_s_of(p.variance[0]);

  RaySample q[kRayChunks];
  float T[kRayChunks], w[kRayChunks];
  float carry = 1.0f, wsum = 0.0f, wmax = -1.0f;
#pragma unroll
  for (int c = 0; c < kRayChunks; ++c) {
    T[c] = 0.f; w[c] = 0.f;
    if (c * 64 < M) {
      const int j = c * 64 + lane;
      q[c] = ray_sample(zs, j, M, p.sample_dist, o, d, p.sdf, p.g, ray * M + j, inv_s, p.cos_anneal);
      T[c] = wave_excl_cumprod(q[c].ok ? 1.0f - q[c].a.alpha + 1e-7f : 1.0f, lane, carry);
      w[c] = q[c].ok ? q[c].a.alpha * T[c] : 0.0f;
      wsum += w[c];
      if (q[c].ok) wmax = fmaxf(wmax, w[c]);
    }
  }
  wsum = wave_sum(wsum);
  wmax = wave_max(wmax);
  int amax = 1 << 30;
#pragma unroll
  for (int c = 0; c < kRayChunks; ++c)
    if (c * 64 < M && q[c].ok && w[c] == wmax && c * 64 + lane < amax) amax = c * 64 + lane;
  amax = wave_min_int(amax);

  const RayUpstream up = ray_upstream(p, ray);

  // d loss / d w_j and the suffix sums S_j = sum_{k>j} wbar_k w_k (reverse scan, chunks from the back)
  float wbar[kRayChunks], S[kRayChunks];
  float rcarry = 0.0f;
#pragma unroll
  for (int c = kRayChunks - 1; c >= 0; --c) {
    wbar[c] = 0.f; S[c] = 0.f;
    if (c * 64 < M) {
      const int j = c * 64 + lane;
      const long pt = ray * M + j;
      wbar[c] = q[c].ok ? sample_wbar(p, up, pt, q[c].z, j == amax) : 0.0f;
      const float x = wbar[c] * w[c];
      const float incl = wave_scan_incl_add_rev(x, lane);
      S[c] = rcarry + (incl - x);
      rcarry = rcarry + __shfl(incl, 0);
    }
  }

  float dinvs = 0.0f, drd[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < kRayChunks; ++c) {
    if (c * 64 < M) {
      const int j = c * 64 + lane;
      const long pt = ray * M + j;
      if (q[c].ok) dinvs += sample_backward(p, up, q[c], d, pt, inv_s, T[c], w[c], wbar[c], S[c], active, drd);
    }
  }
  dinvs = wave_sum(dinvs);
  for (int k = 0; k < 3; ++k) drd[k] = wave_sum(drd[k]);
  if (lane == 0 && active) {
    if (p.d_s_val) dinvs += -p.d_s_val[ray] / (inv_s * inv_s);
    p.dinvs_partial[ray] = dinvs;
    if (p.d_rays_d) for (int k = 0; k < 3; ++k) p.d_rays_d[ray * 3 + k] = drd[k];
  }
}
void be_composite_bwd(const CompositeBwd& p, cnr_stream s) {
  // algorithmic bytes per ray: the forward inputs again, the upstream gradients, and per sample d sdf (4), d g (12), the colour /
  // relight cotangents (12 + 12) -- the buffers themselves are padded to the 16-float rows the narrow GEMMs read
  TimingScope ts_("composite_bwd", 2, 0, p.R, 0, 0, 0, s,
                  (double)p.R * ((4.0 + 4.0 + 12.0 + 12.0 + (p.gcolor ? 12.0 : 0.0)) * p.M + 24.0 + (p.d_delta_relight ? 12.0 * p.M : 0.0) + 32.0 +
                                 (4.0 + 12.0 + 12.0 + (p.has_relight ? 12.0 : 0.0)) * p.M + 16.0));
  hipLaunchKernelGGL(composite_bwd_kernel, dim3((unsigned)((p.R + 3) / 4)), dim3(256), 0, s, p);
  CNR_LAUNCH_CHECK("composite_bwd");
}

// ------------------------------------------------------------------------------------------------
// early-termination compaction (inference): wavefront ballot + popcount prefix per ray
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prune_count_kernel(const PruneCount p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long ray = (long)blockIdx.x * 4 + wave;
  if (ray >= p.R) return;
  int cnt = 0;
  for (int base = 0; base < p.M; base += 64) {
    const int j = base + lane;
    const bool keep = j < p.M && prune_keep(p.weights[ray * p.M + j], p.eps);
    cnt += __popcll(__ballot(keep));
  }
  if (lane == 0) p.counts[ray] = cnt;
}
void be_prune_count(const PruneCount& p, cnr_stream s) {
  TimingScope ts_("prune_count", 2, 0, p.R, 0, 0, 0, s);
  hipLaunchKernelGGL(prune_count_kernel, dim3((unsigned)((p.R + 3) / 4)), dim3(256), 0, s, p);
  CNR_LAUNCH_CHECK("prune_count");
}

// exclusive scan of the per-ray counts (one workgroup; R is a few thousand)
__global__ __launch_bounds__(1024) void prune_scan_kernel(const PruneScan p) {
  __shared__ int wsum[1][16];
  __shared__ int carry[1];
  block_carried_scan<16, 1, 1, int>(p.R, wsum, carry,
                                    [&](long i, int (&x)[1]) { x[0] += p.counts[i]; },
                                    [&](long i, const int (&at)[1]) { p.offsets[i] = at[0]; });
  if (threadIdx.x == 0) p.offsets[p.R] = carry[0];
}
void be_prune_scan(const PruneScan& p, cnr_stream s) {
  TimingScope ts_("prune_scan", 2, 0, p.R, 0, 0, 0, s);
  hipLaunchKernelGGL(prune_scan_kernel, dim3(1), dim3(1024), 0, s, p);
  CNR_LAUNCH_CHECK("prune_scan");
}

__global__ __launch_bounds__(256) void prune_gather_kernel(const PruneGather p) {
  __shared__ int list[4][kMaxRaySamples];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long ray = (long)blockIdx.x * 4 + wave;
  if (ray >= p.R) return;
  int carry = 0;
  for (int base = 0; base < p.M; base += 64) {
    const int j = base + lane;
    const bool keep = j < p.M && prune_keep(p.weights[ray * p.M + j], p.eps);
    const unsigned long long mask = __ballot(keep);
    const int pos = carry + __popcll(mask & ((1ull << lane) - 1ull));
    if (keep) list[wave][pos] = j;
    carry += __popcll(mask);
    if (j < p.M && !keep) prune_zero_dropped(p, ray * p.M + j);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int off = p.offsets[ray];
  for (int k = lane; k < carry; k += 64) p.idx[off + k] = (int)(ray * p.M + list[wave][k]);
  if (p.featx_c == nullptr) return;
  const int nf4 = p.ldfx / 4;
  for (int k = 0; k < carry; ++k) {
    const long src = ray * p.M + list[wave][k];
    const long dst = off + k;
    for (int c = lane; c < nf4; c += 64)
      reinterpret_cast<f4*>(p.featx_c + dst * p.ldfx)[c] = reinterpret_cast<const f4*>(p.featx + src * p.ldfx)[c];
    if (lane < kAux / 4) reinterpret_cast<f4*>(p.aux_c + dst * kAux)[lane] = reinterpret_cast<const f4*>(p.aux + src * kAux)[lane];
  }
}
void be_prune_gather(const PruneGather& p, cnr_stream s) {
  TimingScope ts_("prune_gather", 2, 0, p.R, 0, 0, 0, s);
  hipLaunchKernelGGL(prune_gather_kernel, dim3((unsigned)((p.R + 3) / 4)), dim3(256), 0, s, p);
  CNR_LAUNCH_CHECK("prune_gather");
}

__global__ __launch_bounds__(256) void prune_scatter_kernel(const PruneScatter p) {
  const long n = *p.count;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long pt = p.idx[i];
    reinterpret_cast<f4*>(p.gcol)[pt] = reinterpret_cast<const f4*>(p.gcol_c)[i];
    if (p.relit) reinterpret_cast<f4*>(p.relit)[pt] = reinterpret_cast<const f4*>(p.relit_c)[i];
    if (p.delta) for (int c = 0; c < 3; ++c) p.delta[pt * 3 + c] = p.delta_c[i * 3 + c];
  }
}
void be_prune_scatter(const PruneScatter& p, cnr_stream s) {
  long blocks = (p.P + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  TimingScope ts_("prune_scatter", 2, 0, p.P, 0, 0, 0, s);
  hipLaunchKernelGGL(prune_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
  CNR_LAUNCH_CHECK("prune_scatter");
}

// d rays: one wavefront per ray
__global__ __launch_bounds__(256) void rays_grad_finish_kernel(const RaysGradFinish p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long ray = (long)blockIdx.x * 4 + wave;
  if (ray >= p.R) return;
  const int M = p.M;
  float so[3] = {0.f, 0.f, 0.f}, sd[3] = {0.f, 0.f, 0.f};
  const int npe = p.multires_view > 0 ? 3 + 6 * p.multires_view : 3;
  float spe[27];
  for (int q = 0; q < 27; ++q) spe[q] = 0.0f;
  float dr[3];
  for (int k = 0; k < 3; ++k) dr[k] = p.d[ray * 3 + k];
  float snear = 0.0f, sfar = 0.0f;
  for (int j = lane; j < M; j += 64) {
    const long pt = ray * M + j;
    const float z0 = p.z[pt];
    const float dist = j + 1 < M ? p.z[pt + 1] - z0 : p.sample_dist;
    const float mid = z0 + dist * 0.5f;
    float dmid = 0.0f;
    for (int k = 0; k < 3; ++k) { float pb = p.pbar[pt * 4 + k]; so[k] += pb; sd[k] += pb * mid; dmid += pb * dr[k]; }
    for (int q = 0; q < npe; ++q) {
      float v = 0.0f;
      if (p.daux_dir_c) v += p.daux_dir_c[pt * p.lddir + 6 + q];
      if (p.daux_dir_r) v += p.daux_dir_r[pt * p.lddir + 6 + q];
      spe[q] += v;
    }
    if (p.dz_parts) {
      // mid_j = z_j + dist_j / 2, dist_j = z_{j+1} - z_j (the last section has the constant length 2/S): total cotangent of z_j
      float dz = p.dz_parts[pt * 2] + dmid;
      if (j + 1 < M) dz -= p.dz_parts[pt * 2 + 1] + 0.5f * dmid;
      if (j > 0) {
        float dmid_prev = 0.0f;
        for (int k = 0; k < 3; ++k) dmid_prev += p.pbar[(pt - 1) * 4 + k] * dr[k];
        dz += p.dz_parts[(pt - 1) * 2 + 1] + 0.5f * dmid_prev;
      }
      const float lin = linspace_at(0.0f, 1.0f, M, j);
      snear += dz * (1.0f - lin);
      sfar += dz * lin;
    }
  }
  for (int k = 0; k < 3; ++k) { so[k] = wave_sum(so[k]); sd[k] = wave_sum(sd[k]); }
  for (int q = 0; q < npe; ++q) spe[q] = wave_sum(spe[q]);
  snear = wave_sum(snear); sfar = wave_sum(sfar);
  if (lane == 0) {
    if (p.d_o && p.d_d)
      for (int k = 0; k < 3; ++k) {
        p.d_d[ray * 3 + k] = rays_d_grad(dr[k], sd[k], p.d_rays_d_alpha[ray * 3 + k], spe, k, p.multires_view);
        p.d_o[ray * 3 + k] = so[k];
      }
    if (p.dz_parts && p.d_near && p.d_far) { p.d_near[ray] = snear; p.d_far[ray] = sfar; }
  }
}
void be_rays_grad_finish(const RaysGradFinish& p, cnr_stream s) {
  TimingScope ts_("rays_grad_finish", 2, 0, p.R, 0, 0, 0, s);
  hipLaunchKernelGGL(rays_grad_finish_kernel, dim3((unsigned)((p.R + 3) / 4)), dim3(256), 0, s, p);
  CNR_LAUNCH_CHECK("rays_grad_finish");
}

}  // namespace cnr
