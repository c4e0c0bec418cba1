// Per-sample math shared by the HIP per-ray kernels and their CPU-emulation twins.  What differs by nature stays with each backend: the
// HIP kernels scan and reduce across a wavefront, the emulation in sequential loops; everything a single sample computes is here.
// Formulas follow the reference (file:line cited per function); derivatives are hand-derived and
// checked against autograd of the oracle in tests/.
#pragma once
#include "cnr_backend.h"

namespace cnr {

// torch.linspace(start, end, steps)[i] in float32 (symmetric evaluation used by ATen's CPU/GPU kernels)
CNR_HD float linspace_at(float start, float end, int steps, int i) {
  if (steps <= 1) return start;
  float step = (end - start) / (float)(steps - 1);
  return i < steps / 2 ? start + step * (float)i : end - step * (float)(steps - 1 - i);
}

// positional encoding row: [x, sin(2^0 x), cos(2^0 x), ...]                (PositionEncoding.py:51-76)
CNR_HD void pe_row(const float x[3], int multires, float* out /* 3 + 6*multires */) {
  out[0] = x[0]; out[1] = x[1]; out[2] = x[2];
  float f = 1.0f;
  for (int k = 0; k < multires; ++k) {
    for (int c = 0; c < 3; ++c) {
      float a = x[c] * f, sn, cs;
      sincosf(a, &sn, &cs);   // (one argument reduction for the pair)
      out[3 + 6 * k + c] = sn;
      out[6 + 6 * k + c] = cs;
    }
    f *= 2.0f;
  }
}

// S-density alpha of one section                                  (Color_NeuS.py:69-90 / NeuS.py:236-256)
struct AlphaOut {
  float tc, ic, pe, ne, pc, nc, a_raw, alpha;
};
CNR_HD AlphaOut alpha_forward(float sdf, const float g[3], const float d[3], float dist, float inv_s, float r) {
  AlphaOut o;
  o.tc = d[0] * g[0] + d[1] * g[1] + d[2] * g[2];
  float A = fmaxf(-o.tc * 0.5f + 0.5f, 0.0f);
  float B = fmaxf(-o.tc, 0.0f);
  o.ic = -(A * (1.0f - r) + B * r);
  o.ne = sdf + o.ic * dist * 0.5f;
  o.pe = sdf - o.ic * dist * 0.5f;
  o.pc = sigmoidf_(o.pe * inv_s);
  o.nc = sigmoidf_(o.ne * inv_s);
  o.a_raw = (o.pc - o.nc + 1e-5f) / (o.pc + 1e-5f);
  o.alpha = fminf(fmaxf(o.a_raw, 0.0f), 1.0f);
  return o;
}

// reverse of alpha_forward: given d alpha and d prev_cdf (cdf_fine upstream) produce d sdf, d tc, d inv_s, d dist
struct AlphaGrad {
  float d_sdf, d_tc, d_inv_s, d_dist;
};
CNR_HD AlphaGrad alpha_backward(const AlphaOut& o, float dist, float inv_s, float r, float d_alpha, float d_pc_extra) {
  AlphaGrad gr;
  float da = (o.a_raw >= 0.0f && o.a_raw <= 1.0f) ? d_alpha : 0.0f;
  float den = o.pc + 1e-5f;
  float d_pc = da * (o.nc / (den * den)) + d_pc_extra;
  float d_nc = -da / den;
  float spc = o.pc * (1.0f - o.pc), snc = o.nc * (1.0f - o.nc);
  float d_pe = d_pc * spc * inv_s;
  float d_ne = d_nc * snc * inv_s;
  gr.d_inv_s = d_pc * spc * o.pe + d_nc * snc * o.ne;
  gr.d_sdf = d_pe + d_ne;
  float d_ic = (d_ne - d_pe) * dist * 0.5f;
  gr.d_dist = (d_ne - d_pe) * o.ic * 0.5f;
  float dic_dtc = (o.tc < 1.0f ? 0.5f * (1.0f - r) : 0.0f) + (o.tc < 0.0f ? r : 0.0f);
  gr.d_tc = d_ic * dic_dtc;
  return gr;
}

// The same pair in double, for the per-ray background compositor (N_OUTSIDE > 0: one thread per ray, speed is no concern there): the
// d inv_s terms of one ray cancel to a few percent of their size, so their float32 round-off would show in d variance.
struct AlphaOutD { double tc, ic, pe, ne, pc, nc, a_raw; };
CNR_HD AlphaOutD alpha_forward_d(double sdf, const float g[3], const float d[3], double dist, double inv_s, double r) {
  AlphaOutD o;
  o.tc = (double)d[0] * g[0] + (double)d[1] * g[1] + (double)d[2] * g[2];
  const double A = fmax(-o.tc * 0.5 + 0.5, 0.0), B = fmax(-o.tc, 0.0);
  o.ic = -(A * (1.0 - r) + B * r);
  o.ne = sdf + o.ic * dist * 0.5;
  o.pe = sdf - o.ic * dist * 0.5;
  o.pc = 1.0 / (1.0 + exp(-o.pe * inv_s));
  o.nc = 1.0 / (1.0 + exp(-o.ne * inv_s));
  o.a_raw = (o.pc - o.nc + 1e-5) / (o.pc + 1e-5);
  return o;
}
CNR_HD AlphaGrad alpha_backward_d(const AlphaOutD& o, double dist, double inv_s, double r, double d_alpha, double d_pc_extra, double* d_inv_s) {
  AlphaGrad gr;
  const double da = (o.a_raw >= 0.0 && o.a_raw <= 1.0) ? d_alpha : 0.0;
  const double den = o.pc + 1e-5;
  const double d_pc = da * (o.nc / (den * den)) + d_pc_extra, d_nc = -da / den;
  const double spc = o.pc * (1.0 - o.pc), snc = o.nc * (1.0 - o.nc);
  const double d_pe = d_pc * spc * inv_s, d_ne = d_nc * snc * inv_s;
  *d_inv_s = d_pc * spc * o.pe + d_nc * snc * o.ne;
  gr.d_inv_s = (float)*d_inv_s;
  gr.d_sdf = (float)(d_pe + d_ne);
  const double d_ic = (d_ne - d_pe) * dist * 0.5;
  gr.d_dist = (float)((d_ne - d_pe) * o.ic * 0.5);
  const double dic_dtc = (o.tc < 1.0 ? 0.5 * (1.0 - r) : 0.0) + (o.tc < 0.0 ? r : 0.0);
  gr.d_tc = (float)(d_ic * dic_dtc);
  return gr;
}

// up-sampling section alpha (no clip)                                              (NeuS.py:144-177)
CNR_HD float upsample_alpha(float s0, float s1, float z0, float z1, float cos_val, float inv_s) {
  float mid = (s0 + s1) * 0.5f;
  float dist = z1 - z0;
  float pe = mid - cos_val * dist * 0.5f;
  float ne = mid + cos_val * dist * 0.5f;
  float pc = sigmoidf_(pe * inv_s), nc = sigmoidf_(ne * inv_s);
  return (pc - nc + 1e-5f) / (pc + 1e-5f);
}

// |o + d z|: distance of the ray's point at z from the origin
CNR_HD float ray_radius(const float o[3], const float d[3], float z) {
  const float x = o[0] + d[0] * z, y = o[1] + d[1] * z, w = o[2] + d[2] * z;
  return sqrtf(x * x + y * y + w * w);
}

// searchsorted(a, x, right=True): index of the first entry above x
CNR_HD int upper_bound_idx(const float* a, int n, float x) {
  int lo = 0, hi = n;
  while (lo < hi) { int mid = (lo + hi) >> 1; if (a[mid] > x) hi = mid; else lo = mid + 1; }
  return lo;
}

// cat_z_vals as a stable merge (NeuS.py:183-197): the n old samples (zo, so) and the m new ones (nz, ns) of one ray, each sorted, go to their
// positions in the merged row through put(position, z, sdf).  A worker takes the samples first, first + step, ...
template <class Put>
CNR_HD void merge_samples(const float* zo, const float* so, int n, const float* nz, const float* ns, int m, int first, int step, Put put) {
  for (int i = first; i < n; i += step) {   // old sample i: position = i + #(new < z_i)
    const float z = zo[i];
    int cnt = 0;
    for (int j = 0; j < m; ++j) cnt += nz[j] < z ? 1 : 0;
    put(i + cnt, z, so[i]);
  }
  for (int j = first; j < m; j += step) {   // new sample j: position = #(old <= new_j) + its rank among the new samples
    const float z = nz[j];
    const int lo = upper_bound_idx(zo, n, z);
    int rank = 0;   // (they are monotone in practice; this keeps the merge a bijection regardless)
    for (int q2 = 0; q2 < m; ++q2) rank += (nz[q2] < z || (nz[q2] == z && q2 < j)) ? 1 : 0;
    put(lo + rank, z, ns[j]);
  }
}

// slope of the sdf along the ray in one section of up_sample (NeuS.py:148)
CNR_HD float upsample_slope(float s0, float s1, float z0, float z1) { return (s1 - s0) / (z1 - z0 + 1e-5f); }

// section cosine of up_sample: the smaller of the previous and the own slope, clipped to [-1e3, 0], zero outside the unit sphere (NeuS.py:150-160)
CNR_HD float upsample_cos(float prev, float cur, float r0, float r1) {
  float c = fminf(prev, cur);
  c = fminf(fmaxf(c, -1e3f), 0.0f);
  const bool inside = r0 < 1.0f || r1 < 1.0f;
  return inside ? c : c * 0.0f;
}

// inversion of the cdf in sample_pdf: the bin of u, then linear interpolation inside it; a bin narrower than 1e-5 divides by 1 (ray_utils.py:138-152)
CNR_HD float invert_cdf(const float* cdf, const float* z, int n, float u) {
  const int idx = upper_bound_idx(cdf, n, u);
  const int below = idx - 1 > 0 ? idx - 1 : 0;
  const int above = idx < n - 1 ? idx : n - 1;
  const float c0 = cdf[below], c1 = cdf[above];
  const float b0 = z[below], b1 = z[above];
  float den = c1 - c0;
  if (den < 1e-5f) den = 1.0f;
  const float t = (u - c0) / den;
  return b0 + t * (b1 - b0);
}

// One ray of get_rays_multicam / get_rays_at (ray_utils.py:16-119): camera-frame direction of pixel (px, py), optional normalisation,
// rotation into the world frame, camera centre as origin.  u = unnormalised direction, dirs = (normalised) camera-frame direction.
struct RayGeom { float u[3], un, dirs[3], d[3], o[3]; };
CNR_HD RayGeom ray_geometry(const float* c2w /* one [4][4] */, float fx, float fy, int H, int W, int px, int py, int normalize, int opengl) {
  RayGeom r;
  const float ys = opengl ? -1.0f : 1.0f, zs = opengl ? -1.0f : 1.0f;
  r.u[0] = ((float)px - (float)W * 0.5f) / fx;
  r.u[1] = ys * ((float)py - (float)H * 0.5f) / fy;
  r.u[2] = zs;
  r.un = sqrtf(r.u[0] * r.u[0] + r.u[1] * r.u[1] + r.u[2] * r.u[2]);
  for (int k = 0; k < 3; ++k) r.dirs[k] = normalize ? r.u[k] / r.un : r.u[k];
  for (int k = 0; k < 3; ++k) {
    r.d[k] = r.dirs[0] * c2w[k * 4] + r.dirs[1] * c2w[k * 4 + 1] + r.dirs[2] * c2w[k * 4 + 2];
    r.o[k] = c2w[k * 4 + 3];
  }
  return r;
}

// d/d rgb of inverse_sigmoid (clamp semantics of torch: gradient passes where the clamp is inactive, bounds inclusive)
CNR_HD float inverse_sigmoid_grad(float rgb) {
  if (rgb < 0.0f || rgb > 1.0f) return 0.0f;
  float x = rgb;
  float x1 = fmaxf(x, 1e-5f), x2 = fmaxf(1.0f - x, 1e-5f);
  float g1 = x >= 1e-5f ? 1.0f / x1 : 0.0f;
  float g2 = (1.0f - x) >= 1e-5f ? 1.0f / x2 : 0.0f;
  return g1 + g2;
}

// inv_s = exp(10 variance) clipped to [1e-6, 1e6]                                  (fields.py SingleVarianceNetwork, NeuS.py:224)
CNR_HD float inv_s_of(float variance) { return fminf(fmaxf(expf(variance * 10.0f), 1e-6f), 1e6f); }
// its backward: d variance from d inv_s (the gradient passes where the clip is inactive, bounds inclusive)
CNR_HD float inv_s_backward(float variance, float d_inv_s) {
  const float raw = expf(variance * 10.0f);
  return (raw >= 1e-6f && raw <= 1e6f) ? d_inv_s * 10.0f * raw : 0.0f;
}

// forward quantities of one sample of the compositor, recomputed identically in forward and backward (Color_NeuS.py:41-90 / NeuS.py:209-256).
// z: the ray's M positions; j >= M (the lanes behind a ragged last chunk) repeats sample M - 1 with ok = false
struct RaySample {
  bool ok;
  float z, dist, relax, inside, gn;
  float g[3];
  AlphaOut a;
};
CNR_HD RaySample ray_sample(const float* z, int j, int M, float sample_dist, const float o[3], const float d[3], const float* sdf, const float* g,
                            long pt, float inv_s, float r) {
  RaySample q;
  q.ok = j < M;
  const int jj = q.ok ? j : M - 1;
  q.z = z[jj];
  q.dist = jj + 1 < M ? z[jj + 1] - q.z : sample_dist;
  const float pn = ray_radius(o, d, q.z + q.dist * 0.5f);
  q.inside = pn < 1.0f ? 1.0f : 0.0f;
  q.relax = pn < 1.2f ? 1.0f : 0.0f;
  const long p2 = q.ok ? pt : pt - (j - jj);
  q.g[0] = g[p2 * 3]; q.g[1] = g[p2 * 3 + 1]; q.g[2] = g[p2 * 3 + 2];
  q.gn = sqrtf(q.g[0] * q.g[0] + q.g[1] * q.g[1] + q.g[2] * q.g[2]);
  q.a = alpha_forward(sdf[p2], q.g, d, q.dist, inv_s, r);
  return q;
}

// the upstream gradients of the compositor that are per ray (absent ones are zero); dws includes the background's share of d color_fine
struct RayUpstream { float dcol[3], dglob[3], dws, ddepth, dwmax, dge, eik_den, ddrel_ray; };
CNR_HD RayUpstream ray_upstream(const CompositeBwd& p, long ray) {
  RayUpstream u;
  for (int k = 0; k < 3; ++k) { u.dcol[k] = p.d_color_fine ? p.d_color_fine[ray * 3 + k] : 0.0f; u.dglob[k] = p.d_global_color ? p.d_global_color[ray * 3 + k] : 0.0f; }
  u.dws = p.d_weight_sum ? p.d_weight_sum[ray] : 0.0f;
  if (p.background_rgb) for (int k = 0; k < 3; ++k) u.dws -= u.dcol[k] * p.background_rgb[k];
  u.ddepth = p.d_depth ? p.d_depth[ray] : 0.0f;
  u.dwmax = p.d_weight_max ? p.d_weight_max[ray] : 0.0f;
  u.dge = p.d_gradient_error ? p.d_gradient_error[0] : 0.0f;
  u.eik_den = p.eik_sums[1] + 1e-5f;
  u.ddrel_ray = p.d_delta_relight_ray ? p.d_delta_relight_ray[ray] : 0.0f;
  return u;
}

// d loss / d w of sample pt at position z: the direct terms (those through the transmittance follow from the suffix sums of wbar * w)
CNR_HD float sample_wbar(const CompositeBwd& p, const RayUpstream& u, long pt, float z, bool is_max) {
  float wb = 0.0f;
  for (int k = 0; k < 3; ++k) wb += u.dcol[k] * p.color[pt * p.ldcolor + k];
  if (p.gcolor) for (int k = 0; k < 3; ++k) wb += u.dglob[k] * p.gcolor[pt * p.ldg + k];
  wb += u.dws + u.ddepth * z;
  if (p.d_weights) wb += p.d_weights[pt];
  if (is_max) wb += u.dwmax;
  return wb;
}

// backward of sample pt behind the scans: T its transmittance, w its weight, wbar = sample_wbar, S = sum_{k > j} wbar_k w_k.  Adds the sample's
// term to drd (d rays_d), returns its d inv_s, and, with `store`, writes its rows of gbar, d_z, ztop, dtop and gc_a (pad columns included: one
// launch less than zeroing them apart).  `store` is false for the ray a partly filled HIP workgroup computes a second time.
CNR_HD float sample_backward(const CompositeBwd& p, const RayUpstream& u, const RaySample& q, const float d[3], long pt, float inv_s, float T, float w,
                             float wbar, float S, bool store, float drd[3]) {
  const float dalpha = wbar * T - S / (1.0f - q.a.alpha + 1e-7f);
  const AlphaGrad ag = alpha_backward(q.a, q.dist, inv_s, p.cos_anneal, dalpha, p.d_cdf ? p.d_cdf[pt] : 0.0f);
  const float ecoef = (q.relax > 0.0f && q.gn > 0.0f) ? u.dge / u.eik_den * 2.0f * (q.gn - 1.0f) / q.gn : 0.0f;
  float gb[3];
  for (int k = 0; k < 3; ++k) {
    gb[k] = ag.d_tc * d[k] + ecoef * q.g[k];
    if (p.d_gradients) gb[k] += p.d_gradients[pt * 3 + k];
    drd[k] += ag.d_tc * q.g[k];
  }
  if (!store) return ag.d_inv_s;
  if (p.d_z) { p.d_z[pt * 2] = u.ddepth * w; p.d_z[pt * 2 + 1] = ag.d_dist; }
  p.ztop[pt * p.ldztop + p.ztop_col] = (ag.d_sdf + (p.d_sdf_s ? p.d_sdf_s[pt] : 0.0f)) / p.sdf_scale;
  for (int k = p.ztop_col + 1; k < p.ldztop; ++k) p.ztop[pt * p.ldztop + k] = 0.0f;
  for (int k = 0; k < 3; ++k) p.gbar[pt * 4 + k] = gb[k];
  p.gbar[pt * 4 + 3] = 0.0f;
  for (int k = 0; k < 3; ++k) {
    const float cbar = u.dcol[k] * w + (p.d_color_s ? p.d_color_s[pt * 3 + k] : 0.0f);   // cotangent of the composited (relit) colour sample
    if (p.has_relight) {
      const float relit = p.color[pt * p.ldcolor + k];
      const float gc = p.gcolor[pt * p.ldg + k];
      float tbar, gca = u.dglob[k] * w + (p.d_gcolor_s ? p.d_gcolor_s[pt * 3 + k] : 0.0f);
      if (p.inv_sigmoid) {
        tbar = cbar * relit * (1.0f - relit);
        gca += tbar * inverse_sigmoid_grad(gc);
      } else {
        const float pass = (relit > 0.0f && relit < 1.0f) ? 1.0f : 0.0f;   // clamp(rgb + sigmoid(h) - 0.5, 0, 1)
        const float sg = relit - gc + 0.5f;                                 // = sigmoid(h) where the clamp is inactive
        tbar = cbar * pass * sg * (1.0f - sg);
        gca += cbar * pass;
      }
      p.dtop[pt * p.ldtop + k] = tbar + (p.d_delta_relight ? p.d_delta_relight[pt * 3 + k] : 0.0f) + u.ddrel_ray;
      p.gc_a[pt * p.ldtop + k] = gca;
    } else {
      p.gc_a[pt * p.ldtop + k] = cbar;
    }
  }
  if (p.has_relight) for (int k = 3; k < p.ldtop; ++k) p.dtop[pt * p.ldtop + k] = 0.0f;
  for (int k = 3; k < p.ldtop; ++k) p.gc_a[pt * p.ldtop + k] = 0.0f;
  return ag.d_inv_s;
}

// d loss / d rays_d[k] of one ray from its sums over the samples: sd = sum pbar * mid, d_alpha = CompositeBwd::d_rays_d, spe = the summed
// cotangent of the PE(dir) columns [d, sin(2^m d), cos(2^m d), ...]
CNR_HD float rays_d_grad(float dk, float sd, float d_alpha, const float* spe, int k, int multires_view) {
  float acc = sd + d_alpha + spe[k];
  float f = 1.0f;
  for (int m = 0; m < multires_view; ++m) {
    acc += f * (cosf(dk * f) * spe[3 + 6 * m + k] - sinf(dk * f) * spe[6 + 6 * m + k]);
    f *= 2.0f;
  }
  return acc;
}

}  // namespace cnr
