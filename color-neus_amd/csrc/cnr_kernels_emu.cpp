// CPU emulation of the kernel layer -- TEST INFRASTRUCTURE ONLY (built with -DCNR_CPU_EMU into
// libcolorneus_emu.so, loaded only by tests/ to exercise the host orchestration, operand views, epilogues and
// per-point bodies without a GPU).  The product path never loads this library.
//
// GEMMs are plain loops over the same views / epilogues; per-ray kernels are straightforward serial code.
#include <algorithm>
#include <cstdlib>
#include <cstdio>
#include <vector>

#include "cnr_backend.h"
#include "cnr_bodies.h"
#include "cnr_loss.h"
#include "cnr_optim.h"
#include "cnr_rays.h"
#include "cnr_cameras.h"
#include "cnr_bg.h"
#include "cnr_mc.h"
#include "cnr_nn.h"
#include "cnr_image.h"
#include "cnr_pixels.h"
#include "cnr_raster.h"
#include "cnr_meshcc.h"
#include "cnr_surface.h"
#include "cnr_cull.h"
#include "cnr_register.h"

namespace cnr {

// ---- cnr_runtime.hip
const char* be_name() { return "cpu-emu"; }
void be_timing_enable(int) {}
int be_timing_collect(KernelTiming*, int) { return 0; }
int be_check_last_error(char*, size_t) { return 0; }
void be_range_push(const char*) {}
void be_range_pop() {}
void be_memset_zero(void* p, size_t bytes, cnr_stream) { memset(p, 0, bytes); }
void be_zero_cols(float* p, int ld, int c0, int c1, long rows, cnr_stream) {
  for (long r = 0; r < rows; ++r) for (int c = c0; c < c1; ++c) p[r * ld + c] = 0.0f;
}
void be_copy_cols(float* dst, int ld_dst, const float* src, int ld_src, int ncols, long rows, cnr_stream) {
  for (long r = 0; r < rows; ++r) memcpy(dst + r * ld_dst, src + r * ld_src, (size_t)ncols * sizeof(float));
}

// ---- the layer launches (cnr_gemm*.hip) and what only the HIP build has (cnr_chain*.hip, cnr_sweep0.hip, cnr_narrow_bwd.hip)
void be_layer_gemm(const LayerGemm& g0, cnr_stream) {
  LayerGemm g = g0;
  if (g.P_dev) g.P = *g.P_dev;
  g.K += g.k_extra;   // (the rank-one form is a speed matter of the fused HIP launch)
  const int kp = round_up(g.K, 4);
  std::vector<float> arow(kp + 4);
#pragma omp parallel for firstprivate(arow)
  for (long row = 0; row < g.P; ++row) {
    for (int k = 0; k < kp; k += 4) {
      f4 v = view_eval4(g.A, row, k);
      arow[k] = v.x; arow[k + 1] = v.y; arow[k + 2] = v.z; arow[k + 3] = v.w;
    }
    if (g.dot_w && g.first_col == 0) {   // row dot (LayerGemm::dot_*): the sdf row of the top SDF layer
      float acc = 0.0f;
      for (int k = 0; k < g.K; ++k) acc = fmaf(arow[k], g.dot_w[k], acc);
      g.dot_out[row] = (acc + (g.dot_bias ? g.dot_bias[0] : 0.0f)) * g.dot_scale;
    }
    int ncols = g.N;
    if (g.E.tail_src && g.E.n_out + g.E.tail_n > ncols) ncols = g.E.n_out + g.E.tail_n;
    for (int n = g.first_col; n < round_up(ncols, 32); ++n) {
      const float* w = g.W + (long)(n < round_up(g.N, 32) ? n : 0) * g.ldw;
#ifdef CNR_EMU_DOUBLE_ACC
      double accd = 0.0;
      if (n < round_up(g.N, 32)) for (int k = 0; k < g.K; ++k) accd += (double)arow[k] * (double)w[k];
      float acc = (float)accd;
#else
      float acc = 0.0f;
      if (n < round_up(g.N, 32)) for (int k = 0; k < g.K; ++k) acc = fmaf(arow[k], w[k], acc);
#endif
      epi_apply(g.E, row, n, acc);
    }
  }
}

void be_dw_gemm(const DwGemm& g, cnr_stream) {
#pragma omp parallel for
  for (int chunk = 0; chunk < g.nchunk; ++chunk) {
    float* out = g.partial + (long)chunk * g.Npad * g.ldk;
    std::fill(out, out + (long)g.Npad * g.ldk, 0.0f);
    if (g.colsum) std::fill(g.colsum + (long)chunk * g.Npad, g.colsum + (long)(chunk + 1) * g.Npad, 0.0f);
    long p0 = chunk * g.chunk_pts, p1 = std::min(g.P, p0 + g.chunk_pts);
    std::vector<float> x(round_up(g.N, 4) + 4), y(round_up(g.K, 4) + 4);
    for (int pair = 0; pair < g.npairs; ++pair)
      for (long pt = p0; pt < p1; ++pt) {
        for (int n = 0; n < g.N; n += 4) { f4 v = view_eval4(g.X[pair], pt, n); x[n] = v.x; x[n + 1] = v.y; x[n + 2] = v.z; x[n + 3] = v.w; }
        for (int k = 0; k < g.K; k += 4) { f4 v = view_eval4(g.Y[pair], pt, k); y[k] = v.x; y[k + 1] = v.y; y[k + 2] = v.z; y[k + 3] = v.w; }
        for (int n = 0; n < g.N; ++n) {   // (skip_main is a speed matter of the HIP backend: the emulation forms every tile here)
          float xv = x[n];
          if (pair == 0 && g.colsum) g.colsum[(long)chunk * g.Npad + n] += xv;
          if (xv == 0.0f) continue;
          float* o = out + (long)n * g.ldk;
          for (int k = 0; k < g.K; ++k) o[k] += xv * y[k];
        }
      }
  }
}

bool be_fdw_enabled() { return !debug_flags().no_fdw; }
bool be_fdw_xrow() { return be_fdw_enabled(); }
void be_layer_dw_gemm(const LayerGemm& g, const DwGemm& d, const DwFuse& f, cnr_stream s) {
  // xrow_mode 2: the plain weight-gradient GEMM below forms the extra row itself (d.N covers it) but zero-fills the slots first: keep what
  // the mode-1 launch left there and add it back
  std::vector<float> keep;
  if (f.xrow_mode == 2) {
    keep.resize((size_t)f.nslots * 256);
    for (int c = 0; c < f.nslots; ++c) memcpy(&keep[(size_t)c * 256], f.xrow + (long)c * f.xrow_stride, 256 * sizeof(float));
  }
  be_dw_gemm(d, s);      // (first: EK_VBACK updates o1 in place, but neither dW operand is an output of this launch, so the order is free)
  be_layer_gemm(g, s);
  if (f.xrow_mode == 2)
    for (int c = 0; c < f.nslots; ++c)
      for (int k = 0; k < 256; ++k) f.xrow[(long)c * f.xrow_stride + k] += keep[(size_t)c * 256 + k];
  if (f.xrow_mode == 1)   // column sums of the o2 output over the point slices of d
    for (int c = 0; c < f.nslots; ++c) {
      const long p0 = c * d.chunk_pts, p1 = std::min(d.P, p0 + d.chunk_pts);
      for (int k = 0; k < 256; ++k) {
        float sum = 0.0f;
        for (long pt = p0; pt < p1; ++pt) sum += g.E.o2[pt * g.E.ld2 + k];
        f.xrow[(long)c * f.xrow_stride + k] = sum * f.xrow_scale;
      }
    }
}

// the CPU emulation has no chain-fused kernels: the host orchestration falls back to the per-layer sequence
void be_pack_frags_many(const PackJob*, int, cnr_stream) {}
bool be_sdf_value_chain(const SdfValueChain&, cnr_stream) { return false; }
bool be_relu_chain_fwd(const ReluChainFwd&, cnr_stream) { return false; }
bool be_relu_chain_fwd_enabled() { return false; }
bool be_sdf_save_chain(const SdfSaveChain&, cnr_stream) { return false; }
bool be_sweep0_ok(const LayerGemm&) { return false; }   // (nor the sweep launch that forms its layer's weight-gradient pair)
int be_sweep0_slots(long) { return 0; }
void be_sweep0_dw(const LayerGemm&, float*, int, cnr_stream) {}
bool be_narrow_bwd_ok(const NarrowBwd&) { return false; }   // (nor the one-pass backward of a narrow-input layer)
int be_narrow_bwd_slots(long) { return 0; }
void be_narrow_bwd(const NarrowBwd&, cnr_stream) {}

// ---- cnr_kernels.hip
#define CNR_PW(NAME, PARAM, BODY, COUNT)                \
  void be_##NAME(const PARAM& p, cnr_stream) {          \
    const long n_ = (COUNT);                            \
    _Pragma("omp parallel for") for (long i = 0; i < n_; ++i) BODY(p, i); \
  }
CNR_POINTWISE_KERNELS(CNR_PW)
// the kernels outside that table: their HIP forms stage rows in LDS or spread a point over 16 lanes
CNR_PW(embed_z, EmbedZ, body_embed_z, p.R* p.m)
CNR_PW(embed_pts, EmbedPts, body_embed_pts, p.n)
CNR_PW(fine_setup, FineSetup, body_fine_setup, p.R* p.M)
CNR_PW(grad_finish, GradFinish, body_grad_finish, p.P)
CNR_PW(gbar_finish, GbarFinish, body_gbar_finish, p.P)

void be_head_bwd(const HeadBwd& p, cnr_stream) {
  const long per = round_up((int)((p.P + p.nslots - 1) / p.nslots), 64);
#pragma omp parallel for
  for (int slot = 0; slot < p.nslots; ++slot) {
    float* out = p.partial + (long)slot * p.npad * p.ldk;
    for (int j = 0; j < p.n; ++j) {
      for (int k = 0; k < p.ldk; ++k) out[(long)j * p.ldk + k] = 0.0f;
      if (p.colsum) p.colsum[(long)slot * p.npad + j] = 0.0f;
    }
    const long p0 = slot * per, p1 = std::min(p.P, p0 + per);
    for (long pt = p0; pt < p1; ++pt)
      for (int k = 0; k < p.K; ++k) {
        const float a = p.aux[pt * p.ldaux + k];
        float v = 0.0f;
        for (int j = 0; j < p.n; ++j) {
          const float d = p.dtop[pt * p.ldt + j];
          v = fmaf(p.W[(long)j * p.ldw + k], d, v);
          out[(long)j * p.ldk + k] = fmaf(d, a, out[(long)j * p.ldk + k]);
          if (k == 0 && p.colsum) p.colsum[(long)slot * p.npad + j] += d;
        }
        p.dout[pt * p.ldo + k] = a > 0.0f ? v : 0.0f;
      }
  }
}
void be_head_fwd(const HeadFwd& p, cnr_stream) {
  const long P = p.P_dev ? (long)*p.P_dev : p.P;
#pragma omp parallel for
  for (long row = 0; row < P; ++row)
    for (int j = 0; j < 16; ++j) {
      float acc = 0.0f;
      if (j < p.n) for (int c = 0; c < 256; ++c) acc = fmaf(p.h[row * p.ldh + c], p.W[(long)j * p.ldw + c], acc);
      epi_apply(p.E, row, j, acc);
    }
}
void be_strip_bwd(const StripBwd& p, cnr_stream) {
  const long per = round_up((int)((p.P + p.nslots - 1) / p.nslots), 64);
#pragma omp parallel for
  for (int slot = 0; slot < p.nslots; ++slot) {
    float* out = p.partial + (long)slot * p.npad * p.ldk;
    for (int n = 0; n < 256 && n < p.npad; ++n)
      for (int k = 256; k < p.ldk; ++k) out[(long)n * p.ldk + k] = 0.0f;
    const long p0 = slot * per, p1 = std::min(p.P, p0 + per);
    for (long pt = p0; pt < p1; ++pt)
      for (int j = 0; j < p.nt; ++j) {
        const float y = p.y[pt * p.ldy + j];
        float dot = 0.0f;
        for (int n = 0; n < 256; ++n) {
          const float d = p.dout[pt * p.ldo + n];
          dot = fmaf(d, p.Wt[(long)(256 + j) * p.ldwt + n], dot);
          if (n < p.npad) out[(long)n * p.ldk + 256 + j] = fmaf(d, y, out[(long)n * p.ldk + 256 + j]);
        }
        if (p.tail) p.tail[pt * p.ldt + j] = dot * p.tail_scale;
      }
  }
}
void be_split_planes_many(const SplitJob*, int, cnr_stream) {}

static void prep_weight(const PrepWeight& p) {
  for (int n = 0; n < p.npad; ++n) {
    const bool real = n < p.n;
    const int nr = real ? (n + p.row_rot) % p.n : 0;
    float scale = 1.0f;
    if (p.g && real) {
      double ss = 0.0;   // row norm accumulated in double (weight_norm is the most rounding-sensitive step: x inv_s downstream)
      for (int c = 0; c < p.k_ref; ++c) { double x = p.v[(long)nr * p.k_ref + c]; ss += x * x; }
      scale = weight_norm_scale(p.g[nr], ss);
    }
    for (int j = 0; j < p.kpad; ++j) {
      float val = 0.0f;
      if (real && j < p.ldw) {
        int src = seg_src_of(p.seg, p.nseg, j);
        if (src >= 0) val = p.v[(long)nr * p.k_ref + src] * scale;
      }
      if (j < p.ldw) p.W[(long)n * p.ldw + j] = val;
      if (n < p.ldwt) p.Wt[(long)j * p.ldwt + n] = val;
    }
    p.bias[n] = real && p.b ? p.b[nr] : 0.0f;
  }
}
void be_prep_weights(const PrepWeight* p, int count, cnr_stream) { for (int i = 0; i < count; ++i) prep_weight(p[i]); }

static void finish_weight(const FinishWeight& p) {
  std::vector<float> dwi(p.ldk), dref(p.k_ref);
  for (int n = 0; n < p.n; ++n) {
    const int nr = (n + p.row_rot) % p.n;
    for (int j = 0; j < p.ldk; ++j) {
      float s = 0.0f;
      const int nch = j >= p.col_hi ? p.nchunk_hi : p.nchunk;
      for (int c = 0; c < nch; ++c) s += p.partial[((long)c * p.npad + n) * p.ldk + j];
      dwi[j] = s;
    }
    for (int c = 0; c < p.k_ref; ++c) {
      const int dst = seg_dst_of(p.seg, p.nseg, c);
      dref[c] = dst >= 0 ? dwi[dst] : 0.0f;
    }
    if (p.g) {
      double dotd = 0.0, ssd = 0.0;
      for (int c = 0; c < p.k_ref; ++c) { double vv = p.v[(long)nr * p.k_ref + c]; dotd += (double)dref[c] * vv; ssd += vv * vv; }
      float dot = (float)dotd, nrm = (float)sqrt(ssd), gg = p.g[nr];
      p.dg[nr] = dot / nrm;
      for (int c = 0; c < p.k_ref; ++c) p.dv[(long)nr * p.k_ref + c] = weight_norm_dv(gg, nrm, dot, dref[c], p.v[(long)nr * p.k_ref + c]);
    } else {
      for (int c = 0; c < p.k_ref; ++c) p.dv[(long)nr * p.k_ref + c] = dref[c];
    }
    if (p.db && p.colsum) {
      float s = 0.0f;
      for (int c = 0; c < (p.ncolsum > 0 ? p.ncolsum : p.nchunk); ++c) s += p.colsum[(long)c * p.npad + n];
      p.db[nr] = s;
    }
  }
}
void be_finish_weights(const FinishWeight* f, int count, cnr_stream) { for (int i = 0; i < count; ++i) finish_weight(f[i]); }

void be_reduce_eik(const ReduceEik& p, cnr_stream) {
  float a = 0.0f, b = 0.0f;
  for (long r = 0; r < p.R; ++r) { a += p.partial[r * 2]; b += p.partial[r * 2 + 1]; }
  p.sums[0] = a; p.sums[1] = b;
  if (p.sums_out) { p.sums_out[0] = a; p.sums_out[1] = b; }
  *p.gradient_error = a / (b + 1e-5f);
}

void be_variance_finish(const VarianceFinish& p, cnr_stream) {
  float a = 0.0f;
  for (long r = 0; r < p.R; ++r) a += p.partial[r];
  *p.d_variance = inv_s_backward(p.variance[0], a);
}

// ---- cnr_perray.hip
void be_sampler_step(const SamplerStep& p, cnr_stream s) {   // the three steps one after the other (the fused launch is a speed matter)
  if (p.do_merge) be_merge(p.g, s);
  be_upsample(p.u, s);
  if (p.do_embed) {
    EmbedZ e;
    e.o = p.u.o; e.d = p.u.d; e.R = p.u.R; e.m = p.u.m; e.z = p.u.new_z; e.ldz = p.u.m; e.make_z = 0;
    e.near_ = nullptr; e.far_ = nullptr; e.t_rand = nullptr; e.scale = p.scale; e.multires = p.multires; e.E = p.E;
    be_embed_z(e, s);
  }
}

void be_upsample(const UpSample& p, cnr_stream) {
#pragma omp parallel for
  for (long ray = 0; ray < p.R; ++ray) {
    const int n = p.n, nsec = n - 1;
    const float* z = p.z + ray * p.ldz;
    const float* s = p.w_in ? nullptr : p.sdf + ray * p.lds;
    std::vector<float> rad(n), cs(n), w(n), cdf(n);
    float T = 1.0f, total = 0.0f;
    if (p.w_in) {
      for (int i = 0; i < nsec; ++i) { w[i] = p.w_in[ray * nsec + i] + 1e-5f; total += w[i]; }
    } else {
    for (int i = 0; i < n; ++i) rad[i] = ray_radius(p.o + ray * 3, p.d + ray * 3, z[i]);
    for (int i = 0; i < nsec; ++i) cs[i] = upsample_slope(s[i], s[i + 1], z[i], z[i + 1]);
    for (int i = 0; i < nsec; ++i) {
      float c = upsample_cos(i > 0 ? cs[i - 1] : 0.0f, cs[i], rad[i], rad[i + 1]);
      float a = upsample_alpha(s[i], s[i + 1], z[i], z[i + 1], c, p.inv_s);
      w[i] = a * T + 1e-5f;
      T = T * (1.0f - a + 1e-7f);
      total += w[i];
    }
    }
    cdf[0] = 0.0f;
    float run = 0.0f;
    for (int i = 0; i < nsec; ++i) { run += w[i] / total; cdf[i + 1] = run; }
    for (int k = 0; k < p.m; ++k) {
      float u = p.u_in ? p.u_in[ray * p.m + k] : linspace_at(0.5f / (float)p.m, 1.0f - 0.5f / (float)p.m, p.m, k);
      p.new_z[ray * p.m + k] = invert_cdf(cdf.data(), z, n, u);
    }
  }
}

void be_merge(const MergeZ& p, cnr_stream) {
#pragma omp parallel for
  for (long ray = 0; ray < p.R; ++ray) {
    std::vector<float> z(p.z + ray * p.ldz, p.z + ray * p.ldz + p.n), s(p.n, 0.0f);
    if (p.new_sdf) s.assign(p.sdf_in + ray * p.lds_in, p.sdf_in + ray * p.lds_in + p.n);
    const float* nz = p.new_z + ray * p.m;
    const float* ns = p.new_sdf ? p.new_sdf + ray * p.m : nz;   // (without new_sdf the values go nowhere)
    merge_samples(z.data(), s.data(), p.n, nz, ns, p.m, 0, 1, [&](int at, float zv, float sv) {
      p.z[ray * p.ldz + at] = zv;
      if (p.new_sdf) p.sdf_out[ray * p.lds_out + at] = sv;
    });
  }
}

void be_composite_fwd(const CompositeFwd& p, cnr_stream) {
  const float inv_s = inv_s_of(p.variance[0]);
#pragma omp parallel for
  for (long ray = 0; ray < p.R; ++ray) {
    const int M = p.M;
    const float* z = p.z + ray * M;
    float T = 1.0f, wsum = 0.f, wmax = -1.f, dep = 0.f, col[3] = {0, 0, 0}, gcl[3] = {0, 0, 0}, e0 = 0.f, e1 = 0.f;
    for (int j = 0; j < M; ++j) {
      long pt = ray * M + j;
      RaySample q = ray_sample(z, j, M, p.sample_dist, p.o + ray * 3, p.d + ray * 3, p.sdf, p.g, pt, inv_s, p.cos_anneal);
      float w = q.a.alpha * T;
      T = T * (1.0f - q.a.alpha + 1e-7f);
      wsum += w; wmax = std::max(wmax, w); dep += w * q.z;
      if (p.color) for (int k = 0; k < 3; ++k) col[k] += w * p.color[pt * p.ldcolor + k];
      if (p.gcolor) for (int k = 0; k < 3; ++k) gcl[k] += w * p.gcolor[pt * p.ldg + k];
      e0 += q.relax * (q.gn - 1.0f) * (q.gn - 1.0f); e1 += q.relax;
      p.weights[pt] = w; p.cdf_fine[pt] = q.a.pc; p.inside_sphere[pt] = q.inside;
      if (p.sdf_s) p.sdf_s[pt] = p.sdf[pt];
      if (p.color_s && p.color) for (int k = 0; k < 3; ++k) p.color_s[pt * 3 + k] = p.color[pt * p.ldcolor + k];
      if (p.gcolor_s && p.gcolor) for (int k = 0; k < 3; ++k) p.gcolor_s[pt * 3 + k] = p.gcolor[pt * p.ldg + k];
    }
    for (int k = 0; k < 3; ++k) {
      float cc = col[k];
      if (p.background_rgb) cc = cc + p.background_rgb[k] * (1.0f - wsum);
      p.color_fine[ray * 3 + k] = cc;
      if (p.global_color) p.global_color[ray * 3 + k] = gcl[k];
    }
    p.weight_sum[ray] = wsum; p.weight_max[ray] = wmax; p.depth[ray] = dep; p.s_val[ray] = 1.0f / inv_s;
    p.eik_partial[ray * 2] = e0; p.eik_partial[ray * 2 + 1] = e1;
    if (p.delta && p.delta_ray_sum) {
      float drs = 0.f;
      for (long i = ray * M * 3; i < (ray + 1) * M * 3; ++i) drs += p.delta[i];
      p.delta_ray_sum[ray] = drs;
    }
  }
}

void be_composite_bwd(const CompositeBwd& p, cnr_stream) {
  const float inv_s = inv_s_of(p.variance[0]);
#pragma omp parallel for
  for (long ray = 0; ray < p.R; ++ray) {
    const int M = p.M;
    const float* z = p.z + ray * M;
    const float* d = p.d + ray * 3;
    std::vector<RaySample> q(M);
    std::vector<float> T(M), w(M), wbar(M), S(M);
    float t = 1.0f, wmax = -1.0f;
    int amax = 0;
    for (int j = 0; j < M; ++j) {
      q[j] = ray_sample(z, j, M, p.sample_dist, p.o + ray * 3, d, p.sdf, p.g, ray * M + j, inv_s, p.cos_anneal);
      T[j] = t; w[j] = q[j].a.alpha * t; t = t * (1.0f - q[j].a.alpha + 1e-7f);
      if (w[j] > wmax) { wmax = w[j]; amax = j; }
    }
    const RayUpstream up = ray_upstream(p, ray);
    for (int j = 0; j < M; ++j) wbar[j] = sample_wbar(p, up, ray * M + j, q[j].z, j == amax);
    float run = 0.0f;
    for (int j = M - 1; j >= 0; --j) { S[j] = run; run += wbar[j] * w[j]; }
    float dinvs = 0.0f, drd[3] = {0, 0, 0};
    for (int j = 0; j < M; ++j) dinvs += sample_backward(p, up, q[j], d, ray * M + j, inv_s, T[j], w[j], wbar[j], S[j], true, drd);
    if (p.d_s_val) dinvs += -p.d_s_val[ray] / (inv_s * inv_s);
    p.dinvs_partial[ray] = dinvs;
    if (p.d_rays_d) for (int k = 0; k < 3; ++k) p.d_rays_d[ray * 3 + k] = drd[k];
  }
}

void be_prune_count(const PruneCount& p, cnr_stream) {
  for (long r = 0; r < p.R; ++r) {
    int c = 0;
    for (int j = 0; j < p.M; ++j) c += prune_keep(p.weights[r * p.M + j], p.eps) ? 1 : 0;
    p.counts[r] = c;
  }
}
void be_prune_scan(const PruneScan& p, cnr_stream) {
  int run = 0;
  for (long r = 0; r < p.R; ++r) { p.offsets[r] = run; run += p.counts[r]; }
  p.offsets[p.R] = run;
}
void be_prune_gather(const PruneGather& p, cnr_stream) {
  for (long r = 0; r < p.R; ++r) {
    int k = p.offsets[r];
    for (int j = 0; j < p.M; ++j) {
      long pt = r * p.M + j;
      if (!prune_keep(p.weights[pt], p.eps)) { prune_zero_dropped(p, pt); continue; }
      p.idx[k] = (int)pt;
      if (p.featx_c) {
        memcpy(p.featx_c + (long)k * p.ldfx, p.featx + pt * p.ldfx, sizeof(float) * p.ldfx);
        memcpy(p.aux_c + (long)k * kAux, p.aux + pt * kAux, sizeof(float) * kAux);
      }
      ++k;
    }
  }
}
void be_prune_scatter(const PruneScatter& p, cnr_stream) {
  for (long i = 0; i < *p.count; ++i) {
    long pt = p.idx[i];
    for (int c = 0; c < 4; ++c) p.gcol[pt * 4 + c] = p.gcol_c[i * 4 + c];
    if (p.relit) for (int c = 0; c < 4; ++c) p.relit[pt * 4 + c] = p.relit_c[i * 4 + c];
    if (p.delta) for (int c = 0; c < 3; ++c) p.delta[pt * 3 + c] = p.delta_c[i * 3 + c];
  }
}

void be_rays_grad_finish(const RaysGradFinish& p, cnr_stream) {
  const int npe = p.multires_view > 0 ? 3 + 6 * p.multires_view : 3;
  for (long ray = 0; ray < p.R; ++ray) {
    float so[3] = {0, 0, 0}, sd[3] = {0, 0, 0}, spe[27];
    for (int q = 0; q < 27; ++q) spe[q] = 0.0f;
    const float* dr = p.d + ray * 3;
    float snear = 0.0f, sfar = 0.0f;
    std::vector<float> dmid(p.M);
    for (int j = 0; j < p.M; ++j) {
      long pt = ray * p.M + j;
      float z0 = p.z[pt];
      float dist = j + 1 < p.M ? p.z[pt + 1] - z0 : p.sample_dist;
      float mid = z0 + dist * 0.5f;
      dmid[j] = 0.0f;
      for (int k = 0; k < 3; ++k) { float pb = p.pbar[pt * 4 + k]; so[k] += pb; sd[k] += pb * mid; dmid[j] += pb * dr[k]; }
      for (int q = 0; q < npe; ++q) {
        if (p.daux_dir_c) spe[q] += p.daux_dir_c[pt * p.lddir + 6 + q];
        if (p.daux_dir_r) spe[q] += p.daux_dir_r[pt * p.lddir + 6 + q];
      }
    }
    if (p.dz_parts && p.d_near && p.d_far) {
      for (int j = 0; j < p.M; ++j) {
        long pt = ray * p.M + j;
        float dz = p.dz_parts[pt * 2] + dmid[j];
        if (j + 1 < p.M) dz -= p.dz_parts[pt * 2 + 1] + 0.5f * dmid[j];
        if (j > 0) dz += p.dz_parts[(pt - 1) * 2 + 1] + 0.5f * dmid[j - 1];
        float lin = linspace_at(0.0f, 1.0f, p.M, j);
        snear += dz * (1.0f - lin);
        sfar += dz * lin;
      }
      p.d_near[ray] = snear; p.d_far[ray] = sfar;
    }
    if (!(p.d_o && p.d_d)) continue;
    for (int k = 0; k < 3; ++k) {
      p.d_d[ray * 3 + k] = rays_d_grad(dr[k], sd[k], p.d_rays_d_alpha[ray * 3 + k], spe, k, p.multires_view);
      p.d_o[ray * 3 + k] = so[k];
    }
  }
}

// ---- cnr_loss.hip
void be_loss_sums(const LossArgs& a, float* partial, float* sums, cnr_stream) {
  (void)partial;
  double s_rgb = 0, s_bce = 0, s_rel = 0;   // (the emulation only has to agree with the oracle to test tolerance, not bitwise with the GPU)
  for (long i = 0; i < a.R * 3; ++i) s_rgb += loss_rgb_term(a.color[i], a.gt[i], a.rgb_l1);
  if (a.mask) for (long r = 0; r < a.R; ++r) s_bce += loss_bce_term(a.wsum[r], a.mask[r]);
  if (a.drel) {
    const long per_ray = a.drel_per_ray ? 1 : (long)a.M * 3;
    for (long i = 0; i < a.R * per_ray; ++i) s_rel += a.drel[i] * ((a.include_mask && a.mask) ? a.mask[i / per_ray] : 1.0f);
  }
  sums[0] = (float)s_rgb; sums[1] = (float)s_bce; sums[2] = (float)s_rel; sums[3] = 0.f;
}
void be_loss_combine(const LossScalars& c, const float* sums, const float* gerr, float* out6, cnr_stream) { loss_combine(c, sums, gerr, out6); }
void be_loss_forward(const LossArgs& a, float* partial, unsigned* ticket, const LossScalars& c, const float* gerr, float* sums, float* out6, cnr_stream s) {
  (void)ticket;
  be_loss_sums(a, partial, sums, s);
  loss_combine(c, sums, gerr, out6);
}
void be_loss_shard_stats(const LossArgs& a, float* partial, unsigned* ticket, const float* eik_sums, float* stats8, cnr_stream s) {
  (void)ticket;
  float sums[4];
  be_loss_sums(a, partial, sums, s);
  stats8[0] = sums[0]; stats8[1] = sums[1]; stats8[2] = sums[2]; stats8[3] = eik_sums[0]; stats8[4] = eik_sums[1]; stats8[5] = eik_sums[1]; stats8[6] = stats8[7] = 0.0f;
}
void be_loss_shard_combine(const LossScalars& c, const float* stats8, float* out8, cnr_stream) { loss_shard_combine(c, stats8, out8); }
void be_loss_backward(const LossArgs& a, const LossScalars& c, const float* g_loss, const float* mean_rel, const float* eik_factor, float* coef4, float* d_color,
                      float* d_wsum, float* d_drel_ray, cnr_stream s) {
  loss_coef(c, g_loss, c.use_relight ? mean_rel : g_loss, eik_factor, coef4);
  be_loss_grads(a, coef4, d_color, d_wsum, nullptr, s);
  if (d_drel_ray) for (long r = 0; r < a.R; ++r) d_drel_ray[r] = (a.include_mask && a.mask) ? coef4[2] * a.mask[r] : coef4[2];
}
void be_loss_coef(const LossScalars& c, const float* g_loss, const float* mean_rel, float* coef4, cnr_stream) { loss_coef(c, g_loss, mean_rel, nullptr, coef4); }
void be_loss_grads(const LossArgs& a, const float* coef, float* d_color, float* d_wsum, float* d_drel, cnr_stream) {
  for (long i = 0; i < a.R * 3; ++i) d_color[i] = coef[0] * loss_rgb_grad(a.color[i], a.gt[i], a.rgb_l1);
  if (d_wsum) for (long r = 0; r < a.R; ++r) d_wsum[r] = a.mask ? coef[1] * loss_bce_grad(a.wsum[r], a.mask[r]) : 0.0f;
  if (d_drel) {
    const long per_ray = (long)a.M * 3;
    for (long i = 0; i < a.R * per_ray; ++i) d_drel[i] = coef[2] * ((a.include_mask && a.mask) ? a.mask[i / per_ray] : 1.0f);
  }
}

// ---- cnr_optim.hip
void be_clip_adam(const AdamArgs& a, cnr_stream) {
  for (int k = 0; k < a.count; ++k) {
    const AdamTensor& t = a.t[k];
    float coef = 1.0f;
    if (a.max_norm > 0.0f) {
      float tot = 0.0f;   // per-chunk sums, then the chunks (the summation order differs from the HIP kernels': round-off level)
      for (long c0 = 0; c0 < t.n; c0 += kAdamChunk) {
        float ss = 0.0f;
        for (long i = c0; i < t.n && i < c0 + kAdamChunk; ++i) ss += t.g[i] * t.g[i];
        tot += ss;
      }
      coef = adam_clip_coef(tot, a.max_norm);
    }
    for (long i = 0; i < t.n; ++i) adam_update1(a, t.w + i, t.g[i] * coef, a.m + t.off + i, a.v + t.off + i);
  }
}

// ---- cnr_rays.hip, cnr_cameras.hip, cnr_bg.hip
CNR_RAYS_KERNELS(CNR_PW)
CNR_CAMERA_KERNELS(CNR_PW)
CNR_BG_KERNELS(CNR_PW)

void be_gen_rays_bwd(const GenRaysBwd& q, cnr_stream) {
  for (int cam = 0; cam < q.f.n_cams; ++cam) {
    double acc[14] = {0};   // (the HIP kernel sums in float in a fixed tree order; the tests compare both with autograd)
    for (long i = 0; i < q.f.n; ++i) {
      int c; float out[14];
      body_gen_rays_bwd1(q, i, &c, out);
      if (c == cam) for (int k = 0; k < 14; ++k) acc[k] += out[k];
    }
    for (int k = 0; k < 12; ++k) q.d_c2w[cam * 16 + k] = (float)acc[k];
    for (int k = 12; k < 16; ++k) q.d_c2w[cam * 16 + k] = 0.0f;
    q.d_focal_partial[cam * 2] = (float)acc[12]; q.d_focal_partial[cam * 2 + 1] = (float)acc[13];
  }
  for (int j = 0; j < 2; ++j) {
    float s = 0.0f;
    for (int c = 0; c < q.f.n_cams; ++c) s += q.d_focal_partial[c * 2 + j];
    q.d_focal[j] = s;
  }
}

// ---- cnr_mc.hip
void be_mc_count(const McVolume& m, cnr_stream) {
  const int res = m.res;
  const long n = (long)res * res * res;
  int vo = 0, to = 0;
  for (long v = 0; v < n; ++v) {
    const int z = (int)(v % res), y = (int)((v / res) % res), x = (int)(v / ((long)res * res));
    unsigned char fl;
    const int idx = mc_cell(m.u, res, m.thr, x, y, z, &fl);
    m.flags[v] = fl;
    m.counts[v * 2] = vo; m.counts[v * 2 + 1] = to;
    vo += mc_popcount3(fl);
    to += idx >= 0 ? kMcNumTris[idx] : 0;
  }
  m.totals[0] = vo; m.totals[1] = to;
}
void be_mc_emit(const McVolume& m, const float* bmin, const float* bmax, float* verts, int* tris, cnr_stream) {
  const long n = (long)m.res * m.res * m.res;
  for (long v = 0; v < n; ++v) mc_emit_voxel(m, v, bmin, bmax, verts, tris);
}

// ---- cnr_nn.hip
// twin of nn_search_kernel / nn_unpack_kernel: the same nn_dist2 / nn_update / nn_key on the whole target range, one query per iteration
void be_nn_search(const NnSearch& p, cnr_stream) {
#pragma omp parallel for schedule(static)
  for (long i = 0; i < p.n; ++i) {
    const float qx = p.query[i * 3], qy = p.query[i * 3 + 1], qz = p.query[i * 3 + 2];
    float best = INFINITY;
    int besti = -1;
    for (long j = 0; j < p.m; ++j)
      nn_update(nn_dist2(qx, qy, qz, p.target[j * 3], p.target[j * 3 + 1], p.target[j * 3 + 2]), (int)j, best, besti);
    if (besti < 0)
      for (long j = 0; j < p.m; ++j)
        nn_update_inf(nn_dist2(qx, qy, qz, p.target[j * 3], p.target[j * 3 + 1], p.target[j * 3 + 2]), (int)j, best, besti);
    p.keys[i] = nn_key(best, besti);
    nn_unpack(p.keys[i], &p.dist2[i], &p.idx[i]);
  }
}

// ---- cnr_image.hip
// twin of image_stats_kernel / image_stats_finish_kernel: the same img_* functions, one element per iteration, the row pass of the three
// rows recomputed per element; float64 sums per image row, then the rows in index order (a fixed order, not the HIP build's: DESIGN 5)
void be_image_stats(const ImageStats& p, cnr_stream) {
  const int cs = p.cs;
  const long rowlen = (long)p.W * cs, nrows = p.planes * p.H;
  std::vector<double> part((size_t)nrows * 2);
#pragma omp parallel for schedule(static)
  for (long pr = 0; pr < nrows; ++pr) {
    const long plane = pr / p.H;
    const int r = (int)(pr - plane * p.H);
    const float* px = p.x + plane * p.H * rowlen;
    const float* py = p.y + plane * p.H * rowlen;
    double sum_d = 0.0, sum_s = 0.0;
    for (long g = 0; g < rowlen; ++g) {
      const int pix = (int)(g / cs), ch = (int)(g - (long)pix * cs);
      const long gl = (long)img_reflect(pix - 1, p.W) * cs + ch, gr = (long)img_reflect(pix + 1, p.W) * cs + ch;
      float h[5][3];
      for (int k = 0; k < 3; ++k) {
        const long row = (long)img_reflect(r - 1 + k, p.H) * rowlen;
        const float xl = px[row + gl], xc = px[row + g], xr = px[row + gr];
        const float yl = py[row + gl], yc = py[row + g], yr = py[row + gr];
        h[0][k] = img_tap3(xl, xc, xr);
        h[1][k] = img_tap3(yl, yc, yr);
        h[2][k] = img_tap3(xl * xl, xc * xc, xr * xr);
        h[3][k] = img_tap3(yl * yl, yc * yc, yr * yr);
        h[4][k] = img_tap3(xl * yl, xc * yc, xr * yr);
      }
      float m[5];
      for (int q = 0; q < 5; ++q) m[q] = img_tap3(h[q][0], h[q][1], h[q][2]);
      const float s = img_ssim(m[0], m[1], m[2], m[3], m[4]);
      const long at = (long)r * rowlen + g;
      if (p.map) p.map[plane * p.H * rowlen + at] = s;
      sum_d += (double)img_sqerr(px[at], py[at]);
      sum_s += (double)s;
    }
    part[2 * pr] = sum_d;
    part[2 * pr + 1] = sum_s;
  }
  double a = 0.0, b = 0.0;
  for (long pr = 0; pr < nrows; ++pr) { a += part[2 * pr]; b += part[2 * pr + 1]; }
  p.sums[0] = a;
  p.sums[1] = b;
}

// twin of depth_range_kernel / image_panel_kernel
void be_image_panel(const ImagePanel& p, cnr_stream) {
  p.keys[0] = p.keys[1] = 0xffffffffu;
  for (long i = 0; i < (long)p.H * p.W; ++i) {
    const float d = p.depth[i];
    if (d == d) {
      const unsigned k = img_depth_key(d);
      p.keys[0] = std::min(p.keys[0], k);
      p.keys[1] = std::min(p.keys[1], ~k);
    }
  }
  float vmin, vmax;
  img_depth_range(p.keys, &vmin, &vmax);
  p.range[0] = vmin;
  p.range[1] = vmax;
  const int rowb = p.nsec * 3 * p.W;
#pragma omp parallel for schedule(static)
  for (int row = 0; row < p.H; ++row)
    for (int col = 0; col < rowb; ++col) p.panel[(long)row * rowb + col] = img_panel_byte(p, row, col, vmin, vmax);
}

// ---- cnr_pixels.hip
void be_pixel_table(const PixelTable& t, cnr_stream) {
#pragma omp parallel for schedule(static)
  for (int n = 0; n < t.n_images; ++n) {
    const float* m = t.masks + (long)n * t.hw;
    int* row = t.order + (long)n * t.hw;
    int f = 0, g = 0;
    for (long i = 0; i < t.hw; ++i) f += pix_class(m[i]) == 1;
    for (long i = 0, a = 0; i < t.hw; ++i) {
      const int c = pix_class(m[i]);
      if (c == 1) row[a++] = (int)i;
      else if (c == 2) row[f + g++] = (int)i;
    }
    t.fg_count[n] = f; t.bg_count[n] = g;
  }
}

void be_choose_pixels(const PixelDraw& p, cnr_stream) {
  const PixKey k = pix_key(p.state[0], p.state[1]);
  std::vector<unsigned> pf(p.B), pb(p.B);
  std::vector<int> cams(p.B);
  unsigned F = 0, G = 0;
  for (int b = 0; b < p.B; ++b) {
    unsigned f, g;
    cams[b] = pix_slot_image(p, k, b);
    pix_slot_counts(p, cams[b], &f, &g);
    pf[b] = F += f; pb[b] = G += g;
    if (p.cams_out) p.cams_out[b] = cams[b];
  }
  const unsigned want = (unsigned)pix_want_fg(p), kfg = want < F ? want : F;
  const unsigned long long m = (unsigned long long)p.n - kfg;
  if (p.counts_out) { p.counts_out[0] = p.order ? (int)kfg : 0; p.counts_out[1] = p.order ? (int)(m < G ? m : G) : 0; }
#pragma omp parallel for schedule(static)
  for (long j = 0; j < p.n; ++j) {
    if (p.order) pix_draw_masked(p, k, j, pf.data(), pb.data(), cams.data(), kfg);
    else p.idx[j] = pix_draw_replace(p, k, j);
    if (p.t_rand) p.t_rand[j] = pix_jitter(k, j);
  }
  p.state[1] = (long)((unsigned long long)p.state[1] + 1ull);
}

// ---- cnr_raster.hip
// twin of the four raster_*_kernel launches: the same raster_* functions; triangles one after the other (the minimum of the keys does not
// depend on the order), each over its clipped box, the large ones through the list like the HIP build
void be_mesh_raster(const MeshRaster& p, cnr_stream) {
  const long hw = (long)p.H * p.W;
  p.dropped[0] = 0; p.dropped[1] = 0; *p.n_large = 0;
  for (long i = 0; i < hw; ++i) p.keys[i] = kRasterNoKey;
  if (p.V > 0) {
    const RasterCam cam = raster_cam(p);
#pragma omp parallel for schedule(static)
    for (long i = 0; i < p.V; ++i) p.pv[i] = raster_project(cam, p.vertices + i * 3, p.opengl, p.z_near);
  }
  auto draw = [&](const RasterTri& t, int f) {
    for (int j = t.j0; j <= t.j1; ++j)
      for (int i = t.i0; i <= t.i1; ++i) {
        unsigned long long& k = p.keys[(long)j * p.W + i];
        k = std::min(k, raster_pixel_key(t, f, i, j));
      }
  };
  if (p.V > 0)
    for (long f = 0; f < p.F; ++f) {
      const RasterTri t = raster_setup(p.triangles + f * 3, p.V, p.pv, p.H, p.W);
      if (t.status == 1) ++p.dropped[0];
      if (t.status == 2) ++p.dropped[1];
      if (t.status != 0) continue;
      if (raster_is_small(t)) draw(t, (int)f);
      else p.large[(*p.n_large)++] = (int)f;
    }
  for (int l = 0; l < *p.n_large; ++l) draw(raster_setup(p.triangles + (long)p.large[l] * 3, p.V, p.pv, p.H, p.W), p.large[l]);
#pragma omp parallel for schedule(static)
  for (int j = 0; j < p.H; ++j)
    for (int i = 0; i < p.W; ++i) raster_resolve(p, i, j);
}

// ---- cnr_meshcc.hip
// twins of the meshcc_*_kernel launches: the same meshcc_* functions, one triangle / vertex after the other.  The union-find runs with the
// plain accessor; hooking the larger root under the smaller gives the same roots as every order of the HIP build's hooks.
void be_mesh_components(const MeshComponents& p, cnr_stream) {
  for (int k = 0; k < 4; ++k) p.summary[k] = 0;
  p.dropped[0] = 0;
  for (long v = 0; v < p.V; ++v) { p.labels[v] = (int)v; p.face_count[v] = 0; p.vertex_count[v] = 0; }
  for (long f = 0; f < p.F; ++f) {
    const int* t = p.triangles + f * 3;
    if (!meshcc_valid(t, p.V)) { ++p.dropped[0]; continue; }
    meshcc_unite<MeshccPlain>(p.labels, t[0], t[1]);
    meshcc_unite<MeshccPlain>(p.labels, t[0], t[2]);
  }
  for (long v = 0; v < p.V; ++v) {
    const int root = meshcc_root(p.labels, (int)v);
    p.labels[v] = root;
    ++p.vertex_count[root];
    if (root == (int)v) ++p.summary[0];
  }
  for (long f = 0; f < p.F; ++f) {
    const int* t = p.triangles + f * 3;
    if (meshcc_valid(t, p.V)) ++p.face_count[p.labels[t[0]]];
  }
  unsigned long long best = 0;
  for (long v = 0; v < p.V; ++v)
    if (p.labels[v] == (int)v && p.face_count[v] > 0) {
      ++p.summary[1];
      best = std::max(best, meshcc_key(p.face_count[v], (int)v));
    }
  meshcc_unkey(best, &p.summary[2], &p.summary[3]);
}

// twin of meshcc_scan_kernel: the running counts in element order
void mesh_keep_scan(const MeshKeepScan& p, cnr_stream) {
  p.totals[0] = p.totals[1] = 0;
  for (long v = 0; v < p.V; ++v) p.vertex_map[v] = p.keep_vertex[v] ? p.totals[0]++ : -1;
  for (long f = 0; f < p.F; ++f) p.face_map[f] = p.keep_face[f] ? p.totals[1]++ : -1;
}

void be_mesh_select(const MeshSelect& p, cnr_stream s) {
  const int thr = meshcc_threshold(p.min_faces, p.min_ratio, p.summary[3]);
  for (long v = 0; v < p.V; ++v) p.keep_vertex[v] = meshcc_keep_vertex(p, v, thr);
  for (long f = 0; f < p.F; ++f) p.keep_face[f] = meshcc_keep_face(p, f, thr);
  mesh_keep_scan({p.keep_vertex, p.keep_face, p.V, p.F, p.vertex_map, p.face_map, p.totals}, s);
}

void be_mesh_compact(const MeshCompact& p, cnr_stream) {
  for (long v = 0; v < p.V; ++v) meshcc_compact_vertex(p, v);
  for (long f = 0; f < p.F; ++f) meshcc_compact_face(p, f);
}

// ---- cnr_surface.hip
// twins of surf_area_kernel / surf_cdf_scan_kernel: the same surf_area_bits / surf_weight, the integer max and the prefix sums in face order
void be_mesh_area_cdf(const MeshAreaCdf& p, cnr_stream) {
  unsigned long long amax = 0ull, total = 0ull;
  long long zero = 0, invalid = 0;
  for (long f = 0; f < p.F; ++f) {
    p.cdf[f] = surf_area_bits(p, f);
    if (p.cdf[f] != kSurfInvalid) amax = std::max(amax, p.cdf[f]);
  }
  for (long f = 0; f < p.F; ++f) {
    const unsigned long long bits = p.cdf[f], w = surf_weight(bits, (unsigned)amax);
    total += w; zero += w == 0ull; invalid += bits == kSurfInvalid;
    p.cdf[f] = total;
  }
  p.summary[0] = (long long)total; p.summary[1] = zero; p.summary[2] = invalid; p.summary[3] = (long long)amax;
}
void be_mesh_sample(const MeshSample& p, cnr_stream) {
#pragma omp parallel for schedule(static)
  for (long i = 0; i < p.n; ++i) surf_sample(p, i);
}
// twin of surf_dist_kernel / surf_finish_kernel: the records of all faces once, then the same surf_dist2 / nn_update / nn_key over the whole
// face range in ascending order, one query per iteration
void be_point_mesh_distance(const PointMeshDist& p, cnr_stream) {
  std::vector<SurfTri> rec((size_t)p.F);
#pragma omp parallel for schedule(static)
  for (long f = 0; f < p.F; ++f) rec[(size_t)f] = surf_record(p.vertices, p.V, p.triangles + f * 3);
#pragma omp parallel for schedule(static)
  for (long i = 0; i < p.n; ++i) {
    const float qx = p.query[i * 3], qy = p.query[i * 3 + 1], qz = p.query[i * 3 + 2];
    float best = INFINITY;
    int besti = -1;
    for (long f = 0; f < p.F; ++f) nn_update(surf_dist2(rec[(size_t)f], qx, qy, qz), (int)f, best, besti);
    p.keys[i] = nn_key(best, besti);
    surf_finish(p, i);
  }
}

// ---- cnr_cull.hip
// twins of cull_pack_kernel / cull_hdilate_kernel / cull_vdilate_kernel: the same three word functions, one word after the other
void be_mask_dilate(const MaskDilate& p, cnr_stream) {
  const long rows = p.n * p.H;
#pragma omp parallel for schedule(static)
  for (long row = 0; row < rows; ++row)
    for (int k = 0; k < p.Wq; ++k) p.bits[row * p.Wq + k] = cull_pack_word(p.masks + row * p.W, p.W, k);
#pragma omp parallel for schedule(static)
  for (long row = 0; row < rows; ++row)
    for (int k = 0; k < p.Wq; ++k) p.row_bits[row * p.Wq + k] = cull_hdilate_word(p.bits + row * p.Wq, p.Wq, p.W, k, p.radius);
#pragma omp parallel for schedule(static)
  for (long row = 0; row < rows; ++row) {
    const long img = row / p.H;
    const int j = (int)(row - img * p.H);
    for (int k = 0; k < p.Wq; ++k) p.bits[row * p.Wq + k] = cull_vdilate_word(p.row_bits + img * p.H * p.Wq, p.H, p.Wq, j, k, p.radius);
  }
}

// twin of cull_votes_kernel: the cameras once, then cull_vote per (vertex, view), a vertex's four counts carried through its views
void be_mesh_view_votes(const MeshViewVotes& p, cnr_stream) {
  std::vector<RasterCam> cams((size_t)p.n_views);
  for (long n = 0; n < p.n_views; ++n) cams[(size_t)n] = raster_cam_of(p.c2w + n * 16, p.focal + n * 2, p.origin, p.radius, p.H, p.W);
  const float tol1 = 1.0f + p.depth_tol;
#pragma omp parallel for schedule(static)
  for (long v = 0; v < p.V; ++v) {
    int c[4] = {0, 0, 0, 0};
    for (long n = 0; n < p.n_views; ++n)
      cull_vote(cams[(size_t)n], p.vertices + v * 3, p.opengl, p.z_near, p.H, p.W, p.Wq, p.mask_bits ? p.mask_bits + n * p.H * p.Wq : nullptr,
                p.depth ? p.depth + n * p.H * p.W : nullptr, tol1, c);
    for (int k = 0; k < 4; ++k) p.counts[v * 4 + k] += c[k];
  }
}

// twins of cull_clear_kernel / cull_faces_kernel, then the shared scan
void be_mesh_cull_select(const MeshCullSelect& p, cnr_stream s) {
  p.dropped[0] = 0;
  for (long v = 0; v < p.V; ++v) p.keep_vertex[v] = 0;
  for (long f = 0; f < p.F; ++f) {
    const int k = cull_face(p, f);
    p.keep_face[f] = k > 0 ? 1 : 0;
    if (k < 0) ++p.dropped[0];
    if (k > 0) cull_mark(p, f);
  }
  mesh_keep_scan({p.keep_vertex, p.keep_face, p.V, p.F, p.vertex_map, p.face_map, p.totals}, s);
}

// ---- cnr_register.hip
// twin of icp_move_kernel / icp_moments_kernel / icp_solve_kernel: the same icp_move / icp_pair / icp_finish; the chunk tree x[j] += x[j + h],
// h = 128 .. 1, over 256 rows padded with zeros, then the chunks' rows added in chunk order from +0.0
void be_icp_clear(void* p, size_t bytes, cnr_stream) { memset(p, 0, bytes); }
void be_icp_step(const IcpStep& p, cnr_stream s) {
  const IcpMap k = icp_map(p.transform);
#pragma omp parallel for schedule(static)
  for (long i = 0; i < p.n; ++i) icp_move(p, k, i);
  icp_search(p, s);
  const long chunks = (p.n + kIcpChunk - 1) / kIcpChunk;
  long long n_inliers = 0, n_changed = 0;
#pragma omp parallel for schedule(static) reduction(+ : n_inliers, n_changed)
  for (long b = 0; b < chunks; ++b) {
    std::vector<double> x((size_t)kIcpChunk * kIcpTerms, 0.0);
    for (int j = 0; j < kIcpChunk && b * kIcpChunk + j < p.n; ++j) {
      int inlier, changed;
      icp_pair(p, b * kIcpChunk + j, &x[(size_t)j * kIcpTerms], &inlier, &changed);
      n_inliers += inlier; n_changed += changed;
    }
    for (int h = kIcpChunk / 2; h >= 1; h >>= 1)
      for (int j = 0; j < h; ++j)
        for (int c = 0; c < kIcpTerms; ++c) x[(size_t)j * kIcpTerms + c] += x[(size_t)(j + h) * kIcpTerms + c];
    for (int c = 0; c < kIcpTerms; ++c) p.partials[b * kIcpTerms + c] = x[c];
  }
  double S[kIcpTerms];
  for (int c = 0; c < kIcpTerms; ++c) {
    S[c] = 0.0;
    for (long b = 0; b < chunks; ++b) S[c] += p.partials[b * kIcpTerms + c];
  }
  icp_finish(p, S, n_inliers, n_changed);
}

}  // namespace cnr
