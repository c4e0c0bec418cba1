// The plain linear op and the NeRF++ background network built from the same layer launches, with the sampling and compositing of the
// samples outside the unit sphere (cnr_outside_z*, cnr_composite_background_*).  Nothing here uses the render model or its contexts.
#include "cnr_plan.h"
#include "cnr_bg.h"

namespace cnr {

// ------------------------------------------------------------------------------------------------
// one plain fully-connected layer y = act(x W^T + b) and its backward on the layer / weight-gradient kernels of the render path:
// the NeRF++ background stack (fields.py:192-274) is a chain of these (color-neus_amd/background.py)
// ------------------------------------------------------------------------------------------------
struct LinearOp { Lin q; int ldx = 0, ldy = 0; float *xp = nullptr, *yp = nullptr, *gp = nullptr, *dxp = nullptr; DwPool dw; int nchunk = 1; };

static int linear_check(long n, int k, int n_out) {
  if (n <= 0 || k < 1 || n_out < 1 || k > 4096 || n_out > 4096) return fail("linear: need n > 0, 1 <= k, n_out <= 4096");
  return 0;
}
static void layout_linear(long n, int k, int n_out, bool backward, Arena& a, LinearOp& op) {
  Lin& q = op.q;
  q.n = n_out; q.k_ref = k; identity_seg(q); q.finish_dims(); q.wn = false;
  q.name = "linear"; q.p_v = 0; q.p_b = 1;   // (the op's two-entry parameter lists: {W, b} and {dW, db})
  place_lin(q, a);
  op.ldx = round_up(k, 16); op.ldy = round_up(n_out, 16);
  op.xp = a.f((size_t)n * op.ldx);
  op.yp = a.f((size_t)n * op.ldy);
  if (backward) {
    op.gp = a.f((size_t)n * op.ldy);
    op.dxp = a.f((size_t)n * op.ldx);
    op.nchunk = dw_chunks(n);
    op.dw.place(a, DwPool::region_floats(q, op.nchunk));
  }
  place_slack(a);
}

static void linear_prep(LinearOp& op, const float* W, const float* b, cnr_stream s) {
  const float* params[2] = {W, b};
  prep_layers({&op.q}, params, s);
}

// compact [n][c] -> padded [n][ld] with zero pad columns
static void pad_in(float* dst, int ld, const float* src, int c, long n, cnr_stream s) {
  be_copy_cols(dst, ld, src, c, c, n, s);
  be_zero_cols(dst, ld, c, ld, n, s);
}

// ------------------------------------------------------------------------------------------------
// N_OUTSIDE > 0: the NeRF++ background network (NeRF, fields.py:192-274) evaluated by render_core_outside (NeuS.py:95-134) as ONE library
// call each way: positional encodings, the D x W ReLU stack with its skip concat, density and feature heads, the view branch, density ->
// alpha and sigmoid(rgb); backward through all of it down to the rays and the sample positions.  Layer launches: the render path's layer /
// weight-gradient kernels (whatever shape fits: the 340- and 283-wide layers take the FP32-MFMA forms).
// Internal input order of the skip layer is [h | e] (the reference concatenates [e | h], fields.py:252-253: a column permutation of its
// weights, like colour layer 0), so that the layer in front of it writes h into an aligned position and the backward launch's split
// epilogue separates the two cotangents.
// ------------------------------------------------------------------------------------------------
struct NerfModel {
  cnr_nerf_config c;
  int D, W, ne, nv;                   // depth, width, PE widths (4 + 8 multires, 3 + 6 multires_view)
  std::vector<Lin> pts;               // D layers
  Lin alpha, feat, view, rgb;
  std::vector<ParamInfo> params;
  int skip_at = -1;                   // the layer AFTER which [e | h] is concatenated (input of layer skip_at + 1), -1: none
};
static int build_nerf(const cnr_nerf_config* cfg, NerfModel& m) {
  if (!cfg) return fail("null nerf config");
  m.c = *cfg;
  m.D = cfg->D; m.W = cfg->W;
  if (m.D < 2 || m.D > kMaxLayers - 1 || m.W < 32 || m.W > 256 || m.W % 32) return fail("nerf: D in [2, %d], W a multiple of 32 in [32, 256]", kMaxLayers - 1);
  if (cfg->multires < 0 || cfg->multires > 10 || cfg->multires_view < 0 || cfg->multires_view > 4) return fail("nerf: multires <= 10, multires_view <= 4");
  m.ne = 4 + 8 * cfg->multires; m.nv = 3 + 6 * cfg->multires_view;
  int nskip = 0;
  for (int i = 0; i < m.D - 1; ++i) if ((cfg->skip_mask >> i) & 1) { m.skip_at = i; ++nskip; }
  if (nskip > 1 || (cfg->skip_mask >> (m.D - 1)) != 0) return fail("nerf: at most one skip connection, below the last layer");
  m.pts.resize(m.D);
  for (int i = 0; i < m.D; ++i) {
    Lin& q = m.pts[i];
    q.n = m.W;
    if (i == 0) { q.k_ref = m.ne; identity_seg(q); }
    else if (i - 1 == m.skip_at) {      // reference input [e | h] -> internal [h | e]
      q.k_ref = m.W + m.ne; q.k_int = q.k_ref; q.nseg = 2;
      q.seg[0] = {0, m.ne, m.W}; q.seg[1] = {m.W, 0, m.ne};
    } else { q.k_ref = m.W; identity_seg(q); }
    q.finish_dims();
    add_weight_bias(m.params, q, "pts_linears." + std::to_string(i));
  }
  // nn.Module registration order of NeRF.__init__ (fields.py:215-231): pts_linears, views_linears, feature_linear, alpha_linear, rgb_linear
  m.view.n = m.W / 2; m.view.k_ref = m.W + m.nv; identity_seg(m.view); m.view.finish_dims(); add_weight_bias(m.params, m.view, "views_linears.0");
  m.feat.n = m.W; m.feat.k_ref = m.W; identity_seg(m.feat); m.feat.finish_dims(); add_weight_bias(m.params, m.feat, "feature_linear");
  m.alpha.n = 1; m.alpha.k_ref = m.W; identity_seg(m.alpha); m.alpha.finish_dims(); add_weight_bias(m.params, m.alpha, "alpha_linear");
  m.rgb.n = 3; m.rgb.k_ref = m.W / 2; identity_seg(m.rgb); m.rgb.finish_dims(); add_weight_bias(m.params, m.rgb, "rgb_linear");
  return 0;
}
struct NerfCtx {       // forward-saved state of one background call
  int lde, ldxh, ldfv;
  float *E, *XH, *FV, *HV, *dens, *dist;
  std::vector<float*> H;             // output of pts layer i ([n][W]); H[skip_at] aliases XH (row stride ldxh)
};
static void nerf_layers(NerfModel& m, std::vector<Lin*>& all) {
  for (auto& q : m.pts) all.push_back(&q);
  all.push_back(&m.view); all.push_back(&m.feat); all.push_back(&m.alpha); all.push_back(&m.rgb);
}
static void layout_nerf(NerfModel& m, long n, Arena& a, NerfCtx& x) {
  std::vector<Lin*> all;
  nerf_layers(m, all);
  for (Lin* q : all) place_lin(*q, a);
  x.lde = round_up(m.ne, 16);
  x.ldxh = round_up(m.W + m.ne, 16);
  x.ldfv = round_up(m.W + m.nv, 16);
  x.E = a.f((size_t)n * x.lde);
  x.XH = m.skip_at >= 0 ? a.f((size_t)n * x.ldxh) : nullptr;
  x.FV = a.f((size_t)n * x.ldfv);
  x.HV = a.f((size_t)n * (m.W / 2));
  x.dens = a.f(n);
  x.dist = a.f(n);
  x.H.resize(m.D);
  for (int i = 0; i < m.D; ++i) x.H[i] = (i == m.skip_at) ? x.XH : a.f((size_t)n * m.W);
  place_slack(a);
}
static int nerf_h_ld(const NerfModel& m, const NerfCtx& x, int i) { return i == m.skip_at ? x.ldxh : m.W; }
static void nerf_prep(NerfModel& m, const float* const* params, cnr_stream s) {
  std::vector<Lin*> all;
  nerf_layers(m, all);
  prep_layers(all, params, s);
}
struct NerfBwd { float *dRGB, *dDens, *dDist, *DHV, *dF, *dVE, *T, *dEs, *dE0, *dp; std::vector<float*> DZ; DwPool dw; int nchunk; };
static void layout_nerf_bwd(NerfModel& m, const NerfCtx& x, long n, Arena& a, NerfBwd& b) {
  b.dRGB = a.f((size_t)n * 16); b.dDens = a.f((size_t)n * 16); b.dDist = a.f(n);
  b.DHV = a.f((size_t)n * (m.W / 2)); b.dF = a.f((size_t)n * m.W); b.dVE = a.f((size_t)n * 32);
  b.T = a.f((size_t)n * m.W); b.dEs = m.skip_at >= 0 ? a.f((size_t)n * x.lde) : nullptr; b.dE0 = a.f((size_t)n * x.lde); b.dp = a.f((size_t)n * 8);
  b.DZ.resize(m.D);
  for (int i = 0; i < m.D; ++i) b.DZ[i] = a.f((size_t)n * m.W);
  b.nchunk = dw_chunks(n);
  std::vector<Lin*> all;
  nerf_layers(m, all);
  size_t tot = 0;
  for (Lin* q : all) tot += DwPool::region_floats(*q, b.nchunk);
  b.dw.place(a, tot);
  place_slack(a);
}
// weight + bias gradient of one background layer: dW = sum_pt X (x) Y, db = column sums of X; queued for one batched finish
// (no row scales: dw_main_tile keeps the tiles off the split-f16 form)
static int nerf_dw(const Lin& q, const float* X, int ldx, const float* Y, int ldy, long n, NerfBwd& b, const float* const* params,
                   float* const* dP, cnr_stream s) {
  DwGemm d;
  d.npairs = 1; d.P = n; d.X[0] = direct_view(X, ldx); d.Y[0] = direct_view(Y, ldy);
  return plain_dw(b.dw, q, d, b.nchunk, b.nchunk, params, dP, s);
}
}  // namespace cnr

using namespace cnr;

extern "C" {

size_t cnr_linear_scratch_bytes(int64_t n, int32_t k, int32_t n_out, int32_t backward) {
  LinearOp op;
  if (linear_check(n, k, n_out)) return 0;
  return layout_size(nullptr, [&](Arena& a) { layout_linear(n, k, n_out, backward != 0, a, op); });
}

int cnr_linear_forward(const float* x, int64_t n, int32_t k, const float* W, const float* b, int32_t n_out, int32_t relu, float* y, void* scratch,
                       size_t scratch_bytes, void* stream) {
  if (!x || !W || !y || !scratch) return fail("null argument");
  cnr_stream s = (cnr_stream)stream;
  LinearOp op;
  if (linear_check(n, k, n_out)) return -1;
  if (layout_checked("linear scratch", scratch, scratch_bytes, [&](Arena& a) { layout_linear(n, k, n_out, false, a, op); })) return -1;
  Lin& q = op.q;
  linear_prep(op, W, b, s);
  pad_in(op.xp, op.ldx, x, k, n, s);
  LayerGemm g = fwd_gemm(q, n);
  g.A = direct_view(op.xp, op.ldx);
  g.E.kind = relu ? EK_RELU : EK_STORE; g.E.bias = b ? q.bias : nullptr; g.E.n_out = q.n; g.E.o1 = op.yp; g.E.ld1 = op.ldy;
  be_layer_gemm(g, s);
  be_copy_cols(y, n_out, op.yp, op.ldy, n_out, n, s);
  return check_backend("linear_forward");
}

int cnr_linear_backward(const float* x, const float* y, const float* dy, int64_t n, int32_t k, const float* W, int32_t n_out, int32_t relu,
                        float* dx, float* dW, float* db, void* scratch, size_t scratch_bytes, void* stream) {
  if (!x || !dy || !W || !dW || !scratch || (relu && !y)) return fail("null argument");
  cnr_stream s = (cnr_stream)stream;
  LinearOp op;
  if (linear_check(n, k, n_out)) return -1;
  if (layout_checked("linear scratch", scratch, scratch_bytes, [&](Arena& a) { layout_linear(n, k, n_out, true, a, op); })) return -1;
  Lin& q = op.q;
  linear_prep(op, W, nullptr, s);
  pad_in(op.xp, op.ldx, x, k, n, s);
  pad_in(op.gp, op.ldy, dy, n_out, n, s);
  View dz = direct_view(op.gp, op.ldy);    // cotangent of the pre-activation: dy gated by the ReLU output
  if (relu) { pad_in(op.yp, op.ldy, y, n_out, n, s); dz.kind = VK_RELUGATE; dz.b = op.yp; dz.ldb = op.ldy; }
  // weight and bias gradients: dW[n_out][k] = sum_pt dz (x) x, db = column sums of dz
  // (the GEMM forms the column sums whether or not the caller wants db; the reduction reads them only for a db)
  const float* params[2] = {W, nullptr};
  float* dparams[2] = {dW, db};
  const DwRegion r = op.dw.take(q, op.nchunk);
  if (!r.part) return -1;
  DwGemm d;
  d.npairs = 1; d.P = n; d.X[0] = dz; d.Y[0] = direct_view(op.xp, op.ldx);
  dw_into_region(q, d, r, 0, op.nchunk, n, true, s);
  op.dw.finish(q, r, op.nchunk, db ? op.nchunk : 0, params, dparams);
  op.dw.flush(s);   // (before the dx launch)
  if (dx) {
    LayerGemm g = bwd_gemm(q, n);
    g.A = dz;
    g.E.kind = EK_STORE; g.E.n_out = q.k_int; g.E.o1 = op.dxp; g.E.ld1 = op.ldx;
    be_layer_gemm(g, s);
    be_copy_cols(dx, k, op.dxp, op.ldx, k, n, s);
  }
  return check_backend("linear_backward");
}

// ---- N_OUTSIDE > 0 ------------------------------------------------------------------------------------------------------------------
int cnr_nerf_param_count(const cnr_nerf_config* cfg) {
  NerfModel m;
  if (build_nerf(cfg, m)) return -1;
  return (int)m.params.size();
}
int cnr_nerf_param_info(const cnr_nerf_config* cfg, int index, char* name, int name_len, int* rows, int* cols) {
  NerfModel m;
  return build_nerf(cfg, m) ? -1 : param_info(m.params, index, name, name_len, rows, cols);
}
int cnr_outside_z(const float* far_, const float* t_rand, const float* z_vals, int64_t n_rays, int32_t n_z, int32_t n_outside, int32_t n_samples,
                  float* z_feed, int32_t* src, void* stream) {
  if (!far_ || !z_vals || !z_feed || !src) return fail("null argument");
  if (n_rays <= 0 || n_z < 1 || n_outside < 1 || n_outside > kMaxOutside || n_z + n_outside > kMaxRaySamples || n_samples < 1)
    return fail("outside_z: need n_rays > 0, 1 <= n_outside <= %d, n_z + n_outside <= %d", kMaxOutside, kMaxRaySamples);
  OutsideZ p;
  p.R = n_rays; p.M = n_z; p.n_out = n_outside; p.n_samples = n_samples; p.far_ = far_; p.t_rand = t_rand; p.z = z_vals; p.z_feed = z_feed; p.src = src;
  be_outside_z(p, (cnr_stream)stream);
  return check_backend("outside_z");
}
int cnr_outside_z_backward(const float* t_rand, const int32_t* src, const float* d_z_feed, int64_t n_rays, int32_t n_z, int32_t n_outside,
                           int32_t n_samples, float* d_far, float* d_z, void* stream) {
  if (!src || !d_z_feed || !d_far) return fail("null argument");
  if (n_rays <= 0 || n_z < 1 || n_outside < 1 || n_outside > kMaxOutside || n_z + n_outside > kMaxRaySamples) return fail("outside_z_backward: bad sizes");
  OutsideZBwd p;
  p.R = n_rays; p.M = n_z; p.n_out = n_outside; p.n_samples = n_samples; p.t_rand = t_rand; p.src = src; p.d_z_feed = d_z_feed; p.d_far = d_far; p.d_z = d_z;
  be_outside_z_bwd(p, (cnr_stream)stream);
  return check_backend("outside_z_backward");
}
size_t cnr_background_ctx_bytes(const cnr_nerf_config* cfg, int64_t n_rays, int32_t n_feed) {
  NerfModel m;
  if (build_nerf(cfg, m) || n_rays <= 0 || n_feed < 1) return 0;
  NerfCtx x;
  return layout_size(nullptr, [&](Arena& a) { layout_nerf(m, n_rays * n_feed, a, x); });
}
size_t cnr_background_bwd_scratch_bytes(const cnr_nerf_config* cfg, int64_t n_rays, int32_t n_feed) {
  NerfModel m;
  if (build_nerf(cfg, m) || n_rays <= 0 || n_feed < 1) return 0;
  NerfCtx x;
  NerfBwd b;
  layout_size(nullptr, [&](Arena& a) { layout_nerf(m, n_rays * n_feed, a, x); });
  return layout_size(nullptr, [&](Arena& a) { layout_nerf_bwd(m, x, n_rays * n_feed, a, b); });
}
int cnr_background_forward(const cnr_nerf_config* cfg, const float* const* params, const float* rays_o, const float* rays_d, const float* z_feed,
                           int64_t n_rays, int32_t n_feed, float sample_dist, float* alpha, float* color, void* ctx, size_t ctx_bytes, void* stream) {
  cnr_stream s = (cnr_stream)stream;
  const long R = n_rays;
  const int MF = n_feed;
  NerfModel m;
  if (build_nerf(cfg, m)) return -1;
  if (!params || !rays_o || !rays_d || !z_feed || !alpha || !color || !ctx) return fail("null argument");
  if (R <= 0 || MF < 1 || MF > kMaxRaySamples) return fail("background: n_rays > 0, 1 <= samples per ray <= %d", kMaxRaySamples);
  const long n = R * MF;
  NerfCtx x;
  if (layout_checked("background context", ctx, ctx_bytes, [&](Arena& a) { layout_nerf(m, n, a, x); })) return -1;
  nerf_prep(m, params, s);
  BgEmbed e;
  e.o = rays_o; e.d = rays_d; e.z_feed = z_feed; e.R = R; e.MF = MF; e.sample_dist = sample_dist; e.multires = cfg->multires; e.multires_view = cfg->multires_view;
  e.E = x.E; e.lde = x.lde; e.XH = x.XH; e.ldxh = x.ldxh; e.xh_off = m.W; e.FV = x.FV; e.ldfv = x.ldfv; e.fv_off = m.W; e.dist = x.dist;
  be_bg_embed(e, s);
  for (int i = 0; i < m.D; ++i) {
    const Lin& q = m.pts[i];
    LayerGemm g = fwd_gemm(q, n);
    g.A = i == 0 ? direct_view(x.E, x.lde) : direct_view(x.H[i - 1], nerf_h_ld(m, x, i - 1));
    g.E.kind = EK_RELU; g.E.bias = q.bias; g.E.n_out = q.n; g.E.o1 = x.H[i]; g.E.ld1 = nerf_h_ld(m, x, i);
    be_layer_gemm(g, s);
  }
  const float* hl = x.H[m.D - 1];
  const int ldh = nerf_h_ld(m, x, m.D - 1);
  {
    LayerGemm g = fwd_gemm(m.alpha, n);
    g.A = direct_view(hl, ldh); g.Wp = nullptr;
    g.E.kind = EK_STORE; g.E.bias = m.alpha.bias; g.E.n_out = m.alpha.n; g.E.o1 = x.dens; g.E.ld1 = 1;
    be_layer_gemm(g, s);
    LayerGemm f = fwd_gemm(m.feat, n);
    f.A = direct_view(hl, ldh);
    f.E.kind = EK_STORE; f.E.bias = m.feat.bias; f.E.n_out = m.feat.n; f.E.o1 = x.FV; f.E.ld1 = x.ldfv;
    be_layer_gemm(f, s);
    LayerGemm v = fwd_gemm(m.view, n);
    v.A = direct_view(x.FV, x.ldfv);
    v.E.kind = EK_RELU; v.E.bias = m.view.bias; v.E.n_out = m.view.n; v.E.o1 = x.HV; v.E.ld1 = m.W / 2;
    be_layer_gemm(v, s);
    LayerGemm c = fwd_gemm(m.rgb, n);
    c.A = direct_view(x.HV, m.W / 2); c.Wp = nullptr;
    c.E.kind = EK_SIGMOID; c.E.bias = m.rgb.bias; c.E.n_out = m.rgb.n; c.E.o1 = color; c.E.ld1 = 3;
    be_layer_gemm(c, s);
  }
  BgAlpha ba;
  ba.n = n; ba.density = x.dens; ba.dist = x.dist; ba.alpha = alpha;
  be_bg_alpha(ba, s);
  return check_backend("background_forward");
}
int cnr_background_backward(const cnr_nerf_config* cfg, const float* const* params, const float* rays_o, const float* rays_d, const float* z_feed,
                            int64_t n_rays, int32_t n_feed, float sample_dist, const void* ctx, size_t ctx_bytes, const float* color,
                            const float* d_alpha, const float* d_color, float* const* dP, float* d_rays_o, float* d_rays_d, float* d_z_feed,
                            void* scratch, size_t scratch_bytes, void* stream) {
  cnr_stream s = (cnr_stream)stream;
  const long R = n_rays;
  const int MF = n_feed;
  NerfModel m;
  if (build_nerf(cfg, m)) return -1;
  if (!params || !rays_o || !rays_d || !z_feed || !ctx || !color || !dP || !d_rays_o || !d_rays_d || !d_z_feed || !scratch) return fail("null argument");
  const long n = R * MF;
  NerfCtx x;
  NerfBwd b;
  if (layout_checked("background context", const_cast<void*>(ctx), ctx_bytes, [&](Arena& a) { layout_nerf(m, n, a, x); })) return -1;
  if (layout_checked("background scratch", scratch, scratch_bytes, [&](Arena& a) { layout_nerf_bwd(m, x, n, a, b); })) return -1;
  BgHeadsBwd hb;
  hb.n = n; hb.density = x.dens; hb.dist = x.dist; hb.rgb = color; hb.d_alpha = d_alpha; hb.d_rgb = d_color;
  hb.d_density = b.dDens; hb.ldd = 16; hb.d_rgb_pre = b.dRGB; hb.ldr = 16; hb.d_dist = b.dDist;
  be_bg_heads_bwd(hb, s);
  const float* hl = x.H[m.D - 1];
  const int ldh = nerf_h_ld(m, x, m.D - 1);
  // rgb head: dW, cotangent of the view layer's pre-activation (ReLU mask)
  if (nerf_dw(m.rgb, b.dRGB, 16, x.HV, m.W / 2, n, b, params, dP, s)) return -1;
  {
    LayerGemm g = bwd_gemm(m.rgb, n);
    g.A = direct_view(b.dRGB, 16); g.Wp = nullptr;
    g.E.kind = EK_RELU_MASK; g.E.n_out = m.rgb.k_int; g.E.o1 = b.DHV; g.E.ld1 = m.W / 2; g.E.aux = x.HV; g.E.ldaux = m.W / 2;
    be_layer_gemm(g, s);
  }
  // view layer: dW, cotangent of [feature | PE(view)]
  if (nerf_dw(m.view, b.DHV, m.W / 2, x.FV, x.ldfv, n, b, params, dP, s)) return -1;
  {
    LayerGemm g = bwd_gemm(m.view, n);
    g.A = direct_view(b.DHV, m.W / 2);
    g.E.kind = EK_SPLIT; g.E.n_out = m.view.k_int; g.E.split = m.W; g.E.o1 = b.dF; g.E.ld1 = m.W; g.E.o2 = b.dVE; g.E.ld2 = 32;
    be_layer_gemm(g, s);
  }
  be_zero_cols(b.dVE, 32, m.nv, 32, n, s);
  // feature layer and density head: both read the last hidden activation
  if (nerf_dw(m.feat, b.dF, m.W, hl, ldh, n, b, params, dP, s)) return -1;
  if (nerf_dw(m.alpha, b.dDens, 16, hl, ldh, n, b, params, dP, s)) return -1;
  {
    LayerGemm g = bwd_gemm(m.feat, n);
    g.A = direct_view(b.dF, m.W);
    g.E.kind = EK_STORE; g.E.n_out = m.feat.k_int; g.E.o1 = b.T; g.E.ld1 = m.W;
    be_layer_gemm(g, s);
  }
  if (ldh != m.W) return fail("background: the last layer cannot carry the skip concat");
  BgJoin bj;
  bj.n = n; bj.W = m.W; bj.T = b.T; bj.H = hl; bj.d_density = b.dDens; bj.ldd = 16; bj.w_alpha = m.alpha.W; bj.dZ = b.DZ[m.D - 1];
  be_bg_join(bj, s);
  for (int i = m.D - 1; i >= 0; --i) {
    const Lin& q = m.pts[i];
    const float* in = i == 0 ? x.E : x.H[i - 1];
    const int ld_in = i == 0 ? x.lde : nerf_h_ld(m, x, i - 1);
    if (nerf_dw(q, b.DZ[i], m.W, in, ld_in, n, b, params, dP, s)) return -1;
    LayerGemm g = bwd_gemm(q, n);
    g.A = direct_view(b.DZ[i], m.W); g.E.n_out = q.k_int;
    if (i == 0) { g.E.kind = EK_STORE; g.E.o1 = b.dE0; g.E.ld1 = x.lde; }
    else if (i - 1 == m.skip_at) {    // input [h | e]: h part through the ReLU mask of the layer below, e part to its own buffer
      g.E.kind = EK_RELU_MASK; g.E.split = m.W; g.E.o1 = b.DZ[i - 1]; g.E.ld1 = m.W; g.E.aux = x.H[i - 1]; g.E.ldaux = ld_in; g.E.o2 = b.dEs; g.E.ld2 = x.lde;
    } else { g.E.kind = EK_RELU_MASK; g.E.split = 1 << 30; g.E.o1 = b.DZ[i - 1]; g.E.ld1 = m.W; g.E.aux = x.H[i - 1]; g.E.ldaux = ld_in; }
    be_layer_gemm(g, s);
  }
  be_zero_cols(b.dE0, x.lde, m.ne, x.lde, n, s);
  if (b.dEs) be_zero_cols(b.dEs, x.lde, m.ne, x.lde, n, s);
  b.dw.flush(s);
  BgEmbedBwd eb;
  eb.o = rays_o; eb.d = rays_d; eb.z_feed = z_feed; eb.R = R; eb.MF = MF; eb.sample_dist = sample_dist; eb.multires = cfg->multires; eb.multires_view = cfg->multires_view;
  eb.dE0 = b.dE0; eb.lde0 = x.lde; eb.dE1 = b.dEs; eb.lde1 = x.lde; eb.dVE = b.dVE; eb.ldve = 32; eb.dp = b.dp;
  be_bg_embed_bwd(eb, s);
  BgRaysBwd rb;
  rb.d = rays_d; rb.z_feed = z_feed; rb.R = R; rb.MF = MF; rb.sample_dist = sample_dist; rb.dp = b.dp; rb.d_dist = b.dDist;
  rb.d_o = d_rays_o; rb.d_d = d_rays_d; rb.d_z_feed = d_z_feed;
  be_memset_zero(d_z_feed, (size_t)n * sizeof(float), s);
  be_bg_rays_bwd(rb, s);
  return check_backend("background_backward");
}
static int composite_bg_args(const cnr_bg_composite_in* in, const cnr_render_outputs* out, CompositeBg& p) {
  if (!in || !out) return fail("null argument");
  if (in->n_rays <= 0 || in->n_z < 1 || in->n_feed < in->n_z || in->n_feed > kMaxRaySamples) return fail("composite_background: bad sample counts");
  if (!in->rays_o || !in->rays_d || !in->z_vals || !in->z_feed || !in->sdf_samples || !in->gradients || !in->color_samples || !in->bg_alpha ||
      !in->bg_color || !in->variance) return fail("composite_background: missing input");
  if (!out->color_fine || !out->s_val || !out->cdf_fine || !out->weight_sum || !out->weight_max || !out->weights || !out->inside_sphere ||
      !out->depth || !out->gradient_error || !out->eik_sums) return fail("composite_background: missing output buffer");
  if (in->global_color_samples && !out->global_color) return fail("composite_background: global_color buffer missing");
  p.o = in->rays_o; p.d = in->rays_d; p.z = in->z_vals; p.z_feed = in->z_feed; p.R = in->n_rays; p.M = in->n_z; p.MF = in->n_feed; p.sample_dist = in->sample_dist;
  p.sdf = in->sdf_samples; p.g = in->gradients; p.color = in->color_samples; p.gcolor = in->global_color_samples; p.bg_alpha = in->bg_alpha; p.bg_color = in->bg_color;
  p.variance = in->variance; p.cos_anneal = in->cos_anneal_ratio; p.background_rgb = in->background_rgb;
  p.color_fine = out->color_fine; p.s_val = out->s_val; p.cdf_fine = out->cdf_fine; p.weight_sum = out->weight_sum; p.weight_max = out->weight_max;
  p.weights = out->weights; p.inside_sphere = out->inside_sphere; p.depth = out->depth; p.global_color = in->global_color_samples ? out->global_color : nullptr;
  p.eik_partial = nullptr;
  return 0;
}
size_t cnr_composite_background_scratch_bytes(int64_t n_rays) { return n_rays > 0 ? round_up_sz((size_t)n_rays * 2 * sizeof(float), 256) + 256 : 0; }
int cnr_composite_background_forward(const cnr_bg_composite_in* in, const cnr_render_outputs* out, void* scratch, size_t scratch_bytes, void* stream) {
  CompositeBg p;
  if (composite_bg_args(in, out, p)) return -1;
  if (!scratch || scratch_bytes < cnr_composite_background_scratch_bytes(in->n_rays)) return fail("composite_background: scratch too small");
  cnr_stream s = (cnr_stream)stream;
  Arena a(scratch);
  p.eik_partial = a.f((size_t)in->n_rays * 2);
  float* sums = a.f(64);
  be_composite_bg(p, s);
  ReduceEik re;
  re.partial = p.eik_partial; re.R = in->n_rays; re.sums = sums; re.sums_out = out->eik_sums; re.gradient_error = out->gradient_error;
  be_reduce_eik(re, s);
  return check_backend("composite_background_forward");
}
int cnr_composite_background_backward(const cnr_bg_composite_in* in, const cnr_render_outputs* out, const cnr_render_out_grads* go,
                                      const cnr_bg_composite_grads* gi, void* scratch, size_t scratch_bytes, void* stream) {
  CompositeBgBwd b;
  if (composite_bg_args(in, out, b.f)) return -1;
  if (!go || !gi || !scratch || scratch_bytes < cnr_composite_background_scratch_bytes(in->n_rays)) return fail("composite_background_backward: null argument / scratch too small");
  if (!gi->d_sdf_samples || !gi->d_gradients || !gi->d_color_samples || !gi->d_bg_alpha || !gi->d_bg_color || !gi->d_variance || !gi->d_rays_d || !gi->d_z_vals ||
      !gi->d_z_feed || (in->global_color_samples && !gi->d_global_color_samples)) return fail("composite_background_backward: missing gradient buffer");
  cnr_stream s = (cnr_stream)stream;
  Arena a(scratch);
  float* dinvs = a.f((size_t)in->n_rays * 2);
  b.d_color_fine = go->color_fine; b.d_s_val = go->s_val; b.d_cdf = go->cdf_fine; b.d_weight_sum = go->weight_sum; b.d_weight_max = go->weight_max;
  b.d_weights = go->weights; b.d_gradient_error = go->gradient_error; b.d_depth = go->depth; b.d_global_color = go->global_color; b.d_gradients = go->gradients;
  b.eik_sums = out->eik_sums;
  b.d_sdf = gi->d_sdf_samples; b.d_g = gi->d_gradients; b.d_color = gi->d_color_samples; b.d_gcolor = gi->d_global_color_samples; b.d_bg_alpha = gi->d_bg_alpha;
  b.d_bg_color = gi->d_bg_color; b.d_inv_s_partial = dinvs; b.d_rays_d = gi->d_rays_d; b.d_z = gi->d_z_vals; b.d_z_feed = gi->d_z_feed;
  be_composite_bg_bwd(b, s);
  VarianceFinish vf;
  vf.partial = dinvs; vf.R = in->n_rays; vf.variance = in->variance; vf.d_variance = gi->d_variance;
  be_variance_finish(vf, s);
  return check_backend("composite_background_backward");
}

}  // extern "C"
