// The forward pass of the render path (reference NeuS.forward, NeuS.py:294-408):
//   weight preparation -> coarse z -> [SDF value chain -> up_sample -> merge] x K -> fine set-up ->
//   SDF chain (stores pre-activations) -> analytic gradient chain (reverse sweep, replaces the reference's second
//   SDF forward + autograd.grad, fields.py:105-115) -> colour chain -> relight chain -> alpha + compositing.
// cnr_render_forward, cnr_render_forward_only (the same launches, nothing kept for a backward pass) and cnr_sample_z.  The chains on embedded
// points (prep_all, embed_points, sdf_chain, point_pipeline, color_input_view) also serve cnr_points.cpp.
#include "cnr_plan.h"

namespace cnr {

// sdf_only: the SDF layers alone (point queries: the other entries of params may be null)
void prep_all(Model& m, const float* const* params, cnr_stream s, bool sdf_only) {
  std::vector<Lin*> layers;
  for (auto& q : m.sdf) layers.push_back(&q);
  if (!sdf_only) for (auto& q : m.col) layers.push_back(&q);
  if (!sdf_only) for (auto& q : m.rel) layers.push_back(&q);
  prep_layers(layers, params, s);
  std::vector<PackJob> pj;
  for (auto& q : m.sdf) if (q.Wf) pj.push_back(PackJob{q.Wp, (long)q.wpad * q.ldw, q.wpad, q.ldw, q.Wf});
  // the hidden layers of the ReLU stacks (chain-fused forward, cnr_chain_fwd.hip); their 3-wide heads stay fp32
  if (!sdf_only) for (auto& q : m.col) if (q.Wf && q.n == 256) pj.push_back(PackJob{q.Wp, (long)q.wpad * q.ldw, q.wpad, q.ldw, q.Wf});
  if (!sdf_only) for (auto& q : m.rel) if (q.Wf && q.n == 256) pj.push_back(PackJob{q.Wp, (long)q.wpad * q.ldw, q.wpad, q.ldw, q.Wf});
  be_pack_frags_many(pj.data(), (int)pj.size(), s);         // fragment-major copies for the chain-fused kernels: one launch
}

// forward-input view of SDF layer l (value path): e, softplus(z_{l-1}) or the skip concat / sqrt(2)
View sdf_input_view(const Model& m, int l, const float* E, const float* const* Z) {
  View v;
  if (l == 0) {
    v.kind = VK_DIRECT; v.a = E; v.lda = kEmb;
  } else {
    v.kind = VK_SOFTPLUS; v.a = Z[l - 1]; v.lda = m.Hs;
    if (m.skip(l)) { v.math_split = m.sdf[l - 1].n; v.scale = kInvSqrt2; }   // tail columns of Z[l-1] hold e (tail fill)
  }
  return v;
}

// SDF value chain on n points; Z[l] receive the pre-activations of the hidden layers.  If value_only the top
// layer only evaluates row 0 (the sdf) and writes sign*sdf/scale... (sign folded by the caller through `top_scale`).
static bool sdf_value_chain_fused(const Model& m, long n, const float* E, float* sdf_out, float top_scale, cnr_stream s) {
  if (m.Hs != 256 || m.L < 1) return false;
  // what the kernel hard-codes beyond the hidden width: the top layer is not a skip layer, the last hidden layer is 256 wide and the sdf
  // row of the top layer is readable as 256 contiguous floats; anything else stays on the per-layer path
  if (m.skip(m.L) || m.sdf[m.L - 1].n != 256 || m.sdf[m.L].ldw < 256) return false;
  SdfValueChain c;
  c.E = E; c.P = n; c.nl = m.L; c.skip_mask = m.c.sdf_skip_mask; c.emb = m.emb;
  for (int l = 0; l < m.L; ++l) {
    const Lin& q = m.sdf[l];
    if (!q.Wf) return false;
    c.lay[l] = FusedLayer{q.Wf, q.Wps, q.bias, q.ldw, q.n};
  }
  const Lin& t = m.sdf[m.L];
  c.wtop = t.W + (long)m.F * t.ldw; c.btop = t.bias + m.F; c.top_scale = top_scale; c.sdf_out = sdf_out;
  return be_sdf_value_chain(c, s);
}

// the SAVING forward (pre-activations, row scales, feature rows for the backward pass) as one chain-fused launch (cnr_chain_fwd.hip)
static bool sdf_save_chain_fused(const Model& m, long n, const float* E, float* const* Z, float* sdf_out, float* feat_out, int ld_feat,
                                 float top_scale, float* const* rs, cnr_stream s) {
  if (m.Hs != 256 || m.L < 1 || m.F != 256 || m.L + 1 > kMaxLayers) return false;
  if (m.skip(m.L) || m.sdf[m.L - 1].n != 256 || m.sdf[m.L].ldw != 256 || !m.sdf[m.L].Wf) return false;
  // Where the chain pays: it loads the layer weights once per 128-point tile from L2 instead of once per launch and workgroup, and saves
  // 17 launches' fixed costs -- decisive for small batches; at large batches its stores do not overlap its MFMA phases and the per-layer
  // launches are faster (measured: DESIGN.md section 4.5).  CNR_CHAIN_SDF_MAXP moves the switch-over (points).
  const long maxp = debug_flags().chain_sdf_maxp;
  if (n > maxp) return false;
  SdfSaveChain c;
  c.v.E = E; c.v.P = n; c.v.nl = m.L; c.v.skip_mask = m.c.sdf_skip_mask; c.v.emb = m.emb;
  for (int l = 0; l < m.L; ++l) {
    const Lin& q = m.sdf[l];
    if (!q.Wf || !Z[l]) return false;
    c.v.lay[l] = FusedLayer{q.Wf, q.Wps, q.bias, q.ldw, q.n};
    c.Z[l] = Z[l];
  }
  c.ldz = m.Hs;
  for (int l = 1; l <= m.L; ++l) c.rs[l] = rs ? rs[l] : nullptr;
  const Lin& t = m.sdf[m.L];
  c.top = FusedLayer{t.Wf, t.Wps, t.bias, t.ldw, m.F};
  c.feat = feat_out; c.ld_feat = ld_feat;
  c.v.wtop = t.W + (long)m.F * t.ldw; c.v.btop = t.bias + m.F; c.v.top_scale = top_scale; c.v.sdf_out = sdf_out;
  return be_sdf_save_chain(c, s);
}

void sdf_chain(const Model& m, long n, const float* E, float* const* Z, float* sdf_out, float* feat_out, int ld_feat,
               float top_scale, cnr_stream s, float* const* rs /* [L+1] row scales of the layer inputs, see Ctx::rsY */) {
  if (!feat_out && !rs && sdf_value_chain_fused(m, n, E, sdf_out, top_scale, s)) return;   // value only: one chain-fused launch
  if (feat_out && sdf_save_chain_fused(m, n, E, Z, sdf_out, feat_out, ld_feat, top_scale, rs, s)) return;
  for (int l = 0; l <= m.L; ++l) {
    const Lin& q = m.sdf[l];
    LayerGemm g = fwd_gemm(q, n);
    g.A = sdf_input_view(m, l, E, Z);
    if (rs && (l < m.L || feat_out)) g.rs_out = rs[l];
    if (l < m.L) {
      g.E.kind = EK_STORE; g.E.n_out = q.n; g.E.bias = q.bias; g.E.o1 = Z[l]; g.E.ld1 = m.Hs;
      if (m.skip(l + 1)) { g.E.tail_src = E; g.E.ld_tail = kEmb; g.E.tail_n = m.emb; }   // next layer reads [h | e]
    } else if (feat_out) {
      // internal row order [features (F) | sdf]: the F feature columns by the layer launch, the sdf row as a row dot formed while the launch
      // stages its input rows (no second launch over the same rows)
      g.N = m.F;
      g.E.kind = EK_SDF_TOP; g.E.n_out = m.F; g.E.bias = q.bias; g.E.scale = top_scale; g.E.split = m.F;
      g.E.o1 = feat_out; g.E.ld1 = ld_feat; g.E.o2 = sdf_out;
      g.dot_w = q.W + (long)m.F * q.ldw; g.dot_bias = q.bias + m.F; g.dot_scale = top_scale; g.dot_out = sdf_out;
    } else {   // value only: just the sdf row (last internal row)
      g.W = q.W + (long)m.F * q.ldw; g.N = 1; g.Wp = nullptr;
      g.E.kind = EK_STORE; g.E.n_out = 1; g.E.bias = q.bias + m.F; g.E.scale = top_scale; g.E.o1 = sdf_out; g.E.ld1 = 1;
    }
    be_layer_gemm(g, s);
  }
}

static void run_sampler(const Model& m, const cnr_render_inputs* in, float* z, Ctx& x, cnr_stream s) {
  const long R = in->n_rays;
  const float scale = m.c.sdf_scale;
  EmbedZ e;
  e.o = in->rays_o; e.d = in->rays_d; e.R = R; e.m = m.S; e.z = z; e.ldz = m.M; e.make_z = 1;
  e.near_ = in->near_; e.far_ = in->far_; e.t_rand = in->t_rand; e.scale = scale; e.multires = m.c.sdf_multires; e.E = x.sE;
  be_embed_z(e, s);
  if (m.I <= 0) return;
  float* Zp[kMaxLayers];
  for (int l = 0; l < m.L; ++l) Zp[l] = (l & 1) ? x.sZb : x.sZa;
  sdf_chain(m, R * m.S, x.sE, Zp, x.s_sdf0, nullptr, 0, 1.0f / scale, s);
  const int mnew = m.I / m.K;
  int n = m.S;
  const bool unfused = debug_flags().no_sampler_fuse;   // debugging aid: merge / up_sample / embedding as launches of their own
  MergeZ prev;   // the merge of iteration i - 1 rides on the launch of iteration i
  for (int i = 0; i < m.K; ++i) {
    const bool last = i + 1 == m.K;
    UpSample u;
    u.o = in->rays_o; u.d = in->rays_d; u.R = R; u.z = z; u.ldz = m.M;
    u.sdf = i == 0 ? x.s_sdf0 : x.s_sdf; u.lds = i == 0 ? m.S : m.M; u.n = n; u.m = mnew;
    u.inv_s = 64.0f * (float)(1 << i); u.new_z = x.s_newz;
    EmbedZ e2 = e;
    e2.m = mnew; e2.z = x.s_newz; e2.ldz = mnew; e2.make_z = 0;
    if (!unfused && mnew <= 64) {
      SamplerStep st;
      st.do_merge = i > 0; st.g = prev; st.u = u; st.do_embed = !last; st.E = x.sE; st.scale = scale; st.multires = m.c.sdf_multires;
      be_sampler_step(st, s);
    } else {
      if (i > 0) be_merge(prev, s);
      be_upsample(u, s);
      if (!last) be_embed_z(e2, s);
    }
    if (!last) sdf_chain(m, R * mnew, x.sE, Zp, x.s_newsdf, nullptr, 0, 1.0f / scale, s);
    MergeZ g;
    g.R = R; g.z = z; g.ldz = m.M; g.sdf_in = i == 0 ? x.s_sdf0 : x.s_sdf; g.lds_in = i == 0 ? m.S : m.M;
    g.sdf_out = x.s_sdf; g.lds_out = m.M; g.n = n; g.new_z = x.s_newz; g.new_sdf = last ? nullptr : x.s_newsdf; g.m = mnew;
    if (last) be_merge(g, s);
    prev = g;
    n += mnew;
  }
}

// analytic gradient chain: cotangent of `sdf` pushed down through the layers
static void sdf_grad_chain(const Model& m, long P, const float* E, const float* const* Z, float* const* V, float* CE0, float* CES,
                           cnr_stream s, float* const* rs = nullptr /* [L] row scales of sigma'(z_l) v_l, see Ctx::rsX1 */) {
  const float inv_scale = 1.0f / m.c.sdf_scale;
  // V[l-1] of a skip layer is written over n < round_up(n,16) columns only (EK_SPLIT) but read back over the padded width by the
  // next GEMM of this chain: its pad columns must hold finite values whatever the caller's scratch contained (every user of the
  // chain -- render, vertex colour -- gets this here rather than at the call site)
  // (zeroed right in front of the launch that leaves them unwritten: the forward-only layout reuses two V buffers for all layers)
  bool ces_written = false;
  for (int l = m.L - 1; l >= 0; --l) {
    const Lin& q = m.sdf[l];
    if (l >= 1 && m.skip(l) && V[l - 1] && round_up(m.sdf[l - 1].n, 16) > m.sdf[l - 1].n)
      be_zero_cols(V[l - 1], m.Hs, m.sdf[l - 1].n, round_up(m.sdf[l - 1].n, 16), P, s);
    LayerGemm g = bwd_gemm(q, P);
    g.A.a = Z[l]; g.A.lda = m.Hs;
    if (l == m.L - 1) { g.A.kind = VK_SIGMUL_ROW; g.A.b = m.sdf[m.L].W + (long)m.F * m.sdf[m.L].ldw; g.A.scale = inv_scale; }   // v_{L-1} = W_top[0,:]/scale
    else { g.A.kind = VK_SIGMUL; g.A.b = V[l]; g.A.ldb = m.Hs; }
    if (rs) g.rs_out = rs[l];
    if (l == 0) {
      g.E.kind = EK_STORE; g.E.n_out = m.emb; g.E.o1 = CE0; g.E.ld1 = kEmb;
      // the 39-column end of the chain as one streaming pass over z_0 / v_0 with the W^T planes in LDS (cnr_narrow_bwd.hip, its product-only form)
      NarrowBwd nb;
      nb.X = Z[0]; nb.ldx = m.Hs; nb.Xb = g.A.b; nb.ldxb = g.A.ldb; nb.P = P;
      narrow_bwd_weights(nb, q);
      nb.dx = CE0; nb.lddx = kEmb; nb.ndx = m.emb;
      if (g.A.kind == VK_SIGMUL && g.A.scale == 1.0f && g.rs_out == nullptr && q.n == 256 && m.Hs == 256 && be_narrow_bwd_ok(nb)) { be_narrow_bwd(nb, s); continue; }
    } else if (m.skip(l)) {
      g.E.kind = EK_SPLIT; g.E.n_out = q.k_int; g.E.scale = kInvSqrt2; g.E.split = m.sdf[l - 1].n;
      g.E.o1 = V[l - 1]; g.E.ld1 = m.Hs; g.E.o2 = CES; g.E.ld2 = kEmb; g.E.o2_off = skip_off(m);
      g.E.o2_acc = ces_written; ces_written = true;   // (the sweep runs from the top layer down: the first skip layer it meets stores, the others add)
    } else {
      g.E.kind = EK_STORE; g.E.n_out = q.k_int; g.E.o1 = V[l - 1]; g.E.ld1 = m.Hs;
    }
    be_layer_gemm(g, s);
  }
}

// E (and AUX[., 0:3] where the context has aux rows) of n explicit points, or of n lattice points from index `start` on when pts is null
void embed_points(const Model& m, const float* pts, long n, float* E, float* AUX, cnr_stream s, const float* bmin, const float* bmax,
                  int res, long start) {
  EmbedPts ep;
  ep.pts = pts; ep.n = n; ep.res = res; ep.start = start;
  for (int c = 0; c < 3; ++c) { ep.bmin[c] = bmin ? bmin[c] : 0.f; ep.bmax[c] = bmax ? bmax[c] : 0.f; }
  ep.scale = m.c.sdf_scale; ep.multires = m.c.sdf_multires; ep.E = E; ep.AUX = AUX;
  be_embed_pts(ep, s);
}

// The point pipeline on the P embedded points of a filled context: SDF value chain (sdf, feature rows into featx, Z[l]) -> analytic gradient
// chain -> be_grad_finish (the gradient rows; g and, where asked, PE(view) into the aux rows).  Row scales are stored where the context
// holds them (rsY / rsX1 entries that are not null), AUX is written where the context has it.
void point_pipeline(const Model& m, long P, const Ctx& x, const PointOpts& o, cnr_stream s) {
  const float scale = m.c.sdf_scale;
  { RangeScope r_("sdf value chain"); sdf_chain(m, P, x.E, x.Z.data(), x.sdf, x.featx, x.ldfx, 1.0f / scale, s, x.rsY.data()); }
  if (!o.grad) return;
  { RangeScope r_("sdf gradient chain"); sdf_grad_chain(m, P, x.E, x.Z.data(), x.V.data(), x.CE0, x.CES, s, x.rsX1.data()); }
  GradFinish gf;
  gf.featx = o.aux_to_featx ? x.featx : nullptr; gf.ldfx = o.aux_to_featx ? x.ldfx : 0; gf.F = m.F;
  gf.P = P; gf.E = x.E; gf.ce0 = x.CE0; gf.ces = has_skip(m) ? x.CES + skip_off(m) : nullptr; gf.scale = scale; gf.multires = m.c.sdf_multires;
  gf.grad_out = o.grad_out; gf.AUX = x.AUX; gf.neg_g_as_view = o.neg_g_as_view; gf.multires_view = o.multires_view;
  be_grad_finish(gf, s);
}

View color_input_view(const Model& m, int l, const Ctx& x) {
  View v;
  v.kind = VK_DIRECT;
  if (l == 0) { v.a = x.featx; v.lda = x.ldfx; }     // [feat | p g PE(view) | 0]
  else { v.a = x.HC[l - 1]; v.lda = m.Hc; }
  return v;
}

// a narrow head (rgb, relight delta) on a 256-wide hidden layer: one streaming pass instead of a 32-column tile of the FP32-MFMA layer kernel
static bool head_fwd(const Lin& q, const LayerGemm& g, cnr_stream s) {
  const bool off = debug_flags().no_head_fwd;   // debugging aid: the layer kernel for the heads
  if (off || q.n > 4 || q.k_int != 256 || g.A.kind != VK_DIRECT || g.A.scale != 1.0f || (g.A.lda & 3) != 0 || (q.ldw & 3) != 0 || g.E.tail_src != nullptr) return false;
  HeadFwd h;
  h.h = g.A.a; h.ldh = g.A.lda; h.P = g.P; h.P_dev = g.P_dev; h.W = q.W; h.ldw = q.ldw; h.n = q.n; h.E = g.E;
  be_head_fwd(h, s);
  return true;
}

static void color_chain(const Model& m, long P, const Ctx& x, cnr_stream s, const int* P_dev = nullptr) {
  for (int l = 0; l < m.NC; ++l) {
    const Lin& q = m.col[l];
    LayerGemm g = fwd_gemm(q, P);
    g.A = color_input_view(m, l, x); g.P_dev = P_dev;
    g.E.bias = q.bias; g.E.n_out = q.n;
    if (!P_dev && (size_t)l < x.rsC.size()) g.rs_out = x.rsC[l];
    if (l + 1 < m.NC) { g.E.kind = EK_RELU; g.E.o1 = x.HC[l]; g.E.ld1 = m.Hc; }
    else {
      g.E.kind = m.c.col_squeeze_out ? EK_SIGMOID : EK_LINEAR_SIG; g.E.o1 = x.gcol; g.E.ld1 = 4;
      if (m.has_relight) { g.E.o2 = x.hry; g.E.ld2 = x.ldy; g.E.o2_off = m.Hr; }   // relight y-layer input tail [.. | rgb | 0]
    }
    if (l + 1 == m.NC && head_fwd(q, g, s)) continue;
    be_layer_gemm(g, s);
  }
}

View relight_input_view(const Model& m, int i /* rl_mlp index, -1 = in_layer */, const Ctx& x) {
  View v;
  v.kind = VK_DIRECT;
  if (i < 0) { v.a = x.AUX; v.lda = kAux; }
  else { v.a = x.HR[i]; v.lda = hr_ld(m, x, i); }    // i == y: hry = [h | rgb | 0]
  return v;
}

static void relight_chain(const Model& m, long P, const Ctx& x, float* delta_out, cnr_stream s, const int* P_dev = nullptr) {
  {
    const Lin& q = m.rel[0];
    LayerGemm g = fwd_gemm(q, P);
    g.A = relight_input_view(m, -1, x); g.P_dev = P_dev;
    g.E.kind = EK_RELU; g.E.bias = q.bias; g.E.n_out = q.n; g.E.o1 = x.HR[0]; g.E.ld1 = hr_ld(m, x, 0);
    be_layer_gemm(g, s);
  }
  for (int i = 0; i < m.NR; ++i) {
    const Lin& q = m.rel[1 + i];
    LayerGemm g = fwd_gemm(q, P);
    g.A = relight_input_view(m, i, x); g.P_dev = P_dev;
    g.E.bias = q.bias; g.E.n_out = q.n;
    if (!P_dev && (size_t)i < x.rsR.size()) g.rs_out = x.rsR[i];
    if (i + 1 < m.NR) { g.E.kind = EK_RELU; g.E.o1 = x.HR[i + 1]; g.E.ld1 = hr_ld(m, x, i + 1); }
    else {
      g.E.kind = EK_RELIGHT_TOP; g.E.o1 = delta_out; g.E.ld1 = 3; g.E.o2 = x.relit; g.E.ld2 = 4;
      g.E.aux = x.gcol; g.E.ldaux = 4; g.E.inv_sigmoid = m.c.rel_inv_sigmoid;
    }
    if (i + 1 == m.NR && head_fwd(q, g, s)) continue;
    be_layer_gemm(g, s);
  }
}

// Colour chain + relight chain as ONE chain-fused launch (cnr_chain_fwd.hip) where the shapes allow: 256-wide hidden layers, a 256-wide
// feature vector, heads of <= 3 outputs.  Returns false (nothing launched) otherwise: the per-layer chains above then run.
static bool relu_chains_fused(const Model& m, long P, const Ctx& x, float* delta_out, cnr_stream s, const int* P_dev = nullptr, const int* row_idx = nullptr) {
  if (!relu_fused_shapes(m)) return false;   // (one definition of the shapes: the forward-only layout relies on the same answer)
  ReluChainFwd c;
  c.P = P; c.P_dev = P_dev; c.row_idx = row_idx;
  auto hidden_ok = [](const Lin& q, int k_lo, int k_hi) { return q.n == 256 && q.Wf && q.wpad >= 256 && q.k_int >= k_lo && q.k_int <= k_hi; };
  auto head_ok = [](const Lin& q) { return q.n >= 1 && q.n <= 3 && q.k_int == 256 && (q.ldw & 3) == 0; };
  auto fill = [](ChainFwdStep& st, const Lin& q) { st.Wf = q.Wf; st.wsc = q.Wps; st.bias = q.bias; st.nkb_w = q.ldw / 16; };
  int n = 0;
  // ---- colour: lin0 takes [feat (256) | p g PE(view) (ldw - 256 columns of the aux part)], lin1.. the hidden vector
  for (int l = 0; l + 1 < m.NC; ++l) {
    const Lin& q = m.col[l];
    ChainFwdStep& st = c.st[n++];
    fill(st, q);
    if (l == 0) {
      if (!hidden_ok(q, 257, 304) || q.ldw > x.ldfx) return false;
      st.in = x.featx; st.ld_in = x.ldfx; st.nkb_main = 16; st.nkb_x = q.ldw / 16 - 16; st.x_src = 1;
    } else {
      if (!hidden_ok(q, 256, 256) || q.ldw != 256) return false;
      st.nkb_main = 16;
    }
    st.save = x.HC[l]; st.ld_save = m.Hc;
    st.rs_in = (size_t)l < x.rsC.size() ? x.rsC[l] : nullptr;
  }
  c.st[n - 1].head = 1;
  {
    const Lin& q = m.col[m.NC - 1];
    if (!head_ok(q)) return false;
    c.col_head = ChainFwdHead{q.W, q.ldw, q.bias, q.n};
    c.col_squeeze = m.c.col_squeeze_out ? 1 : 0;
    c.gcol = x.gcol;
    if (m.has_relight && x.hry) { c.rgb_tail = x.hry + m.Hr; c.ld_tail = x.ldy; }   // (forward-only: the y-layer takes rgb from the chip, no tail is kept)
  }
  if (m.has_relight) {
    if (m.Hr != 256 || m.NR < 2) return false;
    const int y = m.c.rel_y_in_layer - 1;                    // rl_mlp[y] takes [h | rgb]
    if (y < 1 || y > m.NR - 2) return false;                 // (y == 0 would put the tail on the in_layer's output; the head takes no tail)
    {
      const Lin& q = m.rel[0];
      if (q.n != 256 || !q.Wf || q.ldw > kAux || q.ldw < 16) return false;
      ChainFwdStep& st = c.st[n++];
      fill(st, q);
      st.in = x.AUX; st.ld_in = kAux; st.nkb_main = q.ldw / 16;
      st.save = x.HR[0]; st.ld_save = hr_ld(m, x, 0);
    }
    for (int i = 0; i + 1 < m.NR; ++i) {
      const Lin& q = m.rel[1 + i];
      ChainFwdStep& st = c.st[n++];
      fill(st, q);
      st.nkb_main = 16;
      if (i == y) {
        if (!hidden_ok(q, 257, 259) || q.ldw != 272) return false;
        st.nkb_x = 1; st.x_src = 2;
      } else if (!hidden_ok(q, 256, 256) || q.ldw != 256) return false;
      st.save = x.HR[i + 1]; st.ld_save = hr_ld(m, x, i + 1);
      st.rs_in = (size_t)i < x.rsR.size() ? x.rsR[i] : nullptr;
    }
    c.st[n - 1].head = 2;
    const Lin& q = m.rel[m.NR];
    if (!head_ok(q) || q.n != m.col[m.NC - 1].n) return false;
    c.rel_head = ChainFwdHead{q.W, q.ldw, q.bias, q.n};
    c.inv_sigmoid = m.c.rel_inv_sigmoid;
    c.delta = delta_out; c.relit = x.relit;
  }
  c.nsteps = n;
  return be_relu_chain_fwd(c, s);
}

// Early termination, first half: the weights (they need only sdf and its gradient; the colour buffers hold nothing yet), per-ray counts of the
// samples with weight >= eps, their offsets, and the gather pass -- pg arrives with what the caller's form of it takes (compact copies, or
// outputs to zero for the dropped samples) and gets the index list here
static void prune_select(const CompositeFwd& cf, float eps, const Ctx& x, PruneGather pg, cnr_stream s) {
  CompositeFwd cw = cf;
  cw.color = nullptr; cw.gcolor = nullptr; cw.delta = nullptr; cw.delta_ray_sum = nullptr;
  be_composite_fwd(cw, s);
  PruneCount pc; pc.weights = cf.weights; pc.R = cf.R; pc.M = cf.M; pc.eps = eps; pc.counts = x.p_counts;
  be_prune_count(pc, s);
  PruneScan ps; ps.counts = x.p_counts; ps.R = cf.R; ps.offsets = x.p_offsets;
  be_prune_scan(ps, s);
  pg.weights = cf.weights; pg.R = cf.R; pg.M = cf.M; pg.eps = eps; pg.offsets = x.p_offsets; pg.idx = x.p_idx;
  pg.featx = x.featx; pg.ldfx = x.ldfx; pg.aux = x.AUX;
  be_prune_gather(pg, s);
}

// infer: the forward-only form (cnr_render_forward_only): same launches for everything that produces a value -- outputs are bit-identical --
// but nothing is written for a backward pass (no row scales, no hidden activations of the ReLU stacks, no V_l beyond the one in flight)
static int render_forward(const cnr_config* cfg, const float* const* params, const cnr_render_inputs* in,
                          const cnr_render_outputs* out, void* ctx, size_t ctx_bytes, cnr_stream s, bool infer = false) {
  Model m;
  if (build_model(cfg, m)) return -1;
  if (!params || !in || !out || !ctx) return fail("null argument");
  const long R = in->n_rays;
  if (R <= 0) return fail("n_rays must be positive");
  Ctx x;
  auto layout = [&](Arena& a) { if (infer) layout_ctx_infer(m, R, a, x); else layout_ctx(m, R, a, x); };
  if (layout_checked(infer ? "scratch buffer" : "context buffer", ctx, ctx_bytes, layout)) return -1;
  if (!out->z_vals || !out->weights || !out->color_fine || !out->cdf_fine || !out->inside_sphere ||
      !out->weight_sum || !out->weight_max || !out->depth || !out->s_val || !out->gradient_error)
    return fail("missing output buffer");
  if (m.has_relight && !out->global_color) return fail("Color_NeuS needs a global_color buffer");
  if (m.has_relight && !out->delta_relight && !out->delta_relight_ray_sum) return fail("Color_NeuS needs delta_relight or delta_relight_ray_sum");
  if (in->prune_eps > 0.0f && m.has_relight && !out->delta_relight && !x.infer_fused) return fail("prune_eps > 0 needs the delta_relight buffer");
  if (in->prune_eps > 0.0f && out->delta_relight_ray_sum) return fail("prune_eps > 0 (inference) does not go with the loss-only training outputs");
  float* const g_out = out->gradients ? out->gradients : x.gbuf;                       // "loss only" callers leave both to the context buffer
  float* const delta_out = m.has_relight ? (out->delta_relight ? out->delta_relight : x.delta_s) : nullptr;
  const long P = R * m.M;
  const float scale = m.c.sdf_scale;

  RangeScope range_fwd("cnr_render_forward");
  { RangeScope r_("weights"); prep_all(m, params, s); }
  if (in->z_vals_override) {
    if (in->z_vals_override != out->z_vals) return fail("z_vals_override must alias outputs.z_vals (copy it there first)");
  } else {
    RangeScope r_("sampler");
    run_sampler(m, in, out->z_vals, x, s);
  }
  FineSetup fs;
  fs.o = in->rays_o; fs.d = in->rays_d; fs.z = out->z_vals; fs.R = R; fs.M = m.M; fs.sample_dist = 2.0f / (float)m.S;
  fs.scale = scale; fs.multires = m.c.sdf_multires; fs.multires_view = m.mv; fs.E = x.E; fs.AUX = x.AUX;
  be_fine_setup(fs, s);
  PointOpts po;
  po.grad_out = g_out; po.multires_view = m.mv;
  point_pipeline(m, P, x, po, s);
  CompositeFwd cf;
  cf.o = in->rays_o; cf.d = in->rays_d; cf.z = out->z_vals; cf.R = R; cf.M = m.M; cf.sample_dist = 2.0f / (float)m.S;
  cf.sdf = x.sdf; cf.g = g_out;
  cf.color = m.has_relight ? x.relit : x.gcol; cf.ldcolor = 4;
  cf.gcolor = m.has_relight ? x.gcol : nullptr; cf.ldg = 4;
  cf.variance = params[m.p_variance]; cf.cos_anneal = in->cos_anneal_ratio; cf.background_rgb = in->background_rgb;
  cf.color_fine = out->color_fine; cf.s_val = out->s_val; cf.cdf_fine = out->cdf_fine; cf.weight_sum = out->weight_sum;
  cf.weight_max = out->weight_max; cf.weights = out->weights; cf.inside_sphere = out->inside_sphere; cf.depth = out->depth;
  cf.global_color = m.has_relight ? out->global_color : nullptr; cf.eik_partial = x.eik_partial;
  cf.sdf_s = out->sdf_samples; cf.color_s = out->color_samples; cf.gcolor_s = m.has_relight ? out->global_color_samples : nullptr;
  if (m.has_relight && out->delta_relight_ray_sum) { cf.delta = delta_out; cf.delta_ray_sum = out->delta_relight_ray_sum; }

  if (in->prune_eps > 0.0f && x.infer_fused) {
    // early termination on the forward-only path: a ballot / popcount pass per ray builds the list of samples with weight >= eps (and zeroes
    // the colour outputs of the others), and the chain-fused colour + relight launch reads its rows through that list and writes the kept
    // samples' outputs in place -- no compact copies, no scatter
    PruneGather pg;
    pg.featx_c = nullptr; pg.aux_c = nullptr;
    pg.zero_gcol = x.gcol; pg.zero_relit = m.has_relight ? x.relit : nullptr; pg.zero_delta = delta_out;
    prune_select(cf, in->prune_eps, x, pg, s);
    if (!relu_chains_fused(m, P, x, delta_out, s, x.p_offsets + R, x.p_idx)) return fail("render_forward_only: the chain-fused colour / relight launch refused its shapes");
  } else if (in->prune_eps > 0.0f) {
    // inference-only early termination: the colour / relight networks on the compacted list of samples with weight >= eps, scattered
    // back into zero-filled per-sample buffers
    be_memset_zero(x.gcol, (size_t)P * 4 * sizeof(float), s);
    be_memset_zero(x.relit, (size_t)P * 4 * sizeof(float), s);
    if (m.has_relight) be_memset_zero(out->delta_relight, (size_t)P * 3 * sizeof(float), s);
    PruneGather pg;
    pg.featx_c = x.featx_c; pg.aux_c = x.aux_c;
    prune_select(cf, in->prune_eps, x, pg, s);
    Ctx xc = x;   // the chains run on the compact buffers; only the device knows how many rows they hold
    xc.featx = x.featx_c; xc.AUX = x.aux_c; xc.gcol = x.gcol_c; xc.relit = x.relit_c;
    const int* kept = x.p_offsets + R;
    color_chain(m, P, xc, s, kept);
    if (m.has_relight) relight_chain(m, P, xc, x.delta_c, s, kept);
    PruneScatter sc; sc.P = P; sc.count = kept; sc.idx = x.p_idx; sc.gcol_c = x.gcol_c; sc.relit_c = m.has_relight ? x.relit_c : nullptr;
    sc.delta_c = m.has_relight ? x.delta_c : nullptr; sc.gcol = x.gcol; sc.relit = m.has_relight ? x.relit : nullptr;
    sc.delta = m.has_relight ? out->delta_relight : nullptr;
    be_prune_scatter(sc, s);
  } else {
    RangeScope r_("colour + relight chains");
    if (!relu_chains_fused(m, P, x, delta_out, s)) {
      // (the forward-only layout holds no hidden-layer buffers when it counted on the chain-fused launch: never fall through to the per-layer chains then)
      if (x.infer_fused) return fail("render_forward_only: the chain-fused colour / relight launch refused its shapes");
      color_chain(m, P, x, s);
      if (m.has_relight) relight_chain(m, P, x, delta_out, s);
    }
  }
  RangeScope r_comp("compositor");
  be_composite_fwd(cf, s);
  ReduceEik re;
  re.partial = x.eik_partial; re.R = R; re.sums = x.eik_sums; re.sums_out = out->eik_sums; re.gradient_error = out->gradient_error;
  be_reduce_eik(re, s);
  return check_backend(infer ? "render_forward_only" : "render_forward");
}

}  // namespace cnr

using namespace cnr;

extern "C" {

int cnr_render_forward_only(const cnr_config* cfg, const float* const* params, const cnr_render_inputs* in, const cnr_render_outputs* out,
                            void* scratch, size_t scratch_bytes, void* stream) {
  return render_forward(cfg, params, in, out, scratch, scratch_bytes, (cnr_stream)stream, true);
}

int cnr_render_forward(const cnr_config* cfg, const float* const* params, const cnr_render_inputs* in,
                       const cnr_render_outputs* out, void* ctx, size_t ctx_bytes, void* stream) {
  return render_forward(cfg, params, in, out, ctx, ctx_bytes, (cnr_stream)stream);
}

int cnr_sample_z(const cnr_config* cfg, const float* const* params, const cnr_render_inputs* in, float* z_vals, void* ctx, size_t ctx_bytes,
                 void* stream) {
  Model m;
  if (build_model(cfg, m)) return -1;
  if (!params || !in || !z_vals || !ctx) return fail("null argument");
  if (in->n_rays <= 0) return fail("n_rays must be positive");
  Ctx x;
  if (layout_checked("context buffer", ctx, ctx_bytes, [&](Arena& a) { layout_ctx(m, in->n_rays, a, x); })) return -1;
  prep_all(m, params, (cnr_stream)stream);
  run_sampler(m, in, z_vals, x, (cnr_stream)stream);
  return check_backend("sample_z");
}

}  // extern "C"
