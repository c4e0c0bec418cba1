// The render model (build_model: the configuration's checks, the layers, the parameter list) and every layout of the render path: weights,
// forward context (training and forward-only), backward scratch with the slot policies of its weight-gradient pool; the parameter and
// *_bytes queries of the ABI, which run the same layout functions as the entry points they size.
#include "cnr_plan.h"

namespace cnr {

int build_model(const cnr_config* cfg, Model& m) {
  if (!cfg) return fail("null config");
  m.c = *cfg;
  const cnr_config& c = m.c;
  m.S = c.n_samples; m.I = c.n_importance; m.M = m.S + m.I; m.K = c.up_sample_steps;
  if (m.S < 2 || m.M > kMaxRaySamples) return fail("n_samples + n_importance must be in [2, %d]", kMaxRaySamples);
  if (m.I > 0 && (m.K < 1 || m.I % m.K != 0 || m.I / m.K > 64)) return fail("n_importance must be a multiple of up_sample_steps (<= 64 new samples per step)");
  if (c.sdf_multires < 1 || c.sdf_multires > 6) return fail("sdf multires must be in [1,6]");
  m.emb = 3 + 6 * c.sdf_multires;
  m.Hs = c.sdf_d_hidden; m.L = c.sdf_n_layers; m.F = c.sdf_d_out - 1;
  if (m.Hs < 48 || m.Hs > 256 || m.Hs % 16) return fail("sdf d_hidden must be a multiple of 16 in [48,256]");
  if (m.L < 1 || m.L > kMaxLayers) return fail("sdf n_layers out of range");
  if (m.F < 1 || m.F > 256 || m.F != c.col_d_feature) return fail("sdf d_out - 1 must equal colour d_feature (<= 256)");
  if (c.sdf_skip_mask & 1) return fail("skip connection at layer 0 is not supported");
  if ((c.sdf_skip_mask >> m.L) & 1) return fail("skip connection at the top layer is not supported");
  // Several skip connections (fields.py:45-48 allows any SKIP_IN; every shipped YAML has [4]): the embedding cotangents of the gradient chain and of
  // the backward pass have one buffer each (Ctx::CES, ebars); the launch of the FIRST skip layer a sweep meets stores into it, the later ones add
  // (Epi::o2_acc).  Round 6: a [2, 4] fixture captured from the reference showed that such a network used to be accepted and rendered wrong normals.
  m.has_relight = c.type == 1;
  m.Hc = c.col_d_hidden; m.NC = c.col_n_layers + 1;
  if (m.Hc < 16 || m.Hc > 256 || m.Hc % 16 || c.col_n_layers < 1 || c.col_n_layers >= kMaxLayers) return fail("colour d_hidden must be a multiple of 16 in [16,256]");
  const bool col_view = c.col_mode != 1;
  if (col_view && c.col_multires_view > 4) return fail("colour multires_view must be <= 4");
  int mv_c = col_view ? c.col_multires_view : -1, mv_r = m.has_relight ? c.rel_multires_view : -1;
  if (mv_c >= 0 && mv_r >= 0 && mv_c != mv_r) return fail("colour and relight multires_view must match when both use view directions");
  m.mv = mv_c >= 0 ? mv_c : (mv_r >= 0 ? mv_r : 0);
  if (m.mv > 4) return fail("multires_view must be <= 4");
  m.nv = (mv_c >= 0 || mv_r >= 0) ? (m.mv > 0 ? 3 + 6 * m.mv : 3) : 0;
  m.naux = 6 + m.nv;
  if (m.naux > kAux) return fail("aux input too wide");

  // ---- SDF layers (fields.py:31-75)
  m.sdf.resize(m.L + 1);
  int prev = m.emb;
  for (int l = 0; l <= m.L; ++l) {
    Lin& q = m.sdf[l];
    q.k_ref = (l == 0) ? m.emb : m.Hs;
    int out = (l == m.L) ? c.sdf_d_out : m.Hs;
    if (l < m.L && m.skip(l + 1)) out = m.Hs - m.emb;
    q.n = out;
    if (l > 0 && !m.skip(l) && prev != q.k_ref) return fail("inconsistent SDF dims");
    if (l > 0 && m.skip(l) && prev + m.emb != q.k_ref) return fail("inconsistent SDF skip dims");
    identity_seg(q);
    if (l == m.L) q.row_rot = 1;   // internal rows [features (F) | sdf]: the 256 feature columns stay 16-byte aligned
    q.finish_dims();
    // the layer below a skip connection: its launches also write the embedding into the columns behind its own (tail fill); zero weight rows
    // under those columns let every 32-column block of the launch run the same code (the stream form of the layer kernel)
    if (l < m.L && m.skip(l + 1) && round_up(q.n + m.emb, 32) <= 256) q.wpad = round_up(q.n + m.emb, 32);
    add_linear_params(m.params, q, "sdf_network.lin" + std::to_string(l), c.sdf_weight_norm != 0);
    prev = out;
  }
  m.p_variance = (int)m.params.size();
  m.params.push_back({"deviation_network.variance", 1, 1});
  // ---- colour layers (fields.py:138-153); layer 0 input is permuted to [feat | p g PE(view)]
  m.col.resize(m.NC);
  for (int l = 0; l < m.NC; ++l) {
    Lin& q = m.col[l];
    q.n = (l == m.NC - 1) ? 3 : m.Hc;
    if (l == 0) {
      const int F = m.F, nvc = col_view ? m.nv : 0;
      if (c.col_mode == 1) {         // [p, g, feat]
        q.k_ref = 6 + F; q.k_int = F + 6; q.nseg = 3;
        q.seg[0] = {0, 6, F}; q.seg[1] = {F, 0, 3}; q.seg[2] = {F + 3, 3, 3};
      } else if (c.col_mode == 0) {  // [p, PE(v), g, feat]
        q.k_ref = 6 + nvc + F; q.k_int = F + 6 + nvc; q.nseg = 4;
        q.seg[0] = {0, 6 + nvc, F}; q.seg[1] = {F, 0, 3}; q.seg[2] = {F + 3, 3 + nvc, 3}; q.seg[3] = {F + 6, 3, nvc};
      } else {                       // [p, PE(v), feat]
        q.k_ref = 3 + nvc + F; q.k_int = F + 6 + nvc; q.nseg = 3;
        q.seg[0] = {0, 3 + nvc, F}; q.seg[1] = {F, 0, 3}; q.seg[2] = {F + 6, 3, nvc};
      }
    } else {
      q.k_ref = m.Hc;
      identity_seg(q);
    }
    q.finish_dims();
    add_linear_params(m.params, q, "color_network.lin" + std::to_string(l), c.col_weight_norm != 0);
  }
  // ---- relight layers (fields.py:305-325)
  if (m.has_relight) {
    m.Hr = c.rel_d_hidden; m.NR = c.rel_n_layers;
    if (m.Hr < 16 || m.Hr > 256 || m.Hr % 16 || m.NR < 1 || m.NR >= kMaxLayers) return fail("relight d_hidden must be a multiple of 16 in [16,256]");
    if (c.rel_y_in_layer < 1 || c.rel_y_in_layer > m.NR) return fail("relight y_in_layer out of range");
    m.rel.resize(m.NR + 1);
    {
      Lin& q = m.rel[0];
      q.n = m.Hr;
      const int ig = c.rel_include_grad ? 3 : 0;
      q.k_ref = 3 + m.nv + ig; q.k_int = 6 + m.nv; q.nseg = 0;
      q.seg[q.nseg++] = {0, 0, 3};
      if (ig) q.seg[q.nseg++] = {3, 3 + m.nv, 3};
      q.seg[q.nseg++] = {6, 3, m.nv};
      q.finish_dims();
      add_weight_bias(m.params, q, "relight_network.in_layer");
    }
    for (int i = 0; i < m.NR; ++i) {
      Lin& q = m.rel[1 + i];
      const bool y = i == c.rel_y_in_layer - 1;
      q.n = (i == m.NR - 1) ? 3 : m.Hr;
      if (y) {
        q.k_ref = 3 + m.Hr; q.k_int = m.Hr + 3; q.nseg = 2;
        q.seg[0] = {0, 3, m.Hr}; q.seg[1] = {m.Hr, 0, 3};
      } else {
        q.k_ref = m.Hr; identity_seg(q);
      }
      q.finish_dims();
      add_weight_bias(m.params, q, "relight_network.rl_mlp." + std::to_string(i));
    }
  } else {
    m.Hr = 0; m.NR = 0;
  }
  return 0;
}

// The cotangents of the skip-connection embedding leave the split epilogues through o2 at column offset split % 4, which makes
// their 16-byte stores aligned; every reader of those buffers (CES, ebars) adds the same offset.
int skip_off(const Model& m) {
  for (int l = 1; l < m.L; ++l) if (m.skip(l)) return m.sdf[l - 1].n & 3;
  return 0;
}

int top_skip(const Model& m) {   // the highest layer fed by a skip connection (-1: none)
  for (int l = m.L - 1; l >= 1; --l) if (m.skip(l)) return l;
  return -1;
}
bool has_skip(const Model& m) {
  for (int l = 1; l < m.L; ++l) if (m.skip(l)) return true;
  return false;
}

int hr_ld(const Model& m, const Ctx& x, int i) { return i == m.c.rel_y_in_layer - 1 ? x.ldy : m.Hr; }

void layout_weights(Model& m, Arena& a) {
  for (auto& q : m.sdf) place_lin(q, a);
  for (auto& q : m.col) place_lin(q, a);
  for (auto& q : m.rel) place_lin(q, a);
}

// shapes the chain-fused forward of the ReLU stacks takes (cnr_chain_fwd.hip).  THE definition: relu_chains_fused below starts with this test (what it
// checks after that are buffer pointers), and layout_ctx_infer decides by it that the forward-only layout needs no hidden-layer buffers.
bool relu_fused_shapes(const Model& m) {
  if (m.Hc != 256 || m.F != 256 || m.NC < 2 || m.NC - 1 + (m.has_relight ? m.NR : 0) > kChainSteps) return false;
  const int ldfx = round_up(m.F + kAux, 16);
  for (int l = 0; l + 1 < m.NC; ++l) {
    const Lin& q = m.col[l];
    if (q.n != 256 || q.wpad < 256 || q.ldw > 304) return false;
    if (l == 0 ? (q.k_int < 257 || q.k_int > 304 || q.ldw > ldfx) : (q.k_int != 256 || q.ldw != 256)) return false;
  }
  { const Lin& q = m.col[m.NC - 1]; if (q.n < 1 || q.n > 3 || q.k_int != 256 || (q.ldw & 3)) return false; }
  if (m.has_relight) {
    if (m.Hr != 256 || m.NR < 2) return false;
    const int y = m.c.rel_y_in_layer - 1;
    if (y < 1 || y > m.NR - 2) return false;
    if (m.rel[0].n != 256 || m.rel[0].ldw > kAux || m.rel[0].ldw < 16) return false;
    for (int i = 0; i + 1 < m.NR; ++i) {
      const Lin& q = m.rel[1 + i];
      if (q.n != 256 || q.wpad < 256) return false;
      if (i == y ? (q.k_int < 257 || q.k_int > 259 || q.ldw != 272) : (q.k_int != 256 || q.ldw != 256)) return false;
    }
    const Lin& q = m.rel[m.NR];
    if (q.n < 1 || q.n > 3 || q.k_int != 256 || (q.ldw & 3) || q.n != m.col[m.NC - 1].n) return false;
  }
  return true;
}

// ------------------------------------------------------------------------------------------------
// The buffer groups that the context layouts share.  Every a.f() rounds to 256 bytes on its own, so the size of a layout does not depend on
// the order of its groups; the training layouts (layout_ctx, layout_bwd) keep theirs fixed all the same, and with it every offset of the
// timed path.
// ------------------------------------------------------------------------------------------------
// geometry of P points: the embedding, the aux rows [p g PE(view)], the sdf and the colour net's input rows [feat | aux | 0]
void place_geometry(const Model& m, long P, Arena& a, Ctx& x) {
  x.E = a.f((size_t)P * kEmb);
  x.AUX = a.f((size_t)P * kAux);
  x.sdf = a.f(P);
  x.ldfx = round_up(m.F + kAux, 16);
  x.featx = a.f((size_t)P * x.ldfx);
}
// the embedding cotangents of the gradient chain and the two per-point colours
void place_grad_colors(long P, Arena& a, Ctx& x) {
  x.CE0 = a.f((size_t)P * kEmb);
  x.CES = a.f((size_t)P * kEmb);
  x.gcol = a.f((size_t)P * 4);
  x.relit = a.f((size_t)P * 4);
}
// what a render keeps per ray, and the gradient / relight rows of callers that do not take them as outputs
static void place_ray_state(const Model& m, long R, Arena& a, Ctx& x) {
  x.eik_partial = a.f((size_t)R * 2);
  x.eik_sums = a.f(64);
  x.gbuf = a.f((size_t)R * m.M * 3);
  x.delta_s = m.has_relight ? a.f((size_t)R * m.M * 3) : nullptr;
}
void place_sdf_z(const Model& m, long P, Arena& a, Ctx& x) {
  x.Z.resize(m.L);
  for (int l = 0; l < m.L; ++l) x.Z[l] = a.f((size_t)P * m.Hs);
  x.ldztop = round_up(m.F + 1, 16);
}
// V[l] of the gradient chain: one buffer per layer where a backward pass reads them again, two ping-pong buffers otherwise (the chain's
// launch l reads V[l] and writes V[l - 1]).  V[L - 1] stays null: it is the broadcast row W_top[0,:]/scale
void place_sdf_v(const Model& m, long P, bool saved, Arena& a, Ctx& x) {
  x.V.assign(m.L, nullptr);
  float* pp[2] = {nullptr, nullptr};
  if (!saved && m.L >= 2) pp[0] = a.f((size_t)P * m.Hs);
  if (!saved && m.L >= 3) pp[1] = a.f((size_t)P * m.Hs);
  for (int l = 0; l + 1 < m.L; ++l) x.V[l] = saved ? a.f((size_t)P * m.Hs) : pp[l & 1];
}
static void place_sampler(const Model& m, long R, Arena& a, Ctx& x) {
  const long Ps = R * m.S;
  x.sE = a.f((size_t)Ps * kEmb);
  x.sZa = a.f((size_t)Ps * m.Hs);
  x.sZb = a.f((size_t)Ps * m.Hs);
  x.s_sdf0 = a.f(Ps);
  x.s_sdf = a.f((size_t)R * m.M);
  x.s_newz = a.f((size_t)R * 64);
  x.s_newsdf = a.f((size_t)R * 64);
}
// early-termination compaction: the index list with its per-ray counts / offsets and, where the per-layer chains run on the kept samples
// (copies), compact copies of their inputs and outputs (the chain-fused form reads its rows through the index list)
static void place_compaction(long R, long P, bool copies, Arena& a, Ctx& x) {
  x.featx_c = copies ? a.f((size_t)P * x.ldfx) : nullptr;
  x.aux_c = copies ? a.f((size_t)P * kAux) : nullptr;
  x.gcol_c = copies ? a.f((size_t)P * 4) : nullptr;
  x.relit_c = copies ? a.f((size_t)P * 4) : nullptr;
  x.delta_c = copies ? a.f((size_t)P * 4) : nullptr;
  x.p_idx = reinterpret_cast<int*>(a.f(P));
  x.p_counts = reinterpret_cast<int*>(a.f(R));
  x.p_offsets = reinterpret_cast<int*>(a.f(R + 1));
}

// Forward-only layout (cnr_render_forward_only): the same buffers as layout_ctx for everything the forward kernels exchange, but nothing that
// only the backward pass reads: two ping-pong buffers instead of the L - 1 saved V_l, no row scales, the hidden layers of the ReLU stacks
// not at all when they run chain-fused (two ping-pong buffers + the relight y-layer's input otherwise), compact copies for the
// early-termination compaction only where the per-layer chains need them.
void layout_ctx_infer(Model& m, long R, Arena& a, Ctx& x) {
  const long P = R * m.M;
  x.infer = true;
  x.infer_fused = relu_fused_shapes(m) && be_relu_chain_fwd_enabled();
  layout_weights(m, a);
  place_geometry(m, P, a, x);
  x.ldy = m.has_relight ? m.Hr + 16 : 0;
  place_grad_colors(P, a, x);
  place_ray_state(m, R, a, x);
  place_sdf_z(m, P, a, x);
  place_sdf_v(m, P, false, a, x);
  x.HC.assign(m.NC - 1, nullptr);
  x.HR.assign(m.NR, nullptr);
  x.hry = nullptr;
  if (!x.infer_fused) {
    const int hw = m.Hc > m.Hr ? m.Hc : m.Hr;
    float* hpp[2] = {a.f((size_t)P * hw), a.f((size_t)P * hw)};
    x.hry = m.has_relight ? a.f((size_t)P * x.ldy) : nullptr;
    for (int l = 0; l + 1 < m.NC; ++l) x.HC[l] = hpp[l & 1];
    for (int i = 0; i < m.NR; ++i) x.HR[i] = (i == m.c.rel_y_in_layer - 1) ? x.hry : hpp[i & 1];
  }
  place_sampler(m, R, a, x);
  place_compaction(R, P, !x.infer_fused, a, x);
  x.rsY.assign(m.L + 1, nullptr); x.rsX1.assign(m.L, nullptr); x.rsC.assign(m.NC, nullptr); x.rsR.assign(m.NR, nullptr);
  place_slack(a);
}

// Training layout (cnr_render_forward / cnr_render_backward / cnr_sample_z).  The order of the groups is part of it: see above.
void layout_ctx(Model& m, long R, Arena& a, Ctx& x) {
  const long P = R * m.M;
  layout_weights(m, a);
  place_geometry(m, P, a, x);
  x.ldy = m.has_relight ? m.Hr + 16 : 0;
  x.hry = m.has_relight ? a.f((size_t)P * x.ldy) : nullptr;
  place_grad_colors(P, a, x);
  place_ray_state(m, R, a, x);
  place_sdf_z(m, P, a, x);
  place_sdf_v(m, P, true, a, x);
  x.HC.resize(m.NC - 1);
  for (int l = 0; l + 1 < m.NC; ++l) x.HC[l] = a.f((size_t)P * m.Hc);
  x.HR.resize(m.NR);
  for (int i = 0; i < m.NR; ++i) x.HR[i] = (i == m.c.rel_y_in_layer - 1) ? x.hry : a.f((size_t)P * m.Hr);
  place_sampler(m, R, a, x);
  place_compaction(R, P, true, a, x);
  // per-point row scales of GEMM operands that the weight-gradient GEMMs read again (see Ctx)
  place_row_scales(x.rsY, m.L + 1, 1, m.L + 1, P, a);
  place_row_scales(x.rsX1, m.L, 1, m.L, P, a);
  place_row_scales(x.rsC, m.NC, 0, m.NC - 1, P, a);
  place_row_scales(x.rsR, m.NR, 0, m.NR - 1, P, a);
  place_slack(a);
}

// point ranges of a fused launch: at least four 32-point tiles per range, a multiple of 8 (two column halves per range share an XCD)
static int fdw_slots(long P) {
  long s = round_up((int)((P / 32 + 3) / 4), 8);
  if (s < 8) s = 8;
  if (s > kFdwSlots) s = kFdwSlots;
  return (int)s;
}

// slots reserved for a layer: a narrow-input layer (K <= 48) may hold two one-workgroup-per-CU launches (cnr_sweep0.hip, cnr_narrow_bwd.hip) or one
// of them + a separate GEMM over nchunk slots
int region_slots(const Lin& q, const Bwd& b) {
  const int narrow = (b.nchunk > b.cu_slots ? b.nchunk : b.cu_slots) + b.cu_slots;
  return (q.k_int <= 48 && b.cap_slots < narrow) ? narrow : b.cap_slots;
}

// the static part of head_bwd_ok (below): the streaming backward of a <= 4-wide head on a 256-wide ReLU layer
bool head_bwd_static_ok(const Lin& q, int ldaux) {
  const bool off = debug_flags().no_head_bwd;   // debugging aid: layer launch + strip launch as before
  return !off && q.n <= 4 && q.k_int == 256 && q.ldw == 256 && (ldaux & 3) == 0;
}

// the slot counts of the weight-gradient launches over P points
static void bwd_slots(long P, Bwd& b) {
  b.nchunk = dw_chunks(P);
  b.chunk_pts = round_up((int)((P + b.nchunk - 1) / b.nchunk), 16);
  b.fslots = fdw_slots(P);
  b.cap_slots = b.fslots + (b.nchunk > b.fslots ? b.nchunk : b.fslots);   // a fused pair + either a second fused pair or a separate GEMM over nchunk slots
  b.cu_slots = cu_tile_slots(P);
}

// The SDF half of the backward scratch (sdf_backward: render backward and point-query backward), as the groups between which the render
// layout places its own buffers.  grad_path = false (a query backward without a cotangent on the gradient) leaves out what only the
// second-order sweep touches.
void place_sdf_seeds(long P, bool grad_path, const Ctx& x, Arena& a, Bwd& b) {
  b.ZTOP = a.f((size_t)P * x.ldztop);
  b.gbar_a = grad_path ? a.f((size_t)P * 4) : nullptr;
}
void place_sdf_cotangents(long P, bool grad_path, Arena& a, Bwd& b) {
  b.gbar_t = grad_path ? a.f((size_t)P * 4) : nullptr;
  b.cbar = grad_path ? a.f((size_t)P * kEmb) : nullptr;
  b.ebar0 = a.f((size_t)P * kEmb);
  b.ebars = a.f((size_t)P * kEmb);
  b.pbar = a.f((size_t)P * 4);
}
void place_sdf_sweeps(const Model& m, long P, bool grad_path, Arena& a, Bwd& b) {
  b.VB.assign(m.L, nullptr); b.Z2.resize(m.L);
  for (int l = 0; l < m.L; ++l) { if (grad_path) b.VB[l] = a.f((size_t)P * m.Hs); b.Z2[l] = a.f((size_t)P * m.Hs); }
}
// the slot counts over P points and the partial-sum pool: region_slots slots for every layer of the stacks
void place_dw_pool(std::initializer_list<const std::vector<Lin>*> stacks, long P, Arena& a, Bwd& b) {
  bwd_slots(P, b);
  size_t tot = 0;
  for (auto* st : stacks)
    for (auto& q : *st) tot += DwPool::region_floats(q, region_slots(q, b));
  b.dw.place(a, tot);
}
// row scales of the SDF cotangents z-bar_l (value pairs) and, with the gradient path, q-bar_l (gradient-chain pairs)
void place_sdf_bwd_row_scales(const Model& m, long P, bool grad_path, Arena& a, Bwd& b) {
  place_row_scales(b.rsX0, m.L + 1, 1, m.L + 1, P, a);
  place_row_scales(b.rsY1, m.L + 1, 1, grad_path ? m.L : 1, P, a);
}

void layout_bwd(const Model& m, long R, const Ctx& x, Arena& a, Bwd& b) {
  const long P = R * m.M;
  place_sdf_seeds(P, true, x, a, b);
  // The 3-wide cotangents of the two heads: packed 16-byte rows when both heads take the streaming head kernel (it reads one float4 per point),
  // 16-float rows for the narrow GEMM launches otherwise (they read whole 64-byte rows: the compositor's backward then moves 58 KB per ray
  // where 12 KB are live)
  const bool packed = m.NC >= 2 && head_bwd_static_ok(m.col[m.NC - 1], m.Hc) && (m.Hc & 3) == 0 &&
                      (!m.has_relight || (m.NR >= 2 && head_bwd_static_ok(m.rel[m.NR], hr_ld(m, x, m.NR - 1)) && (m.Hr & 3) == 0));
  b.ldtop = packed ? 4 : kTop;
  b.dtop = a.f((size_t)P * b.ldtop);
  b.gc_a = a.f((size_t)P * b.ldtop);
  b.gc_b = a.f((size_t)P * 4);
  b.dctop = a.f((size_t)P * b.ldtop);
  b.dinvs = a.f(R);
  b.drd_alpha = a.f((size_t)R * 3);
  b.dAUXc = a.f((size_t)P * kAux);
  b.dAUXr = a.f((size_t)P * kAux);
  place_sdf_cotangents(P, true, a, b);
  b.dzparts = m.I == 0 ? a.f((size_t)P * 2) : nullptr;
  place_sdf_sweeps(m, P, true, a, b);
  // The cotangents of the relight / colour hidden layers (steps 2 and 3 of the backward pass) are dead before the second-order sweep (step 5)
  // writes the first VB / Z2 buffer, and everything runs on one stream: they share that memory where the widths agree (7 KB per point less)
  b.D.resize(m.NR);
  b.DC.resize(m.NC > 0 ? m.NC - 1 : 0);
  const int nshare = m.NR + (int)b.DC.size();
  const bool share = (m.NR == 0 || m.Hr == m.Hs) && m.Hc == m.Hs && nshare <= 2 * m.L;
  auto shared = [&](int k) { return (k & 1) ? b.Z2[k >> 1] : b.VB[k >> 1]; };
  for (int i = 0; i < m.NR; ++i) b.D[i] = share ? shared(i) : a.f((size_t)P * m.Hr);
  for (int l = 0; l + 1 < m.NC; ++l) b.DC[l] = share ? shared(m.NR + l) : a.f((size_t)P * m.Hc);
  place_dw_pool({&m.sdf, &m.col, &m.rel}, P, a, b);
  place_sdf_bwd_row_scales(m, P, true, a, b);
  b.rsD = a.f(P);
  place_slack(a);
}

}  // namespace cnr

using namespace cnr;

extern "C" {

int cnr_param_count(const cnr_config* cfg) {
  Model m;
  if (build_model(cfg, m)) return -1;
  return (int)m.params.size();
}

int cnr_param_info(const cnr_config* cfg, int index, char* name, int name_len, int* rows, int* cols) {
  Model m;
  return build_model(cfg, m) ? -1 : param_info(m.params, index, name, name_len, rows, cols);
}

size_t cnr_ctx_bytes(const cnr_config* cfg, int64_t n_rays) {
  Model m;
  if (build_model(cfg, m) || n_rays <= 0) return 0;
  Ctx x;
  return layout_size(nullptr, [&](Arena& a) { layout_ctx(m, n_rays, a, x); });
}

size_t cnr_bwd_scratch_bytes(const cnr_config* cfg, int64_t n_rays) {
  Model m;
  if (build_model(cfg, m) || n_rays <= 0) return 0;
  Ctx x;
  Bwd b;
  layout_size(nullptr, [&](Arena& a) { layout_ctx(m, n_rays, a, x); });
  return layout_size(nullptr, [&](Arena& a) { layout_bwd(m, n_rays, x, a, b); });
}

size_t cnr_infer_scratch_bytes(const cnr_config* cfg, int64_t n_rays) {
  Model m;
  if (build_model(cfg, m) || n_rays <= 0) return 0;
  Ctx x;
  return layout_size(nullptr, [&](Arena& a) { layout_ctx_infer(m, n_rays, a, x); });
}

}  // extern "C"
