// Host orchestration of the Color-NeuS render path + the C ABI (include/colorneus_render.h).
//
// Forward  (reference NeuS.forward, NeuS.py:294-408):
//   weight preparation -> coarse z -> [SDF value chain -> up_sample -> merge] x K -> fine set-up ->
//   SDF chain (stores pre-activations) -> analytic gradient chain (reverse sweep, replaces the reference's second
//   SDF forward + autograd.grad, fields.py:105-115) -> colour chain -> relight chain -> alpha + compositing.
// Backward (autograd of the above incl. double backward through grad_x SDF):
//   compositor backward -> relight / colour chains backward -> second-order forward sweep through the SDF net ->
//   SDF value backward -> weight-gradient GEMMs (two operand pairs for the SDF net) -> weight-norm backward.
//
// This file contains no arithmetic on tensor data: it only sizes buffers, builds kernel descriptors and enqueues
// kernels through cnr_backend.h.  It is shared verbatim by the HIP build and the CPU-emulation build (tests only).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/colorneus_render.h"
#include "cnr_backend.h"

namespace cnr {

// The library's ONLY read of the environment (cnr_debug.h lists the switches): parsed once, on first use.
const DebugFlags& debug_flags() {
  static const DebugFlags flags = [] {
    DebugFlags d;
    struct B { const char* name; bool DebugFlags::*m; };
    struct I { const char* name; int DebugFlags::*m; };
    static const B bools[] = {
        {"CNR_NO_FUSED", &DebugFlags::no_fused}, {"CNR_NO_CHAIN_FWD", &DebugFlags::no_chain_fwd}, {"CNR_NO_CHAIN_SDF", &DebugFlags::no_chain_sdf},
        {"CNR_NO_FDW", &DebugFlags::no_fdw}, {"CNR_FDW_SPLIT", &DebugFlags::fdw_split},
        {"CNR_NO_TOP_FUSE", &DebugFlags::no_top_fuse}, {"CNR_NO_HEAD_BWD", &DebugFlags::no_head_bwd}, {"CNR_NO_HEAD_FWD", &DebugFlags::no_head_fwd},
        {"CNR_NO_STRIP_BWD", &DebugFlags::no_strip_bwd}, {"CNR_NO_SAMPLER_FUSE", &DebugFlags::no_sampler_fuse}, {"CNR_NO_SWEEP0", &DebugFlags::no_sweep0},
        {"CNR_NO_NARROW_BWD", &DebugFlags::no_narrow_bwd}, {"CNR_NO_NARROW_DX", &DebugFlags::no_narrow_dx}, {"CNR_DISABLE_WS", &DebugFlags::disable_ws},
        {"CNR_WS_GENERIC", &DebugFlags::ws_generic}, {"CNR_WS_NOSTREAM", &DebugFlags::ws_nostream}, {"CNR_DW_FP32", &DebugFlags::dw_fp32},
        {"CNR_DW_BF16", &DebugFlags::dw_bf16}, {"CNR_ROCTX", &DebugFlags::roctx}};
    static const I ints[] = {
        {"CNR_WS_SERP", &DebugFlags::ws_serp},
#ifdef CNR_TUNING
        {"CNR_WS_KINDS", &DebugFlags::ws_kinds}, {"CNR_WS_MINW", &DebugFlags::ws_minw}, {"CNR_WS_WGS", &DebugFlags::ws_wgs}, {"CNR_WS_MINTPW", &DebugFlags::ws_mintpw},
        {"CNR_CHAIN_WGS", &DebugFlags::chain_wgs}, {"CNR_CHAIN_SHAPE", &DebugFlags::chain_shape}, {"CNR_CHAIN_FWD_RT", &DebugFlags::chain_fwd_rt},
        {"CNR_FDW_NOREV", &DebugFlags::fdw_norev}, {"CNR_FDW_REVMODE", &DebugFlags::fdw_revmode},
        {"CNR_FDW_DBG", &DebugFlags::fdw_dbg}, {"CNR_CHAIN_FWD_DBG", &DebugFlags::chain_fwd_dbg},
#endif
    };
    auto env = [](const char* name) { return getenv(name); };   // <- the one call site
    const char* v;
    for (const B& b : bools) d.*(b.m) = env(b.name) != nullptr;
    for (const I& i : ints) if ((v = env(i.name)) != nullptr) d.*(i.m) = *v ? atoi(v) : 1;
#ifdef CNR_TUNING
    if ((v = env("CNR_CHAIN_SDF_MAXP")) != nullptr) d.chain_sdf_maxp = atol(v);
#endif
    return d;
  }();
  return flags;
}

static thread_local std::string g_err;
static int fail(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return -1;
}

struct Lin {
  int n = 0, k_ref = 0, k_int = 0;
  int nseg = 0;
  Segment seg[4];
  int ldw = 0, npad = 0, ldwt = 0, kpad = 0;
  int wpad = 0;                                   // rows of W / its planes / bias that exist (zero beyond n): npad, or more when a tail fill widens the launch
  bool wn = false;
  int row_rot = 0;            // internal row i = reference row (i + row_rot) % n
  int p_b = -1, p_g = -1, p_v = -1;
  float *W = nullptr, *Wt = nullptr, *bias = nullptr;
  unsigned short *Wp = nullptr, *Wtp = nullptr;   // two f16 planes (hi, lo) of the row-scaled W / Wt
  unsigned short* Wf = nullptr;                   // the planes of W in the fragment-major order of the chain-fused kernels
  float *Wps = nullptr, *Wtps = nullptr;          // per-row inverse scales
  std::string name;
  void finish_dims() {
    ldw = round_up(k_int, 16);
    npad = round_up(n, 32);
    wpad = npad;
    ldwt = round_up(n, 16);
    kpad = round_up(k_int, 32);
  }
  size_t bytes() const { return ((size_t)wpad * ldw + (size_t)kpad * ldwt + wpad) * sizeof(float); }
};

struct ParamInfo { std::string name; int rows, cols; };

struct Model {
  cnr_config c;
  int S, I, M, K;
  int emb;            // 3 + 6*multires
  int Hs, L;          // SDF hidden width, number of hidden layers (top linear layer has index L)
  int F;              // feature width = sdf_d_out - 1
  int Hc, NC;         // colour hidden width, number of linear layers
  int Hr, NR;         // relight hidden width, number of rl_mlp layers (+1 in_layer)
  int nv;             // width of PE(view dir) in AUX (0 if unused)
  int mv;             // multires_view used for AUX
  int naux;           // 6 + nv
  bool has_relight;
  std::vector<Lin> sdf, col, rel;   // rel[0] = in_layer, rel[1+i] = rl_mlp[i]
  std::vector<ParamInfo> params;
  int p_variance = -1;
  bool skip(int l) const { return (c.sdf_skip_mask >> l) & 1; }
};

static void identity_seg(Lin& l) {
  l.k_int = l.k_ref;
  l.nseg = 1;
  l.seg[0] = {0, 0, l.k_ref};
}

// Parameter registration.  The order is part of the ABI (checkpoints, cnr_param_info): bias, then weight_g / weight_v (or weight) for the
// SDF and colour stacks (add_linear_params); weight, then bias for the plain layers of the relight and background networks (add_weight_bias).
static void add_linear_params(std::vector<ParamInfo>& params, Lin& l, const std::string& prefix, bool wn) {
  l.name = prefix;
  l.wn = wn;
  l.p_b = (int)params.size();
  params.push_back({prefix + ".bias", l.n, 1});
  if (wn) {
    l.p_g = (int)params.size();
    params.push_back({prefix + ".weight_g", l.n, 1});
  }
  l.p_v = (int)params.size();
  params.push_back({prefix + (wn ? ".weight_v" : ".weight"), l.n, l.k_ref});
}
static void add_weight_bias(std::vector<ParamInfo>& params, Lin& l, const std::string& name) {
  l.name = name; l.wn = false;
  l.p_v = (int)params.size(); params.push_back({name + ".weight", l.n, l.k_ref});
  l.p_b = (int)params.size(); params.push_back({name + ".bias", l.n, 1});
}
static int param_info(const std::vector<ParamInfo>& params, int index, char* name, int name_len, int* rows, int* cols) {
  if (index < 0 || index >= (int)params.size()) return fail("parameter index out of range");
  if (name && name_len > 0) snprintf(name, name_len, "%s", params[index].name.c_str());
  if (rows) *rows = params[index].rows;
  if (cols) *cols = params[index].cols;
  return 0;
}

static int build_model(const cnr_config* cfg, Model& m) {
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

// ------------------------------------------------------------------------------------------------
// bump allocator over a caller-provided buffer (dry-run when base == nullptr)
// ------------------------------------------------------------------------------------------------
struct Arena {
  char* base; size_t off = 0;
  explicit Arena(void* b) : base((char*)b) {}
  float* f(size_t count) {
    size_t bytes = round_up_sz(count * sizeof(float), 256);
    float* p = base ? (float*)(base + off) : nullptr;
    off += bytes;
    return p;
  }
};

// Lay out and check: layout_checked runs a layout function over a caller's buffer and refuses a buffer that is too small -- THE wording of that message;
// layout_size is the dry run behind every *_bytes query of the ABI (the same layout function, so a query cannot disagree with its entry point).
template <class Layout> static size_t layout_size(void* buf, Layout&& layout) {
  Arena a(buf);
  layout(a);
  return a.off;
}
template <class Layout> static int layout_checked(const char* what, void* buf, size_t bytes, Layout&& layout) {
  const size_t need = layout_size(buf, layout);
  return need > bytes ? fail("%s too small: need %zu bytes, got %zu", what, need, bytes) : 0;
}

struct Ctx {   // forward-saved state
  // effective weights live in the Lin structs
  float *E, *AUX, *sdf, *featx, *hry, *CE0, *CES, *gcol, *relit, *eik_partial, *eik_sums;
  float *gbuf, *delta_s;   // [P][3] each: sdf gradients / relight offsets when the caller does not take them as outputs ("loss only" training)
  // early-termination compaction (inference): compact copies of the colour-chain inputs/outputs + index list
  float *featx_c, *aux_c, *gcol_c, *relit_c, *delta_c; int *p_idx, *p_counts, *p_offsets;
  int ldfx = 0, ldy = 0;   // row strides of featx = [feat | aux | 0] and hry = [relight hidden | global colour | 0]
  std::vector<float*> Z, V, HC, HR;
  // per-point row scales of GEMM operands that the weight-gradient GEMMs read again (LayerGemm::rs_out -> DwGemm::sx / sy):
  // rsY[l] input of SDF layer l, rsX1[l] = sigma'(z_l) v_l, rsC[l] input of colour layer l, rsR[i] input of relight rl_mlp layer i
  std::vector<float*> rsY, rsX1, rsC, rsR;
  // sampler scratch (forward only)
  float *sE, *sZa, *sZb, *s_sdf0, *s_sdf, *s_newz, *s_newsdf;
  int ldztop;
  bool infer = false;        // forward-only layout (cnr_render_forward_only): nothing is kept for a backward pass
  bool infer_fused = false;  // ... and the colour / relight stacks run chain-fused (no hidden-layer buffers, compaction by an index list)
};

static int hr_ld(const Model& m, const Ctx& x, int i) { return i == m.c.rel_y_in_layer - 1 ? x.ldy : m.Hr; }

static void place_lin(Lin& q, Arena& a) {
  q.W = a.f((size_t)q.wpad * q.ldw);
  q.Wt = a.f((size_t)q.kpad * q.ldwt);
  q.bias = a.f(q.wpad);
  q.Wp = reinterpret_cast<unsigned short*>(a.f((size_t)q.wpad * q.ldw));
  q.Wtp = reinterpret_cast<unsigned short*>(a.f((size_t)q.kpad * q.ldwt));
  q.Wps = a.f(q.wpad > 256 ? q.wpad : 256);   // (the fused kernels read 256 column scales; entries >= npad are never used)
  q.Wtps = a.f(q.kpad > 256 ? q.kpad : 256);  // (likewise)
  q.Wf = (q.ldw <= 304) ? reinterpret_cast<unsigned short*>(a.f((size_t)8 * (q.ldw / 16) * 2 * 64 * 8 / 2)) : nullptr;   // (<= 19 k16 blocks: 256 + 48)
}

static void layout_weights(Model& m, Arena& a) {
  for (auto& q : m.sdf) place_lin(q, a);
  for (auto& q : m.col) place_lin(q, a);
  for (auto& q : m.rel) place_lin(q, a);
}

// The weight operand of a layer launch over P rows: y = x W^T (fwd_gemm: W, its planes and row scales) or dx = dy W (bwd_gemm: the
// transposed copies).  THE place where a Lin becomes LayerGemm fields; a call site sets only its input view, its epilogue and what differs.
static LayerGemm fwd_gemm(const Lin& q, long P) {
  LayerGemm g;
  g.W = q.W; g.ldw = q.ldw; g.Wp = q.Wp; g.wp_stride = (long)q.wpad * q.ldw; g.w_rows = q.wpad; g.wscale = q.Wps; g.N = q.n; g.K = q.k_int; g.P = P;
  return g;
}
static LayerGemm bwd_gemm(const Lin& q, long P) {   // (w_rows stays at its default: the launches take round_up(N, 32) rows of W^T)
  LayerGemm g;
  g.W = q.Wt; g.ldw = q.ldwt; g.Wp = q.Wtp; g.wp_stride = (long)q.kpad * q.ldwt; g.wscale = q.Wtps; g.N = q.k_int; g.K = q.n; g.P = P;
  return g;
}
// ... and of the one-pass narrow backward (cnr_narrow_bwd.hip), which stages all kpad rows of the W^T planes
static void narrow_bwd_weights(NarrowBwd& nb, const Lin& q) {
  const LayerGemm t = bwd_gemm(q, 0);
  nb.Wp = t.Wp; nb.wp_stride = t.wp_stride; nb.ldw = t.ldw; nb.w_rows = q.kpad; nb.wscale = t.wscale;
}
static View direct_view(const float* a, int lda) {
  View v;
  v.a = a; v.lda = lda;
  return v;
}

// shapes the chain-fused forward of the ReLU stacks takes (cnr_chain_fwd.hip).  THE definition: relu_chains_fused below starts with this test (what it
// checks after that are buffer pointers), and layout_ctx_infer decides by it that the forward-only layout needs no hidden-layer buffers.
static bool relu_fused_shapes(const Model& m) {
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
static void place_geometry(const Model& m, long P, Arena& a, Ctx& x) {
  x.E = a.f((size_t)P * kEmb);
  x.AUX = a.f((size_t)P * kAux);
  x.sdf = a.f(P);
  x.ldfx = round_up(m.F + kAux, 16);
  x.featx = a.f((size_t)P * x.ldfx);
}
// the embedding cotangents of the gradient chain and the two per-point colours
static void place_grad_colors(long P, Arena& a, Ctx& x) {
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
static void place_sdf_z(const Model& m, long P, Arena& a, Ctx& x) {
  x.Z.resize(m.L);
  for (int l = 0; l < m.L; ++l) x.Z[l] = a.f((size_t)P * m.Hs);
  x.ldztop = round_up(m.F + 1, 16);
}
// V[l] of the gradient chain: one buffer per layer where a backward pass reads them again, two ping-pong buffers otherwise (the chain's
// launch l reads V[l] and writes V[l - 1]).  V[L - 1] stays null: it is the broadcast row W_top[0,:]/scale
static void place_sdf_v(const Model& m, long P, bool saved, Arena& a, Ctx& x) {
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
// per-point row scales rs[lo .. hi) of a stack of n launches (null elsewhere)
static void place_row_scales(std::vector<float*>& rs, int n, int lo, int hi, long P, Arena& a) {
  rs.assign(n, nullptr);
  for (int l = lo; l < hi; ++l) rs[l] = a.f(P);
}
static void place_slack(Arena& a) { a.f(1024); }   // GEMM tiles may read (never use) a few columns past the last row of a buffer

// Forward-only layout (cnr_render_forward_only): the same buffers as layout_ctx for everything the forward kernels exchange, but nothing that
// only the backward pass reads: two ping-pong buffers instead of the L - 1 saved V_l, no row scales, the hidden layers of the ReLU stacks
// not at all when they run chain-fused (two ping-pong buffers + the relight y-layer's input otherwise), compact copies for the
// early-termination compaction only where the per-layer chains need them.
static void layout_ctx_infer(Model& m, long R, Arena& a, Ctx& x) {
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
static void layout_ctx(Model& m, long R, Arena& a, Ctx& x) {
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

// ------------------------------------------------------------------------------------------------
// The pool of weight-gradient partial sums, shared by every backward entry point.  A layer's region is [slots][npad][ldw] partial sums +
// [slots][npad] column sums (the bias gradient); every layer keeps its own until one batched reduction at the end.  A layout sums
// region_floats over its layers and places the pool; the launch code takes the regions in its own order, and take refuses to leave the
// pool.  Several launches may fill consecutive slot groups of one region (SDF layers: value pair | gradient-chain pair, each either fused
// into its layer launch or a separate GEMM); finish queues the one reduction over all of them.  Only the group at slot 0 carries column
// sums.  How many slots a layer gets is the caller's policy (region_slots, dw_chunks).  Who fills which slot group is decided by the
// callers' plans before they take a region: plan_sdf_backward (SdfBwdPlan: per SDF layer the producer of each pair, value_slots and
// grad_slots with the gradient group at offset value_slots, checked once against region_slots), plan_stack_layer (a ReLU-stack layer) and
// narrow_pass_ok (a narrow-input layer).  The execution code reads the plan and never re-derives a slot count.
// ------------------------------------------------------------------------------------------------
struct DwRegion { float* part = nullptr; float* csum = nullptr; };   // (part == nullptr: refused by DwPool::take)
struct DwPool {
  float* base = nullptr;
  size_t floats = 0, off = 0;
  std::vector<FinishWeight> pending;   // reductions queued by finish, issued as one launch by flush

  static size_t csum_floats(const Lin& q, int slots) { return round_up_sz((size_t)slots * q.npad, 64); }
  static size_t region_floats(const Lin& q, int slots) { return round_up_sz((size_t)slots * q.npad * q.ldw, 64) + csum_floats(q, slots); }
  void place(Arena& a, size_t n) {
    floats = n; off = 0;
    base = a.f(n);
    pending.clear();
  }
  // the next region; past the end of the pool: an error (cnr_last_error) and a null region, into which the caller launches nothing
  DwRegion take(const Lin& q, int slots) {
    DwRegion r;
    const size_t need = region_floats(q, slots);
    if (!base) return r;   // (a dry-run layout: there is nothing to hand out, and nothing to overrun)
    if (need > floats - off) {
      fail("weight-gradient pool: %d slots of layer %s need %zu floats, %zu of %zu are left", slots, q.name.c_str(), need, floats - off, floats);
      return r;
    }
    r.part = base + off;
    off += need;
    r.csum = base + off - csum_floats(q, slots);
    return r;
  }
  // THE place where a Lin becomes a FinishWeight: the reduction over the first nslots slots of r (column sums over the first ncolsum)
  void finish(const Lin& q, const DwRegion& r, int nslots, int ncolsum, const float* const* params, float* const* dparams) {
    FinishWeight f;
    f.partial = r.part; f.nchunk = nslots; f.npad = q.npad; f.ldk = q.ldw; f.colsum = ncolsum > 0 ? r.csum : nullptr; f.ncolsum = ncolsum;
    f.g = q.p_g >= 0 ? params[q.p_g] : nullptr; f.v = params[q.p_v];
    f.n = q.n; f.k_ref = q.k_ref; f.nseg = q.nseg;
    for (int i = 0; i < q.nseg; ++i) f.seg[i] = q.seg[i];
    f.dg = q.p_g >= 0 ? dparams[q.p_g] : nullptr; f.dv = dparams[q.p_v]; f.db = dparams[q.p_b]; f.row_rot = q.row_rot;
    pending.push_back(f);
  }
  // the columns >= 256 of the layer queued last were filled by be_strip_bwd, over nslots slots
  void strip_columns_of_last_finish(int nslots) { pending.back().col_hi = 256; pending.back().nchunk_hi = nslots; }
  void flush(cnr_stream s) {   // all queued reductions (+ weight-norm backward) in one launch
    if (!pending.empty()) be_finish_weights(pending.data(), (int)pending.size(), s);
    pending.clear();
  }
};

struct Bwd {   // backward scratch
  float *ZTOP, *gbar_a, *dtop, *gc_a, *gc_b, *dctop, *dinvs, *drd_alpha, *dAUXc, *dAUXr, *gbar_t, *cbar, *ebar0, *ebars, *pbar, *dzparts;
  std::vector<float*> D, DC, VB, Z2;
  std::vector<float*> rsX0, rsY1;   // row scales of the SDF cotangents z-bar_l (value pair) and q-bar_l (gradient-chain pair)
  float* rsD;                       // row scales of the colour / relight cotangent consumed right after its layer GEMM
  DwPool dw;                          // per-layer weight-gradient partial sums
  int nchunk; long chunk_pts;
  int fslots;                         // slots (point ranges) of a fused layer + weight-gradient launch (cnr_gemm_fdw.hip)
  int cap_slots;                      // slots reserved per layer in the pool: fslots + max(nchunk, fslots)
  int cu_slots;                       // slots of a one-workgroup-per-CU launch over 32-point tiles (cnr_sweep0.hip, cnr_narrow_bwd.hip)
  int ldtop;                          // row stride of dtop / gc_a / dctop: 4 when both heads run the streaming head kernel, kTop for the narrow GEMM launches
};

// point ranges of a fused launch: at least four 32-point tiles per range, a multiple of 8 (two column halves per range share an XCD)
static int fdw_slots(long P) {
  long s = round_up((int)((P / 32 + 3) / 4), 8);
  if (s < 8) s = 8;
  if (s > kFdwSlots) s = kFdwSlots;
  return (int)s;
}

// slots reserved for a layer: a narrow-input layer (K <= 48) may hold two one-workgroup-per-CU launches (cnr_sweep0.hip, cnr_narrow_bwd.hip) or one
// of them + a separate GEMM over nchunk slots
static int region_slots(const Lin& q, const Bwd& b) {
  const int narrow = (b.nchunk > b.cu_slots ? b.nchunk : b.cu_slots) + b.cu_slots;
  return (q.k_int <= 48 && b.cap_slots < narrow) ? narrow : b.cap_slots;
}

// the static part of head_bwd_ok (below): the streaming backward of a <= 4-wide head on a 256-wide ReLU layer
static bool head_bwd_static_ok(const Lin& q, int ldaux) {
  const bool off = debug_flags().no_head_bwd;   // debugging aid: layer launch + strip launch as before
  return !off && q.n <= 4 && q.k_int == 256 && q.ldw == 256 && (ldaux & 3) == 0;
}

// point chunks (slots) of a separate weight-gradient GEMM: one workgroup per CU as soon as every chunk has a few 16-point slabs
static int dw_chunks(long P) {
  const long nch = P / 128;
  return nch < 1 ? 1 : nch > 256 ? 256 : (int)nch;
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
static void place_sdf_seeds(long P, bool grad_path, const Ctx& x, Arena& a, Bwd& b) {
  b.ZTOP = a.f((size_t)P * x.ldztop);
  b.gbar_a = grad_path ? a.f((size_t)P * 4) : nullptr;
}
static void place_sdf_cotangents(long P, bool grad_path, Arena& a, Bwd& b) {
  b.gbar_t = grad_path ? a.f((size_t)P * 4) : nullptr;
  b.cbar = grad_path ? a.f((size_t)P * kEmb) : nullptr;
  b.ebar0 = a.f((size_t)P * kEmb);
  b.ebars = a.f((size_t)P * kEmb);
  b.pbar = a.f((size_t)P * 4);
}
static void place_sdf_sweeps(const Model& m, long P, bool grad_path, Arena& a, Bwd& b) {
  b.VB.assign(m.L, nullptr); b.Z2.resize(m.L);
  for (int l = 0; l < m.L; ++l) { if (grad_path) b.VB[l] = a.f((size_t)P * m.Hs); b.Z2[l] = a.f((size_t)P * m.Hs); }
}
// the slot counts over P points and the partial-sum pool: region_slots slots for every layer of the stacks
static void place_dw_pool(std::initializer_list<const std::vector<Lin>*> stacks, long P, Arena& a, Bwd& b) {
  bwd_slots(P, b);
  size_t tot = 0;
  for (auto* st : stacks)
    for (auto& q : *st) tot += DwPool::region_floats(q, region_slots(q, b));
  b.dw.place(a, tot);
}
// row scales of the SDF cotangents z-bar_l (value pairs) and, with the gradient path, q-bar_l (gradient-chain pairs)
static void place_sdf_bwd_row_scales(const Model& m, long P, bool grad_path, Arena& a, Bwd& b) {
  place_row_scales(b.rsX0, m.L + 1, 1, m.L + 1, P, a);
  place_row_scales(b.rsY1, m.L + 1, 1, grad_path ? m.L : 1, P, a);
}

static void layout_bwd(const Model& m, long R, const Ctx& x, Arena& a, Bwd& b) {
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

// ------------------------------------------------------------------------------------------------
// sdf_only: the SDF layers alone (point queries: the other entries of params may be null)
// THE place where a Lin becomes a PrepWeight (g only with weight norm) and the two SplitJobs of its f16 planes (W and W^T)
static PrepWeight prep_desc(const Lin& q, const float* const* params) {
  PrepWeight p;
  p.g = q.p_g >= 0 ? params[q.p_g] : nullptr;
  p.v = params[q.p_v];
  p.b = params[q.p_b];
  p.n = q.n; p.k_ref = q.k_ref;
  p.nseg = q.nseg;
  for (int i = 0; i < q.nseg; ++i) p.seg[i] = q.seg[i];
  p.W = q.W; p.ldw = q.ldw; p.npad = q.wpad;
  p.Wt = q.Wt; p.ldwt = q.ldwt; p.kpad = q.kpad;
  p.bias = q.bias; p.row_rot = q.row_rot;
  return p;
}
static void add_split_jobs(const Lin& q, std::vector<SplitJob>& sj) {
  sj.push_back(SplitJob{q.W, q.wpad, q.ldw, q.Wp, q.Wps});
  sj.push_back(SplitJob{q.Wt, q.kpad, q.ldwt, q.Wtp, q.Wtps});
}
// effective weights of the layers (one launch) and their f16 planes (one launch)
static void prep_layers(const std::vector<Lin*>& layers, const float* const* params, cnr_stream s) {
  std::vector<PrepWeight> pw;
  std::vector<SplitJob> sj;
  for (const Lin* q : layers) { pw.push_back(prep_desc(*q, params)); add_split_jobs(*q, sj); }
  be_prep_weights(pw.data(), (int)pw.size(), s);
  be_split_planes_many(sj.data(), (int)sj.size(), s);
}
static void prep_all(Model& m, const float* const* params, cnr_stream s, bool sdf_only = false) {
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
static View sdf_input_view(const Model& m, int l, const float* E, const float* const* Z) {
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

static void sdf_chain(const Model& m, long n, const float* E, float* const* Z, float* sdf_out, float* feat_out, int ld_feat,
                      float top_scale, cnr_stream s, float* const* rs = nullptr /* [L+1] row scales of the layer inputs, see Ctx::rsY */) {
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
// The cotangents of the skip-connection embedding leave the split epilogues through o2 at column offset split % 4, which makes
// their 16-byte stores aligned; every reader of those buffers (CES, ebars) adds the same offset.
static int skip_off(const Model& m) {
  for (int l = 1; l < m.L; ++l) if (m.skip(l)) return m.sdf[l - 1].n & 3;
  return 0;
}

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

static int top_skip(const Model& m) {   // the highest layer fed by a skip connection (-1: none)
  for (int l = m.L - 1; l >= 1; --l) if (m.skip(l)) return l;
  return -1;
}
static bool has_skip(const Model& m) {
  for (int l = 1; l < m.L; ++l) if (m.skip(l)) return true;
  return false;
}

// E (and AUX[., 0:3] where the context has aux rows) of n explicit points, or of n lattice points from index `start` on when pts is null
static void embed_points(const Model& m, const float* pts, long n, float* E, float* AUX, cnr_stream s, const float* bmin = nullptr,
                         const float* bmax = nullptr, int res = 0, long start = 0) {
  EmbedPts ep;
  ep.pts = pts; ep.n = n; ep.res = res; ep.start = start;
  for (int c = 0; c < 3; ++c) { ep.bmin[c] = bmin ? bmin[c] : 0.f; ep.bmax[c] = bmax ? bmax[c] : 0.f; }
  ep.scale = m.c.sdf_scale; ep.multires = m.c.sdf_multires; ep.E = E; ep.AUX = AUX;
  be_embed_pts(ep, s);
}

// The point pipeline on the P embedded points of a filled context: SDF value chain (sdf, feature rows into featx, Z[l]) -> analytic gradient
// chain -> be_grad_finish (the gradient rows; g and, where asked, PE(view) into the aux rows).  Row scales are stored where the context
// holds them (rsY / rsX1 entries that are not null), AUX is written where the context has it.
struct PointOpts {
  bool grad = true;             // false: the value chain alone
  float* grad_out = nullptr;    // [P][3]
  bool aux_to_featx = true;     // the aux row is copied behind the features (the colour net's input rows)
  int neg_g_as_view = 0;        // vertex colouring: view_dirs = -g
  int multires_view = 0;
};
static void point_pipeline(const Model& m, long P, const Ctx& x, const PointOpts& o, cnr_stream s) {
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

static View color_input_view(const Model& m, int l, const Ctx& x) {
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

static View relight_input_view(const Model& m, int i /* rl_mlp index, -1 = in_layer */, const Ctx& x) {
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

static int check_backend(const char* what) {
  char msg[256];
  if (be_check_last_error(msg, sizeof msg) != 0) return fail("%s: %s", what, msg);
  return 0;
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

// ------------------------------------------------------------------------------------------------
// separate weight-gradient GEMM into slots [slot0, slot0 + nchunk) of a region (bias column sums only for a group at slot 0)
static void dw_into_region(const Lin& q, DwGemm& g, const DwRegion& r, int slot0, int nchunk, long P, bool with_bias, cnr_stream s, int kmain = 0) {
  with_bias = with_bias && slot0 == 0;
  g.N = q.n; g.K = kmain > 0 ? kmain : q.k_int;   // (kmain: the columns beyond it are formed by be_strip_bwd)
  g.nchunk = nchunk; g.chunk_pts = round_up((int)((P + nchunk - 1) / nchunk), 16);
  g.partial = r.part + (size_t)slot0 * q.npad * q.ldw; g.Npad = q.npad; g.ldk = q.ldw; g.colsum = with_bias ? r.csum : nullptr;
  be_dw_gemm(g, s);   // (which of its 256 x 256 tiles run split-f16: dw_main_tile, from the row scales g carries)
}
// layer launch + its weight-gradient pair (d.X[0] / d.Y[0]: the pair as a plain weight-gradient GEMM -- what the CPU emulation and the HIP
// backend's unfused fallback run; se = row scales of the epilogue-side operand) into slots [slot0, slot0 + b.fslots) of a region
static void fused_into_region(const Lin& q, const LayerGemm& g, DwGemm& d, const float* se, int transposed, const DwRegion& r, int slot0, Bwd& b,
                              bool with_bias, cnr_stream s, int kmain = 0, const DwFuse* xrow = nullptr, int rev = 0) {
  with_bias = with_bias && slot0 == 0 && !transposed;
  DwFuse f;
  if (xrow) f = *xrow;   // (the extra-row request; everything else is set below)
  const bool no_rev = debug_flags().fdw_norev != 0;   // tuning aid: every fused launch walks its ranges upwards
  const int rev_mode = debug_flags().fdw_revmode;    // tuning aid: 1 = the opposite parities, 2 = every launch downwards
  f.rev = no_rev ? 0 : (rev_mode == 1 ? !rev : (rev_mode == 2 ? 1 : rev));
  f.se = se; f.partial = r.part + (size_t)slot0 * q.npad * q.ldw; f.Npad = q.npad; f.ldk = q.ldw; f.colsum = with_bias ? r.csum : nullptr;
  f.transposed = transposed; f.nslots = b.fslots;
  d.npairs = 1; d.P = g.P; d.N = q.n; d.K = kmain > 0 ? kmain : q.k_int; d.nchunk = b.fslots; d.chunk_pts = round_up((int)((g.P + b.fslots - 1) / b.fslots), 16);
  d.partial = f.partial; d.Npad = q.npad; d.ldk = q.ldw; d.colsum = f.colsum;
  be_layer_dw_gemm(g, d, f, s);
}

// A 256-wide layer with a few more input columns (relight y-layer: + rgb; colour layer 0: + p, g): the cotangent of those columns and their
// weight-gradient strip in one streaming pass over the layer's output cotangent (be_strip_bwd) instead of a narrow layer launch + a strip
// launch; the main launches then cover the 256 x 256 part only.
static bool strip_bwd_ok(const Lin& q, const LayerGemm& g, const DwGemm& d) {
  const bool off = debug_flags().no_strip_bwd;   // debugging aid: narrow layer launch + strip launch as before
  const int nt = q.k_int - 256;
  return !off && q.n == 256 && nt >= 1 && nt <= 8 && q.ldw >= 256 + nt && g.A.kind == VK_DIRECT && (g.A.lda & 3) == 0 && g.A.scale == 1.0f &&
         (g.E.kind == EK_RELU_MASK || g.E.kind == EK_SPLIT) && g.E.split == 256 && g.E.bias == nullptr &&
         d.Y[0].kind == VK_DIRECT && d.Y[0].scale == 1.0f && d.npairs == 1;
}
// narrows g to its 256 main columns and returns the strip launch, complete but for the region (to be issued after the main launches; then
// DwPool::strip_columns_of_last_finish)
static StripBwd take_strips(const Lin& q, LayerGemm& g, const DwGemm& d, const Bwd& b) {
  StripBwd sb;
  sb.dout = g.A.a; sb.ldo = g.A.lda; sb.P = g.P; sb.nt = q.k_int - 256; sb.Wt = q.Wt; sb.ldwt = q.ldwt;
  sb.tail = g.E.o2 ? g.E.o2 + (g.E.kind == EK_SPLIT ? g.E.o2_off : 0) : nullptr; sb.ldt = g.E.ld2;
  sb.tail_scale = g.E.kind == EK_SPLIT ? g.E.scale : 1.0f;
  sb.y = d.Y[0].a + 256; sb.ldy = d.Y[0].lda;
  sb.npad = q.npad; sb.ldk = q.ldw; sb.nslots = b.nchunk;   // (partial: the layer's region, once it is taken)
  g.N = 256; g.E.n_out = 256; g.E.o2 = nullptr;
  return sb;
}

// backward of a narrow head (<= 4 outputs on a <= 256-wide ReLU layer) in one streaming launch: cotangent of the layer below + weight / bias gradient
static bool head_bwd_ok(const Lin& q, const LayerGemm& g) {
  return head_bwd_static_ok(q, g.E.ldaux) && (g.E.ld1 & 3) == 0 && g.A.kind == VK_DIRECT && (g.A.lda & 3) == 0 && g.E.kind == EK_RELU_MASK &&
         g.E.split >= q.k_int && g.E.aux != nullptr && g.E.o1 != nullptr;
}
// THE plain weight gradient of a layer: a region of cap slots, one GEMM of g's operand pairs over its first nchunk slots, the reduction queued
static int plain_dw(DwPool& pool, const Lin& q, DwGemm& g, int cap, int nchunk, const float* const* params, float* const* dparams, cnr_stream s) {
  const DwRegion r = pool.take(q, cap);
  if (!r.part) return -1;
  dw_into_region(q, g, r, 0, nchunk, g.P, true, s);
  pool.finish(q, r, nchunk, nchunk, params, dparams);
  return 0;
}

// Walk direction (DwFuse::rev) of the fused launch that `pos` launches of its chain precede: the launches of a chain alternate, so that each
// starts on the rows its producer wrote last (still in L2 / Infinity Cache).  first_rev is the direction of the chain's first launch: upwards
// (0) for the ReLU stacks, whose first launch is the head kernel, which walks upwards, and for the sweep; downwards (1) for the value backward.
// The parities are fixed per launch site, so the order of every sum is deterministic.
static int walk_rev(int pos, int first_rev = 0) { return (pos + first_rev) & 1; }

// Backward of one layer of a ReLU stack (relight rl_mlp, colour): g = the launch that forms the cotangent of the layer's input, d = its
// weight-gradient pair (X = the output cotangent, Y = the forward input, sy = rs_in, the row scales the forward saved for that input).
// The decision, made before the region is taken and before any launch: a narrow head takes the streaming head kernel; otherwise the extra
// input columns of a 256 + few wide layer go to the strip launch (g is narrowed to its main columns) and the rest is one fused layer +
// weight-gradient launch where the shape allows, or a layer launch and a weight-gradient launch.
// nslots: slots of the (main) weight-gradient launch; rev: walk direction of a fused one; sb: the strip launch, complete but for the region
struct StackLayerPlan { bool head = false, strips = false, fused = false; int nslots = 0, rev = 0; StripBwd sb; };
static StackLayerPlan plan_stack_layer(const Lin& q, LayerGemm& g, const DwGemm& d, const float* rs_in, int pos, const Bwd& b) {
  StackLayerPlan p; p.head = head_bwd_ok(q, g);
  p.strips = !p.head && strip_bwd_ok(q, g, d);
  if (p.strips) p.sb = take_strips(q, g, d, b);
  // layer launch + weight gradient in one launch where the shape allows (cnr_gemm_fdw.hip)
  p.fused = !p.head && be_fdw_enabled() && fdw_shape_ok(g) && rs_in && q.npad == 256 && q.ldw <= 320;
  p.nslots = p.fused ? b.fslots : b.nchunk; p.rev = walk_rev(pos);
  return p;
}
// pos: launches of the stack's backward chain before this one (0: the top layer, whose cotangent rows are packed (b.ldtop != kTop) only for
// the head kernel)
static int stack_layer_bwd(const Lin& q, LayerGemm& g, DwGemm& d, const float* rs_in, int pos, Bwd& b, const float* const* params, float* const* dP,
                           cnr_stream s) {
  StackLayerPlan p = plan_stack_layer(q, g, d, rs_in, pos, b);
  if (!p.head && pos == 0 && b.ldtop != kTop) return fail("render_backward: packed head cotangents without the streaming head kernel");   // (layout_bwd decides both from the same predicate)
  const DwRegion r = b.dw.take(q, region_slots(q, b));
  if (!r.part) return -1;
  const int kmain = p.strips ? 256 : 0;
  if (p.head) {
    HeadBwd h;
    h.dtop = g.A.a; h.ldt = g.A.lda; h.aux = g.E.aux; h.ldaux = g.E.ldaux; h.W = q.W; h.ldw = q.ldw; h.n = q.n; h.K = q.k_int; h.P = g.P;
    h.dout = g.E.o1; h.ldo = g.E.ld1; h.partial = r.part; h.colsum = r.csum; h.npad = q.npad; h.ldk = q.ldw; h.nslots = p.nslots;
    be_head_bwd(h, s);
  } else if (p.fused) {
    fused_into_region(q, g, d, rs_in, 0, r, 0, b, true, s, kmain, nullptr, p.rev);
  } else {
    if (q.n > 32) g.rs_out = b.rsD;
    be_layer_gemm(g, s);
    d.sx[0] = g.rs_out;
    dw_into_region(q, d, r, 0, p.nslots, g.P, true, s, kmain);
  }
  if (p.strips) { p.sb.partial = r.part; be_strip_bwd(p.sb, s); }
  b.dw.finish(q, r, p.nslots, p.nslots, params, dP);
  if (p.strips) b.dw.strip_columns_of_last_finish(b.nchunk);
  return 0;
}

// Backward of a narrow-input layer (K <= 48: relight layer 0, SDF layer 0): the cotangent of its input columns, its weight gradient and its
// bias gradient in one pass over the layer's output cotangent (cnr_narrow_bwd.hip), or a narrow layer launch + a weight-gradient launch.
// narrow_pass_ok decides, given the descriptor without a region: the shape test must see a backward form (partial set selects the switch
// be_narrow_bwd_ok honours), so a copy stands on the pool's base for it.
static bool narrow_pass_ok(NarrowBwd nb, const Lin& q, int hidden, const Bwd& b) {
  nb.partial = nb.colsum = b.dw.base;
  return be_fdw_enabled() && q.n == 256 && q.npad == 256 && hidden == 256 && be_narrow_bwd_ok(nb) && be_narrow_bwd_slots(nb.P) <= region_slots(q, b);
}
// one_pass: the region (taken here and its reduction queued here, unless the caller shares one it took and finishes it itself: SDF layer 0),
// the completed descriptor, the launch.  Otherwise the narrow layer launch where the descriptor asks for the input cotangent (dx) and, for a
// layer with a region of its own, the plain weight gradient; both read the operands the descriptor names.
static int narrow_layer_bwd(const Lin& q, NarrowBwd nb, bool one_pass, const DwRegion* taken, Bwd& b, const float* const* params, float* const* dP,
                            cnr_stream s) {
  if (!one_pass) {
    LayerGemm g = bwd_gemm(q, nb.P);
    g.A = direct_view(nb.X, nb.ldx); g.E.kind = EK_STORE; g.E.n_out = nb.ndx; g.E.o1 = nb.dx; g.E.ld1 = nb.lddx;
    if (nb.dx) be_layer_gemm(g, s);
    DwGemm d; d.npairs = 1; d.P = nb.P; d.X[0] = g.A; d.Y[0] = direct_view(nb.Y, nb.ldy);
    return taken ? 0 : plain_dw(b.dw, q, d, region_slots(q, b), b.nchunk, params, dP, s);
  }
  const DwRegion r = taken ? *taken : b.dw.take(q, region_slots(q, b));
  if (!r.part) return -1;
  nb.partial = r.part; nb.colsum = r.csum;
  be_narrow_bwd(nb, s);
  if (!taken) b.dw.finish(q, r, be_narrow_bwd_slots(nb.P), be_narrow_bwd_slots(nb.P), params, dP);
  return 0;
}

struct SdfBwdArgs {
  const float* daux_c = nullptr; const float* daux_r = nullptr;   // cotangents of the colour / relight aux rows [p g ..] (render) or null (query)
  bool grad_path = true;    // false: no cotangent on grad_x sdf -- no gbar / second-order sweep (Z2 starts from zero), value pairs only
  bool pts_grad = false;    // form ebar0 / ebars and the total point cotangent b.pbar (camera refinement, point queries)
};

// The launches of steps 5 and 6 of the backward pass and their weight-gradient pairs as descriptors (none of them needs a region).
struct SdfBwdDescs {
  const Model& m; long P; const Ctx& x; const Bwd& b; bool rays_grad; float inv_scale;
  View qbar_view(int l) const {
    View v;
    v.kind = VK_DIRECT;
    if (l == 0) { v.a = b.cbar; v.lda = kEmb; }
    else { v.a = b.VB[l - 1]; v.lda = m.Hs; if (m.skip(l)) v.scale = kInvSqrt2; }   // skip: tail columns of VB[l-1] hold cbar
    return v;
  }
  LayerGemm sweep_gemm(int l) const {
    const Lin& q = m.sdf[l];
    LayerGemm g = fwd_gemm(q, P);
    g.A = qbar_view(l);
    g.E.kind = EK_SWEEP; g.E.n_out = q.n; g.E.z = x.Z[l]; g.E.ldz = m.Hs;
    if (l == m.L - 1) { g.E.v = m.sdf[m.L].W + (long)m.F * m.sdf[m.L].ldw; g.E.ldv = 0; g.E.vscale = inv_scale; }
    else { g.E.v = x.V[l]; g.E.ldv = m.Hs; }
    g.E.o1 = b.Z2[l]; g.E.ld1 = m.Hs; g.E.o2 = b.VB[l]; g.E.ld2 = m.Hs;
    if (m.skip(l + 1)) { g.E.tail_src = b.cbar; g.E.ld_tail = kEmb; g.E.tail_n = m.emb; }
    return g;
  }
  LayerGemm vback_gemm(int l) const {
    const Lin& q = m.sdf[l];
    LayerGemm g = bwd_gemm(q, P);
    g.A = l == m.L ? direct_view(b.ZTOP, x.ldztop) : direct_view(b.Z2[l], m.Hs);
    g.E.kind = EK_VBACK; g.E.n_out = q.k_int; g.E.z = x.Z[l - 1]; g.E.ldz = m.Hs; g.E.o1 = b.Z2[l - 1]; g.E.ld1 = m.Hs;
    if (m.skip(l)) { g.E.scale = kInvSqrt2; g.E.split = m.sdf[l - 1].n; g.E.o2 = rays_grad ? b.ebars : nullptr; g.E.ld2 = kEmb; g.E.o2_off = skip_off(m);
                     g.E.o2_acc = l != top_skip(m);   // (the value backward runs from the top layer down: the highest skip layer stores, the others add)
                     g.E.vscale = kInvSqrt2; }   // (vscale: the scale of the layer's input view, for the fused launch's epilogue-side operand)
    return g;
  }
  // The first layer (narrow input): the cotangent of its input columns (camera refinement) and its value pair in one pass over Z2[0]
  // (cnr_narrow_bwd.hip) instead of a narrow layer launch + a weight-gradient launch; the descriptor without its region
  NarrowBwd narrow0() const {
    const Lin& q = m.sdf[0];
    NarrowBwd nb;
    nb.X = b.Z2[0]; nb.ldx = m.Hs; nb.Y = x.E; nb.ldy = kEmb; nb.ky = q.k_int; nb.P = P; nb.ldk = q.ldw;
    if (rays_grad) { narrow_bwd_weights(nb, q); nb.dx = b.ebar0; nb.lddx = kEmb; nb.ndx = m.emb; }
    return nb;
  }
  // value pair of layer l: X = zbar_l, Y = the layer's forward input
  void value_pair(int l, DwGemm& d) const {
    d.X[0] = l == m.L ? direct_view(b.ZTOP, x.ldztop) : direct_view(b.Z2[l], m.Hs);
    d.Y[0] = sdf_input_view(m, l, x.E, x.Z.data());
    d.sx[0] = b.rsX0[l]; d.sy[0] = x.rsY[l];
  }
  // gradient-chain pair of layer l into operand slot i of d: X = u_l = sp'(z_l) v_l, Y = qbar_l
  void grad_pair(int l, DwGemm& d, int i) const {
    if (l == m.L) {
      d.X[i].kind = VK_CONST_COL0; d.X[i].a = b.ZTOP; d.X[i].lda = x.ldztop; d.X[i].scale = inv_scale; d.X[i].math_split = m.F;
      d.Y[i].kind = VK_DIRECT; d.Y[i].a = b.VB[m.L - 1]; d.Y[i].lda = m.Hs;
    } else {
      d.X[i].a = x.Z[l]; d.X[i].lda = m.Hs;
      if (l == m.L - 1) { d.X[i].kind = VK_SIGMUL_ROW; d.X[i].b = m.sdf[m.L].W + (long)m.F * m.sdf[m.L].ldw; d.X[i].scale = inv_scale; }
      else { d.X[i].kind = VK_SIGMUL; d.X[i].b = x.V[l]; d.X[i].ldb = m.Hs; }
      d.Y[i] = qbar_view(l);
      d.sx[i] = x.rsX1[l]; d.sy[i] = b.rsY1[l];
    }
  }
};

// THE place where the SDF backward decides which launch forms which weight-gradient pair.  Each SDF layer's two pairs go into one region of
// the partial-sum pool, [value pair (zbar_l, input_l) | gradient-chain pair (u_l, qbar_l)]: the value pair in slots [0, value_slots) (it
// carries the bias column sums), the gradient-chain pair in [value_slots, value_slots + grad_slots).  A pair takes fslots slots when it is
// fused into its layer launch, the slots of a one-workgroup-per-CU launch from sweep0 / narrow_bwd, and nchunk slots as a separate GEMM (one
// workgroup per slot: fewer would leave CUs idle); when both are separate one GEMM over nchunk slots forms both.
// Who forms the value pair: SEPARATE = the weight-gradient GEMM of step 7; FUSED = value-backward launch l (cnr_gemm_fdw.hip); NARROW_PASS =
// layer 0 only, the one-pass launch that ends step 6 (cnr_narrow_bwd.hip).
enum class ValueBy : char { SEPARATE, FUSED, NARROW_PASS };
// Who forms the gradient-chain pair: NONE = there is no gradient path (sa.grad_path == false); SEPARATE = the weight-gradient GEMM of step 7;
// FUSED = sweep launch l (cnr_gemm_fdw.hip); SWEEP0 = narrow-input layer (layer 0), the sweep launch forms the pair from its epilogue's side
// inputs, one slot per workgroup (cnr_sweep0.hip); XROW = the fused top layer, whose pair has one live row, the extra row of sweep launch
// L - 1: no slots of its own.
enum class GradBy : char { NONE, SEPARATE, FUSED, SWEEP0, XROW };
struct SdfLayerPlan {
  ValueBy value = ValueBy::SEPARATE; GradBy grad = GradBy::NONE;
  int value_slots = 0, grad_slots = 0, value_rev = 0, grad_rev = 0;   // rev: walk directions of value-backward launch l / sweep launch l when fused
  bool both_in_one() const { return value == ValueBy::SEPARATE && grad == GradBy::SEPARATE; }
};
// The top layer (F features + the sdf row, F == 256 = its input width) without launches of its own (top_fused): its value-backward launch
// (gtop) takes the sdf column of the cotangent as a rank-one update of the 256-wide product (k_extra) and forms the main 256 x 256 weight
// gradient like any other layer; the sdf ROW of the weight gradient is made of values two launches hold anyway -- the gradient-chain pair's
// unit vector makes it inv_scale * column sums of VB[L-1], the o2 output of the sweep launch of layer L-1 (xrow1, xrow_mode 1), and the value
// pair adds sum zbar_sdf[pt] * softplus(z_{L-1})[pt][:], whose factors the value-backward launch has in its epilogue (xrow2, xrow_mode 2).
// layer: [L + 1]; xrow1 / xrow2: the extra-row requests, complete once the top layer's region is known (xrow, xbias)
struct SdfBwdPlan { std::vector<SdfLayerPlan> layer; bool top_fused = false; LayerGemm gtop; DwFuse xrow1, xrow2; };
static SdfBwdPlan plan_sdf_backward(const SdfBwdDescs& D, bool want_dw, const SdfBwdArgs& sa) {
  const Model& m = D.m; const Ctx& x = D.x; const Bwd& b = D.b;
  const bool fdw = be_fdw_enabled() && want_dw;   // (the fused layer + weight-gradient launches only where weight gradients are wanted)
  const bool gfdw = fdw && sa.grad_path;
  SdfBwdPlan pl; pl.layer.resize(m.L + 1);
  for (int l = 0; l <= m.L; ++l) {
    const Lin& q = m.sdf[l]; SdfLayerPlan& p = pl.layer[l];
    const bool sq = q.npad >= 224 && q.npad <= 256 && q.ldw == 256;
    if (fdw && sq && l >= 1 && l < m.L && x.rsY[l] && fdw_shape_ok(D.vback_gemm(l))) p.value = ValueBy::FUSED;
    if (sa.grad_path) p.grad = GradBy::SEPARATE;
    if (gfdw && sq && l < m.L && x.rsX1[l] && fdw_shape_ok(D.sweep_gemm(l))) p.grad = GradBy::FUSED;
    else if (gfdw && l < m.L && q.npad == 256 && be_sweep0_ok(D.sweep_gemm(l))) p.grad = GradBy::SWEEP0;
    p.value_rev = walk_rev(m.L - l, 1); p.grad_rev = walk_rev(l);
  }
  const GradBy g0 = pl.layer[0].grad;
  if (fdw && (g0 == GradBy::FUSED || g0 == GradBy::SWEEP0) && narrow_pass_ok(D.narrow0(), m.sdf[0], m.Hs, b)) pl.layer[0].value = ValueBy::NARROW_PASS;
  const Lin& qtop = m.sdf[m.L];
  pl.gtop = D.vback_gemm(m.L); pl.gtop.K = 256; pl.gtop.k_extra = 1;
  // (no_top_fuse: debugging aid, the top layer as three launches of its own)
  pl.top_fused = !debug_flags().no_top_fuse && fdw && be_fdw_xrow() && m.L >= 2 && pl.layer[m.L - 1].grad == GradBy::FUSED && m.F == 256 && qtop.n == 257 && qtop.k_int == 256 &&
                 qtop.ldw == 256 && qtop.npad <= 288 && x.ldztop >= 260 && x.rsY[m.L] && !m.skip(m.L) && fdw_shape_ok(pl.gtop);
  if (pl.top_fused) { pl.layer[m.L].value = ValueBy::FUSED; pl.layer[m.L].grad = GradBy::XROW; }
  pl.xrow1.xrow_mode = 1; pl.xrow1.xrow_stride = (long)qtop.npad * qtop.ldw; pl.xrow1.xrow_scale = D.inv_scale;
  pl.xrow2.xrow_mode = 2; pl.xrow2.xrow_stride = pl.xrow1.xrow_stride; pl.xrow2.xrow_scale = 1.0f; pl.xrow2.xbias_stride = qtop.npad;
  // The slot groups, and the one check that they fit the layer's region.  region_slots reserves room for every combination above, so the
  // fallback (the one-workgroup-per-CU forms give way to the separate GEMM, whose groups always fit) is not taken at any accepted width.
  for (int l = 0; l <= m.L; ++l)
    for (int pass = 0; pass < 2; ++pass) {
      SdfLayerPlan& p = pl.layer[l];
      p.value_slots = p.value == ValueBy::NARROW_PASS ? be_narrow_bwd_slots(D.P) : p.value == ValueBy::FUSED ? b.fslots : b.nchunk;
      p.grad_slots = p.grad == GradBy::SWEEP0 ? be_sweep0_slots(D.P) : p.grad == GradBy::FUSED ? b.fslots : (p.grad == GradBy::SEPARATE && p.value == ValueBy::FUSED) ? b.nchunk : 0;
      if (p.value_slots + p.grad_slots <= region_slots(m.sdf[l], b)) break;
      if (p.value == ValueBy::NARROW_PASS) p.value = ValueBy::SEPARATE;
      if (p.grad == GradBy::SWEEP0) p.grad = GradBy::SEPARATE;
    }
  return pl;
}

// Steps 4-7 of the backward pass and the point cotangent of step 8: the complete first- and second-order backward of the SDF network, shared
// by render_backward and cnr_sdf_query_backward.  Seeds: b.ZTOP (cotangent of the top layer's outputs [feat | sdf / scale | 0]) and b.gbar_a
// (cotangent of grad_x sdf).  Entered inside an open range (be_range_push), which it closes after the weight-gradient reductions.
// The plan is built first; every region of the partial-sum pool is taken before the first launch that writes into one (-1 when the pool
// refuses); the three loops then issue what the plan says.
static int sdf_backward(const Model& m, long P, const Ctx& x, Bwd& b, const float* const* params, float* const* dP /* null: no weight gradients */,
                         const SdfBwdArgs& sa, cnr_stream s) {
  const float scale = m.c.sdf_scale;
  const bool rays_grad = sa.pts_grad, skipnet = has_skip(m);
  const SdfBwdDescs D{m, P, x, b, rays_grad, 1.0f / scale};
  SdfBwdPlan pl = plan_sdf_backward(D, dP != nullptr, sa);
  // ---- 4. total d g and the tangent of the embedding
  GbarFinish gb;
  gb.P = P; gb.gbar_alpha = b.gbar_a; gb.daux_c = sa.daux_c; gb.daux_r = sa.daux_r; gb.E = x.E; gb.scale = scale;
  gb.multires = m.c.sdf_multires; gb.gbar_total = b.gbar_t; gb.cbar = b.cbar;
  if (sa.grad_path) be_gbar_finish(gb, s);
  std::vector<DwRegion> sreg(m.L + 1);
  for (int l = 0; l <= m.L; ++l)
    if (!(sreg[l] = b.dw.take(m.sdf[l], region_slots(m.sdf[l], b))).part) { be_range_pop(); return -1; }
  pl.xrow1.xrow = pl.xrow2.xrow = sreg[m.L].part + (size_t)256 * m.sdf[m.L].ldw; pl.xrow2.xbias = sreg[m.L].csum + 256;
  // ---- 5. second-order forward sweep (tangent of h_l in the direction induced by gbar)
  if (!sa.grad_path)   // value path only: the value backward adds into Z2, which no sweep has written
    for (int l = 0; l < m.L; ++l) be_memset_zero(b.Z2[l], (size_t)P * m.Hs * sizeof(float), s);
  for (int l = 0; sa.grad_path && l < m.L; ++l) {
    const Lin& q = m.sdf[l]; const SdfLayerPlan& p = pl.layer[l];
    LayerGemm g = D.sweep_gemm(l);
    DwGemm d; d.npairs = 1; d.P = P;
    switch (p.grad) {
      case GradBy::SWEEP0: be_sweep0_dw(g, sreg[l].part + (size_t)p.value_slots * q.npad * q.ldw, q.ldw, s); break;
      case GradBy::FUSED:
        D.grad_pair(l, d, 0);
        d.sy[0] = nullptr;   // (a fused launch does not need qbar_l's row scales; the unfused fallback then takes the split-bf16 tiles)
        fused_into_region(q, g, d, x.rsX1[l], 1, sreg[l], p.value_slots, b, false, s, 0, (pl.top_fused && l == m.L - 1) ? &pl.xrow1 : nullptr, p.grad_rev);
        break;
      default: g.rs_out = b.rsY1[l]; be_layer_gemm(g, s);
    }
  }
  be_range_pop(); be_range_push("sdf value backward");
  // ---- 6. value-path backward through the SDF net (in place: Z2[l] becomes the total cotangent of z_l)
  for (int l = m.L; l >= 1; --l) {
    const Lin& q = m.sdf[l];
    const bool top = l == m.L && pl.top_fused;
    LayerGemm g = top ? pl.gtop : D.vback_gemm(l);
    DwGemm d; d.npairs = 1; d.P = P;
    switch (pl.layer[l].value) {
      case ValueBy::FUSED:
        D.value_pair(l, d);
        d.sx[0] = nullptr;
        fused_into_region(q, g, d, x.rsY[l], 0, sreg[l], 0, b, true, s, 0, top ? &pl.xrow2 : nullptr, pl.layer[l].value_rev);
        break;
      default: g.rs_out = b.rsX0[l]; be_layer_gemm(g, s);
    }
  }
  // layer 0: one pass into the region it shares with the gradient-chain pair, or (camera refinement, point queries) the narrow layer launch
  narrow_layer_bwd(m.sdf[0], D.narrow0(), pl.layer[0].value == ValueBy::NARROW_PASS, &sreg[0], b, params, dP, s);
  be_range_pop(); be_range_push("weight gradients: leftovers + finish");
  // ---- 7. SDF weight gradients that were not formed inside a layer launch
  for (int l = 0; dP && l <= m.L; ++l) {
    const Lin& q = m.sdf[l]; const DwRegion& r = sreg[l]; const SdfLayerPlan& p = pl.layer[l];
    DwGemm d; d.npairs = 1; d.P = P;
    switch (p.value) {
      case ValueBy::SEPARATE:      // the value pair into the leading slots; with a separate gradient-chain pair both in one launch sharing the accumulators
        D.value_pair(l, d);
        if (p.both_in_one()) { d.npairs = 2; D.grad_pair(l, d, 1); }
        dw_into_region(q, d, r, 0, p.value_slots, P, true, s);
        break;
      case ValueBy::FUSED:         // the gradient-chain pair alone, behind the fused value pair
        if (p.grad != GradBy::SEPARATE) break;
        D.grad_pair(l, d, 0);
        dw_into_region(q, d, r, p.value_slots, p.grad_slots, P, false, s);
        break;
      case ValueBy::NARROW_PASS: break;   // (formed by the one-pass launch of step 6)
    }
    b.dw.finish(q, r, p.value_slots + p.grad_slots, p.value_slots, params, dP);
  }
  b.dw.flush(s);   // all partial-sum reductions + weight-norm backward in one launch
  be_range_pop();
  // ---- 8 (first part). total cotangent of the points
  if (rays_grad) {
    PbarFinish pf;
    pf.P = P; pf.daux_c = sa.daux_c; pf.daux_r = sa.daux_r; pf.ebar0 = b.ebar0; pf.ebars = skipnet ? b.ebars + skip_off(m) : nullptr;
    pf.E = x.E; pf.ce0 = x.CE0; pf.ces = skipnet ? x.CES + skip_off(m) : nullptr; pf.gbar_total = sa.grad_path ? b.gbar_t : nullptr; pf.scale = scale;
    pf.multires = m.c.sdf_multires; pf.pbar = b.pbar;
    be_pbar_finish(pf, s);
  }
  return 0;
}

static int render_backward(const cnr_config* cfg, const float* const* params, const cnr_render_inputs* in,
                           const cnr_render_outputs* out, const void* ctx, size_t ctx_bytes, const cnr_render_out_grads* go,
                           const cnr_render_in_grads* gi, void* scratch, size_t scratch_bytes, cnr_stream s) {
  Model m;
  if (build_model(cfg, m)) return -1;
  if (!params || !in || !out || !ctx || !go || !gi || !gi->d_params || !scratch) return fail("null argument");
  if (in->prune_eps > 0.0f) return fail("cnr_render_backward: the forward pass ran with prune_eps > 0 (inference-only early termination)");
  const long R = in->n_rays;
  const long P = R * m.M;
  Ctx x;
  Bwd b;
  if (layout_checked("context buffer", const_cast<void*>(ctx), ctx_bytes, [&](Arena& a) { layout_ctx(m, R, a, x); })) return -1;
  if (layout_checked("backward scratch", scratch, scratch_bytes, [&](Arena& a) { layout_bwd(m, R, x, a, b); })) return -1;
  const float scale = m.c.sdf_scale;
  const bool rays_out = gi->d_rays_o != nullptr || gi->d_rays_d != nullptr;
  if (rays_out && (!gi->d_rays_o || !gi->d_rays_d)) return fail("d_rays_o and d_rays_d must be given together");
  if ((gi->d_near != nullptr) != (gi->d_far != nullptr)) return fail("d_near and d_far must be given together");
  // z depends on near / far only without importance sampling and without an override (NeuS.py:311-313 vs :343)
  const bool nf_live = gi->d_near != nullptr && m.I == 0 && !in->z_vals_override;
  if (gi->d_near && !nf_live) {
    be_memset_zero(gi->d_near, (size_t)R * sizeof(float), s);
    be_memset_zero(gi->d_far, (size_t)R * sizeof(float), s);
  }
  const bool rays_grad = rays_out || nf_live;   // both need the total cotangent of the sample points
  float* const* dP = gi->d_params;

  RangeScope range_bwd("cnr_render_backward");
  be_range_push("compositor backward");
  // ---- 1. compositor backward
  // (pad columns of ZTOP = [feat cotangent | sdf cotangent | 0]: written by the compositor's backward together with the sdf column)
  CompositeBwd cb;
  cb.o = in->rays_o; cb.d = in->rays_d; cb.z = out->z_vals; cb.R = R; cb.M = m.M; cb.sample_dist = 2.0f / (float)m.S;
  cb.sdf = x.sdf; cb.g = out->gradients ? out->gradients : x.gbuf; cb.color = m.has_relight ? x.relit : x.gcol; cb.ldcolor = 4;
  cb.gcolor = m.has_relight ? x.gcol : nullptr; cb.ldg = 4;
  cb.variance = params[m.p_variance]; cb.cos_anneal = in->cos_anneal_ratio; cb.background_rgb = in->background_rgb;
  cb.eik_sums = x.eik_sums; cb.sdf_scale = scale; cb.inv_sigmoid = m.c.rel_inv_sigmoid; cb.has_relight = m.has_relight ? 1 : 0;
  cb.d_color_fine = go->color_fine; cb.d_s_val = go->s_val; cb.d_cdf = go->cdf_fine; cb.d_weight_sum = go->weight_sum;
  cb.d_weight_max = go->weight_max; cb.d_gradients = go->gradients; cb.d_weights = go->weights;
  cb.d_gradient_error = go->gradient_error; cb.d_depth = go->depth; cb.d_global_color = m.has_relight ? go->global_color : nullptr;
  cb.d_delta_relight = m.has_relight ? go->delta_relight : nullptr;
  cb.d_delta_relight_ray = m.has_relight ? go->delta_relight_per_ray : nullptr;
  cb.d_sdf_s = go->sdf_samples; cb.d_color_s = go->color_samples; cb.d_gcolor_s = m.has_relight ? go->global_color_samples : nullptr;
  cb.ztop = b.ZTOP; cb.ldztop = x.ldztop; cb.ztop_col = m.F; cb.gbar = b.gbar_a; cb.dtop = b.dtop; cb.gc_a = b.gc_a; cb.ldtop = b.ldtop; cb.dinvs_partial = b.dinvs;
  cb.d_rays_d = rays_grad ? b.drd_alpha : nullptr; cb.d_z = nf_live ? b.dzparts : nullptr;
  be_composite_bwd(cb, s);
  VarianceFinish vf;
  vf.partial = b.dinvs; vf.R = R; vf.variance = params[m.p_variance]; vf.d_variance = dP[m.p_variance];
  be_variance_finish(vf, s);

  be_range_pop(); be_range_push("relight chain backward");
  // ---- 2. relight chain backward
  if (m.has_relight) {
    const int y = m.c.rel_y_in_layer - 1;
    for (int i = m.NR - 1; i >= 0; --i) {
      const Lin& q = m.rel[1 + i];
      const float* dout = (i == m.NR - 1) ? b.dtop : b.D[i + 1];
      const int ldo = (i == m.NR - 1) ? b.ldtop : m.Hr;
      LayerGemm g = bwd_gemm(q, P);
      g.A = direct_view(dout, ldo);
      g.E.kind = EK_RELU_MASK; g.E.n_out = q.k_int; g.E.split = m.Hr; g.E.o1 = b.D[i]; g.E.ld1 = m.Hr;
      g.E.aux = x.HR[i]; g.E.ldaux = hr_ld(m, x, i); g.E.o2 = (i == y) ? b.gc_b : nullptr; g.E.ld2 = 4;
      DwGemm d; d.npairs = 1; d.P = P;
      d.X[0] = g.A; d.sy[0] = x.rsR[i];
      d.Y[0] = relight_input_view(m, i, x);
      if (stack_layer_bwd(q, g, d, x.rsR[i], m.NR - 1 - i, b, params, dP, s)) return -1;
    }
    {
      const Lin& q = m.rel[0];
      // one pass over D[0] for the cotangent of the layer's inputs, its weight gradient and its bias gradient, or a narrow layer launch + a
      // weight-gradient launch (narrow_layer_bwd)
      NarrowBwd nb;
      nb.X = b.D[0]; nb.ldx = m.Hr; nb.Y = x.AUX; nb.ldy = kAux; nb.ky = q.k_int; nb.P = P;
      narrow_bwd_weights(nb, q);
      nb.dx = b.dAUXr; nb.lddx = kAux; nb.ndx = q.k_int; nb.ldk = q.ldw;
      if (narrow_layer_bwd(q, nb, narrow_pass_ok(nb, q, m.Hr, b), nullptr, b, params, dP, s)) return -1;
    }
  }
  be_range_pop(); be_range_push("colour chain backward");
  // ---- 3. colour chain backward
  ColTopBwd ct;
  ct.P = P; ct.gc_a = b.gc_a; ct.gc_b = m.has_relight ? b.gc_b : nullptr; ct.gcolor = x.gcol; ct.squeeze = m.c.col_squeeze_out;
  ct.out = b.dctop; ct.ldtop = b.ldtop;
  be_coltop_bwd(ct, s);
  for (int l = m.NC - 1; l >= 0; --l) {
    const Lin& q = m.col[l];
    const float* dout = (l == m.NC - 1) ? b.dctop : b.DC[l];
    const int ldo = (l == m.NC - 1) ? b.ldtop : m.Hc;
    LayerGemm g = bwd_gemm(q, P);
    g.A = direct_view(dout, ldo);
    if (l > 0) {
      g.E.kind = EK_RELU_MASK; g.E.n_out = q.k_int; g.E.o1 = b.DC[l - 1]; g.E.ld1 = m.Hc; g.E.aux = x.HC[l - 1]; g.E.ldaux = m.Hc;
    } else {   // cotangent of [feat | aux]: feat part lands in ZTOP[., 0:F] (the sdf cotangent sits in column F), aux part in dAUXc
      g.E.kind = EK_SPLIT; g.E.n_out = q.k_int; g.E.split = m.F; g.E.o1 = b.ZTOP; g.E.ld1 = x.ldztop; g.E.o1_off = 0;
      g.E.o2 = b.dAUXc; g.E.ld2 = kAux;
      g.E.aux = x.featx; g.E.ldaux = x.ldfx;   // (the layer's forward input: the epilogue-side operand of the fused launch)
    }
    DwGemm d; d.npairs = 1; d.P = P;
    d.X[0] = g.A; d.sy[0] = x.rsC[l];
    d.Y[0] = color_input_view(m, l, x);
    if (stack_layer_bwd(q, g, d, x.rsC[l], m.NC - 1 - l, b, params, dP, s)) return -1;
  }
  be_range_pop(); be_range_push("sdf second-order sweep");
  SdfBwdArgs args;
  args.daux_c = b.dAUXc; args.daux_r = m.has_relight ? b.dAUXr : nullptr; args.grad_path = true; args.pts_grad = rays_grad;
  if (sdf_backward(m, P, x, b, params, dP, args, s)) return -1;
  // ---- 8. d rays (camera refinement configs)
  if (rays_grad) {
    RaysGradFinish rg;
    rg.R = R; rg.M = m.M; rg.d = in->rays_d; rg.z = out->z_vals; rg.sample_dist = 2.0f / (float)m.S; rg.pbar = b.pbar;
    rg.daux_dir_c = (m.c.col_mode != 1 && m.nv > 0) ? b.dAUXc : nullptr;
    rg.daux_dir_r = (m.has_relight && m.nv > 0) ? b.dAUXr : nullptr;
    rg.lddir = kAux; rg.multires_view = m.mv; rg.d_rays_d_alpha = b.drd_alpha; rg.d_o = gi->d_rays_o; rg.d_d = gi->d_rays_d;
    rg.dz_parts = nf_live ? b.dzparts : nullptr; rg.d_near = nf_live ? gi->d_near : nullptr; rg.d_far = nf_live ? gi->d_far : nullptr;
    be_rays_grad_finish(rg, s);
  }
  return check_backend("render_backward");
}

// ------------------------------------------------------------------------------------------------
// evaluation paths: dense SDF queries and vertex colours
// ------------------------------------------------------------------------------------------------
constexpr long kEvalChunk = 1 << 18;   // points per pass (activations ping-pong: 2 x chunk x H floats)

struct EvalBuf { float *E, *Za, *Zb; };
static void layout_eval(Model& m, long chunk, Arena& a, EvalBuf& e) {
  layout_weights(m, a);
  e.E = a.f((size_t)chunk * kEmb);
  e.Za = a.f((size_t)chunk * m.Hs);
  e.Zb = a.f((size_t)chunk * m.Hs);
  place_slack(a);
}

static int sdf_eval_impl(const cnr_config* cfg, const float* const* params, const float* pts, const float* bmin, const float* bmax,
                         int res, long n, float sign, float* out, void* scratch, size_t scratch_bytes, cnr_stream s, long lattice_start = 0) {
  Model m;
  if (build_model(cfg, m)) return -1;
  if (!params || !out || !scratch) return fail("null argument");
  const long chunk = n < kEvalChunk ? n : kEvalChunk;
  EvalBuf e;
  if (layout_checked("scratch", scratch, scratch_bytes, [&](Arena& a) { layout_eval(m, chunk, a, e); })) return -1;
  prep_all(m, params, s, true);   // (the SDF layers are all it runs: the other entries of params may be null)
  float* Zp[kMaxLayers];
  for (int l = 0; l < m.L; ++l) Zp[l] = (l & 1) ? e.Zb : e.Za;
  for (long start = 0; start < n; start += chunk) {
    const long cnt = (n - start) < chunk ? (n - start) : chunk;
    embed_points(m, pts ? pts + start * 3 : nullptr, cnt, e.E, nullptr, s, bmin, bmax, res, lattice_start + start);
    sdf_chain(m, cnt, e.E, Zp, out + start, nullptr, 0, sign / m.c.sdf_scale, s);
  }
  return check_backend("sdf_eval");
}

static size_t eval_scratch_bytes(const cnr_config* cfg, long n) {
  Model m;
  if (build_model(cfg, m)) return 0;
  EvalBuf e;
  return layout_size(nullptr, [&](Arena& a) { layout_eval(m, n < kEvalChunk ? n : kEvalChunk, a, e); });
}

// vertex colour (cnr_vertex_color): the point pipeline and the colour stack on chunks of n points, nothing saved
static void layout_vc(Model& m, long n, Arena& a, Ctx& x) {
  layout_weights(m, a);
  place_geometry(m, n, a, x);
  x.hry = nullptr; x.ldy = 0;
  place_grad_colors(n, a, x);   // (relit serves as the [n][3] gradient buffer)
  place_sdf_z(m, n, a, x);
  place_sdf_v(m, n, true, a, x);
  x.HC.resize(m.NC - 1);
  for (int l = 0; l + 1 < m.NC; ++l) x.HC[l] = a.f((size_t)n * m.Hc);
  x.rsY.assign(m.L + 1, nullptr); x.rsX1.assign(m.L, nullptr);
  place_slack(a);
}

// ------------------------------------------------------------------------------------------------
// SDF point queries (cnr_sdf_query_*): sdf_network.forward / .gradient (fields.py:81-115) at the caller's points and their backward -- the
// render path's SDF chains and its SDF backward (sdf_backward) on P = round_up(n, kQueryTile) rows.  Padded rows sit at the origin (finite
// activations), carry zero cotangents (an all-zero row gets a zero row scale, which the split-f16 weight-gradient products treat as a zero
// row) and are never copied out.  The forward stores the row scales the training forward stores, so the backward makes the same fused choices
// (plan_sdf_backward) as a render backward over the same number of points.
// ------------------------------------------------------------------------------------------------
constexpr long kQueryTile = 128;
static long query_rows(long n) { return (n + kQueryTile - 1) / kQueryTile * kQueryTile; }

struct QueryBuf { Ctx x; int* tag = nullptr; float* pts = nullptr; };
// the context: SDF weights, the tag (QueryIn), padded points, E, Z[l], the sdf / feature rows (x.featx, without an aux part) and the row
// scales rsY; with want_grad BEHIND them V[l], CE0 / CES, the gradient rows and rsX1 -- so that a value-only backward finds the value-path
// buffers at the same offsets whichever form the forward took
static void layout_query(Model& m, long P, bool want_grad, Arena& a, QueryBuf& q) {
  for (auto& l : m.sdf) place_lin(l, a);
  Ctx& x = q.x;
  q.tag = reinterpret_cast<int*>(a.f(64));
  q.pts = a.f((size_t)P * 3);
  x.E = a.f((size_t)P * kEmb);
  x.sdf = a.f(P);
  x.ldfx = round_up(m.F, 16);
  x.featx = a.f((size_t)P * x.ldfx);
  place_sdf_z(m, P, a, x);
  place_row_scales(x.rsY, m.L + 1, 1, m.L + 1, P, a);
  x.AUX = want_grad ? a.f((size_t)P * kAux) : nullptr;   // (be_grad_finish also writes g into AUX[., 3:6]; nothing reads it here)
  x.gbuf = want_grad ? a.f((size_t)P * 3) : nullptr;
  x.CE0 = want_grad ? a.f((size_t)P * kEmb) : nullptr;
  x.CES = want_grad ? a.f((size_t)P * kEmb) : nullptr;
  x.V.assign(m.L, nullptr);
  if (want_grad) place_sdf_v(m, P, true, a, x);
  place_row_scales(x.rsX1, m.L, 1, want_grad ? m.L : 1, P, a);
  place_slack(a);
}

static void layout_query_bwd(const Model& m, long P, bool grad_path, const Ctx& x, Arena& a, Bwd& b) {
  place_sdf_seeds(P, grad_path, x, a, b);
  place_sdf_cotangents(P, grad_path, a, b);
  place_sdf_sweeps(m, P, grad_path, a, b);
  place_dw_pool({&m.sdf}, P, a, b);
  place_sdf_bwd_row_scales(m, P, grad_path, a, b);
  b.rsD = nullptr;
  place_slack(a);
}

static size_t query_ctx_bytes(const cnr_config* cfg, long n, bool want_grad) {
  Model m;
  if (build_model(cfg, m) || n <= 0) return 0;
  QueryBuf q{};
  return layout_size(nullptr, [&](Arena& a) { layout_query(m, query_rows(n), want_grad, a, q); });
}

static size_t query_bwd_scratch_bytes(const cnr_config* cfg, long n, bool want_grad) {
  Model m;
  if (build_model(cfg, m) || n <= 0) return 0;
  QueryBuf q{};
  Bwd b{};
  layout_size(nullptr, [&](Arena& a) { layout_query(m, query_rows(n), want_grad, a, q); });
  return layout_size(nullptr, [&](Arena& a) { layout_query_bwd(m, query_rows(n), want_grad, q.x, a, b); });
}

static int sdf_query_forward(const cnr_config* cfg, const float* const* params, const float* pts, long n, bool want_grad, float* sdf, float* feat,
                             float* grad, void* ctx, size_t ctx_bytes, cnr_stream s) {
  Model m;
  if (build_model(cfg, m)) return -1;
  if (!params || !pts || !sdf || !ctx) return fail("null argument");
  if (n <= 0) return fail("n_points must be positive");
  if (want_grad != (grad != nullptr)) return fail("the grad buffer is given iff want_grad");
  const long P = query_rows(n);
  QueryBuf q{};
  if (layout_checked("context buffer", ctx, ctx_bytes, [&](Arena& a) { layout_query(m, P, want_grad, a, q); })) return -1;
  Ctx& x = q.x;
  RangeScope range_("sdf query forward");
  prep_all(m, params, s, true);
  QueryIn qi;
  qi.n = n; qi.P = P; qi.pts = pts; qi.out = q.pts; qi.tag = q.tag; qi.tag_value = kQueryCtxTag + (want_grad ? 1 : 0);
  be_query_in(qi, s);
  embed_points(m, q.pts, P, x.E, x.AUX, s);
  PointOpts po;
  po.grad = want_grad; po.grad_out = x.gbuf; po.aux_to_featx = false;   // (the feature rows have no aux part here)
  point_pipeline(m, P, x, po, s);
  QueryOut qo;
  qo.n = n; qo.F = m.F; qo.ldf = x.ldfx; qo.ldg = 3;
  qo.sdf_in = x.sdf; qo.feat_in = x.featx; qo.g_in = x.gbuf;
  qo.sdf = sdf; qo.feat = feat; qo.g = want_grad ? grad : nullptr;
  be_query_out(qo, s);
  return check_backend("sdf_query_forward");
}

static int sdf_query_backward(const cnr_config* cfg, const float* const* params, long n, bool want_grad, const float* d_sdf, const float* d_feat,
                              const float* d_grad, const void* ctx, size_t ctx_bytes, float* const* d_params, float* d_pts, void* scratch,
                              size_t scratch_bytes, cnr_stream s) {
  Model m;
  if (build_model(cfg, m)) return -1;
  if (!params || !ctx || !scratch) return fail("null argument");
  if (n <= 0) return fail("n_points must be positive");
  if (d_grad && !want_grad) return fail("d_grad needs a forward with want_grad");
  const long P = query_rows(n);
  QueryBuf q{};
  if (layout_checked("context buffer", const_cast<void*>(ctx), ctx_bytes, [&](Arena& a) { layout_query(m, P, want_grad, a, q); })) return -1;
  // no cotangent on the gradient: the second-order half of the backward is identically zero and is not run
  const bool grad_path = want_grad && d_grad != nullptr;
  Bwd b{};
  if (layout_checked("backward scratch", scratch, scratch_bytes, [&](Arena& a) { layout_query_bwd(m, P, grad_path, q.x, a, b); })) return -1;
  if (!d_params && !d_pts) return 0;
  RangeScope range_("sdf query backward");
  QuerySeed qs;
  qs.n = n; qs.P = P; qs.F = m.F; qs.ldztop = q.x.ldztop; qs.inv_scale = 1.0f / m.c.sdf_scale;
  qs.d_sdf = d_sdf; qs.d_feat = d_feat; qs.d_grad = d_grad; qs.ztop = b.ZTOP; qs.gbar = grad_path ? b.gbar_a : nullptr;
  qs.tag = q.tag; qs.want_grad = grad_path ? 1 : 0;   // (a value-only backward reads only the buffers every form of the forward wrote)
  be_query_seed(qs, s);
  be_range_push("sdf second-order sweep");
  SdfBwdArgs args;
  args.grad_path = grad_path; args.pts_grad = d_pts != nullptr;
  if (sdf_backward(m, P, q.x, b, params, d_params, args, s)) return -1;
  if (d_pts) {
    QueryOut qo;
    qo.n = n; qo.F = m.F; qo.ldf = 0; qo.ldg = 4;
    qo.sdf_in = nullptr; qo.feat_in = nullptr; qo.g_in = b.pbar;
    qo.sdf = nullptr; qo.feat = nullptr; qo.g = d_pts;
    be_query_out(qo, s);
  }
  return check_backend("sdf_query_backward");
}

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
static int background_forward(const cnr_nerf_config* cfg, const float* const* params, const float* rays_o, const float* rays_d, const float* z_feed,
                              long R, int MF, float sample_dist, float* alpha, float* color, void* ctx, size_t ctx_bytes, cnr_stream s) {
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
static int background_backward(const cnr_nerf_config* cfg, const float* const* params, const float* rays_o, const float* rays_d, const float* z_feed,
                               long R, int MF, float sample_dist, const void* ctx, size_t ctx_bytes, const float* color, const float* d_alpha,
                               const float* d_color, float* const* dP, float* d_rays_o, float* d_rays_d, float* d_z_feed, void* scratch,
                               size_t scratch_bytes, cnr_stream s) {
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

constexpr long kVcChunk = 1 << 16;

}  // namespace cnr

// =================================================================================================
// C ABI
// =================================================================================================
using namespace cnr;

extern "C" {

int cnr_abi_version(void) { return CNR_ABI_VERSION; }
const char* cnr_backend_name(void) { return be_name(); }
const char* cnr_last_error(void) { return g_err.c_str(); }

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

int cnr_render_backward(const cnr_config* cfg, const float* const* params, const cnr_render_inputs* in,
                        const cnr_render_outputs* out, const void* ctx, size_t ctx_bytes, const cnr_render_out_grads* gout,
                        const cnr_render_in_grads* gin, void* scratch, size_t scratch_bytes, void* stream) {
  return render_backward(cfg, params, in, out, ctx, ctx_bytes, gout, gin, scratch, scratch_bytes, (cnr_stream)stream);
}

void cnr_timing_enable(int on) { be_timing_enable(on); }

// [kLossBlocks][4] partial sums + 16 bytes whose first 4 are the completion counter of the one-launch forms
constexpr size_t kLossTicketOff = (size_t)kLossBlocks * 4 * sizeof(float);
size_t cnr_loss_scratch_bytes(int64_t n_rays) { (void)n_rays; return kLossTicketOff + 16; }

static int loss_args(const cnr_loss_config* cfg, const float* color, const float* wsum, const float* drel, const float* gt, const float* mask,
                     int64_t n_rays, int32_t n_samples, LossArgs& a) {
  if (!cfg || !color || !gt) return fail("null argument");
  if (n_rays <= 0 || n_samples <= 0) return fail("n_rays and n_samples must be positive");
  a.color = color; a.wsum = wsum; a.drel = drel; a.gt = gt; a.mask = mask; a.R = n_rays; a.M = n_samples;
  a.rgb_l1 = cfg->rgb_l1; a.include_mask = cfg->include_mask;
  return 0;
}

int cnr_loss_sums(const cnr_loss_config* cfg, const float* color_fine, const float* weight_sum, const float* delta_relight, const float* rgb_gt,
                  const float* mask, int64_t n_rays, int32_t n_samples, float* sums, void* scratch, size_t scratch_bytes, void* stream) {
  LossArgs a;
  if (loss_args(cfg, color_fine, weight_sum, delta_relight, rgb_gt, mask, n_rays, n_samples, a)) return -1;
  if (!sums || !scratch) return fail("null argument");
  if (mask && !weight_sum) return fail("weight_sum is required with a mask");
  if (scratch_bytes < cnr_loss_scratch_bytes(n_rays)) return fail("loss scratch too small");
  be_loss_sums(a, static_cast<float*>(scratch), sums, (cnr_stream)stream);
  return check_backend("loss_sums");
}

int cnr_loss_sums_ray(const cnr_loss_config* cfg, const float* color_fine, const float* weight_sum, const float* delta_relight_ray_sum,
                      const float* rgb_gt, const float* mask, int64_t n_rays, int32_t n_samples, float* sums, void* scratch, size_t scratch_bytes,
                      void* stream) {
  LossArgs a;
  if (loss_args(cfg, color_fine, weight_sum, delta_relight_ray_sum, rgb_gt, mask, n_rays, n_samples, a)) return -1;
  if (!sums || !scratch) return fail("null argument");
  if (mask && !weight_sum) return fail("weight_sum is required with a mask");
  if (scratch_bytes < cnr_loss_scratch_bytes(n_rays)) return fail("loss scratch too small");
  a.drel_per_ray = 1;
  be_loss_sums(a, static_cast<float*>(scratch), sums, (cnr_stream)stream);
  return check_backend("loss_sums_ray");
}

int cnr_loss_grads(const cnr_loss_config* cfg, const float* color_fine, const float* weight_sum, const float* rgb_gt, const float* mask,
                   int64_t n_rays, int32_t n_samples, const float* coef, float* d_color_fine, float* d_weight_sum, float* d_delta_relight,
                   void* stream) {
  LossArgs a;
  if (loss_args(cfg, color_fine, weight_sum, nullptr, rgb_gt, mask, n_rays, n_samples, a)) return -1;
  if (!coef || !d_color_fine) return fail("null argument");
  if (d_weight_sum && mask && !weight_sum) return fail("weight_sum is required with a mask");
  be_loss_grads(a, coef, d_color_fine, d_weight_sum, d_delta_relight, (cnr_stream)stream);
  return check_backend("loss_grads");
}

static int loss_scalars(const cnr_loss_config* cfg, float n_rays_global, int32_t n_samples, int32_t use_mask, int32_t use_relight, LossScalars& c) {
  if (!cfg) return fail("null argument");
  if (!(n_rays_global > 0.0f) || n_samples < 1) return fail("loss: n_rays_global and n_samples must be positive");
  const double Rg = (double)n_rays_global, M = (double)n_samples;
  c.lf = cfg->lambda_fine; c.le = cfg->lambda_eikonal; c.lm = cfg->lambda_mask; c.lr = cfg->lambda_relight;
  c.Rg = (float)Rg; c.den_rgb = (float)(Rg * 3.0); c.den_rel = (float)(Rg * M * 3.0);
  c.c_rgb = (float)((double)cfg->lambda_fine * (cfg->rgb_l1 ? 1.0 : 2.0) / (Rg * 3.0));
  c.c_bce = (float)((double)cfg->lambda_mask / Rg);
  c.c_rel = (float)((double)cfg->lambda_relight * 2.0 / (Rg * M * 3.0));
  c.use_mask = use_mask != 0; c.use_relight = use_relight != 0;
  return 0;
}

int cnr_loss_combine(const cnr_loss_config* cfg, const float* sums, const float* gradient_error, float n_rays_global, int32_t n_samples,
                     int32_t use_mask, int32_t use_relight, float* out, void* stream) {
  LossScalars c;
  if (loss_scalars(cfg, n_rays_global, n_samples, use_mask, use_relight, c)) return -1;
  if (!sums || !gradient_error || !out) return fail("null argument");
  be_loss_combine(c, sums, gradient_error, out, (cnr_stream)stream);
  return check_backend("loss_combine");
}

int cnr_loss_coef(const cnr_loss_config* cfg, const float* g_loss, const float* mean_rel, float n_rays_global, int32_t n_samples,
                  int32_t use_mask, int32_t use_relight, float* coef, void* stream) {
  LossScalars c;
  if (loss_scalars(cfg, n_rays_global, n_samples, use_mask, use_relight, c)) return -1;
  if (!g_loss || !coef || (use_relight && !mean_rel)) return fail("null argument");
  be_loss_coef(c, g_loss, mean_rel, coef, (cnr_stream)stream);
  return check_backend("loss_coef");
}

int cnr_loss_forward(const cnr_loss_config* cfg, const float* color_fine, const float* weight_sum, const float* delta_relight, int32_t delta_per_ray,
                     const float* rgb_gt, const float* mask, const float* gradient_error, int64_t n_rays, int32_t n_samples, float n_rays_global,
                     int32_t use_mask, int32_t use_relight, float* sums, float* out, void* scratch, size_t scratch_bytes, void* stream) {
  LossArgs a;
  LossScalars c;
  if (loss_args(cfg, color_fine, weight_sum, delta_relight, rgb_gt, mask, n_rays, n_samples, a)) return -1;
  if (loss_scalars(cfg, n_rays_global, n_samples, use_mask, use_relight, c)) return -1;
  if (!sums || !out || !scratch || !gradient_error) return fail("null argument");
  if (mask && !weight_sum) return fail("weight_sum is required with a mask");
  if (scratch_bytes < cnr_loss_scratch_bytes(n_rays)) return fail("loss scratch too small");
  a.drel_per_ray = delta_per_ray != 0;
  be_loss_forward(a, static_cast<float*>(scratch), reinterpret_cast<unsigned*>(static_cast<char*>(scratch) + kLossTicketOff), c, gradient_error, sums, out, (cnr_stream)stream);
  return check_backend("loss_forward");
}

int cnr_loss_shard_stats(const cnr_loss_config* cfg, const float* color_fine, const float* weight_sum, const float* delta_relight, int32_t delta_per_ray,
                         const float* rgb_gt, const float* mask, const float* eik_sums, int64_t n_rays, int32_t n_samples, float* stats, void* scratch,
                         size_t scratch_bytes, void* stream) {
  LossArgs a;
  if (loss_args(cfg, color_fine, weight_sum, delta_relight, rgb_gt, mask, n_rays, n_samples, a)) return -1;
  if (!stats || !scratch || !eik_sums) return fail("null argument");
  if (mask && !weight_sum) return fail("weight_sum is required with a mask");
  if (scratch_bytes < cnr_loss_scratch_bytes(n_rays)) return fail("loss scratch too small");
  a.drel_per_ray = delta_per_ray != 0;
  be_loss_shard_stats(a, static_cast<float*>(scratch), reinterpret_cast<unsigned*>(static_cast<char*>(scratch) + kLossTicketOff), eik_sums, stats, (cnr_stream)stream);
  return check_backend("loss_shard_stats");
}

int cnr_loss_shard_combine(const cnr_loss_config* cfg, const float* stats, float n_rays_global, int32_t n_samples, int32_t use_mask, int32_t use_relight,
                           float* out, void* stream) {
  LossScalars c;
  if (loss_scalars(cfg, n_rays_global, n_samples, use_mask, use_relight, c)) return -1;
  if (!stats || !out) return fail("null argument");
  be_loss_shard_combine(c, stats, out, (cnr_stream)stream);
  return check_backend("loss_shard_combine");
}

int cnr_loss_backward(const cnr_loss_config* cfg, const float* color_fine, const float* weight_sum, const float* rgb_gt, const float* mask,
                      int64_t n_rays, int32_t n_samples, const float* g_loss, const float* mean_rel, const float* eik_factor, float n_rays_global,
                      int32_t use_mask, int32_t use_relight, float* coef, float* d_color_fine, float* d_weight_sum, float* d_delta_relight_per_ray,
                      void* stream) {
  LossArgs a;
  LossScalars c;
  if (loss_args(cfg, color_fine, weight_sum, nullptr, rgb_gt, mask, n_rays, n_samples, a)) return -1;
  if (loss_scalars(cfg, n_rays_global, n_samples, use_mask, use_relight, c)) return -1;
  if (!g_loss || !coef || !d_color_fine || (use_relight && !mean_rel)) return fail("null argument");
  if (d_weight_sum && mask && !weight_sum) return fail("weight_sum is required with a mask");
  be_loss_backward(a, c, g_loss, mean_rel, eik_factor, coef, d_color_fine, d_weight_sum, d_delta_relight_per_ray, (cnr_stream)stream);
  return check_backend("loss_backward");
}

static int gen_rays_args(const int64_t* pix_idx, int64_t n, const float* c2w, int32_t n_cams, const float* focal, int32_t H, int32_t W,
                         int32_t normalize, int32_t opengl, const float* origin, float radius, GenRays& g) {
  if (!c2w || !focal) return fail("null argument");
  if (n <= 0 || n_cams <= 0 || H <= 0 || W <= 0) return fail("gen_rays: n, n_cams, H, W must be positive");
  if (origin && !(radius > 0.0f)) return fail("gen_rays: radius must be positive");
  static_assert(sizeof(long) == sizeof(int64_t), "int64 pixel indices");
  g.pix_idx = reinterpret_cast<const long*>(pix_idx); g.n = n; g.c2w = c2w; g.n_cams = n_cams; g.focal = focal; g.H = H; g.W = W;
  g.normalize = normalize; g.opengl = opengl; g.origin = origin; g.radius = radius;
  g.image = nullptr; g.mask = nullptr; g.rays_o = nullptr; g.rays_d = nullptr; g.rgb = nullptr; g.mask_sel = nullptr; g.near_ = nullptr; g.far_ = nullptr;
  return 0;
}

int cnr_gen_rays(const int64_t* pix_idx, int64_t n, const float* c2w, int32_t n_cams, const float* focal, int32_t H, int32_t W,
                 int32_t normalize, int32_t opengl, const float* image, const float* mask, const float* origin, float radius,
                 float* rays_o, float* rays_d, float* rgb, float* mask_sel, float* near_, float* far_, int32_t* bad_index_count, void* stream) {
  GenRays g;
  if (gen_rays_args(pix_idx, n, c2w, n_cams, focal, H, W, normalize, opengl, origin, radius, g)) return -1;
  if (!rays_o || !rays_d) return fail("null argument");
  if ((rgb && !image) || (mask_sel && !mask)) return fail("gen_rays: rgb / mask_sel need image / mask");
  if ((near_ != nullptr) != (far_ != nullptr)) return fail("gen_rays: near and far must be given together");
  g.image = image; g.mask = mask; g.rays_o = rays_o; g.rays_d = rays_d; g.rgb = rgb; g.mask_sel = mask_sel; g.near_ = near_; g.far_ = far_; g.bad_count = bad_index_count;
  be_gen_rays(g, (cnr_stream)stream);
  return check_backend("gen_rays");
}

int cnr_gen_rays_backward(const int64_t* pix_idx, int64_t n, const float* c2w, int32_t n_cams, const float* focal, int32_t H, int32_t W,
                          int32_t normalize, int32_t opengl, const float* origin, float radius, const float* d_rays_o, const float* d_rays_d,
                          const float* d_near, const float* d_far, float* d_c2w, float* d_focal, void* scratch, size_t scratch_bytes, void* stream) {
  GenRaysBwd q;
  if (gen_rays_args(pix_idx, n, c2w, n_cams, focal, H, W, normalize, opengl, origin, radius, q.f)) return -1;
  if (!d_c2w || !d_focal || !scratch) return fail("null argument");
  if (scratch_bytes < (size_t)n_cams * 2 * sizeof(float)) return fail("gen_rays_backward scratch too small");
  if ((d_near != nullptr) != (d_far != nullptr)) return fail("gen_rays_backward: d_near and d_far must be given together");
  q.d_rays_o = d_rays_o; q.d_rays_d = d_rays_d; q.d_near = d_near; q.d_far = d_far; q.d_c2w = d_c2w; q.d_focal = d_focal;
  q.d_focal_partial = static_cast<float*>(scratch);
  be_gen_rays_bwd(q, (cnr_stream)stream);
  return check_backend("gen_rays_backward");
}

// ---- on-device pixel choice
static long pixel_tiles(int64_t hw) { return (long)((hw + kPixTile - 1) / kPixTile); }
static int pixel_table_dims(const char* who, int32_t n_images, int64_t hw) {
  if (n_images <= 0 || hw <= 0) return fail("%s: n_images and pixels_per_image must be positive", who);
  if (hw >= (int64_t)1 << 31) return fail("%s: pixels_per_image must be below 2^31 (pixel indices are int32)", who);
  if ((double)n_images * (double)hw >= 4294967296.0) return fail("%s: n_images * pixels_per_image must be below 2^32", who);
  return 0;
}
size_t cnr_pixel_table_scratch_bytes(int32_t n_images, int64_t pixels_per_image) {
  if (n_images <= 0 || pixels_per_image <= 0) return 0;
  return round_up_sz((size_t)n_images * (size_t)pixel_tiles(pixels_per_image) * 2 * sizeof(int), 256);
}

int cnr_pixel_table_build(const float* masks, int32_t n_images, int64_t pixels_per_image, int32_t* order, int32_t* fg_count, int32_t* bg_count,
                          void* scratch, size_t scratch_bytes, void* stream) {
  if (pixel_table_dims("pixel_table_build", n_images, pixels_per_image)) return -1;
  if (!masks || !order || !fg_count || !bg_count || !scratch) return fail("pixel_table_build: null argument");
  if (scratch_bytes < cnr_pixel_table_scratch_bytes(n_images, pixels_per_image)) return fail("pixel_table_build scratch too small");
  PixelTable t;
  t.masks = masks; t.n_images = n_images; t.hw = (long)pixels_per_image; t.order = order; t.fg_count = fg_count; t.bg_count = bg_count;
  t.tile_counts = static_cast<int*>(scratch); t.tiles = pixel_tiles(pixels_per_image);
  if ((double)n_images * (double)t.tiles >= 2147483648.0) return fail("pixel_table_build: too many tiles (n_images * ceil(pixels_per_image / %d) must be below 2^31)", kPixTile);
  be_pixel_table(t, (cnr_stream)stream);
  return check_backend("pixel_table_build");
}

int cnr_choose_pixels(int64_t* state, int64_t n, int32_t want_fg, const int32_t* want_fg_dev, const int32_t* cam_ids, int32_t images_per_step,
                      int32_t n_images, int64_t pixels_per_image, const int32_t* order, const int32_t* fg_count, const int32_t* bg_count, int64_t span,
                      int64_t* idx, int32_t* cams_out, int32_t* counts_out, float* t_rand, void* stream) {
  if (n <= 0) return fail("choose_pixels: n must be positive");
  if (n >= (int64_t)1 << 31) return fail("choose_pixels: n must be below 2^31");
  if (pixel_table_dims("choose_pixels", n_images, pixels_per_image)) return -1;
  if (images_per_step <= 0) return fail("choose_pixels: images_per_step must be positive");
  if (images_per_step > kPixMaxSlots) return fail("choose_pixels: at most %d images per step (got %d)", kPixMaxSlots, (int)images_per_step);
  if (images_per_step > n_images) return fail("choose_pixels: images_per_step %d exceeds the table's %d images", (int)images_per_step, (int)n_images);
  if (!state || !idx) return fail("choose_pixels: null argument");
  const bool table = order && fg_count && bg_count;
  if (!table && (order || fg_count || bg_count)) return fail("choose_pixels: order, fg_count and bg_count must be given together");
  if (!table && (want_fg > 0 || want_fg_dev)) return fail("choose_pixels: foreground draws need the pixel table (order, fg_count, bg_count)");
  if (want_fg < 0 || want_fg > n) return fail("choose_pixels: want_fg must be in [0, n]");
  if (span < 0 || (double)span > (double)n_images * (double)pixels_per_image) return fail("choose_pixels: span must be in [0, n_images * pixels_per_image]");
  static_assert(sizeof(long) == sizeof(int64_t), "int64 state and indices");
  PixelDraw p;
  p.state = reinterpret_cast<long*>(state); p.n = (long)n; p.want_fg = want_fg; p.want_fg_dev = want_fg_dev; p.cam_ids = cam_ids; p.B = images_per_step;
  p.n_images = n_images; p.hw = (long)pixels_per_image; p.order = table ? order : nullptr; p.fg_count = fg_count; p.bg_count = bg_count;
  p.span = (unsigned long long)(span ? span : pixels_per_image);
  p.idx = reinterpret_cast<long*>(idx); p.cams_out = cams_out; p.counts_out = counts_out; p.t_rand = t_rand;
  be_choose_pixels(p, (cnr_stream)stream);
  return check_backend("choose_pixels");
}

static int camera_args(const cnr_camera_config* cfg, const float* r, const float* t, const float* init_c2w, const float* fx, const float* fy,
                       const int64_t* cam_ids, int64_t B, bool pose, bool focal, Camera& c) {
  if (!cfg) return fail("camera: null argument cfg");
  if (!pose && !focal) return fail("camera: null argument: neither the pose nor the focal part is given");
  c = Camera{};
  c.num_cams = cfg->num_cams; c.H = cfg->H; c.W = cfg->W; c.focal_order = cfg->focal_order; c.fx_only = cfg->fx_only != 0;
  if (pose) {
    if (cfg->num_cams <= 0) return fail("camera: num_cams must be positive");
    if (B <= 0) return fail("camera: B must be positive");
    if (cfg->pose_mode != CNR_POSE_3D && cfg->pose_mode != CNR_POSE_6D) return fail("camera: unknown pose_mode %d", (int)cfg->pose_mode);
    if (!r || !t) return fail("camera: null argument r / t");
    if ((cfg->has_init_c2w != 0) != (init_c2w != nullptr)) return fail("camera: init_c2w must be given exactly when cfg->has_init_c2w is set");
    if (!cam_ids && B != cfg->num_cams) return fail("camera: B must equal num_cams when cam_ids is null");
    static_assert(sizeof(long) == sizeof(int64_t), "int64 camera ids");
    c.r = r; c.t = t; c.init_c2w = init_c2w; c.cam_ids = reinterpret_cast<const long*>(cam_ids); c.B = B; c.six_d = cfg->pose_mode == CNR_POSE_6D;
  }
  if (focal) {
    if (cfg->focal_order != 1 && cfg->focal_order != 2) return fail("camera: unknown focal_order %d", (int)cfg->focal_order);
    if (cfg->H <= 0 || cfg->W <= 0) return fail("camera: H, W must be positive");
    if (!fx || (!cfg->fx_only && !fy)) return fail("camera: null argument fx / fy");
    c.fx = fx; c.fy = fy;
  }
  return 0;
}

int cnr_camera_forward(const cnr_camera_config* cfg, const float* r, const float* t, const float* init_c2w, const float* fx, const float* fy,
                       const int64_t* cam_ids, int64_t B, float* c2w, float* focal, void* stream) {
  Camera c;
  if (camera_args(cfg, r, t, init_c2w, fx, fy, cam_ids, B, c2w != nullptr, focal != nullptr, c)) return -1;
  c.c2w = c2w; c.focal = focal;
  be_camera_fwd(c, (cnr_stream)stream);
  return check_backend("camera_forward");
}

int cnr_camera_backward(const cnr_camera_config* cfg, const float* r, const float* t, const float* init_c2w, const float* fx, const float* fy,
                        const int64_t* cam_ids, int64_t B, const float* d_c2w, const float* d_focal, float* d_r, float* d_t, float* d_fx,
                        float* d_fy, void* stream) {
  CameraBwd q;
  if (camera_args(cfg, r, t, init_c2w, fx, fy, cam_ids, B, d_c2w != nullptr, d_focal != nullptr, q.f)) return -1;
  if (d_c2w && !d_r && !d_t) return fail("camera_backward: null argument: d_c2w without d_r or d_t");
  if (d_focal && !d_fx && !d_fy) return fail("camera_backward: null argument: d_focal without d_fx or d_fy");
  q.d_c2w = d_c2w; q.d_focal = d_focal; q.d_r = d_r; q.d_t = d_t; q.d_fx = d_fx; q.d_fy = q.f.fx_only ? nullptr : d_fy;
  be_camera_bwd(q, (cnr_stream)stream);
  return check_backend("camera_backward");
}

size_t cnr_clip_adam_scratch_bytes(int32_t n_tensors, const int64_t* sizes) {
  if (!sizes || n_tensors <= 0) return 0;
  size_t chunks = 0;
  for (int i = 0; i < n_tensors; ++i) chunks += (size_t)((sizes[i] > 0 ? sizes[i] : 0) + kAdamChunk - 1) / kAdamChunk;
  return (chunks + 1) * sizeof(float);
}

int cnr_clip_adam_step(const cnr_adam_config* cfg, int32_t n_tensors, const int64_t* sizes, float* const* params, const float* const* grads,
                       float* exp_avg, float* exp_avg_sq, void* scratch, size_t scratch_bytes, void* stream) {
  if (!cfg || !sizes || !params || !grads || !exp_avg || !exp_avg_sq || !scratch) return fail("null argument");
  if (n_tensors <= 0) return fail("n_tensors must be positive");
  if (cfg->step < 1 && !cfg->hyper_dev) return fail("step is 1-based");
  if (scratch_bytes < cnr_clip_adam_scratch_bytes(n_tensors, sizes)) return fail("clip_adam scratch too small");
  AdamArgs a;
  a.m = exp_avg; a.v = exp_avg_sq;
  a.lr = cfg->lr; a.beta1 = cfg->beta1; a.beta2 = cfg->beta2; a.eps = cfg->eps; a.max_norm = cfg->max_norm;
  a.hyper = cfg->hyper_dev;
  const int step = cfg->step < 1 ? 1 : cfg->step;
  a.bc1 = (float)(1.0 - pow((double)cfg->beta1, (double)step));
  a.bc2_sqrt = (float)sqrt(1.0 - pow((double)cfg->beta2, (double)step));
  long off = 0;
  float* part = static_cast<float*>(scratch);
  a.count = 0; a.nchunks = 0; a.partial = part;
  for (int i = 0; i < n_tensors; ++i) {
    if (sizes[i] < 0 || !params[i] || !grads[i]) return fail("tensor %d: null pointer or negative size", i);
    a.t[a.count++] = AdamTensor{params[i], grads[i], off, (long)sizes[i], a.nchunks};
    a.nchunks += (int)((sizes[i] + kAdamChunk - 1) / kAdamChunk);
    off += sizes[i];
    if (a.count == kAdamBatch || i + 1 == n_tensors) {
      be_clip_adam(a, (cnr_stream)stream);
      part += a.nchunks;
      a.count = 0; a.nchunks = 0; a.partial = part;
    }
  }
  return check_backend("clip_adam_step");
}

int cnr_timing_collect(cnr_kernel_timing* out, int max_records) {
  static_assert(sizeof(cnr_kernel_timing) == sizeof(KernelTiming), "timing record layout");
  return be_timing_collect(reinterpret_cast<KernelTiming*>(out), max_records);
}

static int sample_pdf_impl(const float* bins, const float* weights, const float* u_draws, int64_t n_rays, int32_t n, int32_t n_samples, float* out, void* stream) {
  if (!bins || !weights || !out) return fail("null argument");
  if (n_rays <= 0 || n < 2 || n > kMaxRaySamples || n_samples < 1 || n_samples > 64) return fail("sample_pdf: need 2 <= n <= %d bins and 1 <= n_samples <= 64", kMaxRaySamples);
  UpSample u;
  u.o = nullptr; u.d = nullptr; u.R = n_rays; u.z = bins; u.ldz = n; u.sdf = nullptr; u.lds = 0; u.n = n; u.m = n_samples; u.inv_s = 0.0f;
  u.new_z = out; u.w_in = weights; u.u_in = u_draws;
  be_upsample(u, (cnr_stream)stream);
  return check_backend("sample_pdf");
}
int cnr_sample_pdf(const float* bins, const float* weights, int64_t n_rays, int32_t n, int32_t n_samples, float* out, void* stream) {
  return sample_pdf_impl(bins, weights, nullptr, n_rays, n, n_samples, out, stream);
}
int cnr_sample_pdf_u(const float* bins, const float* weights, const float* u, int64_t n_rays, int32_t n, int32_t n_samples, float* out, void* stream) {
  if (!u) return fail("null argument");
  return sample_pdf_impl(bins, weights, u, n_rays, n, n_samples, out, stream);
}

int cnr_up_sample(const float* rays_o, const float* rays_d, const float* z_vals, const float* sdf, int64_t n_rays, int32_t n,
                  int32_t n_importance, float inv_s, float* out, void* stream) {
  if (!rays_o || !rays_d || !z_vals || !sdf || !out) return fail("null argument");
  if (n_rays <= 0 || n < 2 || n > kMaxRaySamples || n_importance < 1 || n_importance > 64) return fail("up_sample: need 2 <= n <= %d samples and 1 <= n_importance <= 64", kMaxRaySamples);
  UpSample u;
  u.o = rays_o; u.d = rays_d; u.R = n_rays; u.z = z_vals; u.ldz = n; u.sdf = sdf; u.lds = n; u.n = n; u.m = n_importance; u.inv_s = inv_s;
  u.new_z = out;
  be_upsample(u, (cnr_stream)stream);
  return check_backend("up_sample");
}

size_t cnr_sdf_eval_scratch_bytes(const cnr_config* cfg, int64_t n_points) { return eval_scratch_bytes(cfg, n_points); }

int cnr_sdf_eval(const cnr_config* cfg, const float* const* params, const float* pts, int64_t n_points, float sign, float* out,
                 void* scratch, size_t scratch_bytes, void* stream) {
  if (!pts) return fail("null points");
  return sdf_eval_impl(cfg, params, pts, nullptr, nullptr, 0, n_points, sign, out, scratch, scratch_bytes, (cnr_stream)stream);
}

size_t cnr_sdf_grid_scratch_bytes(const cnr_config* cfg, int32_t resolution) {
  return eval_scratch_bytes(cfg, (long)resolution * resolution * resolution);
}

int cnr_sdf_grid(const cnr_config* cfg, const float* const* params, const float* bound_min, const float* bound_max,
                 int32_t resolution, float* u, void* scratch, size_t scratch_bytes, void* stream) {
  if (!bound_min || !bound_max || resolution < 2) return fail("bad lattice");
  const long n = (long)resolution * resolution * resolution;
  return sdf_eval_impl(cfg, params, nullptr, bound_min, bound_max, resolution, n, -1.0f, u, scratch, scratch_bytes, (cnr_stream)stream);
}

size_t cnr_sdf_grid_slab_scratch_bytes(const cnr_config* cfg, int32_t resolution, int32_t x_begin, int32_t x_end) {
  if (x_begin < 0 || x_end > resolution || x_begin >= x_end) return 0;
  return eval_scratch_bytes(cfg, (long)(x_end - x_begin) * resolution * resolution);
}

int cnr_sdf_grid_slab(const cnr_config* cfg, const float* const* params, const float* bound_min, const float* bound_max, int32_t resolution,
                      int32_t x_begin, int32_t x_end, float* u_slab, void* scratch, size_t scratch_bytes, void* stream) {
  if (!bound_min || !bound_max || resolution < 2) return fail("bad lattice");
  if (x_begin < 0 || x_end > resolution || x_begin >= x_end) return fail("sdf_grid_slab: need 0 <= x_begin < x_end <= resolution");
  const long plane = (long)resolution * resolution;
  return sdf_eval_impl(cfg, params, nullptr, bound_min, bound_max, resolution, (long)(x_end - x_begin) * plane, -1.0f, u_slab, scratch, scratch_bytes,
                       (cnr_stream)stream, (long)x_begin * plane);
}

static int mc_layout(int32_t res, float thr, const float* u, void* scratch, size_t scratch_bytes, McVolume& v) {
  if (!u || !scratch) return fail("null argument");
  if (res < 2 || res > 1290) return fail("marching cubes: resolution must be in [2, 1290]");   // res^3 voxel ids and 2 * res^3 counts stay below 2^31
  if (scratch_bytes < cnr_mc_scratch_bytes(res)) return fail("marching cubes scratch too small");
  const size_t n = (size_t)res * res * res;
  const size_t nblocks = (n + kMcScanBlock - 1) / kMcScanBlock;
  char* p = static_cast<char*>(scratch);
  v.u = u; v.res = res; v.thr = thr;
  v.counts = reinterpret_cast<int*>(p); p += round_up_sz(n * 2 * sizeof(int), 256);
  v.block_sums = reinterpret_cast<int*>(p); p += round_up_sz(nblocks * 2 * sizeof(int), 256);
  v.flags = reinterpret_cast<unsigned char*>(p);
  v.totals = nullptr;
  return 0;
}

size_t cnr_mc_scratch_bytes(int32_t resolution) {
  if (resolution < 2) return 0;
  const size_t n = (size_t)resolution * resolution * resolution;
  const size_t nblocks = (n + kMcScanBlock - 1) / kMcScanBlock;
  return round_up_sz(n * 2 * sizeof(int), 256) + round_up_sz(nblocks * 2 * sizeof(int), 256) + round_up_sz(n, 256);
}

int cnr_mc_count(const float* u, int32_t resolution, float threshold, void* scratch, size_t scratch_bytes, int32_t* totals, void* stream) {
  McVolume v;
  if (mc_layout(resolution, threshold, u, scratch, scratch_bytes, v)) return -1;
  if (!totals) return fail("null argument");
  v.totals = totals;
  be_mc_count(v, (cnr_stream)stream);
  return check_backend("mc_count");
}

int cnr_mc_emit(const float* u, int32_t resolution, float threshold, const float* bound_min, const float* bound_max, void* scratch,
                size_t scratch_bytes, float* vertices, int32_t* triangles, void* stream) {
  McVolume v;
  if (mc_layout(resolution, threshold, u, scratch, scratch_bytes, v)) return -1;
  if (!bound_min || !bound_max || !vertices || !triangles) return fail("null argument");
  be_mc_emit(v, bound_min, bound_max, vertices, triangles, (cnr_stream)stream);
  return check_backend("mc_emit");
}

size_t cnr_nn_scratch_bytes(int64_t n_query, int64_t n_target) {
  (void)n_target;
  if (n_query <= 0) return 0;
  return round_up_sz((size_t)n_query * sizeof(unsigned long long), 256);   // one 64-bit candidate key per query
}

int cnr_nn_search(const float* query, int64_t n_query, const float* target, int64_t n_target, float* dist2, int32_t* idx, void* scratch,
                  size_t scratch_bytes, void* stream) {
  if (n_query < 0) return fail("nn_search: n_query < 0");
  if (n_query == 0) return 0;
  if (n_target <= 0) return fail("nn_search: no target points (n_target = %lld)", (long long)n_target);
  if (n_target >= (int64_t)1 << 31) return fail("nn_search: n_target must be below 2^31 (the index is an int32)");
  if (!query || !target || !dist2 || !idx || !scratch) return fail("null argument");
  if (scratch_bytes < cnr_nn_scratch_bytes(n_query, n_target)) return fail("nn_search scratch too small");
  NnSearch p;
  p.query = query; p.n = (long)n_query; p.target = target; p.m = (long)n_target; p.dist2 = dist2; p.idx = idx;
  p.keys = static_cast<unsigned long long*>(scratch);
  be_nn_search(p, (cnr_stream)stream);
  return check_backend("nn_search");
}

// one {sum d*d, sum ssim} pair of doubles per tile of the [B][C][H][W] form (the channels-last form of the same image never has more tiles),
// and 256 bytes for the two range keys of cnr_image_panel
static long image_blocks(int64_t planes, int H, int W, int cs) { return (long)planes * img_tiles_y(H) * img_tiles_x(W, cs); }
size_t cnr_image_scratch_bytes(int64_t n_images, int channels, int H, int W) {
  if (n_images <= 0 || channels < 1 || H < 1 || W < 1) return 0;
  return round_up_sz((size_t)image_blocks(n_images * channels, H, W, 1) * 2 * sizeof(double), 256) + 256;
}

int cnr_image_metrics(const float* img0, const float* img1, int64_t n_images, int channels, int H, int W, int channels_last, float* ssim_map,
                      double* sums, void* scratch, size_t scratch_bytes, void* stream) {
  if (n_images < 0) return fail("image_metrics: n_images < 0");
  if (!sums) return fail("image_metrics: null argument (sums)");
  ImageStats p;
  p.x = img0; p.y = img1; p.planes = 0; p.H = H; p.W = W; p.cs = 1; p.map = ssim_map; p.partials = nullptr; p.nblocks = 0; p.sums = sums;
  if (n_images > 0) {
    if (channels < 1) return fail("image_metrics: channels must be at least 1 (got %d)", channels);
    if (H < 2 || W < 2) return fail("image_metrics: H and W must be at least 2, the reflected border reads a neighbour (got %d x %d)", H, W);
    if ((double)n_images * channels * H * W >= 2147483648.0) return fail("image_metrics: the element count must be below 2^31");
    if (channels_last && channels > kImgMaxCs) return fail("image_metrics: the channels-last form takes at most %d channels (got %d)", kImgMaxCs, channels);
    if (!img0 || !img1 || !scratch) return fail("image_metrics: null argument");
    if (scratch_bytes < cnr_image_scratch_bytes(n_images, channels, H, W)) return fail("image_metrics scratch too small");
    p.cs = channels_last ? channels : 1;
    p.planes = channels_last ? (long)n_images : (long)n_images * channels;
    p.nblocks = image_blocks(p.planes, H, W, p.cs);
    p.partials = static_cast<double*>(scratch);
  }
  be_image_stats(p, (cnr_stream)stream);
  return check_backend("image_metrics");
}

int cnr_image_panel(const float* gt, const float* render, const float* depth, int H, int W, uint8_t* panel, float* range, void* scratch,
                    size_t scratch_bytes, void* stream) {
  if (H < 1 || W < 1) return fail("image_panel: H and W must be at least 1 (got %d x %d)", H, W);
  if ((double)H * W * 9.0 >= 2147483648.0) return fail("image_panel: the panel must have fewer than 2^31 bytes");
  if (!depth || !panel || !range || !scratch || (gt == nullptr) != (render == nullptr)) return fail("image_panel: null argument");
  if (scratch_bytes < 2 * sizeof(unsigned)) return fail("image_panel scratch too small");
  ImagePanel p;
  p.gt = gt; p.render = render; p.depth = depth; p.H = H; p.W = W; p.nsec = gt ? 3 : 1; p.panel = panel; p.range = range;
  p.keys = static_cast<unsigned*>(scratch);
  be_image_panel(p, (cnr_stream)stream);
  return check_backend("image_panel");
}


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
  return background_forward(cfg, params, rays_o, rays_d, z_feed, n_rays, n_feed, sample_dist, alpha, color, ctx, ctx_bytes, (cnr_stream)stream);
}
int cnr_background_backward(const cnr_nerf_config* cfg, const float* const* params, const float* rays_o, const float* rays_d, const float* z_feed,
                            int64_t n_rays, int32_t n_feed, float sample_dist, const void* ctx, size_t ctx_bytes, const float* color,
                            const float* d_alpha, const float* d_color, float* const* d_params, float* d_rays_o, float* d_rays_d, float* d_z_feed,
                            void* scratch, size_t scratch_bytes, void* stream) {
  return background_backward(cfg, params, rays_o, rays_d, z_feed, n_rays, n_feed, sample_dist, ctx, ctx_bytes, color, d_alpha, d_color, d_params,
                             d_rays_o, d_rays_d, d_z_feed, scratch, scratch_bytes, (cnr_stream)stream);
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

size_t cnr_vertex_color_scratch_bytes(const cnr_config* cfg, int64_t n_points) {
  Model m;
  if (build_model(cfg, m) || n_points <= 0) return 0;
  Ctx x;
  return layout_size(nullptr, [&](Arena& a) { layout_vc(m, n_points < kVcChunk ? n_points : kVcChunk, a, x); });
}

int cnr_vertex_color(const cnr_config* cfg, const float* const* params, const float* verts, int64_t n_points, float* rgb,
                     void* scratch, size_t scratch_bytes, void* stream) {
  Model m;
  if (build_model(cfg, m)) return -1;
  if (!params || !verts || !rgb || !scratch) return fail("null argument");
  cnr_stream s = (cnr_stream)stream;
  const long chunk = n_points < kVcChunk ? n_points : kVcChunk;
  Ctx x;
  if (layout_checked("scratch", scratch, scratch_bytes, [&](Arena& a) { layout_vc(m, chunk, a, x); })) return -1;
  prep_all(m, params, s);
  for (long start = 0; start < n_points; start += chunk) {
    const long cnt = (n_points - start) < chunk ? (n_points - start) : chunk;
    embed_points(m, verts + start * 3, cnt, x.E, x.AUX, s);
    PointOpts po;
    po.grad_out = x.relit; po.neg_g_as_view = (m.c.col_mode != 1) ? 1 : 0; po.multires_view = m.mv;
    point_pipeline(m, cnt, x, po, s);
    // colour chain with the final layer written straight into the caller's [n][3] buffer
    for (int l = 0; l < m.NC; ++l) {
      const Lin& q = m.col[l];
      LayerGemm g = fwd_gemm(q, cnt);
      g.A = color_input_view(m, l, x);
      g.E.bias = q.bias; g.E.n_out = q.n;
      if (l + 1 < m.NC) { g.E.kind = EK_RELU; g.E.o1 = x.HC[l]; g.E.ld1 = m.Hc; }
      else { g.E.kind = m.c.col_squeeze_out ? EK_SIGMOID : EK_LINEAR_SIG; g.E.o1 = rgb + start * 3; g.E.ld1 = 3; }
      be_layer_gemm(g, s);
    }
  }
  return check_backend("vertex_color");
}

size_t cnr_sdf_query_ctx_bytes(const cnr_config* cfg, int64_t n_points, int32_t want_grad) { return query_ctx_bytes(cfg, n_points, want_grad != 0); }
size_t cnr_sdf_query_bwd_scratch_bytes(const cnr_config* cfg, int64_t n_points, int32_t want_grad) {
  return query_bwd_scratch_bytes(cfg, n_points, want_grad != 0);
}
int cnr_sdf_query_forward(const cnr_config* cfg, const float* const* params, const float* pts, int64_t n_points, int32_t want_grad, float* sdf,
                          float* feat, float* grad, void* ctx, size_t ctx_bytes, void* stream) {
  return sdf_query_forward(cfg, params, pts, n_points, want_grad != 0, sdf, feat, grad, ctx, ctx_bytes, (cnr_stream)stream);
}
int cnr_sdf_query_backward(const cnr_config* cfg, const float* const* params, const float* pts, int64_t n_points, int32_t want_grad,
                           const float* d_sdf, const float* d_feat, const float* d_grad, const void* ctx, size_t ctx_bytes,
                           float* const* d_params, float* d_pts, void* scratch, size_t scratch_bytes, void* stream) {
  (void)pts;   // (the context holds the padded copy the forward embedded)
  return sdf_query_backward(cfg, params, n_points, want_grad != 0, d_sdf, d_feat, d_grad, ctx, ctx_bytes, d_params, d_pts, scratch, scratch_bytes,
                            (cnr_stream)stream);
}

}  // extern "C"
