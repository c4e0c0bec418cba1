// Core of the host orchestration: what every host unit uses and nothing of the render path's own.  The host side of the library is seven
// translation units over one private header (cnr_plan.h):
//   cnr_plan.cpp        this file: the environment (debug_flags), the error string, layers as launch operands, weight preparation, the separate
//                       weight-gradient GEMM, and the ABI's version / backend / error / timing entry points
//   cnr_model.cpp       build_model and every render-path layout, the parameter and *_bytes queries
//   cnr_render_fwd.cpp  the forward pass: sampler, SDF chains, colour / relight chains, compositor
//   cnr_render_bwd.cpp  the backward pass and the SDF network's backward that the point queries share
//   cnr_points.cpp      dense SDF evaluation, vertex colours, differentiable point queries
//   cnr_background.cpp  the plain linear op and the NeRF++ background
//   cnr_ops.cpp         the stand-alone ops: loss, rays, pixel choice, cameras, clip + Adam, sample_pdf, marching cubes, neighbours, image metrics
//
// No unit contains arithmetic on tensor data: they only size buffers, build kernel descriptors and enqueue kernels through cnr_backend.h.
// All are shared verbatim by the HIP build and the CPU-emulation build (tests only).
#include "cnr_plan.h"

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
int fail(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return -1;
}

void identity_seg(Lin& l) {
  l.k_int = l.k_ref;
  l.nseg = 1;
  l.seg[0] = {0, 0, l.k_ref};
}

// Parameter registration.  The order is part of the ABI (checkpoints, cnr_param_info): bias, then weight_g / weight_v (or weight) for the
// SDF and colour stacks (add_linear_params); weight, then bias for the plain layers of the relight and background networks (add_weight_bias).
void add_linear_params(std::vector<ParamInfo>& params, Lin& l, const std::string& prefix, bool wn) {
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
void add_weight_bias(std::vector<ParamInfo>& params, Lin& l, const std::string& name) {
  l.name = name; l.wn = false;
  l.p_v = (int)params.size(); params.push_back({name + ".weight", l.n, l.k_ref});
  l.p_b = (int)params.size(); params.push_back({name + ".bias", l.n, 1});
}
int param_info(const std::vector<ParamInfo>& params, int index, char* name, int name_len, int* rows, int* cols) {
  if (index < 0 || index >= (int)params.size()) return fail("parameter index out of range");
  if (name && name_len > 0) snprintf(name, name_len, "%s", params[index].name.c_str());
  if (rows) *rows = params[index].rows;
  if (cols) *cols = params[index].cols;
  return 0;
}

void place_lin(Lin& q, Arena& a) {
  q.W = a.f((size_t)q.wpad * q.ldw);
  q.Wt = a.f((size_t)q.kpad * q.ldwt);
  q.bias = a.f(q.wpad);
  q.Wp = reinterpret_cast<unsigned short*>(a.f((size_t)q.wpad * q.ldw));
  q.Wtp = reinterpret_cast<unsigned short*>(a.f((size_t)q.kpad * q.ldwt));
  q.Wps = a.f(q.wpad > 256 ? q.wpad : 256);   // (the fused kernels read 256 column scales; entries >= npad are never used)
  q.Wtps = a.f(q.kpad > 256 ? q.kpad : 256);  // (likewise)
  q.Wf = (q.ldw <= 304) ? reinterpret_cast<unsigned short*>(a.f((size_t)8 * (q.ldw / 16) * 2 * 64 * 8 / 2)) : nullptr;   // (<= 19 k16 blocks: 256 + 48)
}

// per-point row scales rs[lo .. hi) of a stack of n launches (null elsewhere)
void place_row_scales(std::vector<float*>& rs, int n, int lo, int hi, long P, Arena& a) {
  rs.assign(n, nullptr);
  for (int l = lo; l < hi; ++l) rs[l] = a.f(P);
}
void place_slack(Arena& a) { a.f(1024); }   // GEMM tiles may read (never use) a few columns past the last row of a buffer

// The weight operand of a layer launch over P rows: y = x W^T (fwd_gemm: W, its planes and row scales) or dx = dy W (bwd_gemm: the
// transposed copies).  THE place where a Lin becomes LayerGemm fields; a call site sets only its input view, its epilogue and what differs.
LayerGemm fwd_gemm(const Lin& q, long P) {
  LayerGemm g;
  g.W = q.W; g.ldw = q.ldw; g.Wp = q.Wp; g.wp_stride = (long)q.wpad * q.ldw; g.w_rows = q.wpad; g.wscale = q.Wps; g.N = q.n; g.K = q.k_int; g.P = P;
  return g;
}
LayerGemm bwd_gemm(const Lin& q, long P) {   // (w_rows stays at its default: the launches take round_up(N, 32) rows of W^T)
  LayerGemm g;
  g.W = q.Wt; g.ldw = q.ldwt; g.Wp = q.Wtp; g.wp_stride = (long)q.kpad * q.ldwt; g.wscale = q.Wtps; g.N = q.k_int; g.K = q.n; g.P = P;
  return g;
}
// ... and of the one-pass narrow backward (cnr_narrow_bwd.hip), which stages all kpad rows of the W^T planes
void narrow_bwd_weights(NarrowBwd& nb, const Lin& q) {
  const LayerGemm t = bwd_gemm(q, 0);
  nb.Wp = t.Wp; nb.wp_stride = t.wp_stride; nb.ldw = t.ldw; nb.w_rows = q.kpad; nb.wscale = t.wscale;
}
View direct_view(const float* a, int lda) {
  View v;
  v.a = a; v.lda = lda;
  return v;
}

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
void prep_layers(const std::vector<Lin*>& layers, const float* const* params, cnr_stream s) {
  std::vector<PrepWeight> pw;
  std::vector<SplitJob> sj;
  for (const Lin* q : layers) { pw.push_back(prep_desc(*q, params)); add_split_jobs(*q, sj); }
  be_prep_weights(pw.data(), (int)pw.size(), s);
  be_split_planes_many(sj.data(), (int)sj.size(), s);
}

int check_backend(const char* what) {
  char msg[256];
  if (be_check_last_error(msg, sizeof msg) != 0) return fail("%s: %s", what, msg);
  return 0;
}

// point chunks (slots) of a separate weight-gradient GEMM: one workgroup per CU as soon as every chunk has a few 16-point slabs
int dw_chunks(long P) {
  const long nch = P / 128;
  return nch < 1 ? 1 : nch > 256 ? 256 : (int)nch;
}

// separate weight-gradient GEMM into slots [slot0, slot0 + nchunk) of a region (bias column sums only for a group at slot 0)
void dw_into_region(const Lin& q, DwGemm& g, const DwRegion& r, int slot0, int nchunk, long P, bool with_bias, cnr_stream s, int kmain) {
  with_bias = with_bias && slot0 == 0;
  g.N = q.n; g.K = kmain > 0 ? kmain : q.k_int;   // (kmain: the columns beyond it are formed by be_strip_bwd)
  g.nchunk = nchunk; g.chunk_pts = round_up((int)((P + nchunk - 1) / nchunk), 16);
  g.partial = r.part + (size_t)slot0 * q.npad * q.ldw; g.Npad = q.npad; g.ldk = q.ldw; g.colsum = with_bias ? r.csum : nullptr;
  be_dw_gemm(g, s);   // (which of its 256 x 256 tiles run split-f16: dw_main_tile, from the row scales g carries)
}

// THE plain weight gradient of a layer: a region of cap slots, one GEMM of g's operand pairs over its first nchunk slots, the reduction queued
int plain_dw(DwPool& pool, const Lin& q, DwGemm& g, int cap, int nchunk, const float* const* params, float* const* dparams, cnr_stream s) {
  const DwRegion r = pool.take(q, cap);
  if (!r.part) return -1;
  dw_into_region(q, g, r, 0, nchunk, g.P, true, s);
  pool.finish(q, r, nchunk, nchunk, params, dparams);
  return 0;
}

}  // namespace cnr

using namespace cnr;

extern "C" {

int cnr_abi_version(void) { return CNR_ABI_VERSION; }
const char* cnr_backend_name(void) { return be_name(); }
const char* cnr_last_error(void) { return g_err.c_str(); }

void cnr_timing_enable(int on) { be_timing_enable(on); }

int cnr_timing_collect(cnr_kernel_timing* out, int max_records) {
  static_assert(sizeof(cnr_kernel_timing) == sizeof(KernelTiming), "timing record layout");
  return be_timing_collect(reinterpret_cast<KernelTiming*>(out), max_records);
}

}  // extern "C"
