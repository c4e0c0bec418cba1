// Entry points on explicit points: dense SDF evaluation (points, lattice, lattice slab), vertex colours, and the differentiable point
// queries.  All run the render path's chains (cnr_render_fwd.cpp) and its SDF backward (cnr_render_bwd.cpp) on layouts of their own.
#include "cnr_plan.h"

namespace cnr {

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
constexpr long kVcChunk = 1 << 16;
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

}  // namespace cnr

using namespace cnr;

extern "C" {

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

size_t cnr_sdf_query_ctx_bytes(const cnr_config* cfg, int64_t n, int32_t want_grad) {
  Model m;
  if (build_model(cfg, m) || n <= 0) return 0;
  QueryBuf q{};
  return layout_size(nullptr, [&](Arena& a) { layout_query(m, query_rows(n), want_grad != 0, a, q); });
}

size_t cnr_sdf_query_bwd_scratch_bytes(const cnr_config* cfg, int64_t n, int32_t want_grad) {
  Model m;
  if (build_model(cfg, m) || n <= 0) return 0;
  QueryBuf q{};
  Bwd b{};
  layout_size(nullptr, [&](Arena& a) { layout_query(m, query_rows(n), want_grad != 0, a, q); });
  return layout_size(nullptr, [&](Arena& a) { layout_query_bwd(m, query_rows(n), want_grad != 0, q.x, a, b); });
}

int cnr_sdf_query_forward(const cnr_config* cfg, const float* const* params, const float* pts, int64_t n_points, int32_t want_grad_flag, float* sdf,
                          float* feat, float* grad, void* ctx, size_t ctx_bytes, void* stream) {
  cnr_stream s = (cnr_stream)stream;
  const long n = n_points;
  const bool want_grad = want_grad_flag != 0;
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

int cnr_sdf_query_backward(const cnr_config* cfg, const float* const* params, const float* pts, int64_t n_points, int32_t want_grad_flag,
                           const float* d_sdf, const float* d_feat, const float* d_grad, const void* ctx, size_t ctx_bytes,
                           float* const* d_params, float* d_pts, void* scratch, size_t scratch_bytes, void* stream) {
  (void)pts;   // (the context holds the padded copy the forward embedded)
  cnr_stream s = (cnr_stream)stream;
  const long n = n_points;
  const bool want_grad = want_grad_flag != 0;
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

}  // extern "C"
