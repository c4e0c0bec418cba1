// The backward pass of the render path (autograd of the forward incl. double backward through grad_x SDF):
//   compositor backward -> relight / colour chains backward -> second-order forward sweep through the SDF net ->
//   SDF value backward -> weight-gradient GEMMs (two operand pairs for the SDF net) -> weight-norm backward.
// cnr_render_backward, and sdf_backward -- the complete first- and second-order backward of the SDF network -- which the point queries
// (cnr_points.cpp) share.  Every launch decision is made in a plan before the first region of the weight-gradient pool is taken.
#include "cnr_plan.h"

namespace cnr {

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
int sdf_backward(const Model& m, long P, const Ctx& x, Bwd& b, const float* const* params, float* const* dP /* null: no weight gradients */,
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

}  // namespace cnr

using namespace cnr;

extern "C" {

int cnr_render_backward(const cnr_config* cfg, const float* const* params, const cnr_render_inputs* in,
                        const cnr_render_outputs* out, const void* ctx, size_t ctx_bytes, const cnr_render_out_grads* go,
                        const cnr_render_in_grads* gi, void* scratch, size_t scratch_bytes, void* stream) {
  cnr_stream s = (cnr_stream)stream;
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

}  // extern "C"
