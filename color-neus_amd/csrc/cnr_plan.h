// What the host units (cnr_plan.cpp, cnr_model.cpp, cnr_render_fwd.cpp, cnr_render_bwd.cpp, cnr_points.cpp, cnr_background.cpp, cnr_ops.cpp)
// share: the layer / model / arena / context / weight-gradient-pool types and the declarations of every function more than one unit calls.
// Private to csrc/: the library's interface is include/colorneus_render.h.  Every function declared here has one definition, in the unit
// named beside it; a function one unit alone uses is static there.
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/colorneus_render.h"
#include "cnr_backend.h"

namespace cnr {

// ---- errors (cnr_plan.cpp)
int fail(const char* fmt, ...);        // formats cnr_last_error's text (one thread_local string), returns -1
int check_backend(const char* what);   // the backend's pending launch error as `what: message`, or 0

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

// ---- layers and parameter registration (cnr_plan.cpp)
void identity_seg(Lin& l);
void add_linear_params(std::vector<ParamInfo>& params, Lin& l, const std::string& prefix, bool wn);
void add_weight_bias(std::vector<ParamInfo>& params, Lin& l, const std::string& name);
int param_info(const std::vector<ParamInfo>& params, int index, char* name, int name_len, int* rows, int* cols);

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
// A base must be kBaseAlign-aligned (include/colorneus_render.h): the Arena places every sub-buffer at a multiple of 256 bytes FROM the base,
// and the kernels access those sub-buffers with 16-byte vectors and 8-byte atomics.  (Entry points that do not lay out through
// layout_checked -- cnr_ops.cpp, cnr_composite_background_* -- do not check their base: the header says which.)
constexpr size_t kBaseAlign = 16;
template <class Layout> static int layout_checked(const char* what, void* buf, size_t bytes, Layout&& layout) {
  if ((uintptr_t)buf % kBaseAlign != 0)
    return fail("%s misaligned: its address must be a multiple of %zu bytes, got %p", what, kBaseAlign, buf);
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

void place_lin(Lin& q, Arena& a);
void place_row_scales(std::vector<float*>& rs, int n, int lo, int hi, long P, Arena& a);
void place_slack(Arena& a);

// ---- a Lin as the operand of a launch, and the weight preparation of a list of layers (cnr_plan.cpp)
LayerGemm fwd_gemm(const Lin& q, long P);
LayerGemm bwd_gemm(const Lin& q, long P);
void narrow_bwd_weights(NarrowBwd& nb, const Lin& q);
View direct_view(const float* a, int lda);
void prep_layers(const std::vector<Lin*>& layers, const float* const* params, cnr_stream s);

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

// ---- the separate weight-gradient GEMM (cnr_plan.cpp)
int dw_chunks(long P);
void dw_into_region(const Lin& q, DwGemm& g, const DwRegion& r, int slot0, int nchunk, long P, bool with_bias, cnr_stream s, int kmain = 0);
int plain_dw(DwPool& pool, const Lin& q, DwGemm& g, int cap, int nchunk, const float* const* params, float* const* dparams, cnr_stream s);

// ---- the render model and its layouts (cnr_model.cpp)
int build_model(const cnr_config* cfg, Model& m);
int hr_ld(const Model& m, const Ctx& x, int i);
int skip_off(const Model& m);
int top_skip(const Model& m);
bool has_skip(const Model& m);
bool relu_fused_shapes(const Model& m);
bool head_bwd_static_ok(const Lin& q, int ldaux);
int region_slots(const Lin& q, const Bwd& b);
void layout_weights(Model& m, Arena& a);
void place_geometry(const Model& m, long P, Arena& a, Ctx& x);
void place_grad_colors(long P, Arena& a, Ctx& x);
void place_sdf_z(const Model& m, long P, Arena& a, Ctx& x);
void place_sdf_v(const Model& m, long P, bool saved, Arena& a, Ctx& x);
void layout_ctx_infer(Model& m, long R, Arena& a, Ctx& x);
void layout_ctx(Model& m, long R, Arena& a, Ctx& x);
void place_sdf_seeds(long P, bool grad_path, const Ctx& x, Arena& a, Bwd& b);
void place_sdf_cotangents(long P, bool grad_path, Arena& a, Bwd& b);
void place_sdf_sweeps(const Model& m, long P, bool grad_path, Arena& a, Bwd& b);
void place_dw_pool(std::initializer_list<const std::vector<Lin>*> stacks, long P, Arena& a, Bwd& b);
void place_sdf_bwd_row_scales(const Model& m, long P, bool grad_path, Arena& a, Bwd& b);
void layout_bwd(const Model& m, long R, const Ctx& x, Arena& a, Bwd& b);

// ---- the forward chains (cnr_render_fwd.cpp)
// what point_pipeline runs and where its results go
struct PointOpts {
  bool grad = true;             // false: the value chain alone
  float* grad_out = nullptr;    // [P][3]
  bool aux_to_featx = true;     // the aux row is copied behind the features (the colour net's input rows)
  int neg_g_as_view = 0;        // vertex colouring: view_dirs = -g
  int multires_view = 0;
};
void prep_all(Model& m, const float* const* params, cnr_stream s, bool sdf_only = false);
View sdf_input_view(const Model& m, int l, const float* E, const float* const* Z);
void sdf_chain(const Model& m, long n, const float* E, float* const* Z, float* sdf_out, float* feat_out, int ld_feat,
               float top_scale, cnr_stream s, float* const* rs = nullptr /* [L+1] row scales of the layer inputs, see Ctx::rsY */);
void embed_points(const Model& m, const float* pts, long n, float* E, float* AUX, cnr_stream s, const float* bmin = nullptr,
                  const float* bmax = nullptr, int res = 0, long start = 0);
void point_pipeline(const Model& m, long P, const Ctx& x, const PointOpts& o, cnr_stream s);
View color_input_view(const Model& m, int l, const Ctx& x);
View relight_input_view(const Model& m, int i /* rl_mlp index, -1 = in_layer */, const Ctx& x);

// ---- the SDF network's backward (cnr_render_bwd.cpp)
struct SdfBwdArgs {
  const float* daux_c = nullptr; const float* daux_r = nullptr;   // cotangents of the colour / relight aux rows [p g ..] (render) or null (query)
  bool grad_path = true;    // false: no cotangent on grad_x sdf -- no gbar / second-order sweep (Z2 starts from zero), value pairs only
  bool pts_grad = false;    // form ebar0 / ebars and the total point cotangent b.pbar (camera refinement, point queries)
};
int sdf_backward(const Model& m, long P, const Ctx& x, Bwd& b, const float* const* params, float* const* dP /* null: no weight gradients */,
                 const SdfBwdArgs& sa, cnr_stream s);

}  // namespace cnr
