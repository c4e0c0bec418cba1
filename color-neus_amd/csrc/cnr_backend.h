// Kernel launch interface of the render path between the host orchestration (the host units listed in cnr_plan.cpp, sharing cnr_plan.h) and the
// kernels: weight preparation, the layer / chain / narrow / head / strip launches, sampler, compositor and prune, the *_finish kernels and the
// point-query rows, the memset / column helpers, timing, ranges and the error check.  Every stand-alone family (loss, optimiser, rays, pixels,
// cameras, marching cubes, nearest neighbour, image metrics, background, mesh raster, mesh components, mesh surface, mesh culling, registration)
// has a header of its own: cnr_<family>.h.
// Implemented twice: the .hip translation units (HIP, gfx950 -- the product) and cnr_kernels_emu.cpp (CPU emulation, tests only).
#pragma once
#include "cnr_common.h"
#include "cnr_views.h"

namespace cnr {

constexpr int kMaxRaySamples = 256;   // per-ray kernels stage one ray in LDS: M <= 256

struct Segment { int dst, src, len; };   // internal column [dst, dst+len) <- reference column [src, src+len)
// the column permutation a layer's segments describe: the reference column behind internal column j / the internal column of reference column c
// (-1: none -- zero padding / a column the layer does not read).  A layer's segments are disjoint in dst and in src (build_model in cnr_model.cpp, the
// only place that writes them, deals consecutive pieces of the reference columns to consecutive internal ones), so at most one segment matches
// and the order of the search does not matter.
CNR_HD int seg_src_of(const Segment* seg, int nseg, int j) {
  int src = -1;
  for (int q = 0; q < nseg; ++q)
    if (j >= seg[q].dst && j < seg[q].dst + seg[q].len) src = seg[q].src + (j - seg[q].dst);
  return src;
}
CNR_HD int seg_dst_of(const Segment* seg, int nseg, int c) {
  int dst = -1;
  for (int q = 0; q < nseg; ++q)
    if (c >= seg[q].src && c < seg[q].src + seg[q].len) dst = seg[q].dst + (c - seg[q].src);
  return dst;
}
// weight-norm (w = g * v / |v| per row): the row's scale from its sum of squares, and the backward of one entry from the row's dot = <dw, v> and nrm = |v|
// (d g of the row is dot / nrm).  The sums are the caller's, in double: the row norm is the most rounding-sensitive step (x inv_s downstream)
CNR_HD float weight_norm_scale(float g, double ss) { return g / (float)sqrt(ss); }
CNR_HD float weight_norm_dv(float g, float nrm, float dot, float dw, float v) { return (g / nrm) * (dw - dot / (nrm * nrm) * v); }

// effective-weight preparation (weight-norm, column permutation, padding, transpose)
struct PrepWeight {
  const float* g = nullptr;   // weight_g [n] or null (plain nn.Linear)
  const float* v = nullptr;   // weight_v / weight [n][k_ref]
  const float* b = nullptr;   // bias [n]
  int n = 0, k_ref = 0;
  int nseg = 0; Segment seg[4];
  float* W = nullptr; int ldw = 0; int npad = 0;      // [npad][ldw]
  float* Wt = nullptr; int ldwt = 0; int kpad = 0;    // [kpad][ldwt]
  float* bias = nullptr;                              // [npad]
  int row_rot = 0;            // internal row i holds reference row (i + row_rot) % n  (SDF top layer: [features | sdf])
};

// dW partial reduction + weight-norm backward + un-permutation
struct FinishWeight {
  const float* partial = nullptr; int nchunk = 0; int npad = 0; int ldk = 0;   // [nchunk][npad][ldk]
  const float* colsum = nullptr;                                             // [ncolsum][npad] or null
  int ncolsum = 0;            // slots that carry column sums (the first group of a region); 0 with colsum != null means nchunk
  const float* g = nullptr; const float* v = nullptr;
  int n = 0, k_ref = 0;
  int nseg = 0; Segment seg[4];
  float* dg = nullptr; float* dv = nullptr; float* db = nullptr;   // outputs (dg null for plain Linear; dv = d weight)
  int row_rot = 0;            // see PrepWeight
  int col_hi = 1 << 30, nchunk_hi = 0;   // columns >= col_hi are summed over nchunk_hi slots (strip columns filled by be_strip_bwd)
};

struct EmbedZ {   // E[r*m + j][0..kEmb) = PE(scale * (o_r + d_r * z[r*ldz + j])), optional coarse-z generation
  const float* o; const float* d; long R; int m;
  float* z; int ldz;            // when make_z: written; else read
  int make_z;                   // 1: z = near + (far-near)*lin(j) (+ (t_rand-0.5)*2/S)          (NeuS.py:311-326)
  const float* near_; const float* far_; const float* t_rand;
  float scale; int multires;
  float* E;                     // [R*m][kEmb]
};

struct EmbedPts {  // E (and optionally AUX[.,0:3]) from explicit points or from a lattice (NeuS.py:15-24)
  const float* pts; long n;            // pts [n][3] or null -> lattice
  int res; float bmin[3], bmax[3]; long start;   // lattice point index = start + i, order x-major (x, y, z)
  float scale; int multires;
  float* E; float* AUX;
};

struct UpSample {   // NeuS.py:136-181 + ray_utils.py:123-154 (det=True)
  const float* o; const float* d; long R;
  const float* z; int ldz; const float* sdf; int lds; int n;   // current samples per ray
  int m;                                             // new samples per ray
  float inv_s;
  float* new_z;                                      // [R][m]
  const float* w_in = nullptr;                       // optional [R][n-1]: section weights given by the caller (plain sample_pdf(det=True),
                                                     // ray_utils.py:123-154, bins = z); o / d / sdf / inv_s are then unused
  const float* u_in = nullptr;                       // optional [R][m]: the uniform draws of sample_pdf(det=False) (ray_utils.py:135-136: torch.rand, drawn by the caller
                                                     // from the CPU generator like the reference); null: det=True, u_k = (k + 0.5) / m
};

struct MergeZ {     // NeuS.py:183-197
  long R; float* z; int ldz; const float* sdf_in; int lds_in; float* sdf_out; int lds_out; int n;   // z merged in place
  const float* new_z; const float* new_sdf; int m;   // new_sdf null on the last step (sdf not updated)
};

struct SamplerStep {   // one launch per up-sampling iteration: [merge of the previous iteration] + up_sample + [PE rows of the new samples]
  int do_merge; MergeZ g;          // cat_z_vals of the previous iteration's new samples (its new_z / new_sdf are read before u.new_z is rewritten)
  UpSample u;                      // on the merged row (u.n = g.n + g.m after a merge); u.w_in must be null
  int do_embed; float* E; float scale; int multires;   // E[(ray * u.m + j)][kEmb] = PE(scale * (o + d * new_z[j])) like EmbedZ
};
void be_sampler_step(const SamplerStep& p, cnr_stream s);

struct FineSetup {  // Color_NeuS.py:41-50: section midpoints, PE input of the SDF net, auxiliary inputs
  const float* o; const float* d; const float* z; long R; int M; float sample_dist;
  float scale; int multires; int multires_view;
  float* E;      // [P][kEmb]
  float* AUX;    // [P][kAux] = [p(3) g(3) PE(dir)(3+6*mv) 0...]
};

struct GradFinish { // g = scale * J_PE^T (ce0 + ce_skip)
  long P; const float* E; const float* ce0; const float* ces; float scale; int multires;
  float* grad_out;   // [P][3] (the 'gradients' output tensor)
  float* AUX;        // g copied to AUX[.,3:6]
  int neg_g_as_view; int multires_view;   // vertex colouring (NeuS.py:60): view_dirs = -g -> AUX[.,6:] = PE(-g)
  float* featx; int ldfx; int F;          // colour-net input [feat | aux | 0]: the aux row is copied to featx[.,F:ldfx)
};

struct CompositeFwd {   // Color_NeuS.py:66-123, NeuS.py:382-399
  const float* o; const float* d; const float* z; long R; int M; float sample_dist;
  const float* sdf; const float* g; const float* color; int ldcolor; const float* gcolor; int ldg;   // gcolor null for plain NeuS
  const float* variance; float cos_anneal; const float* background_rgb;
  float* color_fine; float* s_val; float* cdf_fine; float* weight_sum; float* weight_max; float* weights;
  float* inside_sphere; float* depth; float* global_color;
  float* eik_partial;    // [R][2]
  // optional per-sample copies of the network outputs for callers that composite themselves (N_OUTSIDE > 0 background mixing)
  float* sdf_s; float* color_s; float* gcolor_s;   // [P], [P][3], [P][3] or null
  const float* delta = nullptr; float* delta_ray_sum = nullptr;   // optional: [P][3] relight offsets -> [R] sums over samples and rgb
};

// inference-only early-termination compaction: samples whose compositing weight is below eps contribute < eps to the pixel,
// so the colour / relight networks are evaluated only on the kept samples (valid when the caller consumes colour / depth only)
struct PruneCount { const float* weights; long R; int M; float eps; int* counts; };
struct PruneScan { const int* counts; long R; int* offsets /*[R+1]*/; };
struct PruneGather {
  const float* weights; long R; int M; float eps; const int* offsets;
  int* idx;                                       // [kept] original point index
  const float* featx; int ldfx; float* featx_c;   // rows gathered to the compact list (featx_c null: index list only)
  const float* aux; float* aux_c;                 // [.][kAux]
  // index-list form (forward-only render, chain-fused ReLU stacks read their rows through idx): the per-sample outputs of the DROPPED samples
  // are zeroed here instead of by three memsets over the whole buffers
  float* zero_gcol = nullptr; float* zero_relit = nullptr; float* zero_delta = nullptr;   // [P][4], [P][4] or null, [P][3] or null
  // (zero_gcol and zero_relit are written as whole f4 rows on both backends: 16-byte aligned, as every sub-buffer of the 256-byte arena is)
};
// the keep test of a sample, and what a dropped one leaves behind: its per-sample colour outputs read as zero (it contributes nothing)
CNR_HD bool prune_keep(float weight, float eps) { return weight >= eps; }
CNR_HD void prune_zero_dropped(const PruneGather& p, long pt) {
  if (!p.zero_gcol) return;
  const f4 z4 = {0.f, 0.f, 0.f, 0.f};
  reinterpret_cast<f4*>(p.zero_gcol)[pt] = z4;
  if (p.zero_relit) reinterpret_cast<f4*>(p.zero_relit)[pt] = z4;
  if (p.zero_delta) { p.zero_delta[pt * 3] = 0.f; p.zero_delta[pt * 3 + 1] = 0.f; p.zero_delta[pt * 3 + 2] = 0.f; }
}
struct PruneScatter {
  long P; const int* count; const int* idx;
  const float* gcol_c; const float* relit_c; const float* delta_c;   // compact [.][4], [.][4], [.][3] (relit/delta null for plain NeuS)
  float* gcol; float* relit; float* delta;                            // full-size, pre-zeroed
};

struct ReduceEik { const float* partial; long R; float* sums /*[2]*/; float* sums_out /*[2] or null*/; float* gradient_error; };

struct CompositeBwd {
  const float* o; const float* d; const float* z; long R; int M; float sample_dist;
  const float* sdf; const float* g; const float* color; int ldcolor; const float* gcolor; int ldg;
  const float* variance; float cos_anneal; const float* background_rgb; const float* eik_sums; float sdf_scale;
  int inv_sigmoid; int has_relight;
  // upstream gradients (any may be null)
  const float* d_color_fine; const float* d_s_val; const float* d_cdf; const float* d_weight_sum; const float* d_weight_max;
  const float* d_gradients; const float* d_weights; const float* d_gradient_error; const float* d_depth;
  const float* d_global_color; const float* d_delta_relight; const float* d_delta_relight_ray /* [R] or null, see cnr_render_out_grads */;
  const float* d_sdf_s; const float* d_color_s; const float* d_gcolor_s;   // per-sample cotangents of CompositeFwd::sdf_s / color_s / gcolor_s (or null)
  // per-point cotangents
  float* ztop; int ldztop; int ztop_col;   // ztop[pt][ztop_col] = d sdf / scale (the sdf row is the LAST internal row of the top layer)
  float* gbar;                 // [P][4] d loss / d g through alpha, eikonal and the 'gradients' output
  int ldtop = kTop;            // row stride of dtop / gc_a: kTop (16: the narrow GEMM launches read 16-float rows) or 4 (packed: the streaming head kernels)
  float* dtop;                 // [P][ldtop] cotangent of the last relight layer output (pre-activation), zero padded
  float* gc_a;                 // [P][ldtop] cotangent of the global colour (post-sigmoid): direct + inverse-sigmoid path
  float* dinvs_partial;        // [R]
  float* d_rays_d;             // [R][3] (null when rays need no grad): sum_j d tc_j * g_j
  float* d_z;                  // [P][2] or null: {d loss / d z_j through depth, d loss / d dist_j through alpha} (near / far gradients, N_IMPORTANCE == 0)
};

struct ColTopBwd {  // cotangent of the colour net's last pre-activation
  long P; const float* gc_a /*[P][ldtop]*/; const float* gc_b /* [P][4], may be null */; const float* gcolor; int squeeze; float* out; /*[P][ldtop]*/
  int ldtop = kTop;
};

struct GbarFinish { // total d g, then tangent of the embedding: cbar = J_PE (scale * gbar)
  long P; const float* gbar_alpha; const float* daux_c; const float* daux_r; const float* E; float scale; int multires;
  float* gbar_total /*[P][4]*/; float* cbar /*[P][kEmb]*/;
};

struct VarianceFinish { const float* partial; long R; const float* variance; float* d_variance; };

struct RaysGradFinish {  // d rays_o / d rays_d from the point cotangents (only when rays require grad)
  long R; int M; const float* d; const float* z; float sample_dist;
  const float* pbar;      // [P][4] total cotangent of p
  const float* daux_dir_c; const float* daux_dir_r; int lddir; int multires_view;   // cotangent of PE(dir) parts (may be null)
  const float* d_rays_d_alpha;   // [R][3] from CompositeBwd
  float* d_o; float* d_d;        // may both be null (only near / far need gradients)
  // N_IMPORTANCE == 0: z_j = near + (far - near) * linspace(0,1,S)[j] (+ jitter) is differentiable w.r.t. near / far (NeuS.py:311-313)
  const float* dz_parts;         // [P][2] from CompositeBwd::d_z, or null
  float* d_near; float* d_far;   // [R] or null
};

struct PbarFinish {   // total cotangent of p: colour/relight aux inputs + SDF value path + gradient path (PE second derivative)
  long P; const float* daux_c; const float* daux_r; const float* ebar0; const float* ebars; const float* E;
  const float* ce0; const float* ces; const float* gbar_total /* null: no cotangent on g (value-only SDF query), ce0 / ces unread */;
  float scale; int multires; float* pbar;
};

// SDF point queries (cnr_sdf_query_forward / _backward): the caller's n dense rows <-> the P = round_up(n, kQueryTile) rows of the internal
// buffers.  Padded rows hold the origin as input and zero cotangents; nothing is written past row n of a caller's buffer.
// The forward also writes a tag into the context (kQueryCtxTag + want_grad); the backward's seed launch checks it against the backward's
// want_grad and seeds NaN on a mismatch (a context without the gradient-path buffers, or no query context at all), so that every output of
// such a call is NaN instead of silently wrong.  The library never synchronises, so the check cannot be a host-side error.
constexpr int kQueryCtxTag = 0x53515900;
struct QueryIn {     // pts [n][3] -> out [P][3], rows >= n zero; element 0 also writes *tag = tag_value
  long n, P; const float* pts; float* out; int* tag; int tag_value;
};
struct QuerySeed {   // ztop [P][ldztop] = [d_feat | d_sdf * inv_scale | 0], gbar [P][4] = [d_grad | 0] (gbar may be null); null inputs are zero, rows >= n zero
  long n, P; int F, ldztop; float inv_scale;
  const float* d_sdf; const float* d_feat; const float* d_grad;
  float* ztop; float* gbar;
  const int* tag; int want_grad;   // the forward's tag; want_grad = 1 needs a forward with want_grad, 0 takes either
};
struct QueryOut {    // the first n rows of the internal buffers into the caller's dense ones; every pair may be null
  long n; int F, ldf, ldg;
  const float* sdf_in; const float* feat_in; const float* g_in;   // [P], [P][ldf], [P][ldg]
  float* sdf; float* feat; float* g;                               // [n], [n][F], [n][3]
};
void be_query_in(const QueryIn& p, cnr_stream s);
void be_query_seed(const QuerySeed& p, cnr_stream s);
void be_query_out(const QueryOut& p, cnr_stream s);

// ---- chain-fused kernels (cnr_chain.hip): a tile of points goes through all layers of a chain without leaving the CU
struct PackJob {    // f16 planes [2][rows][ld] (be_split_planes_many) -> fragment-major planes Wf[8][ld/16][2][64][8] of the fused kernels
  const unsigned short* planes; long plane_stride; int rows; int ld; unsigned short* Wf;
};
void be_pack_frags_many(const PackJob* jobs, int count, cnr_stream s);
struct FusedLayer {
  const unsigned short* Wf;   // fragment-major f16 planes of the row-scaled weights
  const float* wsc;           // per output column: 1 / weight row scale
  const float* bias;          // per output column (readable up to column 255; columns >= N are ignored)
  int K;                      // input width, multiple of 16, <= 256
  int N;                      // output columns, <= 256
};
struct SdfValueChain {   // sdf = SDFNetwork.sdf(x) from the embedding rows E (fields.py:81-100), value only
  const float* E; long P;          // [P][kEmb]
  int nl;                          // hidden layers; the narrow top layer (sdf row) is folded into the last epilogue
  FusedLayer lay[kMaxLayers];
  int skip_mask; int emb;          // bit l: layer l takes [softplus(z_{l-1}) | e] / sqrt(2)
  const float* wtop; const float* btop; float top_scale;   // sdf row of the top layer (fp32 effective weights), its bias, sign / scale
  float* sdf_out;                  // [P]
};
bool be_sdf_value_chain(const SdfValueChain& c, cnr_stream s);   // false: not handled (backend without fused kernels / unsupported shape)
// The SAVING SDF forward (Color_NeuS.py:52-54 on the fine samples): the value chain above that also leaves behind what the backward pass
// reads -- every hidden layer's PRE-activation row z_l (the tail columns of the layer in front of a skip connection receive e: the tail fill
// of the per-layer launches), the row scales of the layer inputs, the feature rows of the top layer -- in one launch (cnr_chain_fwd.hip).
struct SdfSaveChain {
  SdfValueChain v;                 // E, P, hidden layers, skip mask, sdf row of the top layer, sdf_out
  float* Z[kMaxLayers] = {};       // [P][ldz] per hidden layer
  int ldz = 0;
  float* rs[kMaxLayers + 1] = {};  // optional [P]: power-of-two scale of the input row of layer l (l >= 1; LayerGemm::rs_out convention)
  FusedLayer top;                  // the feature rows of the top layer (K == 256, N == 256): feat = h W^T + b, no activation
  float* feat = nullptr; int ld_feat = 0;   // [P][ld_feat]
};
bool be_sdf_save_chain(const SdfSaveChain& c, cnr_stream s);      // false: not handled

// The SAVING forward chains of the ReLU stacks (colour network fields.py:161-188, relight network fields.py:332-368) in ONE launch
// (cnr_chain_fwd.hip): a 128-point tile goes through colour lin0..lin(NC-2) + the rgb head, then relight in_layer + rl_mlp[0..NR-2] + the
// relight head, without the activations leaving the CU between layers; every hidden layer's ReLU output is stored once for the backward
// pass (rows transposed through LDS into full 128-byte lines), the row scales of the layer inputs with it.
constexpr int kChainSteps = 12;
struct ChainFwdStep {
  const unsigned short* Wf = nullptr;   // fragment-major f16 planes of the layer (FusedLayer::Wf layout, nkb_w k16 blocks per column block)
  const float* wsc = nullptr;           // per output column: 1 / weight row scale (256 readable)
  const float* bias = nullptr;          // per output column (256 readable)
  int nkb_w = 0;                        // ldw / 16
  int nkb_main = 0;                     // k16 blocks of the main input segment: 16 (a 256-wide row) or 1..3 (a narrow global input)
  int nkb_x = 0;                        // k16 blocks of the extra segment (W columns from 16 * nkb_main on): 0..3
  const float* in = nullptr; int ld_in = 0;   // main segment = columns [0, 16 nkb_main) of these global rows; null: the previous step's ReLU output (on chip)
  int x_src = 0;                        // extra segment: 1 = columns [16 nkb_main, 16 (nkb_main + nkb_x)) of the same global row,
                                        // 2 = the colour head's output kept on chip ([rgb | 0...], the relight y-layer's input tail)
  float* save = nullptr; int ld_save = 0;     // [P][ld_save]: ReLU output of this step (256 columns)
  float* rs_in = nullptr;               // optional [P]: power-of-two scale of this step's whole input row (LayerGemm::rs_out convention)
  int head = 0;                         // 1 / 2: the colour / relight head follows this step (end of a chain)
};
struct ChainFwdHead { const float* W = nullptr; int ldw = 0; const float* bias = nullptr; int n = 0; };   // fp32 effective weights [n <= 4][ldw >= 256]
struct ReluChainFwd {
  long P = 0; int nsteps = 0; ChainFwdStep st[kChainSteps];
  ChainFwdHead col_head; int col_squeeze = 1;           // rgb = sigmoid(.) (EK_SIGMOID) or plain (EK_LINEAR_SIG)
  float* gcol = nullptr;                                // [P][4]
  float* rgb_tail = nullptr; int ld_tail = 0;           // optional: rgb_tail[row * ld_tail + c] = rgb (c < n) or 0 (c < 16): the relight y-layer's input tail
  ChainFwdHead rel_head; int inv_sigmoid = 1;
  float* delta = nullptr;                               // [P][3] relight offsets (pre-activation)
  float* relit = nullptr;                               // [P][4] relight_apply(rgb, delta)
  int dbg = 0;                                          // ablation switches (CNR_CHAIN_FWD_DBG; wrong results): 1 no saves, 2 no MFMAs, 8 no global stores
  // forward-only render with early-termination compaction (inference): the chains run on the first *P_dev entries of row_idx only -- chain-start
  // rows are read from, and the heads' outputs written to, point row_idx[i]; P is then the upper bound that sizes the launch.  No saves.
  const int* P_dev = nullptr; const int* row_idx = nullptr;
};
bool be_relu_chain_fwd(const ReluChainFwd& c, cnr_stream s);   // false: not handled (per-layer launches instead)
bool be_relu_chain_fwd_enabled();                               // the debugging switches that turn the chain-fused ReLU forward off are not set

void be_layer_gemm(const LayerGemm& g, cnr_stream s);
// Second-order sweep launch of a narrow-input layer (K <= 48, 256 outputs) that also forms the gradient-chain weight-gradient pair of the layer
// (u = sp'(z) v from the epilogue's side inputs, the launch's input rows) into be_sweep0_slots(g.P) slots of [256][ldk] floats (cnr_sweep0.hip).
// Backward of a narrow-input layer (<= 48 input columns, 256 outputs) in one pass over its 256-wide output cotangent X (cnr_narrow_bwd.hip):
// dW[j][c] = sum X[pt][j] Y[pt][c] and db[j] = sum X[pt][j] into be_narrow_bwd_slots(P) slots ([256][ldk] / [256] floats each), and -- with Wp --
// dx[pt][c] = sum_j X[pt][j] Wt[c][j] for c < ndx (Wp / wscale: the f16 planes and row scales of W^T, rows = input columns, ldw = 256).
// partial == nullptr: only dx (then X may be the view sp'(X) * Xb: the 39-column end of the forward gradient chain).
struct NarrowBwd {
  const float* X = nullptr; int ldx = 0;
  const float* Xb = nullptr; int ldxb = 0;   // optional: X stands for the view softplus100'(X) * Xb (launches without a weight gradient: partial == nullptr)
  const float* Y = nullptr; int ldy = 0; int ky = 0;
  long P = 0;
  const unsigned short* Wp = nullptr; long wp_stride = 0; int ldw = 0; int w_rows = 0; const float* wscale = nullptr;
  float* dx = nullptr; int lddx = 0; int ndx = 0;
  float* partial = nullptr; int ldk = 0; float* colsum = nullptr;
};
bool be_narrow_bwd_ok(const NarrowBwd& p);
int be_narrow_bwd_slots(long P);
void be_narrow_bwd(const NarrowBwd& p, cnr_stream s);
bool be_sweep0_ok(const LayerGemm& g);
int be_sweep0_slots(long P);
void be_sweep0_dw(const LayerGemm& g, float* partial, int ldk, cnr_stream s);
void be_dw_gemm(const DwGemm& g, cnr_stream s);
// Layer launch g + the single-pair weight gradient d (X[0] = the launch's input view, Y[0] = the operand its epilogue derives from its side
// inputs, see DwFuse in cnr_views.h) with d.partial / d.colsum laid out in kFdwSlots slots.  Callers test be_fdw_enabled() && fdw_shape_ok(g)
// first; the backend may still run the two parts as separate launches (same results, same slots).
// Backward of a <= 4-wide head (rgb / relight offset: nn.Linear(256, 3) after a ReLU) in ONE streaming launch instead of a K = 3 layer launch +
// a weight-gradient strip launch that re-reads the same 1 KB/point: dout[pt][k] = aux[pt][k] > 0 ? sum_j W[j][k] dtop[pt][j] : 0 (the
// EK_RELU_MASK epilogue), dW[j][k] = sum_pt dtop[pt][j] aux[pt][k], db[j] = sum_pt dtop[pt][j]; fp32 FMAs, fixed-order partial sums per slot.
struct HeadBwd {
  const float* dtop; int ldt;     // [P][ldt] cotangent of the head's output (n live columns)
  const float* aux; int ldaux;    // [P][ldaux] the head's input = ReLU output of the layer below (K live columns)
  const float* W; int ldw;        // [n][ldw] effective weights (natural orientation)
  int n; int K; long P;           // n <= 4, K <= 256 (one thread per column)
  float* dout; int ldo;           // [P][ldo] cotangent of the layer below (pre-activation)
  float* partial; float* colsum; int npad, ldk, nslots;   // [nslots][npad][ldk], [nslots][npad]
};
void be_head_bwd(const HeadBwd& p, cnr_stream s);
// Forward pass of a narrow head (<= 4 outputs) on a 256-wide activation: y[pt][j] = sum_c h[pt][c] * W[j][c], through the head's epilogue E
// (epi_apply, columns 0..15: bias, sigmoid / relight, pad-column handling).  One streaming pass; a launch of the FP32-MFMA layer kernel
// spends a 32-column tile on the 3 columns.
struct HeadFwd {
  const float* h; int ldh; long P; const int* P_dev;   // [P][ldh], 256 live columns (ldh % 4 == 0); P_dev: optional device-side row count
  const float* W; int ldw; int n;                       // [n][ldw] effective weights
  Epi E;
};
void be_head_fwd(const HeadFwd& p, cnr_stream s);
// The few input columns beyond 256 of a 256-wide layer (relight y-layer: + rgb, colour layer 0: + p, g) in the backward pass, one streaming
// pass over the layer's output cotangent instead of a narrow layer launch plus a weight-gradient strip launch:
//   tail[pt][j]                    = tail_scale * sum_n dout[pt][n] * Wt[256 + j][n]          (cotangent of input column 256 + j)
//   partial[slot][n][256 + j]      = sum over the slot's points of dout[pt][n] * y[pt][j]     (weight-gradient strip; zero for nt <= j < ldk - 256)
struct StripBwd {
  const float* dout; int ldo; long P;   // [P][ldo], 256 live columns (ldo % 4 == 0)
  int nt;                               // extra input columns, 1..8
  const float* Wt; int ldwt;            // transposed fp32 weights [k][ldwt]: row 256 + j is used
  float* tail; int ldt; float tail_scale;   // [P][ldt] (null: cotangent not wanted)
  const float* y; int ldy;              // [P][ldy]: column j = input column 256 + j of the layer
  float* partial; int npad, ldk, nslots;    // [nslots][npad][ldk]
};
void be_strip_bwd(const StripBwd& p, cnr_stream s);
bool be_fdw_enabled();
bool be_fdw_xrow();          // DwFuse::xrow_mode / LayerGemm::k_extra are available in be_layer_dw_gemm
void be_layer_dw_gemm(const LayerGemm& g, const DwGemm& d, const DwFuse& f, cnr_stream s);
// all layers of a model in two launches (the per-layer launches are latency-bound: 57 launches of a few microseconds each)
// SplitJob: fp32 matrix [rows][ld] -> two f16 planes of the row-scaled matrix (x * 2^e = hi + lo, 22 significand bits) + 1/2^e per row,
// for the weight-stationary f16-split GEMM (cnr_gemm.hip)
struct SplitJob { const float* src; int rows; int ld; unsigned short* planes; float* inv_scale; };
void be_prep_weights(const PrepWeight* p, int count, cnr_stream s);
void be_finish_weights(const FinishWeight* f, int count, cnr_stream s);   // every layer keeps its own partial buffer until this launch
void be_split_planes_many(const SplitJob* jobs, int count, cnr_stream s);
void be_embed_z(const EmbedZ& p, cnr_stream s);
void be_embed_pts(const EmbedPts& p, cnr_stream s);
void be_upsample(const UpSample& p, cnr_stream s);
void be_merge(const MergeZ& p, cnr_stream s);
void be_fine_setup(const FineSetup& p, cnr_stream s);
void be_grad_finish(const GradFinish& p, cnr_stream s);
void be_composite_fwd(const CompositeFwd& p, cnr_stream s);
void be_reduce_eik(const ReduceEik& p, cnr_stream s);
void be_prune_count(const PruneCount& p, cnr_stream s);
void be_prune_scan(const PruneScan& p, cnr_stream s);
void be_prune_gather(const PruneGather& p, cnr_stream s);
void be_prune_scatter(const PruneScatter& p, cnr_stream s);
void be_composite_bwd(const CompositeBwd& p, cnr_stream s);
void be_coltop_bwd(const ColTopBwd& p, cnr_stream s);
void be_gbar_finish(const GbarFinish& p, cnr_stream s);
void be_variance_finish(const VarianceFinish& p, cnr_stream s);
void be_pbar_finish(const PbarFinish& p, cnr_stream s);
void be_rays_grad_finish(const RaysGradFinish& p, cnr_stream s);
void be_memset_zero(void* p, size_t bytes, cnr_stream s);

// p[row][c] = 0 for c in [c0, c1), row < rows: zero the pad columns a GEMM reads without touching the rest of a wide buffer
void be_zero_cols(float* p, int ld, int c0, int c1, long rows, cnr_stream s);
// dst[row][c] = src[row][c] for c < ncols (two row-major matrices with different row strides): compact <-> padded operand buffers
void be_copy_cols(float* dst, int ld_dst, const float* src, int ld_src, int ncols, long rows, cnr_stream s);
struct KernelTiming { char name[32]; int kind; int nt; long P; int N, K, pairs; float ms; double bytes; };
void be_timing_enable(int on);
int be_timing_collect(KernelTiming* out, int max_records);   // synchronises the recorded events, returns #records, resets
const char* be_name();
int be_check_last_error(char* msg, size_t n);   // 0 ok
// Named ranges for profilers (rocprofv3 --marker-trace): roctxRangePush / Pop of librocprofiler-sdk-roctx / libroctx64, loaded on first use
// when CNR_ROCTX=1 (no link dependency; without the variable or the library these are no-ops)
void be_range_push(const char* name);
void be_range_pop();
struct RangeScope { explicit RangeScope(const char* name) { be_range_push(name); } ~RangeScope() { be_range_pop(); } };

}  // namespace cnr
