// The stand-alone ops of the ABI: each checks its arguments, fills one descriptor and enqueues its kernels.  None uses the render model, a
// context or the arena: this unit takes only fail / check_backend from cnr_plan.h.
#include "cnr_plan.h"
#include "cnr_loss.h"
#include "cnr_optim.h"
#include "cnr_rays.h"
#include "cnr_pixels.h"
#include "cnr_cameras.h"
#include "cnr_mc.h"
#include "cnr_nn.h"
#include "cnr_image.h"
#include "cnr_raster.h"
#include "cnr_meshcc.h"
#include "cnr_surface.h"
#include "cnr_cull.h"
#include "cnr_register.h"

using namespace cnr;

extern "C" {

// the one layout of the loss scratch: [kLossBlocks][4] partial sums | 16 bytes whose first 4 are the completion counter of the one-launch forms.
// Returns the size; with a base pointer it also places the two parts.
struct LossScratch { float* partial; unsigned* ticket; };
static size_t loss_layout(void* base, LossScratch* p) {
  const size_t partial = (size_t)kLossBlocks * 4 * sizeof(float);
  if (p) { p->partial = static_cast<float*>(base); p->ticket = reinterpret_cast<unsigned*>(static_cast<char*>(base) + partial); }
  return partial + 16;
}
size_t cnr_loss_scratch_bytes(int64_t n_rays) { (void)n_rays; return loss_layout(nullptr, nullptr); }

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
  LossArgs a; LossScratch w;
  if (loss_args(cfg, color_fine, weight_sum, delta_relight, rgb_gt, mask, n_rays, n_samples, a)) return -1;
  if (!sums || !scratch) return fail("null argument");
  if (mask && !weight_sum) return fail("weight_sum is required with a mask");
  if (scratch_bytes < loss_layout(scratch, &w)) return fail("loss scratch too small");
  be_loss_sums(a, w.partial, sums, (cnr_stream)stream);
  return check_backend("loss_sums");
}

int cnr_loss_sums_ray(const cnr_loss_config* cfg, const float* color_fine, const float* weight_sum, const float* delta_relight_ray_sum,
                      const float* rgb_gt, const float* mask, int64_t n_rays, int32_t n_samples, float* sums, void* scratch, size_t scratch_bytes,
                      void* stream) {
  LossArgs a; LossScratch w;
  if (loss_args(cfg, color_fine, weight_sum, delta_relight_ray_sum, rgb_gt, mask, n_rays, n_samples, a)) return -1;
  if (!sums || !scratch) return fail("null argument");
  if (mask && !weight_sum) return fail("weight_sum is required with a mask");
  if (scratch_bytes < loss_layout(scratch, &w)) return fail("loss scratch too small");
  a.drel_per_ray = 1;
  be_loss_sums(a, w.partial, sums, (cnr_stream)stream);
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
  LossArgs a; LossScratch w;
  LossScalars c;
  if (loss_args(cfg, color_fine, weight_sum, delta_relight, rgb_gt, mask, n_rays, n_samples, a)) return -1;
  if (loss_scalars(cfg, n_rays_global, n_samples, use_mask, use_relight, c)) return -1;
  if (!sums || !out || !scratch || !gradient_error) return fail("null argument");
  if (mask && !weight_sum) return fail("weight_sum is required with a mask");
  if (scratch_bytes < loss_layout(scratch, &w)) return fail("loss scratch too small");
  a.drel_per_ray = delta_per_ray != 0;
  be_loss_forward(a, w.partial, w.ticket, c, gradient_error, sums, out, (cnr_stream)stream);
  return check_backend("loss_forward");
}

int cnr_loss_shard_stats(const cnr_loss_config* cfg, const float* color_fine, const float* weight_sum, const float* delta_relight, int32_t delta_per_ray,
                         const float* rgb_gt, const float* mask, const float* eik_sums, int64_t n_rays, int32_t n_samples, float* stats, void* scratch,
                         size_t scratch_bytes, void* stream) {
  LossArgs a; LossScratch w;
  if (loss_args(cfg, color_fine, weight_sum, delta_relight, rgb_gt, mask, n_rays, n_samples, a)) return -1;
  if (!stats || !scratch || !eik_sums) return fail("null argument");
  if (mask && !weight_sum) return fail("weight_sum is required with a mask");
  if (scratch_bytes < loss_layout(scratch, &w)) return fail("loss scratch too small");
  a.drel_per_ray = delta_per_ray != 0;
  be_loss_shard_stats(a, w.partial, w.ticket, eik_sums, stats, (cnr_stream)stream);
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
// the one layout of the pixel table's scratch (loss_layout's form): a {foreground, background} count pair per image and tile
static size_t pixel_table_layout(int32_t n_images, int64_t hw, void* base, PixelTable* t) {
  const long tiles = pixel_tiles(hw);
  if (t) { t->tile_counts = static_cast<int*>(base); t->tiles = tiles; }
  return round_up_sz((size_t)n_images * (size_t)tiles * 2 * sizeof(int), 256);
}
size_t cnr_pixel_table_scratch_bytes(int32_t n_images, int64_t pixels_per_image) {
  return n_images <= 0 || pixels_per_image <= 0 ? 0 : pixel_table_layout(n_images, pixels_per_image, nullptr, nullptr);
}

int cnr_pixel_table_build(const float* masks, int32_t n_images, int64_t pixels_per_image, int32_t* order, int32_t* fg_count, int32_t* bg_count,
                          void* scratch, size_t scratch_bytes, void* stream) {
  if (pixel_table_dims("pixel_table_build", n_images, pixels_per_image)) return -1;
  if (!masks || !order || !fg_count || !bg_count || !scratch) return fail("pixel_table_build: null argument");
  PixelTable t;
  if (scratch_bytes < pixel_table_layout(n_images, pixels_per_image, scratch, &t)) return fail("pixel_table_build scratch too small");
  t.masks = masks; t.n_images = n_images; t.hw = (long)pixels_per_image; t.order = order; t.fg_count = fg_count; t.bg_count = bg_count;
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

// the one layout of the marching-cubes scratch (loss_layout's form): counts [n][2] | block sums [nblocks][2] | flags [n], n = res^3 voxels
static size_t mc_layout(int32_t res, char* base, McVolume* v) {
  const size_t n = (size_t)res * res * res;
  const size_t nblocks = (n + kMcScanBlock - 1) / kMcScanBlock;
  const size_t counts = round_up_sz(n * 2 * sizeof(int), 256), sums = round_up_sz(nblocks * 2 * sizeof(int), 256);
  if (v) { v->counts = reinterpret_cast<int*>(base); v->block_sums = reinterpret_cast<int*>(base + counts); v->flags = reinterpret_cast<unsigned char*>(base + counts + sums); }
  return counts + sums + round_up_sz(n, 256);
}
size_t cnr_mc_scratch_bytes(int32_t resolution) { return resolution < 2 ? 0 : mc_layout(resolution, nullptr, nullptr); }

static int mc_volume(int32_t res, float thr, const float* u, void* scratch, size_t scratch_bytes, McVolume& v) {
  if (!u || !scratch) return fail("null argument");
  if (res < 2 || res > 1290) return fail("marching cubes: resolution must be in [2, 1290]");   // res^3 voxel ids and 2 * res^3 counts stay below 2^31
  if (scratch_bytes < mc_layout(res, static_cast<char*>(scratch), &v)) return fail("marching cubes scratch too small");
  v.u = u; v.res = res; v.thr = thr; v.totals = nullptr;
  return 0;
}

int cnr_mc_count(const float* u, int32_t resolution, float threshold, void* scratch, size_t scratch_bytes, int32_t* totals, void* stream) {
  McVolume v;
  if (mc_volume(resolution, threshold, u, scratch, scratch_bytes, v)) return -1;
  if (!totals) return fail("null argument");
  v.totals = totals;
  be_mc_count(v, (cnr_stream)stream);
  return check_backend("mc_count");
}

int cnr_mc_emit(const float* u, int32_t resolution, float threshold, const float* bound_min, const float* bound_max, void* scratch,
                size_t scratch_bytes, float* vertices, int32_t* triangles, void* stream) {
  McVolume v;
  if (mc_volume(resolution, threshold, u, scratch, scratch_bytes, v)) return -1;
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

static long image_blocks(int64_t planes, int H, int W, int cs) { return (long)planes * img_tiles_y(H) * img_tiles_x(W, cs); }
// the one layout of the image scratch (loss_layout's form), which serves one call at a time: cnr_image_metrics' {sum d*d, sum ssim} pair of doubles
// per tile of the [B][C][H][W] form (the channels-last form never has more tiles) and 256 bytes, or cnr_image_panel's two range keys at its start
static size_t image_layout(int64_t n_images, int channels, int H, int W, void* base, double** partials, unsigned** keys) {
  if (partials) *partials = static_cast<double*>(base);
  if (keys) *keys = static_cast<unsigned*>(base);
  return round_up_sz((size_t)image_blocks(n_images * channels, H, W, 1) * 2 * sizeof(double), 256) + 256;
}
size_t cnr_image_scratch_bytes(int64_t n_images, int channels, int H, int W) {
  return n_images <= 0 || channels < 1 || H < 1 || W < 1 ? 0 : image_layout(n_images, channels, H, W, nullptr, nullptr, nullptr);
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
    if (scratch_bytes < image_layout(n_images, channels, H, W, scratch, &p.partials, nullptr)) return fail("image_metrics scratch too small");
    p.cs = channels_last ? channels : 1;
    p.planes = channels_last ? (long)n_images : (long)n_images * channels;
    p.nblocks = image_blocks(p.planes, H, W, p.cs);
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
  image_layout(1, 3, H, W, scratch, nullptr, &p.keys);
  be_image_panel(p, (cnr_stream)stream);
  return check_backend("image_panel");
}

// the one layout of the rasteriser's scratch: projected vertices | z-buffer keys | large-triangle list | its length.  Returns the size; with a
// base pointer it also places the four parts.
static size_t raster_layout(int64_t V, int64_t F, int64_t hw, char* base, MeshRaster* p) {
  const size_t pv = round_up_sz((size_t)V * sizeof(RasterVert), 256), keys = round_up_sz((size_t)hw * sizeof(unsigned long long), 256);
  const size_t large = round_up_sz((size_t)F * sizeof(int), 256);
  if (p) {
    p->pv = reinterpret_cast<RasterVert*>(base);
    p->keys = reinterpret_cast<unsigned long long*>(base + pv);
    p->large = reinterpret_cast<int*>(base + pv + keys);
    p->n_large = reinterpret_cast<int*>(base + pv + keys + large);
  }
  return pv + keys + large + 256;
}
static bool raster_sizes_ok(int64_t V, int64_t F, int32_t H, int32_t W) {
  return V >= 0 && F >= 0 && V < (int64_t)1 << 31 && F < (int64_t)1 << 31 && H >= 1 && W >= 1 && (int64_t)H * W < (int64_t)1 << 31;
}
size_t cnr_mesh_raster_scratch_bytes(int64_t n_vertices, int64_t n_triangles, int32_t H, int32_t W) {
  if (!raster_sizes_ok(n_vertices, n_triangles, H, W)) return 0;
  return raster_layout(n_vertices, n_triangles, (int64_t)H * W, nullptr, nullptr);
}

int cnr_mesh_raster(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const float* colors, const float* c2w,
                    const float* focal, int32_t H, int32_t W, int32_t opengl, const float* origin, float radius, float z_near,
                    const float* background, float* rgb, float* depth, int32_t* tri_id, int32_t* dropped, void* scratch, size_t scratch_bytes,
                    void* stream) {
  if (H < 1 || W < 1) return fail("mesh_raster: H and W must be at least 1 (got %d x %d)", H, W);
  if ((int64_t)H * W >= (int64_t)1 << 31) return fail("mesh_raster: the image must have fewer than 2^31 pixels");
  if (n_vertices < 0 || n_triangles < 0) return fail("mesh_raster: n_vertices and n_triangles must not be negative");
  if (n_vertices >= (int64_t)1 << 31 || n_triangles >= (int64_t)1 << 31)
    return fail("mesh_raster: n_vertices and n_triangles must be below 2^31 (the indices are int32)");
  if ((n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles) || !c2w || !focal || !depth || !tri_id || !dropped || !scratch)
    return fail("mesh_raster: null argument");
  if ((rgb == nullptr) != (colors == nullptr)) return fail("mesh_raster: rgb and colors must be given together or be null together");
  if (scratch_bytes < raster_layout(n_vertices, n_triangles, (int64_t)H * W, nullptr, nullptr)) return fail("mesh_raster scratch too small");
  MeshRaster p;
  p.vertices = vertices; p.V = (long)n_vertices; p.triangles = triangles; p.F = (long)n_triangles; p.colors = colors;
  p.c2w = c2w; p.focal = focal; p.origin = origin; p.radius = radius; p.z_near = z_near; p.H = H; p.W = W; p.opengl = opengl;
  for (int k = 0; k < 3; ++k) p.background[k] = background ? background[k] : 0.0f;
  p.rgb = rgb; p.depth = depth; p.tri_id = tri_id; p.dropped = dropped;
  raster_layout(n_vertices, n_triangles, (int64_t)H * W, static_cast<char*>(scratch), &p);
  be_mesh_raster(p, (cnr_stream)stream);
  return check_backend("mesh_raster");
}

// the three mesh-cleaning entries share the size rule: indices and counts are int32
static int mesh_sizes(const char* what, int64_t F, int64_t V) {
  if (F < 0 || V < 0) return fail("%s: n_triangles and n_vertices must not be negative", what);
  if (F > INT32_MAX || V > INT32_MAX)
    return fail("%s: n_triangles and n_vertices must not exceed 2^31 - 1 (indices and counts are int32; got %lld and %lld)", what, (long long)F, (long long)V);
  return 0;
}

int cnr_mesh_components(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, int32_t* labels, int32_t* face_count,
                        int32_t* vertex_count, int32_t* summary, int32_t* dropped, void* stream) {
  if (mesh_sizes("mesh_components", n_triangles, n_vertices)) return -1;
  if ((n_triangles > 0 && !triangles) || (n_vertices > 0 && (!labels || !face_count || !vertex_count)) || !summary || !dropped)
    return fail("mesh_components: null argument");
  if (reinterpret_cast<uintptr_t>(summary) % 8 != 0) return fail("mesh_components: summary must be 8-byte aligned");
  MeshComponents p;
  p.triangles = triangles; p.F = (long)n_triangles; p.V = (long)n_vertices;
  p.labels = labels; p.face_count = face_count; p.vertex_count = vertex_count; p.summary = summary; p.dropped = dropped;
  be_mesh_components(p, (cnr_stream)stream);
  return check_backend("mesh_components");
}

int cnr_mesh_select(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, const int32_t* labels, const int32_t* face_count,
                    const int32_t* summary, int32_t mode, int32_t min_faces, float min_ratio, uint8_t* keep_vertex, uint8_t* keep_face,
                    int32_t* vertex_map, int32_t* face_map, int32_t* totals, void* stream) {
  if (mesh_sizes("mesh_select", n_triangles, n_vertices)) return -1;
  if (mode != CNR_MESH_KEEP_LARGEST && mode != CNR_MESH_KEEP_THRESHOLD) return fail("mesh_select: mode must be 0 (largest) or 1 (threshold), got %d", mode);
  if (min_faces < 0 || !(min_ratio >= 0.0f)) return fail("mesh_select: min_faces and min_ratio must not be negative (or NaN)");
  if ((n_triangles > 0 && (!triangles || !keep_face || !face_map)) || (n_vertices > 0 && (!labels || !face_count || !keep_vertex || !vertex_map)) ||
      !summary || !totals)
    return fail("mesh_select: null argument");
  MeshSelect p;
  p.triangles = triangles; p.F = (long)n_triangles; p.V = (long)n_vertices; p.labels = labels; p.face_count = face_count; p.summary = summary;
  p.mode = mode; p.min_faces = min_faces; p.min_ratio = min_ratio;
  p.keep_vertex = keep_vertex; p.keep_face = keep_face; p.vertex_map = vertex_map; p.face_map = face_map; p.totals = totals;
  be_mesh_select(p, (cnr_stream)stream);
  return check_backend("mesh_select");
}

int cnr_mesh_compact(const float* vertices, const float* colors, const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                     const int32_t* vertex_map, const int32_t* face_map, float* out_vertices, float* out_colors, int32_t* out_triangles,
                     void* stream) {
  if (mesh_sizes("mesh_compact", n_triangles, n_vertices)) return -1;
  // (an output array is empty, and may be NULL, when its map keeps nothing: V' and F' are the caller's knowledge, from cnr_mesh_select's totals)
  if ((n_triangles > 0 && (!triangles || !face_map)) || (n_vertices > 0 && (!vertices || !vertex_map))) return fail("mesh_compact: null argument");
  if ((colors == nullptr) != (out_colors == nullptr)) return fail("mesh_compact: colors and out_colors must be given together or be null together");
  MeshCompact p;
  p.vertices = vertices; p.colors = colors; p.triangles = triangles; p.F = (long)n_triangles; p.V = (long)n_vertices;
  p.vertex_map = vertex_map; p.face_map = face_map; p.out_vertices = out_vertices; p.out_colors = out_colors; p.out_triangles = out_triangles;
  be_mesh_compact(p, (cnr_stream)stream);
  return check_backend("mesh_compact");
}

// the three surface entries share the mesh's size rule: at least one face, indices and face numbers are int32
static int surface_sizes(const char* what, int64_t F, int64_t V) {
  if (F <= 0) return fail("%s: the mesh has no faces (n_triangles = %lld)", what, (long long)F);
  if (V < 0) return fail("%s: n_vertices must not be negative", what);
  if (F >= (int64_t)1 << 31 || V >= (int64_t)1 << 31)
    return fail("%s: n_triangles and n_vertices must be below 2^31 (indices and face numbers are int32; got %lld and %lld)", what, (long long)F, (long long)V);
  return 0;
}

int cnr_mesh_area_cdf(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, uint64_t* cdf, int64_t* summary,
                      void* stream) {
  if (surface_sizes("mesh_area_cdf", n_triangles, n_vertices)) return -1;
  if ((n_vertices > 0 && !vertices) || !triangles || !cdf || !summary) return fail("mesh_area_cdf: null argument");
  if (reinterpret_cast<uintptr_t>(cdf) % 8 != 0 || reinterpret_cast<uintptr_t>(summary) % 8 != 0)
    return fail("mesh_area_cdf: cdf and summary must be 8-byte aligned");
  MeshAreaCdf p;
  p.vertices = vertices; p.V = (long)n_vertices; p.triangles = triangles; p.F = (long)n_triangles;
  p.cdf = reinterpret_cast<unsigned long long*>(cdf); p.summary = reinterpret_cast<long long*>(summary);
  be_mesh_area_cdf(p, (cnr_stream)stream);
  return check_backend("mesh_area_cdf");
}

int cnr_mesh_sample(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const uint64_t* cdf, int64_t n_samples,
                    int64_t seed, float* points, int32_t* faces, float* bary, void* stream) {
  if (n_samples < 0) return fail("mesh_sample: n_samples < 0");
  if (surface_sizes("mesh_sample", n_triangles, n_vertices)) return -1;
  if (n_samples == 0) return 0;
  if ((n_vertices > 0 && !vertices) || !triangles || !cdf || !points || !faces) return fail("mesh_sample: null argument");
  if (reinterpret_cast<uintptr_t>(cdf) % 8 != 0) return fail("mesh_sample: cdf must be 8-byte aligned");
  MeshSample p;
  p.vertices = vertices; p.V = (long)n_vertices; p.triangles = triangles; p.F = (long)n_triangles;
  p.cdf = reinterpret_cast<const unsigned long long*>(cdf); p.n = (long)n_samples;
  p.seed_lo = (unsigned)((uint64_t)seed & 0xffffffffull); p.seed_hi = (unsigned)((uint64_t)seed >> 32);
  p.points = points; p.faces = faces; p.bary = bary;
  be_mesh_sample(p, (cnr_stream)stream);
  return check_backend("mesh_sample");
}

int cnr_point_mesh_distance(const float* query, int64_t n_query, const float* vertices, int64_t n_vertices, const int32_t* triangles,
                            int64_t n_triangles, float* dist2, int32_t* face, float* closest, uint64_t* keys, void* stream) {
  if (n_query < 0) return fail("point_mesh_distance: n_query < 0");
  if (surface_sizes("point_mesh_distance", n_triangles, n_vertices)) return -1;
  if (n_query == 0) return 0;
  if (!query || (n_vertices > 0 && !vertices) || !triangles || !dist2 || !face || !keys) return fail("point_mesh_distance: null argument");
  if (reinterpret_cast<uintptr_t>(keys) % 8 != 0) return fail("point_mesh_distance: keys must be 8-byte aligned");
  PointMeshDist p;
  p.query = query; p.n = (long)n_query; p.vertices = vertices; p.V = (long)n_vertices; p.triangles = triangles; p.F = (long)n_triangles;
  p.dist2 = dist2; p.face = face; p.closest = closest; p.keys = reinterpret_cast<unsigned long long*>(keys);
  be_point_mesh_distance(p, (cnr_stream)stream);
  return check_backend("point_mesh_distance");
}

// the two view entries share the image's size rule: the packed rows of a stack are indexed below 2^31 words
static int cull_image_sizes(const char* what, int64_t n, int32_t H, int32_t W) {
  if (n < 0) return fail("%s: the number of images must not be negative (got %lld)", what, (long long)n);
  if (H < 1 || W < 1) return fail("%s: H and W must be at least 1 (got %d x %d)", what, H, W);
  if ((int64_t)H * W >= (int64_t)1 << 31) return fail("%s: the image must have fewer than 2^31 pixels", what);
  if (n > 0 && ((int64_t)1 << 31) / ((int64_t)H * ((W + 63) / 64)) <= n) return fail("%s: the packed stack must have fewer than 2^31 words", what);
  return 0;
}

int cnr_mask_dilate(const float* masks, int64_t n_images, int32_t H, int32_t W, int32_t radius, uint64_t* row_bits, uint64_t* bits, void* stream) {
  if (cull_image_sizes("mask_dilate", n_images, H, W)) return -1;
  if (radius < 0 || radius > kCullMaxRadius) return fail("mask_dilate: radius must lie in [0, %d] (got %d)", kCullMaxRadius, radius);
  if (n_images == 0) return 0;
  if (!masks || !row_bits || !bits) return fail("mask_dilate: null argument");
  if (reinterpret_cast<uintptr_t>(row_bits) % 8 != 0 || reinterpret_cast<uintptr_t>(bits) % 8 != 0)
    return fail("mask_dilate: row_bits and bits must be 8-byte aligned");
  MaskDilate p;
  p.masks = masks; p.n = (long)n_images; p.H = H; p.W = W; p.Wq = (W + 63) / 64; p.radius = radius;
  p.row_bits = reinterpret_cast<unsigned long long*>(row_bits); p.bits = reinterpret_cast<unsigned long long*>(bits);
  be_mask_dilate(p, (cnr_stream)stream);
  return check_backend("mask_dilate");
}

int cnr_mesh_view_votes(const float* vertices, int64_t n_vertices, const float* c2w, const float* focal, const float* origin, float radius,
                        float z_near, int32_t opengl, int64_t n_views, int32_t H, int32_t W, const uint64_t* mask_bits, const float* depth,
                        float depth_tol, int32_t* counts, void* stream) {
  if (n_vertices < 0 || n_vertices >= (int64_t)1 << 31) return fail("mesh_view_votes: n_vertices must lie in [0, 2^31) (got %lld)", (long long)n_vertices);
  if (cull_image_sizes("mesh_view_votes", n_views, H, W)) return -1;
  if (n_views == 0 || n_vertices == 0) return 0;
  if (!vertices || !c2w || !focal || !counts) return fail("mesh_view_votes: null argument");
  if (reinterpret_cast<uintptr_t>(mask_bits) % 8 != 0) return fail("mesh_view_votes: mask_bits must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(counts) % 16 != 0) return fail("mesh_view_votes: counts must be 16-byte aligned (a vertex's row is one access)");
  MeshViewVotes p;
  p.vertices = vertices; p.V = (long)n_vertices; p.c2w = c2w; p.focal = focal; p.origin = origin; p.radius = radius; p.z_near = z_near;
  p.opengl = opengl; p.n_views = (long)n_views; p.H = H; p.W = W; p.Wq = (W + 63) / 64;
  p.mask_bits = reinterpret_cast<const unsigned long long*>(mask_bits); p.depth = depth; p.depth_tol = depth_tol; p.counts = counts;
  be_mesh_view_votes(p, (cnr_stream)stream);
  return check_backend("mesh_view_votes");
}

int cnr_mesh_cull_select(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, const int32_t* counts, int32_t min_views,
                         int32_t max_outside, int32_t min_visible, int32_t face_rule, uint8_t* keep_vertex, uint8_t* keep_face, int32_t* vertex_map,
                         int32_t* face_map, int32_t* totals, int32_t* dropped, void* stream) {
  if (mesh_sizes("mesh_cull_select", n_triangles, n_vertices)) return -1;
  if (face_rule != CNR_CULL_FACE_ALL && face_rule != CNR_CULL_FACE_ANY) return fail("mesh_cull_select: face_rule must be 0 (all) or 1 (any), got %d", face_rule);
  if (min_views < 0 || max_outside < 0 || min_visible < 0)
    return fail("mesh_cull_select: min_views, max_outside and min_visible must not be negative (got %d, %d, %d)", min_views, max_outside, min_visible);
  if ((n_triangles > 0 && (!triangles || !keep_face || !face_map)) || (n_vertices > 0 && (!counts || !keep_vertex || !vertex_map)) || !totals || !dropped)
    return fail("mesh_cull_select: null argument");
  MeshCullSelect p;
  p.triangles = triangles; p.F = (long)n_triangles; p.V = (long)n_vertices; p.counts = counts;
  p.min_views = min_views; p.max_outside = max_outside; p.min_visible = min_visible; p.face_rule = face_rule;
  p.keep_vertex = keep_vertex; p.keep_face = keep_face; p.vertex_map = vertex_map; p.face_map = face_map; p.totals = totals; p.dropped = dropped;
  be_mesh_cull_select(p, (cnr_stream)stream);
  return check_backend("mesh_cull_select");
}

// ICP: `iterations` times move, search, moments and solve on the stream; the transform stays on the device between them
int cnr_icp(const float* source, int64_t n_source, const float* target, int64_t n_target, const int32_t* triangles, int64_t n_triangles,
            const double* pivots, int32_t with_scale, float max_dist2, int32_t iterations, int32_t resume, double* transform, double* history,
            float* moved, float* matched, float* dist2, int32_t* idx, uint64_t* keys, double* partials, void* stream) {
  const int64_t lim = (int64_t)1 << 31;
  if (n_source < 0 || n_source >= lim) return fail("icp: n_source must be in [0, 2^31) (got %lld)", (long long)n_source);
  if (n_target < 1 || n_target >= lim) return fail("icp: n_target must be in [1, 2^31) (got %lld)", (long long)n_target);
  if (n_triangles < 0 || n_triangles >= lim) return fail("icp: n_triangles must be in [0, 2^31) (got %lld)", (long long)n_triangles);
  if ((triangles == nullptr) != (n_triangles == 0)) return fail("icp: triangles must be null exactly when n_triangles == 0 (a cloud target)");
  if (iterations < 0) return fail("icp: iterations < 0");
  if (!(max_dist2 >= 0.0f)) return fail("icp: max_dist2 must not be NaN or negative (+inf: no gate)");
  if (n_source == 0 || iterations == 0) return 0;
  if (!source || !target || !pivots || !transform || !history || !moved || !matched || !dist2 || !idx || !keys || !partials)
    return fail("icp: null argument");
  if (reinterpret_cast<uintptr_t>(transform) % 8 != 0 || reinterpret_cast<uintptr_t>(history) % 8 != 0 ||
      reinterpret_cast<uintptr_t>(keys) % 8 != 0 || reinterpret_cast<uintptr_t>(partials) % 8 != 0)
    return fail("icp: transform, history, keys and partials must be 8-byte aligned");
  IcpStep p;
  p.source = source; p.n = (long)n_source; p.target = target; p.m = (long)n_target; p.triangles = triangles; p.F = (long)n_triangles;
  for (int r = 0; r < 3; ++r) { p.c_src[r] = pivots[r]; p.c_tgt[r] = pivots[3 + r]; }
  p.with_scale = with_scale != 0; p.max_dist2 = max_dist2; p.transform = transform;
  p.moved = moved; p.matched = matched; p.dist2 = dist2; p.idx = idx; p.keys = reinterpret_cast<unsigned long long*>(keys); p.partials = partials;
  be_icp_clear(history, (size_t)iterations * 4 * sizeof(double), (cnr_stream)stream);
  for (int k = 0; k < iterations; ++k) {
    p.first = k == 0 && resume == 0;
    p.history = history + (size_t)k * 4;
    be_icp_step(p, (cnr_stream)stream);
  }
  return check_backend("icp");
}

}  // extern "C"
