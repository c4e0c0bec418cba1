/* colorneus_render.h -- C ABI of the MI355X-native Color-NeuS volume renderer (libcolorneus_hip.so).
 *
 * The reference (Colmar-zlicheng/Color-NeuS) is pure Python and has no FFI boundary of its own; its plug-in
 * interface for this path is the RENDERER registry class whose forward() is
 *     NeuS.forward(rays_o, rays_d, near, far, perturb_overwrite=-1, background_rgb=None, cos_anneal_ratio=0.0)
 *                                                              (lib/models/renderers/NeuS.py:294-408)
 * with Color_NeuS.render_core (lib/models/renderers/Color_NeuS.py:24-138) underneath, plus
 *     NeuS.extract_geometry / extract_fields   (NeuS.py:14-40, 410-417)   -> cnr_sdf_grid / cnr_sdf_eval
 *     NeuS.extract_color                       (NeuS.py:44-64, 419-420)   -> cnr_vertex_color
 * The entry points below are what a ctypes / cffi binding of that class calls.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless stated otherwise; the caller owns all memory
 *     (outputs, context, scratch); the library allocates nothing.  No RESULT depends on state kept between calls; what the
 *     process does keep: the first-error latch behind cnr_last_error(), the optional timing records (cnr_timing_enable), debug
 *     switches read once from the environment (CNR_*), the per-(kernel, device) "dynamic LDS opt-in applied" flags, and an
 *     atomic launch counter whose parity only picks the order in which a layer launch walks its tiles (speed, never a value)
 *   - alignment: the render, evaluation (sdf_eval, sdf_grid, vertex_color), point-query, linear and background-network
 *     entry points place sub-buffers at multiples of 256 bytes from the address of their `void* ctx` / `void* scratch`
 *     and access them with 16-byte vector loads / stores and 8-byte atomics: that address must be a multiple of 16 bytes,
 *     and these entry points refuse one that is not ("... misaligned: its address must be a multiple of 16 bytes")
 *     before anything is launched.  The other entry points with a scratch buffer (loss, clip_adam, pixel table, mc, nn,
 *     image, mesh raster, composite_background, gen_rays_backward) do not check its address: give them, like every
 *     buffer, what hipMalloc gives (256-byte aligned)
 *   - all work is enqueued on the given hipStream_t (passed as void*); no internal synchronisation
 *   - return value: 0 on success, negative on error; cnr_last_error() returns a message for the calling thread
 *   - parameters are passed as an array of device pointers in the canonical order reported by cnr_param_info()
 *     (names are the reference's state_dict names, e.g. "sdf_network.lin0.weight_v")
 */
#ifndef COLORNEUS_RENDER_H_
#define COLORNEUS_RENDER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNR_ABI_VERSION 9

typedef struct cnr_config {
  int32_t type;              /* 0 = NeuS (NeuS.py:68), 1 = Color_NeuS (Color_NeuS.py:10) */
  int32_t n_samples;         /* N_SAMPLES      (NeuS.py:80) */
  int32_t n_importance;      /* N_IMPORTANCE   (NeuS.py:81) */
  int32_t up_sample_steps;   /* UP_SAMPLE_STEPS(NeuS.py:83) */
  /* SDFNetwork (fields.py:19-29) */
  int32_t sdf_d_hidden, sdf_n_layers, sdf_d_out, sdf_multires, sdf_skip_mask /* bit l set <=> l in SKIP_IN */, sdf_weight_norm;
  float sdf_scale;
  /* RenderingNetwork (fields.py:126-134): mode 0 = idr, 1 = no_view_dir, 2 = no_normal */
  int32_t col_mode, col_d_feature, col_d_hidden, col_n_layers, col_multires_view, col_weight_norm, col_squeeze_out;
  /* RelightNetwork (fields.py:296-303), ignored when type == 0 */
  int32_t rel_d_hidden, rel_n_layers, rel_y_in_layer, rel_multires_view, rel_include_grad, rel_inv_sigmoid;
} cnr_config;

typedef struct cnr_render_inputs {
  const float* rays_o;          /* [R][3] */
  const float* rays_d;          /* [R][3] */
  const float* near_;           /* [R]    */
  const float* far_;            /* [R]    */
  const float* t_rand;          /* [R] uniform [0,1) jitter draw (the reference's torch.rand([R,1]), NeuS.py:325) or NULL = no perturb */
  const float* z_vals_override; /* [R][M] or NULL: skip the sampler and render at these z (parity gate G2) */
  const float* background_rgb;  /* [3] or NULL */
  int64_t n_rays;               /* > 0 (an empty batch is the host layer's business: renderer.py renders it like the reference, as empty
                                   outputs with zero gradients; the entry points reject n_rays <= 0 with an error) */
  float cos_anneal_ratio;
  float prune_eps;              /* > 0: INFERENCE ONLY early-termination compaction -- the colour / relight networks run only on samples
                                   whose compositing weight is >= prune_eps (pixel error < prune_eps per skipped sample); per-sample
                                   colour outputs of skipped samples are zero and cnr_render_backward must not be called */
} cnr_render_inputs;

/* the reference's return dict (NeuS.py:387-408) plus the final z_vals; M = n_samples + n_importance */
typedef struct cnr_render_outputs {
  float* color_fine;     /* [R][3]    */
  float* s_val;          /* [R]       */
  float* cdf_fine;       /* [R][M]    */
  float* weight_sum;     /* [R]       */
  float* weight_max;     /* [R]       */
  float* gradients;      /* [R][M][3] or NULL (the library then keeps them in its context buffer; see delta_relight_ray_sum) */
  float* weights;        /* [R][M]    */
  float* gradient_error; /* [1]       */
  float* inside_sphere;  /* [R][M]    */
  float* depth;          /* [R]       */
  float* global_color;   /* [R][3]    (Color_NeuS only, else NULL) */
  float* delta_relight;  /* [R][M][3] (Color_NeuS only, else NULL); may also be NULL for Color_NeuS when only delta_relight_ray_sum is wanted */
  float* z_vals;         /* [R][M]    */
  float* eik_sums;       /* [2] or NULL: {sum relax*(|g|-1)^2, sum relax} of this call's rays -- lets a ray-sharded run rebuild the global eikonal ratio */
  /* optional per-sample network outputs, for callers that do their own alpha / compositing (the N_OUTSIDE > 0 background mixing of
     NeuS.py:262-268 / Color_NeuS.py:97-102 runs above the ABI): */
  float* sdf_samples;           /* [R][M]    or NULL: sdf at the section midpoints */
  float* color_samples;         /* [R][M][3] or NULL: the colour that is composited (relit colour for Color_NeuS) */
  float* global_color_samples;  /* [R][M][3] or NULL: colour-network output before relighting (Color_NeuS only) */
  /* "loss only" training outputs: compute_loss (NeuS_Trainer.py:129-171) consumes `gradients` only through
     gradient_error and `delta_relight` only through mean(delta_relight * mask) -- with this per-ray sum the two [R][M][3] dict tensors
     need not be materialised for the caller (pass gradients = delta_relight = NULL): */
  float* delta_relight_ray_sum; /* [R] or NULL: sum over the samples and rgb of delta_relight of each ray (Color_NeuS only) */
} cnr_render_outputs;

/* upstream gradients of the outputs; any member may be NULL (= zero) */
typedef struct cnr_render_out_grads {
  const float* color_fine; const float* s_val; const float* cdf_fine; const float* weight_sum; const float* weight_max;
  const float* gradients; const float* weights; const float* gradient_error; const float* depth;
  const float* global_color; const float* delta_relight;
  const float* sdf_samples; const float* color_samples; const float* global_color_samples;   /* gradients of the per-sample outputs, or NULL */
  const float* delta_relight_per_ray;   /* [R] or NULL: the gradient of delta_relight when it is constant along a ray and over rgb -- the
                                           relight term of the training loss, mean(delta_relight * mask)^2 (NeuS_Trainer.py:153), yields
                                           exactly that; lets the loss seed the backward pass without an [R][M][3] buffer.  Added to
                                           delta_relight when both are given. */
} cnr_render_out_grads;

typedef struct cnr_render_in_grads {
  float* const* d_params;   /* host array of device pointers, same order/shapes as the parameters; overwritten (not accumulated) */
  float* d_rays_o;          /* [R][3] or NULL */
  float* d_rays_d;          /* [R][3] or NULL */
  float* d_near;            /* [R] or NULL; with d_far.  Non-zero only when n_importance == 0 and no z override: z is then an affine   */
  float* d_far;             /* function of near / far (NeuS.py:311-313); with importance sampling z is built under no_grad (:343)     */
} cnr_render_in_grads;

/* optional per-launch timing (HIP events on the launch stream); used by bench.py for the roofline figures */
typedef struct cnr_kernel_timing {
  char name[32];
  int32_t kind;     /* 0 = layer GEMM, 1 = weight-gradient GEMM, 2 = other */
  int32_t nt;       /* tile variant */
  int64_t P;        /* points (rows) or rays */
  int32_t N, K, pairs;
  float ms;
  double bytes;     /* algorithmic HBM bytes of the launch (operands read once + outputs written once); 0 = not modelled */
} cnr_kernel_timing;
void cnr_timing_enable(int on);
int cnr_timing_collect(cnr_kernel_timing* out, int max_records);

/* ---- loss of the training step (replaces NeuS_Trainer.compute_loss, NeuS_Trainer.py:129-171, the consumer right after the path) ----
 * loss = lambda_fine * mean((color_fine - rgb_gt)^2 or |.|) + lambda_eikonal * gradient_error
 *      + lambda_mask * BCE(clip(weight_sum, 1e-3, 1 - 1e-3), mask) + lambda_relight * mean(delta_relight * mask)^2
 * Two phases so that a ray-sharded run can all-reduce the three sums in between:
 *   cnr_loss_sums : sums[0] = sum of squared (or absolute) colour errors, sums[1] = sum of the BCE terms, sums[2] = sum of
 *                   delta_relight (* mask); fixed-order reductions.
 *   cnr_loss_grads: d_color_fine = coef[0] * (c - gt) (or sign), d_weight_sum = coef[1] * dBCE/dws, d_delta_relight = coef[2] (* mask);
 *                   the caller folds lambda, 1/N and the upstream gradient into the three device-side coefficients. */
typedef struct cnr_loss_config {
  float lambda_fine, lambda_eikonal, lambda_mask, lambda_relight;
  int32_t rgb_l1;        /* 0: MSE (RGB_LOSS_TYPE "mse"), 1: L1 */
  int32_t include_mask;  /* relight term uses delta_relight * mask */
} cnr_loss_config;
size_t cnr_loss_scratch_bytes(int64_t n_rays);
int cnr_loss_sums(const cnr_loss_config* cfg, const float* color_fine, const float* weight_sum, const float* delta_relight /* or NULL */,
                  const float* rgb_gt, const float* mask /* [R] or NULL */, int64_t n_rays, int32_t n_samples, float* sums /* device [4] */,
                  void* scratch, size_t scratch_bytes, void* stream);
/* cnr_loss_sums with the relight term given as the per-ray sums cnr_render_outputs.delta_relight_ray_sum [R] instead of [R][M][3] */
int cnr_loss_sums_ray(const cnr_loss_config* cfg, const float* color_fine, const float* weight_sum, const float* delta_relight_ray_sum,
                      const float* rgb_gt, const float* mask, int64_t n_rays, int32_t n_samples, float* sums, void* scratch, size_t scratch_bytes,
                      void* stream);
int cnr_loss_grads(const cnr_loss_config* cfg, const float* color_fine, const float* weight_sum, const float* rgb_gt, const float* mask,
                   int64_t n_rays, int32_t n_samples, const float* coef /* device [4] */, float* d_color_fine, float* d_weight_sum,
                   float* d_delta_relight /* or NULL */, void* stream);
/* The scalar arithmetic around the two phases on the device, one launch each (single-process runs; a ray-sharded run all-reduces the sums
 * in between and keeps these few operations in the host language).  fp32, the operation order of NeuS_Trainer.compute_loss:
 *   cnr_loss_combine: out[1] = rgb = sums[0] / (3 Rg); out[2] = eikonal = gradient_error[0]; out[3] = mask = sums[1] / Rg (0 unless use_mask);
 *                     out[5] = mean_rel = sums[2] / (3 Rg M); out[4] = relight = mean_rel^2 (0 unless use_relight);
 *                     out[0] = loss = lambda_fine * rgb + lambda_eikonal * eikonal (+ lambda_mask * mask) (+ lambda_relight * relight)
 *   cnr_loss_coef:    the coefficients of cnr_loss_grads from the upstream gradient g = g_loss[0]:
 *                     coef[0] = g * lambda_fine * (1 for L1, 2 for MSE) / (3 Rg); coef[1] = g * lambda_mask / Rg (0 unless use_mask);
 *                     coef[2] = g * lambda_relight * 2 / (3 Rg M) * mean_rel[0] (0 unless use_relight); coef[3] = g * lambda_eikonal = d loss / d gradient_error */
int cnr_loss_combine(const cnr_loss_config* cfg, const float* sums /* device [4] */, const float* gradient_error /* device [1] */,
                     float n_rays_global, int32_t n_samples, int32_t use_mask, int32_t use_relight, float* out /* device [6] */, void* stream);
int cnr_loss_coef(const cnr_loss_config* cfg, const float* g_loss /* device [1] */, const float* mean_rel /* device [1] */,
                  float n_rays_global, int32_t n_samples, int32_t use_mask, int32_t use_relight, float* coef /* device [4] */, void* stream);

/* The same two sides as ONE launch each (single process; replaces NeuS_Trainer.compute_loss, NeuS_Trainer.py:129-171, and its autograd graph):
 *   cnr_loss_forward : cnr_loss_sums (delta_per_ray == 0: delta_relight is [R][M][3]; != 0: the per-ray sums [R]) + cnr_loss_combine; the block that
 *                      finishes last folds the partial sums in the fixed order of cnr_loss_sums -- bitwise the same sums and scalars.  Its completion
 *                      counter is the 4 bytes at offset cnr_loss_scratch_bytes() - 16 of the CALLER's scratch: zero before the first call that uses
 *                      the buffer, left zero by every call.  So is the rest of the buffer: the folding block clears the partial sums it has read,
 *                      and a scratch that was all zero before a call is all zero after it.  A buffer may be reused call after call on one
 *                      stream; calls that may overlap (other streams or threads) need buffers of their own.  cnr_loss_sums / cnr_loss_sums_ray
 *                      never touch the counter.
 *   cnr_loss_backward: cnr_loss_coef (also written to coef[4] for the caller: coef[2] * mask is d / d delta_relight, coef[3] is d / d gradient_error)
 *                      + cnr_loss_grads for d_color_fine / d_weight_sum.  eik_factor (device [1] or NULL = 1): coef[3] = g * lambda_eikonal * eik_factor
 *                      (ray-sharded runs, below). */
int cnr_loss_forward(const cnr_loss_config* cfg, const float* color_fine, const float* weight_sum, const float* delta_relight /* or NULL */, int32_t delta_per_ray,
                     const float* rgb_gt, const float* mask /* or NULL */, const float* gradient_error /* device [1] */, int64_t n_rays, int32_t n_samples,
                     float n_rays_global, int32_t use_mask, int32_t use_relight, float* sums /* device [4] */, float* out /* device [6] */,
                     void* scratch, size_t scratch_bytes, void* stream);
int cnr_loss_backward(const cnr_loss_config* cfg, const float* color_fine, const float* weight_sum, const float* rgb_gt, const float* mask /* or NULL */,
                      int64_t n_rays, int32_t n_samples, const float* g_loss /* device [1] */, const float* mean_rel /* device [1] */,
                      const float* eik_factor /* device [1] or NULL */, float n_rays_global, int32_t use_mask, int32_t use_relight,
                      float* coef /* device [4] */, float* d_color_fine, float* d_weight_sum /* or NULL */,
                      float* d_delta_relight_per_ray /* [R] or NULL: coef[2] (* mask[r]), what cnr_render_out_grads.delta_relight_per_ray takes */, void* stream);

/* Ray-sharded runs (one process per GPU, the rays of a batch split over the ranks; the reference is single-GPU, train.py:111): the eikonal term is a
 * ratio of sums over ALL rays (Color_NeuS.py:122-123) and the relight term the square of a mean over ALL samples (NeuS_Trainer.py:153), so the
 * objective needs ONE exchange between the two sides.  Three launches around one 5-float all-reduce (the caller's: RCCL):
 *   cnr_loss_shard_stats  : one launch (the fold by the last block, as cnr_loss_forward; same scratch contract): stats[0..2] = the three sums of
 *                           cnr_loss_sums over this rank's rays, stats[3..4] = eik_sums of this rank (cnr_render_outputs.eik_sums),
 *                           stats[5] = stats[4] again (the rank's own value survives the all-reduce there), stats[6..7] = 0
 *   caller                : all-reduce(sum) of stats[0..5) over the ranks
 *   cnr_loss_shard_combine: out[0..5] as cnr_loss_combine with eikonal = stats[3] / (stats[4] + 1e-5), the GLOBAL loss on every rank;
 *                           out[6] = eik_factor = (stats[5] + 1e-5) / (stats[4] + 1e-5) = d eikonal / d (this rank's gradient_error output); out[7] = 0
 *   cnr_loss_backward     : with n_rays_global, mean_rel = out + 5 and eik_factor = out + 6: the rank-local gradients whose sum over the ranks is the
 *                           single-GPU gradient. */
int cnr_loss_shard_stats(const cnr_loss_config* cfg, const float* color_fine, const float* weight_sum, const float* delta_relight /* or NULL */,
                         int32_t delta_per_ray, const float* rgb_gt, const float* mask /* or NULL */, const float* eik_sums /* device [2] */, int64_t n_rays,
                         int32_t n_samples, float* stats /* device [8] */, void* scratch, size_t scratch_bytes, void* stream);
int cnr_loss_shard_combine(const cnr_loss_config* cfg, const float* stats /* device [8] */, float n_rays_global, int32_t n_samples, int32_t use_mask,
                           int32_t use_relight, float* out /* device [8] */, void* stream);

/* ---- ray generation for the selected pixels, the producer right in front of the path (NeuS_Trainer.render, NeuS_Trainer.py:104-120):
 * get_rays_multicam / get_rays_at (lib/models/tools/ray_utils.py:16-119) evaluated ONLY for the chosen pixels (the reference builds the
 * rays of all N*H*W pixels and gathers), with the trainer's (rays_o - origin) / radius normalisation and near_far_from_sphere
 * (ray_utils.py:7-13) folded in.  pix_idx: device int64 [n], flat index cam*H*W + row*W + col (NULL: pixel i of camera 0, i.e.
 * get_rays_at over a whole H x W image when n = H*W); c2w [n_cams][4][4]; focal device [2]; image [n_cams][H][W][3] / mask
 * [n_cams][H][W] may be NULL together with rgb / mask_sel; origin (device [3]) may be NULL; near_ / far_ may be NULL.
 * cnr_gen_rays_backward: d c2w [n_cams][4][4] and d focal [2] from d rays_o, d rays_d (and d near / d far when given) for learnable
 * poses / focal (config/Color_NeuS_iho.yml:18-20); scratch: n_cams * 2 floats. */
int cnr_gen_rays(const int64_t* pix_idx, int64_t n, const float* c2w, int32_t n_cams, const float* focal, int32_t H, int32_t W,
                 int32_t normalize, int32_t opengl, const float* image, const float* mask, const float* origin, float radius,
                 float* rays_o, float* rays_d, float* rgb, float* mask_sel, float* near_, float* far_,
                 int32_t* bad_index_count /* ABI 8; device or NULL: incremented once per index outside [0, n_cams*H*W) -- such a ray's outputs are NaN (the
                                             reference's torch indexing raises; the caller reads the counter at its next synchronisation point and raises) */,
                 void* stream);
int cnr_gen_rays_backward(const int64_t* pix_idx, int64_t n, const float* c2w, int32_t n_cams, const float* focal, int32_t H, int32_t W,
                          int32_t normalize, int32_t opengl, const float* origin, float radius, const float* d_rays_o, const float* d_rays_d,
                          const float* d_near, const float* d_far, float* d_c2w, float* d_focal, void* scratch, size_t scratch_bytes, void* stream);

/* ---- on-device pixel choice, the producer in front of cnr_gen_rays: the sampling SEMANTICS of get_rays_multicam's pixel choice
 * (lib/models/tools/ray_utils.py:57-76: a share of the batch from the foreground pixels and the rest from the background, both without
 * replacement, the result shuffled) on a counter-based random stream of its own -- NOT torch's CPU stream (that route stays in the host
 * layer and stays the default).  No host synchronisation, no allocation, capturable in a HIP graph, and a pure function of
 * (seed, step, table, arguments): every rank of a ray-sharded run draws the same batch without communicating.  Everything below is
 * integer-exact (the jitter is an exact dyadic float), so the specification can be restated and compared bitwise.
 *
 * Random primitive: Philox4x32-10 (Salmon et al. 2011).  Counter (c0, c1, c2, c3), key (k0, k1), all uint32; ten times
 *     (c0, c1, c2, c3) <- (hi(0xCD9E8D57 * c2) ^ c1 ^ k0,  lo(0xCD9E8D57 * c2),  hi(0xD2511F53 * c0) ^ c3 ^ k1,  lo(0xD2511F53 * c0))
 *   (hi / lo: the halves of the 64-bit product), with (k0, k1) += (0x9E3779B9, 0xBB67AE85) between rounds (nine times).  Known answers:
 *     counter 0,0,0,0 key 0,0                                                 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *     counter and key all ffffffff                                            -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *     counter 243f6a88 85a308d3 13198a2e 03707344 key a4093822 299f31d0       -> d16cfe09 94fdcceb 5001e420 24126ea1
 * State: device int64 state[2] = {seed, step}.  Key = (seed & 0xffffffff, (seed >> 32) & 0xffffffff); counter word 3 = step & 0xffffffff;
 *   counter word 2 = the stream id: 0 image choice, 1 foreground, 2 background, 3 shuffle, 4 draws with replacement, 5 jitter.
 *   philox(a, b, s) below is Philox4x32-10 of the counter (a, b, s, step & 0xffffffff) under that key; [i] is its output word i.
 * Keyed bijection perm(j, D, s) of [0, D), D < 2^32, j < D:  D <= 1: 0.  Otherwise bits = bit_length(D - 1), h = (bits + 1) / 2 (integer
 *   division), m = 2^h - 1, x = j; repeat { L = x >> h, R = x & m; for r = 0 .. 7: (L, R) <- (R, L ^ (philox(R, r, s)[0] & m)); x = (L << h) | R }
 *   until x < D (cycle walking on an 8-round Feistel network over 2h bits: the network permutes [0, 2^2h) and 2^2h < 4 D, so the walk ends
 *   and takes fewer than 4 rounds of the loop on average).  A bijection and not rejection of repeated draws: every draw is a function of its
 *   own index alone -- O(1) work per draw whatever the share of the domain that is drawn (want_fg >= F returns every foreground pixel), no
 *   shared state between the threads of the launch, no dependence on the launch shape.  (Four Feistel rounds are measurably non-uniform on small domains: the joint table of perm on D = 5
 *   / D = 7 over 3000 steps had chi^2 126 / 174 at 16 / 36 degrees of freedom; eight rounds 19.8 / 47.6.)
 *
 * Pixel table (cnr_pixel_table_build) of a mask stack masks [n_images][pixels_per_image] (float32): per image, order [n_images][pixels_per_image]
 *   (int32) holds the pixel indices with mask > 0 in ascending order, then those with mask == 0 in ascending order; fg_count / bg_count
 *   [n_images] their numbers.  A pixel that is neither (negative, NaN) is in neither list; the tail of its image's row of `order` is not
 *   written.  Three launches: per-tile counts (wavefront ballot + popcount), a per-image exclusive scan of the tile counts, a stable scatter;
 *   the mask is read twice, nothing is allocated.  scratch: cnr_pixel_table_scratch_bytes, contents need not be initialised.
 *   n_images * pixels_per_image < 2^32, pixels_per_image < 2^31.
 *
 * Draw (cnr_choose_pixels): n pixel indices idx [n] (int64), GLOBAL over the table's images: cam * pixels_per_image + pixel -- they pair with
 *   cnr_gen_rays given the c2w / image / mask stacks of all n_images.
 *   images    B = images_per_step slots, 1 <= B <= min(n_images, 1024).  cam_ids (device int32 [B]) names the image of each slot; with
 *             cam_ids == NULL slot b is image perm(b, n_images, 0) (B == n_images: a permutation of all images).  A cam_ids entry outside
 *             [0, n_images) makes an empty slot.
 *   want_fg   the number of foreground draws wanted: the host value, or, when want_fg_dev != NULL, the device int32 it points at (as
 *             cnr_adam_config.hyper_dev: a captured launch follows a schedule); clamped to [0, n] on the device.
 *   With a table (order, fg_count, bg_count given): F / G = the sums of fg_count / bg_count over the B slots in slot order, k = min(want_fg, F),
 *             m = n - k.  Foreground draw j < k has rank perm(j, F, 1); the rank maps to (slot, offset) by upper bound in the slot-order
 *             inclusive prefix of fg_count (the first slot whose prefix exceeds the rank; offset = rank - the prefix before that slot); its
 *             pixel is order[cam][offset].  Background draw j < min(m, G): rank perm(j, G, 2), prefix of bg_count, pixel
 *             order[cam][fg_count[cam] + offset].  A draw that cannot be served (j >= G) is -1: cnr_gen_rays makes that ray NaN and counts it.
 *             The list (foreground draws, then background draws) is written shuffled: idx[perm(j, n, 3)] = list[j].
 *             counts_out [2] = {k, min(m, G)}.
 *   Without a table (all three NULL; want_fg must be 0 and want_fg_dev NULL): n draws WITH replacement, idx[j] = the upper 64 bits of the
 *             128-bit product ((w[0] << 32) | w[1]) * span, w = philox(j, 0, 4); span = the argument, or pixels_per_image when it is 0 (the
 *             reference's unmasked draws never leave camera 0, ray_utils.py:58), at most n_images * pixels_per_image.  counts_out = {0, 0}.
 *   cams_out  [B] (or NULL): the image of every slot.
 *   t_rand    [n] (or NULL): the renderer's per-ray jitter draw, t_rand[j] = (philox(j, 0, 5)[0] >> 8) * 2^-24, in [0, 1).
 *   state     after the draw state[1] (the step, all 64 bits) is advanced by one, by the same launch behind a workgroup barrier: stream-ordered and part
 *             of whatever graph captured the call.  One launch of one workgroup: O(n + B) work. */
size_t cnr_pixel_table_scratch_bytes(int32_t n_images, int64_t pixels_per_image);
int cnr_pixel_table_build(const float* masks /* [n_images][pixels_per_image] */, int32_t n_images, int64_t pixels_per_image,
                          int32_t* order /* [n_images][pixels_per_image] */, int32_t* fg_count /* [n_images] */, int32_t* bg_count /* [n_images] */,
                          void* scratch, size_t scratch_bytes, void* stream);
int cnr_choose_pixels(int64_t* state /* device [2] */, int64_t n, int32_t want_fg, const int32_t* want_fg_dev /* device [1] or NULL */,
                      const int32_t* cam_ids /* device [B] or NULL */, int32_t images_per_step, int32_t n_images, int64_t pixels_per_image,
                      const int32_t* order, const int32_t* fg_count, const int32_t* bg_count, int64_t span /* 0: pixels_per_image */,
                      int64_t* idx /* [n] */, int32_t* cams_out /* [B] or NULL */, int32_t* counts_out /* [2] or NULL */,
                      float* t_rand /* [n] or NULL */, void* stream);

/* ---- learnable cameras, the producer in front of cnr_gen_rays: the reference's Focal_Net and Pose_Net (lib/models/tools/camera_net.py:8-109,
 * called at the top of every training step, NeuS_Trainer.py:183-184) and their backward, one launch each.  All arithmetic fp32.
 *   focal [2]: order 2: {(fx*fx)*W, (fy*fy)*H}; order 1: {fx*W, fy*H}; with fx_only both entries are the first one (fy is not read, may be NULL).
 *   c2w [B][4][4]: slot i takes camera cam = cam_ids[i] (device int64; duplicates allowed, any order; NULL: camera i, B == num_cams):
 *     c2w[i] = [[R, t[cam]], [0 0 0 1]] @ init_c2w[cam]   (the full 4x4 product), or without the product when init_c2w is NULL; R from r[cam]:
 *       CNR_POSE_6D, r [num_cams][6] (Zhou et al. 2019): b1 = a1 / max(|a1|, 1e-12), b2' = a2 - (b1 . a2) b1, b2 = b2' / max(|b2'|, 1e-12),
 *         b3 = b1 x b2 with a1 = r[0:3], a2 = r[3:6]; the ROWS of R are b1, b2, b3;
 *       CNR_POSE_3D, r [num_cams][3] (axis-angle): R = I + A K + B K^2, K = [r]x, theta = |r|, A = sin(theta) / theta,
 *         B = 2 sin^2(theta / 2) / theta^2; for theta^2 < 1e-4 the series A = 1 - theta^2 / 6, B = 1/2 - theta^2 / 24 (R = I and
 *         dR/dr_k = [e_k]x at r = 0, the initial value).
 *     A slot whose id is outside [0, num_cams) reads nothing: its c2w is NaN and it contributes nothing to the backward (the convention of
 *     cnr_gen_rays for pixel indices).
 * Either part may be left out: c2w == NULL (r, t, init_c2w, cam_ids, B, num_cams, pose_mode are then not used) or focal == NULL (fx, fy,
 * focal_order, fx_only, H, W are not used), not both.
 * cnr_camera_backward: from d_c2w [B][4][4] and d_focal [2] (either may be NULL like the output it belongs to) the DENSE gradients
 * d_r [num_cams][6 or 3], d_t [num_cams][3] and d_fx [1], d_fy [1]; each is overwritten; one that is not wanted may be NULL (d_fy is not
 * written with fx_only).  Rows of cameras no slot names are exactly 0; the slots of one camera are added in ascending slot order by one
 * thread (no float atomics: bitwise reproducible).  No scratch. */
#define CNR_POSE_3D 0
#define CNR_POSE_6D 1
typedef struct cnr_camera_config {
  int32_t num_cams;
  int32_t pose_mode;      /* CNR_POSE_3D / CNR_POSE_6D */
  int32_t focal_order;    /* 1 or 2 */
  int32_t fx_only;
  int32_t H, W;
  int32_t has_init_c2w;   /* must agree with init_c2w != NULL */
} cnr_camera_config;
int cnr_camera_forward(const cnr_camera_config* cfg, const float* r, const float* t, const float* init_c2w /* or NULL */, const float* fx,
                       const float* fy /* NULL with fx_only */, const int64_t* cam_ids /* [B] or NULL */, int64_t B, float* c2w, float* focal,
                       void* stream);
int cnr_camera_backward(const cnr_camera_config* cfg, const float* r, const float* t, const float* init_c2w, const float* fx, const float* fy,
                        const int64_t* cam_ids, int64_t B, const float* d_c2w, const float* d_focal, float* d_r, float* d_t, float* d_fx,
                        float* d_fy, void* stream);

/* ---- optimiser step of the training loop (the consumer after loss.backward(), train.py:72-77): per-parameter gradient clipping
 * (clip_gradient -> torch.nn.utils.clip_grad_norm_ on EACH parameter tensor, lib/utils/net_utils.py:174-184) followed by
 * torch.optim.Adam (net_utils.py:88: betas (0.9, 0.99), eps 1e-8, no weight decay) in ONE launch over all tensors.
 * params / grads: host arrays of n_tensors device pointers, sizes: host array of element counts; exp_avg / exp_avg_sq: device, flat,
 * sum(sizes) floats each, tensor i at offset sum(sizes[0..i)); step is 1-based; max_norm <= 0 disables the clip.
 * scratch: device, cnr_clip_adam_scratch_bytes(n_tensors, sizes) bytes (per-chunk partial sums of the gradient norms). */
typedef struct cnr_adam_config {
  float lr, beta1, beta2, eps, max_norm;
  int32_t step;
  const float* hyper_dev;   /* ABI 8; NULL, or DEVICE [3] = {lr, 1 - beta1^step, sqrt(1 - beta2^step)}: the step-dependent scalars read from device memory
                               instead of lr / step above, so that a launch sequence captured ONCE in a HIP graph (hipStreamBeginCapture; every entry point
                               only enqueues on the caller's stream and allocates nothing) can be replayed for every step -- the caller refreshes the three
                               floats before each replay (optim.ClipAdam(capturable=True).prepare_step) */
} cnr_adam_config;
size_t cnr_clip_adam_scratch_bytes(int32_t n_tensors, const int64_t* sizes);
int cnr_clip_adam_step(const cnr_adam_config* cfg, int32_t n_tensors, const int64_t* sizes, float* const* params, const float* const* grads,
                       float* exp_avg, float* exp_avg_sq, void* scratch, size_t scratch_bytes, void* stream);

int cnr_abi_version(void);
const char* cnr_backend_name(void);
const char* cnr_last_error(void);

/* parameter inventory in canonical order */
int cnr_param_count(const cnr_config* cfg);
int cnr_param_info(const cnr_config* cfg, int index, char* name, int name_len, int* rows, int* cols);

/* bytes of the context buffer (saved activations, written by forward, read by backward) and of the backward scratch */
size_t cnr_ctx_bytes(const cnr_config* cfg, int64_t n_rays);
size_t cnr_bwd_scratch_bytes(const cnr_config* cfg, int64_t n_rays);

/* renderer(rays_o, rays_d, near, far) -- NeuS.forward / Color_NeuS.render_core */
int cnr_render_forward(const cnr_config* cfg, const float* const* params, const cnr_render_inputs* in,
                       const cnr_render_outputs* out, void* ctx, size_t ctx_bytes, void* stream);

/* Forward-only render -- the inference use of the path: NeuS_Trainer.validate_image (NeuS_Trainer.py:236-245 consumes color_fine and depth of every
 * chunk) and evaluation.py.  Same inputs, same outputs, BIT-IDENTICAL values to cnr_render_forward (every value-producing launch is the same
 * kernel on the same operands), but nothing is written for cnr_render_backward: no row scales, no hidden activations of the colour / relight
 * stacks, two reused buffers instead of the saved V_l of the gradient chain.  `scratch` (cnr_infer_scratch_bytes, about half of
 * cnr_ctx_bytes: 14.1 GB against 29.7 GB for 8192 rays) holds no state after the call.  prune_eps > 0 (cnr_render_inputs): the colour / relight stacks run only on the samples
 * whose compositing weight is >= prune_eps -- per ray a wavefront ballot + popcount builds the index list, the chain-fused launch reads its
 * rows through it; the pixel error per skipped sample is < prune_eps, the per-sample colour outputs of skipped samples are zero. */
size_t cnr_infer_scratch_bytes(const cnr_config* cfg, int64_t n_rays);
int cnr_render_forward_only(const cnr_config* cfg, const float* const* params, const cnr_render_inputs* in, const cnr_render_outputs* out,
                            void* scratch, size_t scratch_bytes, void* stream);

/* the hierarchical sampler on its own (NeuS.forward up to the render_core call, NeuS.py:309-356): writes the final z_vals [R][M];
 * ctx is a buffer of cnr_ctx_bytes(cfg, n_rays) bytes used as scratch */
int cnr_sample_z(const cnr_config* cfg, const float* const* params, const cnr_render_inputs* in, float* z_vals, void* ctx, size_t ctx_bytes,
                 void* stream);

/* autograd backward of cnr_render_forward (loss.backward(), train.py:70): parameter gradients incl. the
 * second-order terms through grad_x SDF, and optionally d rays_o / d rays_d */
int cnr_render_backward(const cnr_config* cfg, const float* const* params, const cnr_render_inputs* in,
                        const cnr_render_outputs* out, const void* ctx, size_t ctx_bytes,
                        const cnr_render_out_grads* gout, const cnr_render_in_grads* gin,
                        void* scratch, size_t scratch_bytes, void* stream);

/* the two sampler functions on their own (the render call runs them inside the hierarchical sampler; these entry points expose the
 * same kernel so that its tie / flat-cdf / denom < 1e-5 semantics can be exercised directly):
 *   cnr_sample_pdf = ray_utils.sample_pdf(bins, weights, n_samples, det=True)            (lib/models/tools/ray_utils.py:123-154)
 *   cnr_up_sample  = NeuS.up_sample(rays_o, rays_d, z_vals, sdf, n_importance, inv_s)     (lib/models/renderers/NeuS.py:136-181)
 * n <= 256 bins / samples per ray, n_samples (n_importance) <= 64 */
int cnr_sample_pdf(const float* bins /* [R][n] */, const float* weights /* [R][n-1] */, int64_t n_rays, int32_t n, int32_t n_samples,
                   float* out /* [R][n_samples] */, void* stream);
/* ray_utils.sample_pdf(..., det=False) (ray_utils.py:135-136): the same inversion of the cdf at the caller's uniform draws u [R][n_samples] -- the
 * reference's torch.rand(list(cdf.shape[:-1]) + [n_samples]), taken by the host layer from the CPU generator exactly like the reference takes it.
 * Not on the render path (NeuS.up_sample calls det=True, NeuS.py:180); exported so that the function is complete. */
int cnr_sample_pdf_u(const float* bins, const float* weights, const float* u, int64_t n_rays, int32_t n, int32_t n_samples, float* out, void* stream);
int cnr_up_sample(const float* rays_o, const float* rays_d, const float* z_vals /* [R][n] */, const float* sdf /* [R][n] */, int64_t n_rays,
                  int32_t n, int32_t n_importance, float inv_s, float* out /* [R][n_importance] */, void* stream);

/* sdf_network.sdf(pts): out[i] = sign * sdf(pts[i]); extract_fields uses sign = -1 (NeuS.py:416).  Here and in cnr_sdf_grid* only the
 * sdf_network.* entries of params are read (the others may be NULL). */
size_t cnr_sdf_eval_scratch_bytes(const cnr_config* cfg, int64_t n_points);
int cnr_sdf_eval(const cnr_config* cfg, const float* const* params, const float* pts, int64_t n_points, float sign,
                 float* out, void* scratch, size_t scratch_bytes, void* stream);

/* ---- differentiable SDF point queries: sdf_network.forward / .sdf / .gradient (SDFNetwork, fields.py:81-115) at arbitrary points and their
 * backward, through the render path's SDF chains and its first- and second-order SDF backward (the fused layer + weight-gradient launches).
 *   forward : sdf[i] = h_top[0] / scale, feat[i][:] = h_top[1:] (F = sdf_d_out - 1), and with want_grad != 0 grad[i] = d sdf / d x in world
 *             coordinates; sdf is required, feat may be NULL, grad is given iff want_grad.  ctx (cnr_sdf_query_ctx_bytes) keeps what the
 *             backward reads; the backward only reads it, so it may run any number of times on one forward.
 *   backward: cotangents d_sdf [n], d_feat [n][F], d_grad [n][3] (each may be NULL = zero; d_grad only after a forward with want_grad) ->
 *             the gradients of the sdf_network.* entries of the canonical inventory in d_params (overwritten; the other entries are not
 *             touched and may be NULL; d_params == NULL: no weight-gradient launches at all) and d_pts [n][3] (or NULL), the total cotangent
 *             of the points: value path + the Hessian applied to d_grad.  want_grad = 1 needs a forward with want_grad = 1 (the forward tags the
 *             context; on a mismatch every output of the backward is NaN -- nothing synchronises, so it cannot be an error code); a
 *             want_grad = 0 backward takes either context.
 * params: the canonical inventory (cnr_param_info); only its sdf_network.* entries are read, the others may be NULL.  n_points > 0.
 * Internally the rows are padded to a multiple of 128 (padded rows at the origin with zero cotangents; nothing is written past row n of a
 * caller's buffer).  Without a cotangent on the gradient the second-order half of the backward is skipped. */
size_t cnr_sdf_query_ctx_bytes(const cnr_config* cfg, int64_t n_points, int32_t want_grad);
size_t cnr_sdf_query_bwd_scratch_bytes(const cnr_config* cfg, int64_t n_points, int32_t want_grad);
int cnr_sdf_query_forward(const cnr_config* cfg, const float* const* params, const float* pts /* [n][3] */, int64_t n_points, int32_t want_grad,
                          float* sdf /* [n] */, float* feat /* [n][F] or NULL */, float* grad /* [n][3] iff want_grad */, void* ctx, size_t ctx_bytes,
                          void* stream);
int cnr_sdf_query_backward(const cnr_config* cfg, const float* const* params, const float* pts /* the forward's points */, int64_t n_points,
                           int32_t want_grad, const float* d_sdf /* [n] or NULL */, const float* d_feat /* [n][F] or NULL */,
                           const float* d_grad /* [n][3] or NULL */, const void* ctx, size_t ctx_bytes, float* const* d_params /* or NULL */,
                           float* d_pts /* [n][3] or NULL */, void* scratch, size_t scratch_bytes, void* stream);

/* extract_fields: u[x][y][z] = -sdf on linspace(bmin,bmax,res)^3 (NeuS.py:14-28); bmin/bmax are HOST floats */
size_t cnr_sdf_grid_scratch_bytes(const cnr_config* cfg, int32_t resolution);
int cnr_sdf_grid(const cnr_config* cfg, const float* const* params, const float* bound_min, const float* bound_max,
                 int32_t resolution, float* u, void* scratch, size_t scratch_bytes, void* stream);
/* the slab x in [x_begin, x_end) of the same lattice (u_slab[x - x_begin][y][z], identical values): extract_fields sharded over the GPUs
 * of a node, one slab per rank, gathered by the caller (the reference walks the lattice in 64^3 blocks, NeuS.py:19-27) */
size_t cnr_sdf_grid_slab_scratch_bytes(const cnr_config* cfg, int32_t resolution, int32_t x_begin, int32_t x_end);
int cnr_sdf_grid_slab(const cnr_config* cfg, const float* const* params, const float* bound_min, const float* bound_max, int32_t resolution,
                      int32_t x_begin, int32_t x_end, float* u_slab, void* scratch, size_t scratch_bytes, void* stream);

/* extract_geometry's iso-surface step on the device-resident lattice (NeuS.py:31-40 calls the third-party CPU mcubes.marching_cubes on
 * a host copy of u): marching cubes over u[x][y][z] at `threshold`, "inside" = u > threshold, vertices on the lattice edges by linear
 * interpolation, shared between neighbouring cells, already mapped to world coordinates (v / (res - 1) * (bmax - bmin) + bmin,
 * NeuS.py:36-39), triangle normals pointing out of the u > threshold region.  Triangle table: built by tools/gen_mc_table.py
 * (no mcubes fixture exists: vertex / triangle ORDER and the resolution of ambiguous faces are this library's own; the surface is
 * the same piecewise-linear level set).
 * Two phases because the caller owns the output buffers: cnr_mc_count classifies, scans and leaves {n_vertices, n_triangles} in the
 * device int32 pair `totals`; after reading them the caller allocates and calls cnr_mc_emit with the same scratch. */
size_t cnr_mc_scratch_bytes(int32_t resolution);
int cnr_mc_count(const float* u, int32_t resolution, float threshold, void* scratch, size_t scratch_bytes, int32_t* totals, void* stream);
int cnr_mc_emit(const float* u, int32_t resolution, float threshold, const float* bound_min /* host [3] */, const float* bound_max /* host [3] */,
                void* scratch, size_t scratch_bytes, float* vertices /* [V][3] */, int32_t* triangles /* [F][3] */, void* stream);

/* Exact nearest neighbour of every query point among the target points: the search behind the Chamfer distance / F-score of two meshes
 * (lib/utils/mesh_tools.py:59-70 hands the vertices of two mesh files to pytorch3d.loss.chamfer_distance).  For query i,
 *     d2(i, j) = (dx*dx + dy*dy) + dz*dz,  dx = query[i].x - target[j].x, ...   every operation one rounded fp32 operation, in this order,
 * dist2[i] = min over j of d2(i, j), idx[i] = the lowest j that attains it.  A NaN d2 never wins; a query whose every d2 is NaN gets
 * idx = -1 and a NaN dist2.  Brute force over all n_query * n_target pairs, exact; results are bitwise reproducible (integer-min reduction).
 * n_query == 0 is a successful no-op; n_target must be in [1, 2^31).  scratch: cnr_nn_scratch_bytes, contents need not be initialised. */
size_t cnr_nn_scratch_bytes(int64_t n_query, int64_t n_target);
int cnr_nn_search(const float* query /* [n_query][3] */, int64_t n_query, const float* target /* [n_target][3] */, int64_t n_target,
                  float* dist2 /* [n_query] */, int32_t* idx /* [n_query] */, void* scratch, size_t scratch_bytes, void* stream);

/* ---- image evaluation: what NeuS_Trainer.validate_image does behind its render loop (NeuS_Trainer.py:250-277), on the device.
 * cnr_image_metrics: sums[0] = sum of the squared differences (PSNR, lib/metrics/similarity.py:24), sums[1] = sum of the SSIM map
 * (kornia.metrics.ssim(img0, img1, 3), similarity.py:55) over all n_images * channels * H * W elements, and optionally the map.
 * Every operation below is one rounded fp32 operation, in the order written (no FMA; `/` is the correctly rounded IEEE quotient):
 *   window   the normalised 3-tap Gaussian of sigma 1.5 as float32 torch evaluates it: w1 = 0x1.3b3046p-2 (outer taps), w0 = 0x1.899f76p-2
 *   border   reflection without repeating the edge: index -1 reads 1, index n reads n - 2 (hence H >= 2 and W >= 2)
 *   filt(p)  separable, rows first: h[r][c] = (w1*p[r][c-1] + w0*p[r][c]) + w1*p[r][c+1], then (w1*h[r-1][c] + w0*h[r][c]) + w1*h[r+1][c]
 *   per element, x = img0 and y = img1:
 *            mu1 = filt(x), mu2 = filt(y), e11 = filt(x*x), e22 = filt(y*y), e12 = filt(x*y)
 *            m11 = mu1*mu1, m22 = mu2*mu2, m12 = mu1*mu2, s1 = e11 - m11, s2 = e22 - m22, s12 = e12 - m12
 *            num = (2*m12 + 1e-4f) * (2*s12 + 9e-4f),  den = ((m11 + m22) + 1e-4f) * ((s1 + s2) + 9e-4f),  ssim = num / (den + 1e-12f)
 *            d = x - y, squared difference d*d
 *   Every [H][W] plane is filtered on its own: nothing reaches across channels or images.
 * This is kornia 0.6.9's ssim(img1, img2, window_size=3, max_val=1.0, eps=1e-12, padding="same") as its documentation states it.
 * Layout: channels_last == 0: [n_images][channels][H][W]; != 0: [n_images][H][W][channels] (at most 32 channels); ssim_map (or NULL) has the
 * inputs' layout.  The two sums are float64, added in a fixed order (per-block partials in scratch, then one block that adds those in index
 * order; no floating-point atomics): two calls give the same bits.  The HIP build and the CPU emulation order the float64 additions
 * differently; their totals agree to N * 2^-53 relative (N terms of magnitude <= 1).
 * n_images == 0 is a successful no-op that writes sums = {0, 0}.  Errors: H < 2 or W < 2, channels < 1, a null required pointer, scratch
 * too small, 2^31 or more elements.
 *
 * cnr_image_panel: the picture validate_image saves (NeuS_Trainer.py:250-263), uint8 [H][3W][3] = gt | render | depth, and
 * range = {vmin, vmax} of the depth.  With gt == render == NULL only the depth map is written, [H][W][3].
 *   colour   q = (uint8)(int)min(max(v * 255.0f, 0.0f), 255.0f): truncation, as rgb.mul(255.0).numpy().astype(np.uint8) (:252-256); NaN gives 0.
 *            The clamp is a deviation: numpy wraps values outside [0, 256).
 *   depth    viztools.cmap (lib/models/tools/viztools.py:145-162): vmin / vmax over the non-NaN depths ({0, 0} when there is none; exact and
 *            order-independent), t = (d - vmin) / (vmax - vmin), v = (int)(t * 255.0f) clamped to [0, 255]; a range below 1e-10f or a NaN
 *            depth gives v = 0.  Then the HOT ramp with u = v / 255.0f: r = clamp(2.5f*u), g = clamp(2.5f*u - 1.0f), b = clamp(5.0f*u - 4.0f),
 *            clamp to [0, 1], each channel (uint8)(int)(255.0f*c + 0.5f), stored in cv2's order B, G, R (what the reference's cmap returns
 *            and writes into its panel unswapped).  These are the three lines that OpenCV's 64-sample HOT table samples; cv2 interpolates its
 *            256 entries from those samples, so its table can differ from this one by a level or two beside the knees at 0.4 and 0.8.
 * scratch for either call: cnr_image_scratch_bytes (for the panel: of (1, 3, H, W)); contents need not be initialised. */
size_t cnr_image_scratch_bytes(int64_t n_images, int channels, int H, int W);
int cnr_image_metrics(const float* img0, const float* img1, int64_t n_images, int channels, int H, int W, int channels_last,
                      float* ssim_map /* same layout as the inputs, or null */, double* sums /* [2] */,
                      void* scratch, size_t scratch_bytes, void* stream);
int cnr_image_panel(const float* gt /* [H][W][3] */, const float* render /* [H][W][3] */, const float* depth /* [H][W] */, int H, int W,
                    uint8_t* panel /* [H][3W][3] */, float* range /* [2]: vmin, vmax */, void* scratch, size_t scratch_bytes, void* stream);

/* extract_color: rgb = color_network(pts, g, -g, feat) per vertex (NeuS.py:44-64) */
size_t cnr_vertex_color_scratch_bytes(const cnr_config* cfg, int64_t n_points);
int cnr_vertex_color(const cnr_config* cfg, const float* const* params, const float* verts, int64_t n_points,
                     float* rgb, void* scratch, size_t scratch_bytes, void* stream);

/* ---- mesh rasteriser: the coloured mesh (cnr_mc_emit's vertices and triangles, cnr_vertex_color's colours) seen from a camera, as a z-buffer
 * of opaque triangles: rgb [H][W][3], depth [H][W] (camera depth, the ray parameter of get_rays_at(normalize=False)) and tri_id [H][W].
 * Cameras are device pointers as for cnr_gen_rays, and origin / radius normalise the camera centre as there: t = (c2w[:3,3] - origin) / radius
 * (origin NULL: t = c2w[:3,3]); the vertices are in that normalised frame (where extract_geometry leaves them).
 * Every float operation below is one rounded fp32 operation, in the order written (no FMA; `/` is the correctly rounded IEEE quotient); the
 * integer operations are exact (int64).
 *   vertex    d = p - t;  xc = (R00*d0 + R10*d1) + R20*d2, yc and zc likewise with columns 1 and 2 of R = c2w[:3,:3].  This is R^T d: the
 *             rotation is taken as orthonormal (it is in every dataset of the reference); a c2w with scale or shear is not inverted.
 *             opengl != 0: yc = -yc, zc = -zc.   u = (fx*xc)/zc + W*0.5f,  v = (fy*yc)/zc + H*0.5f: the inverse of get_rays_at, pixel (i, j)
 *             is sampled at integer (i, j), so a pixel is covered exactly when its ray hits the triangle.
 *             X = (int)rintf(u*256.0f), Y = (int)rintf(v*256.0f): 1/256-pixel fixed point, round half to even.
 *             A vertex is usable iff zc > z_near (a NaN fails) and |u| < 2^21 and |v| < 2^21.
 *   triangle  dropped whole when an index is outside [0, n_vertices) (counted in dropped[1]; the vertex array is never read out of bounds) or
 *             when a vertex is not usable (counted in dropped[0]).  THERE IS NO POLYGON CLIPPING: a triangle that reaches behind z_near is not
 *             drawn in part.  The cameras of every shipped configuration sit outside the unit sphere that holds the mesh.
 *             A = (X1-X0)*(Y2-Y0) - (Y1-Y0)*(X2-X0).  A == 0 is skipped silently.  A < 0: vertices 1 and 2 are swapped for what follows (both
 *             facings are drawn, no culling).
 *   coverage  E0 = edge(1,2), E1 = edge(2,0), E2 = edge(0,1), edge(p,q) = (Xq-Xp)*(256 j - Yp) - (Yq-Yp)*(256 i - Xp), at pixel column i, row j.
 *             Covered iff all three are >= 0: edges are inclusive and there is no top-left rule.  A pixel on a shared edge is covered by both
 *             neighbours and the depth key decides its owner, so two triangles that share an edge leave no hole.
 *   pixel     b_k = (float)E_k / (float)A;  q_k = b_k / z_k (z_k = zc of vertex k);  s = (q0 + q1) + q2;  depth = 1.0f / s.  A depth that is not
 *             > 0 is skipped.  key = (uint64)bits(depth) << 32 | (uint32)triangle index; the z-buffer keeps the MINIMUM key per pixel (a 64-bit
 *             integer min, no float atomics): the nearest depth wins, of equal depths the lowest triangle index.  The result does not depend on
 *             the order in which triangles arrive or on how the work is split: two calls give the same bits.
 *   resolve   for the winning triangle E_k, b_k, q_k and s are recomputed from the same integers (the same bits); w_k = q_k / s;
 *             rgb = (w0*c0 + w1*c1) + w2*c2 per channel (c_k the colour of vertex k after the swap); depth comes from the key, tri_id is the index.
 *             A pixel no triangle covers gets tri_id = -1, depth = NaN, rgb = background (cnr_image_panel leaves NaN depths out of its range and
 *             draws them as level 0).
 * No anti-aliasing, culling, textures, shading or gradients.  colors and rgb are NULL together (then only depth and tri_id are written).
 * dropped: device int32 [2], overwritten.  n_triangles == 0 or n_vertices == 0 succeeds and writes an all-background image.
 * Errors: H or W < 1; H*W >= 2^31; n_vertices or n_triangles >= 2^31 (or negative); a null required pointer; rgb and colors not null together;
 * scratch too small.  scratch: cnr_mesh_raster_scratch_bytes, contents need not be initialised (0 for sizes the entry point refuses). */
size_t cnr_mesh_raster_scratch_bytes(int64_t n_vertices, int64_t n_triangles, int32_t H, int32_t W);
int cnr_mesh_raster(const float* vertices /* [V][3] */, int64_t n_vertices, const int32_t* triangles /* [F][3] */, int64_t n_triangles,
                    const float* colors /* [V][3] or NULL */, const float* c2w /* device [4][4] */, const float* focal /* device [2] */,
                    int32_t H, int32_t W, int32_t opengl, const float* origin /* device [3] or NULL */, float radius, float z_near,
                    const float* background /* host [3] or NULL = 0,0,0 */, float* rgb /* [H][W][3]; NULL iff colors NULL */,
                    float* depth /* [H][W] */, int32_t* tri_id /* [H][W] */, int32_t* dropped /* device [2] */,
                    void* scratch, size_t scratch_bytes, void* stream);

/* ---- mesh connected components and floater removal: label the components of an indexed triangle mesh (cnr_mc_emit's welded vertices make face
 * connectivity vertex connectivity), choose the ones to keep, and compact vertices, colours and triangles in their original order.  All of it is
 * integer work: every result is exact and the same bits for every face order, launch order and build.
 * Definitions:
 *   valid       a triangle whose three indices lie in [0, n_vertices).  An invalid one connects nothing, belongs to no component, is counted in
 *               dropped[0] and is never kept (cnr_mesh_raster's rule for dropped[1]; the vertex arrays are never read out of bounds).
 *   connected   two vertices are connected when a valid triangle contains both.  Degenerate (a, a, b) and duplicate triangles are valid.  A vertex
 *               in no valid triangle is a component of its own with zero faces.
 *   labels[v]   the smallest vertex index of v's component; the component's root is the vertex r with labels[r] == r.
 *   face_count[r], vertex_count[r]   the component's totals at its root, 0 at every other index.  A valid triangle counts for labels[t[0]].
 *   summary     {n_components, n_components_with_faces, largest_label, largest_face_count}: "largest" = most faces, ties to the lowest label,
 *               zero-face components are no candidates; without a valid triangle largest_label = -1 and largest_face_count = 0.
 * There is no size query and no scratch: the working storage is the typed arrays themselves, device memory owned by the caller, all overwritten:
 *   cnr_mesh_components   labels, face_count, vertex_count: int32 [n_vertices] each (labels holds the union-find's parent array while the call
 *                         runs); summary: int32 [4], 8-BYTE ALIGNED (its second half holds a 64-bit key while the call runs); dropped: int32 [1]
 *   cnr_mesh_select       keep_vertex: uint8 [n_vertices], keep_face: uint8 [n_triangles] (0 or 1); vertex_map: int32 [n_vertices], face_map:
 *                         int32 [n_triangles]: the element's index after compaction (the number of kept elements before it), -1 when it goes;
 *                         totals: int32 [2] = {V', F'}.  labels, face_count and summary are cnr_mesh_components' results for the same mesh.
 *   cnr_mesh_compact      out_vertices, out_colors: float [V'][3], out_triangles: int32 [F'][3], exactly that long (the caller reads totals
 *                         first; an array of length 0 may be NULL); out_triangles[face_map[f]][k] = vertex_map[triangles[f][k]].  vertex_map
 *                         and face_map are cnr_mesh_select's for the same mesh.
 * Selection: mode 0 (largest) keeps the faces of component largest_label and nothing else (min_faces and min_ratio are not used); mode 1
 * (threshold) keeps face f iff it is valid and face_count[labels[t[0]]] >= max(min_faces, ceil(min_ratio * largest_face_count)), the product
 * and the ceiling in fp32.  A vertex is kept iff its component is kept AND has at least one face: unreferenced vertices go.
 * n_triangles == 0 and n_vertices == 0 are legal (with n_vertices == 0 every triangle is invalid): launches over an empty range are left out,
 * summary, dropped and totals are still written.  Errors: n_triangles or n_vertices negative or above 2^31 - 1; a null pointer to an array
 * that is not empty; summary not 8-byte aligned; a mode other than 0 / 1; min_faces < 0; min_ratio < 0 or NaN; colors and out_colors not
 * null together.  Nothing is differentiable. */
int cnr_mesh_components(const int32_t* triangles /* [F][3] */, int64_t n_triangles, int64_t n_vertices, int32_t* labels, int32_t* face_count,
                        int32_t* vertex_count, int32_t* summary /* [4] */, int32_t* dropped /* [1] */, void* stream);
int cnr_mesh_select(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, const int32_t* labels, const int32_t* face_count,
                    const int32_t* summary, int32_t mode, int32_t min_faces, float min_ratio, uint8_t* keep_vertex, uint8_t* keep_face,
                    int32_t* vertex_map, int32_t* face_map, int32_t* totals /* [2] */, void* stream);
int cnr_mesh_compact(const float* vertices /* [V][3] */, const float* colors /* [V][3] or NULL */, const int32_t* triangles, int64_t n_triangles,
                     int64_t n_vertices, const int32_t* vertex_map, const int32_t* face_map, float* out_vertices, float* out_colors /* NULL iff colors NULL */,
                     int32_t* out_triangles, void* stream);

/* ---- mesh surface sampling and exact point-to-mesh distance: points drawn uniformly by area on an indexed triangle mesh, and for every query
 * point the closest triangle of a mesh -- what surface-to-surface accuracy / completeness / Chamfer / F-score need (the vertex clouds that
 * cnr_nn_search scores depend on the tessellation).  vertices: float [n_vertices][3]; triangles: int32 [n_triangles][3], 0 < n_triangles < 2^31,
 * 0 <= n_vertices < 2^31.  Every float operation below is ONE rounded fp32 operation in the written order (no FMA; sqrt and / correctly rounded),
 * everything else is integer arithmetic: results are the same bits on every run, launch shape and build.  There is no size query and no scratch:
 * cdf, summary and keys are typed device arrays owned by the caller (8-byte aligned), contents need not be initialised.  Nothing is differentiable.
 * A face is INVALID when one of its indices lies outside [0, n_vertices): it is never read through, has weight 0 and is never the closest face.
 *
 * cnr_mesh_area_cdf: integer sampling weights and their prefix sums.  For face f = (a, b, c): e1 = b - a, e2 = c - a,
 *     n = ((e1y*e2z) - (e1z*e2y), (e1z*e2x) - (e1x*e2z), (e1x*e2y) - (e1y*e2x)),   A_f = sqrtf((nx*nx + ny*ny) + nz*nz)   (the doubled area).
 *   A face whose A_f is NaN or +inf counts as invalid too.  amax = the largest A_f of the valid faces (an integer max of the bit patterns);
 *     w_f = (uint64)((A_f / amax) * 4294967296.0f)  (truncated; at most 2^32),   w_f = 0 for an invalid face and when amax == 0.
 *   A face below 2^-32 of the largest area has weight 0 and is never drawn: that is the resolution of the weights, not an error.
 *   cdf[f] = w_0 + ... + w_f (uint64 [n_triangles], exact);  summary (int64 [4]) = {total = cdf[F - 1], the number of faces with w_f == 0
 *   (the invalid ones included), the number of invalid faces, the bit pattern of amax}.
 *
 * cnr_mesh_sample: n_samples points uniform by area, counter based: sample i depends on (seed, i) alone, not on n_samples.
 *     (w0, w1, w2, w3) = Philox4x32-10 of the counter (lo32(i), hi32(i), 0, 0) under the key (lo32(seed), hi32(seed))   (cnr_choose_pixels' generator)
 *     r = the high 64 bits of ((w0 << 32) | w1) * total;   face = the first f with cdf[f] > r   (a face of weight 0 is never drawn)
 *     iu = w2 >> 8, iv = w3 >> 8;  if iu + iv > 2^24 (that is u + v > 1):  iu = 2^24 - iu, iv = 2^24 - iv;   u = iu * 2^-24, v = iv * 2^-24   (exact)
 *     point = (a + u * e1) + v * e2 per component, e1 = b - a, e2 = c - a  (the barycentric weights of a, b, c are 1 - u - v, u, v)
 *   points: float [n][3], faces: int32 [n], bary: float [n][2] = (u, v) or NULL.  total == 0 gives face = -1 and NaN in points and bary.
 *   cdf is cnr_mesh_area_cdf's for the same mesh.  n_samples == 0 is a successful no-op.
 *
 * cnr_point_mesh_distance: for query i, dist2[i] = the minimum over the faces of the squared distance to the CLOSED triangle, face[i] = the
 *   LOWEST face index that attains it, closest[i] (float [n][3] or NULL) = the closest point on that face.  Brute force over all pairs, exact.
 *   Per face: ab = b - a, ac = c - a, abab = ab.ab, abac = ab.ac, acac = ac.ac, every dot product (x*x' + y*y') + z*z'.  Per pair:
 *     ap = q - a;  d1 = ab.ap, d2 = ac.ap;  d3 = d1 - abab, d4 = d2 - abac;  d5 = d1 - abac, d6 = d2 - acac
 *     vc = d1*d4 - d3*d2,  vb = d5*d2 - d1*d6,  va = d3*d6 - d5*d4;   e43 = d4 - d3,  e56 = d5 - d6
 *   the FIRST of these regions that holds sets (n1, n2, den):
 *     vertex a   d1 <= 0 and d2 <= 0                  (0, 0, 1)
 *     vertex b   d3 >= 0 and d4 <= d3                 (1, 0, 1)
 *     edge ab    vc <= 0 and d1 >= 0 and d3 <= 0      (d1, 0, d1 - d3)
 *     vertex c   d6 >= 0 and d5 <= d6                 (0, 1, 1)
 *     edge ac    vb <= 0 and d2 >= 0 and d6 <= 0      (0, d2, d2 - d6)
 *     edge bc    va <= 0 and e43 >= 0 and e56 >= 0    (e56, e43, e43 + e56)
 *     interior   otherwise                            (vb, vc, (va + vb) + vc)
 *   inv = 1 / den,  v = n1 * inv,  w = n2 * inv,  closest = (a + v * ab) + w * ac per component,
 *     d2(i, f) = (dx*dx + dy*dy) + dz*dz,  dx = q.x - closest.x, ...   (cnr_nn_search's expression).
 *   Candidates are ordered by the 64-bit key (bits(d2) << 32) | f, folded with an integer min.  A d2 that is NaN or +inf never wins, nor does an
 *   invalid face; a query without a candidate (a NaN query, only invalid faces) gets dist2 = NaN, face = -1 and NaN in closest.  A triangle
 *   collapsed to one point (a == b == c) is "vertex a" for every query: it behaves as that point.  Any other degenerate triangle can reach
 *   den == 0 and then a non-finite d2, which never wins.  keys: uint64 [n_query] scratch.  n_query == 0 is a successful no-op.
 *
 * Errors (a negative status, the text in cnr_last_error): n_triangles <= 0 or >= 2^31; n_vertices < 0 or >= 2^31; a negative n_samples / n_query; a
 * null pointer other than bary / closest (vertices may be NULL when n_vertices == 0); cdf, summary or keys not 8-byte aligned. */
int cnr_mesh_area_cdf(const float* vertices /* [V][3] */, int64_t n_vertices, const int32_t* triangles /* [F][3] */, int64_t n_triangles,
                      uint64_t* cdf /* [F] */, int64_t* summary /* [4] */, void* stream);
int cnr_mesh_sample(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const uint64_t* cdf /* [F] */,
                    int64_t n_samples, int64_t seed, float* points /* [n][3] */, int32_t* faces /* [n] */, float* bary /* [n][2] or NULL */,
                    void* stream);
int cnr_point_mesh_distance(const float* query /* [n][3] */, int64_t n_query, const float* vertices, int64_t n_vertices, const int32_t* triangles,
                            int64_t n_triangles, float* dist2 /* [n] */, int32_t* face /* [n] */, float* closest /* [n][3] or NULL */,
                            uint64_t* keys /* [n] */, void* stream);

/* ---- culling an extracted mesh against the views: what the cameras never constrained goes.  An SDF trained with masks is supervised only inside
 * the union of the view cones through the masks; outside it the iso-surface grows sheets and caps that are ATTACHED to the object, so the
 * component selection above keeps them.  Three entries: pack and dilate the mask stack, count per vertex over the views, turn the counts into
 * cnr_mesh_select's flags, maps and totals (cnr_mesh_compact consumes them unchanged).  Integer work, and separately rounded fp32 in the vertex
 * stage: the same bits on every run, launch order and build.  There is no size query and no scratch beyond row_bits: typed device arrays owned
 * by the caller, sized by the formulas below.  Nothing is differentiable.
 *
 * cnr_mask_dilate: masks float [n_images][H][W]; foreground = mask > 0 (cnr_choose_pixels' rule: NaN and negatives are background).
 *   Packed form: one bit per pixel, Wq = ceil(W / 64) uint64 words per row, [n_images][H][Wq]; bit b of word k is pixel 64 k + b; THE BITS AT
 *   COLUMNS >= W ARE ZERO.  Output pixel (j, i) is set iff some foreground pixel (j', i') of the SAME image has |j - j'| <= radius and
 *   |i - i'| <= radius: cv2.dilate with a (2 radius + 1)^2 box of ones, pixels outside the image being background.  radius == 0 is pure
 *   packing; 0 <= radius <= 32767, and a radius beyond the image floods the rows and columns that hold a foreground pixel within reach.
 *   row_bits: scratch, bits: the result, both uint64 [n_images][H][Wq], 8-byte aligned, contents need not be initialised.
 *   n_images == 0 is a successful no-op.  Errors: n_images < 0; H or W < 1; H * W >= 2^31; n_images * H * Wq >= 2^31; a radius out of range;
 *   a null pointer; row_bits or bits not 8-byte aligned.
 *
 * cnr_mesh_view_votes: per (vertex v, view n), with cnr_mesh_raster's camera and vertex stage for c2w[n], focal[n] and the shared origin / radius /
 *   z_near / opengl (the same arithmetic: camera frame, pinhole projection, X = rint(256 u), Y = rint(256 v), zc):
 *     usable = the vertex stage accepts the vertex (finite, zc > z_near, |u|, |v| < 2^21)
 *     i = (X + 128) >> 8,  j = (Y + 128) >> 8   (arithmetic shift: the nearest pixel centre; centres sit at integer coordinates)
 *     seen = usable and 0 <= i < W and 0 <= j < H
 *     counts[v][0] += 1
 *     counts[v][1] += seen
 *     counts[v][2] += seen && (mask_bits == NULL || bit (j, i) of view n)
 *     counts[v][3] += seen && (depth == NULL || !(zc > depth[n][j][i] * (1.0f + depth_tol)))    (the sum and the product one fp32 rounding each;
 *                     a NaN depth -- no surface at that pixel, cnr_mesh_raster's value -- fails the comparison and counts as visible)
 *   counts: int32 [n_vertices][4], 16-BYTE ALIGNED, ADDED TO: the caller zeroes it, and calls on one stream accumulate (views in chunks).  Each
 *   row is read and written by one lane, once per call: no atomics.  mask_bits: cnr_mask_dilate's packed form for the same H, W, or NULL;
 *   depth: float [n_views][H][W] (cnr_mesh_raster's depth maps) or NULL; c2w float [n_views][4][4], focal float [n_views][2], origin float [3]
 *   or NULL, all device memory.  n_views == 0 and n_vertices == 0 are successful no-ops.  Errors: n_vertices < 0 or >= 2^31; the image errors
 *   of cnr_mask_dilate with n_views for n_images; a null vertices, c2w, focal or counts; mask_bits not 8-byte or counts not 16-byte aligned.
 *
 * cnr_mesh_cull_select: with (total, seen, inside, visible) = counts[v], vertex v PASSES iff
 *     seen >= min_views  &&  seen - inside <= max_outside  &&  visible >= min_visible.
 *   A valid face (three indices in [0, n_vertices), as above) is kept iff all three of its vertices pass (face_rule 0) or any of them passes
 *   (face_rule 1); an invalid face is never kept and is counted in dropped[0].  keep_vertex[v] = 1 iff some kept face names v (so with
 *   face_rule 1 a vertex that does not pass can stay, and a passing vertex without a kept face goes).  keep_vertex uint8 [n_vertices],
 *   keep_face uint8 [n_triangles], vertex_map int32 [n_vertices], face_map int32 [n_triangles], totals int32 [2] = {V', F'}: exactly
 *   cnr_mesh_select's outputs; dropped int32 [1].  All overwritten.  n_triangles == 0 and n_vertices == 0 are legal, totals and dropped are
 *   still written.  Errors: n_triangles or n_vertices negative or above 2^31 - 1; a face_rule other than 0 / 1; a negative min_views,
 *   max_outside or min_visible; a null pointer to an array that is not empty, a null totals or dropped. */
int cnr_mask_dilate(const float* masks /* [n][H][W] */, int64_t n_images, int32_t H, int32_t W, int32_t radius,
                    uint64_t* row_bits /* scratch [n][H][Wq] */, uint64_t* bits /* out [n][H][Wq] */, void* stream);
int cnr_mesh_view_votes(const float* vertices /* [V][3] */, int64_t n_vertices, const float* c2w /* [n][4][4] */, const float* focal /* [n][2] */,
                        const float* origin /* [3] or NULL */, float radius, float z_near, int32_t opengl, int64_t n_views, int32_t H, int32_t W,
                        const uint64_t* mask_bits /* [n][H][Wq] or NULL */, const float* depth /* [n][H][W] or NULL */, float depth_tol,
                        int32_t* counts /* [V][4], ADDED to */, void* stream);
int cnr_mesh_cull_select(const int32_t* triangles /* [F][3] */, int64_t n_triangles, int64_t n_vertices, const int32_t* counts /* [V][4] */,
                         int32_t min_views, int32_t max_outside, int32_t min_visible, int32_t face_rule, uint8_t* keep_vertex, uint8_t* keep_face,
                         int32_t* vertex_map, int32_t* face_map, int32_t* totals /* [2] */, int32_t* dropped /* [1] */, void* stream);

/* ---- ICP registration: the rigid or similarity map x' = s*R*x + t that takes a point set onto a cloud or a mesh, by iterated closest
 * points.  With learnable cameras a reconstruction drifts by a similarity against its ground truth; the mesh metrics above then measure the
 * drift.  One call enqueues `iterations` iterations on the stream with no host synchronisation and no allocation (capturable); the match of
 * every iteration is cnr_nn_search's search (cloud target: triangles NULL, n_triangles 0, n_target points) or cnr_point_mesh_distance's (mesh
 * target: n_target vertices, n_triangles faces) as they stand.  There is no size query and no scratch: every buffer is a typed device array
 * owned by the caller, contents need not be initialised (transform, and idx with resume != 0, are inputs).  pivots is a HOST array
 * {c_src[3], c_tgt[3]}, read when the call is issued: the moments are taken about them (the clouds' means keep the sums small).
 * Every float and double operation below is ONE rounded operation in the written order (no FMA; / and sqrt correctly rounded): the same bits
 * on every run, launch shape and build.  transform = {R row-major [9], t [3], s, 0, 0, 0}.  Iteration k:
 *   1. move     m[r][c] = (float)(s*R[r][c]) (the double product rounded once), tf[r] = (float)t[r];
 *               moved_i[r] = ((m[r][0]*x + m[r][1]*y) + m[r][2]*z) + tf[r] in fp32, (x, y, z) = source_i.
 *   2. match    dist2_i, idx_i = the search of moved_i (the nearest target point / the closest face; lowest index on ties; NaN and -1
 *               without a candidate); matched_i = that target point, or the closest point on that face (cnr_point_mesh_distance's
 *               `closest`, evaluated with the moments), NaN when idx_i = -1.
 *   3. moments  i is an inlier iff idx_i >= 0 and dist2_i <= max_dist2 (fp32; +inf: no gate).  a = (double)source_i - c_src (the ORIGINAL
 *               point: the solved map is absolute, not an increment), b = (double)matched_i - c_tgt.  Eighteen fp64 terms: a (3), b (3),
 *               b[r]*a[c] (9, row-major), a.a, b.b, (double)dist2_i, every dot product (x*x + y*y) + z*z; eighteen zeros for a non-inlier.
 *               ONE summation order: chunks of 256 consecutive points padded with zeros, within a chunk the tree x[j] += x[j + h] for
 *               h = 128, 64, ..., 1 (the chunk's sums: a row of partials), then the rows added one after the other in chunk order, from +0.0.
 *               n_inliers and n_changed (idx_i differs from the previous iteration's) are integer counts.  With resume == 0 the first
 *               iteration does not read idx and n_changed = n_source; with resume != 0 idx holds the previous call's last result.
 *   4. solve    n = n_inliers; abar = Sa/n, bbar = Sb/n; C[r][c] = Sba[r][c] - Sb[r]*abar[c]; va = Saa - ((Sa0*abar0 + Sa1*abar1) + Sa2*abar2).
 *               Horn's symmetric 4x4 matrix of C, with Sxy = C[y][x] (the source axis first):
 *                 N00 = (Sxx + Syy) + Szz  N01 = Syz - Szy          N02 = Szx - Sxz          N03 = Sxy - Syx
 *                                          N11 = (Sxx - Syy) - Szz  N12 = Sxy + Syx          N13 = Szx + Sxz
 *                                                                   N22 = (Syy - Sxx) - Szz  N23 = Syz + Szy
 *                                                                                            N33 = (Szz - Sxx) - Syy
 *               TEN cyclic Jacobi sweeps, each the planes (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), V = I at the start.  A rotation whose
 *               off-diagonal element N[p][q] is exactly 0 is skipped; otherwise theta = (N[q][q] - N[p][p]) / (2*N[p][q]),
 *               tt = sgn(theta) / (|theta| + sqrt(theta*theta + 1)) (sgn(0) = +1), c = 1 / sqrt(tt*tt + 1), sn = tt*c, h = tt*N[p][q];
 *               N[p][p] -= h, N[q][q] += h, N[p][q] = N[q][p] = 0; for the other two rows r: N[r][p] = c*arp - sn*arq, N[r][q] = sn*arp + c*arq
 *               (arp, arq the old N[r][p], N[r][q]; mirrored); for every row r of V the same pair of expressions on V[r][p], V[r][q].
 *               (w, x, y, z) = the column of V under the largest diagonal element (the lowest index on ties), each divided by
 *               nrm = sqrt(((w*w + x*x) + y*y) + z*z), all four negated when w < 0.  A unit quaternion always gives a proper rotation:
 *                 R = [1 - 2*(y*y + z*z), 2*(x*y - w*z), 2*(x*z + w*y);  2*(x*y + w*z), 1 - 2*(x*x + z*z), 2*(y*z - w*x);
 *                      2*(x*z - w*y), 2*(y*z + w*x), 1 - 2*(x*x + y*y)]
 *               s = (R[0][0]*C[0][0] + R[0][1]*C[0][1] + ..., the nine products added one after the other in row-major order) / va with
 *               with_scale, else 1;  t[r] = (bbar[r] + c_tgt[r]) - s*((R[r][0]*p0 + R[r][1]*p1) + R[r][2]*p2), p = abar + c_src.
 *               Degenerate -- n_inliers < 3, a sum that is not finite, va <= 0, or a result that is not finite or whose s is not positive:
 *               the transform is left exactly as it was and the status is 1; else the status is 0.
 *   5. history  history[k] = {n_inliers, n_changed, the sum of the inliers' dist2, status}, all measured under the transform iteration k
 *               STARTED with; the counts are exact in a double.
 * After the call moved, matched, dist2 and idx hold the last iteration's correspondence.  The transform is absolute and the sums have one
 * order, so an iteration with n_changed == 0 and the same inlier set is a fixed point (every later iteration writes the same bits), and
 * `a` iterations followed by a resume != 0 call of `b` give the bits of one call of a + b.  Nothing is differentiable.
 * Errors (a negative status, the text in cnr_last_error): n_source < 0 or >= 2^31; n_target outside [1, 2^31); n_triangles < 0 or >= 2^31;
 * triangles NULL with n_triangles != 0 or the reverse; iterations < 0; max_dist2 NaN or negative; a null pointer; transform, history, keys
 * or partials not 8-byte aligned.  n_source == 0 or iterations == 0 is a successful no-op that leaves transform untouched. */
int cnr_icp(const float* source /* [n][3] */, int64_t n_source, const float* target /* cloud [m][3], or mesh vertices [V][3] */, int64_t n_target,
            const int32_t* triangles /* [F][3], or NULL with n_triangles == 0: cloud target */, int64_t n_triangles,
            const double* pivots /* HOST [6]: c_src, c_tgt */, int32_t with_scale, float max_dist2, int32_t iterations, int32_t resume,
            double* transform /* device [16], in/out */, double* history /* device [iterations][4] */, float* moved /* [n][3] */,
            float* matched /* [n][3] */, float* dist2 /* [n] */, int32_t* idx /* [n] */, uint64_t* keys /* [n] */,
            double* partials /* [ceil(n/256)][18] */, void* stream);

/* ---- one plain fully-connected layer on the layer / weight-gradient kernels of the render path: y = act(x W^T + b), act = ReLU or none.
 * The NeRF++ background network of NeuS (NeRF, fields.py:192-274; N_OUTSIDE > 0, NeuS.py:95-134) is a chain of nn.Linear (+ ReLU) layers;
 * color-neus_amd/background.py evaluates each of them through these two entry points.  x [n][k], y / dy [n][n_out], W [n_out][k] and b [n_out]
 * are compact row-major device fp32 (nn.Linear's layout); backward: dx (or NULL), dW [n_out][k], db (or NULL) are overwritten. */
size_t cnr_linear_scratch_bytes(int64_t n, int32_t k, int32_t n_out, int32_t backward);
int cnr_linear_forward(const float* x, int64_t n, int32_t k, const float* W, const float* b /* or NULL */, int32_t n_out, int32_t relu, float* y,
                       void* scratch, size_t scratch_bytes, void* stream);
int cnr_linear_backward(const float* x, const float* y /* the forward output (ReLU gate); may be NULL without ReLU */, const float* dy, int64_t n,
                        int32_t k, const float* W, int32_t n_out, int32_t relu, float* dx, float* dW, float* db, void* scratch,
                        size_t scratch_bytes, void* stream);

/* ---- N_OUTSIDE > 0: the NeRF++ background of NeuS.forward (lib/models/renderers/NeuS.py:313-369) -----------------------------------------
 * The reference evaluates a second network (NeRF, fields.py:192-274, built with its defaults: NeuS.py:87-91) on the foreground samples
 * merged with n_outside inverse-depth samples beyond `far`, and mixes its alpha / colour into render_core by the inside-sphere mask
 * (NeuS.py:262-268, Color_NeuS.py:97-102).  No shipped configuration sets N_OUTSIDE.  Four steps, each a forward / backward pair; the
 * foreground fields come from cnr_render_forward's per-sample outputs (sdf_samples, gradients, color_samples, global_color_samples) and
 * their gradients go back through cnr_render_out_grads:
 *   cnr_outside_z                  z_vals_outside (NeuS.py:315-338) merged into the sorted z_vals_feed (NeuS.py:353-355)
 *   cnr_background_forward         render_core_outside (NeuS.py:95-134) up to its per-sample outputs: alpha and sigmoid(rgb)
 *   cnr_composite_background_*     the tail of render_core with background_alpha / background_sampled_color given
 * Parameters of the background network: cnr_nerf_param_info order = nn.Module order of NeRF (pts_linears.i.weight / .bias, views_linears.0.*,
 * feature_linear.*, alpha_linear.*, rgb_linear.*), plain nn.Linear tensors. */
typedef struct cnr_nerf_config {
  int32_t D, W;              /* depth / width of the pts stack (NeRF defaults 8 / 256) */
  int32_t multires;          /* PE of the 4-vector (x / r, 1 / r): default 10 */
  int32_t multires_view;     /* PE of the view direction: default 4 */
  int32_t skip_mask;         /* bit i: [PE | h] is concatenated after pts layer i (default 1 << 4) */
} cnr_nerf_config;
int cnr_nerf_param_count(const cnr_nerf_config* cfg);
int cnr_nerf_param_info(const cnr_nerf_config* cfg, int index, char* name, int name_len, int* rows, int* cols);

/* z_feed [R][n_z + n_outside] = sort(cat(z_vals [R][n_z] (ascending), far / flip(zz) + 1 / n_samples)); t_rand [R][n_outside] = the
 * torch.rand draw of NeuS.py:335 or NULL (no perturbation); src [R][n_z + n_outside] (int32, for the backward call): where each entry came from.
 * Backward: d_far [R] through the background samples, d_z [R][n_z] (or NULL) for the copies of z_vals. */
int cnr_outside_z(const float* far_, const float* t_rand, const float* z_vals, int64_t n_rays, int32_t n_z, int32_t n_outside, int32_t n_samples,
                  float* z_feed, int32_t* src, void* stream);
int cnr_outside_z_backward(const float* t_rand, const int32_t* src, const float* d_z_feed, int64_t n_rays, int32_t n_z, int32_t n_outside,
                           int32_t n_samples, float* d_far, float* d_z, void* stream);

/* alpha [R][n_feed], color [R][n_feed][3] of the background network at the n_feed samples of every ray; ctx keeps the activations for
 * cnr_background_backward, which overwrites d_params (host array of device pointers, cnr_nerf_param_info order), d_rays_o / d_rays_d [R][3]
 * and d_z_feed [R][n_feed]. */
size_t cnr_background_ctx_bytes(const cnr_nerf_config* cfg, int64_t n_rays, int32_t n_feed);
size_t cnr_background_bwd_scratch_bytes(const cnr_nerf_config* cfg, int64_t n_rays, int32_t n_feed);
int cnr_background_forward(const cnr_nerf_config* cfg, const float* const* params, const float* rays_o, const float* rays_d, const float* z_feed,
                           int64_t n_rays, int32_t n_feed, float sample_dist, float* alpha, float* color, void* ctx, size_t ctx_bytes, void* stream);
int cnr_background_backward(const cnr_nerf_config* cfg, const float* const* params, const float* rays_o, const float* rays_d, const float* z_feed,
                            int64_t n_rays, int32_t n_feed, float sample_dist, const void* ctx, size_t ctx_bytes, const float* color,
                            const float* d_alpha, const float* d_color, float* const* d_params, float* d_rays_o, float* d_rays_d, float* d_z_feed,
                            void* scratch, size_t scratch_bytes, void* stream);

/* render_core's alpha / mixing / compositing over n_feed = n_z + n_outside samples.  Outputs: the members of cnr_render_outputs that render_core
 * returns (weights is [R][n_feed] here; gradients / delta_relight / z_vals / the per-sample members are not written); eik_sums must be given.
 * Backward: upstream gradients in cnr_render_out_grads (color_fine, s_val, cdf_fine, weight_sum, weight_max, weights [R][n_feed],
 * gradient_error, depth, global_color, gradients), results in cnr_bg_composite_grads (all overwritten; d_variance is [1]). */
typedef struct cnr_bg_composite_in {
  const float* rays_o; const float* rays_d; const float* z_vals /* [R][n_z] */; const float* z_feed /* [R][n_feed] */;
  int64_t n_rays; int32_t n_z, n_feed; float sample_dist;
  const float* sdf_samples; const float* gradients /* [R][n_z][3] */; const float* color_samples; const float* global_color_samples /* or NULL (NeuS) */;
  const float* bg_alpha /* [R][n_feed] */; const float* bg_color /* [R][n_feed][3] */;
  const float* variance /* deviation_network.variance, device [1] */; float cos_anneal_ratio; const float* background_rgb /* [3] or NULL */;
} cnr_bg_composite_in;
typedef struct cnr_bg_composite_grads {
  float* d_sdf_samples; float* d_gradients; float* d_color_samples; float* d_global_color_samples; float* d_bg_alpha; float* d_bg_color;
  float* d_variance; float* d_rays_d /* [R][3] */; float* d_z_vals /* [R][n_z] */; float* d_z_feed /* [R][n_feed] */;
} cnr_bg_composite_grads;
size_t cnr_composite_background_scratch_bytes(int64_t n_rays);
int cnr_composite_background_forward(const cnr_bg_composite_in* in, const cnr_render_outputs* out, void* scratch, size_t scratch_bytes, void* stream);
int cnr_composite_background_backward(const cnr_bg_composite_in* in, const cnr_render_outputs* out, const cnr_render_out_grads* gout,
                                      const cnr_bg_composite_grads* gin, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* COLORNEUS_RENDER_H_ */
