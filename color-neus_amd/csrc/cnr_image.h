// Image evaluation (PSNR / SSIM statistics, the validation panel): descriptors, launches and the per-element arithmetic both builds share.
#pragma once
#include "cnr_common.h"

namespace cnr {

// ---- image evaluation (cnr_image_metrics / cnr_image_panel): what NeuS_Trainer.validate_image does behind its render loop
// (NeuS_Trainer.py:250-277): squared error (PSNR), the window-3 SSIM of lib/metrics/similarity.py:55, and the gt | render | depth picture.
// The arithmetic is specified in include/colorneus_render.h; every operation below is a separately rounded fp32 operation in the order
// written (the build passes -ffp-contract=off), so the HIP kernel and the emulation produce the same bits per pixel.
// Both layouts are one picture of `planes` planes of H rows of `rowlen` floats whose horizontal neighbours are `cs` floats apart:
//   [B][C][H][W]  planes = B*C, rowlen = W,   cs = 1          [B][H][W][C]  planes = B, rowlen = W*C, cs = C
struct ImageStats {
  const float* x; const float* y;      // the two images
  long planes; int H, W, cs;           // rowlen = W * cs
  float* map;                          // SSIM per element, the inputs' layout, or null
  double* partials; long nblocks;      // [nblocks][2] scratch: per-block {sum d*d, sum ssim}
  double* sums;                        // [2]
};
void be_image_stats(const ImageStats& p, cnr_stream s);
struct ImagePanel {
  const float* gt; const float* render;   // [H][W][3], or both null: the panel is the depth map alone, [H][W][3]
  const float* depth;                     // [H][W]
  int H, W, nsec;                         // nsec = 3 (gt | render | depth) or 1
  unsigned char* panel;                   // [H][nsec*W][3]
  float* range;                           // [2] vmin, vmax over the non-NaN depths ({0, 0} when there is none)
  unsigned* keys;                         // [2] scratch: min of img_depth_key, min of ~img_depth_key
};
void be_image_panel(const ImagePanel& p, cnr_stream s);
constexpr int kImgMaxCs = 32;             // channels-last form: at most this many channels (the halo of a staged row is cs floats each side)
constexpr int kImgTileW = 64, kImgTileH = 16;   // floats x rows of one block's tile
CNR_HD long img_tiles_x(int W, int cs) { return ((long)W * cs + kImgTileW - 1) / kImgTileW; }
CNR_HD long img_tiles_y(int H) { return (H + kImgTileH - 1) / kImgTileH; }
// reflection without repeating the edge: -1 -> 1, n -> n - 2 (only called with i in [-1, n], n >= 2)
CNR_HD int img_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
// one pass of the normalised 3-tap Gaussian (sigma 1.5, as float32 torch evaluates it): outer taps w1, centre w0
CNR_HD float img_tap3(float a, float b, float c) {
  const float w1 = 0x1.3b3046p-2f, w0 = 0x1.899f76p-2f;
  return (w1 * a + w0 * b) + w1 * c;
}
CNR_HD float img_ssim(float mu1, float mu2, float e11, float e22, float e12) {
  const float m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
  const float s1 = e11 - m11, s2 = e22 - m22, s12 = e12 - m12;
  const float num = (2.0f * m12 + 1e-4f) * (2.0f * s12 + 9e-4f);
  const float den = ((m11 + m22) + 1e-4f) * ((s1 + s2) + 9e-4f);
  return num / (den + 1e-12f);
}
CNR_HD float img_sqerr(float x, float y) {
  const float d = x - y;
  return d * d;
}
// clamp to [lo, hi] that sends NaN to lo
CNR_HD float img_clamp(float v, float lo, float hi) {
  v = v > lo ? v : lo;
  return v < hi ? v : hi;
}
// rgb.mul(255.0).astype(np.uint8) (NeuS_Trainer.py:252-256): truncation; out-of-range values are clamped (numpy wraps them), NaN gives 0
CNR_HD unsigned char img_quant(float v) { return (unsigned char)(int)img_clamp(v * 255.0f, 0.0f, 255.0f); }
// order-preserving key of a non-NaN float (negative values: all bits flipped, others: sign bit set)
CNR_HD unsigned img_depth_key(float d) {
  unsigned b;
  memcpy(&b, &d, sizeof b);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
CNR_HD float img_depth_unkey(unsigned k) {
  const unsigned b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float d;
  memcpy(&d, &b, sizeof d);
  return d;
}
// keys = {min key, min ~key} as be_image_panel's range pass leaves them -> vmin, vmax ({0, 0} when no depth was a number)
CNR_HD void img_depth_range(const unsigned* keys, float* vmin, float* vmax) {
  const unsigned kmin = keys[0], kmax = ~keys[1];
  if (kmin > kmax) { *vmin = 0.0f; *vmax = 0.0f; return; }
  *vmin = img_depth_unkey(kmin); *vmax = img_depth_unkey(kmax);
}
// image_float_to_uint8 (viztools.py:145-155): level 0..255 of a depth in [vmin, vmax]; a range below 1e-10 or a NaN depth gives 0
CNR_HD int img_depth_level(float d, float vmin, float vmax) {
  const float range = vmax - vmin;
  if (!(range >= 1e-10f)) return 0;
  const float t = (d - vmin) / range;
  return (int)img_clamp(t * 255.0f, 0.0f, 255.0f);
}
// channel ch (0 blue, 1 green, 2 red: cv2's order) of the HOT ramp at level v
CNR_HD unsigned char img_hot(int v, int ch) {
  const float u = (float)v / 255.0f;
  const float c = ch == 2 ? 2.5f * u : (ch == 1 ? 2.5f * u - 1.0f : 5.0f * u - 4.0f);
  return (unsigned char)(int)(255.0f * img_clamp(c, 0.0f, 1.0f) + 0.5f);
}
// byte `col` (0 .. nsec*3W) of panel row `row`
CNR_HD unsigned char img_panel_byte(const ImagePanel& p, int row, int col, float vmin, float vmax) {
  const int w3 = 3 * p.W, sec = col / w3, c = col - sec * w3;
  if (sec < p.nsec - 1) return img_quant((sec == 0 ? p.gt : p.render)[(long)row * w3 + c]);
  return img_hot(img_depth_level(p.depth[(long)row * p.W + c / 3], vmin, vmax), c % 3);
}

}  // namespace cnr
