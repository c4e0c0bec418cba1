// On-device pixel choice: descriptors, launches and the integer arithmetic both builds share.
#pragma once
#include "cnr_common.h"
#include "cnr_philox.h"   // pix_philox, pix_mulhi64

namespace cnr {

// ---- on-device pixel choice (cnr_pixel_table_build / cnr_choose_pixels; specified in include/colorneus_render.h): the sampling semantics of
// get_rays_multicam's pixel choice (ray_utils.py:57-76) on a Philox stream keyed by a device {seed, step}.  The arithmetic (pix_* below)
// is shared by the HIP kernels and the emulation; all of it is integer arithmetic.
constexpr int kPixTile = 4096;            // pixels of one image that one workgroup counts / scatters (16 wave-chunks of 256: 64 lanes x one 16-byte load)
constexpr int kPixMaxSlots = 1024;        // images per draw: the slot prefixes live in LDS
struct PixelTable {
  const float* masks; int n_images; long hw;   // [n_images][hw]
  int* order;                             // [n_images][hw]: foreground pixels ascending, then background pixels ascending
  int* fg_count; int* bg_count;           // [n_images]
  int* tile_counts; long tiles;           // [n_images][tiles][2] scratch: per-tile {fg, bg} counts -> exclusive offsets within the image
};
void be_pixel_table(const PixelTable& t, cnr_stream s);
struct PixelDraw {
  long* state;                            // device {seed, step}; the step is advanced behind the draw
  long n; int want_fg; const int* want_fg_dev;
  const int* cam_ids; int B, n_images; long hw;
  const int* order; const int* fg_count; const int* bg_count;   // all null: draws with replacement over [0, span)
  unsigned long long span;
  long* idx; int* cams_out; int* counts_out; float* t_rand;
};
void be_choose_pixels(const PixelDraw& p, cnr_stream s);

// ---- on-device pixel choice (PixelTable / PixelDraw): the integer arithmetic that include/colorneus_render.h specifies
struct PixKey { unsigned k0, k1, step; };   // Philox key (seed_lo, seed_hi) and counter word 3 of one draw
CNR_HD PixKey pix_key(long seed, long step) {
  const unsigned long long s = (unsigned long long)seed;
  return PixKey{(unsigned)(s & 0xffffffffull), (unsigned)(s >> 32), (unsigned)((unsigned long long)step & 0xffffffffull)};
}
CNR_HD unsigned pix_word0(const PixKey& k, unsigned a, unsigned b, unsigned stream) {
  unsigned w[4];
  pix_philox(a, b, stream, k.step, k.k0, k.k1, w);
  return w[0];
}
// the keyed bijection of [0, D): cycle walking on an 8-round Feistel network over 2h bits, 2^2h < 4 D
CNR_HD unsigned pix_perm(const PixKey& k, unsigned j, unsigned D, unsigned stream) {
  if (D <= 1u) return 0u;
  int bits = 0;
  for (unsigned v = D - 1u; v; v >>= 1) ++bits;
  const int h = (bits + 1) / 2;
  const unsigned m = (1u << h) - 1u;        // h <= 16
  unsigned x = j;
  do {
    unsigned L = x >> h, R = x & m;
    for (unsigned r = 0; r < 8u; ++r) {
      const unsigned t = L ^ (pix_word0(k, R, r, stream) & m);
      L = R; R = t;
    }
    x = (L << h) | R;
  } while (x >= D);
  return x;
}
// 1: foreground (mask > 0), 2: background (mask == 0), 0: neither (negative, NaN)
CNR_HD int pix_class(float v) { return v > 0.0f ? 1 : (v == 0.0f ? 2 : 0); }
// the image of slot b
CNR_HD int pix_slot_image(const PixelDraw& p, const PixKey& k, int b) {
  return p.cam_ids ? p.cam_ids[b] : (int)pix_perm(k, (unsigned)b, (unsigned)p.n_images, 0u);
}
// {foreground, background} pixels of a slot's image: none for an image outside the table; clamped so that no offset below fg + bg leaves the
// image's row of `order`, whatever the count arrays hold
CNR_HD void pix_slot_counts(const PixelDraw& p, int cam, unsigned* fg, unsigned* bg) {
  *fg = 0u; *bg = 0u;
  if (!p.order || cam < 0 || cam >= p.n_images) return;
  long f = p.fg_count[cam], g = p.bg_count[cam];
  f = f < 0 ? 0 : (f > p.hw ? p.hw : f);
  g = g < 0 ? 0 : (g > p.hw - f ? p.hw - f : g);
  *fg = (unsigned)f; *bg = (unsigned)g;
}
CNR_HD int pix_want_fg(const PixelDraw& p) {
  const long w = p.want_fg_dev ? (long)p.want_fg_dev[0] : (long)p.want_fg;
  return (int)(w < 0 ? 0 : (w > p.n ? p.n : w));
}
// draws without a table: element j of the list with replacement
CNR_HD long pix_draw_replace(const PixelDraw& p, const PixKey& k, long j) {
  unsigned w[4];
  pix_philox((unsigned)j, 0u, 4u, k.step, k.k0, k.k1, w);
  return (long)pix_mulhi64(((unsigned long long)w[0] << 32) | w[1], p.span);
}
// element j of the list (foreground draws, then background draws) and where the shuffle puts it.  pf / pb: inclusive slot-order prefixes of the
// foreground / background counts (pf[B - 1] = F, pb[B - 1] = G); cams: the image of every slot; kfg = min(want_fg, F)
CNR_HD void pix_draw_masked(const PixelDraw& p, const PixKey& k, long j, const unsigned* pf, const unsigned* pb, const int* cams, unsigned kfg) {
  const bool fg = (unsigned long long)j < kfg;
  const unsigned* pre = fg ? pf : pb;
  const unsigned D = pre[p.B - 1], jj = fg ? (unsigned)j : (unsigned)j - kfg;
  long val = -1;
  if (jj < D) {
    const unsigned rank = pix_perm(k, jj, D, fg ? 1u : 2u);
    int lo = 0, hi = p.B - 1;                 // the first slot whose prefix exceeds the rank (pre[B - 1] = D > rank)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (pre[mid] > rank) hi = mid; else lo = mid + 1;
    }
    const unsigned off = rank - (lo ? pre[lo - 1] : 0u);
    const int cam = cams[lo];                 // a slot with pixels names a valid image
    const long at = (long)cam * p.hw + (fg ? 0u : pf[lo] - (lo ? pf[lo - 1] : 0u)) + off;   // background: behind the image's foreground list
    val = (long)cam * p.hw + p.order[at];
  }
  p.idx[pix_perm(k, (unsigned)j, (unsigned)p.n, 3u)] = val;
}
CNR_HD float pix_jitter(const PixKey& k, long j) { return (float)(pix_word0(k, (unsigned)j, 0u, 5u) >> 8) * 0x1p-24f; }

}  // namespace cnr
