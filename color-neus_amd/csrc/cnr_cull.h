// Culling an extracted mesh against the views (cnr_mask_dilate / cnr_mesh_view_votes / cnr_mesh_cull_select): the per-element code the HIP
// kernels (cnr_cull.hip) and the CPU emulation (cnr_kernels_emu.cpp) share.  The masks and the selection are integer work; the votes use the
// rasteriser's camera and vertex stage (raster_cam_of / raster_project, cnr_raster.h) and one fp32 product for the depth test, every float
// operation separately rounded (-ffp-contract=off).  Both builds, any launch order and any run give the same bits.
//
// Definitions (the contract; include/colorneus_render.h states them for the caller):
//   * a packed mask row holds one bit per pixel, Wq = ceil(W / 64) words: bit b of word k is pixel 64 k + b, the bits at columns >= W are zero
//   * foreground is mask > 0 (pix_foreground's rule, cnr_pixels.h: NaN and negatives are background); the dilation of radius r sets pixel
//     (j, i) iff a foreground pixel (j', i') of the same image has |j - j'| <= r and |i - i'| <= r, pixels outside the image being background
//   * the box is separable: cull_pack_word packs, cull_hdilate_word dilates a packed row along the columns, cull_vdilate_word ORs the 2r + 1
//     rows around a word; each writes whole words, so no launch order matters
//   * per (vertex, view): usable = raster_project's depth is not NaN; pixel i = (X + 128) >> 8, j = (Y + 128) >> 8 (the nearest pixel centre);
//     seen = usable and inside the image; counts[v] += {1, seen, seen && mask bit, seen && !(zc > depth * (1 + depth_tol))}
//   * a vertex passes iff seen >= min_views && seen - inside <= max_outside && visible >= min_visible; a valid face is kept iff all
//     (face_rule 0) or any (face_rule 1) of its vertices pass; keep_vertex[v] = 1 iff a kept face names v; the maps and totals are
//     cnr_mesh_select's (mesh_keep_scan, cnr_meshcc.h)
#pragma once
#include "cnr_common.h"
#include "cnr_raster.h"
#include "cnr_meshcc.h"

namespace cnr {

constexpr int CNR_CULL_FACE_ALL = 0, CNR_CULL_FACE_ANY = 1;   // cnr_mesh_cull_select's face_rule
constexpr int kCullMaxRadius = 32767;

struct MaskDilate {
  const float* masks; long n; int H, W, Wq, radius;   // [n][H][W]
  unsigned long long* row_bits;                       // [n][H][Wq] scratch: the rows dilated along the columns
  unsigned long long* bits;                           // [n][H][Wq] out (holds the packed, undilated rows between the first two launches)
};
void be_mask_dilate(const MaskDilate& p, cnr_stream s);

struct MeshViewVotes {
  const float* vertices; long V;        // [V][3]
  const float* c2w; const float* focal; const float* origin;   // device [n][4][4], [n][2], [3] or null
  float radius, z_near; int opengl; long n_views; int H, W, Wq;
  const unsigned long long* mask_bits;  // [n][H][Wq] or null
  const float* depth; float depth_tol;  // [n][H][W] or null
  int* counts;                          // [V][4], added to
};
void be_mesh_view_votes(const MeshViewVotes& p, cnr_stream s);

struct MeshCullSelect {
  const int* triangles; long F, V;
  const int* counts;                    // [V][4]
  int min_views, max_outside, min_visible, face_rule;
  unsigned char* keep_vertex; unsigned char* keep_face;   // [V], [F]
  int* vertex_map; int* face_map; int* totals; int* dropped;   // [V], [F], [2], [1]
};
void be_mesh_cull_select(const MeshCullSelect& p, cnr_stream s);

// ---- masks
CNR_HD bool cull_foreground(float m) { return m > 0.0f; }
// the bits a row's word k may hold: all 64, or the low W % 64 of the row's last word
CNR_HD unsigned long long cull_pad_mask(int W, int k) {
  const int left = W - k * 64;
  return left >= 64 ? ~0ull : (1ull << left) - 1ull;
}
// bits [0, hi] / [lo, 63] of a word (hi, lo in 0 .. 63)
CNR_HD unsigned long long cull_bits_upto(int hi) { return hi >= 63 ? ~0ull : (1ull << (hi + 1)) - 1ull; }
CNR_HD unsigned long long cull_bits_from(int lo) { return ~0ull << lo; }
CNR_HD int cull_highest(unsigned long long x) { return 63 - __builtin_clzll(x); }   // x != 0
CNR_HD int cull_lowest(unsigned long long x) { return __builtin_ctzll(x); }        // x != 0
// word k of a row of floats (the emulation's form of the wave's ballot)
CNR_HD unsigned long long cull_pack_word(const float* row, int W, int k) {
  unsigned long long w = 0ull;
  for (int b = 0; b < 64 && k * 64 + b < W; ++b) w |= (unsigned long long)cull_foreground(row[k * 64 + b]) << b;
  return w;
}
// x | x << 1 | ... | x << m and x | x >> 1 | ... | x >> m inside one word, m in 0 .. 63: the reach doubles until it is m
CNR_HD unsigned long long cull_smear_word(unsigned long long x, int m) {
  unsigned long long up = x, down = x;
  for (int have = 0; have < m;) {
    const int step = have + 1 < m - have ? have + 1 : m - have;
    up |= up << step; down |= down >> step;
    have += step;
  }
  return up | down;
}
// Word k of a packed row (Wq words, pad bits zero) dilated along the columns by r = 64 q + m.  A source word at word distance below q covers
// word k whole; the word q to the left reaches the bits up to (its highest bit) + m, the word q + 1 to the left up to (its highest bit) + m - 64,
// and likewise from the right with the lowest bits; with q == 0 the word itself is smeared by m.
CNR_HD unsigned long long cull_hdilate_word(const unsigned long long* row, int Wq, int W, int k, int r) {
  const int q = r >> 6, m = r & 63;
  unsigned long long out = 0ull;
  if (q == 0) {
    out = cull_smear_word(row[k], m);
  } else {
    const int a = k - (q - 1) < 0 ? 0 : k - (q - 1), b = k + (q - 1) > Wq - 1 ? Wq - 1 : k + (q - 1);
    for (int s = a; s <= b; ++s) if (row[s]) { out = ~0ull; break; }
    if (k - q >= 0 && row[k - q]) out |= cull_bits_upto(cull_highest(row[k - q]) + m);
    if (k + q < Wq && row[k + q]) out |= cull_bits_from(cull_lowest(row[k + q]) - m < 0 ? 0 : cull_lowest(row[k + q]) - m);
  }
  if (k - q - 1 >= 0 && row[k - q - 1]) {
    const int hi = cull_highest(row[k - q - 1]) + m - 64;
    if (hi >= 0) out |= cull_bits_upto(hi);
  }
  if (k + q + 1 < Wq && row[k + q + 1]) {
    const int lo = 64 + cull_lowest(row[k + q + 1]) - m;
    if (lo <= 63) out |= cull_bits_from(lo);
  }
  return out & cull_pad_mask(W, k);
}
// word k of row j of an image's column-dilated rows (rows: [H][Wq]) ORed over the rows within r of j, clipped to the image
CNR_HD unsigned long long cull_vdilate_word(const unsigned long long* rows, int H, int Wq, int j, int k, int r) {
  const int j0 = j - r < 0 ? 0 : j - r, j1 = r > H - 1 - j ? H - 1 : j + r;
  unsigned long long out = 0ull;
  for (int jj = j0; jj <= j1; ++jj) out |= rows[(long)jj * Wq + k];
  return out;
}

// ---- votes
CNR_HD int cull_round256(int x) { return (x + 128) >> 8; }   // the nearest pixel centre of a 1/256-pixel coordinate (arithmetic shift)
// the four additions of one (vertex, view): c[0..3] += {1, seen, inside, visible}.  mask: the view's packed rows or null; depth: the view's
// [H][W] map or null; tol1 = 1.0f + depth_tol.
CNR_HD void cull_vote(const RasterCam& cam, const float* v, int opengl, float z_near, int H, int W, int Wq, const unsigned long long* mask,
                      const float* depth, float tol1, int* c) {
  c[0] += 1;
  const RasterVert pv = raster_project(cam, v, opengl, z_near);
  if (!(pv.z == pv.z)) return;
  const int i = cull_round256(pv.X), j = cull_round256(pv.Y);
  if (i < 0 || i >= W || j < 0 || j >= H) return;
  c[1] += 1;
  if (!mask || ((mask[(long)j * Wq + (i >> 6)] >> (i & 63)) & 1ull)) c[2] += 1;
  if (!depth || !(pv.z > depth[(long)j * W + i] * tol1)) c[3] += 1;
}

// ---- selection
CNR_HD bool cull_vertex_passes(const MeshCullSelect& p, int v) {
  const int* c = p.counts + (long)v * 4;
  return c[1] >= p.min_views && c[1] - c[2] <= p.max_outside && c[3] >= p.min_visible;
}
// face f: 1 kept, 0 valid and not kept, -1 invalid (counted in dropped[0], never kept)
CNR_HD int cull_face(const MeshCullSelect& p, long f) {
  const int* t = p.triangles + f * 3;
  if (!meshcc_valid(t, p.V)) return -1;
  const bool a = cull_vertex_passes(p, t[0]), b = cull_vertex_passes(p, t[1]), c = cull_vertex_passes(p, t[2]);
  return (p.face_rule == CNR_CULL_FACE_ANY ? (a || b || c) : (a && b && c)) ? 1 : 0;
}
// the marks of a kept face: plain stores of 1 (lanes that store to the same vertex store the same value)
CNR_HD void cull_mark(const MeshCullSelect& p, long f) {
  const int* t = p.triangles + f * 3;
  for (int k = 0; k < 3; ++k) p.keep_vertex[t[k]] = 1;
}

}  // namespace cnr
