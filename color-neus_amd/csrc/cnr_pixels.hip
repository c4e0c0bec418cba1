// On-device pixel choice for gfx950 (cnr_pixel_table_build / cnr_choose_pixels; specified in include/colorneus_render.h).  The arithmetic --
// Philox4x32-10, the keyed bijection, the classification of a mask value, one draw -- is the pix_* functions of cnr_pixels.h, shared with the
// CPU emulation; the kernels only decide who computes what.  Integer arithmetic only, plain C++, vector stores.
//
//   pixel_count_kernel    one block = one tile of kPixTile pixels of one image.  A wave reads a chunk of 256 pixels with one 16-byte load per
//                         lane (scalar loads where the image's row is not 16-byte aligned or runs out), four chunks per wave; the number of
//                         foreground / background pixels of a chunk is the popcount of four ballots -> tile_counts[image][tile][2]
//   pixel_scan_kernel     one block per image: exclusive scan of its tile counts in place, totals -> fg_count / bg_count
//   pixel_scatter_kernel  the tile again: the classes of a lane's 16 pixels stay in one register; chunk counts through LDS give every chunk its
//                         offset in the tile; rank inside a chunk = popcount of the ballots below the lane (+ the lane's own earlier pixels):
//                         a stable compaction, every pixel index stored once
//   choose_pixels_kernel  ONE block: slot images and their counts (thread b = slot b), block scan into the LDS prefixes, then a grid-stride
//                         loop over the n draws (each a function of its index alone), a barrier, and thread 0 advances the step
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cnr_pixels.h"
#include "cnr_hip_util.h"
#include "cnr_wave.h"

namespace cnr {

constexpr int kPixThreads = 256;
constexpr int kPixWaves = kPixThreads / 64;
constexpr int kPixChunk = 256;                                   // pixels of one wave-wide 16-byte load
constexpr int kPixIters = kPixTile / (kPixWaves * kPixChunk);    // chunks per wave and tile
constexpr int kPixChunks = kPixWaves * kPixIters;                // chunks per tile; chunk c = it * kPixWaves + wave, in pixel order
static_assert(kPixTile == kPixChunks * kPixChunk && kPixIters * 4 * 2 <= 32, "a lane's classes of one tile fit one 32-bit register");

// the classes (pix_class, two bits each) of the four pixels p0 .. p0 + 3 of one image row; a pixel past the row is in neither list
__device__ __forceinline__ unsigned pix_classes4(const float* row, long hw, long p0) {
  const float* a = row + p0;
  float v[4];
  if (p0 + 3 < hw && (reinterpret_cast<uintptr_t>(a) & 15) == 0) {
    const f4 q = *reinterpret_cast<const f4*>(a);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = p0 + e < hw ? a[e] : -1.0f;
  }
  unsigned c = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) c |= (unsigned)pix_class(v[e]) << (2 * e);
  return c;
}

__global__ __launch_bounds__(kPixThreads) void pixel_count_kernel(const PixelTable t) {
  __shared__ int wcnt[kPixWaves][2];
  const long image = blockIdx.x / t.tiles, tile = blockIdx.x - image * t.tiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* row = t.masks + image * t.hw;
  int nf = 0, nb = 0;                                            // wave-uniform
#pragma unroll
  for (int it = 0; it < kPixIters; ++it) {
    const long p0 = tile * kPixTile + (long)(it * kPixWaves + wave) * kPixChunk + 4 * lane;
    const unsigned c = pix_classes4(row, t.hw, p0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      nf += __popcll(__ballot(((c >> (2 * e)) & 3u) == 1u));
      nb += __popcll(__ballot(((c >> (2 * e)) & 3u) == 2u));
    }
  }
  if (lane == 0) { wcnt[wave][0] = nf; wcnt[wave][1] = nb; }
  __syncthreads();
  if (threadIdx.x < 2) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < kPixWaves; ++w) s += wcnt[w][threadIdx.x];
    t.tile_counts[(long)blockIdx.x * 2 + threadIdx.x] = s;
  }
}

// per image: tile counts -> exclusive offsets, totals
__global__ __launch_bounds__(kPixThreads) void pixel_scan_kernel(const PixelTable t) {
  __shared__ int wsum[2][kPixWaves];
  __shared__ int carry[2];
  int* counts = t.tile_counts + (long)blockIdx.x * t.tiles * 2;
  block_carried_scan<kPixWaves, 1, 2, int>(t.tiles, wsum, carry,
                                           [&](long i, int (&x)[2]) { x[0] += counts[i * 2]; x[1] += counts[i * 2 + 1]; },
                                           [&](long i, const int (&at)[2]) { counts[i * 2] = at[0]; counts[i * 2 + 1] = at[1]; });
  if (threadIdx.x == 0) { t.fg_count[blockIdx.x] = carry[0]; t.bg_count[blockIdx.x] = carry[1]; }
}

__global__ __launch_bounds__(kPixThreads) void pixel_scatter_kernel(const PixelTable t) {
  __shared__ int ccnt[kPixChunks][2];
  const long image = blockIdx.x / t.tiles, tile = blockIdx.x - image * t.tiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* row = t.masks + image * t.hw;
  int* out = t.order + image * t.hw;
  unsigned classes = 0;                                          // two bits per pixel: iteration it, element e at bit 8 * it + 2 * e
#pragma unroll
  for (int it = 0; it < kPixIters; ++it) {
    const long p0 = tile * kPixTile + (long)(it * kPixWaves + wave) * kPixChunk + 4 * lane;
    const unsigned c = pix_classes4(row, t.hw, p0);
    classes |= c << (8 * it);
    int nf = 0, nb = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      nf += __popcll(__ballot(((c >> (2 * e)) & 3u) == 1u));
      nb += __popcll(__ballot(((c >> (2 * e)) & 3u) == 2u));
    }
    if (lane == 0) { ccnt[it * kPixWaves + wave][0] = nf; ccnt[it * kPixWaves + wave][1] = nb; }
  }
  __syncthreads();
  const long nfg = t.fg_count[image];
  const long tf = t.tile_counts[(long)blockIdx.x * 2], tb = nfg + t.tile_counts[(long)blockIdx.x * 2 + 1];   // where this tile's two runs start
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int it = 0; it < kPixIters; ++it) {
    const int chunk = it * kPixWaves + wave;
    long of = tf, ob = tb;                                       // + the chunks in front of this one
    for (int c = 0; c < chunk; ++c) { of += ccnt[c][0]; ob += ccnt[c][1]; }
    const unsigned c4 = (classes >> (8 * it)) & 0xffu;
    unsigned long long bf[4], bb[4];
    int rf = 0, rb = 0;                                          // pixels of the lanes below, in this chunk
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bf[e] = __ballot(((c4 >> (2 * e)) & 3u) == 1u);
      bb[e] = __ballot(((c4 >> (2 * e)) & 3u) == 2u);
      rf += __popcll(bf[e] & below);
      rb += __popcll(bb[e] & below);
    }
    const long p0 = tile * kPixTile + (long)chunk * kPixChunk + 4 * lane;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned cls = (c4 >> (2 * e)) & 3u;
      const long dst = cls == 1u ? of + rf : ob + rb;
      if (cls != 0u && dst < t.hw) out[dst] = (int)(p0 + e);    // (dst < hw by construction: fg + bg <= hw; the test costs nothing)
      rf += cls == 1u;
      rb += cls == 2u;
    }
  }
}

void be_pixel_table(const PixelTable& t, cnr_stream s) {
  const unsigned blocks = (unsigned)((long)t.n_images * t.tiles);
  const double px = (double)t.n_images * (double)t.hw;
  {
    TimingScope ts_("pixel_count_kernel", 2, 0, t.n_images, 0, 0, 0, s, 4.0 * px);
    hipLaunchKernelGGL(pixel_count_kernel, dim3(blocks), dim3(kPixThreads), 0, s, t);
  }
  {
    TimingScope ts_("pixel_scan_kernel", 2, 0, t.n_images, 0, 0, 0, s, 16.0 * (double)blocks);
    hipLaunchKernelGGL(pixel_scan_kernel, dim3((unsigned)t.n_images), dim3(kPixThreads), 0, s, t);
  }
  {
    TimingScope ts_("pixel_scatter_kernel", 2, 0, t.n_images, 0, 0, 0, s, 8.0 * px);
    hipLaunchKernelGGL(pixel_scatter_kernel, dim3(blocks), dim3(kPixThreads), 0, s, t);
  }
  CNR_LAUNCH_CHECK("pixel_table");
}

constexpr int kDrawThreads = 1024;
static_assert(kDrawThreads == kPixMaxSlots, "thread b owns slot b");

__global__ __launch_bounds__(kDrawThreads) void choose_pixels_kernel(const PixelDraw p) {
  __shared__ unsigned pf[kPixMaxSlots], pb[kPixMaxSlots];       // inclusive slot-order prefixes of the foreground / background counts
  __shared__ int cams[kPixMaxSlots];
  __shared__ unsigned wsum[2][kDrawThreads / 64];
  const int tid = threadIdx.x;
  const long seed = p.state[0], step = p.state[1];              // every thread reads the state in front of the barriers; thread 0 writes it behind them
  const PixKey k = pix_key(seed, step);
  const unsigned want = (unsigned)pix_want_fg(p);
  unsigned fg[2] = {0, 0};
  if (tid < p.B) {
    const int cam = pix_slot_image(p, k, tid);
    pix_slot_counts(p, cam, &fg[0], &fg[1]);
    cams[tid] = cam;
    if (p.cams_out) p.cams_out[tid] = cam;
  }
  unsigned excl[2];
  block_excl_scan<kDrawThreads / 64, 2, unsigned>(fg, excl, wsum, nullptr);
  if (tid < p.B) { pf[tid] = excl[0] + fg[0]; pb[tid] = excl[1] + fg[1]; }
  __syncthreads();
  const unsigned F = pf[p.B - 1], G = pb[p.B - 1];
  const unsigned kfg = want < F ? want : F;
  if (tid == 0 && p.counts_out) {
    const unsigned long long m = (unsigned long long)p.n - kfg;
    p.counts_out[0] = p.order ? (int)kfg : 0;
    p.counts_out[1] = p.order ? (int)(m < G ? m : G) : 0;
  }
  for (long j = tid; j < p.n; j += kDrawThreads) {
    if (p.order) pix_draw_masked(p, k, j, pf, pb, cams, kfg);
    else p.idx[j] = pix_draw_replace(p, k, j);
    if (p.t_rand) p.t_rand[j] = pix_jitter(k, j);
  }
  __syncthreads();
  if (tid == 0) p.state[1] = (long)((unsigned long long)step + 1ull);
}

void be_choose_pixels(const PixelDraw& p, cnr_stream s) {
  TimingScope ts_("choose_pixels_kernel", 2, 0, p.n, p.B, 0, 0, s, 8.0 * (double)p.n);
  hipLaunchKernelGGL(choose_pixels_kernel, dim3(1), dim3(kDrawThreads), 0, s, p);
  CNR_LAUNCH_CHECK("choose_pixels");
}

}  // namespace cnr
