// Image evaluation for gfx950 (cnr_image_metrics / cnr_image_panel): squared error and window-3 SSIM sums of two images, and the
// gt | render | depth picture of validate_image as bytes.  The per-pixel arithmetic is the img_* functions of cnr_image.h, shared with
// the CPU emulation; the kernels only decide who computes what.
//
//   image_stats_kernel         one block = one tile of kImgTileH rows x kImgTileW floats of one plane (cnr_image.h: both layouts are
//                              planes of rows whose horizontal neighbours are cs floats apart, so a channels-last tile is a contiguous
//                              piece of every row with all channels in it).  The tile of both images and a halo of one row / cs floats
//                              (reflected at the image border) goes to LDS with row-contiguous loads, once; the row pass of the five
//                              filtered maps (x, y, x*x, y*y, x*y) runs once per staged row and tile column into LDS, the column pass
//                              once per output element.  d*d and ssim are added in float64: four elements per lane in row order, the
//                              64 lanes by shuffles, the four waves in wave order -> partials[block].  No atomics.
//   image_stats_finish_kernel  one block: lane t adds a contiguous run of partials in index order, then lanes and waves as above -> sums[2]
//   depth_range_kernel         min / max of the non-NaN depths by integer atomic min on order-preserving keys (exact in any order)
//   image_panel_kernel         four panel bytes per lane, stored as one 32-bit word; the colour sections read one float4 per lane
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cnr_image.h"
#include "cnr_hip_util.h"

namespace cnr {

constexpr int kImgThreads = 256;
constexpr int kImgWaves = kImgThreads / 64;
constexpr int kImgRows = kImgTileH + 2;                 // staged rows: the tile and one halo row above and below
constexpr int kImgPlane = kImgRows * kImgTileW;         // one row-filtered map in LDS
static_assert(kImgTileW == 64 && kImgTileH == 4 * kImgWaves, "one wave per four tile rows, one lane per tile column");

// {a, b} summed over the block in a fixed order: lanes by shuffle (the same tree every time), then the waves in wave order; valid in thread 0
__device__ __forceinline__ void img_block_sum(double& a, double& b, double* wsum) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off);
    b += __shfl_down(b, off);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { wsum[wave * 2] = a; wsum[wave * 2 + 1] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = wsum[0]; b = wsum[1];
#pragma unroll
    for (int w = 1; w < kImgWaves; ++w) { a += wsum[w * 2]; b += wsum[w * 2 + 1]; }
  }
}

__global__ __launch_bounds__(kImgThreads) void image_stats_kernel(const ImageStats p, long tx, long ty) {
  extern __shared__ float img_lds[];
  __shared__ double wsum[kImgWaves * 2];
  const int cs = p.cs, sw = kImgTileW + 2 * cs;
  float* rx = img_lds;                      // [kImgRows][sw] staged x: column j is row float f0 - cs + j
  float* ry = rx + kImgRows * sw;           // the same of y
  float* h = ry + kImgRows * sw;            // [5][kImgRows][kImgTileW] row-filtered x, y, x*x, y*y, x*y
  long b = blockIdx.x;
  const long bx = b % tx; b /= tx;
  const long by = b % ty;
  const long plane = b / ty;
  const long rowlen = (long)p.W * cs;
  const long f0 = bx * kImgTileW;
  const int y0 = (int)by * kImgTileH;
  const long base = plane * p.H * rowlen;
  const float* px = p.x + base;
  const float* py = p.y + base;
  for (int i = threadIdx.x; i < kImgRows * sw; i += kImgThreads) {
    const int r = i / sw, j = i - r * sw;
    int gy = y0 - 1 + r;
    long g = f0 - cs + j;
    float vx = 0.0f, vy = 0.0f;
    if (gy <= p.H && g < rowlen + cs) {     // inside the image or its one-pixel reflected border
      gy = img_reflect(gy, p.H);
      if (g < 0) g += 2 * cs;               // pixel -1 -> pixel 1, same channel
      else if (g >= rowlen) g -= 2 * cs;    // pixel W -> pixel W - 2
      vx = px[gy * rowlen + g];
      vy = py[gy * rowlen + g];
    }
    rx[i] = vx;
    ry[i] = vy;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kImgPlane; i += kImgThreads) {
    const int r = i >> 6, j = i & 63;
    const float* ax = rx + r * sw + j;
    const float* ay = ry + r * sw + j;
    const float xl = ax[0], xc = ax[cs], xr = ax[2 * cs];
    const float yl = ay[0], yc = ay[cs], yr = ay[2 * cs];
    h[i] = img_tap3(xl, xc, xr);
    h[kImgPlane + i] = img_tap3(yl, yc, yr);
    h[2 * kImgPlane + i] = img_tap3(xl * xl, xc * xc, xr * xr);
    h[3 * kImgPlane + i] = img_tap3(yl * yl, yc * yc, yr * yr);
    h[4 * kImgPlane + i] = img_tap3(xl * yl, xc * yc, xr * yr);
  }
  __syncthreads();
  const int j = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * 4;
  const long g = f0 + j;
  double sum_d = 0.0, sum_s = 0.0;
  if (g < rowlen) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = r0 + k, gy = y0 + r;    // output row r of the tile: staged rows r, r + 1, r + 2
      if (gy >= p.H) break;
      float m[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        const float* hq = h + q * kImgPlane + r * kImgTileW + j;
        m[q] = img_tap3(hq[0], hq[kImgTileW], hq[2 * kImgTileW]);
      }
      const float s = img_ssim(m[0], m[1], m[2], m[3], m[4]);
      const float e = img_sqerr(rx[(r + 1) * sw + cs + j], ry[(r + 1) * sw + cs + j]);
      if (p.map) p.map[base + gy * rowlen + g] = s;
      sum_d += (double)e;
      sum_s += (double)s;
    }
  }
  img_block_sum(sum_d, sum_s, wsum);
  if (threadIdx.x == 0) { p.partials[2 * (long)blockIdx.x] = sum_d; p.partials[2 * (long)blockIdx.x + 1] = sum_s; }
}

__global__ __launch_bounds__(kImgThreads) void image_stats_finish_kernel(const ImageStats p) {
  __shared__ double wsum[kImgWaves * 2];
  const long per = (p.nblocks + kImgThreads - 1) / kImgThreads;
  const long i0 = threadIdx.x * per;
  const long i1 = i0 + per < p.nblocks ? i0 + per : p.nblocks;
  double a = 0.0, b = 0.0;
  for (long i = i0; i < i1; ++i) { a += p.partials[2 * i]; b += p.partials[2 * i + 1]; }
  img_block_sum(a, b, wsum);
  if (threadIdx.x == 0) { p.sums[0] = a; p.sums[1] = b; }
}

__global__ __launch_bounds__(kImgThreads) void depth_range_kernel(const ImagePanel p) {
  const long n = (long)p.H * p.W;
  unsigned kmin = 0xffffffffu, kinv = 0xffffffffu;
  for (long i = (long)blockIdx.x * kImgThreads + threadIdx.x; i < n; i += (long)gridDim.x * kImgThreads) {
    const float d = p.depth[i];
    if (d == d) {
      const unsigned k = img_depth_key(d);
      kmin = k < kmin ? k : kmin;
      kinv = ~k < kinv ? ~k : kinv;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned a = (unsigned)__shfl_xor((int)kmin, off), c = (unsigned)__shfl_xor((int)kinv, off);
    kmin = a < kmin ? a : kmin;
    kinv = c < kinv ? c : kinv;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&p.keys[0], kmin);
    atomicMin(&p.keys[1], kinv);
  }
}

__global__ __launch_bounds__(kImgThreads) void image_panel_kernel(const ImagePanel p) {
  const unsigned rowb = (unsigned)p.nsec * 3u * (unsigned)p.W;        // bytes per panel row; the panel has fewer than 2^31 bytes
  const unsigned total = (unsigned)p.H * rowb;
  const unsigned b0 = 4u * (blockIdx.x * (unsigned)kImgThreads + threadIdx.x);
  if (b0 >= total) return;
  float vmin, vmax;
  img_depth_range(p.keys, &vmin, &vmax);
  if (b0 == 0) { p.range[0] = vmin; p.range[1] = vmax; }
  const unsigned row = b0 / rowb, col = b0 - row * rowb;
  const unsigned w3 = 3u * (unsigned)p.W, sec = col / w3, c = col - sec * w3;
  unsigned char q[4] = {0, 0, 0, 0};
  const float* src = sec == 0 ? p.gt : p.render;
  const bool colour = (int)sec < p.nsec - 1 && c + 3 < w3;             // four bytes of one colour section of one row
  if (colour && (reinterpret_cast<uintptr_t>(src + (size_t)row * w3 + c) & 15) == 0) {
    const f4 v = *reinterpret_cast<const f4*>(src + (size_t)row * w3 + c);
    q[0] = img_quant(v.x); q[1] = img_quant(v.y); q[2] = img_quant(v.z); q[3] = img_quant(v.w);
  } else {
    unsigned rr = row, cc = col;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (b0 + k < total) q[k] = img_panel_byte(p, (int)rr, (int)cc, vmin, vmax);
      if (++cc == rowb) { cc = 0; ++rr; }
    }
  }
  if (b0 + 4 <= total && (reinterpret_cast<uintptr_t>(p.panel) & 3) == 0) {
    *reinterpret_cast<unsigned*>(p.panel + b0) = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16) | ((unsigned)q[3] << 24);
  } else {
    for (int k = 0; k < 4; ++k)
      if (b0 + k < total) p.panel[b0 + k] = q[k];
  }
}

void be_image_stats(const ImageStats& p, cnr_stream s) {
  if (p.nblocks == 0) {
    device_fill(p.sums, 0, 2 * sizeof(double), s, "image_stats memset");
    return;
  }
  const long tx = img_tiles_x(p.W, p.cs), ty = img_tiles_y(p.H);
  const double n = (double)p.planes * p.H * p.W * p.cs;
  const size_t lds = ((size_t)2 * kImgRows * (kImgTileW + 2 * p.cs) + 5 * kImgPlane) * sizeof(float);   // <= 41.5 KB at cs = kImgMaxCs
  {
    TimingScope ts_("image_stats_kernel", 2, 0, p.planes, p.H, p.W * p.cs, p.cs, s, (p.map ? 12.0 : 8.0) * n + 16.0 * (double)p.nblocks);
    hipLaunchKernelGGL(image_stats_kernel, dim3((unsigned)p.nblocks), dim3(kImgThreads), lds, s, p, tx, ty);
  }
  {
    TimingScope ts_("image_stats_finish_kernel", 2, 0, p.nblocks, 0, 0, 0, s, 16.0 * (double)p.nblocks + 16.0);
    hipLaunchKernelGGL(image_stats_finish_kernel, dim3(1), dim3(kImgThreads), 0, s, p);
  }
  CNR_LAUNCH_CHECK("image_stats");
}

void be_image_panel(const ImagePanel& p, cnr_stream s) {
  const long n = (long)p.H * p.W;
  device_fill(p.keys, 0xff, 2 * sizeof(unsigned), s, "image_panel memset");
  {
    long blocks = (n + kImgThreads * 4 - 1) / (kImgThreads * 4);
    if (blocks > 1024) blocks = 1024;
    TimingScope ts_("depth_range_kernel", 2, 0, n, 0, 0, 0, s, 4.0 * (double)n);
    hipLaunchKernelGGL(depth_range_kernel, dim3((unsigned)blocks), dim3(kImgThreads), 0, s, p);
  }
  {
    const long total = n * 3 * p.nsec, words = (total + 3) / 4;
    TimingScope ts_("image_panel_kernel", 2, 0, n, p.nsec, 0, 0, s, (double)n * (24.0 * (p.nsec - 1) / 2 + 4.0) + (double)total);
    hipLaunchKernelGGL(image_panel_kernel, dim3((unsigned)((words + kImgThreads - 1) / kImgThreads)), dim3(kImgThreads), 0, s, p);
  }
  CNR_LAUNCH_CHECK("image_panel");
}

}  // namespace cnr
