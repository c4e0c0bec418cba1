// Mesh rasteriser for gfx950 (cnr_mesh_raster): a z-buffer of opaque triangles with per-vertex colours, the per-element arithmetic of cnr_raster.h.
// The depth test is a 64-bit unsigned integer atomic min on (bits(depth) << 32) | triangle: exact and order-independent, no float atomics.
//
//   raster_project_kernel   one vertex per lane -> {X, Y, zc} (12 bytes) in scratch; the same grid sets the H*W keys to "no triangle" and zeroes
//                           the two drop counters and the length of the large-triangle list
//   raster_small_kernel     one triangle per lane: gather its three projected vertices, reject, clip the box; a box of at most CNR_RASTER_SMALL
//                           pixels on a side is walked by the lane, one atomic min per covered pixel.  A larger one goes into the list: its
//                           place by wave ballot + popcount, one atomic add per wave.  The drop counters are counted the same way.
//   raster_large_kernel     a fixed grid of workgroups strides over the list (its length is read on the device: no host synchronisation); a
//                           workgroup's 256 lanes stride over the triangle's clipped box in 64-pixel row segments
//   raster_resolve_kernel   one pixel per lane: decode the key, gather the winner's vertices and colours, write rgb / depth / tri_id
#include <hip/hip_runtime.h>

#include "cnr_raster.h"
#include "cnr_hip_util.h"
#include "cnr_wave.h"

namespace cnr {

constexpr int kRasterThreads = 256;
constexpr int kRasterLargeBlocks = 1024;   // 4 resident workgroups per CU x 256 CUs
constexpr int kRasterSeg = 64;             // pixels of one row segment of the large-triangle walk

__global__ __launch_bounds__(kRasterThreads) void raster_project_kernel(const MeshRaster p) {
  const long i = (long)blockIdx.x * kRasterThreads + threadIdx.x;
  if (i == 0) { p.dropped[0] = 0; p.dropped[1] = 0; *p.n_large = 0; }
  if (i < (long)p.H * p.W) p.keys[i] = kRasterNoKey;
  if (i < p.V) {
    const RasterCam cam = raster_cam(p);
    const float v[3] = {p.vertices[i * 3], p.vertices[i * 3 + 1], p.vertices[i * 3 + 2]};
    p.pv[i] = raster_project(cam, v, p.opengl, p.z_near);
  }
}

__global__ __launch_bounds__(kRasterThreads) void raster_small_kernel(const MeshRaster p) {
  const long f = (long)blockIdx.x * kRasterThreads + threadIdx.x;
  RasterTri t;
  t.status = 3;
  if (f < p.F) {
    const int tri[3] = {p.triangles[f * 3], p.triangles[f * 3 + 1], p.triangles[f * 3 + 2]};
    t = raster_setup(tri, p.V, p.pv, p.H, p.W);
  }
  const bool draw = t.status == 0, small = draw && raster_is_small(t);
  (void)wave_append(t.status == 1, &p.dropped[0]);
  (void)wave_append(t.status == 2, &p.dropped[1]);
  const int at = wave_append(draw && !small, p.n_large);
  if (draw && !small) p.large[at] = (int)f;
  if (!small) return;
  for (int j = t.j0; j <= t.j1; ++j)
    for (int i = t.i0; i <= t.i1; ++i) {
      const unsigned long long key = raster_pixel_key(t, (int)f, i, j);
      if (key != kRasterNoKey) atomicMin(&p.keys[(long)j * p.W + i], key);
    }
}

__global__ __launch_bounds__(kRasterThreads) void raster_large_kernel(const MeshRaster p) {
  const int n = *p.n_large;
  for (int l = blockIdx.x; l < n; l += gridDim.x) {
    const int f = p.large[l];
    const RasterTri t = raster_setup(p.triangles + (long)f * 3, p.V, p.pv, p.H, p.W);   // status 0: the small-triangle launch listed it
    const long segs = (t.i1 - t.i0 + kRasterSeg) / kRasterSeg, rows = t.j1 - t.j0 + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long sgm = wave; sgm < segs * rows; sgm += kRasterThreads / 64) {
      const int j = t.j0 + (int)(sgm / segs), i = t.i0 + (int)(sgm % segs) * kRasterSeg + lane;
      if (i > t.i1) continue;
      const unsigned long long key = raster_pixel_key(t, f, i, j);
      if (key != kRasterNoKey) atomicMin(&p.keys[(long)j * p.W + i], key);
    }
  }
}

__global__ __launch_bounds__(kRasterThreads) void raster_resolve_kernel(const MeshRaster p) {
  const long at = (long)blockIdx.x * kRasterThreads + threadIdx.x;
  if (at >= (long)p.H * p.W) return;
  const int j = (int)(at / p.W);
  raster_resolve(p, (int)(at - (long)j * p.W), j);
}

void be_mesh_raster(const MeshRaster& p, cnr_stream s) {
  const long hw = (long)p.H * p.W;
  const long n0 = p.V > hw ? p.V : hw;
  const double V = (double)p.V, F = (double)p.F, HW = (double)hw;
  {
    TimingScope ts_("raster_project_kernel", 2, 0, p.V, p.H, p.W, 0, s, 24.0 * V + 8.0 * HW);
    hipLaunchKernelGGL(raster_project_kernel, dim3((unsigned)((n0 + kRasterThreads - 1) / kRasterThreads)), dim3(kRasterThreads), 0, s, p);
  }
  if (p.F > 0 && p.V > 0) {
    {
      TimingScope ts_("raster_small_kernel", 2, 0, p.F, p.H, p.W, 0, s, 48.0 * F);
      hipLaunchKernelGGL(raster_small_kernel, dim3((unsigned)((p.F + kRasterThreads - 1) / kRasterThreads)), dim3(kRasterThreads), 0, s, p);
    }
    {
      TimingScope ts_("raster_large_kernel", 2, 0, p.F, p.H, p.W, 0, s, 0.0);
      hipLaunchKernelGGL(raster_large_kernel, dim3(kRasterLargeBlocks), dim3(kRasterThreads), 0, s, p);
    }
  }
  {
    TimingScope ts_("raster_resolve_kernel", 2, 0, hw, p.H, p.W, 0, s, (p.rgb ? 28.0 : 16.0) * HW);
    hipLaunchKernelGGL(raster_resolve_kernel, dim3((unsigned)((hw + kRasterThreads - 1) / kRasterThreads)), dim3(kRasterThreads), 0, s, p);
  }
  CNR_LAUNCH_CHECK("mesh_raster");
}

}  // namespace cnr
