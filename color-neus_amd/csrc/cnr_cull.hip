// Culling an extracted mesh against the views for gfx950 (cnr_mask_dilate / cnr_mesh_view_votes / cnr_mesh_cull_select): the per-element code
// of cnr_cull.h.  Integer work and separately rounded fp32; every output element is written by one lane (the marks of cull_faces_kernel are
// racing stores of the same value), so the results do not depend on the order in which lanes, waves or workgroups run.
//
//   cull_pack_kernel      one wave per kCullPackPer words of the packed stack: 64 consecutive floats of a row per word (a coalesced 256-byte
//                         load), the word is the wave's ballot of mask > 0; columns >= W load nothing and vote 0, so the pad bits are zero
//   cull_hdilate_kernel   one word per lane: the row's words around it through cull_hdilate_word (bits -> row_bits)
//   cull_vdilate_kernel   one word per lane: the OR of the 2r + 1 words above and below it, clipped to the image (row_bits -> bits).  The
//                         packed stack is 1/32 of the float stack and stays in L2
//   cull_votes_kernel     one vertex per lane.  The workgroup builds the cameras of kCullViews views in LDS (raster_cam_of: the origin's
//                         division once per view and workgroup, not once per vertex), every lane then votes its vertex through them; the
//                         four counts stay in registers over all views and go out as ONE 16-byte load and store per vertex
//   cull_clear_kernel     keep_vertex = 0, dropped = 0
//   cull_faces_kernel     one face per lane: three gathers of the corners' counts, the rule, keep_face, the marks of a kept face's corners;
//                         invalid faces counted by ballot + popcount, one add per wave
//   meshcc_scan_kernel    (cnr_meshcc.hip, mesh_keep_scan) the flags -> the maps and totals
#include <hip/hip_runtime.h>

#include "cnr_cull.h"
#include "cnr_hip_util.h"
#include "cnr_wave.h"

namespace cnr {

constexpr int kCullThreads = 256;
constexpr int kCullPackPer = 4;     // words per wave of cull_pack_kernel: four row segments in flight per lane
constexpr int kCullViews = 16;      // cameras in LDS per trip of cull_votes_kernel

__global__ __launch_bounds__(kCullThreads) void cull_pack_kernel(const MaskDilate p, long words) {
  const int lane = threadIdx.x & 63;
  const long w0 = ((long)blockIdx.x * (kCullThreads / 64) + (threadIdx.x >> 6)) * kCullPackPer;
  float m[kCullPackPer];
#pragma unroll
  for (int t = 0; t < kCullPackPer; ++t) {
    const long w = w0 + t, row = w / p.Wq;
    const int i = (int)(w - row * p.Wq) * 64 + lane;
    m[t] = w < words && i < p.W ? p.masks[row * p.W + i] : 0.0f;
  }
#pragma unroll
  for (int t = 0; t < kCullPackPer; ++t) {
    const unsigned long long word = __ballot(cull_foreground(m[t]));
    if (lane == t && w0 + t < words) p.bits[w0 + t] = word;
  }
}

__global__ __launch_bounds__(kCullThreads) void cull_hdilate_kernel(const MaskDilate p, long words) {
  const long w = (long)blockIdx.x * kCullThreads + threadIdx.x;
  if (w >= words) return;
  const long row = w / p.Wq;
  p.row_bits[w] = cull_hdilate_word(p.bits + row * p.Wq, p.Wq, p.W, (int)(w - row * p.Wq), p.radius);
}

__global__ __launch_bounds__(kCullThreads) void cull_vdilate_kernel(const MaskDilate p, long words) {
  const long w = (long)blockIdx.x * kCullThreads + threadIdx.x;
  if (w >= words) return;
  const long row = w / p.Wq, img = row / p.H;
  p.bits[w] = cull_vdilate_word(p.row_bits + img * p.H * p.Wq, p.H, p.Wq, (int)(row - img * p.H), (int)(w - row * p.Wq), p.radius);
}

void be_mask_dilate(const MaskDilate& p, cnr_stream s) {
  const long words = p.n * p.H * p.Wq;
  const double px = (double)p.n * p.H * p.W, wb = 8.0 * (double)words;
  const int rows = 2 * p.radius + 1 < p.H ? 2 * p.radius + 1 : p.H;
  const unsigned blocks = (unsigned)((words + kCullThreads - 1) / kCullThreads);
  {
    constexpr int per = kCullThreads / 64 * kCullPackPer;
    TimingScope ts_("cull_pack_kernel", 2, 0, words, p.H, p.W, 0, s, 4.0 * px + wb);
    hipLaunchKernelGGL(cull_pack_kernel, dim3((unsigned)((words + per - 1) / per)), dim3(kCullThreads), 0, s, p, words);
  }
  {
    TimingScope ts_("cull_hdilate_kernel", 2, 0, words, p.H, p.W, 0, s, 2.0 * wb);
    hipLaunchKernelGGL(cull_hdilate_kernel, dim3(blocks), dim3(kCullThreads), 0, s, p, words);
  }
  {
    // (every word is read by up to 2r + 1 lanes; from memory once)
    TimingScope ts_("cull_vdilate_kernel", 2, 0, words, p.H, rows, 0, s, 2.0 * wb);
    hipLaunchKernelGGL(cull_vdilate_kernel, dim3(blocks), dim3(kCullThreads), 0, s, p, words);
  }
  CNR_LAUNCH_CHECK("mask_dilate");
}

__global__ __launch_bounds__(kCullThreads) void cull_votes_kernel(const MeshViewVotes p) {
  __shared__ RasterCam cams[kCullViews];
  const long v = (long)blockIdx.x * kCullThreads + threadIdx.x;
  const bool live = v < p.V;
  float x[3] = {0.0f, 0.0f, 0.0f};
  if (live) { x[0] = p.vertices[v * 3]; x[1] = p.vertices[v * 3 + 1]; x[2] = p.vertices[v * 3 + 2]; }
  const float tol1 = 1.0f + p.depth_tol;
  int c[4] = {0, 0, 0, 0};
  for (long n0 = 0; n0 < p.n_views; n0 += kCullViews) {
    const int nv = p.n_views - n0 < kCullViews ? (int)(p.n_views - n0) : kCullViews;
    __syncthreads();      // (the cameras of the trip before are no longer read)
    if ((int)threadIdx.x < nv) {
      const long n = n0 + threadIdx.x;
      cams[threadIdx.x] = raster_cam_of(p.c2w + n * 16, p.focal + n * 2, p.origin, p.radius, p.H, p.W);
    }
    __syncthreads();
    if (live)
      for (int k = 0; k < nv; ++k) {
        const long n = n0 + k;
        cull_vote(cams[k], x, p.opengl, p.z_near, p.H, p.W, p.Wq, p.mask_bits ? p.mask_bits + n * p.H * p.Wq : nullptr,
                  p.depth ? p.depth + n * p.H * p.W : nullptr, tol1, c);
      }
  }
  if (live) {
    int4* at = reinterpret_cast<int4*>(p.counts) + v;
    int4 o = *at;
    o.x += c[0]; o.y += c[1]; o.z += c[2]; o.w += c[3];
    *at = o;
  }
}

void be_mesh_view_votes(const MeshViewVotes& p, cnr_stream s) {
  // per vertex 12 bytes in and its 16-byte row in and out; per (vertex, view) at most one mask word and one depth value
  const double per_pair = (p.mask_bits ? 8.0 : 0.0) + (p.depth ? 4.0 : 0.0);
  TimingScope ts_("cull_votes_kernel", 2, 0, p.V, p.H, p.W, (int)(p.n_views > 0x7fffffff ? 0x7fffffff : p.n_views), s,
                  (44.0 + per_pair * (double)p.n_views) * (double)p.V);
  hipLaunchKernelGGL(cull_votes_kernel, dim3((unsigned)((p.V + kCullThreads - 1) / kCullThreads)), dim3(kCullThreads), 0, s, p);
  CNR_LAUNCH_CHECK("mesh_view_votes");
}

__global__ __launch_bounds__(kCullThreads) void cull_clear_kernel(const MeshCullSelect p) {
  const long v = (long)blockIdx.x * kCullThreads + threadIdx.x;
  if (v == 0) p.dropped[0] = 0;
  if (v < p.V) p.keep_vertex[v] = 0;
}

__global__ __launch_bounds__(kCullThreads) void cull_faces_kernel(const MeshCullSelect p) {
  const long f = (long)blockIdx.x * kCullThreads + threadIdx.x;
  const int k = f < p.F ? cull_face(p, f) : 0;
  (void)wave_append(f < p.F && k < 0, p.dropped);
  if (f >= p.F) return;
  p.keep_face[f] = k > 0 ? 1 : 0;
  if (k > 0) cull_mark(p, f);
}

void be_mesh_cull_select(const MeshCullSelect& p, cnr_stream s) {
  const double V = (double)p.V, F = (double)p.F;
  {
    TimingScope ts_("cull_clear_kernel", 2, 0, p.V, 0, 0, 0, s, V + 4.0);
    hipLaunchKernelGGL(cull_clear_kernel, dim3((unsigned)((p.V + kCullThreads - 1) / kCullThreads) + (p.V == 0)), dim3(kCullThreads), 0, s, p);
  }
  if (p.F > 0) {
    // (12 bytes of indices, three 16-byte rows of counts, the flag; the marks of a kept face: up to 3 bytes)
    TimingScope ts_("cull_faces_kernel", 2, 0, p.F, 0, 0, 0, s, 64.0 * F);
    hipLaunchKernelGGL(cull_faces_kernel, dim3((unsigned)((p.F + kCullThreads - 1) / kCullThreads)), dim3(kCullThreads), 0, s, p);
  }
  mesh_keep_scan({p.keep_vertex, p.keep_face, p.V, p.F, p.vertex_map, p.face_map, p.totals}, s);
  CNR_LAUNCH_CHECK("mesh_cull_select");
}

}  // namespace cnr
