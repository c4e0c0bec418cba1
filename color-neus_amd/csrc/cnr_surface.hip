// Mesh surface sampling and exact point-to-mesh distance for gfx950 (cnr_mesh_area_cdf / cnr_mesh_sample / cnr_point_mesh_distance): the
// kernels behind the surface-to-surface mesh metrics.  The per-element arithmetic is cnr_surface.h's, shared with the CPU emulation.
//
//   surf_area_kernel       one face per lane: its area bits (or the invalid mark) into cdf[f]; the largest by a 64-bit integer atomic max
//   surf_cdf_scan_kernel   ONE workgroup carries an inclusive 64-bit integer scan of the weights through cdf[] in trips of kMeshScanChunk faces
//                          (block_carried_scan), counting the faces of weight 0 and the invalid ones in two more channels of the same scan
//   surf_sample_kernel     one sample per lane: Philox words, binary search in cdf[], barycentric fold, point
//   surf_dist_kernel       closest_search (cnr_search.h) over the faces.  The tile holds SurfTri records (a, ab, ac and their dot products: 48
//                          bytes, staged by one lane per face), read back by all lanes at the same address (a broadcast: three ds_read_b128
//                          serve 64 lanes x kQ closest-point evaluations).  The pair loop is branch-free VALU work (surf_closest: selects over
//                          Ericson's regions, one division).
//   surf_finish_kernel     keys -> dist2 / face and, when wanted, the closest point (recomputed on the winning face)
#include <hip/hip_runtime.h>

#include "cnr_surface.h"
#include "cnr_hip_util.h"
#include "cnr_search.h"
#include "cnr_wave.h"

namespace cnr {

constexpr int kSurfThreads = 256;
constexpr int kSurfQ = 2;              // queries per lane
constexpr int kSurfTile = 256;         // faces per LDS tile (12 KB), one per thread

__global__ __launch_bounds__(kSurfThreads) void surf_area_kernel(const MeshAreaCdf p) {
  const long f = (long)blockIdx.x * kSurfThreads + threadIdx.x;
  if (f >= p.F) return;
  const unsigned long long bits = surf_area_bits(p, f);
  p.cdf[f] = bits;
  if (bits != kSurfInvalid) bid_max(reinterpret_cast<unsigned long long*>(p.summary + 3), bits);
}

__global__ __launch_bounds__(kMeshScanThreads) void surf_cdf_scan_kernel(const MeshAreaCdf p) {
  __shared__ unsigned long long wsum[3][kMeshScanThreads / 64];
  __shared__ unsigned long long carry[3];
  const unsigned amax_bits = (unsigned)p.summary[3];
  using Sums = unsigned long long[3];   // {weight, faces of weight 0, invalid faces}
  block_carried_scan<kMeshScanThreads / 64, kMeshScanPer, 3, unsigned long long>(p.F, wsum, carry,
      [&](long i, Sums& x) { const unsigned long long bits = p.cdf[i], w = surf_weight(bits, amax_bits); x[0] += w; x[1] += w == 0ull; x[2] += bits == kSurfInvalid; return w; },
      [&](long i, Sums& at, unsigned long long w) { at[0] += w; p.cdf[i] = at[0]; });   // the inclusive value
  if (threadIdx.x < 3) p.summary[threadIdx.x] = (long long)carry[threadIdx.x];
}

void be_mesh_area_cdf(const MeshAreaCdf& p, cnr_stream s) {
  const double F = (double)p.F;
  device_fill(p.summary, 0, 4 * sizeof(long long), s, "mesh_area_cdf memset");
  {
    TimingScope ts_("surf_area_kernel", 2, 0, p.F, 0, 0, 0, s, 56.0 * F);
    hipLaunchKernelGGL(surf_area_kernel, dim3((unsigned)((p.F + kSurfThreads - 1) / kSurfThreads)), dim3(kSurfThreads), 0, s, p);
  }
  {
    TimingScope ts_("surf_cdf_scan_kernel", 2, 0, p.F, 0, 0, 0, s, 16.0 * F + 32.0);
    hipLaunchKernelGGL(surf_cdf_scan_kernel, dim3(1), dim3(kMeshScanThreads), 0, s, p);
  }
  CNR_LAUNCH_CHECK("mesh_area_cdf");
}

__global__ __launch_bounds__(kSurfThreads) void surf_sample_kernel(const MeshSample p) {
  for (long i = (long)blockIdx.x * kSurfThreads + threadIdx.x; i < p.n; i += (long)gridDim.x * kSurfThreads) surf_sample(p, i);
}

void be_mesh_sample(const MeshSample& p, cnr_stream s) {
  if (p.n <= 0) return;
  long blocks = (p.n + kSurfThreads - 1) / kSurfThreads;
  if (blocks > 8192) blocks = 8192;
  {
    TimingScope ts_("surf_sample_kernel", 2, 0, p.n, 0, 0, 0, s, (p.bary ? 72.0 : 64.0) * (double)p.n);
    hipLaunchKernelGGL(surf_sample_kernel, dim3((unsigned)blocks), dim3(kSurfThreads), 0, s, p);
  }
  CNR_LAUNCH_CHECK("mesh_sample");
}

// the candidates of surf_dist_kernel (closest_search, cnr_search.h): faces as SurfTri records
struct SurfFaces {
  using Record = SurfTri;
  static constexpr int kThreads = kSurfThreads, kQ = kSurfQ, kTile = kSurfTile;
  static_assert(kTile == kThreads, "one face per thread");
  static __device__ __forceinline__ long count(const PointMeshDist& p) { return p.F; }
  static __device__ __forceinline__ void stage(const PointMeshDist& p, long jb, SurfTri* tile) {
    const long j = jb + threadIdx.x;
    int idx[3] = {-1, -1, -1};   // past the end of the faces: an invalid record (never read: the pair loop stops at the last face)
    if (j < p.F) { idx[0] = p.triangles[j * 3]; idx[1] = p.triangles[j * 3 + 1]; idx[2] = p.triangles[j * 3 + 2]; }
    tile[threadIdx.x] = surf_record(p.vertices, p.V, idx);
  }
  static __device__ __forceinline__ void scan(const PointMeshDist& p, long jb, const SurfTri* tile, const float (&qx)[kQ], const float (&qy)[kQ],
                                              const float (&qz)[kQ], float (&best)[kQ], int (&besti)[kQ]) {
    const int count = p.F - jb < (long)kTile ? (int)(p.F - jb) : kTile;
    const unsigned jb32 = (unsigned)jb;
    // not unrolled: two faces in flight hold 97 VGPRs and spill the regions' lane masks out of the SGPRs; one holds 64 VGPRs (8 waves per SIMD)
#pragma unroll 1
    for (int jj = 0; jj < count; ++jj) {
      const SurfTri r = tile[jj];
      const int j = (int)(jb32 + (unsigned)jj);
#pragma unroll
      for (int k = 0; k < kQ; ++k) nn_update(surf_dist2(r, qx[k], qy[k], qz[k]), j, best[k], besti[k]);
    }
  }
};

__global__ __launch_bounds__(kSurfThreads) void surf_dist_kernel(const PointMeshDist p, long tiles_per_split) {
  __shared__ SurfTri tile[kSurfTile];
  closest_search<SurfFaces>(p, tiles_per_split, tile);
}

__global__ __launch_bounds__(kSurfThreads) void surf_finish_kernel(const PointMeshDist p) {
  const long i = (long)blockIdx.x * kSurfThreads + threadIdx.x;
  if (i < p.n) surf_finish(p, i);
}

void be_point_mesh_distance(const PointMeshDist& p, cnr_stream s) {
  const SearchSplit sp = search_split(p.n, kSurfThreads * kSurfQ, (p.F + kSurfTile - 1) / kSurfTile);
  device_fill(p.keys, 0xff, (size_t)p.n * sizeof(unsigned long long), s, "point_mesh_distance memset");   // kNnNoKey
  {
    TimingScope ts_("surf_dist_kernel", 2, 0, p.n, (int)p.F, 3, (int)sp.nsplit, s,
                    12.0 * (double)p.n + 48.0 * (double)p.F * (double)sp.qblocks);
    hipLaunchKernelGGL(surf_dist_kernel, dim3((unsigned)sp.qblocks, (unsigned)sp.nsplit), dim3(kSurfThreads), 0, s, p, sp.tiles_per_split);
  }
  {
    TimingScope ts_("surf_finish_kernel", 2, 0, p.n, 0, 0, 0, s, (p.closest ? 76.0 : 16.0) * (double)p.n);
    hipLaunchKernelGGL(surf_finish_kernel, dim3((unsigned)((p.n + kSurfThreads - 1) / kSurfThreads)), dim3(kSurfThreads), 0, s, p);
  }
  CNR_LAUNCH_CHECK("point_mesh_distance");
}

}  // namespace cnr
