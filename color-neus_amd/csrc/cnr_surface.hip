// Mesh surface sampling and exact point-to-mesh distance for gfx950 (cnr_mesh_area_cdf / cnr_mesh_sample / cnr_point_mesh_distance): the
// kernels behind the surface-to-surface mesh metrics.  The per-element arithmetic is cnr_surface.h's, shared with the CPU emulation.
//
//   surf_area_kernel       one face per lane: its area bits (or the invalid mark) into cdf[f]; the largest by a 64-bit integer atomic max
//   surf_cdf_scan_kernel   ONE workgroup carries an inclusive 64-bit integer scan of the weights through cdf[] in trips of kMeshScanChunk faces
//                          (meshcc_scan_kernel's form), counting the faces of weight 0 and the invalid ones in two more channels of the same scan
//   surf_sample_kernel     one sample per lane: Philox words, binary search in cdf[], barycentric fold, point
//   surf_dist_kernel       nn_search_kernel's shape.  256 threads, every lane keeps kSurfQ queries in registers; the block's part of the face range
//                          goes tile by tile through LDS as SurfTri records (a, ab, ac and their dot products: 48 bytes, staged by one lane per
//                          face), read back by all lanes at the same address (a broadcast: three ds_read_b128 serve 64 lanes x kSurfQ closest-point
//                          evaluations).  The pair loop is branch-free VALU work (surf_closest: selects over Ericson's regions, one division).
//                          blockIdx.y splits the face range; every block folds its best keys into keys[query] with a 64-bit unsigned integer
//                          atomic min, so the result is the same bits for every split.
//   surf_finish_kernel     keys -> dist2 / face and, when wanted, the closest point (recomputed on the winning face)
#include <hip/hip_runtime.h>

#include "cnr_surface.h"
#include "cnr_hip_util.h"
#include "cnr_wave.h"

namespace cnr {

constexpr int kSurfThreads = 256;
constexpr int kSurfQ = 2;              // queries per lane
constexpr int kSurfTile = 256;         // faces per LDS tile (12 KB), one per thread
constexpr long kSurfBlocksWanted = 2048;   // 8 resident blocks per CU x 256 CUs

__global__ __launch_bounds__(kSurfThreads) void surf_area_kernel(const MeshAreaCdf p) {
  const long f = (long)blockIdx.x * kSurfThreads + threadIdx.x;
  if (f >= p.F) return;
  const unsigned long long bits = surf_area_bits(p, f);
  p.cdf[f] = bits;
  if (bits != kSurfInvalid) {
    // (a bid below the best so far cannot win: only the others pay for an atomic on the one word)
    unsigned long long* best = reinterpret_cast<unsigned long long*>(p.summary + 3);
    if (bits > __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(best, bits);
  }
}

__global__ __launch_bounds__(kMeshScanThreads) void surf_cdf_scan_kernel(const MeshAreaCdf p) {
  __shared__ unsigned long long wsum[3][kMeshScanThreads / 64];
  __shared__ unsigned long long carry[3];
  if (threadIdx.x < 3) carry[threadIdx.x] = 0ull;
  __syncthreads();
  const unsigned amax_bits = (unsigned)p.summary[3];
  for (long base = 0; base < p.F; base += kMeshScanChunk) {
    const long i0 = base + (long)threadIdx.x * kMeshScanPer;
    unsigned long long w[kMeshScanPer];
    unsigned long long x[3] = {0ull, 0ull, 0ull};   // {weight, faces of weight 0, invalid faces}
#pragma unroll
    for (int j = 0; j < kMeshScanPer; ++j) {
      w[j] = 0ull;
      if (i0 + j < p.F) {
        const unsigned long long bits = p.cdf[i0 + j];
        w[j] = surf_weight(bits, amax_bits);
        x[0] += w[j]; x[1] += w[j] == 0ull; x[2] += bits == kSurfInvalid;
      }
    }
    unsigned long long excl[3];
    block_excl_scan<kMeshScanThreads / 64, 3, unsigned long long>(x, excl, wsum, carry);
    unsigned long long at = excl[0];
#pragma unroll
    for (int j = 0; j < kMeshScanPer; ++j) { at += w[j]; if (i0 + j < p.F) p.cdf[i0 + j] = at; }
  }
  if (threadIdx.x < 3) p.summary[threadIdx.x] = (long long)carry[threadIdx.x];
}

void be_mesh_area_cdf(const MeshAreaCdf& p, cnr_stream s) {
  const double F = (double)p.F;
  hipError_t e = hipMemsetAsync(p.summary, 0, 4 * sizeof(long long), s);
  if (e != hipSuccess && g_first_error == hipSuccess) { g_first_error = e; g_first_error_where = "mesh_area_cdf memset"; }
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

__global__ __launch_bounds__(kSurfThreads) void surf_dist_kernel(const PointMeshDist p, long tiles_per_split) {
  __shared__ SurfTri tile[kSurfTile];
  const long q0 = (long)blockIdx.x * (kSurfThreads * kSurfQ) + threadIdx.x;
  float qx[kSurfQ], qy[kSurfQ], qz[kSurfQ], best[kSurfQ];
  int besti[kSurfQ];
#pragma unroll
  for (int k = 0; k < kSurfQ; ++k) {
    long i = q0 + (long)k * kSurfThreads;
    if (i >= p.n) i = p.n - 1;     // lanes past the end repeat the last query and write nothing
    qx[k] = p.query[i * 3]; qy[k] = p.query[i * 3 + 1]; qz[k] = p.query[i * 3 + 2];
    best[k] = INFINITY; besti[k] = -1;
  }
  const long ntiles = (p.F + kSurfTile - 1) / kSurfTile;
  const long t0 = (long)blockIdx.y * tiles_per_split;
  const long t1 = t0 + tiles_per_split < ntiles ? t0 + tiles_per_split : ntiles;
  for (long t = t0; t < t1; ++t) {
    const long jb = t * kSurfTile;
    __syncthreads();               // every lane is done with the previous tile
    {
      const long j = jb + threadIdx.x;
      int idx[3] = {-1, -1, -1};   // past the end of the faces: an invalid record (never read: the pair loop stops at the last face)
      if (j < p.F) { idx[0] = p.triangles[j * 3]; idx[1] = p.triangles[j * 3 + 1]; idx[2] = p.triangles[j * 3 + 2]; }
      tile[threadIdx.x] = surf_record(p.vertices, p.V, idx);
    }
    __syncthreads();
    const int count = p.F - jb < (long)kSurfTile ? (int)(p.F - jb) : kSurfTile;
    const unsigned jb32 = (unsigned)jb;
    // not unrolled: two faces in flight hold 97 VGPRs and spill the regions' lane masks out of the SGPRs; one holds 64 VGPRs (8 waves per SIMD)
#pragma unroll 1
    for (int jj = 0; jj < count; ++jj) {
      const SurfTri r = tile[jj];
      const int j = (int)(jb32 + (unsigned)jj);
#pragma unroll
      for (int k = 0; k < kSurfQ; ++k) nn_update(surf_dist2(r, qx[k], qy[k], qz[k]), j, best[k], besti[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < kSurfQ; ++k) {
    const long i = q0 + (long)k * kSurfThreads;
    if (i < p.n && besti[k] >= 0) atomicMin(&p.keys[i], nn_key(best[k], besti[k]));
  }
}

__global__ __launch_bounds__(kSurfThreads) void surf_finish_kernel(const PointMeshDist p) {
  const long i = (long)blockIdx.x * kSurfThreads + threadIdx.x;
  if (i < p.n) surf_finish(p, i);
}

void be_point_mesh_distance(const PointMeshDist& p, cnr_stream s) {
  const long ntiles = (p.F + kSurfTile - 1) / kSurfTile;
  const long qblocks = (p.n + kSurfThreads * kSurfQ - 1) / (kSurfThreads * kSurfQ);
  long want = kSurfBlocksWanted / qblocks;
  if (want < 1) want = 1;
  const long tiles_per_split = (ntiles + want - 1) / want;
  const long nsplit = (ntiles + tiles_per_split - 1) / tiles_per_split;   // <= kSurfBlocksWanted: fits gridDim.y
  hipError_t e = hipMemsetAsync(p.keys, 0xff, (size_t)p.n * sizeof(unsigned long long), s);   // kNnNoKey
  if (e != hipSuccess && g_first_error == hipSuccess) { g_first_error = e; g_first_error_where = "point_mesh_distance memset"; }
  {
    TimingScope ts_("surf_dist_kernel", 2, 0, p.n, (int)p.F, 3, (int)nsplit, s,
                    12.0 * (double)p.n + 48.0 * (double)p.F * (double)qblocks);
    hipLaunchKernelGGL(surf_dist_kernel, dim3((unsigned)qblocks, (unsigned)nsplit), dim3(kSurfThreads), 0, s, p, tiles_per_split);
  }
  {
    TimingScope ts_("surf_finish_kernel", 2, 0, p.n, 0, 0, 0, s, (p.closest ? 76.0 : 16.0) * (double)p.n);
    hipLaunchKernelGGL(surf_finish_kernel, dim3((unsigned)((p.n + kSurfThreads - 1) / kSurfThreads)), dim3(kSurfThreads), 0, s, p);
  }
  CNR_LAUNCH_CHECK("point_mesh_distance");
}

}  // namespace cnr
