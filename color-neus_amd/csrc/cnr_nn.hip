// Exact brute-force nearest-neighbour search of 3-D point sets for gfx950 (cnr_nn_search): the hot path of the Chamfer / F-score mesh metrics.
//
//   nn_search_kernel   closest_search (cnr_search.h) over the target points.  The tile holds them as float4, read back by all lanes at the same
//                      address (a broadcast: one ds_read_b128 serves 64 lanes x kQ distance evaluations).  The pair loop is VALU work only:
//                      3 subtractions, 3 multiplications, 2 additions, 1 compare, 2 selects -- no FMA, so that the distance is the separately
//                      rounded fp32 expression the CPU emulation evaluates (nn_dist2 in cnr_nn.h).
//   nn_unpack_kernel   keys -> dist2 / idx
#include <hip/hip_runtime.h>

#include "cnr_nn.h"
#include "cnr_hip_util.h"
#include "cnr_search.h"

namespace cnr {

// the candidates of nn_search_kernel (closest_search, cnr_search.h): target points as float4, 1024 per LDS tile (16 KB), 4 queries per lane
struct NnPoints {
  using Record = f4;
  static constexpr int kThreads = 256, kQ = 4, kTile = 1024;
  static __device__ __forceinline__ long count(const NnSearch& p) { return p.m; }
  static __device__ __forceinline__ void stage(const NnSearch& p, long jb, f4* tile) {
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int k = 0; k < kTile / kThreads; ++k) {
      const int jj = threadIdx.x + k * kThreads;
      const long j = jb + jj;
      f4 v = {nan, nan, nan, 0.0f};   // past the end of the targets: a NaN distance never wins
      if (j < p.m) { v.x = p.target[j * 3]; v.y = p.target[j * 3 + 1]; v.z = p.target[j * 3 + 2]; }
      tile[jj] = v;
    }
  }
  static __device__ __forceinline__ void scan(const NnSearch&, long jb, const f4* tile, const float (&qx)[kQ], const float (&qy)[kQ],
                                              const float (&qz)[kQ], float (&best_io)[kQ], int (&besti_io)[kQ]) {
    float best[kQ]; int besti[kQ];   // (in locals: updated through the references, the kernel holds 65 VGPRs and 7 waves per SIMD; so 62 and 8)
#pragma unroll
    for (int k = 0; k < kQ; ++k) { best[k] = best_io[k]; besti[k] = besti_io[k]; }
    const unsigned jb32 = (unsigned)jb;
#pragma unroll 8
    for (int jj = 0; jj < kTile; ++jj) {
      const f4 v = tile[jj];
      const int j = (int)(jb32 + (unsigned)jj);
#pragma unroll
      for (int k = 0; k < kQ; ++k) nn_update(nn_dist2(qx[k], qy[k], qz[k], v.x, v.y, v.z), j, best[k], besti[k]);
    }
    // rare: a query that has taken nothing yet (every d2 so far NaN or +inf) looks for the first +inf of this tile
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
      if (besti[k] < 0) {
        for (int jj = 0; jj < kTile; ++jj) {
          const f4 v = tile[jj];
          nn_update_inf(nn_dist2(qx[k], qy[k], qz[k], v.x, v.y, v.z), (int)(jb32 + (unsigned)jj), best[k], besti[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kQ; ++k) { best_io[k] = best[k]; besti_io[k] = besti[k]; }
  }
};

__global__ __launch_bounds__(NnPoints::kThreads) void nn_search_kernel(const NnSearch p, long tiles_per_split) {
  __shared__ f4 tile[NnPoints::kTile];
  closest_search<NnPoints>(p, tiles_per_split, tile);
}

__global__ __launch_bounds__(256) void nn_unpack_kernel(const NnSearch p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < p.n) nn_unpack(p.keys[i], &p.dist2[i], &p.idx[i]);
}

void be_nn_search(const NnSearch& p, cnr_stream s) {
  const SearchSplit sp = search_split(p.n, NnPoints::kThreads * NnPoints::kQ, (p.m + NnPoints::kTile - 1) / NnPoints::kTile);
  device_fill(p.keys, 0xff, (size_t)p.n * sizeof(unsigned long long), s, "nn_search memset");   // kNnNoKey
  {
    TimingScope ts_("nn_search_kernel", 2, 0, p.n, (int)p.m, 3, (int)sp.nsplit, s, 12.0 * (double)p.n + 12.0 * (double)p.m * (double)sp.qblocks);
    hipLaunchKernelGGL(nn_search_kernel, dim3((unsigned)sp.qblocks, (unsigned)sp.nsplit), dim3(NnPoints::kThreads), 0, s, p, sp.tiles_per_split);
  }
  {
    TimingScope ts_("nn_unpack_kernel", 2, 0, p.n, 0, 0, 0, s, 16.0 * (double)p.n);
    hipLaunchKernelGGL(nn_unpack_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p);
  }
  CNR_LAUNCH_CHECK("nn_search");
}

}  // namespace cnr
