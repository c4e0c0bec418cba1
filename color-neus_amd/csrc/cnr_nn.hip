// Exact brute-force nearest-neighbour search of 3-D point sets for gfx950 (cnr_nn_search): the hot path of the Chamfer / F-score mesh metrics.
//
//   nn_search_kernel   256 threads, every lane keeps kNnQ queries in registers; the block's part of the target range goes tile by tile through LDS as
//                      float4 and is read back by all lanes at the same address (a broadcast: one ds_read_b128 serves 64 lanes x kNnQ distance
//                      evaluations).  The pair loop is VALU work only: 3 subtractions, 3 multiplications, 2 additions, 1 compare, 2 selects -- no FMA,
//                      so that the distance is the separately rounded fp32 expression the CPU emulation evaluates (nn_dist2 in cnr_nn.h).
//                      blockIdx.y splits the target range, so that few queries against many targets still fill the chip; every block folds its
//                      best keys into keys[query] with a 64-bit unsigned integer atomic min (order-independent: DESIGN 5).
//   nn_unpack_kernel   keys -> dist2 / idx
#include <hip/hip_runtime.h>

#include "cnr_nn.h"
#include "cnr_hip_util.h"

namespace cnr {

constexpr int kNnThreads = 256;
constexpr int kNnQ = 4;            // queries per lane
constexpr int kNnTile = 1024;      // targets per LDS tile (16 KB)
constexpr long kNnBlocksWanted = 2048;   // 8 resident blocks per CU x 256 CUs

__global__ __launch_bounds__(kNnThreads) void nn_search_kernel(const NnSearch p, long tiles_per_split) {
  __shared__ f4 tile[kNnTile];
  const long q0 = (long)blockIdx.x * (kNnThreads * kNnQ) + threadIdx.x;
  float qx[kNnQ], qy[kNnQ], qz[kNnQ], best[kNnQ];
  int besti[kNnQ];
#pragma unroll
  for (int k = 0; k < kNnQ; ++k) {
    long i = q0 + (long)k * kNnThreads;
    if (i >= p.n) i = p.n - 1;     // lanes past the end repeat the last query and write nothing
    qx[k] = p.query[i * 3]; qy[k] = p.query[i * 3 + 1]; qz[k] = p.query[i * 3 + 2];
    best[k] = INFINITY; besti[k] = -1;
  }
  const long ntiles = (p.m + kNnTile - 1) / kNnTile;
  const long t0 = (long)blockIdx.y * tiles_per_split;
  const long t1 = t0 + tiles_per_split < ntiles ? t0 + tiles_per_split : ntiles;
  const float nan = __builtin_nanf("");
  for (long t = t0; t < t1; ++t) {
    const long jb = t * kNnTile;
    __syncthreads();               // every lane is done with the previous tile
#pragma unroll
    for (int k = 0; k < kNnTile / kNnThreads; ++k) {
      const int jj = threadIdx.x + k * kNnThreads;
      const long j = jb + jj;
      f4 v = {nan, nan, nan, 0.0f};   // past the end of the targets: a NaN distance never wins
      if (j < p.m) { v.x = p.target[j * 3]; v.y = p.target[j * 3 + 1]; v.z = p.target[j * 3 + 2]; }
      tile[jj] = v;
    }
    __syncthreads();
    const unsigned jb32 = (unsigned)jb;
#pragma unroll 8
    for (int jj = 0; jj < kNnTile; ++jj) {
      const f4 v = tile[jj];
      const int j = (int)(jb32 + (unsigned)jj);
#pragma unroll
      for (int k = 0; k < kNnQ; ++k) nn_update(nn_dist2(qx[k], qy[k], qz[k], v.x, v.y, v.z), j, best[k], besti[k]);
    }
    // rare: a query that has taken nothing yet (every d2 so far NaN or +inf) looks for the first +inf of this tile
#pragma unroll
    for (int k = 0; k < kNnQ; ++k) {
      if (besti[k] < 0) {
        for (int jj = 0; jj < kNnTile; ++jj) {
          const f4 v = tile[jj];
          nn_update_inf(nn_dist2(qx[k], qy[k], qz[k], v.x, v.y, v.z), (int)(jb32 + (unsigned)jj), best[k], besti[k]);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kNnQ; ++k) {
    const long i = q0 + (long)k * kNnThreads;
    if (i < p.n && besti[k] >= 0) atomicMin(&p.keys[i], nn_key(best[k], besti[k]));
  }
}

__global__ __launch_bounds__(256) void nn_unpack_kernel(const NnSearch p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < p.n) nn_unpack(p.keys[i], &p.dist2[i], &p.idx[i]);
}

void be_nn_search(const NnSearch& p, cnr_stream s) {
  const long ntiles = (p.m + kNnTile - 1) / kNnTile;
  const long qblocks = (p.n + kNnThreads * kNnQ - 1) / (kNnThreads * kNnQ);
  long want = kNnBlocksWanted / qblocks;
  if (want < 1) want = 1;
  const long tiles_per_split = (ntiles + want - 1) / want;
  const long nsplit = (ntiles + tiles_per_split - 1) / tiles_per_split;   // <= kNnBlocksWanted: fits gridDim.y
  hipError_t e = hipMemsetAsync(p.keys, 0xff, (size_t)p.n * sizeof(unsigned long long), s);   // kNnNoKey
  if (e != hipSuccess && g_first_error == hipSuccess) { g_first_error = e; g_first_error_where = "nn_search memset"; }
  {
    TimingScope ts_("nn_search_kernel", 2, 0, p.n, (int)p.m, 3, (int)nsplit, s, 12.0 * (double)p.n + 12.0 * (double)p.m * (double)qblocks);
    hipLaunchKernelGGL(nn_search_kernel, dim3((unsigned)qblocks, (unsigned)nsplit), dim3(kNnThreads), 0, s, p, tiles_per_split);
  }
  {
    TimingScope ts_("nn_unpack_kernel", 2, 0, p.n, 0, 0, 0, s, 16.0 * (double)p.n);
    hipLaunchKernelGGL(nn_unpack_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p);
  }
  CNR_LAUNCH_CHECK("nn_search");
}

}  // namespace cnr
