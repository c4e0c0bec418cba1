// The exact brute-force closest-candidate search of the HIP units (nn_search_kernel: the nearest point; surf_dist_kernel: the closest face):
// how the launch splits the candidate range, and the kernel's frame around a kind's own tile staging and tile scan.  Every lane keeps kQ queries
// in registers; the block's part of the candidate range goes tile by tile through LDS as the kind's records and is read back by all lanes at the
// same address (a broadcast).  blockIdx.y splits the candidate range, so that few queries against many candidates still fill the chip; every
// block folds its best keys into keys[query] (filled with kNnNoKey, 0xff bytes, in front of the launch) with a 64-bit unsigned integer atomic
// min (nn_key, cnr_nn.h), so the result is the same bits for every split.
#pragma once
#include <hip/hip_runtime.h>
#include "cnr_nn.h"

namespace cnr {

// grid = (qblocks, nsplit); the block (x, y) scans the tiles [y * tiles_per_split, (y + 1) * tiles_per_split) of the candidates
struct SearchSplit { long qblocks, tiles_per_split, nsplit; };
inline SearchSplit search_split(long n_queries, int queries_per_block, long n_tiles) {
  constexpr long kSearchBlocksWanted = 2048;   // 8 resident blocks per CU x 256 CUs
  const long qblocks = (n_queries + queries_per_block - 1) / queries_per_block;
  long want = kSearchBlocksWanted / qblocks;
  if (want < 1) want = 1;
  const long tiles_per_split = (n_tiles + want - 1) / want;
  return {qblocks, tiles_per_split, (n_tiles + tiles_per_split - 1) / tiles_per_split};   // nsplit <= kSearchBlocksWanted: fits gridDim.y
}

// A Kind states: Record (what a tile holds), kThreads, kQ (queries per lane), kTile (records per tile) and, all static __device__,
//   count(p)                                     the number of candidates (p: the launch's descriptor, with query [n][3], n and keys [n])
//   stage(p, jb, tile)                           the records jb .. jb + kTile - 1 from global memory into the tile (between the two barriers)
//   scan(p, jb, tile, qx, qy, qz, best, besti)   the staged tile against the lane's kQ queries: nn_update in ascending candidate order
template <class Kind, class Param>
__device__ __forceinline__ void closest_search(const Param& p, long tiles_per_split, typename Kind::Record* tile) {
  constexpr int kQ = Kind::kQ, kThreads = Kind::kThreads;
  const long q0 = (long)blockIdx.x * (kThreads * kQ) + threadIdx.x;
  float qx[kQ], qy[kQ], qz[kQ], best[kQ];
  int besti[kQ];
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    long i = q0 + (long)k * kThreads;
    if (i >= p.n) i = p.n - 1;     // lanes past the end repeat the last query and write nothing
    qx[k] = p.query[i * 3]; qy[k] = p.query[i * 3 + 1]; qz[k] = p.query[i * 3 + 2];
    best[k] = INFINITY; besti[k] = -1;
  }
  const long ntiles = (Kind::count(p) + Kind::kTile - 1) / Kind::kTile;
  const long t0 = (long)blockIdx.y * tiles_per_split;
  const long t1 = t0 + tiles_per_split < ntiles ? t0 + tiles_per_split : ntiles;
  for (long t = t0; t < t1; ++t) {
    const long jb = t * Kind::kTile;
    __syncthreads();               // every lane is done with the previous tile
    Kind::stage(p, jb, tile);
    __syncthreads();
    Kind::scan(p, jb, tile, qx, qy, qz, best, besti);
  }
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    const long i = q0 + (long)k * kThreads;
    if (i < p.n && besti[k] >= 0) atomicMin(&p.keys[i], nn_key(best[k], besti[k]));
  }
}

}  // namespace cnr
