// ICP registration for gfx950 (cnr_icp): the loop around the existing searches, kept on the device.  The per-element arithmetic and the solve
// are cnr_register.h's, shared with the CPU emulation; the searches are be_nn_search / be_point_mesh_distance as they stand.
//
//   icp_move_kernel      one point per lane: the fp32 map from the 13 doubles of the transform (an L2 broadcast), 12 bytes in, 12 out; with a
//                        previous correspondence, idx_i into the bits of matched[i][0] (the search overwrites idx)
//   icp_moments_kernel   one chunk of 256 points per workgroup: the gather of the matched point (or the closest point of the matched face),
//                        the eighteen fp64 terms in registers, then THE tree x[j] += x[j + h], h = 128 .. 1: two LDS levels across the four
//                        waves in three passes of six planes (6 KB, not the 36 KB of all planes at once), six shuffle levels in wave 0
//                        (wave_fold_down).  Lane 0 writes the chunk's row of partials; the two counts are integers: a block sum, one 64-bit
//                        atomic add each into the history row
//   icp_solve_kernel     ONE wave: 18 lanes add the chunks' rows in chunk order, lane 0 runs icp_finish (Horn's matrix, Jacobi, scale,
//                        translation).  Latency work behind the moments launch in stream order: no flags, no spinning
#include <hip/hip_runtime.h>

#include "cnr_register.h"
#include "cnr_hip_util.h"
#include "cnr_wave.h"

namespace cnr {

constexpr int kIcpGroup = 6;   // planes per LDS pass of the moments tree

__global__ __launch_bounds__(256) void icp_move_kernel(const IcpStep p) {
  const IcpMap k = icp_map(p.transform);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (long)gridDim.x * 256) icp_move(p, k, i);
}

__global__ __launch_bounds__(kIcpChunk) void icp_moments_kernel(const IcpStep p) {
  __shared__ double plane[kIcpGroup][kIcpChunk / 2];
  __shared__ int count4[4];
  const int t = threadIdx.x;
  const long i = (long)blockIdx.x * kIcpChunk + t;
  double x[kIcpTerms];
  int inlier = 0, changed = 0;
  if (i < p.n) {
    icp_pair(p, i, x, &inlier, &changed);
  } else {
#pragma unroll
    for (int c = 0; c < kIcpTerms; ++c) x[c] = 0.0;   // the chunk is padded with zeros
  }
#pragma unroll
  for (int g = 0; g < kIcpTerms; g += kIcpGroup) {
    __syncthreads();               // every lane is done with the previous pass's planes
    if (t >= 128) {
#pragma unroll
      for (int c = 0; c < kIcpGroup; ++c) plane[c][t - 128] = x[g + c];
    }
    __syncthreads();
    if (t < 128) {
#pragma unroll
      for (int c = 0; c < kIcpGroup; ++c) x[g + c] += plane[c][t];   // h = 128
    }
    __syncthreads();
    if (t >= 64 && t < 128) {
#pragma unroll
      for (int c = 0; c < kIcpGroup; ++c) plane[c][t - 64] = x[g + c];
    }
    __syncthreads();
    if (t < 64) {
#pragma unroll
      for (int c = 0; c < kIcpGroup; ++c) x[g + c] += plane[c][t];   // h = 64
    }
  }
  if (t < 64) {
#pragma unroll
    for (int c = 0; c < kIcpTerms; ++c) x[c] = wave_fold_down(x[c]);   // h = 32 .. 1
    if (t == 0) {
#pragma unroll
      for (int c = 0; c < kIcpTerms; ++c) p.partials[(long)blockIdx.x * kIcpTerms + c] = x[c];
    }
  }
  // at most 256 of each per chunk: both counts in one int
  const int both = block_sum_256(inlier | (changed << 16), count4);
  if (t == 0) {
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(p.history);
    if (both & 0xffff) atomicAdd(&counts[0], (unsigned long long)(both & 0xffff));
    if (both >> 16) atomicAdd(&counts[1], (unsigned long long)(both >> 16));
  }
}

__global__ __launch_bounds__(64) void icp_solve_kernel(const IcpStep p, long chunks) {
  __shared__ double S[kIcpTerms];
  const int t = threadIdx.x;
  if (t < kIcpTerms) {
    double s = 0.0;
#pragma unroll 8
    for (long j = 0; j < chunks; ++j) s += p.partials[j * kIcpTerms + t];
    S[t] = s;
  }
  __syncthreads();
  if (t == 0) {
    const unsigned long long* counts = reinterpret_cast<const unsigned long long*>(p.history);
    icp_finish(p, S, (long long)counts[0], (long long)counts[1]);
  }
}

void be_icp_clear(void* p, size_t bytes, cnr_stream s) { device_fill(p, 0, bytes, s, "icp history"); }

void be_icp_step(const IcpStep& p, cnr_stream s) {
  const long chunks = (p.n + kIcpChunk - 1) / kIcpChunk;
  {
    long blocks = chunks > 8192 ? 8192 : chunks;
    TimingScope ts_("icp_move_kernel", 2, 0, p.n, 0, 0, 0, s, (p.first ? 24.0 : 32.0) * (double)p.n);
    hipLaunchKernelGGL(icp_move_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
  }
  icp_search(p, s);
  {
    TimingScope ts_("icp_moments_kernel", 2, 0, p.n, 0, 0, 0, s, (p.F > 0 ? 116.0 : 56.0) * (double)p.n + 144.0 * (double)chunks);
    hipLaunchKernelGGL(icp_moments_kernel, dim3((unsigned)chunks), dim3(kIcpChunk), 0, s, p);
  }
  {
    TimingScope ts_("icp_solve_kernel", 2, 0, chunks, 0, 0, 0, s, 144.0 * (double)chunks + 160.0);
    hipLaunchKernelGGL(icp_solve_kernel, dim3(1), dim3(64), 0, s, p, chunks);
  }
  CNR_LAUNCH_CHECK("icp");
}

}  // namespace cnr
