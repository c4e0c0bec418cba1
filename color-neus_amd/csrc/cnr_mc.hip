// Marching cubes on the device lattice: the 512^3 volume never leaves HBM between extract_fields and the mesh.
// Cell classification + edge ownership, an exclusive scan of the two count channels, vertex / triangle emission (mc_emit_voxel, cnr_mc.h).
#include <hip/hip_runtime.h>

#define CNR_MC_QUAL static __constant__ const   // (the tables in constant memory)
#include "cnr_mc.h"
#include "cnr_hip_util.h"
#include "cnr_wave.h"

namespace cnr {

__global__ __launch_bounds__(256) void mc_count_kernel(const McVolume m) {
  const long n = (long)m.res * m.res * m.res;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < n; v += (long)gridDim.x * 256) {
    const int z = (int)(v % m.res), y = (int)((v / m.res) % m.res), x = (int)(v / ((long)m.res * m.res));
    unsigned char fl;
    const int idx = mc_cell(m.u, m.res, m.thr, x, y, z, &fl);
    m.flags[v] = fl;
    m.counts[v * 2] = mc_popcount3(fl);
    m.counts[v * 2 + 1] = idx >= 0 ? kMcNumTris[idx] : 0;
  }
}
// exclusive scan of the two count channels: per-block sums, one workgroup scans the block sums, blocks rescan with their offset
__global__ __launch_bounds__(256) void mc_block_sum_kernel(const McVolume m, long n) {
  // (both channels behind ONE barrier, the result in thread 0 only: two block_sum_256 calls hold four barriers and cost 2 VGPRs)
  __shared__ int red[2][4];
  const long base = (long)blockIdx.x * kMcScanBlock;
  int a = 0, b = 0;
  for (int j = threadIdx.x; j < kMcScanBlock; j += 256) { const long v = base + j; if (v < n) { a += m.counts[v * 2]; b += m.counts[v * 2 + 1]; } }
  a = wave_sum(a); b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    m.block_sums[blockIdx.x * 2] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    m.block_sums[blockIdx.x * 2 + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}
__global__ __launch_bounds__(1024) void mc_scan_sums_kernel(const McVolume m, int nblocks) {
  __shared__ int wsum[2][16];
  __shared__ int carry[2];
  block_carried_scan<16, 1, 2, int>(nblocks, wsum, carry,
                                    [&](int i, int (&x)[2]) { x[0] += m.block_sums[i * 2]; x[1] += m.block_sums[i * 2 + 1]; },
                                    [&](int i, const int (&at)[2]) { m.block_sums[i * 2] = at[0]; m.block_sums[i * 2 + 1] = at[1]; });
  if (threadIdx.x == 0) { m.totals[0] = carry[0]; m.totals[1] = carry[1]; }
}
__global__ __launch_bounds__(256) void mc_scan_apply_kernel(const McVolume m, long n) {
  // one workgroup rescans its 2048-element chunk: 8 elements per thread, wave scan of their sums, wave offsets through LDS.  (block_excl_scan's steps
  // with the block's offset added in front of the barrier, where its load is hidden: through the function the kernel took 2 more VGPRs)
  __shared__ int wsum[2][4];
  const long base = (long)blockIdx.x * kMcScanBlock + (long)threadIdx.x * 8;
  int a[8], b[8], sum[2] = {0, 0};
#pragma unroll
  for (int j = 0; j < 8; ++j) { const long v = base + j; a[j] = v < n ? m.counts[v * 2] : 0; b[j] = v < n ? m.counts[v * 2 + 1] : 0; sum[0] += a[j]; sum[1] += b[j]; }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl[2] = {sum[0], sum[1]};
  wave_incl_scan_int(incl, lane);
  if (lane == 63) { wsum[0][wave] = incl[0]; wsum[1][wave] = incl[1]; }
  __syncthreads();
  int oa = m.block_sums[blockIdx.x * 2] + incl[0] - sum[0], ob = m.block_sums[blockIdx.x * 2 + 1] + incl[1] - sum[1];
  for (int w = 0; w < wave; ++w) { oa += wsum[0][w]; ob += wsum[1][w]; }
#pragma unroll
  for (int j = 0; j < 8; ++j) { const long v = base + j; if (v < n) { m.counts[v * 2] = oa; m.counts[v * 2 + 1] = ob; } oa += a[j]; ob += b[j]; }
}
void be_mc_count(const McVolume& m, cnr_stream s) {
  const long n = (long)m.res * m.res * m.res;
  const int nblocks = (int)((n + kMcScanBlock - 1) / kMcScanBlock);
  TimingScope ts_("mc_count_scan", 2, 0, n, 0, 0, 0, s, (double)n * (4.0 * 4.0 + 1.0 + 8.0 * 3.0));
  long cb = (n + 255) / 256; if (cb > 65535 * 4) cb = 65535 * 4;
  hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)cb), dim3(256), 0, s, m);
  hipLaunchKernelGGL(mc_block_sum_kernel, dim3(nblocks), dim3(256), 0, s, m, n);
  hipLaunchKernelGGL(mc_scan_sums_kernel, dim3(1), dim3(1024), 0, s, m, nblocks);
  hipLaunchKernelGGL(mc_scan_apply_kernel, dim3(nblocks), dim3(256), 0, s, m, n);
  CNR_LAUNCH_CHECK("mc_count");
}

struct McEmit { McVolume m; float bmin[3], bmax[3]; float* verts; int* tris; };
__global__ __launch_bounds__(256) void mc_emit_kernel(const McEmit e) {
  const long n = (long)e.m.res * e.m.res * e.m.res;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < n; v += (long)gridDim.x * 256) mc_emit_voxel(e.m, v, e.bmin, e.bmax, e.verts, e.tris);
}
void be_mc_emit(const McVolume& m, const float* bmin, const float* bmax, float* verts, int* tris, cnr_stream s) {
  McEmit e;
  e.m = m; e.verts = verts; e.tris = tris;
  for (int c = 0; c < 3; ++c) { e.bmin[c] = bmin[c]; e.bmax[c] = bmax[c]; }
  const long n = (long)m.res * m.res * m.res;
  TimingScope ts_("mc_emit", 2, 0, n, 0, 0, 0, s);
  long cb = (n + 255) / 256; if (cb > 65535 * 4) cb = 65535 * 4;
  hipLaunchKernelGGL(mc_emit_kernel, dim3((unsigned)cb), dim3(256), 0, s, e);
  CNR_LAUNCH_CHECK("mc_emit");
}

}  // namespace cnr
