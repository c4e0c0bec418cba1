// Chain-fused MLP kernels for gfx950 (MI355X / CDNA4): a workgroup carries a tile of points through ALL layers of a chain.
//
// Why: the per-layer weight-stationary kernel (cnr_gemm_ws.h) streams every activation through HBM (2 KB per point and layer) and
// sits at ~0.5 of the HBM peak with the matrix cores ~20 % busy.  Here the activations never leave the CU between layers:
//   * the tile's current activations live in LDS as two f16 planes (hi + lo of the exactly power-of-two scaled fp32 row: the same
//     error-free split as the per-layer kernel, 3 x v_mfma_f32_32x32x16_f16 per product, fp32 accumulation);
//   * the layer's weights are NOT resident: every wave streams the fragments of its 32 output columns from L2 / Infinity Cache
//     straight into registers (fragment-major layout written by pack_frags_kernel: one contiguous, fully coalesced 1 KB read per
//     k16 block and plane), 4 blocks ahead of their use -- 256 KB per layer and tile, shared by every CU of an XCD through its L2;
//   * the MFMA is issued TRANSPOSED (A operand = weights, B operand = activations): a lane then owns ONE point and 16 CONSECUTIVE
//     output columns (the weight rows are dealt to the fragment so that register r <-> column c0 + 16 * half + r), so the fused
//     epilogue (bias, softplus, skip concat, row max, f16 split) is plain per-lane code and the next layer's planes are written with
//     16-byte LDS stores -- no transpose through LDS, one exchange between the two 32-lane halves per row for the row max (a VALU lane swap, cnr_pair32_max);
//   * two barriers per layer (row-max exchange, planes ready).
// Arithmetic is the per-layer kernels' arithmetic (same split, same scales, same MFMA order; the epilogue uses fused multiply-adds),
// so results agree with the unfused path to fp32 round-off.
// Scope: the chains that save nothing (sampler, lattice, sdf()).  A variant that also stored the pre-activations, features and
// row scales for the backward pass was built and measured (commit eeb54d9: parity green, 3.8 ms against 2.4 ms for the nine
// per-layer launches at 524 288 points): in the transposed layout a lane owns a 64-byte piece of a row, a wave-wide store
// touches 32 rows, and such stores drain at ~8 B/clk/CU; with the activations saved the chain is no longer MFMA/VALU bound either
// way (1 KB written per point and layer against 2 KB moved by the per-layer kernel), so the saving chains stay per layer.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "cnr_backend.h"
#include "cnr_hip_util.h"
#include "cnr_gemm_int.h"
#include "cnr_chain_util.h"

namespace cnr {

// ------------------------------------------------------------------------------------------------
// fragment-major weight planes: Wf[cb][kb][plane][lane][8] = plane[n(cb, lane & 31)][kb * 16 + (lane >> 5) * 8 + 0..7]
// with n(cb, m) = cb * 32 + 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3): MFMA row m of the transposed product -> layer column
// ------------------------------------------------------------------------------------------------
// one 64-thread block per 1 KB fragment block blk = (cb * nkb + kb) * 2 + plane of a job
__device__ __forceinline__ void pack_frags_block(const PackJob& j, const int blk) {
  const int nkb = j.ld / 16;
  const int plane = blk & 1, kb = (blk >> 1) % nkb, cb = (blk >> 1) / nkb;
  const int lane = threadIdx.x, m = lane & 31;
  const int n = cb * 32 + 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3);
  typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
  u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (n < j.rows) v = *reinterpret_cast<const u16x8*>(j.planes + (long)plane * j.plane_stride + (long)n * j.ld + kb * 16 + (lane >> 5) * 8);
  *reinterpret_cast<u16x8*>(j.Wf + ((long)blk * 64 + lane) * 8) = v;
}

using PackBatch = RowBatch<PackJob, 64>;
__global__ __launch_bounds__(64) void pack_frags_kernel(const PackBatch b) { const auto at = b.locate(blockIdx.x); pack_frags_block(at.job, at.row); }
void be_pack_frags_many(const PackJob* jobs, int count, cnr_stream s) {
  launch_row_batches<PackBatch>(pack_frags_kernel, "pack_frags", jobs, count, 64, s, [](const PackJob& j) { return 8 * (j.ld / 16) * 2; });
}

// ------------------------------------------------------------------------------------------------
// SDF value chain (no-grad uses: hierarchical sampler NeuS.py:345,191; extract_fields NeuS.py:14-28; sdf()): E -> sdf, nothing saved
//
// Geometry <RT, CB>: a workgroup of 8 / CB waves owns a tile of T = 32 * RT points; a wave owns CB blocks of 32 output columns
// (12 = 3 * RT * CB MFMAs per k16 block for both shipped shapes):
//   <4, 1>  512 threads, 128 points, one workgroup per CU: least weight traffic (2 KB per point and layer from L2), but MFMA and
//           epilogue phases of the whole CU alternate in lockstep;
//   <2, 2>  256 threads, 64 points, two workgroups per CU (74 KB of LDS each) at 4 KB of L2 weight reads per point and layer.
//           Measured equal to <4, 1> (6.5 ms for 2 M points): the two workgroups start together, do identical work and stay in phase
//           (both in the MFMA phase, then both in the epilogue), also when half of them are started a few microseconds late;
//   <1, 2>  32-point tiles for small point counts (fills the chip from 8192 points).
// Tried and dropped (round 4, commit 52bf6b3): two 4-wave groups per workgroup, each on its own 64-point half tile (<2, 2> per group), group 1
// running two barriers behind group 0 so that on every SIMD one wave is in an MFMA phase while the other is in an epilogue phase -- enforced by
// the barriers (4 per layer), with the weight ring pinned four blocks deep.  Bit-identical, and no faster: 1.57 ms against 1.55 ms per step for
// the sampler's chains, the same for a delay of 0, 1, 2 or 3 barriers.  MFMA time and epilogue time add up whatever the phase relation; the
// chip runs these kernels at 1.9-2.1 GHz of its 2.4 GHz (GRBM_GUI_ACTIVE / duration), i.e. it is at its power limit either way.
// ------------------------------------------------------------------------------------------------
// The kernel's LDS image, stated once: the kernel carves its regions from these byte offsets, the launcher passes the total
template <int RT, int CB>
struct SdfValueLds {
  static constexpr int T = 32 * RT;
  static constexpr int rs = 2 * T * CH_ALD;                 // (in front: [2][T][CH_ALD] hi | lo planes)  [T] 1 / row scale of the current layer input
  static constexpr int pm = rs + T * 4;                     // [T][8] per-wave partial row maxima / per-block partial dot products
  static constexpr int cwb = pm + T * 8 * 4;                // [2][512] column scales | biases of the current / next layer
  static constexpr int wtop = cwb + 2 * 512 * 4;            // [256] sdf row of the top layer
  static constexpr int total = wtop + 256 * 4;
  static_assert((size_t)total <= kChainLdsMax, "LDS budget");
};

template <int RT, int CB>
__global__ __launch_bounds__(512 / CB, 2 / (3 - CB) + 0) void sdf_value_chain_kernel(const SdfValueChain c) {
  constexpr int WAVES = 8 / CB, THREADS = 64 * WAVES;
  constexpr int T = 32 * RT;
  constexpr int APLANE = T * CH_ALD;
  using Lds = SdfValueLds<RT, CB>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* rs = reinterpret_cast<float*>(smem + Lds::rs);
  float* pm = reinterpret_cast<float*>(smem + Lds::pm);
  float* cwb = reinterpret_cast<float*>(smem + Lds::cwb);
  float* wtop = reinterpret_cast<float*>(smem + Lds::wtop);
  const int tid0 = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  const long ntiles = (c.P + T - 1) / T;

  f16x8 wr1[4][CB], wr2[4][CB];                              // weight fragment ring: 4 k16 blocks in flight
  auto wprime = [&](const FusedLayer& L, int lane_) __attribute__((always_inline)) {
    chain_wprime<CB>(wr1, wr2, chain_wlane<CB>(L.Wf, L.K >> 4, wave, lane_), L.K >> 4, 0, L.K >> 4);
  };

  wprime(c.lay[0], tid0 & 63);
  for (int i = tid0; i < 256; i += THREADS) wtop[i] = c.wtop[i];
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long tile0 = tile * T;
    const int rows_left = (int)((c.P - tile0) < T ? (c.P - tile0) : T);              // rows of this tile that exist (>= 1)
    {
      // ---- layer-0 input: E rows -> planes
      const ChainLane<CB> ln(tid0, wave);
      chain_cw_park(cwb, ln.tid, chain_cw_fetch(c.lay[0], ln.tid));
      chain_stage_rows<T, THREADS>(c.E, tile0, rows_left, ln.tid, smem, rs);
    }
    cnr_lds_barrier();

    for (int l = 0; l < c.nl; ++l) {
      const ChainLane<CB> ln(tid0, wave);
      const FusedLayer& L = c.lay[l];
      const int nkb = L.K >> 4;
      const bool last = l + 1 == c.nl;
      const FusedLayer& Ln = c.lay[last ? l : l + 1];
      const unsigned short* wlane = chain_wlane<CB>(L.Wf, nkb, wave, ln.lane);
      const f4 cw_next = chain_cw_fetch(Ln, ln.tid);   // lands while the MFMAs run; parked in LDS behind the row-max barrier
      f32x16 acc[CB][RT];
#pragma unroll
      for (int j = 0; j < CB; ++j)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[j][rt][r] = 0.0f;
      const unsigned char* Ab = smem + ln.pt * CH_ALD + ln.half * 16;
      // The k16 blocks of a layer are straight-line code (block count pinned at compile time), weight ring four blocks deep, scheduling fence
      // per block (chain_mfma_blocks in cnr_chain_util.h)
      if (nkb == 16) chain_mfma_blocks<RT, CB, 16>(acc, wr1, wr2, Ab, APLANE, wlane, 16, 0);
      else chain_mfma_blocks<RT, CB, 3>(acc, wr1, wr2, Ab, APLANE, wlane, 3, 0);
      // the next layer's (or the next tile's first layer's) leading weight blocks travel while the epilogue runs
      wprime(last ? c.lay[0] : c.lay[l + 1], ln.lane);

      // ---- epilogue: z = acc * (1 / row scale) * (1 / column scale) + bias ; a = softplus(z) ; skip concat ; row max
      const float* cw = cwb + (l & 1) * 512;
      const bool next_skip = !last && ((c.skip_mask >> (l + 1)) & 1);
      const float oscale = next_skip ? kInvSqrt2 : 1.0f;
      const bool ragged = L.N < 256;   // wave-uniform: only the layer in front of a skip connection (217 columns + 39 of e)
      ChainActSoftplus act{next_skip};
      float red[RT], dotj[CB][RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        red[rt] = 0.0f;
#pragma unroll
        for (int j = 0; j < CB; ++j) dotj[j][rt] = 0.0f;
      }
#pragma unroll
      for (int j = 0; j < CB; ++j) {
        const int c0 = ln.cbase + 32 * j;
        const ChainColumns k = chain_columns(cw, c0);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const int row_l = rt * 32 + ln.pt;
          chain_affine16(acc[j][rt], k, rs[row_l], act);
          if (ragged && c0 + 16 > L.N) {
            const int row_c = row_l < rows_left ? row_l : rows_left - 1;
            CHAIN_SKIP_TAIL(acc[j][rt], c0, L.N, c.E + tile0 * kEmb + row_c * kEmb, c.emb, next_skip, oscale)
          }
          if (last) dotj[j][rt] = chain_dot16(acc[j][rt], wtop + c0);
          else red[rt] = fmaxf(red[rt], chain_absmax16(acc[j][rt]));
        }
      }
      // partial results per row: the row maximum per wave; the sdf dot product per 32-column block, slot = block index (chain_partial_sum)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        if (last) {
#pragma unroll
          for (int j = 0; j < CB; ++j) chain_partial_sum(pm, rt * 32 + ln.pt, wave * CB + j, ln.half, dotj[j][rt]);
        } else {
          chain_partial_max(pm, rt * 32 + ln.pt, wave, ln.half, red[rt]);
        }
      }
      cnr_lds_barrier();   // partial maxima visible; every wave is done reading the planes of this layer's input
      if (!last) {
        chain_cw_park(cwb + ((l + 1) & 1) * 512, ln.tid, cw_next);
        chain_replane<RT, CB, WAVES>(acc, pm, smem, rs, nullptr, nullptr, false, nullptr, tile0, rows_left, ln, wave);
      } else {
        chain_sdf_finish<T>(pm, ln.tid, tile0, rows_left, c.btop, c.top_scale, c.sdf_out);
      }
      cnr_lds_barrier();
    }
  }
}

template <int RT, int CB>
static void launch_sdf_value_chain(const SdfValueChain& c, cnr_stream s) {
  using Lds = SdfValueLds<RT, CB>;
  double macs = 0.0;
  for (int l = 0; l < c.nl; ++l) macs += (double)c.lay[l].K * 256.0;
  chain_launch<&sdf_value_chain_kernel<RT, CB>>(c, 32 * RT, 512 / CB, Lds::total, chain_wgs_for(Lds::total), c.P, "chain_sdf_value", RT * 10 + CB, macs,
                                                 (double)c.P * (kEmb + 1) * 4.0, s);
}

bool be_sdf_value_chain(const SdfValueChain& c, cnr_stream s) {
  const bool off = debug_flags().no_fused;   // debugging aid: per-layer kernels everywhere
  if (off || c.P <= 0) return false;
  for (int l = 0; l < c.nl; ++l)
    if ((c.lay[l].K != 256 && c.lay[l].K != 48) || c.lay[l].N > 256 || c.lay[l].N < 1) return false;   // k16 block counts the kernel pins
  // tile shape RT * 10 + CB: the tile heights of chain_rt_for (the saving chains' thresholds), two column blocks per wave below 128-point tiles
  const int force = debug_flags().chain_shape;   // tuning aid: 41, 22, 12
  const int rt = chain_rt_for(c.P, 0);
  const int shape = force ? force : (rt == 4 ? 41 : (rt == 2 ? 22 : 12));
  if (shape == 41) launch_sdf_value_chain<4, 1>(c, s);
  else if (shape == 22) launch_sdf_value_chain<2, 2>(c, s);
  else launch_sdf_value_chain<1, 2>(c, s);
  CNR_LAUNCH_CHECK("chain_sdf_value");
  return true;
}

}  // namespace cnr
