// Device helpers shared by the chain-fused kernels (cnr_chain.hip: value-only SDF chain; cnr_chain_fwd.hip: the saving forward chains).
#pragma once
#include <hip/hip_runtime.h>

#include "cnr_backend.h"
#include "cnr_hip_util.h"
#include "cnr_gemm_int.h"
#include "cnr_split.h"

namespace cnr {

constexpr int CH_ALD = 256 * 2 + 16;   // bytes per LDS row of one plane (+16: conflict-free ds_read_b128 of the fragments)

// Packed fp32 arithmetic (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32: two elements per VALU issue).  The epilogue of a layer runs
// with every wave of the workgroup in the same phase (the barriers keep MFMA and epilogue phases in lockstep), so its VALU
// instruction count is wall time: measured on 2 M points, 6.57 ms = 3.44 ms of MFMA + 3.13 ms of everything else.
// (tools/probes/overlap_probe.hip: VALU work of one wave does hide behind the MFMAs of the OTHER wave of its SIMD -- 12 MFMAs 223 ns,
// 96 VALU 334 ns, both 386 ns -- but two workgroups per CU running the same phases at the same time gain nothing from it.)
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 pk_splat(float x) { f2 r = {x, x}; return r; }

// nn.Softplus(beta=100, threshold=20) on two elements: max(z,0) + log2(1 + 2^(-|100 z| / ln 2)) * ln 2 / 100 (see cnr_common.h)
__device__ __forceinline__ f2 softplus100_pk(f2 z) {
  const f2 m = z * pk_splat(144.26950408889634f);
  f2 e;
  e.x = __builtin_amdgcn_exp2f(-fabsf(m.x)); e.y = __builtin_amdgcn_exp2f(-fabsf(m.y));   // (the sign / abs modifiers are free)
  const f2 s = e + pk_splat(1.0f);
  f2 l, r;
  l.x = __builtin_amdgcn_logf(s.x); l.y = __builtin_amdgcn_logf(s.y);
  r.x = fmaxf(z.x, 0.0f); r.y = fmaxf(z.y, 0.0f);
  return pk_fma(l, pk_splat(0.0069314718055994531f), r);
}

// ------------------------------------------------------------------------------------------------
// One MFMA phase of a chain-fused kernel: NKB k16 blocks of the transposed product acc[j][rt] += W_frag(kb) x Act_frag(kb, rt) as straight-line
// code (3 x v_mfma_f32_32x32x16_f16 per product: hi x lo, lo x hi, hi x hi).  These kernels stay on 32 x 32 x 16: converted to 16 x 16 x 32 they were
// 1-8 % slower in three forms (profiles/r06_ab_chain_mfma16.txt): they run below the board's power limit, so cheaper MFMAs do not buy time as they do
// in layer_dw.
//   * the weight fragments come from a 4-deep register ring: blocks kb0 .. kb0 + 3 must already be in flight (chain_wprime); block kb + 4 is
//     requested as soon as the MFMAs of block kb have read their slot;
//   * the activation fragments of block kb + 1 are read from LDS into a second register set BEFORE the MFMAs of block kb;
//   * a scheduling fence closes every block.  Without it the compiler sinks each weight load down to its first use (load, s_waitcnt vmcnt(0),
//     MFMA -- checked in the ISA of both chain kernels), i.e. every k16 block waits for an L2 round trip and the "ring" is one block deep.
// Wf layout: [column block cb][k16 block kb (nkb_w per column block)][plane][lane][8]; wbase = this wave's first column block + lane * 8.
// ------------------------------------------------------------------------------------------------
template <int CB>
__device__ __forceinline__ void chain_wload(f16x8 (&wr1)[4][CB], f16x8 (&wr2)[4][CB], int slot, const unsigned short* wlane, int nkb_w, int kb) {
#pragma unroll
  for (int j = 0; j < CB; ++j) {
    const unsigned short* b = wlane + (long)(j * nkb_w + kb) * 1024;
    wr1[slot][j] = *reinterpret_cast<const f16x8*>(b);
    wr2[slot][j] = *reinterpret_cast<const f16x8*>(b + 512);
  }
}
// the first four blocks of a phase of n >= 1 blocks (index clamped: a shorter phase loads its last block again -- no branch between the loads)
template <int CB>
__device__ __forceinline__ void chain_wprime(f16x8 (&wr1)[4][CB], f16x8 (&wr2)[4][CB], const unsigned short* wlane, int nkb_w, int kb0, int n) {
#pragma unroll
  for (int q = 0; q < 4; ++q) chain_wload<CB>(wr1, wr2, q, wlane, nkb_w, kb0 + (q < n ? q : n - 1));
}
// KB0 / NTOT: this call covers the k16 blocks [KB0, KB0 + NKB) of a phase of NTOT blocks (a phase may be cut into several calls with a
// workgroup barrier in between: the ring slots and the refill rule follow the block index within the phase; KB0 a multiple of 4).
template <int RT, int CB, int NKB, int KB0 = 0, int NTOT = NKB>
__device__ __forceinline__ void chain_mfma_blocks(f32x16 (&acc)[CB][RT], f16x8 (&wr1)[4][CB], f16x8 (&wr2)[4][CB], const unsigned char* Ab, int aplane,
                                                  const unsigned short* wlane, int nkb_w, int kb0) {
  static_assert((KB0 & 3) == 0 && KB0 + NKB <= NTOT, "chain_mfma_blocks: block range");
  f16x8 a1[2][RT], a2[2][RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    a1[0][rt] = *reinterpret_cast<const f16x8*>(Ab + rt * 32 * CH_ALD + KB0 * 32);
    a2[0][rt] = *reinterpret_cast<const f16x8*>(Ab + rt * 32 * CH_ALD + aplane + KB0 * 32);
  }
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    const int cur = kb & 1, gk = KB0 + kb;
    if (kb + 1 < NKB) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        a1[cur ^ 1][rt] = *reinterpret_cast<const f16x8*>(Ab + rt * 32 * CH_ALD + (gk + 1) * 32);
        a2[cur ^ 1][rt] = *reinterpret_cast<const f16x8*>(Ab + rt * 32 * CH_ALD + aplane + (gk + 1) * 32);
      }
    }
#pragma unroll
    for (int j = 0; j < CB; ++j)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[j][rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr2[gk & 3][j], a1[cur][rt], acc[j][rt], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < CB; ++j)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[j][rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr1[gk & 3][j], a2[cur][rt], acc[j][rt], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < CB; ++j)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[j][rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr1[gk & 3][j], a1[cur][rt], acc[j][rt], 0, 0, 0);
    if (gk + 4 < NTOT) chain_wload<CB>(wr1, wr2, gk & 3, wlane, nkb_w, kb0 + gk + 4);
    __builtin_amdgcn_sched_barrier(0);
  }
}

}  // namespace cnr
