// The tile steps of the weight-stationary layer kernels, written once: layer_gemm_ws_kernel and its stream form
// (cnr_gemm_ws.h), layer_dw_kernel (cnr_gemm_fdw.hip), sweep0_dw_kernel (cnr_sweep0.hip), narrow_bwd_kernel (cnr_narrow_bwd.hip).
// A layer's weights stay in registers as two f16 planes, points stream through LDS in 32-row tiles, every product is the three MFMAs of
// cnr_split.h.  Device functions and small structs only; none places a barrier or a fence: the kernels own their schedules (which wave group
// fetches, puts and computes, and when) and put the barriers, fences, sched_barriers and priorities between the steps.
#pragma once
#include <hip/hip_runtime.h>

#include "cnr_backend.h"
#include "cnr_hip_util.h"
#include "cnr_gemm_int.h"
#include "cnr_split.h"

namespace cnr {

constexpr int WS_TP = 32;        // points per tile
constexpr int WS_THREADS = 512;
constexpr int WS_TLD = 36;       // floats per row of a wave's accumulator transposition tile

// ---- the tile range of a workgroup: `count` tiles from `first`, cut at the launch's last tile.  tile(i) maps the loop counter to the tile: a
// launch with rev set walks every range downwards (consecutive launches of a chain alternate, so a launch starts on the rows its producer
// wrote last, still in L2 / Infinity Cache).  prefetch(i): the same with the counter clamped to the range, for requests issued unconditionally
// (the redundant tile at the end of a range is loaded and never used).
struct WsRange {
  long t0;
  int n, rev;
  __device__ __forceinline__ WsRange(long ntiles, long first, int count, int rev_)
      : t0(first), n(first < ntiles ? (int)((ntiles - first) < count ? (ntiles - first) : count) : 0), rev(rev_) {}
  __device__ __forceinline__ int last() const { return n > 0 ? n - 1 : 0; }
  __device__ __forceinline__ long tile(int i) const { return t0 + (rev ? last() - i : i); }
  __device__ __forceinline__ long prefetch(int i) const { return tile(i < last() ? i : last()); }
};

// ---- resident weights: the two f16 planes of W in the B-operand layout of each MFMA shape
// 32 x 32 x 16: lane (n = lane & 31, kg = lane >> 5) holds W[row][16 kb + 8 kg ..] of k16 block kb < nkb; ZERO: the blocks beyond nkb are zero
// (a kernel that multiplies all NKB blocks), otherwise they stay unset (a kernel that guards every block)
template <int NKB, bool ZERO>
__device__ __forceinline__ void ws_wfrag32(f16x8 (&w1)[NKB], f16x8 (&w2)[NKB], const LayerGemm& g, int row, int lane, int nkb) {
  const unsigned short* wp = g.Wp + (long)row * g.ldw + (lane >> 5) * 8;
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    if (kb < nkb) {
      w1[kb] = *reinterpret_cast<const f16x8*>(wp + kb * 16);
      w2[kb] = *reinterpret_cast<const f16x8*>(wp + g.wp_stride + kb * 16);
    } else if (ZERO) {
      const f16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
      w1[kb] = z8; w2[kb] = z8;
    }
  }
}
// 16 x 16 x 32, 2 column blocks: lane (n = lane & 15, kg = lane >> 4) holds W[c0 + 16 cb + n][32 kb + 8 kg ..]
template <int NKB2>
__device__ __forceinline__ void ws_wfrag16(f16x8 (&w1)[NKB2][2], f16x8 (&w2)[NKB2][2], const LayerGemm& g, int c0, int lane) {
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const unsigned short* wp = g.Wp + (long)(c0 + 16 * cb + (lane & 15)) * g.ldw + (lane >> 4) * 8;
#pragma unroll
    for (int kb = 0; kb < NKB2; ++kb) {
      w1[kb][cb] = *reinterpret_cast<const f16x8*>(wp + kb * 32);
      w2[kb][cb] = *reinterpret_cast<const f16x8*>(wp + g.wp_stride + kb * 32);
    }
  }
}

// ---- stage-put of one row of a tile: NG groups of 4 columns (64 columns apart) of the staging thread -> row maximum over the 16 threads of the
// row, exact power-of-two row scale, hi / lo planes into LDS (`dst`: the thread's first group in the hi plane; group q is stored where live[q]),
// and 1 / scale into rs[row] by the row's `owner` thread.  Returns the maximum and the scale: ss, rs_out, the row dot and the block exponent are
// the caller's.
struct WsRowScale { float mx, sc; };
template <int NG>
__device__ __forceinline__ float ws_absmax_groups(const f4 (&v)[NG]) {
  static_assert(NG == 1 || NG == 4 || NG == 5, "column groups of a staging thread");
  if constexpr (NG == 1) return ws_absmax4(v[0]);
  else {
    const float m4 = fmaxf(fmaxf(ws_absmax4(v[0]), ws_absmax4(v[1])), fmaxf(ws_absmax4(v[2]), ws_absmax4(v[3])));
    if constexpr (NG == 4) return m4; else return fmaxf(m4, ws_absmax4(v[4]));
  }
}
template <int NG>
__device__ __forceinline__ WsRowScale ws_stage_put(const f4 (&v)[NG], const bool (&live)[NG], unsigned char* dst, int plane, float* rs, int row, bool owner) {
  const float mx = cnr_max16(ws_absmax_groups<NG>(v));
  const float sc = split_row_scale(mx);
#pragma unroll
  for (int q = 0; q < NG; ++q)
    if (live[q]) split_put4(v[q], sc, dst + 128 * q, plane);
  if (owner) rs[row] = cnr_pow2_rcp(sc);
  return {mx, sc};
}

// ---- the k loop of a tile's product on resident weights
// 32 x 32 x 16: Ab = the lane's A fragment of k16 block 0 in the hi plane (row lane & 31, 16 bytes per lane >> 5); wfrag(kb, w1, w2) hands out
// the weight planes of block kb (registers, or LDS in narrow_bwd); blocks at or beyond nkb are skipped
template <int NKB, class WF>
__device__ __forceinline__ void ws_product32(f32x16& acc, const unsigned char* Ab, int aplane, int nkb, WF&& wfrag) {
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    if (kb < nkb) {
      const f16x8 a1 = *reinterpret_cast<const f16x8*>(Ab + kb * 32);
      const f16x8 a2 = *reinterpret_cast<const f16x8*>(Ab + aplane + kb * 32);
      f16x8 w1, w2;
      wfrag(kb, w1, w2);
      split_mfma3_32(acc, a1, a2, w1, w2);
    }
  }
}
// 16 x 16 x 32, [2 row blocks of 16 points][2 column blocks]: Ab = tile[lane & 15][8 (lane >> 4) ..] in the hi plane, `ald` bytes per row
template <int NKB2>
__device__ __forceinline__ void ws_product16(f32x4 (&acc)[2][2], const unsigned char* Ab, int ald, int aplane, const f16x8 (&w1)[NKB2][2], const f16x8 (&w2)[NKB2][2]) {
#pragma unroll
  for (int kb = 0; kb < NKB2; ++kb) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const f16x8 a1 = *reinterpret_cast<const f16x8*>(Ab + rb * 16 * ald + kb * 64);
      const f16x8 a2 = *reinterpret_cast<const f16x8*>(Ab + rb * 16 * ald + aplane + kb * 64);
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) split_mfma3_16(acc[rb][cb], a1, a2, w1[kb][cb], w2[kb][cb]);
    }
  }
}

// ---- a wave's [32 points x 32 columns] accumulator block through its transposition tile T ([32][WS_TLD] floats): stored in the MFMA's lane
// map, read back as 4 consecutive columns of one row with the row and column scales undone (exact).  The wave fences between the two.
__device__ __forceinline__ void ws_acc_to_tile32(float* T, const f32x16& acc, int hi, int cl) {   // (hi = lane >> 5, cl = lane & 31)
#pragma unroll
  for (int r = 0; r < 16; ++r) T[((r & 3) + 8 * (r >> 2) + 4 * hi) * WS_TLD + cl] = acc[r];
}
__device__ __forceinline__ void ws_acc_to_tile16(float* T, const f32x4 (&acc)[2][2], int lane) {
  const int q4 = lane >> 4, cl = lane & 15;   // result block: rows 4 q4 + r, column cl
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) T[(16 * rb + 4 * q4 + r) * WS_TLD + 16 * cb + cl] = acc[rb][cb][r];
}
__device__ __forceinline__ f4 ws_tile_row4(const float* T, const float* rs, int rr, int cc, const f4& wsc) {
  const float rsc = rs[rr];
  f4 v = *reinterpret_cast<const f4*>(T + rr * WS_TLD + cc);
  v.x *= rsc * wsc.x; v.y *= rsc * wsc.y; v.z *= rsc * wsc.z; v.w *= rsc * wsc.w;
  return v;
}

// ---- MFMA fragments out of ROW-MAJOR [point][column] f16 planes by the LDS transpose read (gfx950 ds_read_b64_tr_b16): a 16-lane group reads a
// [4 points][16 columns] block, 8 contiguous bytes per lane (lane i: block row i >> 2, columns 4 (i & 3) ..), and lane i receives column i of it.
// Two reads make one fragment (8 k positions of the lane's row / column).  The four rows of a block are taken 4 POINTS APART: with a row stride of
// 4 banks mod 64 (528 B, 272 B, 144 B) they sit 16 banks apart and the 2 x 4 x 4 eight-byte pieces of a 32-lane half cover the 64 banks exactly
// once.  So position q = 4 h + r of k group kg in k16 block kb holds point 16 kb + 4 r + 2 kg + h (ws_kslot is the inverse) -- for both operands of
// a product over points, which is all the MFMA needs.  `src`: the lane's piece for h = 0; the piece for h = 1 lies one point row (ld bytes) below.
typedef short ws_s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f16x8 ws_tr8(const unsigned char* src, int ld) {
  typedef __attribute__((address_space(3))) ws_s16x4* lds_s16x4;
  const ws_s16x4 h0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(src));
  const ws_s16x4 h1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(src + ld));
  return __builtin_bit_cast(f16x8, __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7));
}
__device__ __forceinline__ int ws_kslot(int pt) {   // k position (within a 32-point tile) at which the fragments above hold point pt
  return (pt & 16) | ((pt & 2) << 2) | ((pt & 1) << 2) | ((pt >> 2) & 3);
}
// the lane's piece (h = 0) of a block of the 32 x 32 x 16 shape: point row and first column within a 32-column operand block
struct WsTrPiece { int prow, pcol; };
__device__ __forceinline__ WsTrPiece ws_tr_piece32(int lane, int kb) {   // k16 block kb of the tile, k group lane >> 5
  return {kb * 16 + (lane >> 5) * 2 + 4 * ((lane & 15) >> 2), (lane & 16) + (lane & 3) * 4};
}

// ---- weight-gradient fragment step: dW block += sum over the points of a k step of A'[pt][row] * B'[pt][column], both operands split
// (32 x 32 x 16; layer_dw_kernel's D waves, on 16 x 16 x 32, keep their own words: cnr_gemm_fdw.hip)  The wave's [32 x 64] block; a1 / a2 are the planes of its 32 rows, the 2 x 32 columns come out of the planes at `bsrc` (`ld`
// bytes per point row, lo plane `plane` bytes behind); columns at or beyond `climit` read the pad behind a row and are masked
__device__ __forceinline__ void ws_dw_step32(f32x16 (&dacc)[2], const f16x8& a1, const f16x8& a2, const unsigned char* bsrc, int ld, int plane, const WsTrPiece& pc, int lane, int climit) {
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const unsigned char* src = bsrc + pc.prow * ld + (cb * 32 + pc.pcol) * 2;
    f16x8 b1 = ws_tr8(src, ld);
    f16x8 b2 = ws_tr8(src + plane, ld);
    if (cb * 32 + (lane & 31) >= climit) {
      const f16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
      b1 = z8; b2 = z8;
    }
    split_mfma3_32(dacc[cb], a1, a2, b1, b2);
  }
}
// ---- a wave's [32 rows from c0 x 64 columns] accumulator pair into a partial-sum slot [256][ldk]: columns below `klim` get the sums (UNDO:
// times the two exact factors that take 2^G back), the columns from there to ldk zeros, so that every slot is written in full
template <bool UNDO>
__device__ __forceinline__ void ws_store_slot32(float* out, int ldk, int c0, int lane, const f32x16 (&acc)[2], int klim, float u1 = 1.0f, float u2 = 1.0f) {
  const int m = lane & 31, kg = lane >> 5;
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int c = cb * 32 + m;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = c0 + (r & 3) + 8 * (r >> 2) + 4 * kg;
      if (c < ldk) out[(long)j * ldk + c] = c < klim ? (UNDO ? acc[cb][r] * u1 * u2 : acc[cb][r]) : 0.0f;
    }
  }
}

}  // namespace cnr
