// Device helpers shared by the chain-fused kernels (cnr_chain.hip: value-only SDF chain; cnr_chain_fwd.hip: the saving forward chains).
#pragma once
#include <hip/hip_runtime.h>

#include "cnr_backend.h"
#include "cnr_debug.h"
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

// ================================================================================================
// The tile steps of the chain-fused forward kernels (sdf_value_chain_kernel, sdf_save_chain_kernel, relu_chain_fwd_kernel), written once.
// Every block works on one lane's registers or one tile's LDS rows and has NO barrier of its own: the kernels place the barriers.
// Geometry: T = 32 * RT points per tile; a wave owns CB blocks of 32 output columns; a lane owns point pt (+ 32 rt) and the 16 consecutive
// columns cbase + 32 j .. + 15 of its j-th block.  LDS planes: [2][T][CH_ALD] bytes (hi | lo), the lo plane T * CH_ALD bytes behind the hi plane.
// ================================================================================================

// Per-lane indices, re-derived from a LAUNDERED copy of the thread index once per step: hoisted out of the step loop they pin dozens of address
// registers for the whole kernel (29 - 33 spilled VGPRs before); derived from the laundered copy the compiler recomputes them per step
// (a few integer operations).
template <int CB>
struct ChainLane {
  int tid, lane, half, pt, cbase;
  __device__ __forceinline__ ChainLane(int tid0, int wave) {
    tid = tid0;
    asm volatile("" : "+v"(tid));
    lane = tid & 63; half = lane >> 5; pt = lane & 31;
    cbase = wave * CB * 32 + 16 * half;   // this lane's 16 consecutive output columns of its j-th block: cbase + 32 j
  }
};

// this lane's part of the fragments of its wave's first column block (chain_mfma_blocks: wlane)
template <int CB>
__device__ __forceinline__ const unsigned short* chain_wlane(const unsigned short* Wf, int nkb_w, int wave, int lane) {
  return Wf + (long)wave * CB * nkb_w * 1024 + lane * 8;
}

// [column scales (256) | biases (256)] of a step: threads 0..127 fetch one float4 each while the MFMAs of the step before run (chain_cw_fetch) and
// park it in LDS behind the row-max barrier (chain_cw_park), when every wave has read the values it replaces
// (L: the step's descriptor, FusedLayer or ChainFwdStep; its two pointers are read where they are used: handed in as two values they cost the
// saving SDF chain 4 VGPRs)
template <class L>
__device__ __forceinline__ f4 chain_cw_fetch(const L& d, int tid) {
  f4 v = {0.f, 0.f, 0.f, 0.f};
  if (tid < 64) v = *reinterpret_cast<const f4*>(d.wsc + tid * 4);
  else if (tid < 128) v = *reinterpret_cast<const f4*>(d.bias + (tid - 64) * 4);
  return v;
}
__device__ __forceinline__ void chain_cw_park(float* cw, int tid, const f4& v) {
  if (tid < 128) *reinterpret_cast<f4*>(cw + tid * 4) = v;
}

// ---- a chain starts: its input rows HBM -> registers -> exact row scale -> f16 planes (16 threads per row, 4 columns each).
// All loads of the row groups first, then the conversion: consumed one by one the compiler waits for each load before it issues the next
// (one exposed memory round trip per chain start, not one per row group).  Rows past the end of a ragged last tile read the last row (never stored).
// General entry: NG groups of 64 main columns (ncol of them exist) + the magnitude of xcol extra columns behind them (EXTRA: kept in vx for the
// caller, which stages them later with the SAME row scale), rows optionally gathered through ridx, the scale kept (rsf) and stored (rs_out).
// (rs_out by reference: the descriptor's pointer is read where it is used; handed in as a value it costs relu_chain_fwd_kernel<1> a VGPR)
template <int T, int THREADS, int NG, bool EXTRA>
__device__ __forceinline__ void chain_stage_rows(const float* in, int ld, int ncol, int xcol, const int* ridx, long tile0, int rows_left, int tid,
                                                 unsigned char* planes, float* rs, float* rsf, float* const& rs_out, f4 (&vx)[T * 16 / THREADS]) {
  constexpr int NPASS = T * 16 / THREADS, APLANE = T * CH_ALD;
  const float* in_tile = in + (ridx != nullptr ? 0 : tile0 * ld);   // (uniform: scalar base + 32-bit lane offsets)
  const int sc4 = (tid & 15) * 4;
  const f4 z4 = {0.f, 0.f, 0.f, 0.f};
  f4 v[NG][NPASS];
#pragma unroll
  for (int pass = 0; pass < NPASS; ++pass) {
    const int row_l = pass * (THREADS / 16) + (tid >> 4);
    const int row_c = row_l < rows_left ? row_l : rows_left - 1;
    const float* src = ridx != nullptr ? in_tile + (long)ridx[tile0 + row_c] * ld : in_tile + row_c * ld;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      v[g][pass] = z4;
      if (64 * g + sc4 < ncol) v[g][pass] = *reinterpret_cast<const f4*>(src + 64 * g + sc4);
    }
    if (EXTRA) {
      vx[pass] = z4;
      if (sc4 < xcol) vx[pass] = *reinterpret_cast<const f4*>(src + ncol + sc4);   // (here only its magnitude is used: one scale for the whole row)
    }
  }
#pragma unroll
  for (int pass = 0; pass < NPASS; ++pass) {
    const int row_l = pass * (THREADS / 16) + (tid >> 4);
    float mx = ws_absmax4(v[0][pass]);
#pragma unroll
    for (int g = 1; g < NG; ++g) mx = fmaxf(mx, ws_absmax4(v[g][pass]));
    if (EXTRA) mx = fmaxf(mx, ws_absmax4(vx[pass]));
    mx = cnr_max16(mx);
    const float sc = split_row_scale(mx);
    unsigned char* dst = planes + row_l * CH_ALD + sc4 * 2;
#pragma unroll
    for (int g = 0; g < NG; ++g)
      if (64 * g + sc4 < ncol) split_put4(v[g][pass], sc, dst + 128 * g, APLANE);
    if ((tid & 15) == 0) {
      rs[row_l] = cnr_pow2_rcp(sc);
      if (rsf != nullptr) rsf[row_l] = sc;
      if (rs_out != nullptr && row_l < rows_left) rs_out[tile0 + row_l] = split_rs_value(mx, sc);
    }
  }
}
// The SDF chains' entry: the kEmb-wide embedding rows E, nothing kept or stored
template <int T, int THREADS>
__device__ __forceinline__ void chain_stage_rows(const float* E, long tile0, int rows_left, int tid, unsigned char* planes, float* rs) {
  f4 none[T * 16 / THREADS];
  chain_stage_rows<T, THREADS, 1, false>(E, kEmb, kEmb, 0, nullptr, tile0, rows_left, tid, planes, rs, nullptr, nullptr, none);
}

// ---- epilogue: z = acc * (1 / row scale) * (1 / column scale) + bias on a lane's 16 columns, then the activation, two elements per VALU issue
struct ChainColumns { f4 wsc4[4], b4[4]; };   // a lane's 16 column scales and biases, from the parked [scales | biases] block
__device__ __forceinline__ ChainColumns chain_columns(const float* cw, int c0) {
  ChainColumns k;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    k.wsc4[q] = *reinterpret_cast<const f4*>(cw + c0 + 4 * q);
    k.b4[q] = *reinterpret_cast<const f4*>(cw + 256 + c0 + 4 * q);
  }
  return k;
}
struct ChainActNone {      // the top step of the saving SDF chain, and z itself where it is stored before the activation
  __device__ __forceinline__ f2 operator()(f2 z) { return z; }
};
struct ChainActSoftplus {  // softplus, / sqrt(2) in front of a skip layer (scale: that step alone, for columns that carry e instead of softplus(z))
  bool half_power;
  __device__ __forceinline__ f2 scale(f2 a) const { return half_power ? a * pk_splat(kInvSqrt2) : a; }
  __device__ __forceinline__ f2 operator()(f2 z) const { return scale(softplus100_pk(z)); }
};
struct ChainActRelu {      // ReLU; mx: the largest output so far (they are >= 0: the row's abs-max)
  float mx = 0.0f;
  __device__ __forceinline__ f2 operator()(f2 z) {
    z.x = fmaxf(z.x, 0.0f); z.y = fmaxf(z.y, 0.0f);
    mx = fmaxf(fmaxf(z.x, z.y), mx);
    return z;
  }
};
template <class Act>
__device__ __forceinline__ void chain_affine16(f32x16& a, const ChainColumns& k, float rs_row, Act& act) {
  const f2 rsc = pk_splat(rs_row);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f2 w = {k.wsc4[q >> 1][(2 * q) & 3], k.wsc4[q >> 1][(2 * q + 1) & 3]};
    const f2 b = {k.b4[q >> 1][(2 * q) & 3], k.b4[q >> 1][(2 * q + 1) & 3]};
    f2 z = {a[2 * q], a[2 * q + 1]};
    z = act(pk_fma(z, rsc * w, b));                        // acc / (row scale * column scale) + bias
    a[2 * q] = z.x; a[2 * q + 1] = z.y;
  }
}

// The columns >= N_ of the layer in front of a skip connection (only the lanes that own some enter): e * oscale_ where a skip layer follows
// ([softplus(z) | e] / sqrt(2), fields.py:86-87), zero otherwise.  Branch-free per element: the e value is fetched from a clamped index and
// selected; all 16 loads first (consumed one by one the compiler waits for each before it issues the next).
// A macro, not a function: as a function (seven shapes tried: reference / value / per element, N_ and emb_ by value or read through the
// descriptors) the compiler simplifies the body on its own before it inlines it and forms other selects; sdf_value_chain_kernel<2, 2> then
// takes 234 - 237 VGPRs instead of 228 and <1, 2> 163 instead of 152.  a_: the lane's f32x16 block; N_, emb_, next_skip_, oscale_ are read where used.
#define CHAIN_SKIP_TAIL(a_, c0_, N_, erow_, emb_, next_skip_, oscale_)                                                              \
  {                                                                                                                                 \
    const float* skip_erow_ = (erow_);                                                                                              \
    float skip_ev_[16];                                                                                                             \
    _Pragma("unroll") for (int skip_r_ = 0; skip_r_ < 16; ++skip_r_) {                                                              \
      const int skip_ei_ = (c0_) + skip_r_ - (N_);                                                                                  \
      skip_ev_[skip_r_] = skip_erow_[skip_ei_ < 0 ? 0 : (skip_ei_ < kEmb ? skip_ei_ : kEmb - 1)];                                   \
    }                                                                                                                               \
    _Pragma("unroll") for (int skip_r_ = 0; skip_r_ < 16; ++skip_r_) {                                                              \
      const int skip_ei_ = (c0_) + skip_r_ - (N_);                                                                                  \
      const float skip_tail_ = ((next_skip_) && skip_ei_ < (emb_)) ? skip_ev_[skip_r_] * (oscale_) : 0.0f;                          \
      (a_)[skip_r_] = skip_ei_ < 0 ? (a_)[skip_r_] : skip_tail_;                                                                    \
    }                                                                                                                               \
  }
// a lane's 16 columns times the sdf row of the top layer (wt: the row from the lane's first column on).  ONE fmaf chain in column order: the
// sdf of a point must not depend on the tile shape of the call that holds it, so every kernel forms the same partial sums in the same order.
__device__ __forceinline__ float chain_dot16(const f32x16& a, const float* wt) {
  float dot = 0.0f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f4 w = *reinterpret_cast<const f4*>(wt + 4 * q);
    dot = fmaf(a[4 * q], w.x, dot); dot = fmaf(a[4 * q + 1], w.y, dot);
    dot = fmaf(a[4 * q + 2], w.z, dot); dot = fmaf(a[4 * q + 3], w.w, dot);
  }
  return dot;
}
__device__ __forceinline__ float chain_absmax16(const f32x16& a) {
  float mx = 0.0f;
#pragma unroll
  for (int r = 0; r < 16; r += 2) mx = fmaxf(fmaxf(fabsf(a[r]), fabsf(a[r + 1])), mx);
  return mx;
}
// A row's partial result of one 32-column block -> pm[row][slot]: the two 16-column halves combined first (one VALU lane swap).  Maxima: slot =
// wave.  sdf dot products: slot = the block's index (wave * CB + j) -- the same 8 partial sums in the same order for every tile shape
// (round 6: a 1024-ray chunk of a view used to differ from the same rays inside a 65536-ray chunk by one ulp of sdf, because <2, 2> added the
// halves of two blocks first; bench.py asserts that the two chunkings render the same image).
__device__ __forceinline__ void chain_partial_max(float* pm, int row_l, int slot, int half, float mx) {
  const float both = cnr_pair32_max(mx);
  if (half == 0) pm[row_l * 8 + slot] = both;
}
__device__ __forceinline__ void chain_partial_sum(float* pm, int row_l, int slot, int half, float dot) {
  const float both = cnr_pair32_sum(dot);
  if (half == 0) pm[row_l * 8 + slot] = both;
}

// ---- the next step's input planes from the activations in registers: the WAVES partial row maxima -> exact row scale -> hi / lo planes of
// the lane's CB blocks -> rs.  with_x: the row's extra segment (xmag: [T][4], the colour head's output kept on chip) shares the scale.
// rsf: the scale itself is kept too (the extra segment is staged with it).  rs_out: stored for the backward pass (LayerGemm::rs_out convention).
template <int RT, int CB, int WAVES>
__device__ __forceinline__ void chain_replane(const f32x16 (&acc)[CB][RT], const float* pm, unsigned char* planes, float* rs, float* rsf,
                                              const float* xmag, bool with_x, float* rs_out, long tile0, int rows_left,
                                              const ChainLane<CB>& ln, int wave) {
  constexpr int APLANE = 32 * RT * CH_ALD;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int row_l = rt * 32 + ln.pt;
    float mx = pm[row_l * 8];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) mx = fmaxf(mx, pm[row_l * 8 + w]);
    if (with_x) { const f4 g = *reinterpret_cast<const f4*>(xmag + row_l * 4); mx = fmaxf(mx, ws_absmax4(g)); }
    const float sc = split_row_scale(mx);
#pragma unroll
    for (int j = 0; j < CB; ++j) split_put16(acc[j][rt], sc, planes + row_l * CH_ALD + (ln.cbase + 32 * j) * 2, APLANE);
    if (wave == 0 && ln.half == 0) {
      rs[row_l] = cnr_pow2_rcp(sc);
      if (rsf != nullptr) rsf[row_l] = sc;
      if (rs_out != nullptr && row_l < rows_left) rs_out[tile0 + row_l] = split_rs_value(mx, sc);
    }
  }
}

// sdf = (softplus(z_top-1) . w_sdf + b_sdf) * top_scale: the 8 per-block partial sums of a row in slot order, whatever the number of waves
template <int T>
__device__ __forceinline__ void chain_sdf_finish(const float* pd, int tid, long tile0, int rows_left, const float* btop, float top_scale, float* sdf_out) {
  if (tid < T) {
    float sum = pd[tid * 8];
#pragma unroll
    for (int w = 1; w < 8; ++w) sum += pd[tid * 8 + w];
    if (tid < rows_left) sdf_out[tile0 + tid] = (sum + btop[0]) * top_scale;
  }
}

// What the forward chains store for the backward pass is read again tens of launches later: as NON-TEMPORAL stores these rows do not displace the weight fragments
// every tile streams from L2: +0.85 ... 1.0 % of the step against plain stores, same bits (profiles/r06_ab_nt_saved_activations.txt)
#define CH_SAVE_STORE(p_, v_) __builtin_nontemporal_store((v_), reinterpret_cast<f4*>(p_))

// ------------------------------------------------------------------------------------------------
// A wave's 32 x 32 output block (lane = row pt, 16 consecutive columns per half) -> global rows: through the wave's private 2 KB LDS buffer,
// 16 rows at a time (XOR-swizzled 16-byte chunks: conflict-free both ways), stored as 8 rows x 128 contiguous bytes per instruction.
// dst_tile: first row of the tile (uniform) + the wave's first column; row_base: the block's first row within the tile.
// SWITCHED: the call honours `store` (the ReLU chain's).  The unswitched calls are instantiations of their own on purpose: sharing one
// instantiation between the two kernels of cnr_chain_fwd.hip changes the code of sdf_save_chain_kernel (195 / 151 VGPRs against 190 / 146).
// store: false only under the ablation switch "no global stores" of the tuning build (wrong results); the constant true in the product build.
// ------------------------------------------------------------------------------------------------
template <bool NT = false, bool SWITCHED = false>
__device__ __forceinline__ void chain_save_block(const f32x16& a, unsigned char* tb, float* dst_tile, int ld, int row_base, int rows_left, int lane,
                                                 bool store = true) {
  const int half = lane >> 5, pt = lane & 31;
  const int sv_off = (lane >> 3) * ld + (lane & 7) * 4;                          // this lane's row / 16-byte chunk within an 8-row group
#pragma unroll
  for (int hpass = 0; hpass < 2; ++hpass) {
    if ((pt >> 4) == hpass) {
      const int r = pt & 15;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f4 v = {a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]};
        *reinterpret_cast<f4*>(tb + r * 128 + (((4 * half + q) ^ (r & 7)) << 4)) = v;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = (lane >> 3) + 8 * i, ch = lane & 7;
      const f4 v = *reinterpret_cast<const f4*>(tb + r * 128 + ((ch ^ (r & 7)) << 4));
      const int row0 = row_base + hpass * 16 + 8 * i;                             // first row of this 8-row group within the tile
      if (row0 + (lane >> 3) < rows_left && (!SWITCHED || store)) { if (NT) CH_SAVE_STORE(dst_tile + row0 * ld + sv_off, v); else *reinterpret_cast<f4*>(dst_tile + row0 * ld + sv_off) = v; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// ================================================================================================
// Host side: one launcher for the three kernels (DeviceOnce, TimingScope: cnr_hip_util.h; debug_flags: cnr_debug.h).
// ================================================================================================
constexpr size_t kChainLdsMax = 160 * 1024;   // LDS of a CU; every kernel's layout struct holds its total to it

// tile height (32 * RT points) by point count: 128-point tiles once they fill the chip's 256 CUs, 64-point tiles likewise, else 32-point tiles
// (`forced`: tuning aid).  The value chain's shapes 41 / 22 / 12 (RT * 10 + CB) follow the same thresholds.
inline int chain_rt_for(long P, int forced) { return forced ? forced : (P >= 256L * 128 ? 4 : (P >= 256L * 64 ? 2 : 1)); }

// workgroups the chip holds at once for a kernel whose LDS image is `lds` bytes: two per CU where two images fit, else one (256 CUs)
inline long chain_wgs_for(size_t lds) { return lds * 2 <= kChainLdsMax ? 512 : 256; }

// Opt-in to the CU's whole LDS (once per kernel instantiation and device), persistent grid of at most `wgs` workgroups (as many as the chip holds
// at once; CNR_CHAIN_WGS of the tuning build overrides), launch record (kind = RT * 10 + CB), launch.
template <auto Kernel, class Arg>
void chain_launch(const Arg& arg, int T, int threads, size_t lds, long wgs, long P, const char* name, int kind, double macs, double bytes, cnr_stream s) {
  const long ntiles = (P + T - 1) / T;
  const int wgs_env = debug_flags().chain_wgs;
  if (wgs_env > 0) wgs = wgs_env;
  const unsigned grid = (unsigned)(ntiles < wgs ? ntiles : wgs);
  TimingScope ts_(name, 3, kind, P, (int)(macs / 256.0), 256, 1, s, bytes);
  launch_lds<Kernel>(dim3(grid), dim3(threads), lds, kChainLdsMax, s, arg);
}

}  // namespace cnr
