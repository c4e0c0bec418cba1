// Weight-stationary layer GEMM: kernel template and launcher (included by cnr_gemm_ws_a.hip / cnr_gemm_ws_b.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>

#include "cnr_backend.h"
#include "cnr_hip_util.h"
#include "cnr_gemm_int.h"
#include "cnr_split.h"
#include "cnr_ws_tile.h"
#include "cnr_wave.h"

namespace cnr {

// ================================================================================================
// weight-stationary layer GEMM (K <= 256, up to 256 output columns per launch)
//
// The whole layer lives in the REGISTER FILE of one CU: 8 waves x 32 output columns; each wave keeps its slice of W as two f16
// planes in MFMA B-operand layout (2 planes x 16 k-blocks x 4 VGPRs = 128 VGPRs).  Points stream through in 32-row tiles: a tile is
// fetched once, gets the fused prologue (cnr_views.h), is scaled by an exact power of two per row, split into f16 hi + lo
// (11 + 11 significand bits) on its way into LDS and read by all 8 waves.  Each product is three v_mfma_f32_32x32x16_f16
// (a1 w1 + a1 w2 + a2 w1; the dropped a2 w2 is < 2^-22), fp32 accumulation, and the epilogue undoes the row / column scales
// (exact).  Measured (tools/probes/ws_probe.hip): max error 8.3e-7 vs float64 where the FP32 FMA chain of v_mfma_f32_32x32x2_f32 has
// 1.1e-6 -- also with rows spanning 12 orders of magnitude -- at 3 x 32 = 96 MFMA cycles per k16 block instead of 8 x 64 = 512.
// No weight traffic after the prologue, 16 accumulator registers, one barrier per 32 points.
// This general form stays on 32 x 32 x 16: on 16 x 16 x 32 it was 30 % slower (478 against 358 us; its k blocks sit behind run-time guards, so nothing is
// scheduled across them; profiles/r06_ab_general_mfma16.txt).  It and the stream form below (16 x 16 x 32) therefore agree to fp32 round-off, not to the bit
// (tests/test_hip_parity.py::test_stream_form_of_the_layer_kernel_matches_the_general_form).
// ================================================================================================
__device__ __forceinline__ float ws_dot4(const f4& a, const f4& b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }
// a staging register set: the NG column groups (64 columns apart) of a staging thread's row, as fetched
template <int NG>
struct WsRawSet { Raw4 r[NG]; };
// the row dot of a staged row (LayerGemm::dot_w; K <= 256 there): this thread's 16 columns, then the 16 threads of the row
__device__ __forceinline__ float ws_row_dot(const f4* v, const f4 (&dw)[4]) {
  return row16_sum((ws_dot4(v[0], dw[0]) + ws_dot4(v[1], dw[1])) + (ws_dot4(v[2], dw[2]) + ws_dot4(v[3], dw[3])));
}

// VK / EK >= 0 pin the view / epilogue kind at compile time: the interpreted switches of cnr_views.h fold away and each
// instantiation only allocates the registers its own prologue and epilogue need (-1 = generic, interpreted at run time).
// PLAIN promises an epilogue without tail fill and without a split point (most launches): that code folds away as well.
// K17 admits a 17th k16 block (K up to 272: the layers whose input is a 256-wide hidden vector plus a few concatenated columns).
// FULLK promises K > (NKB - 1) * 16, i.e. every k16 block is live: the per-block guards fold away and the LDS fragment reads of the
// next block can be scheduled across the MFMAs of the current one.
template <int VK, int EK, bool PLAIN, bool K17 = false, bool FULLK = false>
__global__ __launch_bounds__(WS_THREADS, 1) void layer_gemm_ws_kernel(const LayerGemm g_in, int tiles_per_wg, int wrows, int rev) {
  constexpr int NKB = K17 ? 17 : 16;
  constexpr int NG = K17 ? 5 : 4;               // column groups of a staging thread (17th block: 4 of the 16 threads of a row)
  LayerGemm g = g_in;
  if (VK >= 0) g.A.kind = VK;
  if (EK >= 0) g.E.kind = EK;
  if (PLAIN) { g.E.tail_src = nullptr; g.E.tail_n = 0; g.E.split = 1 << 30; }
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long Pn = g.P_dev ? (long)*g.P_dev : g.P;
  const WsRange R((Pn + WS_TP - 1) / WS_TP, (long)blockIdx.x * tiles_per_wg, tiles_per_wg, rev);
  const int n = R.n;
  if (n == 0) return;
  const int nkb = FULLK ? NKB : (g.K + 15) >> 4;   // 1..NKB k16 blocks
  const int kpad = nkb * 16;
  const int ald = kpad * 2 + 16;                // bytes per LDS row of one plane (+16: conflict-free ds_read_b128)
  const int aplane = WS_TP * ald;
  const int abuf = 2 * aplane + 128;            // two planes + 32 row scales
  float* T = reinterpret_cast<float*>(smem_b + 2 * abuf) + wave * (32 * WS_TLD);
  const int c0 = g.col0 + wave * 32;            // this wave's first output column
  const bool has_w = c0 < wrows;
  const int ncols_live = g.E.n_out + (g.E.tail_src ? g.E.tail_n : 0);

  // ---- resident weights (two f16 planes of this wave's 32 rows of W)
  f16x8 w1[NKB], w2[NKB];
  ws_wfrag32<NKB, false>(w1, w2, g, has_w ? c0 + (lane & 31) : 0, lane, nkb);
  f4 wsc = {1.f, 1.f, 1.f, 1.f};               // inverse column scales of the 4 columns this lane finishes in the epilogue
  if (has_w) wsc = *reinterpret_cast<const f4*>(g.wscale + c0 + (lane & 7) * 4);
  const int ecol = c0 + (lane & 7) * 4;         // ... and their epilogue path / bias (fixed per lane for the whole launch)
  const bool efast = epi_fast4(g.E, ecol);
  f4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (efast) bias4 = epi_bias4(g.E, ecol);

  // ---- staging map: 16 threads per row, 4 consecutive columns each, up to NG passes of 64 columns
  const int srow = tid >> 4, scol = (tid & 15) * 4;
  bool pv[NG];
#pragma unroll
  for (int q = 0; q < NG; ++q) pv[q] = 64 * q + scol < kpad;
  // DEEP: a second staging register set keeps the activation tiles of two iterations in flight (+7 % on a plain layer,
  // tools/probes/ws_depth_probe.hip); only the instantiations with >= 20 spare VGPRs take it
  constexpr bool DEEP = PLAIN && !K17 && FULLK && (VK == VK_DIRECT || VK == VK_SOFTPLUS) && (EK == EK_STORE || EK == EK_RELU || EK == EK_SDF_TOP);
  WsRawSet<NG> sa, sb;
  const f4 z4 = {0.f, 0.f, 0.f, 0.f};
  constexpr bool WS_DOT = (EK == EK_SDF_TOP || EK < 0);   // the row dot is compiled into the top SDF layer's instantiation (and the runtime-kind one)
  f4 dw[4] = {z4, z4, z4, z4};                    // row-dot weights of this thread's columns (LayerGemm::dot_w; K <= 256 there)
  float dot_b = 0.0f;
  if (WS_DOT && g.dot_w) {
#pragma unroll
    for (int q = 0; q < 4; ++q) if (pv[q]) dw[q] = *reinterpret_cast<const f4*>(g.dot_w + 64 * q + scol);
    if (g.dot_bias) dot_b = g.dot_bias[0];
  }
#pragma unroll
  for (int q = 0; q < NG; ++q) { sa.r[q].a = z4; sa.r[q].b = z4; sb.r[q] = sa.r[q]; }
  auto fetch = [&](const int i, WsRawSet<NG>& S) {
    long row = R.tile(i) * WS_TP + srow; if (row >= Pn) row = Pn - 1;
#pragma unroll
    for (int q = 0; q < NG; ++q) if (pv[q]) S.r[q] = view_fetch4(g.A, row, 64 * q + scol);
  };
  auto put = [&](const int buf, const int i, const WsRawSet<NG>& S) {
    f4 v[NG];
#pragma unroll
    for (int q = 0; q < NG; ++q) v[q] = pv[q] ? view_finish4(g.A, S.r[q], 64 * q + scol) : z4;
    float dsum = 0.0f;
    if (WS_DOT && g.dot_w) dsum = ws_row_dot(v, dw);
    unsigned char* B = smem_b + buf * abuf;
    const bool owner = (tid & 15) == 0;
    const WsRowScale rsc = ws_stage_put<NG>(v, pv, B + srow * ald + scol * 2, aplane, reinterpret_cast<float*>(B + 2 * aplane), srow, owner);
    if (owner) {
      const long prow = R.tile(i) * WS_TP + srow;
      if (WS_DOT && g.dot_w && prow < Pn) g.dot_out[prow] = (dsum + dot_b) * g.dot_scale;
      if (g.rs_out && prow < Pn) g.rs_out[prow] = split_rs_value(rsc.mx, rsc.sc);
    }
  };

  // Waves 0..3 (rows 0..15 of a tile) and waves 4..7 (rows 16..31) share the SIMDs pairwise and run half an iteration out of
  // phase: the late group converts + stores its half of tile t+1 (fetched one iteration earlier) and fetches tile t+2 BEFORE
  // its MFMAs of tile t, the early group fetches tile t+1 before and stores it after -- so one wave of each SIMD is in the
  // matrix pipe while the other does prologue math / LDS stores / epilogue.  One barrier per tile.
  const bool late = wave >= 4;
  // MFMAs + epilogue of the range's tile i from LDS buffer buf
  auto compute = [&](const int i, const int buf) {
    const long t = R.tile(i);
    f32x16 acc;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
    const unsigned char* Ab = smem_b + buf * abuf + (lane & 31) * ald + (lane >> 5) * 16;
    if (has_w) ws_product32<NKB>(acc, Ab, aplane, nkb, [&](const int kb, f16x8& a, f16x8& b) { a = w1[kb]; b = w2[kb]; });
    // epilogue of this 32 x 32 tile: undo the exact row / column scales, then the fused epilogue on 4 columns per lane.
    // The side inputs of all four row groups are requested first: one memory round trip per tile, and no load has to
    // wait behind the stores of the previous row group.
    if (c0 < ncols_live) {
      const float* rs = reinterpret_cast<const float*>(smem_b + buf * abuf + 2 * aplane);
      ws_acc_to_tile32(T, acc, lane >> 5, lane & 31);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      constexpr int EG = (EK == EK_SWEEP || EK == EK_VBACK) ? 2 : 4;   // row groups whose side inputs are in flight together (register budget)
#pragma unroll
      for (int i0 = 0; i0 < 4; i0 += EG) {
        EpiRaw4 er[EG];
#pragma unroll
        for (int q = 0; q < EG; ++q) {
          long row = t * WS_TP + (lane >> 3) + 8 * (i0 + q);
          if (row >= Pn) row = Pn - 1;
          if (efast) er[q] = epi_fetch4(g.E, row, ecol);
        }
#pragma unroll
        for (int q = 0; q < EG; ++q) {
          const int rr = (lane >> 3) + 8 * (i0 + q);
          const long row = t * WS_TP + rr;
          const f4 v = ws_tile_row4(T, rs, rr, (lane & 7) * 4, wsc);
          if (row < Pn) {
            if (efast) epi_finish4(g.E, row, ecol, v, bias4, er[q]);
            else epi_apply4(g.E, row, ecol, v);
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  };
  if (!DEEP) {
    fetch(0, sa);
    put(0, 0, sa);
    if (late && 1 < n) fetch(1, sa);
    cnr_lds_barrier();
    for (int i = 0; i < n; ++i) {
      const int buf = i & 1;
      const bool more = i + 1 < n;
      if (!late) {
        if (more) fetch(i + 1, sa);
      } else if (more) {
        put(buf ^ 1, i + 1, sa);
        if (i + 2 < n) fetch(i + 2, sa);
      }
      compute(i, buf);
      if (!late && more) put(buf ^ 1, i + 1, sa);
      cnr_lds_barrier();
    }
  } else {
    // two staging sets: tile i lives in set a for even i, set b for odd i.  Early waves keep tiles i+1 and i+2 in flight,
    // late waves i+2 and i+3.
    fetch(0, sa);
    put(0, 0, sa);
    if (1 < n) fetch(1, sb);
    if (late && 2 < n) fetch(2, sa);
    cnr_lds_barrier();
    for (int i = 0; i < n; i += 2) {
      {   // even tile i (LDS buffer 0): the next tile waits in set b, set a is free
        const bool more = i + 1 < n;
        if (!late) {
          if (i + 2 < n) fetch(i + 2, sa);
        } else if (more) {
          put(1, i + 1, sb);
          if (i + 3 < n) fetch(i + 3, sb);
        }
        compute(i, 0);
        if (!late && more) put(1, i + 1, sb);
        cnr_lds_barrier();
      }
      if (i + 1 < n) {   // odd tile i + 1 (LDS buffer 1): the next tile waits in set a, set b is free
        const bool more = i + 2 < n;
        if (!late) {
          if (i + 3 < n) fetch(i + 3, sb);
        } else if (more) {
          put(0, i + 2, sa);
          if (i + 4 < n) fetch(i + 4, sa);
        }
        compute(i + 1, 1);
        if (!late && more) put(0, i + 2, sa);
        cnr_lds_barrier();
      }
    }
  }
}

// walk-direction parity of consecutive layer launches: process-wide, atomic (host threads may launch concurrently); it only picks the
// order in which a launch visits its tiles, never a value
inline int ws_next_rev() { static std::atomic<unsigned> parity{0}; return (int)(parity.fetch_add(1u, std::memory_order_relaxed) & 1u); }

// ================================================================================================
// "Stream" form of the same kernel for the launches that need none of its special cases: K in (240, 256], 256 live output columns
// whose epilogue takes the 16-byte path in every lane, no tail fill, no split point, a point count that is a multiple of the tile
// height and known on the host (ws_stream_ok).
// Same tiles, same arithmetic, same order of operations per output element -- what changes is the control flow around the memory
// operations: one loop per wave group (early / late), prefetches issued unconditionally (tile index clamped to the range), first
// iterations peeled.  Every path through a loop then issues the same memory operations in the same order, and the compiler's
// s_waitcnt bookkeeping stays exact: where a staging register set is consumed it waits for THAT set (vmcnt(8..15)) instead of falling back
// to vmcnt(0), which made every wave wait once per tile for its just-issued epilogue stores and for the deeper prefetch
// (tools/probes/ws_depth_probe.hip -> ws_depth3_probe.hip: 0.313 -> 0.280 ms on a plain layer).
// ================================================================================================
// Branch-free forms of epi_fetch4 / epi_finish4 for an epilogue without split point and tail fill (the stream kernel's promise): a branch
// between two memory operations costs the compiler its count of what is still in flight.
// The epilogue's side inputs (pre-activations, ReLU masks, the cotangent a value-backward launch adds to) are read once per launch: as NON-TEMPORAL loads they do not
// push the lines the launch re-reads (its own input tile, the weights) or hands to the next launch (its output rows) out of L2 / Infinity Cache: +0.2-0.3 % of the step,
// same bits (profiles/r06_ab_nt_side_inputs.txt).  The STAGED tile must stay a plain load: non-temporal there costs 2 % (the fused launches read it twice).
// ... and the second-order cotangent a sweep launch writes on z (picked up by the value-backward chain many launches later) as a non-temporal store: +0.2 % (same record).
#define WS_NTLOAD(p_) __builtin_nontemporal_load(reinterpret_cast<const f4*>(p_))
template <int EK>
__device__ __forceinline__ EpiRaw4 epi_fetch4_plain(const Epi& e, long row, int col) {
  EpiRaw4 r;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  r.a = zero; r.b = zero;
  if constexpr (EK == EK_SWEEP) {
    r.a = WS_NTLOAD(e.z + row * e.ldz + col);
    r.b = WS_NTLOAD(e.v + row * e.ldv + col);   // ldv == 0: the broadcast row
  } else if constexpr (EK == EK_VBACK) {
    r.a = WS_NTLOAD(e.z + row * e.ldz + col);
    r.b = WS_NTLOAD(e.o1 + row * e.ld1 + col);
  } else if constexpr (EK == EK_RELU_MASK) {
    r.a = WS_NTLOAD(e.aux + row * e.ldaux + col);
  }
  return r;
}
template <int EK>
__device__ __forceinline__ void epi_finish4_plain(const Epi& e, long row, int col, const f4& acc, const f4& b, const EpiRaw4& raw) {
  if constexpr (EK == EK_SWEEP) {
    const f4 zz = raw.a, vv = raw.b;
    f4 o1, o2;
    o1.x = softplus100_d2(zz.x) * (vv.x * e.vscale) * acc.x; o2.x = softplus100_d1(zz.x) * acc.x;
    o1.y = softplus100_d2(zz.y) * (vv.y * e.vscale) * acc.y; o2.y = softplus100_d1(zz.y) * acc.y;
    o1.z = softplus100_d2(zz.z) * (vv.z * e.vscale) * acc.z; o2.z = softplus100_d1(zz.z) * acc.z;
    o1.w = softplus100_d2(zz.w) * (vv.w * e.vscale) * acc.w; o2.w = softplus100_d1(zz.w) * acc.w;
    __builtin_nontemporal_store(o1, reinterpret_cast<f4*>(e.o1 + row * e.ld1 + col));   // (the second-order cotangent on z: picked up by the value-backward chain many launches later)
    *reinterpret_cast<f4*>(e.o2 + row * e.ld2 + col) = o2;
  } else if constexpr (EK == EK_VBACK) {
    const f4 zz = raw.a;
    f4 o = raw.b;
    o.x = softplus100_d1(zz.x) * (acc.x * e.scale) + o.x;
    o.y = softplus100_d1(zz.y) * (acc.y * e.scale) + o.y;
    o.z = softplus100_d1(zz.z) * (acc.z * e.scale) + o.z;
    o.w = softplus100_d1(zz.w) * (acc.w * e.scale) + o.w;
    *reinterpret_cast<f4*>(e.o1 + row * e.ld1 + col) = o;
  } else {
    epi_finish4(e, row, col, acc, b, raw);
  }
}

template <int EK, bool GEN>
__device__ __forceinline__ EpiRaw4 epi_fetch4_sel(const Epi& e, long row, int col) {
  if constexpr (GEN) return epi_fetch4(e, row, col); else return epi_fetch4_plain<EK>(e, row, col);
}
template <int EK, bool GEN>
__device__ __forceinline__ void epi_finish4_sel(const Epi& e, long row, int col, const f4& acc, const f4& b, const EpiRaw4& raw) {
  if constexpr (GEN) epi_finish4(e, row, col, acc, b, raw); else epi_finish4_plain<EK>(e, row, col, acc, b, raw);
}

// GEN: the epilogue keeps its tail fill / split point (skip-connection layers); it then runs the general 16-byte epilogue code per lane.
template <int VK, int EK, bool GEN = false>
__global__ __launch_bounds__(WS_THREADS, 1) void layer_gemm_ws_stream_kernel(const LayerGemm g_in, int tiles_per_wg, int rev) {
  constexpr int NKB = 16;
  LayerGemm g = g_in;
  g.A.kind = VK; g.E.kind = EK;
  if (!GEN) { g.E.tail_src = nullptr; g.E.tail_n = 0; g.E.split = 1 << 30; }
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long Pn = g.P;                                  // a multiple of the tile height, known on the host (ws_stream_ok)
  const WsRange R(Pn / WS_TP, (long)blockIdx.x * tiles_per_wg, tiles_per_wg, rev);
  const int n = R.n;
  if (n == 0) return;
  constexpr int kpad = NKB * 16;
  constexpr int ald = kpad * 2 + 16;
  constexpr int aplane = WS_TP * ald;
  constexpr int abuf = 2 * aplane + 128;
  float* T = reinterpret_cast<float*>(smem_b + 2 * abuf) + wave * (32 * WS_TLD);
  const int c0 = g.col0 + wave * 32;

  // (round 6) the stream form on v_mfma_f32_16x16x32_f16 -- 12 % cheaper per FLOP than the 32 x 32 x 16 shape and a 15 % higher clock under the board's power
  // limit (profiles/r06_mfma_shapes.txt; against the 32 x 32 x 16 form: profiles/r06_ab_mfma16_ws_stream.txt): B fragments of this wave's 2 x 16 output columns, lane (n = lane & 15, kg = lane >> 4) holds W[c0 + 16 cb + n][32 kb + 8 kg ..]
  constexpr int NKB2 = NKB / 2;
  f16x8 w1[NKB2][2], w2[NKB2][2];
  ws_wfrag16<NKB2>(w1, w2, g, c0, lane);
  const f4 wsc = *reinterpret_cast<const f4*>(g.wscale + c0 + (lane & 7) * 4);
  const int ecol = c0 + (lane & 7) * 4;
  const f4 bias4 = epi_bias4(g.E, ecol);
  const int srow = tid >> 4, scol = (tid & 15) * 4;
  // second staging set (tiles fetched two ahead) where the registers allow it without spilling: the softplus prologue needs the room
  constexpr bool DEEP = VK == VK_DIRECT && (EK == EK_STORE || EK == EK_RELU || EK == EK_SDF_TOP);
  WsRawSet<4> sa, sb;
  const f4 z4 = {0.f, 0.f, 0.f, 0.f};
  f4 dw[4] = {z4, z4, z4, z4};                    // row-dot weights (LayerGemm::dot_w): only the top SDF layer's instantiation carries them
  float dot_b = 0.0f;
  if (EK == EK_SDF_TOP && g.dot_w) {
#pragma unroll
    for (int q = 0; q < 4; ++q) dw[q] = *reinterpret_cast<const f4*>(g.dot_w + 64 * q + scol);
    if (g.dot_bias) dot_b = g.dot_bias[0];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) { sa.r[q].a = z4; sa.r[q].b = z4; sb.r[q] = sa.r[q]; }
  // Fetch and put of the range's tile tile_ through staging set S_ (tile_ may run past the range: clamped, the redundant fetch / LDS tile of
  // the last iterations is never used).  They stay macros: as lambdas over the same sets 7 of the 22 instantiations took 1 - 4 more VGPRs
  // (profiles/ws_refactor_ab.txt).
#define WSS_FETCH(tile_, S_)                                                      \
  {                                                                               \
    const long row_ = R.prefetch(tile_) * WS_TP + srow;                           \
    (S_).r[0] = view_fetch4(g.A, row_, scol);                                       \
    (S_).r[1] = view_fetch4(g.A, row_, 64 + scol);                                  \
    (S_).r[2] = view_fetch4(g.A, row_, 128 + scol);                                 \
    (S_).r[3] = view_fetch4(g.A, row_, 192 + scol);                                 \
    __builtin_amdgcn_sched_barrier(0);                                            \
  }
#define WSS_PUT(buf_, tile_, S_)                                                  \
  {                                                                               \
    __builtin_amdgcn_s_setprio(2);   /* the conversion + LDS stores of the next tile gate every wave's next barrier (-0.05 ms per step) */ \
    const f4 v0 = view_finish4(g.A, (S_).r[0], scol);                                                               \
    const f4 v1 = view_finish4(g.A, (S_).r[1], 64 + scol);                                                          \
    const f4 v2 = view_finish4(g.A, (S_).r[2], 128 + scol);                                                         \
    const f4 v3 = view_finish4(g.A, (S_).r[3], 192 + scol);                                                         \
    const f4 v_[4] = {v0, v1, v2, v3};                                            \
    const bool all_[4] = {true, true, true, true};                                \
    unsigned char* B_ = smem_b + (buf_) * abuf;                                   \
    const WsRowScale rsc_ = ws_stage_put<4>(v_, all_, B_ + srow * ald + scol * 2, aplane, reinterpret_cast<float*>(B_ + 2 * aplane), srow, (tid & 15) == 0); \
    float dsum_ = 0.0f;                                                           \
    if (EK == EK_SDF_TOP && g.dot_w) dsum_ = ws_row_dot(v_, dw);                  \
    if ((tid & 15) == 0) {                                                        \
      const long prow_ = R.prefetch(tile_) * WS_TP + srow;                        \
      if (EK == EK_SDF_TOP && g.dot_w) g.dot_out[prow_] = (dsum_ + dot_b) * g.dot_scale; \
      if (g.rs_out) g.rs_out[prow_] = split_rs_value(rsc_.mx, rsc_.sc);           \
    }                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                            \
    __builtin_amdgcn_s_setprio(0);                                                \
  }
  const bool late = wave >= 4;
  constexpr bool EPRE = EK == EK_VBACK || EK == EK_RELU_MASK || EK == EK_SWEEP;
  EpiRaw4 ern[4];
  if (EPRE) {
#pragma unroll
    for (int i = 0; i < 4; ++i) ern[i] = epi_fetch4_sel<EK, GEN>(g.E, R.tile(0) * WS_TP + (lane >> 3) + 8 * i, ecol);
  }
  auto compute = [&](const int i, const int buf) {
    const long t = R.prefetch(i);
    f32x4 acc[2][2];   // [row block of 16 points][column block of 16 columns]
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[rb][cb][j] = 0.0f;
    ws_product16<NKB2>(acc, smem_b + buf * abuf + (lane & 15) * ald + (lane >> 4) * 16, ald, aplane, w1, w2);
    // (scheduling fences between the phases: the blocks are branch-free now, and an unconstrained scheduler hoists the next phase's loads
    // across the MFMA block until the register file spills)
    __builtin_amdgcn_sched_barrier(0);
    const float* rs = reinterpret_cast<const float*>(smem_b + buf * abuf + 2 * aplane);
    ws_acc_to_tile16(T, acc, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if constexpr (EPRE) {
      // side inputs requested one tile ahead (ern): when they are consumed here they are the OLDEST loads in flight, so the wait
      // leaves the prefetched activation tile and the stores of the previous tiles alone (a load consumed right after its issue is the
      // youngest one, and the in-order counter then drains everything before it: twice per tile in the general kernel)
      const long tn = R.prefetch(i + 1);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rr = (lane >> 3) + 8 * q, cc = (lane & 7) * 4;
        const long row = t * WS_TP + rr;
        const f4 v = ws_tile_row4(T, rs, rr, cc, wsc);
        epi_finish4_sel<EK, GEN>(g.E, row, ecol, v, bias4, ern[q]);
        ern[q] = epi_fetch4_sel<EK, GEN>(g.E, tn * WS_TP + rr, ecol);
      }
    } else {
    constexpr int EG = (EK == EK_SWEEP || EK == EK_VBACK) ? 2 : 4;
#pragma unroll
    for (int i0 = 0; i0 < 4; i0 += EG) {
      EpiRaw4 er[EG];
#pragma unroll
      for (int q = 0; q < EG; ++q) er[q] = epi_fetch4_sel<EK, GEN>(g.E, t * WS_TP + (lane >> 3) + 8 * (i0 + q), ecol);
#pragma unroll
      for (int q = 0; q < EG; ++q) {
        const int rr = (lane >> 3) + 8 * (i0 + q), cc = (lane & 7) * 4;
        const long row = t * WS_TP + rr;
        const f4 v = ws_tile_row4(T, rs, rr, cc, wsc);
        epi_finish4_sel<EK, GEN>(g.E, row, ecol, v, bias4, er[q]);   // (no row test: every tile is full, so no branch sits between the memory operations)
      }
    }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  // LDS buffer of the range's tile i is i & 1.  All waves execute one barrier before the loops and one per tile.
  if (!DEEP) {
    WSS_FETCH(0, sa)
    WSS_PUT(0, 0, sa)
    if (!late) {
      cnr_lds_barrier();
      for (int i = 0; i < n; ++i) {
        const int buf = i & 1;
        WSS_FETCH(i + 1, sa)
        compute(i, buf);
        WSS_PUT(buf ^ 1, i + 1, sa)
        cnr_lds_barrier();
      }
    } else {
      WSS_FETCH(1, sa)
      cnr_lds_barrier();
#define WSS_LATE1(i_)                                                             \
      {                                                                           \
        const int buf = (i_) & 1;                                        \
        WSS_PUT(buf ^ 1, (i_) + 1, sa)                                             \
        WSS_FETCH((i_) + 2, sa)                                                    \
        compute((i_), buf);                                                       \
        cnr_lds_barrier();                                                        \
      }
      WSS_LATE1(0)   // peeled: the loop header then only sees the steady state
      for (int i = 1; i < n; ++i) WSS_LATE1(i)
#undef WSS_LATE1
    }
  } else {
    // two staging sets: tile i lives in set a for even i, set b for odd i; early waves keep tiles i + 1 and i + 2 in flight,
    // late waves i + 2 and i + 3.  Two tiles per trip without a branch in between: the trailing half-trip of an odd range repeats the
    // last tile (clamped index; these epilogues are plain stores, so writing the same values twice is harmless).
    WSS_FETCH(0, sa)
    WSS_PUT(0, 0, sa)
    WSS_FETCH(1, sb)
    if (!late) {
      cnr_lds_barrier();
#define WSS_EARLY2(i_)                                                            \
      {                                                                           \
        WSS_FETCH((i_) + 2, sa)                                                    \
        compute((i_), 0);                                                         \
        WSS_PUT(1, (i_) + 1, sb)                                                   \
        cnr_lds_barrier();                                                        \
        WSS_FETCH((i_) + 3, sb)                                                    \
        compute((i_) + 1, 1);                                                     \
        WSS_PUT(0, (i_) + 2, sa)                                                   \
        cnr_lds_barrier();                                                        \
      }
      WSS_EARLY2(0)
      for (int i = 2; i < n; i += 2) WSS_EARLY2(i)
#undef WSS_EARLY2
    } else {
      WSS_FETCH(2, sa)
      cnr_lds_barrier();
#define WSS_LATE2(i_)                                                             \
      {                                                                           \
        WSS_PUT(1, (i_) + 1, sb)                                                   \
        WSS_FETCH((i_) + 3, sb)                                                    \
        compute((i_), 0);                                                         \
        cnr_lds_barrier();                                                        \
        WSS_PUT(0, (i_) + 2, sa)                                                   \
        WSS_FETCH((i_) + 4, sa)                                                    \
        compute((i_) + 1, 1);                                                     \
        cnr_lds_barrier();                                                        \
      }
      WSS_LATE2(0)
      for (int i = 2; i < n; i += 2) WSS_LATE2(i)
#undef WSS_LATE2
    }
  }
#undef WSS_FETCH
#undef WSS_PUT
}

// host-side test for the stream form: every wave has weights and a live 32-column epilogue block, every lane the 16-byte epilogue path
inline bool ws_stream_ok(const LayerGemm& g, int wrows) {
  const bool off = debug_flags().ws_nostream;   // debugging aid: the general kernel for every launch
  if (off || g.K <= 240 || g.K > 256 || g.P_dev != nullptr || (g.P % WS_TP) != 0) return false;
  if (g.dot_w != nullptr && g.E.kind != EK_SDF_TOP) return false;   // (the row dot lives in that instantiation of the stream form only)
  const int live = g.E.n_out + (g.E.tail_src ? g.E.tail_n : 0);
  if (g.col0 + 256 > wrows || g.col0 + 256 > live) return false;
  for (int c = g.col0; c < g.col0 + 256; c += 4) if (!epi_fast4(g.E, c)) return false;
  return true;
}
inline bool ws_stream_plain(const LayerGemm& g) { return g.E.tail_src == nullptr && g.E.split == (1 << 30); }

template <int VK, int EK, bool GEN>
static void launch_ws_stream(const LayerGemm& g, cnr_stream s) {
  constexpr int abuf = 2 * WS_TP * (16 * 32 + 16) + 128;
  const size_t lds = (size_t)2 * abuf + (size_t)8 * 32 * WS_TLD * sizeof(float);
  const long ntiles = (g.P + WS_TP - 1) / WS_TP;
  if (ntiles == 0) return;
  const int ws_wgs = debug_flags().ws_wgs;
  long tpw = (ntiles + ws_wgs - 1) / ws_wgs;
  if (tpw < 1) tpw = 1;
  const unsigned grid = (unsigned)((ntiles + tpw - 1) / tpw);
  const int ws_serp = debug_flags().ws_serp;
  const int rev = ws_serp ? ws_next_rev() : 0;
  TimingScope ts_("layer_gemm_ws", 0, 100 + (g.N + 31) / 32, g.P, g.N, g.K, 1, s, layer_gemm_bytes(g));
  launch_lds<layer_gemm_ws_stream_kernel<VK, EK, GEN>>(dim3(grid), dim3(WS_THREADS), lds, 160 * 1024, s, g, (int)tpw, rev);
}

template <int VK, int EK, bool PLAIN, bool K17, bool FULLK>
static void launch_ws_tk(const LayerGemm& g, int wrows, cnr_stream s) {
  const int nkb = (g.K + 15) / 16;
  const int abuf = 2 * WS_TP * (nkb * 32 + 16) + 128;
  const size_t lds = (size_t)2 * abuf + (size_t)8 * 32 * WS_TLD * sizeof(float);
  const long ntiles = (g.P + WS_TP - 1) / WS_TP;
  if (ntiles == 0) return;
  const int ws_wgs = debug_flags().ws_wgs;       // tuning knobs (defaults measured on MI355X: 256 / 1)
  const int ws_mintpw = debug_flags().ws_mintpw;
  long tpw = (ntiles + ws_wgs - 1) / ws_wgs;   // one workgroup per CU: the weights are loaded once per CU (measured best of 256 / 512 / 768 / 1024)
  if (tpw < ws_mintpw) tpw = ws_mintpw;
  const unsigned grid = (unsigned)((ntiles + tpw - 1) / tpw);
  const int ws_serp = debug_flags().ws_serp;   // alternate walk direction: +0.35 % (A/B, the last rows of a producer are still in L2)
  const int rev = ws_serp ? ws_next_rev() : 0;
  TimingScope ts_("layer_gemm_ws", 0, 100 + (g.N + 31) / 32, g.P, g.N, g.K, 1, s, layer_gemm_bytes(g));
  launch_lds<layer_gemm_ws_kernel<VK, EK, PLAIN, K17, FULLK>>(dim3(grid), dim3(WS_THREADS), lds, 160 * 1024, s, g, (int)tpw, wrows, rev);
}

template <int VK, int EK, bool PLAIN, bool K17 = false>
static void launch_ws_t(const LayerGemm& g, int wrows, cnr_stream s) {
  const int nkb = (g.K + 15) / 16;
  if constexpr (!K17 && VK >= 0 && EK >= 0) {
    if (ws_stream_ok(g, wrows) && ws_stream_plain(g) == PLAIN) { launch_ws_stream<VK, EK, !PLAIN>(g, s); return; }
  }
  if (nkb == (K17 ? 17 : 16)) launch_ws_tk<VK, EK, PLAIN, K17, true>(g, wrows, s);
  else launch_ws_tk<VK, EK, PLAIN, K17, false>(g, wrows, s);
}

}  // namespace cnr
