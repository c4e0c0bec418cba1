// Chain-fused SAVING forward kernels for gfx950 (MI355X / CDNA4): the ReLU stacks of the render path (colour network, relight network)
// in ONE launch.  A workgroup carries a tile of 32 * RT points through every layer of both stacks; between layers the activations stay on
// the CU as two f16 planes in LDS (the chain-fused value kernel's scheme, cnr_chain.hip: error-free hi / lo split of the exactly
// power-of-two scaled fp32 row, 3 x v_mfma_f32_32x32x16_f16 per product, fp32 accumulation, weights streamed from L2 in MFMA-fragment
// order four k16 blocks ahead, TRANSPOSED product so that a lane owns one point x 16 consecutive output columns).
//
// What the forward pass must leave behind for the backward pass -- every hidden layer's ReLU output (1 KB per point and layer) and the
// row scales of the layer inputs -- is what sank the first saving variant of the chain kernel (commit eeb54d9): in the transposed layout a
// lane holds a 64-byte piece of a row, a wave-wide 16-byte store touches 64 different 64-byte segments, and such stores drain at about
// 8 B/clk/CU.  Here every wave passes its 32 x 32 output block through a private 2 KB LDS buffer, 16 rows at a time (XOR-swizzled 16-byte
// chunks: conflict-free both ways), and stores it as 8 rows x 128 contiguous bytes per instruction -- full cache lines, the store pattern
// of the per-layer kernel's epilogue.
//
// Against the per-layer launches this removes, per point: the read-back of every hidden activation (7 x 1 KB), the second read of the
// 3-wide heads' input (2 x 1 KB), 9 launches, and for the narrow inputs (relight in_layer: 48 columns; colour layer 0: 256 + 16..48
// columns; relight y-layer: 256 + 3) the special launches that re-read 1 KB/point tensors for a 48-column product.
//
// Layers whose input is wider than 256 columns (colour layer 0: [feat | p g PE(v)], relight y-layer: [h | rgb]) run as TWO input
// segments through the same LDS planes: the 256 main columns, then -- one barrier later -- the 16..48 extra columns staged over them, the
// accumulators carried across.  Both segments share ONE row scale (the power of two of the whole input row, as the per-layer kernel
// forms it), so no accumulator rescaling is needed and the k16 blocks are summed in the per-layer kernel's order.
// The 3-wide heads (rgb, relight offset) are fp32 dot products of the last hidden layer's ReLU output while it is still in registers;
// rgb stays in LDS for the relight y-layer and the relight head's inverse-sigmoid combination.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "cnr_backend.h"
#include "cnr_hip_util.h"
#include "cnr_gemm_int.h"
#include "cnr_chain_util.h"

namespace cnr {

// The kernel's LDS image, stated once: the kernel carves its regions from these byte offsets, the launcher passes the total
template <int RT>
struct ReluChainLds {
  static constexpr int T = 32 * RT;
  static constexpr int rs = 2 * T * CH_ALD;                 // (in front: [2][T][CH_ALD] hi | lo planes; at the end of a chain [T][8][4] partial head dot products)  [T] 1 / row scale of the current step's input
  static constexpr int rsf = rs + T * 4;                    // [T] the row scale itself (the extra segment is staged with it)
  static constexpr int pm = rsf + T * 4;                    // [T][8] per-wave partial row maxima
  static constexpr int cwb = pm + T * 8 * 4;                // [2][512] column scales | biases of the current / next step
  static constexpr int rgbs = cwb + 2 * 512 * 4;            // [T][4] output of the colour head (rgb, 0)
  static constexpr int tb = rgbs + T * 4 * 4;               // [8 waves][16 rows][128 B] transposition buffers
  static constexpr int total = tb + 8 * 2048;
  static_assert((size_t)total <= kChainLdsMax, "LDS budget");
};

template <int RT>
__global__ __launch_bounds__(512, 1) void relu_chain_fwd_kernel(const ReluChainFwd c) {
  constexpr int T = 32 * RT;
  constexpr int APLANE = T * CH_ALD;
  using Lds = ReluChainLds<RT>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* rs = reinterpret_cast<float*>(smem + Lds::rs);
  float* rsf = reinterpret_cast<float*>(smem + Lds::rsf);
  float* pm = reinterpret_cast<float*>(smem + Lds::pm);
  float* cwb = reinterpret_cast<float*>(smem + Lds::cwb);
  float* rgbs = reinterpret_cast<float*>(smem + Lds::rgbs);
  const int tid0 = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);   // (scalar: the per-wave bases below stay in SGPRs)
  unsigned char* tb = smem + Lds::tb + wave * 2048;          // this wave's [16 rows][128 B] transposition buffer
  float* hp = reinterpret_cast<float*>(smem);                // [T][8][4] partial head dot products (in the planes: dead at the end of a chain)
  const long P = c.P_dev != nullptr ? (long)*c.P_dev : c.P;   // (compacted runs: only the device knows how many rows there are)
  const int* const ridx = c.row_idx;
  const long ntiles = (P + T - 1) / T;

  f16x8 wr1[4][1], wr2[4][1];                                // weight fragment ring: 4 k16 blocks in flight

  chain_wprime<1>(wr1, wr2, chain_wlane<1>(c.st[0].Wf, c.st[0].nkb_w, wave, tid0 & 63), c.st[0].nkb_w, 0, c.st[0].nkb_main);
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long tile0 = tile * T;
    const int rows_left = (int)((P - tile0) < T ? (P - tile0) : T);                // rows of this tile that exist (>= 1)
    chain_cw_park(cwb, tid0, chain_cw_fetch(c.st[0], tid0));
    for (int s = 0; s < c.nsteps; ++s) {
      const ChainLane<1> ln(tid0, wave);
      const int tid = ln.tid, lane = ln.lane, half = ln.half, pt = ln.pt, cbase = ln.cbase;
      const ChainFwdStep& S = c.st[s];
      const bool last_step = s + 1 == c.nsteps;
      const ChainFwdStep& Sn = c.st[last_step ? 0 : s + 1];
      const unsigned short* wlane = chain_wlane<1>(S.Wf, S.nkb_w, wave, lane);
      const f4 cw_next = chain_cw_fetch(Sn, tid);    // lands while the MFMAs run; parked in LDS behind the row-max barrier
      float hbias[3] = {0.f, 0.f, 0.f};                           // a head follows this step: its biases now (same reason as for the head's weight rows below)
      if (S.head != 0) {
        const ChainFwdHead& Hh = S.head == 1 ? c.col_head : c.rel_head;
#pragma unroll
        for (int j = 0; j < 3; ++j) hbias[j] = Hh.bias[j < Hh.n ? j : 0];
      }
      // ---- a chain starts: its input rows -> planes, up to 256 main columns; the extra input columns of the rows (x_src == 1) are loaded with
      // them and staged after the main MFMA phase
      f4 vx[RT];
#pragma unroll
      for (int pass = 0; pass < RT; ++pass) vx[pass] = f4{0.f, 0.f, 0.f, 0.f};
      if (S.in != nullptr) {
        chain_stage_rows<T, 512, 4, true>(S.in, S.ld_in, 16 * S.nkb_main, S.x_src == 1 ? 16 * S.nkb_x : 0, ridx, tile0, rows_left, tid, smem, rs, rsf, S.rs_in, vx);
        cnr_lds_barrier();
      }

      f32x16 acc1[1][RT];
      f32x16 (&acc)[RT] = acc1[0];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rt][r] = 0.0f;
      const unsigned char* Ab = smem + pt * CH_ALD + half * 16;
      // k16 blocks as straight-line code, ring four blocks deep, one scheduling fence per block (chain_mfma_blocks); kb0: first block of the phase in W
      auto mfma_phase = [&](int nkb, int kb0) __attribute__((always_inline)) {
        if (nkb == 16) chain_mfma_blocks<RT, 1, 16>(acc1, wr1, wr2, Ab, APLANE, wlane, S.nkb_w, kb0);
        else if (nkb == 3) chain_mfma_blocks<RT, 1, 3>(acc1, wr1, wr2, Ab, APLANE, wlane, S.nkb_w, kb0);
        else if (nkb == 2) chain_mfma_blocks<RT, 1, 2>(acc1, wr1, wr2, Ab, APLANE, wlane, S.nkb_w, kb0);
        else chain_mfma_blocks<RT, 1, 1>(acc1, wr1, wr2, Ab, APLANE, wlane, S.nkb_w, kb0);
      };
      if (!(CNR_ABLATION(c.dbg) & 2)) mfma_phase(S.nkb_main, 0);
      if (S.nkb_x > 0) {
        // ---- the extra input columns, staged over the main ones with the SAME row scale
        chain_wprime<1>(wr1, wr2, wlane, S.nkb_w, S.nkb_main, S.nkb_x);
        cnr_lds_barrier();                                        // every wave is done reading the main segment
#pragma unroll
        for (int pass = 0; pass < RT; ++pass) {
          const int row_l = pass * 32 + (tid >> 4), sc4 = (tid & 15) * 4;
          if (sc4 < 16 * S.nkb_x) {
            f4 v = {0.f, 0.f, 0.f, 0.f};
            if (S.x_src == 1) {
              v = vx[pass];                                   // (same thread, same row, same columns as at the chain start)
            } else if (sc4 == 0) {
              v = *reinterpret_cast<const f4*>(rgbs + row_l * 4);
            }
            split_put4(v, rsf[row_l], smem + row_l * CH_ALD + sc4 * 2, APLANE);
          }
        }
        cnr_lds_barrier();
        if (!(CNR_ABLATION(c.dbg) & 2)) {
          if (S.nkb_x == 3) chain_mfma_blocks<RT, 1, 3>(acc1, wr1, wr2, Ab, APLANE, wlane, S.nkb_w, S.nkb_main);
          else if (S.nkb_x == 2) chain_mfma_blocks<RT, 1, 2>(acc1, wr1, wr2, Ab, APLANE, wlane, S.nkb_w, S.nkb_main);
          else chain_mfma_blocks<RT, 1, 1>(acc1, wr1, wr2, Ab, APLANE, wlane, S.nkb_w, S.nkb_main);
        }
      }
      // the next step's (or the next tile's first step's) leading weight blocks travel while the epilogue runs
      chain_wprime<1>(wr1, wr2, chain_wlane<1>(Sn.Wf, Sn.nkb_w, wave, lane), Sn.nkb_w, 0, Sn.nkb_main);

      // ---- epilogue: a = relu(acc / (row scale * column scale) + bias) ; row max
      const float* cw = cwb + (s & 1) * 512;
      const bool chain_end = S.head != 0;                     // a head follows: the next step (if any) starts from global rows
      {
        const ChainColumns k = chain_columns(cw, cbase);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const int row_l = rt * 32 + pt;
          ChainActRelu act;
          chain_affine16(acc[rt], k, rs[row_l], act);
          if (!chain_end) chain_partial_max(pm, row_l, wave, half, act.mx);
        }
      }
      cnr_lds_barrier();   // partial maxima visible; every wave is done reading the planes of this step's input
      chain_cw_park(cwb + ((last_step ? 0 : s + 1) & 1) * 512, tid, cw_next);
      if (!chain_end) {
        // ---- the next step's input planes (its extra segment, if it comes from the colour head, shares the row scale)
        chain_replane<RT, 1, 8>(acc1, pm, smem, rs, rsf, rgbs, Sn.x_src == 2, Sn.rs_in, tile0, rows_left, ln, wave);
      }
      if (chain_end) {
        // ---- the 3-wide head on the ReLU output still in registers: fp32 dot products, partial sums per (row, wave) in a fixed order.
        // BEFORE the row stores below: a load issued behind them is waited for with vmcnt(0), i.e. with the whole store queue of the wave
        const ChainFwdHead& H = S.head == 1 ? c.col_head : c.rel_head;
#pragma unroll 1
        for (int j = 0; j < 3; ++j) {
          f4 wj[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            wj[q] = f4{0.f, 0.f, 0.f, 0.f};
            if (j < H.n) wj[q] = *reinterpret_cast<const f4*>(H.W + (long)j * H.ldw + cbase + 4 * q);
          }
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) {
            float dot = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) dot = fmaf(acc[rt][r], wj[r >> 2][r & 3], dot);
            dot = cnr_pair32_sum(dot);
            if (half == 0) hp[((rt * 32 + pt) * 8 + wave) * 4 + j] = dot;
          }
        }
      }
      // ---- the ReLU output rows for the backward pass (read again only by the backward pass)
      if (S.save != nullptr && !(CNR_ABLATION(c.dbg) & 1)) {
        float* save_tile = S.save + tile0 * S.ld_save + wave * 32;                   // (uniform)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) chain_save_block<true, true>(acc[rt], tb, save_tile, S.ld_save, rt * 32, rows_left, lane, !(CNR_ABLATION(c.dbg) & 8));
      }
      if (chain_end) {
        const ChainFwdHead& H = S.head == 1 ? c.col_head : c.rel_head;
        cnr_lds_barrier();
        if (tid < T) {
          const int row_l = tid;
          const long grow = tile * T + row_l;
          const long orow = (ridx != nullptr && grow < P) ? (long)ridx[grow] : grow;   // where this row's head outputs go
          float v[3];
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            float sum = hp[(row_l * 8) * 4 + j];
#pragma unroll
            for (int w = 1; w < 8; ++w) sum += hp[(row_l * 8 + w) * 4 + j];
            v[j] = j < H.n ? sum + hbias[j] : 0.0f;
          }
          if (S.head == 1) {
            f4 y = {0.f, 0.f, 0.f, 0.f};
            y.x = c.col_squeeze ? sigmoidf_(v[0]) : v[0];
            if (H.n > 1) y.y = c.col_squeeze ? sigmoidf_(v[1]) : v[1];
            if (H.n > 2) y.z = c.col_squeeze ? sigmoidf_(v[2]) : v[2];
            *reinterpret_cast<f4*>(rgbs + row_l * 4) = y;
            if (grow < P) {
              float* g = c.gcol + orow * 4;
              g[0] = y.x;
              if (H.n > 1) g[1] = y.y;
              if (H.n > 2) g[2] = y.z;
              if (c.rgb_tail != nullptr) {
                const f4 z4 = {0.f, 0.f, 0.f, 0.f};
                f4* t = reinterpret_cast<f4*>(c.rgb_tail + orow * c.ld_tail);
                t[0] = y; t[1] = z4; t[2] = z4; t[3] = z4;
              }
            }
          } else if (grow < P) {
            const f4 rgb = *reinterpret_cast<const f4*>(rgbs + row_l * 4);
            const float rv[3] = {rgb.x, rgb.y, rgb.z};
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              if (j < H.n) {
                c.delta[orow * 3 + j] = v[j];
                c.relit[orow * 4 + j] = relight_apply(rv[j], v[j], c.inv_sigmoid);
              }
            }
          }
        }
      }
      cnr_lds_barrier();
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The SAVING SDF value chain (SdfSaveChain): sdf_value_chain_kernel<RT, 1> of cnr_chain.hip plus the stores the backward pass needs.
// Per hidden layer: z = acc / (row scale x column scale) + bias is stored (through chain_save_block) BEFORE the activation; the layer in front
// of a skip connection stores [z | e] (what the per-layer launches' tail fill writes) and hands [softplus(z) | e] / sqrt(2) to the next layer.
// The top layer's 256 feature rows are one more MFMA step whose output goes straight to the colour network's input buffer.
// Shared with the other two chains (cnr_chain_util.h): lane indices, weight-lane address, column-scale fetch / park, chain_save_block,
// chain_absmax16, chain_dot16, chain_sdf_finish (the sdf's summation order: the same code as the value chain's), LDS layout, launcher.
// Written out HERE, in the form this kernel has always had: the chain start, the epilogue affine, the skip tail, the softplus pass, the
// partial-result stores and the replane.  With the shared blocks there (chain_stage_rows, chain_affine16, CHAIN_SKIP_TAIL, chain_replane ...)
// the kernel has the registers of this form or fewer but 4741 instruction lines against 4673 in <4>, and the launch takes 2.21 ms against
// 2.16 ms at 524 288 points (profiles/chain_refactor_ab.txt); as written it compiles to this form's instructions.
// ------------------------------------------------------------------------------------------------
// The kernel's LDS image, stated once: the kernel carves its regions from these byte offsets, the launcher passes the total
template <int RT>
struct SdfSaveLds {
  static constexpr int T = 32 * RT;
  static constexpr int rs = 2 * T * CH_ALD;                 // (in front: [2][T][CH_ALD] hi | lo planes)  [T] 1 / row scale of the current layer input
  static constexpr int pm = rs + T * 4;                     // [T][8] per-wave partial row maxima
  static constexpr int pd = pm + T * 8 * 4;                 // [T][8] per-wave partial dot products of the sdf row
  static constexpr int cwb = pd + T * 8 * 4;                // [512] column scales | biases of the step in flight (rewritten behind the row-max barrier: every wave has read its values by then)
  static constexpr int wtop = cwb + 512 * 4;                // [256] sdf row of the top layer
  static constexpr int tb = wtop + 256 * 4;                 // [8 waves][16 rows][128 B] transposition buffers
  static constexpr int total = tb + 8 * 2048;
  static_assert((size_t)total <= kChainLdsMax, "LDS budget");
};

template <int RT>
__global__ __launch_bounds__(512, 1) void sdf_save_chain_kernel(const SdfSaveChain c) {
  constexpr int T = 32 * RT;
  constexpr int APLANE = T * CH_ALD;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Lds = SdfSaveLds<RT>;
  float* rs = reinterpret_cast<float*>(smem + Lds::rs);
  float* pm = reinterpret_cast<float*>(smem + Lds::pm);
  float* pd = reinterpret_cast<float*>(smem + Lds::pd);
  float* cwb = reinterpret_cast<float*>(smem + Lds::cwb);
  float* wtop = reinterpret_cast<float*>(smem + Lds::wtop);
  const int tid0 = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  unsigned char* tb = smem + Lds::tb + wave * 2048;
  const SdfValueChain& v = c.v;
  const long ntiles = (v.P + T - 1) / T;
  const int nsteps = v.nl + 1;                               // hidden layers + the feature rows of the top layer
  // (the host puts the top layer's feature rows behind the hidden layers, v.lay[v.nl]: one array index for every step -- a choice between
  // two kernel-argument references would make the compiler copy the argument block to scratch)

  f16x8 wr1[4][1], wr2[4][1];
  chain_wprime<1>(wr1, wr2, chain_wlane<1>(v.lay[0].Wf, v.lay[0].K >> 4, wave, tid0 & 63), v.lay[0].K >> 4, 0, v.lay[0].K >> 4);
  for (int i = tid0; i < 256; i += 512) wtop[i] = v.wtop[i];
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long tile0 = tile * T;
    const int rows_left = (int)((v.P - tile0) < T ? (v.P - tile0) : T);
    {
      // ---- layer-0 input: E rows -> planes (16 threads per row, 4 columns each)
      const int tid = ChainLane<1>(tid0, wave).tid;
      if (tid < 128) chain_cw_park(cwb, tid, chain_cw_fetch(v.lay[0], tid));   // (fetched by the threads that park: no load for the others)
      const int sc4 = (tid & 15) * 4;
      f4 x[RT];
#pragma unroll
      for (int pass = 0; pass < RT; ++pass) {
        const int row_l = pass * 32 + (tid >> 4);
        const int row_c = row_l < rows_left ? row_l : rows_left - 1;
        x[pass] = f4{0.f, 0.f, 0.f, 0.f};
        if (sc4 < kEmb) x[pass] = *reinterpret_cast<const f4*>(v.E + (tile0 + row_c) * kEmb + sc4);
      }
#pragma unroll
      for (int pass = 0; pass < RT; ++pass) {
        const int row_l = pass * 32 + (tid >> 4);
        float mx = ws_absmax4(x[pass]);
        mx = cnr_max16(mx);
        const float sc = split_row_scale(mx);
        if (sc4 < kEmb) split_put4(x[pass], sc, smem + row_l * CH_ALD + sc4 * 2, APLANE);
        if ((tid & 15) == 0) rs[row_l] = cnr_pow2_rcp(sc);
      }
      cnr_lds_barrier();
    }
    for (int l = 0; l < nsteps; ++l) {
      const ChainLane<1> ln(tid0, wave);
      const int tid = ln.tid, lane = ln.lane, half = ln.half, pt = ln.pt, cbase = ln.cbase;
      const bool is_top = l == v.nl, last_hidden = l + 1 == v.nl;
      const FusedLayer& L = v.lay[l];
      const FusedLayer& Ln = v.lay[is_top ? 0 : l + 1];
      const int nkb = L.K >> 4;
      const f4 cw_next = chain_cw_fetch(Ln, tid);
      f32x16 acc1[1][RT];
      f32x16 (&acc)[RT] = acc1[0];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rt][r] = 0.0f;
      const unsigned char* Ab = smem + pt * CH_ALD + half * 16;
      if (nkb == 16) chain_mfma_blocks<RT, 1, 16>(acc1, wr1, wr2, Ab, APLANE, chain_wlane<1>(L.Wf, nkb, wave, lane), 16, 0);
      else chain_mfma_blocks<RT, 1, 3>(acc1, wr1, wr2, Ab, APLANE, chain_wlane<1>(L.Wf, nkb, wave, lane), 3, 0);
      chain_wprime<1>(wr1, wr2, chain_wlane<1>(Ln.Wf, Ln.K >> 4, wave, lane), Ln.K >> 4, 0, Ln.K >> 4);

      const float* cw = cwb;
      const bool next_skip = !is_top && !last_hidden && ((v.skip_mask >> (l + 1)) & 1);
      const bool ragged = !is_top && L.N < 256;             // wave-uniform: only the layer in front of a skip connection
      float* out_tile = (is_top ? c.feat + tile0 * c.ld_feat : c.Z[l] + tile0 * c.ldz) + wave * 32;
      const int out_ld = is_top ? c.ld_feat : c.ldz;
      float rmax[RT], rdot[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) { rmax[rt] = 0.0f; rdot[rt] = 0.0f; }
      {
        f4 wsc4[4], b4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          wsc4[q] = *reinterpret_cast<const f4*>(cw + cbase + 4 * q);
          b4[q] = *reinterpret_cast<const f4*>(cw + 256 + cbase + 4 * q);
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const int row_l = rt * 32 + pt;
          const f2 rsc = pk_splat(rs[row_l]);
          // z (or, for the top layer, the feature row): acc / (row scale * column scale) + bias
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const f2 w = {wsc4[q >> 1][(2 * q) & 3], wsc4[q >> 1][(2 * q + 1) & 3]};
            const f2 b = {b4[q >> 1][(2 * q) & 3], b4[q >> 1][(2 * q + 1) & 3]};
            f2 a = {acc[rt][2 * q], acc[rt][2 * q + 1]};
            a = pk_fma(a, rsc * w, b);
            acc[rt][2 * q] = a.x; acc[rt][2 * q + 1] = a.y;
          }
          const bool tail_lane = ragged && cbase + 16 > L.N;  // owns columns >= N: they carry e (fields.py:86-87)
          if (tail_lane) {
            const int row_c = row_l < rows_left ? row_l : rows_left - 1;
            const float* erow = v.E + (tile0 + row_c) * kEmb;
            float ev[16];   // (all 16 loads first: consumed one by one the compiler waits for each before it issues the next)
#pragma unroll
            for (int r = 0; r < 16; ++r) { const int ei = cbase + r - L.N; ev[r] = erow[ei < 0 ? 0 : (ei < kEmb ? ei : kEmb - 1)]; }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int ei = cbase + r - L.N;
              acc[rt][r] = ei < 0 ? acc[rt][r] : ((next_skip && ei < v.emb) ? ev[r] : 0.0f);
            }
          }
          if (is_top) chain_save_block<false>(acc[rt], tb, out_tile, out_ld, rt * 32, rows_left, lane);   // (the feature rows: the colour network reads them next)
          else chain_save_block<true>(acc[rt], tb, out_tile, out_ld, rt * 32, rows_left, lane);           // (pre-activations: read again only by the gradient chain / backward pass)
          if (!is_top) {
            // a = softplus(z) (the tail columns keep e), / sqrt(2) in front of a skip layer ; row max ; partial dot with the sdf row
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              f2 z = {acc[rt][2 * q], acc[rt][2 * q + 1]};
              f2 a = softplus100_pk(z);
              if (tail_lane) { a.x = cbase + 2 * q >= L.N ? z.x : a.x; a.y = cbase + 2 * q + 1 >= L.N ? z.y : a.y; }
              if (next_skip) a = a * pk_splat(kInvSqrt2);
              acc[rt][2 * q] = a.x; acc[rt][2 * q + 1] = a.y;
            }
            rmax[rt] = chain_absmax16(acc[rt]);
            if (last_hidden) rdot[rt] = chain_dot16(acc[rt], wtop + cbase);
          }
        }
      }
      if (!is_top) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const float o = cnr_pair32_max(rmax[rt]);
          if (half == 0) pm[(rt * 32 + pt) * 8 + wave] = o;
          if (last_hidden) { const float od = cnr_pair32_sum(rdot[rt]); if (half == 0) pd[(rt * 32 + pt) * 8 + wave] = od; }
        }
      }
      cnr_lds_barrier();   // partial maxima / dots visible; every wave is done reading the planes of this step's input
      chain_cw_park(cwb, tid, cw_next);
      if (!is_top) {
        float* rso = c.rs[l + 1];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const int row_l = rt * 32 + pt;
          float mx = pm[row_l * 8];
#pragma unroll
          for (int w = 1; w < 8; ++w) mx = fmaxf(mx, pm[row_l * 8 + w]);
          const float sc = split_row_scale(mx);
          split_put16(acc[rt], sc, smem + row_l * CH_ALD + cbase * 2, APLANE);
          if (wave == 0 && half == 0) {
            rs[row_l] = cnr_pow2_rcp(sc);
            if (rso != nullptr && row_l < rows_left) rso[tile0 + row_l] = split_rs_value(mx, sc);
          }
        }
        if (last_hidden) chain_sdf_finish<T>(pd, tid, tile0, rows_left, v.btop, v.top_scale, v.sdf_out);
      }
      cnr_lds_barrier();
    }
  }
}

template <int RT>
static void launch_sdf_save_chain(const SdfSaveChain& c, cnr_stream s) {
  double macs = 256.0 * 256.0, bytes = (double)c.v.P * ((kEmb + 1) * 4.0 + 1024.0);
  for (int l = 0; l < c.v.nl; ++l) { macs += (double)c.v.lay[l].K * 256.0; bytes += (double)c.v.P * (1024.0 + (c.rs[l + 1] ? 4.0 : 0.0)); }
  SdfSaveChain cc = c;
  cc.v.lay[c.v.nl] = c.top;
  chain_launch<&sdf_save_chain_kernel<RT>>(cc, 32 * RT, 512, SdfSaveLds<RT>::total, 256, c.v.P, "chain_sdf_fwd", RT * 10 + 1, macs, bytes, s);
}

bool be_sdf_save_chain(const SdfSaveChain& c, cnr_stream s) {
  const bool off = debug_flags().no_fused || debug_flags().no_chain_sdf;   // debugging aids: per-layer launches
  const SdfValueChain& v = c.v;
  if (off || v.P <= 0 || v.nl < 1 || v.nl >= kMaxLayers) return false;
  for (int l = 0; l < v.nl; ++l) {
    if ((v.lay[l].K != 256 && !(l == 0 && v.lay[l].K == 48)) || v.lay[l].N > 256 || v.lay[l].N < 1 || !v.lay[l].Wf || !c.Z[l]) return false;
    if (l + 1 < v.nl && v.lay[l].N < 256 && !((v.skip_mask >> (l + 1)) & 1)) return false;   // a narrow layer only in front of a skip connection
  }
  if (v.lay[v.nl - 1].N != 256 || c.top.K != 256 || c.top.N != 256 || !c.top.Wf || !c.feat || (c.ld_feat & 3) || (c.ldz & 3) || c.ldz < 256) return false;
  const int rt = chain_rt_for(v.P, debug_flags().chain_fwd_rt);
  if (rt == 4) launch_sdf_save_chain<4>(c, s);
  else if (rt == 2) launch_sdf_save_chain<2>(c, s);
  else launch_sdf_save_chain<1>(c, s);
  CNR_LAUNCH_CHECK("chain_sdf_fwd");
  return true;
}

template <int RT>
static void launch_relu_chain_fwd(const ReluChainFwd& c, cnr_stream s) {
  double macs = 0.0, bytes = 0.0;
  for (int i = 0; i < c.nsteps; ++i) {
    const ChainFwdStep& S = c.st[i];
    macs += 16.0 * (S.nkb_main + S.nkb_x) * 256.0;
    if (S.in) bytes += (double)c.P * 4.0 * 16.0 * (S.nkb_main + (S.x_src == 1 ? S.nkb_x : 0));
    if (S.save) bytes += (double)c.P * 1024.0;
    if (S.rs_in) bytes += (double)c.P * 4.0;
    if (S.head) bytes += (double)c.P * (S.head == 1 ? (c.rgb_tail ? 80.0 : 16.0) : 28.0);
  }
  ReluChainFwd cc = c;
  cc.dbg = debug_flags().chain_fwd_dbg;
  chain_launch<&relu_chain_fwd_kernel<RT>>(cc, 32 * RT, 512, ReluChainLds<RT>::total, 256, c.P, "chain_fwd", RT * 10 + 1, macs, bytes, s);   // (one workgroup per CU)
}

bool be_relu_chain_fwd_enabled() {
  const bool off = debug_flags().no_fused || debug_flags().no_chain_fwd;   // debugging aids: per-layer launches
  return !off;
}

bool be_relu_chain_fwd(const ReluChainFwd& c, cnr_stream s) {
  const bool off = !be_relu_chain_fwd_enabled();
  if ((c.row_idx != nullptr) != (c.P_dev != nullptr)) return false;
  if (off || c.P <= 0 || c.nsteps < 1 || c.nsteps > kChainSteps) return false;
  for (int i = 0; i < c.nsteps; ++i) {
    const ChainFwdStep& S = c.st[i];
    const bool main_ok = S.in != nullptr ? (S.nkb_main == 16 || (S.nkb_main >= 1 && S.nkb_main <= 3)) : S.nkb_main == 16;
    if (!S.Wf || !S.wsc || !S.bias || !main_ok || S.nkb_x < 0 || S.nkb_x > 3 || S.nkb_main + S.nkb_x > S.nkb_w) return false;
    if (S.nkb_x > 0 && S.x_src != 1 && S.x_src != 2) return false;
    if (S.x_src == 1 && (S.in == nullptr || (S.ld_in & 3) != 0 || S.ld_in < 16 * (S.nkb_main + S.nkb_x))) return false;
    if (S.in != nullptr && ((S.ld_in & 3) != 0 || S.ld_in < 16 * S.nkb_main)) return false;
    if (S.x_src == 2 && S.nkb_x != 1) return false;
    if (S.save != nullptr && (S.ld_save & 3) != 0) return false;
    if (c.row_idx != nullptr && (S.save != nullptr || S.rs_in != nullptr)) return false;   // a compacted run keeps nothing for a backward pass
    if (i == 0 && S.in == nullptr) return false;
    if (i > 0 && c.st[i - 1].head != 0 && S.in == nullptr) return false;   // a chain starts from global rows
    if (S.head == 1 && (!c.col_head.W || c.col_head.n < 1 || c.col_head.n > 3 || (c.col_head.ldw & 3) || !c.gcol || (c.rgb_tail && (c.ld_tail & 3)))) return false;
    if (S.head == 2 && (!c.rel_head.W || c.rel_head.n < 1 || c.rel_head.n > 3 || (c.rel_head.ldw & 3) || !c.delta || !c.relit)) return false;
  }
  if (c.st[c.nsteps - 1].head == 0) return false;
  const int rt = chain_rt_for(c.P, debug_flags().chain_fwd_rt);   // (tuning aid: 4, 2, 1)
  if (rt == 4) launch_relu_chain_fwd<4>(c, s);
  else if (rt == 2) launch_relu_chain_fwd<2>(c, s);
  else launch_relu_chain_fwd<1>(c, s);
  CNR_LAUNCH_CHECK("chain_fwd");
  return true;
}

}  // namespace cnr
