// Weight-gradient GEMMs for gfx950: FP32-MFMA tail tiles, split-bf16 and split-f16 256 x 256 tiles, skinny strips, scale reduction.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "cnr_backend.h"
#include "cnr_hip_util.h"
#include "cnr_gemm_int.h"
#include "cnr_split.h"
#include "cnr_wave.h"

namespace cnr {

// ================================================================================================
// weight-gradient GEMM:  dW[n][k] = sum_pt X[pt][n] * Y[pt][k]
// 8 waves as WR x WC, each wave (MT*32) x (KT*32); block tile TN x TK; points streamed 16 at a time.
// ================================================================================================
// points per slab: 16 for the square tile; the skinny tail tiles are latency-bound streams, so they take as many as LDS holds
constexpr int dw_bp(int tn, int tk) { return tn + tk <= 288 ? 64 : (tn + tk <= 320 ? 48 : 16); }

// a wave's [MT x KT] accumulator blocks of 32 x 32 (lane map of the 32 x 32 MFMAs) into the workgroup's partial-sum slot [Npad][ldk], rows from n0,
// columns from k0 (both with the wave's offset), times the exact factors u1 * u2 where the sums carry a block exponent (UNDO)
template <bool UNDO, int MT, int KT>
__device__ __forceinline__ void dw_store_partial(float* out, const DwGemm& g, const f32x16 (&acc)[MT][KT], int n0, int k0, int lane, float u1 = 1.0f, float u2 = 1.0f) {
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < KT; ++j) {
      const int kk = k0 + j * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (n < g.Npad && kk < g.ldk) out[(long)n * g.ldk + kk] = UNDO ? acc[i][j][r] * u1 * u2 : acc[i][j][r];
      }
    }
}

// The view kinds of a launch pinned at compile time, so that the interpreted prologue folds away.  ONE description generates both sides: the kernel
// applies it to its copy of the launch (apply), the host asks it which launches may take the instantiation (matches).  X0 < 0: nothing is pinned
// (interpreted at run time); X1 < 0: exactly one pair; ONES: the operands whose scale is pinned to 1 (bit 0 / 1: X / Y of pair 0, bit 2 / 3: of pair 1).
template <int X0, int Y0, int X1 = -1, int Y1 = -1, unsigned ONES = 0>
struct DwPin {
  static constexpr bool pinned = X0 >= 0;
  static constexpr bool one_pair = pinned && X1 < 0;   // the pair index folds to 0
  static __host__ __device__ __forceinline__ void apply(DwGemm& g) {
    constexpr int kind[4] = {X0, Y0, X1, Y1};
    View* const v[4] = {&g.X[0], &g.Y[0], &g.X[1], &g.Y[1]};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (kind[i] >= 0) { v[i]->kind = kind[i]; if (ONES >> i & 1) v[i]->scale = 1.0f; }
  }
  static bool matches(const DwGemm& g) {
    if (!pinned) return true;
    if (g.npairs != (one_pair ? 1 : 2)) return false;
    constexpr int kind[4] = {X0, Y0, X1, Y1};
    const View* const v[4] = {&g.X[0], &g.Y[0], &g.X[1], &g.Y[1]};
    for (int i = 0; i < 2 * g.npairs; ++i)
      if (v[i]->kind != kind[i] || ((ONES >> i & 1) && v[i]->scale != 1.0f)) return false;
    return true;
  }
};
typedef DwPin<-1, -1> DwInterpreted;
constexpr unsigned DW_ONES_ALL = 0xf;
// the instantiations of a kernel: the first pin of the list that matches the launch takes it (every list ends with DwInterpreted)
template <class... PINS>
struct DwPinList {
  template <class LAUNCH>
  static void first_match(const DwGemm& g, LAUNCH&& launch) {
    bool done = false;
    ((done = done || (PINS::matches(g) ? (launch(PINS{}), true) : false)), ...);
  }
};

// 16-point slabs are dealt round-robin to the workgroups (the i-th slab of workgroup `chunk` is slab i * nchunk + chunk): at any moment the CUs read one
// contiguous stretch of X and Y, which spreads over all HBM channels.  Every kernel that sums over points in this order takes it from here: the
// partial sums must stay in a fixed order.
struct DwSlabs {
  long total;          // slabs of the point range
  long n;              // slabs of this workgroup
  long chunk; int nchunk;
  __device__ __forceinline__ DwSlabs(long P, long chunk_, int nchunk_)
      : total((P + 15) / 16), n(chunk_ < total ? (total - chunk_ + nchunk_ - 1) / nchunk_ : 0), chunk(chunk_), nchunk(nchunk_) {}
  __device__ __forceinline__ long first_point(long i) const { return (i * nchunk + chunk) * 16; }   // of this workgroup's i-th slab
};

// one operand's part of a slab in flight (dw_gemm_kernel): NR 16-byte column groups per thread, raw as fetched
template <int NR>
struct DwStaged { f4 a[NR], b[NR]; bool ok[NR]; };
// fetch: BP points from pbase x TW columns from col0 (points at and beyond p_end read the last point and are zeroed in dw_finish)
template <int TW, int BP, int NR>
__device__ __forceinline__ void dw_fetch(DwStaged<NR>& r, const View& v, long pbase, long p_end, int col0, int tid) {
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int idx = tid + i * 512;
    if ((BP * TW / 4) % 512 == 0 || idx < BP * TW / 4) {
      const int pl = idx / (TW / 4), c4 = idx % (TW / 4);
      long pt = pbase + pl;
      r.ok[i] = pt < p_end;
      if (!r.ok[i]) pt = p_end - 1;
      const Raw4 q = view_fetch4(v, pt, col0 + c4 * 4);
      r.a[i] = q.a; r.b[i] = q.b;
    }
  }
}
// finish: the view's math, into the operand's LDS slab [BP][TW]
template <int TW, int BP, int NR>
__device__ __forceinline__ void dw_finish(const DwStaged<NR>& r, const View& v, float* dst, int col0, int tid) {
  const f4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int idx = tid + i * 512;
    if ((BP * TW / 4) % 512 == 0 || idx < BP * TW / 4) {
      Raw4 q; q.a = r.a[i]; q.b = r.b[i];
      const f4 val = view_finish4(v, q, col0 + (idx % (TW / 4)) * 4);
      *reinterpret_cast<f4*>(dst + idx * 4) = r.ok[i] ? val : z4;
    }
  }
}

template <int WR, int WC, int MT, int KT, class PIN = DwInterpreted>
__global__ __launch_bounds__(512) void dw_gemm_kernel(const DwGemm g_in, int n0, int k0) {
  DwGemm g = g_in;
  PIN::apply(g);
  constexpr int TN = WR * MT * 32, TK = WC * KT * 32;
  constexpr int DW_BP = dw_bp(TN, TK);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Xs = smem;                       // [2][16][TN]
  float* Ys = smem + 2 * DW_BP * TN;      // [2][16][TK]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave / WC, wc = wave % WC;
  const long chunk = blockIdx.x;
  const long p_begin = chunk * g.chunk_pts;
  long p_end = p_begin + g.chunk_pts;
  if (p_end > g.P) p_end = g.P;
  const int nslab_pair = p_end > p_begin ? (int)((p_end - p_begin + DW_BP - 1) / DW_BP) : 0;
  const int nslab = nslab_pair * g.npairs;
  constexpr int NX = (DW_BP * TN / 4 + 511) / 512, NY = (DW_BP * TK / 4 + 511) / 512;

  f32x16 acc[MT][KT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < KT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  DwStaged<NX> rx;
  DwStaged<NY> ry;
  int staged_pair = 0;
  float csum = 0.0f;
  const bool want_colsum = g.colsum != nullptr && k0 == 0;

  auto load_slab = [&](int s) {
    const int pair = PIN::one_pair ? 0 : s / nslab_pair;
    staged_pair = pair;
    const long pbase = p_begin + (long)(s - pair * nslab_pair) * DW_BP;
    if (pair == 0) { dw_fetch<TN, DW_BP>(rx, g.X[0], pbase, p_end, n0, tid); dw_fetch<TK, DW_BP>(ry, g.Y[0], pbase, p_end, k0, tid); }
    else { dw_fetch<TN, DW_BP>(rx, g.X[1], pbase, p_end, n0, tid); dw_fetch<TK, DW_BP>(ry, g.Y[1], pbase, p_end, k0, tid); }
  };
  auto store_slab = [&](int buf) {   // (a branch per pair, not a selected view: each side keeps its pinned kinds)
    float* const xd = Xs + buf * DW_BP * TN;
    float* const yd = Ys + buf * DW_BP * TK;
    if (staged_pair == 0) { dw_finish<TN, DW_BP>(rx, g.X[0], xd, n0, tid); dw_finish<TK, DW_BP>(ry, g.Y[0], yd, k0, tid); }
    else { dw_finish<TN, DW_BP>(rx, g.X[1], xd, n0, tid); dw_finish<TK, DW_BP>(ry, g.Y[1], yd, k0, tid); }
  };

  if (nslab > 0) {
    load_slab(0);
    store_slab(0);
  }
  __syncthreads();
  for (int s = 0; s < nslab; ++s) {
    const int buf = s & 1;
    if (s + 1 < nslab) load_slab(s + 1);
    const float* Xb = Xs + buf * DW_BP * TN + (lane >> 5) * TN + wr * MT * 32 + (lane & 31);
    const float* Yb = Ys + buf * DW_BP * TK + (lane >> 5) * TK + wc * KT * 32 + (lane & 31);
#pragma unroll
    for (int st = 0; st < DW_BP / 2; ++st) {
      float a[MT], b[KT];
#pragma unroll
      for (int i = 0; i < MT; ++i) a[i] = Xb[st * 2 * TN + i * 32];
#pragma unroll
      for (int j = 0; j < KT; ++j) b[j] = Yb[st * 2 * TK + j * 32];
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < KT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (want_colsum && s < nslab_pair && tid < TN) {   // bias gradient: column sums of the first X operand
      const float* xc = Xs + buf * DW_BP * TN + tid;
#pragma unroll
      for (int pl = 0; pl < DW_BP; ++pl) csum += xc[pl * TN];
    }
    if (s + 1 < nslab) store_slab(buf ^ 1);
    __syncthreads();
  }

  dw_store_partial<false>(g.partial + chunk * (long)g.Npad * g.ldk, g, acc, n0 + wr * MT * 32, k0 + wc * KT * 32, lane);
  if (want_colsum && tid < TN && n0 + tid < g.Npad) g.colsum[chunk * g.Npad + n0 + tid] = csum;
}

template <int WR, int WC, int MT, int KT, class PIN = DwInterpreted>
static void launch_dw(const DwGemm& g, int n0, int k0, cnr_stream s) {
  constexpr int TN = WR * MT * 32, TK = WC * KT * 32;
  constexpr int DW_BP = dw_bp(TN, TK);
  const size_t lds = (size_t)(2 * DW_BP * (TN + TK)) * sizeof(float);
  const int tn_ = (g.N - n0) < TN ? (g.N - n0) : TN, tk_ = (g.K - k0) < TK ? (g.K - k0) : TK;
  TimingScope ts_("dw_gemm", 1, WR * 1000 + WC * 100 + MT * 10 + KT, g.P, tn_, tk_, g.npairs, s, dw_gemm_bytes(g, tn_, tk_));
  launch_lds<dw_gemm_kernel<WR, WC, MT, KT, PIN>>(dim3(g.nchunk), dim3(512), lds, lds, s, g, n0, k0);
}

// ================================================================================================
// weight-gradient GEMM, 256 x 256 output tile on the matrix cores, fp32 operands split into 16-bit planes: ONE kernel over a format
//
// Same output-stationary structure as dw_gemm_kernel<4,2,2,4> (128 accumulator registers per wave, one workgroup per point
// slice).  A format states what differs: the number of planes, the fragment type, how a staged block is split and stored, the
// MFMA sequence of one column tile, whether the operands carry per-point scales (SCALED), its barrier and its pinned launches.
//
// DwBf16 (split-bf16): x = x1 + x2 + x3 (8 + 8 + 8 significand bits, the fp32 exponent range is kept, so no scaling is needed
// along the contraction over points); a product is six v_mfma_f32_32x32x16_bf16 (x1y1 + x1y2 + x2y1 + x2y2 + x1y3 + x3y1, small
// terms first; the dropped terms are < 2^-25 relative).  6 x 32 cycles per 32x32x16 block against 8 x 64 for
// v_mfma_f32_32x32x2_f32: 2.7x the matrix rate at fp32 accuracy.
//
// DwF16 (split-f16, three MFMAs per product instead of six): along the contraction a scale can only be used if it cancels per
// point: X'[pt] = X[pt] * sx[pt] (the power of two that lifts the row into the top f16 binade -- emitted for free by the layer
// GEMM that consumed the same operand, LayerGemm::rs_out) and Y'[pt] = Y[pt] * 2^G / sx[pt], so X'^T Y' = 2^G X^T Y exactly.
// G = 1 + min over the workgroup's points of log2(sx * sy) keeps every Y' row below 2^15; points whose product is far below the
// largest one lose relative precision in Y' but their absolute error stays below 2^-40 of the largest term.  Both operands are
// split hi + lo (11 + 11 bits) and x1 y2 + x2 y1 + x1 y1 is accumulated in fp32; the result is scaled back by 2^-G (exact).
//
// LDS: per operand and plane the 16-point slab is stored as [half h][j = n % 4][c = n / 4][8 points] of 16 bits with 1088-byte
// j-regions: the staging threads (4 columns x 4 points each) write 8-byte point quads, adjacent lanes adjacent quads
// (conflict-free), and an MFMA lane reads the 16 bytes of its row n / point half h (conflict-free: 16 lanes cover 16
// distinct 16-byte bank groups).
// ================================================================================================
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
constexpr int DX_JREG = 1088;                 // bytes per j-region (64 columns x 16 bytes + 64 bytes of bank rotation)
constexpr int DX_HALF = 4 * DX_JREG;          // one point half (8 points) of one plane
constexpr int DX_PLANE = 2 * DX_HALF;         // one 16-bit plane of a 16-point x 256-column slab

__device__ __forceinline__ void dx_split3(float x, __bf16& h1, __bf16& h2, __bf16& h3) {
  h1 = (__bf16)x;
  float r = x - (float)h1;
  h2 = (__bf16)r;
  r = r - (float)h2;
  h3 = (__bf16)r;
}

// In both formats the two row tiles of a wave alternate (c0, c1) so that back-to-back MFMAs never depend on each other; that hand
// interleaving is why DwF16 does not call split_mfma3_32 twice, which would state another order.
struct DwBf16 {
  static constexpr const char* name = "dw_gemm_bx";
  static constexpr int PLANES = 3;
  static constexpr bool SCALED = false;
  typedef bf16x8 frag;
  static __device__ __forceinline__ void barrier() { __syncthreads(); }
  // one column of a staged block (4 points) -> an 8-byte point quad per plane
  static __device__ __forceinline__ void store4(const f4& c, unsigned char* d) {
    bf16x4 h1, h2, h3;
#pragma unroll
    for (int i = 0; i < 4; ++i) { __bf16 a_, b_, c_; dx_split3(c[i], a_, b_, c_); h1[i] = a_; h2[i] = b_; h3[i] = c_; }
    *reinterpret_cast<bf16x4*>(d) = h1;
    *reinterpret_cast<bf16x4*>(d + DX_PLANE) = h2;
    *reinterpret_cast<bf16x4*>(d + 2 * DX_PLANE) = h3;
  }
  static __device__ __forceinline__ void mfma(f32x16& c0, f32x16& c1, const frag (&a)[2][3], const frag (&b)[3]) {
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][2], b[0], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][2], b[0], c1, 0, 0, 0);
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][0], b[2], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][0], b[2], c1, 0, 0, 0);
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][1], b[1], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][1], b[1], c1, 0, 0, 0);
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][1], b[0], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][1], b[0], c1, 0, 0, 0);
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][0], b[1], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][0], b[1], c1, 0, 0, 0);
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][0], b[0], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][0], b[0], c1, 0, 0, 0);
  }
  // the operand combinations of the render plan (cnr_render_bwd.cpp, cnr_background.cpp): MLP layers, SDF value + gradient-chain pairs
  typedef DwPinList<DwPin<VK_DIRECT, VK_DIRECT>, DwPin<VK_DIRECT, VK_SOFTPLUS>, DwPin<VK_DIRECT, VK_SOFTPLUS, VK_SIGMUL, VK_DIRECT>,
                    DwPin<VK_DIRECT, VK_SOFTPLUS, VK_SIGMUL_ROW, VK_DIRECT>, DwPin<VK_DIRECT, VK_SOFTPLUS, VK_CONST_COL0, VK_DIRECT>, DwInterpreted> Pins;
};
struct DwF16 {
  static constexpr const char* name = "dw_gemm_hx";
  static constexpr int PLANES = 2;
  static constexpr bool SCALED = true;
  typedef f16x8 frag;
  static __device__ __forceinline__ void barrier() { cnr_lds_barrier(); }
  static __device__ __forceinline__ void store4(const f4& c, unsigned char* d) { split_store4(c, d, DX_PLANE); }
  static __device__ __forceinline__ void mfma(f32x16& c0, f32x16& c1, const frag (&a)[2][2], const frag (&b)[2]) {
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0][0], b[1], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1][0], b[1], c1, 0, 0, 0);
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0][1], b[0], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1][1], b[0], c1, 0, 0, 0);
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0][0], b[0], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1][0], b[0], c1, 0, 0, 0);
  }
  typedef DwPinList<DwPin<VK_DIRECT, VK_DIRECT>, DwPin<VK_DIRECT, VK_SOFTPLUS>, DwPin<VK_DIRECT, VK_SOFTPLUS, VK_SIGMUL, VK_DIRECT>,
                    DwPin<VK_DIRECT, VK_SOFTPLUS, VK_SIGMUL_ROW, VK_DIRECT>, DwInterpreted> Pins;
};
template <class F> constexpr int dw_split_oper = F::PLANES * DX_PLANE;     // one operand's planes of a slab
template <class F> constexpr int dw_split_buf = 2 * dw_split_oper<F>;      // X and Y; the kernel double-buffers

template <class F, class PIN>
__global__ __launch_bounds__(512, 1) void dw_gemm_split_kernel(const DwGemm g_in, int n0, int k0) {
  DwGemm g = g_in;
  PIN::apply(g);
  constexpr int OPER = dw_split_oper<F>, BUF = dw_split_buf<F>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_d[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;               // 4 x 2 waves, 64 x 128 outputs each
  const long chunk = blockIdx.x;
  const long p_end = g.P;
  const DwSlabs slabs(g.P, chunk, g.nchunk);
  const int nslab_pair = (int)slabs.n;
  const int nslab = nslab_pair * g.npairs;
  // SCALED: exponent of this workgroup's slice of the point range: G = 1 + min log2(sx * sy) over its own points (both pairs, all-zero rows
  // excluded): no separate reduction launch, and a slice of small-magnitude points keeps its own dynamic range
  int G = 0;
  if constexpr (F::SCALED) {
    G = SPLIT_GBIG;
    const int npts = nslab_pair * 16;
    auto scan = [&](const float* sxp, const float* syp) {   // (no run-time index into g: the struct must stay in registers)
      for (int i = tid; i < npts; i += 512) {
        const long pt = slabs.first_point(i >> 4) + (i & 15);
        if (pt < p_end) {
          const float a = sxp[pt], b = syp[pt];   // powers of two (or 0 / NaN)
          const int e = split_exp2_of_product(a, b) + 1;
          if (a > 0.0f && b > 0.0f && e < G) G = e;
        }
      }
    };
    scan(g.sx[0], g.sy[0]);
    if (g.npairs > 1) scan(g.sx[1], g.sy[1]);
    G = wave_min_int(G);
    int* red = reinterpret_cast<int*>(smem_d);
    if (lane == 0) red[wave] = G;
    F::barrier();
#pragma unroll
    for (int w = 0; w < 8; ++w) { const int o = red[w]; G = o < G ? o : G; }
    F::barrier();
    G = __builtin_amdgcn_readfirstlane(G);                // (uniform: keep it in a scalar register)
    if (G >= SPLIT_GBIG) G = 0;                           // no point with two non-zero rows: everything is zero anyway
  }

  f32x16 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  // staging role: threads 0..255 stage X, 256..511 stage Y; each 4 columns x 4 points
  const bool is_y = tid >= 256;
  const int st = tid & 255;
  const int qlo = st & 1, c4 = (st >> 1) & 63, qhi = st >> 7;
  const int q = qhi * 2 + qlo;                          // point quad of the slab
  const int scol = (is_y ? k0 : n0) + c4 * 4;
  unsigned char* const sdst = smem_d + (is_y ? OPER : 0) + qhi * DX_HALF + c4 * 16 + qlo * 8;
  f4 ra[4], rb[4];
  [[maybe_unused]] float rsx[4];                          // SCALED: sx of the 4 points this thread stages
  bool okp[4];
  int staged_pair = 0;
  f4 csum = {0.f, 0.f, 0.f, 0.f};
  const bool want_colsum = g.colsum != nullptr && k0 == 0;

#define DT_FETCH_(V_)                                                                      \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                          \
    long pt = pbase_ + i;                                                                  \
    okp[i] = pt < p_end;                                                                   \
    if (!okp[i]) pt = p_end - 1;                                                           \
    const Raw4 q_ = view_fetch4(V_, pt, scol);                                             \
    ra[i] = q_.a; rb[i] = q_.b;                                                            \
    if constexpr (F::SCALED) rsx[i] = sxp_[pt];                                            \
  }
#define DT_LOAD_SLAB(s_)                                                                   \
  {                                                                                        \
    const int pair_ = PIN::one_pair ? 0 : (s_) / nslab_pair;                               \
    staged_pair = pair_;                                                                   \
    const long pbase_ = slabs.first_point((s_) - pair_ * nslab_pair) + q * 4;              \
    [[maybe_unused]] const float* sxp_ = pair_ == 0 ? g.sx[0] : g.sx[1];                   \
    if (pair_ == 0) { if (is_y) { DT_FETCH_(g.Y[0]) } else { DT_FETCH_(g.X[0]) } }         \
    else { if (is_y) { DT_FETCH_(g.Y[1]) } else { DT_FETCH_(g.X[1]) } }                    \
  }
#define DT_FINISH_(V_)                                                                     \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                          \
    Raw4 q_; q_.a = ra[i]; q_.b = rb[i];                                                   \
    v_[i] = okp[i] ? view_finish4(V_, q_, scol) : z4_;                                     \
  }
#define DT_STORE_SLAB(buf_)                                                                \
  {                                                                                        \
    const f4 z4_ = {0.f, 0.f, 0.f, 0.f};                                                   \
    f4 v_[4];                                                                              \
    if (staged_pair == 0) { if (is_y) { DT_FINISH_(g.Y[0]) } else { DT_FINISH_(g.X[0]) } } \
    else { if (is_y) { DT_FINISH_(g.Y[1]) } else { DT_FINISH_(g.X[1]) } }                  \
    if (want_colsum && !is_y && staged_pair == 0) {                                        \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) { csum.x += v_[i].x; csum.y += v_[i].y; csum.z += v_[i].z; csum.w += v_[i].w; } \
    }                                                                                      \
    if constexpr (F::SCALED) {                                                             \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                      \
        float f_ = rsx[i];                                                                 \
        if (is_y) f_ = split_yscale(f_, G);                                                \
        v_[i].x *= f_; v_[i].y *= f_; v_[i].z *= f_; v_[i].w *= f_;                        \
      }                                                                                    \
    }                                                                                      \
    unsigned char* d_ = sdst + (buf_) * BUF;                                               \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {   /* column j of the 4 points */       \
      const f4 c_ = {v_[0][j], v_[1][j], v_[2][j], v_[3][j]};                              \
      F::store4(c_, d_ + j * DX_JREG);                                                     \
    }                                                                                      \
  }

  // The X-staging waves (0..3) and the Y-staging waves (4..7) share the SIMDs pairwise and run half an iteration out of
  // phase: while one wave of a SIMD issues its MFMAs, the other converts and stores its part of the next slab, so the
  // matrix pipe and the VALU / LDS-store path overlap.  X waves: load(s+1) | MFMA(s) | store(s+1);  Y waves: store(s+1),
  // load(s+2) | MFMA(s).  One barrier per slab.
  if (nslab > 0) {
    DT_LOAD_SLAB(0)
    DT_STORE_SLAB(0)
    if (is_y && nslab > 1) DT_LOAD_SLAB(1)
  }
  F::barrier();
  // operand fragment addresses of this lane: row / column (lane & 31) of each 32-wide tile, point half (lane >> 5)
  const int ln = lane & 31, lh = lane >> 5;
  const int xoff = lh * DX_HALF + (ln & 3) * DX_JREG + (wr * 16 + (ln >> 2)) * 16;              // + i * 8 * 16 per n-tile
  const int yoff = OPER + lh * DX_HALF + (ln & 3) * DX_JREG + (wc * 32 + (ln >> 2)) * 16;       // + j * 8 * 16 per k-tile
  for (int s = 0; s < nslab; ++s) {
    const int buf = s & 1;
    if (!is_y) {
      if (s + 1 < nslab) DT_LOAD_SLAB(s + 1)
    } else if (s + 1 < nslab) {
      DT_STORE_SLAB(buf ^ 1)
      if (s + 2 < nslab) DT_LOAD_SLAB(s + 2)
    }
    const unsigned char* B_ = smem_d + buf * BUF;
    typename F::frag a[2][F::PLANES];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int p = 0; p < F::PLANES; ++p) a[i][p] = *reinterpret_cast<const typename F::frag*>(B_ + xoff + p * DX_PLANE + i * 128);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      typename F::frag b[F::PLANES];
#pragma unroll
      for (int p = 0; p < F::PLANES; ++p) b[p] = *reinterpret_cast<const typename F::frag*>(B_ + yoff + p * DX_PLANE + j * 128);
      f32x16 c0 = acc[0][j], c1 = acc[1][j];
      F::mfma(c0, c1, a, b);
      acc[0][j] = c0; acc[1][j] = c1;
    }
    if (!is_y && s + 1 < nslab) DT_STORE_SLAB(buf ^ 1)
    F::barrier();
  }
#undef DT_LOAD_SLAB
#undef DT_STORE_SLAB
#undef DT_FETCH_
#undef DT_FINISH_

  // SCALED: undo 2^G in two exact steps (G can exceed the fp32 exponent range of a single factor)
  SplitPow2 un = {1.0f, 1.0f};
  if constexpr (F::SCALED) un = split_pow2(-G);
  dw_store_partial<F::SCALED>(g.partial + chunk * (long)g.Npad * g.ldk, g, acc, n0 + wr * 64, k0 + wc * 128, lane, un.u1, un.u2);
  if (want_colsum) {   // bias gradient: the four point-quad owners of a column group add their sums in a fixed order
    float* cs = reinterpret_cast<float*>(smem_d);          // [4 quads][256 columns]; the slab buffers are dead now
    if (!is_y) *reinterpret_cast<f4*>(cs + q * 256 + c4 * 4) = csum;
    F::barrier();
    if (tid < 256 && n0 + tid < g.Npad) g.colsum[chunk * g.Npad + n0 + tid] = ((cs[tid] + cs[256 + tid]) + cs[512 + tid]) + cs[768 + tid];
  }
}

template <class F>
static void launch_dw_split(const DwGemm& g, int n0, int k0, cnr_stream s) {
  F::Pins::first_match(g, [&](auto pin) {
    const size_t lds = (size_t)2 * dw_split_buf<F>;
    const int tn_ = (g.N - n0) < 256 ? (g.N - n0) : 256, tk_ = (g.K - k0) < 256 ? (g.K - k0) : 256;
    TimingScope ts_(F::name, 1, 4224, g.P, tn_, tk_, g.npairs, s, dw_gemm_bytes(g, tn_, tk_));
    launch_lds<dw_gemm_split_kernel<F, decltype(pin)>>(dim3(g.nchunk), dim3(512), lds, lds, s, g, n0, k0);
  });
}

// ================================================================================================
// weight-gradient strips with one very narrow side (<= 8 columns): the 3 / 6 extra input columns of the colour and
// relight nets, the rgb / sdf output rows.  Pure HBM streams (<= 12 FLOP per loaded byte): no matrix cores, no LDS
// staging.  One workgroup per point chunk, 16 waves, each wave walks its own points (slabs dealt as DwSlabs says);
// a lane owns 4 columns of the wide operand x all narrow columns in registers; the 8 waves are folded
// through LDS in a fixed order.  NARROW_X: the narrow operand is X (rows of dW), otherwise Y (columns of dW).
// ================================================================================================
constexpr int SK_WAVES = 8;
// the pinned launches of the strips: every view VK_DIRECT with scale 1 (4 of the 5 strips of a step; the pin of two such pairs also serves a
// single one, whose second pair is never read), and the sdf row of the top SDF layer (zbar x softplus(z) + unit vector x qbar)
typedef DwPin<VK_DIRECT, VK_DIRECT, VK_DIRECT, VK_DIRECT, DW_ONES_ALL> SkDirect;
typedef DwPin<VK_DIRECT, VK_SOFTPLUS, VK_CONST_COL0, VK_DIRECT, 0x9> SkSdfRow;

template <bool NARROW_X, bool NG2, class PIN>
__global__ __launch_bounds__(SK_WAVES * 64) void dw_skinny_kernel(const DwGemm g_in, int n0, int k0, int ncnt) {
  DwGemm g = g_in;
  PIN::apply(g);
  constexpr int SK_UNROLL = NG2 ? 4 : 8;
  extern __shared__ __attribute__((aligned(16))) float smem_k[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long chunk = blockIdx.x;
  const int wide0 = NARROW_X ? k0 : n0, narrow0 = NARROW_X ? n0 : k0;
  const int wide_lim = NARROW_X ? g.ldk : g.Npad;       // wide columns beyond the padded extent are neither read nor written
  const int wcol = wide0 + lane * 4;
  const bool wlive = wcol < wide_lim;
  f4 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { acc[j].x = 0.f; acc[j].y = 0.f; acc[j].z = 0.f; acc[j].w = 0.f; }
  f4 cs0 = {0.f, 0.f, 0.f, 0.f}, cs1 = {0.f, 0.f, 0.f, 0.f};       // column sums of the narrow X operand (bias gradient)
  const bool want_colsum = NARROW_X && g.colsum != nullptr && k0 == 0;
  // points of this workgroup: wave w takes points w and w + 8 of each of its slabs
  const DwSlabs slabs(g.P, chunk, g.nchunk);
  const long my_pts = slabs.n * (16 / SK_WAVES);   // per wave
  const f4 z4 = {0.f, 0.f, 0.f, 0.f};
  for (int pair = 0; pair < g.npairs; ++pair) {
    const View& Vn = NARROW_X ? (pair == 0 ? g.X[0] : g.X[1]) : (pair == 0 ? g.Y[0] : g.Y[1]);
    const View& Vw = NARROW_X ? (pair == 0 ? g.Y[0] : g.Y[1]) : (pair == 0 ? g.X[0] : g.X[1]);
    for (long i0 = 0; i0 < my_pts; i0 += SK_UNROLL) {
      // all loads of the round are issued before any of the (interpreted) view math: one memory round trip per round
      Raw4 wr[SK_UNROLL], nr0[SK_UNROLL], nr1[SK_UNROLL];
      unsigned okmask = 0;
#pragma unroll
      for (int u = 0; u < SK_UNROLL; ++u) {
        const long i = i0 + u;
        const long pt = slabs.first_point(i >> 1) + wave + SK_WAVES * (i & 1);
        const bool ok = i < my_pts && pt < g.P;
        okmask |= ok ? (1u << u) : 0u;
        const long ptc = ok ? pt : g.P - 1;
        wr[u] = view_fetch4(Vw, ptc, wlive ? wcol : wide0);
        nr0[u] = view_fetch4(Vn, ptc, narrow0);
        if (NG2) nr1[u] = view_fetch4(Vn, ptc, narrow0 + 4);
      }
#pragma unroll
      for (int u = 0; u < SK_UNROLL; ++u) {
        const bool ok = (okmask >> u) & 1;
        const f4 w = (ok && wlive) ? view_finish4(Vw, wr[u], wcol) : z4;
        const f4 a0 = ok ? view_finish4(Vn, nr0[u], narrow0) : z4;
        f4 a1 = z4;
        if (NG2 && ok) a1 = view_finish4(Vn, nr1[u], narrow0 + 4);
#pragma unroll
        for (int j = 0; j < (NG2 ? 8 : 4); ++j) {
          const float nj = j < 4 ? a0[j & 3] : a1[j & 3];
          acc[j].x += nj * w.x; acc[j].y += nj * w.y; acc[j].z += nj * w.z; acc[j].w += nj * w.w;
        }
        if (want_colsum && pair == 0) {
          cs0.x += a0.x; cs0.y += a0.y; cs0.z += a0.z; cs0.w += a0.w;
          cs1.x += a1.x; cs1.y += a1.y; cs1.z += a1.z; cs1.w += a1.w;
        }
      }
    }
  }
  // fold the waves in a fixed order: LDS [wave][8 narrow][256 wide]
  float* red = smem_k + (size_t)wave * 8 * 256 + lane * 4;
#pragma unroll
  for (int j = 0; j < 8; ++j) *reinterpret_cast<f4*>(red + j * 256) = acc[j];
  float* csr = smem_k + (size_t)SK_WAVES * 8 * 256;
  if (want_colsum && lane == 0) {
    *reinterpret_cast<f4*>(csr + wave * 8) = cs0;
    *reinterpret_cast<f4*>(csr + wave * 8 + 4) = cs1;
  }
  __syncthreads();
  float* out = g.partial + chunk * (long)g.Npad * g.ldk;
  for (int e = tid; e < 8 * 256; e += SK_WAVES * 64) {
    const int j = e >> 8, c = e & 255;
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < SK_WAVES; ++w) sum += smem_k[(size_t)w * 8 * 256 + e];
    const int n = NARROW_X ? narrow0 + j : wide0 + c, k = NARROW_X ? wide0 + c : narrow0 + j;
    if (j < ncnt && n < g.Npad && k < g.ldk) out[(long)n * g.ldk + k] = sum;
  }
  if (want_colsum && tid < ncnt) {
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < SK_WAVES; ++w) sum += csr[w * 8 + tid];
    if (n0 + tid < g.Npad) g.colsum[chunk * g.Npad + n0 + tid] = sum;
  }
}

template <bool NARROW_X, bool NG2, class PIN>
static void launch_dw_skinny_td(const DwGemm& g, int n0, int k0, int ncnt, cnr_stream s) {
  const size_t lds = ((size_t)SK_WAVES * 8 * 256 + SK_WAVES * 8) * sizeof(float);
  const int wide = NARROW_X ? ((g.K - k0) < 256 ? (g.K - k0) : 256) : ((g.N - n0) < 256 ? (g.N - n0) : 256);
  const int tn_ = NARROW_X ? ncnt : wide, tk_ = NARROW_X ? wide : ncnt;
  TimingScope ts_("dw_skinny", 1, NARROW_X ? 1 : 2, g.P, tn_, tk_, g.npairs, s, dw_gemm_bytes(g, tn_, tk_));
  launch_lds<dw_skinny_kernel<NARROW_X, NG2, PIN>>(dim3(g.nchunk), dim3(SK_WAVES * 64), lds, lds, s, g, n0, k0, ncnt);
}

template <bool NARROW_X, bool NG2>
static void launch_dw_skinny_t(const DwGemm& g, int n0, int k0, int ncnt, cnr_stream s) {
  if (SkDirect::matches(g) || DwPin<VK_DIRECT, VK_DIRECT, -1, -1, DW_ONES_ALL>::matches(g)) launch_dw_skinny_td<NARROW_X, NG2, SkDirect>(g, n0, k0, ncnt, s);
  else if (NARROW_X && SkSdfRow::matches(g)) launch_dw_skinny_td<NARROW_X, NG2, SkSdfRow>(g, n0, k0, ncnt, s);
  else launch_dw_skinny_td<NARROW_X, NG2, DwInterpreted>(g, n0, k0, ncnt, s);
}

template <bool NARROW_X>
static void launch_dw_skinny(const DwGemm& g, int n0, int k0, int ncnt, cnr_stream s) {
  if (ncnt > 4) launch_dw_skinny_t<NARROW_X, true>(g, n0, k0, ncnt, s);
  else launch_dw_skinny_t<NARROW_X, false>(g, n0, k0, ncnt, s);
}

void be_dw_gemm(const DwGemm& g, cnr_stream s) {
  // tile the [Npad x ldk] output: 256x256 main tiles, 256x64 column tails, 32x256 row tails
  const bool dw_fp32 = debug_flags().dw_fp32;   // debugging aid: FP32-MFMA kernel for the main tiles too
  const bool dw_bf16 = debug_flags().dw_bf16;   // debugging aid: split-bf16 kernel even when row scales are available
  for (int n0 = 0; n0 < g.N; n0 += 256) {
    const int nrem = g.N - n0;
    for (int k0 = 0; k0 < g.K;) {
      const int krem = g.K - k0;
      if (nrem > 32) {
        if (krem > 64 && g.skip_main) { k0 += 256; continue; }   // main tile formed by the fused layer + weight-gradient launch
        if (krem > 64) {
          const DwMainTile t = dw_main_tile(g, n0, dw_fp32, dw_bf16);
          DwGemm gm = g;
          gm.npairs = t.npairs;
          if (t.form == DW_TILE_FP32) launch_dw<4, 2, 2, 4>(gm, n0, k0, s);
          else if (t.form == DW_TILE_F16) launch_dw_split<DwF16>(gm, n0, k0, s);
          else launch_dw_split<DwBf16>(gm, n0, k0, s);
          k0 += 256;
        }
        else if (krem <= 8 && !dw_fp32 && !(g.colsum != nullptr && k0 == 0) && (k0 & 3) == 0) { launch_dw_skinny<false>(g, n0, k0, krem, s); k0 += 64; }
        else {   // 9..64-column strips (embedding inputs): FP32-MFMA tile, view kinds pinned for the two shapes of the plan
          DwPinList<DwPin<VK_DIRECT, VK_DIRECT, -1, -1, DW_ONES_ALL>, DwPin<VK_DIRECT, VK_DIRECT, VK_SIGMUL, VK_DIRECT, DW_ONES_ALL>, DwInterpreted>::first_match(
              g, [&](auto pin) { launch_dw<8, 1, 1, 2, decltype(pin)>(g, n0, k0, s); });
          k0 += 64;
        }
      } else if (nrem <= 8 && !dw_fp32 && (n0 & 3) == 0) {
        launch_dw_skinny<true>(g, n0, k0, nrem, s); k0 += 256;
      } else {
        launch_dw<1, 8, 1, 1>(g, n0, k0, s); k0 += 256;
      }
    }
  }
  CNR_LAUNCH_CHECK("dw_gemm");
}


}  // namespace cnr
