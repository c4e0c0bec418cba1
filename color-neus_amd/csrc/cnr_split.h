// The split-f16 arithmetic of every matrix product on the hot path, written once ("Arithmetic").
//
// A row is lifted by an exact power of two into the top f16 binade and split into hi + lo f16 planes (11 + 11 significand bits); three
// MFMAs (hi x lo, lo x hi, hi x hi) form the product in fp32 and the scales are undone exactly.  The weight-gradient kernels contract over
// points, where a scale must cancel per point: X' = X * sx, Y' = Y * 2^G / sx with one block exponent G = 1 + min log2(sx * sy) over the
// points seen, so X'^T Y' = 2^G X^T Y exactly; G is a running minimum (the accumulators are rescaled by the exact power of two when it
// drops) and 2^G is undone at the end in two exact factors (G can exceed the exponent range of one).
// Device functions only, no state.  The CPU emulation does not split.
#pragma once
#include <hip/hip_runtime.h>

#include "cnr_gemm_int.h"

namespace cnr {

// ---- the row scale ------------------------------------------------------------------------------------------------------------
// a row takes part in the scaling when its largest |element| is positive and finite
__device__ __forceinline__ bool split_row_valid(float mx) { return mx > 0.0f && mx < 3.0e38f; }
// exact power of two that lifts a row's largest |element| mx into the top f16 binade: 2^(14 - e), e = the frexpf exponent of mx read from
// the exponent field (no libm call; subnormals land below the clamp, which keeps the scale itself finite: 2^-114 .. 2^114); 1 for a row
// that is all zero or not finite
__device__ __forceinline__ float split_row_scale(float mx) {
  float sc = 1.0f;
  if (split_row_valid(mx)) {
    int e = (int)((__float_as_uint(mx) >> 23) & 0xffu) - 126;
    if (e < -100) e = -100;
    sc = __uint_as_float((unsigned)(127 + 14 - e) << 23);
  }
  return sc;
}
// the row scale as its consumers get it (LayerGemm::rs_out, the ss[] rows in LDS): 0 for an all-zero row, NaN for a non-finite one, which
// must keep poisoning the weight gradient
__device__ __forceinline__ float split_rs_value(float mx, float sc) { return split_row_valid(mx) ? sc : (mx == 0.0f ? 0.0f : __builtin_nanf("")); }

// ---- hi / lo planes -----------------------------------------------------------------------------------------------------------
struct SplitF16 { _Float16 hi, lo; };
__device__ __forceinline__ SplitF16 split_f16(float x) {
  const _Float16 hi = (_Float16)x;
  return {hi, (_Float16)(x - (float)hi)};
}
// 4 values that already carry their scale -> one 8-byte store per plane (`plane`: byte distance from the hi plane to the lo plane)
__device__ __forceinline__ void split_store4(const f4& x, unsigned char* dst, int plane) {
  f16x4 hi, lo;
#pragma unroll
  for (int i = 0; i < 4; ++i) { const SplitF16 s = split_f16(x[i]); hi[i] = s.hi; lo[i] = s.lo; }
  *reinterpret_cast<f16x4*>(dst) = hi;
  *reinterpret_cast<f16x4*>(dst + plane) = lo;
}
// 4 consecutive columns of one row, times the row scale
__device__ __forceinline__ void split_put4(const f4& v, float sc, unsigned char* dst, int plane) { split_store4(v * sc, dst, plane); }
// 16 consecutive columns of one row out of an accumulator block, on packed conversions (two 16-byte stores per plane)
__device__ __forceinline__ void split_put16(const f32x16& a, float sc, unsigned char* dst, int plane) {
  h2 hi[8], lo[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    f2 x = {a[2 * q], a[2 * q + 1]};
    x = x * sc;
    hi[q] = __builtin_convertvector(x, h2);
    const f2 back = __builtin_convertvector(hi[q], f2);
    lo[q] = __builtin_convertvector(x - back, h2);
  }
  f16x8 h1a = {hi[0][0], hi[0][1], hi[1][0], hi[1][1], hi[2][0], hi[2][1], hi[3][0], hi[3][1]};
  f16x8 h1b = {hi[4][0], hi[4][1], hi[5][0], hi[5][1], hi[6][0], hi[6][1], hi[7][0], hi[7][1]};
  f16x8 h2a = {lo[0][0], lo[0][1], lo[1][0], lo[1][1], lo[2][0], lo[2][1], lo[3][0], lo[3][1]};
  f16x8 h2b = {lo[4][0], lo[4][1], lo[5][0], lo[5][1], lo[6][0], lo[6][1], lo[7][0], lo[7][1]};
  *reinterpret_cast<f16x8*>(dst) = h1a;
  *reinterpret_cast<f16x8*>(dst + 16) = h1b;
  *reinterpret_cast<f16x8*>(dst + plane) = h2a;
  *reinterpret_cast<f16x8*>(dst + plane + 16) = h2b;
}

// ---- the three MFMAs of one split product --------------------------------------------------------------------------------------------
// c += a b for a = a1 + a2, b = b1 + b2 (hi + lo planes): a1 b2 + a2 b1 + a1 b1, small terms first; the dropped a2 b2 is < 2^-22 relative
__device__ __forceinline__ void split_mfma3_32(f32x16& c, const f16x8& a1, const f16x8& a2, const f16x8& b1, const f16x8& b2) {
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b2, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a2, b1, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, c, 0, 0, 0);
}
__device__ __forceinline__ void split_mfma3_16(f32x4& c, const f16x8& a1, const f16x8& a2, const f16x8& b1, const f16x8& b2) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b2, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2, b1, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b1, c, 0, 0, 0);
}

// ---- the block exponent of a contraction over points ------------------------------------------------------------------------------
constexpr int SPLIT_GBIG = 0x3f000000;   // "no point with two non-zero rows yet"
// log2(sa * sb) of two power-of-two scales, from their exponent fields
__device__ __forceinline__ int split_exp2_of_product(float sa, float sb) {
  return (int)((__float_as_uint(sa) >> 23) & 0xff) + (int)((__float_as_uint(sb) >> 23) & 0xff) - 254;
}
// 2^G / sx for a power-of-two sx > 0 by exponent arithmetic (0 stays 0, NaN stays NaN, underflow flushes to 0)
__device__ __forceinline__ float split_yscale(float sx, int G) {
  const int field = G - (int)((__float_as_uint(sx) >> 23) & 0xff) + 254;      // biased exponent of 2^(G - log2 sx)
  const float r = __uint_as_float((unsigned)(field < 1 ? 0 : (field > 254 ? 254 : field)) << 23);
  return sx > 0.0f ? (field < 1 ? 0.0f : r) : sx;
}
// 2^e as two exact factors u1 * u2 (e can exceed the fp32 exponent range of a single factor)
struct SplitPow2 { float u1, u2; };
__device__ __forceinline__ SplitPow2 split_pow2(int e) { return {ldexpf(1.0f, e / 2), ldexpf(1.0f, e - e / 2)}; }
// an accumulator (fp32 vector, or array of them) times 2^e, exactly; element by element, so that no half-scaled copy of a block is live
template <class V>
__device__ __forceinline__ void split_rescale(V& v, const SplitPow2& u) {
#pragma unroll
  for (int r = 0; r < (int)(sizeof(V) / sizeof(float)); ++r) v[r] = v[r] * u.u1 * u.u2;
}
template <class V, int N>
__device__ __forceinline__ void split_rescale(V (&a)[N], const SplitPow2& u) {
#pragma unroll
  for (int i = 0; i < N; ++i) split_rescale(a[i], u);
}
// G = 1 + the running minimum of log2(sx * sy) over the tiles folded so far
struct SplitBlockExp {
  int G = SPLIT_GBIG;
  // fold a tile's minimum (SPLIT_GBIG: no live point in it)
  __device__ __forceinline__ void fold(int qmin) {
    if (qmin < SPLIT_GBIG && qmin + 1 < G) G = qmin + 1;
  }
  // ... and carry what has been accumulated under the old exponent over to the new one
  template <class A>
  __device__ __forceinline__ void fold(int qmin, A& acc) {
    if (qmin < SPLIT_GBIG && qmin + 1 < G) {
      if (G < SPLIT_GBIG) split_rescale(acc, split_pow2(qmin + 1 - G));
      G = qmin + 1;
    }
  }
  // the factors that take the finished sums back from 2^G
  __device__ __forceinline__ SplitPow2 undo() const { return split_pow2(G >= SPLIT_GBIG ? 0 : -G); }
};

}  // namespace cnr
