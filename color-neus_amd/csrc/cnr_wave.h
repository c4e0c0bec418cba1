// Wave (64 lanes) and workgroup folds, scans and exchanges of the HIP translation units: every butterfly, scan and halving exchange by shuffle is
// written here once.  A function that holds a workgroup barrier says so; all others are barrier-free and want the whole wave to arrive.
// Float folds have ONE order (results are compared bit for bit between launches and builds); the integer ones are exact in any order.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace cnr {

// ---- folds over the wave: butterfly d = 32 .. 1, the result in every lane -----------------------------------------------------------
template <class T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
  return x;
}
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x = fmaxf(x, __shfl_xor(x, d));
  return x;
}
__device__ __forceinline__ int wave_min_int(int x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const int y = __shfl_xor(x, d); x = y < x ? y : x; }
  return x;
}
// the halving tree x[j] += x[j + d], d = 32 .. 1, over the wave's 64 values in lane order: the result in lane 0 ONLY (the lanes whose partner
// lies past the wave add their own value and are never read).  An order a sequential program restates with the same loop.
template <class T>
__device__ __forceinline__ T wave_fold_down(T x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d);
  return x;
}
// sum over the 16 lanes of a row (lane & ~15 .. | 15): butterfly d = 8 .. 1, the result in every lane of the row
__device__ __forceinline__ float row16_sum(float x) {
#pragma unroll
  for (int d = 8; d >= 1; d >>= 1) x += __shfl_xor(x, d, 16);
  return x;
}
// sum over a 256-thread block, (s0 + s1) + (s2 + s3) over the waves; result valid in every thread.  TWO barriers: one in front of the store of the
// wave sums (sh4 may still be read from an earlier call), one behind it
template <class T>
__device__ __forceinline__ T block_sum_256(T x, T* sh4 /*>= 4 values*/) {
  x = wave_sum(x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = x;
  __syncthreads();
  return (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
}

// ---- float scans along the wave (per-ray kernels: lane = sample) -------------------------------------------------------------------------
__device__ __forceinline__ float wave_scan_incl_add(float x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { float y = __shfl_up(x, d); if (lane >= d) x = y + x; }
  return x;
}
__device__ __forceinline__ float wave_scan_incl_mul(float x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { float y = __shfl_up(x, d); if (lane >= d) x = y * x; }
  return x;
}
// exclusive product scan along a ray in chunks of 64: the product of f over the lanes below times the carry of the earlier chunks, which
// then takes this chunk in
__device__ __forceinline__ float wave_excl_cumprod(float f, int lane, float& carry) {
  const float incl = wave_scan_incl_mul(f, lane);
  float excl = __shfl_up(incl, 1);
  if (lane == 0) excl = 1.0f;
  const float T = carry * excl;
  carry = carry * __shfl(incl, 63);
  return T;
}
// reverse inclusive scan: result[lane] = sum_{l >= lane} x[l]
__device__ __forceinline__ float wave_scan_incl_add_rev(float x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { float y = __shfl_down(x, d); if (lane + d < 64) x = x + y; }
  return x;
}

// ---- integer scans (int or unsigned, or their 64-bit forms; exact whatever the order) -------------------------------------------------------
// inclusive scan of CH channels along the wave, the channels' shuffles interleaved
template <int CH, class T>
__device__ __forceinline__ void wave_incl_scan_int(T (&x)[CH], int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    T y[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) y[c] = sizeof(T) == 8 ? (T)__shfl_up((long long)x[c], d) : (T)__shfl_up((int)x[c], d);
#pragma unroll
    for (int c = 0; c < CH; ++c) if (lane >= d) x[c] += y[c];
  }
}
// Exclusive scan of CH channels over a workgroup of NWAVES waves (thread order): excl[c] = carry[c] + the x[c] of every thread below this one.
// The wave totals travel through wsum (LDS, caller-provided).  carry: LDS, CH values the caller set (and made visible) before the first trip; it
// then takes this trip's total in, so the next trip continues the scan and after the last trip it holds the grand total.  carry == nullptr (a
// compile-time fact at the call): a single trip that starts from zero.
// Barriers: ONE between the wave totals' store and their use; with a carry TWO more, in front of and behind the carry's update -- wsum and carry
// may be reused as soon as the call returns.  Without a carry the caller places a barrier before it touches wsum again.
template <int NWAVES, int CH, class T>
__device__ __forceinline__ void block_excl_scan(const T (&x)[CH], T (&excl)[CH], T (*wsum)[NWAVES], T* carry) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T incl[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) incl[c] = x[c];
  wave_incl_scan_int(incl, lane);
  if (lane == 63) {
#pragma unroll
    for (int c = 0; c < CH; ++c) wsum[c][wave] = incl[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < CH; ++c) excl[c] = (carry ? carry[c] : (T)0) + incl[c] - x[c];
  for (int w = 0; w < wave; ++w) {
#pragma unroll
    for (int c = 0; c < CH; ++c) excl[c] += wsum[c][w];
  }
  if (carry) {
    __syncthreads();
    if (threadIdx.x == NWAVES * 64 - 1) {
#pragma unroll
      for (int c = 0; c < CH; ++c) carry[c] = excl[c] + x[c];
    }
    __syncthreads();
  }
}

// The carried scan of ONE workgroup of NWAVES waves through n elements: an exclusive scan of CH channels in trips of NWAVES * 64 * PER elements,
// thread t of a trip owning PER consecutive ones.  read(i, x) adds element i's contribution to the channel sums x[CH] and may return a small
// payload, kept in registers until the write-back; write(i, at, payload) -- write(i, at) when read returns nothing -- stores element i from the
// running offsets at[CH] (the exclusive values on arrival at the thread's first element) and moves them past the element when PER > 1.  Neither
// is called for i >= n.  wsum and carry are the caller's, as with block_excl_scan; the carry is zeroed here and holds the grand totals on return
// (visible to every thread: the last trip ends behind a barrier).  The whole workgroup must arrive.
template <int NWAVES, int PER, int CH, class T, class I, class Read, class Write>
__device__ __forceinline__ void block_carried_scan(I n, T (*wsum)[NWAVES], T* carry, Read read, Write write) {
  using P = decltype(read(n, *static_cast<T (*)[CH]>(nullptr)));   // the payload's type; void: read keeps nothing
  constexpr bool kKeeps = !std::is_void_v<P>;
  if (threadIdx.x < CH) carry[threadIdx.x] = (T)0;
  __syncthreads();
  for (I base = 0; base < n; base += NWAVES * 64 * PER) {
    const I i0 = base + (I)threadIdx.x * PER;
    T x[CH] = {}, at[CH];
    std::conditional_t<kKeeps, P, char> keep[PER] = {};
#pragma unroll
    for (int j = 0; j < PER; ++j) if (i0 + j < n) { if constexpr (kKeeps) keep[j] = read(i0 + j, x); else read(i0 + j, x); }
    block_excl_scan<NWAVES, CH, T>(x, at, wsum, carry);
#pragma unroll
    for (int j = 0; j < PER; ++j) if (i0 + j < n) { if constexpr (kKeeps) write(i0 + j, at, keep[j]); else write(i0 + j, at); }
  }
}

// A bid for the largest 64-bit key in *best.  Bid only when you can win: a key not above the best so far (a relaxed agent-scope load) cannot
// change it, and its atomic on the one word would only make the others wait.
__device__ __forceinline__ void bid_max(unsigned long long* best, unsigned long long key) {
  if (key > __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(best, key);
}

// ---- appending to a list in global memory ------------------------------------------------------------------------------------------------------
// The lanes of the wave with `flag` take consecutive places behind *counter: ballot + popcount, ONE atomic add per wave (by the first flagged
// lane, none when no lane is flagged).  Returns this lane's place (meaningful in the flagged lanes).  The whole wave must arrive.
__device__ __forceinline__ int wave_append(bool flag, int* counter) {
  const unsigned long long mask = __ballot(flag);
  if (mask == 0) return 0;
  const int lane = threadIdx.x & 63, first = __ffsll((long long)mask) - 1;
  int base = 0;
  if (lane == first) base = atomicAdd(counter, __popcll(mask));
  base = __shfl(base, first);
  return base + __popcll(mask & ((1ull << lane) - 1ull));
}

// ---- 64 sums over the wave at once -----------------------------------------------------------------------------------------------------------
// Halving exchange: every lane brings 64 partial values, lane L gets back the sum of part[L] over the 64 lanes (63 exchanges for 64 sums).  In
// step mk a lane keeps the half of its values that belongs to its side of the mask and adds the partner's.  Steps 32 and 16 by VALU lane swaps:
// v_permlane32_swap(v[i], v[i + mk]) leaves {(lo of v[i], lo of v[i + mk]), (hi of v[i], hi of v[i + mk])}, i.e. in every lane the value it keeps and the
// one its partner sends -- their sum is keep + recv of the shuffle form of the steps below (a + b commutes: the same bits).  Fixed order: deterministic.
__device__ __forceinline__ float wave_halving_sum64(const float (&part)[64]) {
  const int lane = threadIdx.x & 63;
  float v[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) v[i] = part[i];
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[i]), __float_as_uint(v[i + 32]), false, false);
    v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[i]), __float_as_uint(v[i + 16]), false, false);
    v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
#pragma unroll
  for (int mk = 8; mk >= 1; mk >>= 1) {
    const bool up = (lane & mk) != 0;
#pragma unroll
    for (int i = 0; i < mk; ++i) {
      const float keep = up ? v[i + mk] : v[i];
      const float send = up ? v[i] : v[i + mk];
      v[i] = keep + __shfl_xor(send, mk);
    }
  }
  return v[0];
}

}  // namespace cnr
