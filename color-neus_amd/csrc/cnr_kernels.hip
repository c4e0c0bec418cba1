// HIP kernels of the render path for gfx950 (MI355X / CDNA4) that are neither a layer / chain launch (cnr_gemm*.hip, cnr_chain*.hip, cnr_sweep0.hip,
// cnr_narrow_bwd.hip) nor a one-wavefront-per-ray kernel (cnr_perray.hip).  No CUDA compatibility layer, no dual paths: wave = 64 lanes.
//
// Kernels
//   head_fwd / head_bwd / strip_bwd: the <= 4-wide heads and the few input columns beyond 256, one streaming pass each
//   point-wise kernels: the render path's rows of CNR_POINTWISE_KERNELS, the row-staged positional encodings (embed_z / embed_pts / fine_setup),
//                       the PE-Jacobian kernels with 16 lanes per point (grad_finish / gbar_finish)
//   weight preparation (weight-norm), the f16 plane split and the weight-gradient finish: all layers of a model in one launch each
//   reduce_eik / variance_finish: the two one-workgroup folds behind the compositor
// The run-time state shared by all units (error latch, timing, ranges, memset / column helpers) is in cnr_runtime.hip; every stand-alone
// family has a unit of its own (cnr_<family>.hip).
#include <hip/hip_runtime.h>

#include "cnr_backend.h"
#include "cnr_bodies.h"
#include "cnr_hip_util.h"
#include "cnr_split.h"
#include "cnr_wave.h"

namespace cnr {

// ------------------------------------------------------------------------------------------------
// backward of a 3-wide head: one pass over the 1 KB/point input of the head (see HeadBwd in cnr_backend.h).  One thread per column,
// points of a slot in order (fixed summation order), 8 points in flight.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void head_bwd_kernel(const HeadBwd p, long pts_per_slot) {
  // 64 column groups (4 columns, 16-byte accesses) x 8 row lanes; a row lane walks the points p0 + rl, p0 + rl + 8, ... of the slot, eight of
  // them in flight; the row lanes are folded in a fixed order through LDS at the end
  __shared__ float red[8][4][256];
  const int cg = threadIdx.x & 63, rl = threadIdx.x >> 6, k = cg * 4;
  const long p0 = (long)blockIdx.x * pts_per_slot;
  long p1 = p0 + pts_per_slot;
  if (p1 > p.P) p1 = p.P;
  const bool live = k < p.K;                      // (K is a multiple of 4 here: 256)
  f4 w[4], acc[4];
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  const f4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) { acc[j] = z4; w[j] = (live && j < p.n) ? *reinterpret_cast<const f4*>(p.W + (long)j * p.ldw + k) : z4; }
  // the rows of the next trip are requested before this trip's arithmetic and STORES: a load issued behind the stores would be waited for
  // together with the wave's whole store queue (one in-order counter), and one workgroup per CU has nothing else to hide the latency with
  f4 an[8], dn[8];
  const int kl = live ? k : 0;
  auto fetch = [&](long pt) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      long q = pt + 8 * u < p1 ? pt + 8 * u : p1 - 1;
      if (q < 0) q = 0;
      an[u] = *reinterpret_cast<const f4*>(p.aux + q * p.ldaux + kl);   // (every lane loads from a clamped address; dead column groups are masked below)
      dn[u] = *reinterpret_cast<const f4*>(p.dtop + q * p.ldt);     // (ldt is a multiple of 4; columns >= n are zero padding)
    }
  };
  fetch(p0 + rl);
  for (long pt = p0 + rl; pt < p1; pt += 64) {
    f4 a[8], d[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { a[u] = live ? an[u] : z4; d[u] = dn[u]; }
    fetch(pt + 64);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (pt + 8 * u < p1) {
        const float dj[4] = {d[u].x, d[u].y, d[u].z, d[u].w};
        f4 v = z4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v.x = fmaf(w[j].x, dj[j], v.x); v.y = fmaf(w[j].y, dj[j], v.y); v.z = fmaf(w[j].z, dj[j], v.z); v.w = fmaf(w[j].w, dj[j], v.w);
          acc[j].x = fmaf(dj[j], a[u].x, acc[j].x); acc[j].y = fmaf(dj[j], a[u].y, acc[j].y);
          acc[j].z = fmaf(dj[j], a[u].z, acc[j].z); acc[j].w = fmaf(dj[j], a[u].w, acc[j].w);
          cs[j] += dj[j];
        }
        f4 o;
        o.x = a[u].x > 0.0f ? v.x : 0.0f; o.y = a[u].y > 0.0f ? v.y : 0.0f; o.z = a[u].z > 0.0f ? v.z : 0.0f; o.w = a[u].w > 0.0f ? v.w : 0.0f;
        if (live) *reinterpret_cast<f4*>(p.dout + (pt + 8 * u) * p.ldo + k) = o;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) *reinterpret_cast<f4*>(&red[rl][j][k]) = acc[j];
  __shared__ float redc[8][4];
  if (cg == 0) { for (int j = 0; j < 4; ++j) redc[rl][j] = cs[j]; }
  __syncthreads();
  float* out = p.partial + (long)blockIdx.x * p.npad * p.ldk;
  for (int e = threadIdx.x; e < p.n * 256; e += 512) {
    const int j = e >> 8, c = e & 255;
    float sum = 0.0f;
#pragma unroll
    for (int r = 0; r < 8; ++r) sum += red[r][j][c];
    if (c < p.ldk) out[(long)j * p.ldk + c] = sum;
  }
  if (p.colsum && threadIdx.x < p.n) {
    float sum = 0.0f;
    for (int r = 0; r < 8; ++r) sum += redc[r][threadIdx.x];
    p.colsum[(long)blockIdx.x * p.npad + threadIdx.x] = sum;
  }
}
void be_head_bwd(const HeadBwd& p, cnr_stream s) {
  const long per = round_up((int)((p.P + p.nslots - 1) / p.nslots), 64);
  TimingScope ts_("head_bwd", 2, p.n, p.P, p.K, p.n, 1, s, (double)p.P * (8.0 * p.K + 16.0));
  hipLaunchKernelGGL(head_bwd_kernel, dim3(p.nslots), dim3(512), 0, s, p, per);
  CNR_LAUNCH_CHECK("head_bwd");
}

// ------------------------------------------------------------------------------------------------
// strips of a (256 + nt)-input layer in the backward pass (see StripBwd in cnr_backend.h): one pass over the 1 KB/point cotangent.
// A wave owns one point at a time (lane = 4-column group), PTS points in flight.  The PTS x NT partial dot products of a lane are summed
// over the 64 lanes by a halving exchange (each step a lane gives away the half of its values that belongs to the other side of the
// mask): 63 shuffles for 64 sums, lane L ends with the sum of index L = point (L / NT), column (L % NT).  Fixed order: deterministic.
// ------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(512) void strip_bwd_kernel(const StripBwd p, long pts_per_slot) {
  constexpr int PTS = 64 / NT;                    // points in flight per wave
  extern __shared__ __attribute__((aligned(16))) float strip_red[];   // [8 waves][NT][256]
  const int lane = threadIdx.x & 63, k = lane * 4;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long p0 = (long)blockIdx.x * pts_per_slot;
  long p1 = p0 + pts_per_slot;
  if (p1 > p.P) p1 = p.P;
  const f4 z4 = {0.f, 0.f, 0.f, 0.f};
  f4 w[NT], acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) { acc[j] = z4; w[j] = j < p.nt ? *reinterpret_cast<const f4*>(p.Wt + (long)(256 + j) * p.ldwt + k) : z4; }
  const int yu = lane / NT, yj = lane % NT;       // the (point, column) whose y value this lane fetches and whose dot product it ends up with
  // the rows of the next trip are requested before this trip's arithmetic (one workgroup of 8 waves per CU: nothing else hides the latency)
  f4 dn[PTS];
  float yn = 0.0f;
  auto fetch = [&](long pt) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < PTS; ++u) {
      long q = pt + u < p1 ? pt + u : p1 - 1;
      if (q < p0) q = p0 < p.P ? p0 : p.P - 1;          // (an empty slot: never used)
      dn[u] = *reinterpret_cast<const f4*>(p.dout + q * p.ldo + k);
    }
    long qy = pt + yu < p1 ? pt + yu : p1 - 1;
    if (qy < 0) qy = 0;
    yn = p.y[qy * p.ldy + (yj < p.nt ? yj : 0)];        // (every lane loads from a clamped address; masked below)
  };
  fetch(p0 + (long)wv * PTS);
  for (long pt = p0 + (long)wv * PTS; pt < p1; pt += 8 * PTS) {
    f4 d[PTS];
#pragma unroll
    for (int u = 0; u < PTS; ++u) d[u] = dn[u];
    const bool mine = pt + yu < p1 && yj < p.nt;
    const float yl = mine ? yn : 0.0f;
    fetch(pt + 8 * PTS);
    float v[64];
#pragma unroll
    for (int u = 0; u < PTS; ++u) {
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const float yv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, yl), u * NT + j));   // 0 past the end / j >= nt
        acc[j].x = fmaf(yv, d[u].x, acc[j].x); acc[j].y = fmaf(yv, d[u].y, acc[j].y);
        acc[j].z = fmaf(yv, d[u].z, acc[j].z); acc[j].w = fmaf(yv, d[u].w, acc[j].w);
        v[u * NT + j] = fmaf(d[u].w, w[j].w, fmaf(d[u].z, w[j].z, fmaf(d[u].y, w[j].y, d[u].x * w[j].x)));
      }
    }
    const float dot = wave_halving_sum64(v);
    if (p.tail && mine) p.tail[(pt + yu) * p.ldt + yj] = dot * p.tail_scale;
  }
  // fold the 8 waves in a fixed order; a slot row is [ .. 256 main columns (another launch) .. | nt strip columns | zero pad up to ldk ]
#pragma unroll
  for (int j = 0; j < NT; ++j) *reinterpret_cast<f4*>(strip_red + ((long)wv * NT + j) * 256 + k) = acc[j];
  __syncthreads();
  float* out = p.partial + (long)blockIdx.x * p.npad * p.ldk;
  const int wcols = p.ldk - 256;
  for (int e = threadIdx.x; e < 256 * wcols; e += 512) {
    const int n = e / wcols, j = e - n * wcols;
    float sum = 0.0f;
    if (j < p.nt) {
#pragma unroll
      for (int r = 0; r < 8; ++r) sum += strip_red[((long)r * NT + j) * 256 + n];
    }
    if (n < p.npad) out[(long)n * p.ldk + 256 + j] = sum;
  }
}
// forward of a narrow head (see HeadFwd): a wave owns 16 points at a time (lane = 4-column group), the 16 x 4 partial dot products of a lane
// are summed over the 64 lanes by the same halving exchange (wave_halving_sum64); lane L then applies the head's epilogue to point L / 4, column L % 4
// (and to the pad columns 4.., which epi_apply zero-fills where the epilogue kind asks for it).
__global__ __launch_bounds__(256) void head_fwd_kernel(const HeadFwd p) {
  const int lane = threadIdx.x & 63, k = lane * 4;
  const long P = p.P_dev ? (long)*p.P_dev : p.P;
  const f4 z4 = {0.f, 0.f, 0.f, 0.f};
  f4 w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = j < p.n ? *reinterpret_cast<const f4*>(p.W + (long)j * p.ldw + k) : z4;
  const long wave_id = ((long)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (long)gridDim.x * 4;
  for (long pt = wave_id * 16; pt < P; pt += nwaves * 16) {
    f4 d[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const long q = pt + u < P ? pt + u : P - 1;
      d[u] = *reinterpret_cast<const f4*>(p.h + q * p.ldh + k);
    }
    float v[64];
#pragma unroll
    for (int u = 0; u < 16; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) v[u * 4 + j] = fmaf(d[u].w, w[j].w, fmaf(d[u].z, w[j].z, fmaf(d[u].y, w[j].y, d[u].x * w[j].x)));
    const float dot = wave_halving_sum64(v);
    const long row = pt + (lane >> 2);
    if (row < P) {
      const int j = lane & 3;
      epi_apply(p.E, row, j, dot);
      epi_apply(p.E, row, j + 4, 0.0f);
      epi_apply(p.E, row, j + 8, 0.0f);
      epi_apply(p.E, row, j + 12, 0.0f);
    }
  }
}
void be_head_fwd(const HeadFwd& p, cnr_stream s) {
  if (p.P <= 0) return;
  long blocks = (p.P + 63) / 64;          // 4 waves x 16 points per block and trip
  if (blocks > 2048) blocks = 2048;
  TimingScope ts_("head_fwd", 2, p.n, p.P, p.n, 256, 1, s, (double)p.P * (4.0 * 256 + 32.0));
  hipLaunchKernelGGL(head_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
  CNR_LAUNCH_CHECK("head_fwd");
}

template <int NT>
static void launch_strip_bwd(const StripBwd& p, long per, cnr_stream s) {
  launch_lds<strip_bwd_kernel<NT>>(dim3(p.nslots), dim3(512), (size_t)8 * NT * 256 * sizeof(float), 64 * 1024, s, p, per);
}
void be_strip_bwd(const StripBwd& p, cnr_stream s) {
  const long per = round_up((int)((p.P + p.nslots - 1) / p.nslots), 64);
  TimingScope ts_("strip_bwd", 2, p.nt, p.P, 256, p.nt, 1, s, (double)p.P * (4.0 * 256 + 8.0 * p.nt));
  if (p.nt <= 4) launch_strip_bwd<4>(p, per, s); else launch_strip_bwd<8>(p, per, s);
  CNR_LAUNCH_CHECK("strip_bwd");
}

// ================================================================================================
// point-wise kernels
// ================================================================================================
// the render path's rows of CNR_POINTWISE_KERNELS (cnr_bodies.h), each a grid-stride kernel over its body and be_<name> (CNR_PW_KERNEL, cnr_hip_util.h)
CNR_POINTWISE_KERNELS(CNR_PW_KERNEL)

// Point-wise kernels that write kEmb / kAux-wide ROWS (192 B per point): a thread computes its point's rows into LDS (row stride 49 floats:
// conflict-free), then the block stores the 128 rows -- one contiguous 24 KB piece of the output -- with fully coalesced accesses (a thread
// storing its own row touches 64 different rows per wave instruction: 1.4 TB/s against 4+ TB/s).
constexpr int kRowsPerBlock = 128, kRowLd = 49;
static_assert(kEmb == 48 && kAux == 48, "row staging assumes 48-float rows");
template <class PARAM, void (*ROWS)(const PARAM&, long, float*, float*)>
__global__ __launch_bounds__(kRowsPerBlock) void staged_rows_kernel(const PARAM p, long n, float* E, float* AUX) {
  __shared__ float sE[kRowsPerBlock * kRowLd];
  __shared__ float sA[kRowsPerBlock * kRowLd];
  const int tid = threadIdx.x;
  for (long base = (long)blockIdx.x * kRowsPerBlock; base < n; base += (long)gridDim.x * kRowsPerBlock) {
    if (base + tid < n) ROWS(p, base + tid, sE + tid * kRowLd, sA + tid * kRowLd);
    __syncthreads();
    const int cnt = (int)((n - base) < kRowsPerBlock ? (n - base) : kRowsPerBlock) * 48;
    for (int e = tid; e < cnt; e += kRowsPerBlock) {
      const int r = e / 48, c = e - r * 48;
      E[base * 48 + e] = sE[r * kRowLd + c];
      if (AUX) AUX[base * 48 + e] = sA[r * kRowLd + c];
    }
    __syncthreads();
  }
}
template <class PARAM, void (*ROWS)(const PARAM&, long, float*, float*)>
static void staged_rows_launch(const char* name, const PARAM& p, long n, float* E, float* AUX, cnr_stream s) {
  if (n <= 0) return;
  long blocks = (n + kRowsPerBlock - 1) / kRowsPerBlock;
  if (blocks > 16384) blocks = 16384;
  TimingScope ts_(name, 2, 0, n, 0, 0, 0, s);
  hipLaunchKernelGGL((staged_rows_kernel<PARAM, ROWS>), dim3((unsigned)blocks), dim3(kRowsPerBlock), 0, s, p, n, E, AUX);
}
void be_embed_z(const EmbedZ& p, cnr_stream s) { staged_rows_launch<EmbedZ, body_embed_z_rows>("embed_z", p, p.R * p.m, p.E, nullptr, s); CNR_LAUNCH_CHECK("embed_z"); }
void be_embed_pts(const EmbedPts& p, cnr_stream s) { staged_rows_launch<EmbedPts, body_embed_pts_rows>("embed_pts", p, p.n, p.E, p.AUX, s); CNR_LAUNCH_CHECK("embed_pts"); }
void be_fine_setup(const FineSetup& p, cnr_stream s) { staged_rows_launch<FineSetup, body_fine_setup_rows>("fine_setup", p, p.R * p.M, p.E, p.AUX, s); CNR_LAUNCH_CHECK("fine_setup"); }

// ------------------------------------------------------------------------------------------------
// PE-Jacobian kernels: 16 lanes per point, lane j owns the column triple [3j, 3j+3) of the 48-wide rows
// (triple 0 = x, triple 1+2k = sin(2^k x), triple 2+2k = cos(2^k x)), so every row is read/written as one contiguous
// 192-byte segment by its 16 lanes; the sin/cos partner values travel by shuffle.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grad_finish_kernel(const GradFinish p) {
  const int lane16 = threadIdx.x & 15;
  const long pt0 = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
  const long stride = (long)gridDim.x * 16;
  for (long pt = pt0; pt < p.P; pt += stride) {   // all 16 lanes of a group share pt -> uniform trip count inside a group
    const int c0 = lane16 * 3;
    float e[3], ce[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      e[c] = p.E[pt * kEmb + c0 + c];
      ce[c] = p.ce0[pt * kEmb + c0 + c] + (p.ces ? p.ces[pt * kEmb + c0 + c] : 0.0f);
    }
    const int k = lane16 > 0 ? (lane16 - 1) >> 1 : 0;
    const bool is_sin = lane16 >= 1 && (lane16 & 1) == 1 && lane16 <= 2 * p.multires;
    const bool is_cos = lane16 >= 2 && (lane16 & 1) == 0 && lane16 <= 2 * p.multires;
    const float f = (float)(1 << k);
    float part[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float e_next = __shfl_down(e[c], 1, 16);   // sin lane reads cos(2^k x) from its right neighbour
      const float e_prev = __shfl_up(e[c], 1, 16);     // cos lane reads sin(2^k x) from its left neighbour
      float t = 0.0f;
      if (lane16 == 0) t = ce[c];
      else if (is_sin) t = f * (e_next * ce[c]);
      else if (is_cos) t = -(f * (e_prev * ce[c]));
      part[c] = t;
    }
    float g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = row16_sum(part[c]) * p.scale;
    if (lane16 == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) { p.grad_out[pt * 3 + c] = g[c]; p.AUX[pt * kAux + 3 + c] = g[c]; }
    }
    float aux[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) aux[c] = lane16 == 1 ? g[c] : p.AUX[pt * kAux + c0 + c];   // row as it will read after the update
    if (p.neg_g_as_view) {   // AUX[6:] = PE(-g): triple t >= 2 holds encoding triple (t - 2)
      const int et = lane16 - 2;
      if (et >= 0) {
        float v[3] = {-g[0], -g[1], -g[2]};
        const int npe_tr = p.multires_view > 0 ? 1 + 2 * p.multires_view : 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float val = 0.0f;
          if (et == 0) val = v[c];
          else if (et < npe_tr) { const float ff = (float)(1 << ((et - 1) >> 1)); val = (et & 1) ? sinf(v[c] * ff) : cosf(v[c] * ff); }
          if (et < npe_tr) { aux[c] = val; p.AUX[pt * kAux + c0 + c] = val; }
        }
      }
    }
    if (p.featx) {
      const int w = p.ldfx - p.F;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (c0 + c < w) p.featx[pt * p.ldfx + p.F + c0 + c] = aux[c];
      for (int c = kAux + lane16; c < w; c += 16) p.featx[pt * p.ldfx + p.F + c] = 0.0f;
    }
  }
}
void be_grad_finish(const GradFinish& p, cnr_stream s) {
  if (p.P <= 0) return;
  long blocks = (p.P * 16 + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  TimingScope ts_("grad_finish", 2, 0, p.P, 0, 0, 0, s);
  hipLaunchKernelGGL(grad_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
  CNR_LAUNCH_CHECK("grad_finish");
}

__global__ __launch_bounds__(256) void gbar_finish_kernel(const GbarFinish p) {
  const int lane16 = threadIdx.x & 15;
  const long pt0 = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
  const long stride = (long)gridDim.x * 16;
  for (long pt = pt0; pt < p.P; pt += stride) {
    const int c0 = lane16 * 3;
    float e[3], gb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      e[c] = p.E[pt * kEmb + c0 + c];
      float v = p.gbar_alpha[pt * 4 + c];
      if (p.daux_c) v += p.daux_c[pt * kAux + 3 + c];
      if (p.daux_r) v += p.daux_r[pt * kAux + 3 + c];
      gb[c] = v;
    }
    const int k = lane16 > 0 ? (lane16 - 1) >> 1 : 0;
    const bool is_sin = lane16 >= 1 && (lane16 & 1) == 1 && lane16 <= 2 * p.multires;
    const bool is_cos = lane16 >= 2 && (lane16 & 1) == 0 && lane16 <= 2 * p.multires;
    const float f = (float)(1 << k);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float e_next = __shfl_down(e[c], 1, 16);
      const float e_prev = __shfl_up(e[c], 1, 16);
      const float t = gb[c] * p.scale;
      float out = 0.0f;
      if (lane16 == 0) out = t;
      else if (is_sin) out = f * e_next * t;          // d g / d ce_sin = 2^k cos(2^k x0)
      else if (is_cos) out = -f * e_prev * t;         // d g / d ce_cos = -2^k sin(2^k x0)
      p.cbar[pt * kEmb + c0 + c] = out;
    }
    if (lane16 == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) p.gbar_total[pt * 4 + c] = gb[c];
      p.gbar_total[pt * 4 + 3] = 0.0f;
    }
  }
}
void be_gbar_finish(const GbarFinish& p, cnr_stream s) {
  if (p.P <= 0) return;
  long blocks = (p.P * 16 + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  TimingScope ts_("gbar_finish", 2, 0, p.P, 0, 0, 0, s);
  hipLaunchKernelGGL(gbar_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
  CNR_LAUNCH_CHECK("gbar_finish");
}

// ------------------------------------------------------------------------------------------------
// weight preparation and finish: all layers of a model in one launch each (RowBatch, cnr_hip_util.h), one workgroup per row
// ------------------------------------------------------------------------------------------------
// effective weights: weight-norm, column permutation, zero padding, transpose copy.  One block per padded row.
__device__ __forceinline__ void prep_weight_row(const PrepWeight& p, const int n) {
  __shared__ double redd[4];
  const int tid = threadIdx.x;                     // n: internal row
  const bool real = n < p.n;
  const int nr = real ? (n + p.row_rot) % p.n : 0;  // reference row
  float scale = 1.0f;
  if (p.g != nullptr) {
    double ss = 0.0;   // row norm in double: weight_norm is the most rounding-sensitive step (x inv_s downstream)
    if (real)
      for (int c = tid; c < p.k_ref; c += 256) { double x = p.v[(long)nr * p.k_ref + c]; ss += x * x; }
    ss = block_sum_256(ss, redd);
    if (real) scale = weight_norm_scale(p.g[nr], ss);
  }
  for (int j = tid; j < p.kpad; j += 256) {
    float val = 0.0f;
    if (real && j < p.ldw) {
      const int src = seg_src_of(p.seg, p.nseg, j);
      if (src >= 0) val = p.v[(long)nr * p.k_ref + src] * scale;
    }
    if (j < p.ldw) p.W[(long)n * p.ldw + j] = val;
    if (n < p.ldwt) p.Wt[(long)j * p.ldwt + n] = val;
  }
  if (tid == 0) p.bias[n] = real && p.b ? p.b[nr] : 0.0f;
}
using PrepBatch = RowBatch<PrepWeight, 24>;
__global__ __launch_bounds__(256) void prep_weight_batch_kernel(const PrepBatch b) { const auto at = b.locate(blockIdx.x); prep_weight_row(at.job, at.row); }
void be_prep_weights(const PrepWeight* p, int count, cnr_stream s) {
  launch_row_batches<PrepBatch>(prep_weight_batch_kernel, "prep_weight", p, count, 256, s, [](const PrepWeight& j) { return j.npad; });
}

// fp32 matrix -> two f16 planes of the row-scaled matrix: x * 2^e = hi + lo with e chosen per row so that max|x| * 2^e is in
// [2^13, 2^14) (exact scaling; 11 + 11 significand bits), plus 1 / 2^e per row.  One 64-thread block per row.
__device__ __forceinline__ void split_planes_row(const SplitJob& j, const int r) {
  const int ld = j.ld;
  const long plane_stride = (long)j.rows * ld;
  const float* row = j.src + (long)r * ld;
  float mx = 0.0f;
  for (int k = threadIdx.x; k < ld; k += 64) mx = fmaxf(mx, fabsf(row[k]));
  mx = wave_max(mx);
  const float sc = split_row_scale(mx);
  for (int k = threadIdx.x; k < ld; k += 64) {
    const SplitF16 h = split_f16(row[k] * sc);
    j.planes[(long)r * ld + k] = __builtin_bit_cast(unsigned short, h.hi);
    j.planes[plane_stride + (long)r * ld + k] = __builtin_bit_cast(unsigned short, h.lo);
  }
  if (threadIdx.x == 0) j.inv_scale[r] = 1.0f / sc;
}
using SplitBatch = RowBatch<SplitJob, 2 * PrepBatch::kCap>;   // (W and Wt of every prepared layer)
__global__ __launch_bounds__(64) void split_planes_batch_kernel(const SplitBatch b) { const auto at = b.locate(blockIdx.x); split_planes_row(at.job, at.row); }
void be_split_planes_many(const SplitJob* jobs, int count, cnr_stream s) {
  launch_row_batches<SplitBatch>(split_planes_batch_kernel, "split_planes", jobs, count, 64, s, [](const SplitJob& j) { return j.rows; });
}

// reduce dW partials, undo the column permutation, weight-norm backward.  One block per output row.
__device__ __forceinline__ void finish_weight_row(const FinishWeight& p, const int n) {
  __shared__ float red[4];
  __shared__ double redd[4];
  __shared__ float dwi[512];
  const int tid = threadIdx.x;                        // n: internal row
  const int nr = (n + p.row_rot) % p.n;               // reference row
  for (int j = tid; j < p.ldk; j += 256) {
    // fixed-order reduction over the chunks, 8 independent loads in flight (same summation order as a plain loop)
    const float* src = p.partial + (long)n * p.ldk + j;
    const long cs = (long)p.npad * p.ldk;
    float s = 0.0f;
    int c = 0;
    const int nch = j >= p.col_hi ? p.nchunk_hi : p.nchunk;   // (strip columns: their own slot count, see StripBwd)
    for (; c + 8 <= nch; c += 8) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = src[(long)(c + q) * cs];
#pragma unroll
      for (int q = 0; q < 8; ++q) s += v[q];
    }
    for (; c < nch; ++c) s += src[(long)c * cs];
    dwi[j] = s;
  }
  __syncthreads();
  // gather into reference column order (held in registers: <= 2 columns per thread for k_ref <= 512)
  float dref[2] = {0.f, 0.f};
  int cref[2] = {-1, -1};
  int cnt = 0;
  for (int c = tid; c < p.k_ref && cnt < 2; c += 256, ++cnt) {
    const int dst = seg_dst_of(p.seg, p.nseg, c);
    cref[cnt] = c;
    dref[cnt] = dst >= 0 ? dwi[dst] : 0.0f;
  }
  if (p.g != nullptr) {
    double dotd = 0.0, ssd = 0.0;
    for (int q = 0; q < 2; ++q)
      if (cref[q] >= 0) { double vv = p.v[(long)nr * p.k_ref + cref[q]]; dotd += (double)dref[q] * vv; ssd += vv * vv; }
    dotd = block_sum_256(dotd, redd);
    ssd = block_sum_256(ssd, redd);
    const float dot = (float)dotd;
    const float nrm = (float)sqrt(ssd);
    const float gg = p.g[nr];
    if (tid == 0) p.dg[nr] = dot / nrm;
    for (int q = 0; q < 2; ++q)
      if (cref[q] >= 0) p.dv[(long)nr * p.k_ref + cref[q]] = weight_norm_dv(gg, nrm, dot, dref[q], p.v[(long)nr * p.k_ref + cref[q]]);
  } else {
    for (int q = 0; q < 2; ++q)
      if (cref[q] >= 0) p.dv[(long)nr * p.k_ref + cref[q]] = dref[q];
  }
  if (p.db != nullptr && p.colsum != nullptr) {
    float s = 0.0f;
    const int ncs = p.ncolsum > 0 ? p.ncolsum : p.nchunk;
    for (int c = tid; c < ncs; c += 256) s += p.colsum[(long)c * p.npad + n];
    s = block_sum_256(s, red);
    if (tid == 0) p.db[nr] = s;
  }
}
using FinishBatch = RowBatch<FinishWeight, 24>;
__global__ __launch_bounds__(256) void finish_weight_batch_kernel(const FinishBatch b) { const auto at = b.locate(blockIdx.x); finish_weight_row(at.job, at.row); }
void be_finish_weights(const FinishWeight* f, int count, cnr_stream s) {
  launch_row_batches<FinishBatch>(finish_weight_batch_kernel, "finish_weight", f, count, 256, s, [](const FinishWeight& j) { return j.n; });
}

__global__ __launch_bounds__(256) void reduce_eik_kernel(const ReduceEik p) {
  __shared__ float red[4];
  float a = 0.0f, b = 0.0f;
  for (long r = threadIdx.x; r < p.R; r += 256) { a += p.partial[r * 2]; b += p.partial[r * 2 + 1]; }
  a = block_sum_256(a, red);
  b = block_sum_256(b, red);
  if (threadIdx.x == 0) {
    p.sums[0] = a; p.sums[1] = b;
    if (p.sums_out) { p.sums_out[0] = a; p.sums_out[1] = b; }
    *p.gradient_error = a / (b + 1e-5f);
  }
}
void be_reduce_eik(const ReduceEik& p, cnr_stream s) {
  TimingScope ts_("reduce_eik", 2, 0, p.R, 0, 0, 0, s);
  hipLaunchKernelGGL(reduce_eik_kernel, dim3(1), dim3(256), 0, s, p);
  CNR_LAUNCH_CHECK("reduce_eik");
}

__global__ __launch_bounds__(256) void variance_finish_kernel(const VarianceFinish p) {
  __shared__ float red[4];
  float a = 0.0f;
  for (long r = threadIdx.x; r < p.R; r += 256) a += p.partial[r];
  a = block_sum_256(a, red);
  if (threadIdx.x == 0) *p.d_variance = inv_s_backward(p.variance[0], a);
}
void be_variance_finish(const VarianceFinish& p, cnr_stream s) {
  TimingScope ts_("variance_finish", 2, 0, p.R, 0, 0, 0, s);
  hipLaunchKernelGGL(variance_finish_kernel, dim3(1), dim3(256), 0, s, p);
  CNR_LAUNCH_CHECK("variance_finish");
}

}  // namespace cnr
