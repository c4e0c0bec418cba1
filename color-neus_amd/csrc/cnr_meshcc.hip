// Connected components of an indexed triangle mesh, selection of the components to keep and order-preserving compaction for gfx950
// (cnr_mesh_components / cnr_mesh_select / cnr_mesh_compact): a lock-free union-find in the caller's labels array, integer atomics only, the
// per-element code of cnr_meshcc.h.  No host round trip, no iteration count, no scratch: every result is exact and does not depend on the order
// in which lanes, waves or workgroups run.
//
//   meshcc_init_kernel      parent[v] = v, the two count arrays, summary and dropped to zero
//   meshcc_unite_kernel     one triangle per lane: unite(t0, t1), unite(t0, t2); invalid triangles counted (ballot + popcount, one add per wave)
//   meshcc_flatten_kernel   a launch of its own, after the hooks: labels[v] = root(v) (reads only, each entry written by its own lane),
//                           vertex_count[root] += 1, n_components += (root == v)
//   meshcc_faces_kernel     one triangle per lane: face_count[labels[t0]] += 1
//   meshcc_roots_kernel     one vertex per lane: the roots with a face are counted and bid their key for "largest" (64-bit atomic max)
//   meshcc_summary_kernel   one lane decodes the key into summary[2..3]
//   meshcc_keep_kernel      keep_vertex / keep_face from the rule of cnr_mesh_select
//   meshcc_scan_kernel      two workgroups (vertices, faces): a single-workgroup carried exclusive scan of the keep flags -> the maps and totals
//                           (mesh_keep_scan: also the scan of cnr_mesh_cull_select, cnr_cull.hip)
//   meshcc_compact_kernel   one vertex and one face per lane through the maps
//
// The counts: a marching-cubes mesh is spatially ordered, so the 64 elements of a wave nearly always share one label; a wave whose flagged lanes
// all hold the same label issues ONE add of the popcount, any other wave one add per lane (wave_add_by_label).  Measured on the mesh of a
// 512-cell lattice (1.07 M triangles, 78 % of them in one component; profiles/mesh_clean_bench.txt): meshcc_faces_kernel 1.44 ms against 9.45 ms
// with one add per lane.  What remains is the adds on the one address of the main component, about 0.1 us each.
#include <hip/hip_runtime.h>

#include "cnr_meshcc.h"
#include "cnr_hip_util.h"
#include "cnr_wave.h"

namespace cnr {

constexpr int kMeshThreads = 256;

// parent[] during the hooking launch: every access an agent-scope atomic.  The loads inside find must see the hooks of workgroups on other
// XCDs -- a plain load may be served again and again from this CU's L1, which no other CU's store refreshes, and the retry loop of
// meshcc_unite would then re-find the same stale root forever.
struct MeshccAgent {
  static __device__ __forceinline__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ void store(int* p, int x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ bool hook(int* p, int hi, int lo) {
    return __hip_atomic_compare_exchange_strong(p, &hi, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// counts[label] += 1 for every lane with `flag`: one add of the popcount when all flagged lanes hold the same label, else one add per lane.
// The whole wave must arrive.
__device__ __forceinline__ void wave_add_by_label(bool flag, int label, int* counts) {
  const unsigned long long mask = __ballot(flag);
  if (mask == 0) return;
  const int lane = threadIdx.x & 63, first = __ffsll((long long)mask) - 1;
  const int label0 = __shfl(label, first);
  if (__ballot(flag && label != label0) == 0) {
    if (lane == first) atomicAdd(&counts[label0], __popcll(mask));
  } else if (flag) {
    atomicAdd(&counts[label], 1);
  }
}

__global__ __launch_bounds__(kMeshThreads) void meshcc_init_kernel(const MeshComponents p) {
  const long v = (long)blockIdx.x * kMeshThreads + threadIdx.x;
  if (v == 0) { p.summary[0] = 0; p.summary[1] = 0; p.summary[2] = 0; p.summary[3] = 0; p.dropped[0] = 0; }
  if (v < p.V) { p.labels[v] = (int)v; p.face_count[v] = 0; p.vertex_count[v] = 0; }
}

__global__ __launch_bounds__(kMeshThreads) void meshcc_unite_kernel(const MeshComponents p) {
  const long f = (long)blockIdx.x * kMeshThreads + threadIdx.x;
  int t[3] = {0, 0, 0};
  bool valid = false;
  if (f < p.F) {
    for (int k = 0; k < 3; ++k) t[k] = p.triangles[f * 3 + k];
    valid = meshcc_valid(t, p.V);
  }
  (void)wave_append(f < p.F && !valid, p.dropped);
  if (!valid) return;
  if (t[1] != t[0]) meshcc_unite<MeshccAgent>(p.labels, t[0], t[1]);
  if (t[2] != t[0]) meshcc_unite<MeshccAgent>(p.labels, t[0], t[2]);
}

__global__ __launch_bounds__(kMeshThreads) void meshcc_flatten_kernel(const MeshComponents p) {
  const long v = (long)blockIdx.x * kMeshThreads + threadIdx.x;
  int root = -1;
  if (v < p.V) {
    root = meshcc_root(p.labels, (int)v);
    p.labels[v] = root;
  }
  wave_add_by_label(v < p.V, root, p.vertex_count);
  (void)wave_append(v < p.V && root == (int)v, &p.summary[0]);
}

__global__ __launch_bounds__(kMeshThreads) void meshcc_faces_kernel(const MeshComponents p) {
  const long f = (long)blockIdx.x * kMeshThreads + threadIdx.x;
  int label = -1;
  if (f < p.F) {
    const int t[3] = {p.triangles[f * 3], p.triangles[f * 3 + 1], p.triangles[f * 3 + 2]};
    if (meshcc_valid(t, p.V)) label = p.labels[t[0]];
  }
  wave_add_by_label(label >= 0, label, p.face_count);
}

__global__ __launch_bounds__(kMeshThreads) void meshcc_roots_kernel(const MeshComponents p) {
  const long v = (long)blockIdx.x * kMeshThreads + threadIdx.x;
  int faces = 0;
  if (v < p.V && p.labels[v] == (int)v) faces = p.face_count[v];
  (void)wave_append(faces > 0, &p.summary[1]);
  if (faces > 0) bid_max(reinterpret_cast<unsigned long long*>(p.summary + 2), meshcc_key(faces, (int)v));
}

__global__ void meshcc_summary_kernel(const MeshComponents p) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long key = *reinterpret_cast<const unsigned long long*>(p.summary + 2);
    int label, faces;
    meshcc_unkey(key, &label, &faces);
    p.summary[2] = label;
    p.summary[3] = faces;
  }
}

void be_mesh_components(const MeshComponents& p, cnr_stream s) {
  const double V = (double)p.V, F = (double)p.F;
  const unsigned vb = (unsigned)((p.V + kMeshThreads - 1) / kMeshThreads), fb = (unsigned)((p.F + kMeshThreads - 1) / kMeshThreads);
  {
    TimingScope ts_("meshcc_init_kernel", 2, 0, p.V, 0, 0, 0, s, 12.0 * V + 20.0);
    hipLaunchKernelGGL(meshcc_init_kernel, dim3(vb ? vb : 1), dim3(kMeshThreads), 0, s, p);
  }
  if (p.F > 0) {
    // (12 bytes of indices per triangle; the parent entries it reads and hooks depend on the mesh: 3 reads and 1 store counted)
    TimingScope ts_("meshcc_unite_kernel", 2, 0, p.F, 0, 0, 0, s, 28.0 * F);
    hipLaunchKernelGGL(meshcc_unite_kernel, dim3(fb), dim3(kMeshThreads), 0, s, p);
  }
  if (p.V > 0) {
    TimingScope ts_("meshcc_flatten_kernel", 2, 0, p.V, 0, 0, 0, s, 12.0 * V);
    hipLaunchKernelGGL(meshcc_flatten_kernel, dim3(vb), dim3(kMeshThreads), 0, s, p);
  }
  if (p.F > 0 && p.V > 0) {
    TimingScope ts_("meshcc_faces_kernel", 2, 0, p.F, 0, 0, 0, s, 16.0 * F);
    hipLaunchKernelGGL(meshcc_faces_kernel, dim3(fb), dim3(kMeshThreads), 0, s, p);
  }
  if (p.V > 0) {
    TimingScope ts_("meshcc_roots_kernel", 2, 0, p.V, 0, 0, 0, s, 4.0 * V);
    hipLaunchKernelGGL(meshcc_roots_kernel, dim3(vb), dim3(kMeshThreads), 0, s, p);
  }
  {
    TimingScope ts_("meshcc_summary_kernel", 2, 0, 1, 0, 0, 0, s, 16.0);
    hipLaunchKernelGGL(meshcc_summary_kernel, dim3(1), dim3(64), 0, s, p);
  }
  CNR_LAUNCH_CHECK("mesh_components");
}

__global__ __launch_bounds__(kMeshThreads) void meshcc_keep_kernel(const MeshSelect p) {
  const long i = (long)blockIdx.x * kMeshThreads + threadIdx.x;
  const int thr = meshcc_threshold(p.min_faces, p.min_ratio, p.summary[3]);
  if (i < p.V) p.keep_vertex[i] = meshcc_keep_vertex(p, i, thr);
  if (i < p.F) p.keep_face[i] = meshcc_keep_face(p, i, thr);
}

// Exclusive scan of the keep flags into the maps: workgroup 0 the vertices, workgroup 1 the faces.  ONE workgroup carries its scan through the
// array in trips of kMeshScanChunk elements (kMeshScanPer consecutive elements per thread): no workgroup waits for another one.
// block_carried_scan's trip loop in this kernel's own words: here the flags are summed behind the bounds branches, so a thread's kMeshScanPer
// loads are in flight together; through the function every load is waited for inside its branch (0.711 ms against 0.698 ms, the same
// registers: profiles/eval_steps_refactor_ab.txt).
__global__ __launch_bounds__(kMeshScanThreads) void meshcc_scan_kernel(const MeshKeepScan p) {
  __shared__ int wsum[1][kMeshScanThreads / 64];
  __shared__ int carry[1];
  const unsigned char* keep = blockIdx.x ? p.keep_face : p.keep_vertex;
  int* map = blockIdx.x ? p.face_map : p.vertex_map;
  const long n = blockIdx.x ? p.F : p.V;
  if (threadIdx.x == 0) carry[0] = 0;
  __syncthreads();
  for (long base = 0; base < n; base += kMeshScanChunk) {
    const long i0 = base + (long)threadIdx.x * kMeshScanPer;
    unsigned char k[kMeshScanPer];
    int x[1] = {0};
#pragma unroll
    for (int j = 0; j < kMeshScanPer; ++j) { k[j] = i0 + j < n ? keep[i0 + j] : 0; x[0] += k[j]; }
    int excl[1];
    block_excl_scan<kMeshScanThreads / 64, 1, int>(x, excl, wsum, carry);
    int at = excl[0];
#pragma unroll
    for (int j = 0; j < kMeshScanPer; ++j) { if (i0 + j < n) map[i0 + j] = k[j] ? at : -1; at += k[j]; }
  }
  if (threadIdx.x == 0) p.totals[blockIdx.x] = carry[0];
}

void mesh_keep_scan(const MeshKeepScan& p, cnr_stream s) {
  const long n = p.V > p.F ? p.V : p.F;
  TimingScope ts_("meshcc_scan_kernel", 2, 0, n, 0, 0, 0, s, 5.0 * ((double)p.V + (double)p.F) + 8.0);
  hipLaunchKernelGGL(meshcc_scan_kernel, dim3(2), dim3(kMeshScanThreads), 0, s, p);
}

void be_mesh_select(const MeshSelect& p, cnr_stream s) {
  const double V = (double)p.V, F = (double)p.F;
  const long n = p.V > p.F ? p.V : p.F;
  if (n > 0) {
    TimingScope ts_("meshcc_keep_kernel", 2, 0, n, 0, 0, 0, s, 9.0 * V + 21.0 * F);
    hipLaunchKernelGGL(meshcc_keep_kernel, dim3((unsigned)((n + kMeshThreads - 1) / kMeshThreads)), dim3(kMeshThreads), 0, s, p);
  }
  mesh_keep_scan({p.keep_vertex, p.keep_face, p.V, p.F, p.vertex_map, p.face_map, p.totals}, s);
  CNR_LAUNCH_CHECK("mesh_select");
}

__global__ __launch_bounds__(kMeshThreads) void meshcc_compact_kernel(const MeshCompact p) {
  const long i = (long)blockIdx.x * kMeshThreads + threadIdx.x;
  if (i < p.V) meshcc_compact_vertex(p, i);
  if (i < p.F) meshcc_compact_face(p, i);
}

void be_mesh_compact(const MeshCompact& p, cnr_stream s) {
  const long n = p.V > p.F ? p.V : p.F;
  if (n > 0) {
    TimingScope ts_("meshcc_compact_kernel", 2, 0, n, 0, 0, 0, s, (p.colors ? 52.0 : 28.0) * (double)p.V + 40.0 * (double)p.F);
    hipLaunchKernelGGL(meshcc_compact_kernel, dim3((unsigned)((n + kMeshThreads - 1) / kMeshThreads)), dim3(kMeshThreads), 0, s, p);
  }
  CNR_LAUNCH_CHECK("mesh_compact");
}

}  // namespace cnr
