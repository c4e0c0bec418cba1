// Mesh connected components, selection and compaction (cnr_mesh_components / cnr_mesh_select / cnr_mesh_compact): the per-element code the HIP
// kernels (cnr_meshcc.hip) and the CPU emulation (cnr_kernels_emu.cpp) share.  Everything here is integer work and exact: both builds, any
// launch order and any face order give the same bits.
//
// Definitions (the contract; include/colorneus_render.h states them for the caller):
//   * two vertices are connected when a VALID triangle contains both; a triangle is valid when its three indices lie in [0, V)
//   * an invalid triangle connects nothing, belongs to no component, is counted in dropped[0] and is never kept (the rasteriser's status-2 rule)
//   * degenerate (a, a, b) and duplicate triangles are valid; a vertex in no valid triangle is a component of its own with zero faces
//   * labels[v] = the smallest vertex index of v's component
//   * face_count[r] / vertex_count[r] = the component's totals at its root r (labels[r] == r), 0 at every other index; a valid triangle
//     counts for labels[t[0]]
//   * summary = {n_components, n_components_with_faces, largest_label, largest_face_count}: most faces, ties to the lowest label, zero-face
//     vertices are no candidates; without a valid triangle largest_label = -1 and largest_face_count = 0
//
// Storage: only the caller's typed arrays, no scratch.  labels [V] holds the union-find's parent array while cnr_mesh_components runs;
// face_count [V], vertex_count [V], summary [4] (8-byte aligned: summary[2..3] hold the 64-bit selection key until the last launch decodes it),
// dropped [1]; cnr_mesh_select: keep_vertex [V] / keep_face [F] (uint8, 0 or 1), vertex_map [V] / face_map [F] (the new index or -1), totals [2]
// = {V', F'}; cnr_mesh_compact: out_vertices [V'][3], out_colors [V'][3], out_triangles [F'][3].
#pragma once
#include "cnr_common.h"

namespace cnr {

constexpr int CNR_MESH_KEEP_LARGEST = 0, CNR_MESH_KEEP_THRESHOLD = 1;   // cnr_mesh_select's mode
constexpr int kMeshScanThreads = 1024, kMeshScanPer = 8;
constexpr int kMeshScanChunk = kMeshScanThreads * kMeshScanPer;         // elements one trip of the single-workgroup carried scan takes in

struct MeshComponents {
  const int* triangles; long F, V;      // [F][3]
  int* labels; int* face_count; int* vertex_count;   // [V] each
  int* summary; int* dropped;           // [4], [1]
};
void be_mesh_components(const MeshComponents& p, cnr_stream s);

struct MeshSelect {
  const int* triangles; long F, V;
  const int* labels; const int* face_count; const int* summary;
  int mode, min_faces; float min_ratio;
  unsigned char* keep_vertex; unsigned char* keep_face;   // [V], [F]
  int* vertex_map; int* face_map; int* totals;            // [V], [F], [2]
};
void be_mesh_select(const MeshSelect& p, cnr_stream s);

// the keep flags of a selection scanned into the index maps and totals = {V', F'}: the one carried scan (meshcc_scan_kernel) behind
// cnr_mesh_select and cnr_mesh_cull_select (cnr_cull.h)
struct MeshKeepScan {
  const unsigned char* keep_vertex; const unsigned char* keep_face; long V, F;
  int* vertex_map; int* face_map; int* totals;
};
void mesh_keep_scan(const MeshKeepScan& p, cnr_stream s);

struct MeshCompact {
  const float* vertices; const float* colors /* or null */; const int* triangles; long F, V;
  const int* vertex_map; const int* face_map;
  float* out_vertices; float* out_colors /* null iff colors null */; int* out_triangles;
};
void be_mesh_compact(const MeshCompact& p, cnr_stream s);

CNR_HD bool meshcc_valid(const int* t, long V) {
  return t[0] >= 0 && (long)t[0] < V && t[1] >= 0 && (long)t[1] < V && t[2] >= 0 && (long)t[2] < V;
}

// ---- union-find over parent[] = labels[].  A: how an entry is read, stored and hooked -- MeshccPlain below (one thread: the emulation, and the
// flattening launch, which starts after the hooking launch has completed), agent-scope atomics in the hooking launch (cnr_meshcc.hip).
struct MeshccPlain {
  static CNR_HD int load(const int* p) { return *p; }
  static CNR_HD void store(int* p, int x) { *p = x; }
  static CNR_HD bool hook(int* p, int hi, int lo) {
    if (*p != hi) return false;
    *p = lo;
    return true;
  }
};
// The root of v, with path halving.  WHY THIS CANNOT SPIN: a root is only ever hooked under a root with a SMALLER index, and a halving store
// replaces an entry by a grandparent read a moment ago, so at every moment parent[x] names a vertex that is or was an ancestor of x: it lies in
// x's set and parent[x] <= x, with equality only at a root.  Every step of the loop therefore moves to a strictly smaller index: at most v
// steps, whatever other lanes store meanwhile -- also when a racing halving store puts back an older ancestor (the racy stores are benign: any
// of the values leads to the root).  A halving store never touches a root (it is made only after the entry was seen to differ from its index,
// and a hooked entry never becomes a root again), so it cannot undo a hook.
template <class A>
CNR_HD int meshcc_find(int* parent, int v) {
  int p = A::load(parent + v);
  while (p != v) {
    const int g = A::load(parent + p);
    if (g != p) A::store(parent + v, g);
    v = p;
    p = g;
  }
  return v;
}
// Join the sets of a and b: hook the LARGER root under the smaller, so that the final root of a component is its smallest index whatever the
// order of the hooks.  A hook is a compare-and-swap of parent[hi] from hi (still a root) to lo; it fails only when another lane hooked hi
// first.  At most V - 1 hooks succeed in a whole launch and every retry re-finds through loads that see them (A::load), so the retries end.
template <class A>
CNR_HD void meshcc_unite(int* parent, int a, int b) {
  for (;;) {
    a = meshcc_find<A>(parent, a);
    b = meshcc_find<A>(parent, b);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    if (A::hook(parent + hi, hi, lo)) return;
  }
}
// the root of v without a store (the flattening launch: every lane writes only its own entry, and whatever mixture of old and flattened
// entries it reads names ancestors)
CNR_HD int meshcc_root(const int* parent, int v) {
  int p = parent[v];
  while (p != v) { v = p; p = parent[v]; }
  return v;
}

// the selection key of a root with at least one face: more faces win, of equal counts the LOWER label (the idiom of nn_key); 0 = no candidate
CNR_HD unsigned long long meshcc_key(int face_count, int label) {
  return ((unsigned long long)(unsigned)face_count << 32) | (unsigned)(0x7fffffff - label);
}
CNR_HD void meshcc_unkey(unsigned long long key, int* label, int* face_count) {
  *label = key ? 0x7fffffff - (int)(unsigned)(key & 0xffffffffull) : -1;
  *face_count = (int)(unsigned)(key >> 32);
}

// the smallest face count a kept component has in threshold mode: max(min_faces, ceil(min_ratio * largest)), the product and the ceiling in fp32
CNR_HD int meshcc_threshold(int min_faces, float min_ratio, int largest_face_count) {
  const float c = ceilf(min_ratio * (float)largest_face_count);
  const int r = !(c >= 1.0f) ? 0 : (c >= 2147483648.0f ? 0x7fffffff : (int)c);
  return min_faces > r ? min_faces : r;
}
// is the component `label` (with `faces` faces) kept?  Largest mode: the one component summary names; threshold mode: at least `thr` faces
CNR_HD bool meshcc_keep(const MeshSelect& p, int label, int faces, int thr) {
  return p.mode == CNR_MESH_KEEP_LARGEST ? label == p.summary[2] : faces >= thr;
}
// face f: kept iff valid and its component is kept; vertex v: kept iff its component is kept AND has a face (unreferenced vertices go)
CNR_HD unsigned char meshcc_keep_face(const MeshSelect& p, long f, int thr) {
  const int* t = p.triangles + f * 3;
  if (!meshcc_valid(t, p.V)) return 0;
  const int label = p.labels[t[0]];
  return meshcc_keep(p, label, p.face_count[label], thr) ? 1 : 0;
}
CNR_HD unsigned char meshcc_keep_vertex(const MeshSelect& p, long v, int thr) {
  const int label = p.labels[v], faces = p.face_count[label];
  return faces > 0 && meshcc_keep(p, label, faces, thr) ? 1 : 0;
}

// compaction of one vertex / one face through the maps (order preserving: the maps are exclusive scans of the keep flags).  A kept face is
// valid and its vertices are kept (they belong to its component, which has a face); the index check keeps a foreign map from reading outside.
CNR_HD void meshcc_compact_vertex(const MeshCompact& p, long v) {
  const long at = p.vertex_map[v];
  if (at < 0) return;
  for (int c = 0; c < 3; ++c) p.out_vertices[at * 3 + c] = p.vertices[v * 3 + c];
  if (p.colors) for (int c = 0; c < 3; ++c) p.out_colors[at * 3 + c] = p.colors[v * 3 + c];
}
CNR_HD void meshcc_compact_face(const MeshCompact& p, long f) {
  const long at = p.face_map[f];
  const int* t = p.triangles + f * 3;
  if (at < 0 || !meshcc_valid(t, p.V)) return;
  for (int k = 0; k < 3; ++k) p.out_triangles[at * 3 + k] = p.vertex_map[t[k]];
}

}  // namespace cnr
