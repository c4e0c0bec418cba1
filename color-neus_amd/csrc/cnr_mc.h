// Marching cubes: what one voxel emits, shared by the HIP kernel (mc_emit_kernel, cnr_mc.hip) and its emulation twin.  Includes the triangle table: a translation
// unit that wants it in constant memory defines CNR_MC_QUAL first.
#pragma once
#include "cnr_common.h"
#include "cnr_mc_table.h"

namespace cnr {

// ---- iso-surface extraction on the device-resident SDF lattice (replaces the CPU mcubes.marching_cubes call of extract_geometry,
// NeuS.py:31-40): cell classification + edge ownership, two exclusive scans, vertex / triangle emission
struct McVolume {
  const float* u; int res; float thr;      // u[x][y][z], surface where u crosses thr, "inside" = u > thr
  unsigned char* flags;                    // [res^3] bit a: the edge from this voxel along +axis a crosses the level
  int* counts;                             // [res^3][2] -> exclusive offsets {vertex, triangle} after mc_scan
  int* block_sums;                         // [nblocks][2]
  int* totals;                             // [2] device: number of vertices, number of triangles
};
constexpr int kMcScanBlock = 2048;
void be_mc_count(const McVolume& v, cnr_stream s);    // flags + per-voxel {vertex, triangle} counts, scanned into offsets; totals written
void be_mc_emit(const McVolume& v, const float* bmin, const float* bmax, float* verts, int* tris, cnr_stream s);
// shared per-voxel logic (host + device)
CNR_HD int mc_cell(const float* u, int res, float thr, int x, int y, int z, unsigned char* flags_out) {   // returns the cube index or -1 (no cell)
  const long r2 = (long)res * res, v = ((long)x * res + y) * res + z;
  const bool f0 = u[v] > thr;
  unsigned char fl = 0;
  if (x + 1 < res && (u[v + r2] > thr) != f0) fl |= 1;
  if (y + 1 < res && (u[v + res] > thr) != f0) fl |= 2;
  if (z + 1 < res && (u[v + 1] > thr) != f0) fl |= 4;
  *flags_out = fl;
  if (x + 1 >= res || y + 1 >= res || z + 1 >= res) return -1;
  int idx = 0;
  for (int c = 0; c < 8; ++c) {
    const long vc = v + (c & 1) * r2 + ((c >> 1) & 1) * res + ((c >> 2) & 1);
    idx |= (u[vc] > thr ? 1 : 0) << c;
  }
  return idx;
}
CNR_HD int mc_popcount3(unsigned x) { return (int)((x & 1) + ((x >> 1) & 1) + ((x >> 2) & 1)); }

// voxel v of the scanned volume (McVolume::counts holds the exclusive offsets): the vertices on the (up to three) level-crossing edges it owns, and the
// triangles of its cell as indices of the vertices on the cell's edges, each owned by the voxel at the edge's lower end
// (CNR_D, not CNR_HD: a host-callable function that names the static __constant__ tables makes the compiler export them, and the kernel then
// reaches them through the global offset table inside its voxel loop instead of pc-relative: mc_emit measured 4 % slower that way)
CNR_D void mc_emit_voxel(const McVolume& m, long v, const float* bmin, const float* bmax, float* verts, int* tris) {
  const int res = m.res;
  const long r2 = (long)res * res;
  const long stride[3] = {r2, (long)res, 1};
  const unsigned fl = m.flags[v];
  const int xyz[3] = {(int)(v / r2), (int)((v / res) % res), (int)(v % res)};
  if (fl) {
    int k = m.counts[v * 2];
    const float u0 = m.u[v];
    for (int a = 0; a < 3; ++a) {
      if (!((fl >> a) & 1)) continue;
      const float u1 = m.u[v + stride[a]];
      const float t = (m.thr - u0) / (u1 - u0);
      for (int c = 0; c < 3; ++c) {
        const float g = (float)xyz[c] + (c == a ? t : 0.0f);      // lattice index coordinates, like mcubes' vertices
        verts[(long)k * 3 + c] = g / ((float)res - 1.0f) * (bmax[c] - bmin[c]) + bmin[c];   // NeuS.py:36-39
      }
      ++k;
    }
  }
  if (xyz[0] + 1 >= res || xyz[1] + 1 >= res || xyz[2] + 1 >= res) return;   // no cell
  int idx = 0;       // the cube index as mc_cell forms it, without the edge flags (the kernel is 2 VGPRs and 27 instructions shorter than through mc_cell)
  for (int c = 0; c < 8; ++c) idx |= (m.u[v + (c & 1) * r2 + ((c >> 1) & 1) * res + ((c >> 2) & 1)] > m.thr ? 1 : 0) << c;
  const int nt = kMcNumTris[idx];
  const int t0 = m.counts[v * 2 + 1];
  for (int t = 0; t < nt; ++t) {
    for (int q = 0; q < 3; ++q) {
      const int ed = kMcTris[idx][t * 3 + q], a = ed >> 2, kk = ed & 3;
      const int o0 = a == 0 ? 1 : 0, o1 = a == 2 ? 1 : 2;       // the two other axes in increasing order
      const long vo = v + (kk & 1) * stride[o0] + (kk >> 1) * stride[o1];
      tris[(long)(t0 + t) * 3 + q] = m.counts[vo * 2] + mc_popcount3(m.flags[vo] & ((1u << a) - 1u));
    }
  }
}

}  // namespace cnr
