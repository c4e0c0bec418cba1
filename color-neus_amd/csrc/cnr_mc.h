// Marching cubes: what one voxel emits, shared by the HIP kernel (mc_emit_kernel, cnr_mc.hip) and its emulation twin.  Includes the triangle table: a translation
// unit that wants it in constant memory defines CNR_MC_QUAL first.
#pragma once
#include "cnr_backend.h"
#include "cnr_mc_table.h"

namespace cnr {

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
