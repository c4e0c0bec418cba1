// Mesh rasteriser (cnr_mesh_raster): the per-element arithmetic the HIP kernels (cnr_raster.hip) and the CPU emulation (cnr_kernels_emu.cpp)
// share.  The arithmetic is specified in include/colorneus_render.h; every float operation below is a separately rounded fp32 operation in
// the order written (the build passes -ffp-contract=off) and every integer operation is exact, so both builds give the same bits per pixel.
#pragma once
#include "cnr_common.h"

namespace cnr {

constexpr int CNR_RASTER_SMALL = 8;   // a triangle whose clipped box has at most this many pixels on a side is drawn by the lane that set it up
constexpr unsigned long long kRasterNoKey = ~0ull;   // "no triangle": above every key
constexpr float kRasterMaxUV = 2097152.0f;           // 2^21: |u|, |v| below it, so X, Y fit 30 bits and every product of two differences 62

struct RasterVert { int X, Y; float z; };   // 1/256-pixel fixed point and the camera depth; z = NaN: not usable

struct MeshRaster {
  const float* vertices; long V;        // [V][3]
  const int* triangles; long F;         // [F][3]
  const float* colors;                  // [V][3] or null
  const float* c2w; const float* focal; const float* origin;   // device [4][4], [2], [3] or null
  float radius, z_near; int H, W, opengl;
  float background[3];
  float* rgb; float* depth; int* tri_id; int* dropped;   // [H][W][3] or null, [H][W], [H][W], [2]
  RasterVert* pv;                       // [V] scratch
  unsigned long long* keys;             // [H*W] scratch
  int* large;                           // [F] scratch: the triangles the small-triangle launch left to the large one
  int* n_large;                         // [1] scratch
};
void be_mesh_raster(const MeshRaster& p, cnr_stream s);

// the camera of a call: R = c2w[:3,:3], t = (c2w[:3,3] - origin) / radius (as cnr_gen_rays normalises the ray origin; origin null: c2w[:3,3])
// (raster_cam_of: from the arrays of one view, for the callers that hold a stack of views -- cnr_mesh_view_votes, cnr_cull.h)
struct RasterCam { float R[9], t[3], fx, fy, cx, cy; };
CNR_HD RasterCam raster_cam_of(const float* c2w, const float* focal, const float* origin, float radius, int H, int W) {
  RasterCam c;
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) c.R[r * 3 + k] = c2w[r * 4 + k];
    c.t[r] = origin ? (c2w[r * 4 + 3] - origin[r]) / radius : c2w[r * 4 + 3];
  }
  c.fx = focal[0]; c.fy = focal[1];
  c.cx = (float)W * 0.5f; c.cy = (float)H * 0.5f;
  return c;
}
CNR_HD RasterCam raster_cam(const MeshRaster& p) { return raster_cam_of(p.c2w, p.focal, p.origin, p.radius, p.H, p.W); }

// vertex stage: camera frame by R^T (p - t), pinhole projection (the inverse of get_rays_at), snap to 1/256 pixel (round half to even)
CNR_HD RasterVert raster_project(const RasterCam& c, const float* v, int opengl, float z_near) {
  const float d0 = v[0] - c.t[0], d1 = v[1] - c.t[1], d2 = v[2] - c.t[2];
  const float xc = (c.R[0] * d0 + c.R[3] * d1) + c.R[6] * d2;
  float yc = (c.R[1] * d0 + c.R[4] * d1) + c.R[7] * d2;
  float zc = (c.R[2] * d0 + c.R[5] * d1) + c.R[8] * d2;
  if (opengl) { yc = -yc; zc = -zc; }
  const float u = (c.fx * xc) / zc + c.cx, w = (c.fy * yc) / zc + c.cy;
  RasterVert o;
  o.X = 0; o.Y = 0; o.z = __builtin_nanf("");
  if (zc > z_near && fabsf(u) < kRasterMaxUV && fabsf(w) < kRasterMaxUV) {   // a NaN fails every comparison
    o.X = (int)rintf(u * 256.0f); o.Y = (int)rintf(w * 256.0f); o.z = zc;
  }
  return o;
}

// triangle stage.  status: 0 to draw, 1 a vertex not usable (dropped[0]), 2 an index outside [0, V) (dropped[1]), 3 nothing to draw
// (zero area or no pixel inside the clipped box).  After a swap (A < 0) v[1] / v[2] and idx[1] / idx[2] are the swapped ones.
struct RasterTri {
  int status;
  int idx[3];
  RasterVert v[3];
  long long A;
  int i0, i1, j0, j1;      // clipped box, columns [i0, i1] x rows [j0, j1]
};
CNR_HD int raster_floor256(int x) { return x >> 8; }   // (arithmetic shift: floor for negative x)
CNR_HD RasterTri raster_setup(const int* tri, long V, const RasterVert* pv, int H, int W) {
  RasterTri t;
  t.status = 0; t.A = 0; t.i0 = t.j0 = 0; t.i1 = t.j1 = -1;
  for (int k = 0; k < 3; ++k) {
    t.idx[k] = tri[k];
    if (t.idx[k] < 0 || (long)t.idx[k] >= V) t.status = 2;
  }
  if (t.status) return t;
  for (int k = 0; k < 3; ++k) {
    t.v[k] = pv[t.idx[k]];
    if (!(t.v[k].z == t.v[k].z)) t.status = 1;
  }
  if (t.status) return t;
  t.A = (long long)(t.v[1].X - t.v[0].X) * (t.v[2].Y - t.v[0].Y) - (long long)(t.v[1].Y - t.v[0].Y) * (t.v[2].X - t.v[0].X);
  if (t.A == 0) { t.status = 3; return t; }
  if (t.A < 0) {
    const RasterVert v = t.v[1]; t.v[1] = t.v[2]; t.v[2] = v;
    const int i = t.idx[1]; t.idx[1] = t.idx[2]; t.idx[2] = i;
    t.A = -t.A;
  }
  int x0 = t.v[0].X, x1 = x0, y0 = t.v[0].Y, y1 = y0;
  for (int k = 1; k < 3; ++k) {
    x0 = t.v[k].X < x0 ? t.v[k].X : x0; x1 = t.v[k].X > x1 ? t.v[k].X : x1;
    y0 = t.v[k].Y < y0 ? t.v[k].Y : y0; y1 = t.v[k].Y > y1 ? t.v[k].Y : y1;
  }
  t.i0 = raster_floor256(x0 + 255); t.i1 = raster_floor256(x1);     // pixels i with x0 <= 256 i <= x1
  t.j0 = raster_floor256(y0 + 255); t.j1 = raster_floor256(y1);
  t.i0 = t.i0 < 0 ? 0 : t.i0; t.i1 = t.i1 > W - 1 ? W - 1 : t.i1;
  t.j0 = t.j0 < 0 ? 0 : t.j0; t.j1 = t.j1 > H - 1 ? H - 1 : t.j1;
  if (t.i0 > t.i1 || t.j0 > t.j1) t.status = 3;
  return t;
}
CNR_HD bool raster_is_small(const RasterTri& t) { return t.i1 - t.i0 < CNR_RASTER_SMALL && t.j1 - t.j0 < CNR_RASTER_SMALL; }

// edge functions E0 (edge 1 -> 2), E1 (2 -> 0), E2 (0 -> 1) at pixel (i, j) of the triangle's box: exact (|256 i - X| <= 2^30 inside the box)
CNR_HD long long raster_edge(const RasterVert& p, const RasterVert& q, int i, int j) {
  return (long long)(q.X - p.X) * ((long long)j * 256 - p.Y) - (long long)(q.Y - p.Y) * ((long long)i * 256 - p.X);
}
// coverage: all three edge functions >= 0 (edges inclusive, no top-left rule: the depth key decides the owner of a shared edge)
struct RasterEdges { long long E[3]; bool covered; };
CNR_HD RasterEdges raster_edges(const RasterTri& t, int i, int j) {
  RasterEdges e;
  e.E[0] = raster_edge(t.v[1], t.v[2], i, j); e.E[1] = raster_edge(t.v[2], t.v[0], i, j); e.E[2] = raster_edge(t.v[0], t.v[1], i, j);
  e.covered = e.E[0] >= 0 && e.E[1] >= 0 && e.E[2] >= 0;
  return e;
}
// of a covered pixel: the three terms q_k = b_k / z_k, b_k = (float)E_k / (float)A, and s = (q0 + q1) + q2
struct RasterHit { float q[3], s; };
CNR_HD RasterHit raster_hit(const RasterTri& t, const RasterEdges& e) {
  RasterHit h;
  const float A = (float)t.A;
  for (int k = 0; k < 3; ++k) h.q[k] = ((float)e.E[k] / A) / t.v[k].z;
  h.s = (h.q[0] + h.q[1]) + h.q[2];
  return h;
}
// the z-buffer key of a covered pixel, or kRasterNoKey for a depth that is not > 0
CNR_HD unsigned long long raster_key(const RasterHit& h, int tri) {
  const float depth = 1.0f / h.s;
  if (!(depth > 0.0f)) return kRasterNoKey;
  unsigned bits;
  memcpy(&bits, &depth, sizeof bits);
  return ((unsigned long long)bits << 32) | (unsigned)tri;
}
CNR_HD unsigned long long raster_pixel_key(const RasterTri& t, int tri, int i, int j) {
  const RasterEdges e = raster_edges(t, i, j);
  return e.covered ? raster_key(raster_hit(t, e), tri) : kRasterNoKey;
}

// resolve of pixel (i, j): decode the key, recompute the winner's coverage terms from the same integers, interpolate the colours
CNR_HD void raster_resolve(const MeshRaster& p, int i, int j) {
  const long at = (long)j * p.W + i;
  const unsigned long long key = p.keys[at];
  if (key == kRasterNoKey) {
    p.tri_id[at] = -1;
    p.depth[at] = __builtin_nanf("");
    if (p.rgb) for (int c = 0; c < 3; ++c) p.rgb[at * 3 + c] = p.background[c];
    return;
  }
  const int tri = (int)(unsigned)(key & 0xffffffffull);
  const unsigned bits = (unsigned)(key >> 32);
  float depth;
  memcpy(&depth, &bits, sizeof depth);
  p.tri_id[at] = tri;
  p.depth[at] = depth;
  if (!p.rgb) return;
  const RasterTri t = raster_setup(p.triangles + (long)tri * 3, p.V, p.pv, p.H, p.W);
  const RasterHit h = raster_hit(t, raster_edges(t, i, j));
  const float w0 = h.q[0] / h.s, w1 = h.q[1] / h.s, w2 = h.q[2] / h.s;
  const float* c0 = p.colors + (long)t.idx[0] * 3; const float* c1 = p.colors + (long)t.idx[1] * 3; const float* c2 = p.colors + (long)t.idx[2] * 3;
  for (int c = 0; c < 3; ++c) p.rgb[at * 3 + c] = (w0 * c0[c] + w1 * c1[c]) + w2 * c2[c];
}

}  // namespace cnr
