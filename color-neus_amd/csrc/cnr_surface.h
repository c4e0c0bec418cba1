// Mesh surface sampling and exact point-to-mesh distance (cnr_mesh_area_cdf / cnr_mesh_sample / cnr_point_mesh_distance): descriptors,
// launches and the per-element arithmetic the HIP kernels (cnr_surface.hip) and the CPU emulation (cnr_kernels_emu.cpp) share.
// include/colorneus_render.h states the rules for the caller; every float operation below is one separately rounded fp32 operation in the
// written order (the build passes -ffp-contract=off: no FMA), everything else is integer work, so both builds give the same bits.
#pragma once
#include "cnr_common.h"
#include "cnr_meshcc.h"   // meshcc_valid, the single-workgroup scan's shape
#include "cnr_nn.h"       // nn_dist2, nn_update, nn_key, nn_unpack
#include "cnr_philox.h"

namespace cnr {

struct MeshAreaCdf {
  const float* vertices; long V;        // [V][3]
  const int* triangles; long F;         // [F][3], 0 < F < 2^31
  unsigned long long* cdf;              // [F]: the faces' area bits (or kSurfInvalid) between the two launches, then the prefix sums
  long long* summary;                   // [4] = {total, faces of weight 0, invalid faces, bits of amax}
};
void be_mesh_area_cdf(const MeshAreaCdf& p, cnr_stream s);

struct MeshSample {
  const float* vertices; long V; const int* triangles; long F;
  const unsigned long long* cdf;        // [F]
  long n; unsigned seed_lo, seed_hi;
  float* points; int* faces; float* bary /* or null */;   // [n][3], [n], [n][2]
};
void be_mesh_sample(const MeshSample& p, cnr_stream s);

struct PointMeshDist {
  const float* query; long n;           // [n][3]
  const float* vertices; long V; const int* triangles; long F;   // 0 < F < 2^31
  float* dist2; int* face; float* closest /* or null */;         // [n], [n], [n][3]
  unsigned long long* keys;             // [n] scratch
};
void be_point_mesh_distance(const PointMeshDist& p, cnr_stream s);

// ---- sampling weights --------------------------------------------------------------------------------------------------------------------
constexpr unsigned long long kSurfInvalid = ~0ull;   // in cdf[] between the launches: a face with an index outside [0, V) or a non-finite area
// the doubled area of face f as its bit pattern (a non-negative float orders like its bits), kSurfInvalid for an invalid face
CNR_HD unsigned long long surf_area_bits(const MeshAreaCdf& p, long f) {
  const int* t = p.triangles + f * 3;
  if (!meshcc_valid(t, p.V)) return kSurfInvalid;
  const float* a = p.vertices + (long)t[0] * 3;
  const float* b = p.vertices + (long)t[1] * 3;
  const float* c = p.vertices + (long)t[2] * 3;
  const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
  const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
  const float nx = (e1y * e2z) - (e1z * e2y), ny = (e1z * e2x) - (e1x * e2z), nz = (e1x * e2y) - (e1y * e2x);
  const float A = sqrtf((nx * nx + ny * ny) + nz * nz);
  if (!(A <= 3.4028234663852886e38f)) return kSurfInvalid;   // NaN or +inf
  unsigned bits;
  memcpy(&bits, &A, sizeof bits);
  return bits;
}
// the integer weight of a face from its area bits and the bits of the largest area: trunc((A / amax) * 2^32), 0 for an invalid face and when amax == 0
CNR_HD unsigned long long surf_weight(unsigned long long area_bits, unsigned amax_bits) {
  if (area_bits == kSurfInvalid) return 0ull;
  const unsigned ab = (unsigned)area_bits;
  float A, amax;
  memcpy(&A, &ab, sizeof A);
  memcpy(&amax, &amax_bits, sizeof amax);
  if (!(amax > 0.0f)) return 0ull;
  return (unsigned long long)((A / amax) * 4294967296.0f);   // A <= amax: at most 2^32
}

// ---- one sample --------------------------------------------------------------------------------------------------------------------------
// sample i of the draw: Philox words of the counter (lo32(i), hi32(i), 0, 0) under the seed; face = the first f with cdf[f] > mulhi64(w0:w1, total);
// (u, v) = the top 24 bits of w2 / w3, folded into the triangle in integers (iu + iv > 2^24  <=>  u + v > 1: iu = 2^24 - iu, iv = 2^24 - iv);
// point = (a + u * e1) + v * e2.  total == 0 (or a cdf that names an invalid face): face -1, NaN everywhere.
CNR_HD void surf_sample(const MeshSample& p, long i) {
  unsigned w[4];
  pix_philox((unsigned)((unsigned long long)i & 0xffffffffull), (unsigned)((unsigned long long)i >> 32), 0u, 0u, p.seed_lo, p.seed_hi, w);
  const unsigned long long total = p.cdf[p.F - 1];
  const float nan = __builtin_nanf("");
  int face = -1;
  float u = nan, v = nan, px = nan, py = nan, pz = nan;
  if (total > 0ull) {
    const unsigned long long r = pix_mulhi64(((unsigned long long)w[0] << 32) | w[1], total);   // < total = cdf[F - 1]
    long lo = 0, hi = p.F - 1;
    while (lo < hi) {
      const long mid = (lo + hi) >> 1;
      if (p.cdf[mid] > r) hi = mid; else lo = mid + 1;
    }
    const int* t = p.triangles + lo * 3;
    if (meshcc_valid(t, p.V)) {
      face = (int)lo;
      unsigned iu = w[2] >> 8, iv = w[3] >> 8;
      if (iu + iv > 0x1000000u) { iu = 0x1000000u - iu; iv = 0x1000000u - iv; }
      u = (float)iu * 0x1p-24f; v = (float)iv * 0x1p-24f;
      const float* a = p.vertices + (long)t[0] * 3;
      const float* b = p.vertices + (long)t[1] * 3;
      const float* c = p.vertices + (long)t[2] * 3;
      px = (a[0] + u * (b[0] - a[0])) + v * (c[0] - a[0]);
      py = (a[1] + u * (b[1] - a[1])) + v * (c[1] - a[1]);
      pz = (a[2] + u * (b[2] - a[2])) + v * (c[2] - a[2]);
    }
  }
  p.faces[i] = face;
  p.points[i * 3] = px; p.points[i * 3 + 1] = py; p.points[i * 3 + 2] = pz;
  if (p.bary) { p.bary[i * 2] = u; p.bary[i * 2 + 1] = v; }
}

// ---- the closest point of a triangle -------------------------------------------------------------------------------------------------------
// what is precomputed per triangle (the HIP kernel stages these records in LDS): a, ab = b - a, ac = c - a and their three dot products,
// each dot product (x*x' + y*y') + z*z'.  A face with an index outside [0, V) gives a record of NaNs: its distances are NaN and never win.
struct alignas(16) SurfTri {
  float ax, ay, az, abx, aby, abz, acx, acy, acz, abab, abac, acac;
};
CNR_HD SurfTri surf_record(const float* vertices, long V, const int* t) {
  SurfTri r;
  if (!meshcc_valid(t, V)) {
    const float nan = __builtin_nanf("");
    r.ax = r.ay = r.az = r.abx = r.aby = r.abz = r.acx = r.acy = r.acz = r.abab = r.abac = r.acac = nan;
    return r;
  }
  const float* a = vertices + (long)t[0] * 3;
  const float* b = vertices + (long)t[1] * 3;
  const float* c = vertices + (long)t[2] * 3;
  r.ax = a[0]; r.ay = a[1]; r.az = a[2];
  r.abx = b[0] - a[0]; r.aby = b[1] - a[1]; r.abz = b[2] - a[2];
  r.acx = c[0] - a[0]; r.acy = c[1] - a[1]; r.acz = c[2] - a[2];
  r.abab = (r.abx * r.abx + r.aby * r.aby) + r.abz * r.abz;
  r.abac = (r.abx * r.acx + r.aby * r.acy) + r.abz * r.acz;
  r.acac = (r.acx * r.acx + r.acy * r.acy) + r.acz * r.acz;
  return r;
}
// The closest point of the closed triangle to q, by the region classification of Ericson (Real-Time Collision Detection, 5.1.5) on
//   ap = q - a;  d1 = ab.ap, d2 = ac.ap;  d3 = d1 - abab, d4 = d2 - abac  (= ab.bp, ac.bp);  d5 = d1 - abac, d6 = d2 - acac  (= ab.cp, ac.cp)
//   vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4;  e43 = d4 - d3, e56 = d5 - d6
// The first region that holds, in this order, sets (n1, n2, den); then inv = 1 / den, v = n1 * inv, w = n2 * inv and
// closest = (a + v * ab) + w * ac per component:
//   vertex a   d1 <= 0 and d2 <= 0                       (0, 0, 1)
//   vertex b   d3 >= 0 and d4 <= d3                      (1, 0, 1)
//   edge ab    vc <= 0 and d1 >= 0 and d3 <= 0           (d1, 0, d1 - d3)
//   vertex c   d6 >= 0 and d5 <= d6                      (0, 1, 1)
//   edge ac    vb <= 0 and d2 >= 0 and d6 <= 0           (0, d2, d2 - d6)
//   edge bc    va <= 0 and e43 >= 0 and e56 >= 0         (e56, e43, e43 + e56)
//   interior   otherwise                                 (vb, vc, (va + vb) + vc)
// Written as selects from the last region to the first (lanes of a wave see the same triangle from different regions).  A triangle collapsed
// to a point is "vertex a" for every q; any other degenerate triangle may reach den == 0, a non-finite point and so a distance that never wins.
CNR_HD void surf_closest(const SurfTri& t, float qx, float qy, float qz, float* cx, float* cy, float* cz) {
  const float apx = qx - t.ax, apy = qy - t.ay, apz = qz - t.az;
  const float d1 = (t.abx * apx + t.aby * apy) + t.abz * apz;
  const float d2 = (t.acx * apx + t.acy * apy) + t.acz * apz;
  const float d3 = d1 - t.abab, d4 = d2 - t.abac, d5 = d1 - t.abac, d6 = d2 - t.acac;
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  float n1 = vb, n2 = vc, den = (va + vb) + vc;
  const bool bc = va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f;
  n1 = bc ? e56 : n1; n2 = bc ? e43 : n2; den = bc ? e43 + e56 : den;
  const bool ac = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
  n1 = ac ? 0.0f : n1; n2 = ac ? d2 : n2; den = ac ? d2 - d6 : den;
  const bool vxc = d6 >= 0.0f && d5 <= d6;
  n1 = vxc ? 0.0f : n1; n2 = vxc ? 1.0f : n2; den = vxc ? 1.0f : den;
  const bool ab = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
  n1 = ab ? d1 : n1; n2 = ab ? 0.0f : n2; den = ab ? d1 - d3 : den;
  const bool vxb = d3 >= 0.0f && d4 <= d3;
  n1 = vxb ? 1.0f : n1; n2 = vxb ? 0.0f : n2; den = vxb ? 1.0f : den;
  const bool vxa = d1 <= 0.0f && d2 <= 0.0f;
  n1 = vxa ? 0.0f : n1; n2 = vxa ? 0.0f : n2; den = vxa ? 1.0f : den;
  const float inv = 1.0f / den;
  const float v = n1 * inv, w = n2 * inv;
  *cx = (t.ax + v * t.abx) + w * t.acx;
  *cy = (t.ay + v * t.aby) + w * t.acy;
  *cz = (t.az + v * t.abz) + w * t.acz;
}
// the candidate of one (query, face) pair: d2 = nn_dist2(q, closest); the scan over ascending faces keeps the first minimum (nn_update:
// a strictly smaller d2 wins from +inf on, so a NaN or +inf d2 never wins)
CNR_HD float surf_dist2(const SurfTri& t, float qx, float qy, float qz) {
  float cx, cy, cz;
  surf_closest(t, qx, qy, qz, &cx, &cy, &cz);
  return nn_dist2(qx, qy, qz, cx, cy, cz);
}
// keys[i] -> dist2 / face (nn_unpack: no candidate = {NaN, -1}) and, when wanted, the closest point on that face, recomputed by the same function
CNR_HD void surf_finish(const PointMeshDist& p, long i) {
  nn_unpack(p.keys[i], &p.dist2[i], &p.face[i]);
  if (!p.closest) return;
  const float nan = __builtin_nanf("");
  float cx = nan, cy = nan, cz = nan;
  const int f = p.face[i];
  if (f >= 0) surf_closest(surf_record(p.vertices, p.V, p.triangles + (long)f * 3), p.query[i * 3], p.query[i * 3 + 1], p.query[i * 3 + 2], &cx, &cy, &cz);
  p.closest[i * 3] = cx; p.closest[i * 3 + 1] = cy; p.closest[i * 3 + 2] = cz;
}

}  // namespace cnr
