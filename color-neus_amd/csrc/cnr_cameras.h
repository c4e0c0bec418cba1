// Learnable cameras: descriptors, launches and the per-slot / per-camera bodies both builds share.
#pragma once
#include "cnr_common.h"

namespace cnr {

// ---- learnable cameras (camera_net.py:8-109): the producer of c2w / focal in front of the ray generator
struct Camera {
  const float* r; const float* t;       // [num_cams][6 or 3], [num_cams][3]; null: no pose part
  const float* init_c2w;                // [num_cams][4][4] or null
  const float* fx; const float* fy;     // [1] each; fy null with fx_only; fx null: no focal part
  const long* cam_ids; long B;          // [B] or null: slot i is camera i (B == num_cams)
  int num_cams, six_d, focal_order, fx_only, H, W;
  float* c2w; float* focal;             // [B][4][4] (null: no pose part), [2] (null: no focal part)
};
struct CameraBwd {
  Camera f;                             // the forward arguments (outputs unused)
  const float* d_c2w; const float* d_focal;           // [B][4][4], [2]
  float* d_r; float* d_t; float* d_fx; float* d_fy;   // dense [num_cams][6 or 3], [num_cams][3], [1], [1]; any may be null
};
void be_camera_fwd(const Camera& p, cnr_stream s);
void be_camera_bwd(const CameraBwd& q, cnr_stream s);

// ================================================================================================
// Learnable cameras (Pose_Net / Focal_Net, camera_net.py:8-109): c2w = [[R(r), t], [0 0 0 1]] @ init_c2w and focal from fx / fy, and their
// backward.  A few hundred threads at most: plain per-slot / per-camera code, every operation one rounded fp32 operation in the written order.
// ================================================================================================
constexpr float kCamNormEps = 1e-12f;        // eps of the two normalisations of the 6d form (F.normalize's default)
constexpr float kCamSeriesTheta2 = 1e-4f;    // theta^2 below which the exponential map takes its series (theta < 1e-2: the dropped terms are < 1e-10)

CNR_HD float cam_dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
CNR_HD void cam_cross3(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
// y = x / max(|x|, eps); *len = |x|
CNR_HD void cam_normalize3(const float* x, float* y, float* len) {
  *len = sqrtf(cam_dot3(x, x));
  const float n = fmaxf(*len, kCamNormEps);
  for (int k = 0; k < 3; ++k) y[k] = x[k] / n;
}
// gradient of cam_normalize3: gx = (gy - y (y . gy)) / |x|, or gy / eps where the clamp holds (the norm then has no gradient, as in autograd)
CNR_HD void cam_normalize3_bwd(const float* y, float len, const float* gy, float* gx) {
  if (len >= kCamNormEps) {
    const float yg = cam_dot3(y, gy);
    for (int k = 0; k < 3; ++k) gx[k] = (gy[k] - y[k] * yg) / len;
  } else {
    for (int k = 0; k < 3; ++k) gx[k] = gy[k] / kCamNormEps;
  }
}

// 6d (Zhou et al. 2019; pytorch3d rotation_6d_to_matrix): b1 = normalize(a1), b2 = normalize(a2 - (b1 . a2) b1), b3 = b1 x b2 are the ROWS of R
struct Rot6d { float b1[3], b2[3], l1, l2, d; };
CNR_HD void rot6d_fwd(const float* a, float* R, Rot6d& w) {
  cam_normalize3(a, w.b1, &w.l1);
  w.d = cam_dot3(w.b1, a + 3);
  float u[3];
  for (int k = 0; k < 3; ++k) u[k] = a[3 + k] - w.d * w.b1[k];
  cam_normalize3(u, w.b2, &w.l2);
  cam_cross3(w.b1, w.b2, R + 6);
  for (int k = 0; k < 3; ++k) { R[k] = w.b1[k]; R[3 + k] = w.b2[k]; }
}
CNR_HD void rot6d_bwd(const float* a, const Rot6d& w, const float* G /* d R [3][3] */, float* da /* [6] */) {
  float gb1[3], gb2[3], t[3], gu[3];
  cam_cross3(w.b2, G + 6, t);                       // b3 = b1 x b2: d b1 += b2 x g3, d b2 += g3 x b1
  for (int k = 0; k < 3; ++k) gb1[k] = G[k] + t[k];
  cam_cross3(G + 6, w.b1, t);
  for (int k = 0; k < 3; ++k) gb2[k] = G[3 + k] + t[k];
  cam_normalize3_bwd(w.b2, w.l2, gb2, gu);
  const float b1gu = cam_dot3(w.b1, gu);            // u = a2 - (b1 . a2) b1
  for (int k = 0; k < 3; ++k) {
    da[3 + k] = gu[k] - w.b1[k] * b1gu;
    gb1[k] = gb1[k] - (w.d * gu[k] + b1gu * a[3 + k]);
  }
  cam_normalize3_bwd(w.b1, w.l1, gb1, da);
}

// 3d (axis-angle): R = I + A K + B K^2, K = [r]x, K^2 = r r^T - x I, x = theta^2 = r . r; A = sin(theta) / theta, B = 2 sin^2(theta / 2) / x
// (the half-angle form: 1 - cos(theta) loses digits at small angles), A2 = dA/dx = (cos(theta) - A) / (2x), B2 = dB/dx = (A - 2B) / (2x);
// below kCamSeriesTheta2 the series A = 1 - x/6, B = 1/2 - x/24 (and the derivatives of the full series to the same order), finite at r = 0
struct ExpMap { float x, A, B, A2, B2; };
CNR_HD ExpMap expmap_coef(const float* r) {
  ExpMap e;
  e.x = cam_dot3(r, r);
  if (e.x < kCamSeriesTheta2) {
    e.A = 1.0f - e.x / 6.0f;
    e.B = 0.5f - e.x / 24.0f;
    e.A2 = -1.0f / 6.0f + e.x / 60.0f;
    e.B2 = -1.0f / 24.0f + e.x / 360.0f;
  } else {
    const float th = sqrtf(e.x);
    const float h = sinf(0.5f * th);
    e.A = sinf(th) / th;
    e.B = 2.0f * h * h / e.x;
    e.A2 = (cosf(th) - e.A) / (2.0f * e.x);
    e.B2 = (e.A - 2.0f * e.B) / (2.0f * e.x);
  }
  return e;
}
CNR_HD void expmap_fwd(const float* r, float* R) {
  const ExpMap e = expmap_coef(r);
  const float xx = r[0] * r[0], yy = r[1] * r[1], zz = r[2] * r[2];
  R[0] = 1.0f - e.B * (yy + zz); R[4] = 1.0f - e.B * (xx + zz); R[8] = 1.0f - e.B * (xx + yy);
  const float xy = e.B * (r[0] * r[1]), xz = e.B * (r[0] * r[2]), yz = e.B * (r[1] * r[2]);
  R[1] = xy - e.A * r[2]; R[3] = xy + e.A * r[2];
  R[2] = xz + e.A * r[1]; R[6] = xz - e.A * r[1];
  R[5] = yz - e.A * r[0]; R[7] = yz + e.A * r[0];
}
CNR_HD void expmap_bwd(const float* r, const float* G /* d R [3][3] */, float* dr /* [3] */) {
  const ExpMap e = expmap_coef(r);
  const float v[3] = {G[7] - G[5], G[2] - G[6], G[3] - G[1]};   // <G, [e_k]x>
  const float gK = cam_dot3(r, v);                              // <G, K>
  const float tr = (G[0] + G[4]) + G[8];
  float Gr[3], Gtr[3];                                          // G r, G^T r
  for (int k = 0; k < 3; ++k) { Gr[k] = cam_dot3(G + 3 * k, r); Gtr[k] = (G[k] * r[0] + G[3 + k] * r[1]) + G[6 + k] * r[2]; }
  const float gK2 = cam_dot3(r, Gr) - e.x * tr;                 // <G, K^2>
  for (int k = 0; k < 3; ++k)
    dr[k] = (e.A * v[k] + 2.0f * r[k] * (e.A2 * gK + e.B2 * gK2)) + e.B * ((Gr[k] + Gtr[k]) - 2.0f * r[k] * tr);
}

// slot i of the forward: c2w[i] for camera cam_ids[i]; slot 0 also writes focal.  An id outside [0, num_cams) reads nothing and makes that
// slot's c2w NaN (the convention of body_gen_rays); the backward gives such a slot no contribution.
CNR_HD void body_camera_fwd(const Camera& p, long i) {
  if (i == 0 && p.focal) {
    const float fx = p.fx[0], fy = p.fx_only ? fx : p.fy[0];
    const float sx = (float)p.W, sy = p.fx_only ? (float)p.W : (float)p.H;
    p.focal[0] = p.focal_order == 2 ? (fx * fx) * sx : fx * sx;
    p.focal[1] = p.focal_order == 2 ? (fy * fy) * sy : fy * sy;
  }
  if (!p.c2w || i >= p.B) return;
  float* out = p.c2w + i * 16;
  const long cam = p.cam_ids ? p.cam_ids[i] : i;
  if (cam < 0 || cam >= p.num_cams) {
    const float nan_ = __builtin_nanf("");
    for (int k = 0; k < 16; ++k) out[k] = nan_;
    return;
  }
  float R[9];
  if (p.six_d) { Rot6d w; rot6d_fwd(p.r + cam * 6, R, w); } else expmap_fwd(p.r + cam * 3, R);
  const float* t = p.t + cam * 3;
  if (p.init_c2w) {   // [[R, t], [0 0 0 1]] @ init: the last row of the product is init's last row
    const float* I = p.init_c2w + cam * 16;
    for (int a = 0; a < 3; ++a)
      for (int k = 0; k < 4; ++k)
        out[a * 4 + k] = ((R[a * 3] * I[k] + R[a * 3 + 1] * I[4 + k]) + R[a * 3 + 2] * I[8 + k]) + t[a] * I[12 + k];
    for (int k = 0; k < 4; ++k) out[12 + k] = I[12 + k];
  } else {
    for (int a = 0; a < 3; ++a) { for (int k = 0; k < 3; ++k) out[a * 4 + k] = R[a * 3 + k]; out[a * 4 + 3] = t[a]; }
    out[12] = 0.0f; out[13] = 0.0f; out[14] = 0.0f; out[15] = 1.0f;
  }
}

// the contribution of slot s (camera cam) added to dr [6 or 3] and dt [3]
CNR_HD void camera_slot_bwd(const CameraBwd& q, long s, long cam, float* dr, float* dt) {
  const Camera& p = q.f;
  const float* g = q.d_c2w + s * 16;
  float G[9], gt[3];   // d [R | t] = (d c2w @ init^T)[0:3]
  if (p.init_c2w) {
    const float* I = p.init_c2w + cam * 16;
    for (int a = 0; a < 3; ++a) {
      for (int j = 0; j < 3; ++j) G[a * 3 + j] = ((g[a * 4] * I[j * 4] + g[a * 4 + 1] * I[j * 4 + 1]) + g[a * 4 + 2] * I[j * 4 + 2]) + g[a * 4 + 3] * I[j * 4 + 3];
      gt[a] = ((g[a * 4] * I[12] + g[a * 4 + 1] * I[13]) + g[a * 4 + 2] * I[14]) + g[a * 4 + 3] * I[15];
    }
  } else {
    for (int a = 0; a < 3; ++a) { for (int j = 0; j < 3; ++j) G[a * 3 + j] = g[a * 4 + j]; gt[a] = g[a * 4 + 3]; }
  }
  for (int k = 0; k < 3; ++k) dt[k] += gt[k];
  if (!q.d_r) return;
  if (p.six_d) {
    float R[9], da[6]; Rot6d w;
    rot6d_fwd(p.r + cam * 6, R, w);
    rot6d_bwd(p.r + cam * 6, w, G, da);
    for (int k = 0; k < 6; ++k) dr[k] += da[k];
  } else {
    float da[3];
    expmap_bwd(p.r + cam * 3, G, da);
    for (int k = 0; k < 3; ++k) dr[k] += da[k];
  }
}

// camera `cam` of the backward: its dense rows of d r / d t = the contributions of its slots added in ascending slot order (0 for a camera no
// slot names: Adam sees a dense gradient with zero rows, as after the reference's index backward); camera 0 also writes d fx / d fy
CNR_HD void body_camera_bwd(const CameraBwd& q, long cam) {
  const Camera& p = q.f;
  if (cam == 0 && q.d_focal) {
    const float g0 = q.d_focal[0], g1 = q.d_focal[1];
    const float fx = p.fx[0], sx = (float)p.W;
    const float dx = p.focal_order == 2 ? (g0 * sx) * (2.0f * fx) : g0 * sx;
    if (p.fx_only) {
      const float dx1 = p.focal_order == 2 ? (g1 * sx) * (2.0f * fx) : g1 * sx;
      if (q.d_fx) q.d_fx[0] = dx + dx1;
    } else {
      if (q.d_fx) q.d_fx[0] = dx;
      if (q.d_fy) q.d_fy[0] = p.focal_order == 2 ? (g1 * (float)p.H) * (2.0f * p.fy[0]) : g1 * (float)p.H;
    }
  }
  if (!q.d_c2w || cam >= p.num_cams) return;
  float dr[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, dt[3] = {0.0f, 0.0f, 0.0f};
  if (p.cam_ids) {
    for (long s = 0; s < p.B; ++s) if (p.cam_ids[s] == cam) camera_slot_bwd(q, s, cam, dr, dt);
  } else {
    camera_slot_bwd(q, cam, cam, dr, dt);
  }
  const int nr = p.six_d ? 6 : 3;
  if (q.d_r) for (int k = 0; k < nr; ++k) q.d_r[cam * nr + k] = dr[k];
  if (q.d_t) for (int k = 0; k < 3; ++k) q.d_t[cam * 3 + k] = dt[k];
}

// the point-wise kernels of this family (the form of CNR_POINTWISE_KERNELS, cnr_bodies.h)
#define CNR_CAMERA_KERNELS(X)                                                                             \
  X(camera_fwd, Camera, body_camera_fwd, p.c2w && p.B > 1 ? p.B : 1)                                      \
  X(camera_bwd, CameraBwd, body_camera_bwd, p.d_c2w && p.f.num_cams > 1 ? p.f.num_cams : 1)

}  // namespace cnr
