// Ray generation for the selected pixels and its backward: descriptors, launches and the per-ray bodies both builds share.
#pragma once
#include "cnr_common.h"
#include "cnr_raymath.h"

namespace cnr {

// ---- ray generation for the selected pixels (the producer right in front of the path): get_rays_multicam / get_rays_at
// (lib/models/tools/ray_utils.py:16-119) with the trainer's origin / radius normalisation and near_far_from_sphere
// (NeuS_Trainer.py:117-119, ray_utils.py:7-13) folded in, and its backward to the camera poses and the focal lengths
struct GenRays {
  const long* pix_idx; long n;          // flat index over (camera, row, column); null: pixel i of camera 0 (get_rays_at)
  const float* c2w; int n_cams;         // [n_cams][4][4]
  const float* focal;                   // [2] (device)
  int H, W, normalize, opengl;
  const float* image; const float* mask;    // [n_cams][H][W][3] / [n_cams][H][W] or null
  const float* origin; float radius;        // rays_o = (rays_o - origin) / radius when origin != null
  float* rays_o; float* rays_d; float* rgb; float* mask_sel; float* near_; float* far_;   // any of rgb / mask_sel / near_ / far_ may be null
  int* bad_count = nullptr;             // device counter or null: +1 per pixel index outside [0, n_cams * H * W) (an error flag, not arithmetic)
};
struct GenRaysBwd {
  GenRays f;                            // the forward arguments (outputs unused)
  const float* d_rays_o; const float* d_rays_d; const float* d_near; const float* d_far;   // upstream gradients (d_near / d_far may be null)
  float* d_c2w;                         // [n_cams][4][4] (bottom row zero)
  float* d_focal_partial;               // [n_cams][2] per-camera contributions, folded in camera order into d_focal
  float* d_focal;                       // [2]
};
void be_gen_rays(const GenRays& p, cnr_stream s);
void be_gen_rays_bwd(const GenRaysBwd& p, cnr_stream s);

// one ray of GenRays
// An index outside [0, n_cams * H * W) (only a caller-supplied list can hold one) reads nothing: every output of that ray is NaN -- which
// the loss then shows -- where the reference's torch indexing would raise; the backward kernel gives such a ray no contribution.
CNR_HD void body_gen_rays(const GenRays& p, long i) {
  const long hw = (long)p.H * p.W;
  const long idx = p.pix_idx ? p.pix_idx[i] : i;
  if (idx < 0 || idx >= hw * p.n_cams) {
    const float nan_ = __builtin_nanf("");
    for (int k = 0; k < 3; ++k) { p.rays_o[i * 3 + k] = nan_; p.rays_d[i * 3 + k] = nan_; if (p.rgb) p.rgb[i * 3 + k] = nan_; }
    if (p.mask_sel) p.mask_sel[i] = nan_;
    if (p.near_ && p.far_) { p.near_[i] = nan_; p.far_[i] = nan_; }
    // the reference's torch indexing raises here; the device cannot: the ray is NaN (loud in the loss) AND counted, so that the host can raise at
    // its next synchronisation point (rays.raise_if_bad_indices) before the NaN gradients reach the optimiser state
    if (p.bad_count) {
#if defined(CNR_CPU_EMU)
#pragma omp atomic
      *p.bad_count += 1;
#else
      atomicAdd(p.bad_count, 1);
#endif
    }
    return;
  }
  const int cam = (int)(idx / hw);
  const long pix = idx - (long)cam * hw;
  const int py = (int)(pix / p.W), px = (int)(pix - (long)py * p.W);
  const RayGeom r = ray_geometry(p.c2w + (long)cam * 16, p.focal[0], p.focal[1], p.H, p.W, px, py, p.normalize, p.opengl);
  float o[3];
  for (int k = 0; k < 3; ++k) {
    o[k] = p.origin ? (r.o[k] - p.origin[k]) / p.radius : r.o[k];
    p.rays_o[i * 3 + k] = o[k];
    p.rays_d[i * 3 + k] = r.d[k];
  }
  if (p.rgb) for (int k = 0; k < 3; ++k) p.rgb[i * 3 + k] = p.image[idx * 3 + k];
  if (p.mask_sel) p.mask_sel[i] = p.mask[idx];
  if (p.near_ && p.far_) {   // near_far_from_sphere (ray_utils.py:7-13)
    const float a = r.d[0] * r.d[0] + r.d[1] * r.d[1] + r.d[2] * r.d[2];
    const float b = 2.0f * (o[0] * r.d[0] + o[1] * r.d[1] + o[2] * r.d[2]);
    const float mid = 0.5f * (-b) / a;
    p.near_[i] = mid - 1.0f;
    p.far_[i] = mid + 1.0f;
  }
}

// gradient contributions of one ray: out[0..11] = d c2w[cam][k][0..3] (k = 0..2), out[12..13] = d focal
CNR_HD void body_gen_rays_bwd1(const GenRaysBwd& q, long i, int* cam_out, float out[14]) {
  const GenRays& p = q.f;
  const long hw = (long)p.H * p.W;
  const long idx = p.pix_idx ? p.pix_idx[i] : i;
  if (idx < 0 || idx >= hw * p.n_cams) {   // (see body_gen_rays: no camera owns this ray)
    for (int k = 0; k < 14; ++k) out[k] = 0.0f;
    *cam_out = -1;
    return;
  }
  const int cam = (int)(idx / hw);
  const long pix = idx - (long)cam * hw;
  const int py = (int)(pix / p.W), px = (int)(pix - (long)py * p.W);
  const float* c2w = p.c2w + (long)cam * 16;
  const float fx = p.focal[0], fy = p.focal[1];
  const RayGeom r = ray_geometry(c2w, fx, fy, p.H, p.W, px, py, p.normalize, p.opengl);
  float dO[3], dD[3];
  for (int k = 0; k < 3; ++k) { dO[k] = q.d_rays_o ? q.d_rays_o[i * 3 + k] : 0.0f; dD[k] = q.d_rays_d ? q.d_rays_d[i * 3 + k] : 0.0f; }
  if (q.d_near && q.d_far) {   // mid = -(o.d) / (d.d): d mid / d o = -d / a, d mid / d d = (-o - 2 mid d) / a
    float o[3];
    for (int k = 0; k < 3; ++k) o[k] = p.origin ? (r.o[k] - p.origin[k]) / p.radius : r.o[k];
    const float a = r.d[0] * r.d[0] + r.d[1] * r.d[1] + r.d[2] * r.d[2];
    const float mid = -(o[0] * r.d[0] + o[1] * r.d[1] + o[2] * r.d[2]) / a;
    const float dm = q.d_near[i] + q.d_far[i];
    for (int k = 0; k < 3; ++k) { dO[k] += dm * (-r.d[k] / a); dD[k] += dm * (-o[k] - 2.0f * mid * r.d[k]) / a; }
  }
  float ddirs[3] = {0.f, 0.f, 0.f};
  for (int k = 0; k < 3; ++k) {
    for (int j = 0; j < 3; ++j) { out[k * 4 + j] = dD[k] * r.dirs[j]; ddirs[j] += dD[k] * c2w[k * 4 + j]; }
    out[k * 4 + 3] = p.origin ? dO[k] / p.radius : dO[k];
  }
  float du[3];
  if (p.normalize) {
    const float dot = r.dirs[0] * ddirs[0] + r.dirs[1] * ddirs[1] + r.dirs[2] * ddirs[2];
    for (int j = 0; j < 3; ++j) du[j] = (ddirs[j] - r.dirs[j] * dot) / r.un;
  } else {
    for (int j = 0; j < 3; ++j) du[j] = ddirs[j];
  }
  out[12] = -r.u[0] / fx * du[0];
  out[13] = -r.u[1] / fy * du[1];
  *cam_out = cam;
}

// the point-wise kernel of this family (the form of CNR_POINTWISE_KERNELS, cnr_bodies.h); the backward has kernels of its own (cnr_rays.hip)
#define CNR_RAYS_KERNELS(X)                                                                               \
  X(gen_rays, GenRays, body_gen_rays, p.n)

}  // namespace cnr
