// Per-element bodies of the render path's point-wise kernels (host+device; shared by the HIP and CPU-emulation backends).
#pragma once
#include "cnr_backend.h"
#include "cnr_raymath.h"

namespace cnr {

// one (ray, sample) element of EmbedZ; `out`: where the kEmb-wide row goes (the HIP kernels stage rows in LDS and store them coalesced)
CNR_HD void body_embed_z_rows(const EmbedZ& p, long idx, float* out, float*) {
  long r = idx / p.m;
  int j = (int)(idx - r * p.m);
  float zz;
  if (p.make_z) {
    float nr = p.near_[r], fr = p.far_[r];
    zz = nr + (fr - nr) * linspace_at(0.0f, 1.0f, p.m, j);
    if (p.t_rand) zz = zz + (p.t_rand[r] - 0.5f) * 2.0f / (float)p.m;
    p.z[r * p.ldz + j] = zz;
  } else {
    zz = p.z[r * p.ldz + j];
  }
  float x[3];
  for (int c = 0; c < 3; ++c) x[c] = (p.o[r * 3 + c] + p.d[r * 3 + c] * zz) * p.scale;
  for (int c = 0; c < kEmb; ++c) out[c] = 0.0f;
  pe_row(x, p.multires, out);   // (straight into the destination row: a local array indexed by the runtime multires would live in scratch memory)
}
CNR_HD void body_embed_z(const EmbedZ& p, long idx) { body_embed_z_rows(p, idx, p.E + idx * kEmb, nullptr); }

CNR_HD void body_embed_pts_rows(const EmbedPts& p, long i, float* e, float* a) {
  float pp[3];
  if (p.pts) {
    pp[0] = p.pts[i * 3]; pp[1] = p.pts[i * 3 + 1]; pp[2] = p.pts[i * 3 + 2];
  } else {
    long idx = p.start + i;
    long r2 = (long)p.res * p.res;
    int ix = (int)(idx / r2), iy = (int)((idx / p.res) % p.res), iz = (int)(idx % p.res);
    pp[0] = linspace_at(p.bmin[0], p.bmax[0], p.res, ix);
    pp[1] = linspace_at(p.bmin[1], p.bmax[1], p.res, iy);
    pp[2] = linspace_at(p.bmin[2], p.bmax[2], p.res, iz);
  }
  float x[3] = {pp[0] * p.scale, pp[1] * p.scale, pp[2] * p.scale};
  for (int c = 0; c < kEmb; ++c) e[c] = 0.0f;
  pe_row(x, p.multires, e);
  if (p.AUX) {
    for (int c = 0; c < kAux; ++c) a[c] = 0.0f;
    a[0] = pp[0]; a[1] = pp[1]; a[2] = pp[2];
  }
}
CNR_HD void body_embed_pts(const EmbedPts& p, long i) { body_embed_pts_rows(p, i, p.E + i * kEmb, p.AUX ? p.AUX + i * kAux : nullptr); }

CNR_HD void body_fine_setup_rows(const FineSetup& p, long pt, float* e, float* a) {
  long r = pt / p.M;
  int j = (int)(pt - r * p.M);
  float z0 = p.z[r * p.M + j];
  float dist = (j + 1 < p.M) ? p.z[r * p.M + j + 1] - z0 : p.sample_dist;
  float mid = z0 + dist * 0.5f;
  float pp[3], x[3], dd[3];
  for (int c = 0; c < 3; ++c) {
    dd[c] = p.d[r * 3 + c];
    pp[c] = p.o[r * 3 + c] + dd[c] * mid;
    x[c] = pp[c] * p.scale;
  }
  for (int c = 0; c < kEmb; ++c) e[c] = 0.0f;
  pe_row(x, p.multires, e);
  for (int c = 0; c < kAux; ++c) a[c] = 0.0f;
  a[0] = pp[0]; a[1] = pp[1]; a[2] = pp[2];
  if (p.multires_view > 0) pe_row(dd, p.multires_view, a + 6);
  else { a[6] = dd[0]; a[7] = dd[1]; a[8] = dd[2]; }
}
CNR_HD void body_fine_setup(const FineSetup& p, long pt) { body_fine_setup_rows(p, pt, p.E + pt * kEmb, p.AUX + pt * kAux); }

// g = scale * J^T ce with J = d PE / d x0; E holds sin/cos of the encoding
CNR_HD void body_grad_finish(const GradFinish& p, long pt) {
  const float* e = p.E + pt * kEmb;
  const float* c0 = p.ce0 + pt * kEmb;
  const float* cs = p.ces ? p.ces + pt * kEmb : nullptr;
  for (int c = 0; c < 3; ++c) {
    float acc = c0[c] + (cs ? cs[c] : 0.0f);
    float f = 1.0f;
    for (int k = 0; k < p.multires; ++k) {
      float csin = c0[3 + 6 * k + c] + (cs ? cs[3 + 6 * k + c] : 0.0f);
      float ccos = c0[6 + 6 * k + c] + (cs ? cs[6 + 6 * k + c] : 0.0f);
      acc = acc + f * (e[6 + 6 * k + c] * csin - e[3 + 6 * k + c] * ccos);
      f *= 2.0f;
    }
    float g = acc * p.scale;
    p.grad_out[pt * 3 + c] = g;
    p.AUX[pt * kAux + 3 + c] = g;
  }
  if (p.neg_g_as_view) {
    float v[3] = {-p.AUX[pt * kAux + 3], -p.AUX[pt * kAux + 4], -p.AUX[pt * kAux + 5]};
    float row[kAux];
    for (int c = 0; c < kAux; ++c) row[c] = 0.0f;
    if (p.multires_view > 0) pe_row(v, p.multires_view, row);
    else { row[0] = v[0]; row[1] = v[1]; row[2] = v[2]; }
    int npe = p.multires_view > 0 ? 3 + 6 * p.multires_view : 3;
    for (int c = 0; c < npe; ++c) p.AUX[pt * kAux + 6 + c] = row[c];
  }
  if (p.featx) {
    float* fx = p.featx + pt * p.ldfx + p.F;
    const float* a = p.AUX + pt * kAux;
    const int w = p.ldfx - p.F;
    for (int c = 0; c < w; ++c) fx[c] = c < kAux ? a[c] : 0.0f;
  }
}

CNR_HD void body_coltop_bwd(const ColTopBwd& p, long pt) {
  for (int c = 0; c < 3; ++c) {
    float gc = p.gc_a[pt * p.ldtop + c] + (p.gc_b ? p.gc_b[pt * 4 + c] : 0.0f);
    float y = p.gcolor[pt * 4 + c];
    p.out[pt * p.ldtop + c] = p.squeeze ? gc * y * (1.0f - y) : gc;
  }
  for (int c = 3; c < p.ldtop; ++c) p.out[pt * p.ldtop + c] = 0.0f;
}

CNR_HD void body_gbar_finish(const GbarFinish& p, long pt) {
  const float* e = p.E + pt * kEmb;
  float* cb = p.cbar + pt * kEmb;
  for (int c = 0; c < kEmb; ++c) cb[c] = 0.0f;
  for (int c = 0; c < 3; ++c) {
    float gb = p.gbar_alpha[pt * 4 + c];
    if (p.daux_c) gb += p.daux_c[pt * kAux + 3 + c];
    if (p.daux_r) gb += p.daux_r[pt * kAux + 3 + c];
    p.gbar_total[pt * 4 + c] = gb;
    float t = gb * p.scale;
    cb[c] = t;
    float f = 1.0f;
    for (int k = 0; k < p.multires; ++k) {
      cb[3 + 6 * k + c] = f * e[6 + 6 * k + c] * t;     // d g / d ce_sin = 2^k cos(2^k x0)
      cb[6 + 6 * k + c] = -f * e[3 + 6 * k + c] * t;    // d g / d ce_cos = -2^k sin(2^k x0)
      f *= 2.0f;
    }
  }
  p.gbar_total[pt * 4 + 3] = 0.0f;
}

// total cotangent of the sample position p (only evaluated when rays require grad)
CNR_HD void body_pbar_finish(const PbarFinish& p, long pt) {
  const float* e = p.E + pt * kEmb;
  for (int c = 0; c < 3; ++c) {
    float eb = p.ebar0[pt * kEmb + c] + (p.ebars ? p.ebars[pt * kEmb + c] : 0.0f);
    float x0bar = eb;
    float second = 0.0f;
    float f = 1.0f;
    for (int k = 0; k < p.multires; ++k) {
      float s = e[3 + 6 * k + c], co = e[6 + 6 * k + c];
      float ebs = p.ebar0[pt * kEmb + 3 + 6 * k + c] + (p.ebars ? p.ebars[pt * kEmb + 3 + 6 * k + c] : 0.0f);
      float ebc = p.ebar0[pt * kEmb + 6 + 6 * k + c] + (p.ebars ? p.ebars[pt * kEmb + 6 + 6 * k + c] : 0.0f);
      x0bar += f * (co * ebs - s * ebc);
      if (p.gbar_total) {
        float ces = p.ce0[pt * kEmb + 3 + 6 * k + c] + (p.ces ? p.ces[pt * kEmb + 3 + 6 * k + c] : 0.0f);
        float cec = p.ce0[pt * kEmb + 6 + 6 * k + c] + (p.ces ? p.ces[pt * kEmb + 6 + 6 * k + c] : 0.0f);
        second += f * f * (-s * ces - co * cec);
      }
      f *= 2.0f;
    }
    if (p.gbar_total) x0bar += p.gbar_total[pt * 4 + c] * p.scale * second;
    float pb = x0bar * p.scale;
    if (p.daux_c) pb += p.daux_c[pt * kAux + c];
    if (p.daux_r) pb += p.daux_r[pt * kAux + c];
    p.pbar[pt * 4 + c] = pb;
  }
  p.pbar[pt * 4 + 3] = 0.0f;
}

// SDF point queries: element i of the flat [P][3] padded copy of the points (rows >= n at the origin)
CNR_HD void body_query_in(const QueryIn& p, long i) {
  p.out[i] = i < p.n * 3 ? p.pts[i] : 0.0f;
  if (i == 0) *p.tag = p.tag_value;
}
CNR_HD bool query_ctx_mismatch(const QuerySeed& p) {
  const int t = *p.tag;
  return p.want_grad ? t != kQueryCtxTag + 1 : (t != kQueryCtxTag && t != kQueryCtxTag + 1);
}

// four consecutive columns of a ZTOP row (i < P * ldztop / 4), then one gbar row each (i - P * ldztop / 4): one 16-byte store per element
CNR_HD void body_query_seed(const QuerySeed& p, long i) {
  const long q4 = p.ldztop / 4, nz = p.P * q4;
  const float poison = query_ctx_mismatch(p) ? __builtin_nanf("") : 0.0f;   // NaN + x: every seed, hence every output, is NaN
  if (i < nz) {
    const long row = i / q4;
    const int c0 = (int)(i - row * q4) * 4;
    float v[4];
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j;
      float t = 0.0f;
      if (row < p.n) {
        if (c < p.F) t = p.d_feat ? p.d_feat[row * p.F + c] : 0.0f;
        else if (c == p.F) t = p.d_sdf ? p.d_sdf[row] * p.inv_scale : 0.0f;
      }
      v[j] = t + poison;
    }
    f4 o; o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
    *reinterpret_cast<f4*>(p.ztop + row * p.ldztop + c0) = o;
  } else {
    const long row = i - nz;
    const bool live = row < p.n && p.d_grad;
    f4 o;
    o.x = (live ? p.d_grad[row * 3 + 0] : 0.0f) + poison; o.y = (live ? p.d_grad[row * 3 + 1] : 0.0f) + poison;
    o.z = (live ? p.d_grad[row * 3 + 2] : 0.0f) + poison; o.w = 0.0f;
    *reinterpret_cast<f4*>(p.gbar + row * 4) = o;
  }
}

// element i of the concatenated outputs [sdf (n) | feat (n * F) | g (n * 3)] (absent outputs take no elements): consecutive threads write
// consecutive addresses of one caller buffer
CNR_HD void body_query_out(const QueryOut& p, long i) {
  if (p.sdf) {
    if (i < p.n) { p.sdf[i] = p.sdf_in[i]; return; }
    i -= p.n;
  }
  if (p.feat) {
    const long nf = p.n * p.F;
    if (i < nf) { const long r = i / p.F; p.feat[i] = p.feat_in[r * p.ldf + (i - r * p.F)]; return; }
    i -= nf;
  }
  const long r = i / 3;
  p.g[i] = p.g_in[r * p.ldg + (i - r * 3)];
}
CNR_HD long query_out_count(const QueryOut& p) { return (p.sdf ? p.n : 0) + (p.feat ? p.n * p.F : 0) + (p.g ? p.n * 3 : 0); }

// The point-wise kernels whose HIP form is the plain grid-stride loop over a body: X(name, parameter struct, body, element count of p).
// CNR_PW_KERNEL (cnr_hip_util.h) expands a row into kernel + launch + be_<name>, the emulation into an OpenMP loop.  (The row-staged embed_z /
// embed_pts / fine_setup and the 16-lanes-per-point grad_finish / gbar_finish have HIP kernels of their own.)  These are the render path's rows;
// the rows of a stand-alone family are in its header: CNR_RAYS_KERNELS (cnr_rays.h), CNR_CAMERA_KERNELS (cnr_cameras.h), CNR_BG_KERNELS (cnr_bg.h).
#define CNR_POINTWISE_KERNELS(X)                                                                          \
  X(coltop_bwd, ColTopBwd, body_coltop_bwd, p.P)                                                          \
  X(pbar_finish, PbarFinish, body_pbar_finish, p.P)                                                       \
  X(query_in, QueryIn, body_query_in, p.P * 3)                                                            \
  X(query_seed, QuerySeed, body_query_seed, p.P * (p.ldztop / 4) + (p.gbar ? p.P : 0))                    \
  X(query_out, QueryOut, body_query_out, query_out_count(p))

}  // namespace cnr
