// ICP registration of a point set to a cloud or a mesh (cnr_icp): descriptor, launches and the per-element arithmetic the HIP kernels
// (cnr_register.hip) and the CPU emulation (cnr_kernels_emu.cpp) share.  include/colorneus_render.h states the rules for the caller.  The
// search is the existing one (be_nn_search / be_point_mesh_distance, unchanged); what is here is the loop around it: the fp32 move of the
// source under the current transform, the fp64 moments of the inlier pairs in ONE summation order, and the closed-form solve.  Every float
// and double operation below is one separately rounded operation in the written order (-ffp-contract=off: no FMA; fp64 / and sqrt are
// correctly rounded on both builds), so the emulation, the HIP build and a restatement in Python floats give the same bits.
#pragma once
#include "cnr_common.h"
#include "cnr_nn.h"
#include "cnr_surface.h"

namespace cnr {

constexpr int kIcpChunk = 256;    // points per moment chunk: one workgroup of the moments kernel, one row of partials
constexpr int kIcpTerms = 18;     // a (3), b (3), b[r]*a[c] (9, row-major), a.a, b.b, dist2
constexpr int kIcpSweeps = 10;    // cyclic Jacobi sweeps over the 4x4 matrix: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) each

struct IcpStep {
  const float* source; long n;          // [n][3], 0 < n < 2^31
  const float* target; long m;          // cloud [m][3], or the mesh's vertices [V][3]
  const int* triangles; long F;         // [F][3], or null with F == 0: cloud target
  double c_src[3], c_tgt[3];            // the pivots (read on the host when the call is issued)
  int with_scale; float max_dist2;
  int first;                            // 1: idx holds nothing yet -- it is not read, and n_changed = n
  double* transform;                    // [16] in / out: R row-major [9], t [3], s, 3 x 0.0
  double* history;                      // [4] of THIS iteration: {n_inliers, n_changed, sum of the inliers' dist2, status}; between the moments
                                        // and the solve launch the first two hold the counts as 64-bit integers (zero-filled before the launch)
  float* moved; float* matched; float* dist2; int* idx;   // [n][3], [n][3], [n], [n]
  unsigned long long* keys;             // [n] scratch of the search
  double* partials;                     // [ceil(n / 256)][18]
};
// one iteration on the stream: move, search, moments, solve (be_nn_search / be_point_mesh_distance are called by the backend's be_icp_step)
void be_icp_step(const IcpStep& p, cnr_stream s);
// zeros into `bytes` bytes on the stream (the history rows' integer counts start from zero)
void be_icp_clear(void* p, size_t bytes, cnr_stream s);
// the match of an iteration: the existing searches on the moved points; dist2 / idx of the nearest target point, or of the closest face
inline void icp_search(const IcpStep& p, cnr_stream s) {
  if (p.F > 0) {
    PointMeshDist d;
    d.query = p.moved; d.n = p.n; d.vertices = p.target; d.V = p.m; d.triangles = p.triangles; d.F = p.F;
    d.dist2 = p.dist2; d.face = p.idx; d.closest = nullptr; d.keys = p.keys;   // (the closest point: icp_pair, behind the stash in matched)
    be_point_mesh_distance(d, s);
  } else {
    NnSearch q;
    q.query = p.moved; q.n = p.n; q.target = p.target; q.m = p.m; q.dist2 = p.dist2; q.idx = p.idx; q.keys = p.keys;
    be_nn_search(q, s);
  }
}

// ---- move ------------------------------------------------------------------------------------------------------------------------------------
// m[r][c] = (float)(s * R[r][c]) (a double product rounded once to fp32), tf[r] = (float)t[r]
struct IcpMap { float m[9], t[3]; };
CNR_HD IcpMap icp_map(const double* T) {
  IcpMap k;
  for (int j = 0; j < 9; ++j) k.m[j] = (float)(T[12] * T[j]);
  for (int r = 0; r < 3; ++r) k.t[r] = (float)T[9 + r];
  return k;
}
// moved_i[r] = ((m[r][0]*x + m[r][1]*y) + m[r][2]*z) + tf[r].  The search is about to overwrite idx; matched is written only by the moments
// launch, so the previous iteration's idx_i travels through the search in the bits of matched[i][0].
CNR_HD void icp_move(const IcpStep& p, const IcpMap& k, long i) {
  const float x = p.source[i * 3], y = p.source[i * 3 + 1], z = p.source[i * 3 + 2];
  for (int r = 0; r < 3; ++r) p.moved[i * 3 + r] = ((k.m[r * 3] * x + k.m[r * 3 + 1] * y) + k.m[r * 3 + 2] * z) + k.t[r];
  if (!p.first) memcpy(&p.matched[i * 3], &p.idx[i], sizeof(int));
}

// ---- moments ---------------------------------------------------------------------------------------------------------------------------------
// Point i after the search: matched_i (the target point idx_i; on a mesh the closest point of face idx_i, surf_finish's own expression; NaN
// without a candidate), whether idx_i differs from the previous iteration's, whether the pair is an inlier (idx_i >= 0 and dist2_i <=
// max_dist2, an fp32 compare) and its eighteen terms -- all zero for a non-inlier, so that the sum's structure is fixed.
//   a = (double)source_i - c_src (the ORIGINAL point: the solved transform is absolute), b = (double)matched_i - c_tgt
//   x[0..2] = a, x[3..5] = b, x[6 + 3r + c] = b[r]*a[c], x[15] = (a0*a0 + a1*a1) + a2*a2, x[16] = the same of b, x[17] = (double)dist2_i
CNR_HD void icp_pair(const IcpStep& p, long i, double* x /* [kIcpTerms] */, int* inlier, int* changed) {
  const int j = p.idx[i];
  int prev = -2;
  if (!p.first) memcpy(&prev, &p.matched[i * 3], sizeof(int));
  *changed = p.first || prev != j;
  const float nan = __builtin_nanf("");
  float mx = nan, my = nan, mz = nan;
  if (j >= 0) {
    if (p.F > 0) {
      surf_closest(surf_record(p.target, p.m, p.triangles + (long)j * 3), p.moved[i * 3], p.moved[i * 3 + 1], p.moved[i * 3 + 2], &mx, &my, &mz);
    } else {
      mx = p.target[(long)j * 3]; my = p.target[(long)j * 3 + 1]; mz = p.target[(long)j * 3 + 2];
    }
  }
  p.matched[i * 3] = mx; p.matched[i * 3 + 1] = my; p.matched[i * 3 + 2] = mz;
  const float d2 = p.dist2[i];
  *inlier = j >= 0 && d2 <= p.max_dist2;
  for (int t = 0; t < kIcpTerms; ++t) x[t] = 0.0;
  if (*inlier) {
    const double a[3] = {(double)p.source[i * 3] - p.c_src[0], (double)p.source[i * 3 + 1] - p.c_src[1], (double)p.source[i * 3 + 2] - p.c_src[2]};
    const double b[3] = {(double)mx - p.c_tgt[0], (double)my - p.c_tgt[1], (double)mz - p.c_tgt[2]};
    for (int r = 0; r < 3; ++r) { x[r] = a[r]; x[3 + r] = b[r]; }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) x[6 + r * 3 + c] = b[r] * a[c];
    x[15] = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    x[16] = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    x[17] = (double)d2;
  }
}

// ---- solve -----------------------------------------------------------------------------------------------------------------------------------
CNR_HD bool icp_finite(double v) { return v - v == 0.0; }
// One Jacobi rotation of the symmetric 4x4 matrix A in the plane (p, q), accumulated into V (columns = eigenvectors); skipped when A[p][q]
// is exactly 0.  theta = (A[q][q] - A[p][p]) / (2 * A[p][q]);  t = sgn(theta) / (|theta| + sqrt(theta*theta + 1)) with sgn(0) = +1;
// c = 1 / sqrt(t*t + 1), s = t * c;  A[p][p] -= t*A[p][q], A[q][q] += t*A[p][q], A[p][q] = A[q][p] = 0;  for the other two rows r:
// A[r][p] = c*arp - s*arq, A[r][q] = s*arp + c*arq (mirrored);  for every row r of V the same pair of expressions.
CNR_HD void icp_jacobi_rotate(double (&A)[4][4], double (&V)[4][4], int p, int q) {
  const double apq = A[p][q];
  if (apq == 0.0) return;
  const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
  const double den = fabs(theta) + sqrt(theta * theta + 1.0);
  const double t = theta < 0.0 ? -1.0 / den : 1.0 / den;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const double h = t * apq;
  A[p][p] = A[p][p] - h; A[q][q] = A[q][q] + h; A[p][q] = 0.0; A[q][p] = 0.0;
  for (int r = 0; r < 4; ++r) {
    if (r != p && r != q) {
      const double arp = A[r][p], arq = A[r][q];
      A[r][p] = c * arp - s * arq; A[p][r] = A[r][p];
      A[r][q] = s * arp + c * arq; A[q][r] = A[r][q];
    }
  }
  for (int r = 0; r < 4; ++r) {
    const double vrp = V[r][p], vrq = V[r][q];
    V[r][p] = c * vrp - s * vrq;
    V[r][q] = s * vrp + c * vrq;
  }
}
// The similarity that takes the inliers' a onto their b in the least-squares sense, from the eighteen sums S (icp_pair's order) and n_inliers:
//   abar = Sa / n, bbar = Sb / n;  C[r][c] = Sba[r][c] - Sb[r]*abar[c];  va = Saa - ((Sa0*abar0 + Sa1*abar1) + Sa2*abar2)
//   Horn's matrix (Sxy = C[y][x], the source axis first):
//     N00 = (Sxx + Syy) + Szz   N01 = Syz - Szy           N02 = Szx - Sxz           N03 = Sxy - Syx
//                               N11 = (Sxx - Syy) - Szz   N12 = Sxy + Syx           N13 = Szx + Sxz
//                                                         N22 = (Syy - Sxx) - Szz   N23 = Syz + Szy
//                                                                                   N33 = (Szz - Sxx) - Syy
//   kIcpSweeps cyclic Jacobi sweeps; the column of V under the largest diagonal element (the lowest index on ties) is (w, x, y, z);
//   nrm = sqrt(((w*w + x*x) + y*y) + z*z), each component / nrm, all four negated when w < 0;
//   R = [1 - 2(yy + zz), 2(xy - wz), 2(xz + wy);  2(xy + wz), 1 - 2(xx + zz), 2(yz - wx);  2(xz - wy), 2(yz + wx), 1 - 2(xx + yy)]
//   s = (the sum of R[r][c]*C[r][c], added in row-major order) / va with scale, else 1
//   t[r] = (bbar[r] + c_tgt[r]) - s * ((R[r][0]*p0 + R[r][1]*p1) + R[r][2]*p2),  p = abar + c_src
// A quaternion always gives a proper rotation: there is no reflection branch.  Returns the status: 1 and T untouched when n_inliers < 3, a sum
// is not finite, va <= 0, or the result is not finite or its scale not positive; else 0 and T = {R, t, s, 0, 0, 0}.
CNR_HD int icp_solve(const double* S, long long n_inliers, const double* c_src, const double* c_tgt, int with_scale, double* T) {
  if (n_inliers < 3) return 1;
  for (int j = 0; j < kIcpTerms; ++j) if (!icp_finite(S[j])) return 1;
  const double n = (double)n_inliers;
  const double abar[3] = {S[0] / n, S[1] / n, S[2] / n}, bbar[3] = {S[3] / n, S[4] / n, S[5] / n};
  double C[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[r][c] = S[6 + r * 3 + c] - S[3 + r] * abar[c];
  const double va = S[15] - ((S[0] * abar[0] + S[1] * abar[1]) + S[2] * abar[2]);
  if (!(va > 0.0)) return 1;
  const double Sxx = C[0][0], Sxy = C[1][0], Sxz = C[2][0], Syx = C[0][1], Syy = C[1][1], Syz = C[2][1], Szx = C[0][2], Szy = C[1][2], Szz = C[2][2];
  double A[4][4], V[4][4];
  A[0][0] = (Sxx + Syy) + Szz; A[0][1] = Syz - Szy; A[0][2] = Szx - Sxz; A[0][3] = Sxy - Syx;
  A[1][1] = (Sxx - Syy) - Szz; A[1][2] = Sxy + Syx; A[1][3] = Szx + Sxz;
  A[2][2] = (Syy - Sxx) - Szz; A[2][3] = Syz + Szy;
  A[3][3] = (Szz - Sxx) - Syy;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      if (c < r) A[r][c] = A[c][r];
      V[r][c] = r == c ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < kIcpSweeps; ++sweep)
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) icp_jacobi_rotate(A, V, p, q);
  double top = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
  for (int j = 1; j < 4; ++j) {
    const bool above = A[j][j] > top;
    top = above ? A[j][j] : top; w = above ? V[0][j] : w; x = above ? V[1][j] : x; y = above ? V[2][j] : y; z = above ? V[3][j] : z;
  }
  const double nrm = sqrt(((w * w + x * x) + y * y) + z * z);
  w = w / nrm; x = x / nrm; y = y / nrm; z = z / nrm;
  if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
  double R[9];
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
  double s = 1.0;
  if (with_scale) {
    double tr = R[0] * C[0][0];
    for (int j = 1; j < 9; ++j) tr = tr + R[j] * C[j / 3][j % 3];
    s = tr / va;
  }
  double t[3];
  const double p0 = abar[0] + c_src[0], p1 = abar[1] + c_src[1], p2 = abar[2] + c_src[2];
  for (int r = 0; r < 3; ++r) t[r] = (bbar[r] + c_tgt[r]) - s * ((R[r * 3] * p0 + R[r * 3 + 1] * p1) + R[r * 3 + 2] * p2);
  bool ok = icp_finite(s) && s > 0.0;
  for (int j = 0; j < 9; ++j) ok = ok && icp_finite(R[j]);
  for (int r = 0; r < 3; ++r) ok = ok && icp_finite(t[r]);
  if (!ok) return 1;
  for (int j = 0; j < 9; ++j) T[j] = R[j];
  for (int r = 0; r < 3; ++r) T[9 + r] = t[r];
  T[12] = s; T[13] = 0.0; T[14] = 0.0; T[15] = 0.0;
  return 0;
}
// the end of an iteration: the transform (untouched when the status is 1) and the history row, from the eighteen sums and the two counts
CNR_HD void icp_finish(const IcpStep& p, const double* S, long long n_inliers, long long n_changed) {
  const int status = icp_solve(S, n_inliers, p.c_src, p.c_tgt, p.with_scale, p.transform);
  p.history[0] = (double)n_inliers; p.history[1] = (double)n_changed; p.history[2] = S[17]; p.history[3] = (double)status;
}

}  // namespace cnr
