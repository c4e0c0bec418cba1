// Exact nearest-neighbour search of 3-D points: descriptor, launch and the per-candidate arithmetic both builds share.
#pragma once
#include "cnr_common.h"

namespace cnr {

// ---- exact brute-force nearest neighbour of 3-D points (cnr_nn_search): the search behind the Chamfer / F-score mesh metrics
// (lib/utils/mesh_tools.py:59-70 calls pytorch3d.loss.chamfer_distance on the vertices of two meshes).
// For query i: the minimum over the targets j of d2(i, j) and the LOWEST j that attains it.  Candidates are ordered by the 64-bit key
// (bits(d2) << 32) | j: d2 >= 0, so its bit pattern orders like its value, and the minimum key is the answer with the tie-break included.
// A split of the target range folds its best keys with an integer min: the result does not depend on the number of splits or their order.
struct NnSearch {
  const float* query; long n;           // [n][3]
  const float* target; long m;          // [m][3], 0 < m < 2^31
  float* dist2; int* idx;               // [n]; a query whose every d2 is NaN gets NaN / -1
  unsigned long long* keys;             // [n] scratch
};
void be_nn_search(const NnSearch& p, cnr_stream s);
constexpr unsigned long long kNnNoKey = ~0ull;   // "no candidate": above every key, and it unpacks to {NaN, -1}
// every operation a separately rounded fp32 operation in this order (the build passes -ffp-contract=off: no FMA)
CNR_HD float nn_dist2(float qx, float qy, float qz, float tx, float ty, float tz) {
  const float dx = qx - tx, dy = qy - ty, dz = qz - tz;
  return (dx * dx + dy * dy) + dz * dz;
}
// The scan over ascending j keeps {best, besti}, starting from {+inf, -1}: a strictly smaller d2 wins, so the lowest j of equal minima stays and
// a NaN never wins.  The one candidate this misses is d2 == +inf itself (overflowing differences) while nothing has been taken yet: nn_update_inf,
// run over a range whose nn_update pass left besti < 0, takes the first of those.
CNR_HD void nn_update(float d2, int j, float& best, int& besti) {
  if (d2 < best) { best = d2; besti = j; }
}
CNR_HD void nn_update_inf(float d2, int j, float best, int& besti) {
  if (besti < 0 && d2 == best) besti = j;   // best is still +inf here
}
CNR_HD unsigned long long nn_key(float best, int besti) {
  if (besti < 0) return kNnNoKey;
  unsigned bits;
  memcpy(&bits, &best, sizeof bits);
  return ((unsigned long long)bits << 32) | (unsigned)besti;
}
CNR_HD void nn_unpack(unsigned long long key, float* dist2, int* idx) {
  const unsigned bits = (unsigned)(key >> 32);
  memcpy(dist2, &bits, sizeof bits);
  *idx = (int)(unsigned)(key & 0xffffffffull);
}

}  // namespace cnr
