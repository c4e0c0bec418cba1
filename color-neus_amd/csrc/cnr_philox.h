// Counter-based random words and the 64-bit multiply-high both builds share: the integer arithmetic under the on-device pixel choice
// (cnr_pixels.h) and the mesh surface sampler (cnr_surface.h).  include/colorneus_render.h specifies both for the caller.
#pragma once
#include "cnr_common.h"

namespace cnr {

// Philox4x32-10 of the counter (c0, c1, c2, c3) under (k0, k1)
CNR_HD void pix_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4]) {
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
CNR_HD unsigned long long pix_mulhi64(unsigned long long a, unsigned long long b) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(CNR_CPU_EMU)
  return __umul64hi(a, b);
#else
  return (unsigned long long)(((unsigned __int128)a * b) >> 64);
#endif
}

}  // namespace cnr
