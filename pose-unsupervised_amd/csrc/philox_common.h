// The counter-based generator of the device samplers (mi_sample.hip, fundamental.hip): Philox4x32-10
// and the word -> [0, n) map.  include/posu.h gives the stream definitions built on it.
#pragma once
#include "posu_common.h"

namespace posu {

struct Philox {
  uint32_t c[4];
};

__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0;
    const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    c1 = static_cast<uint32_t>(p1);
    c3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c2 = n2;
  }
  return {{c0, c1, c2, c3}};
}

// (w * n) >> 32 on the 64-bit product: [0, n), bias at most n / 2^32
__device__ __forceinline__ int bounded(uint32_t w, int n) {
  return static_cast<int>((static_cast<uint64_t>(w) * static_cast<uint32_t>(n)) >> 32);
}

}  // namespace posu
