// digest.hpp -- the state digest's mixing function, shared by the device kernel (kernels_digest.hip), the host digest
// and the checkpoint file's checksum (checkpoint.cpp).  The definition (include/pic1dp_hip.h, pic1dp_hip_state_digest):
// for slot i of an array holding the 64 bits u,
//     z = u + (i + 1) * 0x9E3779B97F4A7C15            (mod 2^64)
//     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
//     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
//     z =  z ^ (z >> 31)
// and the digest is the sum of z over the slots, mod 2^64: an integer sum, whose order does not matter.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PIC1DP_HD __host__ __device__
#else
#define PIC1DP_HD
#endif

namespace pic1dp {

constexpr uint64_t DIGEST_GOLD = 0x9E3779B97F4A7C15ull;
// g = (i + 1) * DIGEST_GOLD, formed by the caller (a sweep adds its stride's multiple instead of multiplying)
PIC1DP_HD inline uint64_t digest_mix(uint64_t u, uint64_t g) {
  uint64_t z = u + g;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the sum over words[0, n) standing at slots i0, i0 + 1, ... (host)
inline uint64_t digest_words(const uint64_t *words, int64_t n, int64_t i0 = 0) {
  uint64_t s = 0, g = static_cast<uint64_t>(i0 + 1) * DIGEST_GOLD;
  for (int64_t i = 0; i < n; ++i, g += DIGEST_GOLD) s += digest_mix(words[i], g);
  return s;
}

}  // namespace pic1dp
