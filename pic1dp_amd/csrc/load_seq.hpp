// load_seq.hpp -- the definition of the on-device particle load (include/pic1dp_hip.h pic1dp_hip_particle_load_device;
// DESIGN.md 2.16): which two uniform numbers global marker g of a species gets, and the host-computed constants of the
// marker values.  Host arithmetic, no HIP call; the kernel's own form of the same functions is device_load.hpp, which the
// tests hold against this one bit for bit.  All integer arithmetic is mod 2^64.
#pragma once
#include <cstdint>

#include "../../include/pic1dp_hip.h"

namespace pic1dp {

constexpr int LOAD_RANDOM = 1, LOAD_QUIET = 2;
constexpr uint64_t LOAD_KEY_BASE = 0x7069633164704C44ull;   // "pic1dpLD"
constexpr uint64_t LOAD_GOLD = 0x9E3779B97F4A7C15ull;       // splitmix64's increment
constexpr int LOAD_R3_DIGITS = 21;
constexpr uint64_t LOAD_R3_SPAN = 10460353203ull;           // 3^21: the most markers of a species a quiet start serves

// the splitmix64 finaliser
constexpr uint64_t load_mix64(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// kind 1: the key of (seed_offset, species) and draw c of a key -- splitmix64's output c of the state `key`
constexpr uint64_t load_key(int32_t seed_offset, int32_t ispecies) {
  return load_mix64(LOAD_KEY_BASE + 256ull * static_cast<uint64_t>(static_cast<int64_t>(seed_offset)) +
                    static_cast<uint64_t>(static_cast<int64_t>(ispecies)));
}
constexpr uint64_t load_draw(uint64_t key, uint64_t c) { return load_mix64(key + (c + 1ull) * LOAD_GOLD); }
// kind 2: the 64 bits of g reversed, and the 21 base-3 digits of g reversed (g < 3^21)
constexpr uint64_t load_bitrev64(uint64_t g) {
  uint64_t r = 0;
  for (int i = 0; i < 64; ++i) r |= ((g >> i) & 1ull) << (63 - i);
  return r;
}
constexpr uint64_t load_r3(uint64_t g) {
  uint64_t r = 0;
  for (int i = 0; i < LOAD_R3_DIGITS; ++i) {
    r = r * 3ull + g % 3ull;
    g /= 3ull;
  }
  return r;
}
// the top 53 bits of a word as a double in [0, 1)
inline double load_unit(uint64_t r) { return static_cast<double>(r >> 11) * 0x1p-53; }

// (u_v, u_x) of global marker g; key: load_key (kind 1 only)
inline void load_uniforms(int kind, uint64_t key, uint64_t g, double *uv, double *ux) {
  if (kind == LOAD_RANDOM) {
    *uv = load_unit(load_draw(key, 2ull * g));
    *ux = load_unit(load_draw(key, 2ull * g + 1ull));
  } else {
    *uv = load_unit(load_bitrev64(g));
    *ux = static_cast<double>(load_r3(g)) / static_cast<double>(LOAD_R3_SPAN);   // one IEEE division of two exact integers
  }
}

// The constants of a species' marker values, formed on the host as loader.cpp load_block_species forms them (imarker = 2),
// and what the kernel needs of the input beside them.
struct LoadConst {
  double lx, vmax;
  double pref, a1, a2, g1, g2, g8, gs;
  double den, beam, v0;
  int nim;                                    // init_nmode
  double kk[PIC1DP_MAX_INIT_MODES];           // 2 pi / lx * init_mode[j]
  double mcos[PIC1DP_MAX_INIT_MODES], msin[PIC1DP_MAX_INIT_MODES];
};
LoadConst make_load_const(const pic1dp_input &in, int isp);

// first global marker of the first block a process owns: the valid markers of the reference blocks before it
int64_t load_origin(const pic1dp_input &in, int isp, int blk0, int npe);

// why a load of this kind cannot run on this input (null: it can); host checks only
const char *load_refusal(const pic1dp_input &in, int kind, int seed_offset);

}  // namespace pic1dp
