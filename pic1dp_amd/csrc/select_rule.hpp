// select_rule.hpp -- the rule of pic1dp_hip_select (include/pic1dp_hip.h) on the HOST: which markers a
// selection keeps.  Host arithmetic, no HIP call; the kernels' form of the same rule is device_select.hpp, which the tests
// hold against this one and against tests/select_reference.py bit for bit.  The hash is the on-device load's counter-based
// draw (load_seq.hpp load_draw): mix64(key + (g + 1) * 0x9E3779B97F4A7C15) mod 2^64.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/pic1dp_hip.h"
#include "load_seq.hpp"

namespace pic1dp {

// the deposit's wrap (src/pic1dp_interaction.F90:102-104): fmod, then + lx where negative; not stored back
inline double select_wrap(double x, double lx) {
  double r = std::fmod(x, lx);
  if (r < 0.0) r = r + lx;
  return r;
}

// why a selection cannot run (null: it can): a NaN bound
inline const char *select_refusal(const pic1dp_select &s) {
  if (std::isnan(s.x_lo) || std::isnan(s.x_hi)) return "a bound of the x window is NaN (+-inf says: all)";
  if (std::isnan(s.v_lo) || std::isnan(s.v_hi)) return "a bound of the v window is NaN (+-inf says: all)";
  return nullptr;
}

// is valid marker i, at (x, v), selected?  Every comparison is false for a NaN px or v.
inline bool select_keeps(const pic1dp_select &s, double lx, double x, double v, int64_t i) {
  const double px = select_wrap(x, lx);
  const bool in_x = s.x_lo <= s.x_hi ? (s.x_lo <= px && px < s.x_hi) : (px >= s.x_lo || px < s.x_hi);
  if (!in_x || !(s.v_lo <= v && v < s.v_hi)) return false;
  if (s.thin == 0) return true;
  const uint64_t g = static_cast<uint64_t>(s.origin) + static_cast<uint64_t>(i);
  return load_draw(s.key, g) < s.thin;
}

// the threshold of a kept fraction: 0 (keep all) for fraction >= 1, else max(1, floor(fraction 2^64)); false: fraction <= 0
// or NaN.  fraction 2^64 is exact (a power of two) and below 2^64.
inline bool select_thin_of(double fraction, uint64_t *thin) {
  if (!(fraction > 0.0)) return false;
  if (fraction >= 1.0) {
    *thin = 0;
    return true;
  }
  const double t = std::floor(std::ldexp(fraction, 64));
  *thin = t < 1.0 ? 1 : static_cast<uint64_t>(t);
  return true;
}

}  // namespace pic1dp
