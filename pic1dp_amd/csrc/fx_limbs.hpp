// fx_limbs.hpp -- host arithmetic the exact sums share (the charge sum's quantum, the exact diagnostics, the exact moments):
// ceil(log2) of a bound for the quanta, and rows of (hi, lo) limbs -- value = hi 2^32 + lo quanta -- normalised, summed and
// converted to doubles.  Host-only and inline; no HIP call.  Every addition wraps in unsigned arithmetic, as the integer sums
// on the device do: any 64-bit pattern is a defined input (lo is read as unsigned), and a stand-alone program can run all of
// it under the host's sanitizers (tests/fx_limbs_check.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "kernels.hpp"

namespace pic1dp_host {

// ceil(log2 b) of a positive finite b = f 2^k, f in [0.5, 1): k, or k - 1 for a power of two
inline int ceil_log2(double b) {
  int k = 0;
  const double f = std::frexp(b, &k);
  return f == 0.5 ? k - 1 : k;
}

// hi[i] += lo[i] >> 32, lo[i] &= 2^32 - 1, in place
inline void fx_row_normalise(int64_t *hi, int64_t *lo, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const uint64_t u = static_cast<uint64_t>(lo[i]);
    hi[i] = static_cast<int64_t>(static_cast<uint64_t>(hi[i]) + (u >> 32));
    lo[i] = static_cast<int64_t>(u & 0xffffffffull);
  }
}

// (H, L) <- the sum of the row's values as one pair of limbs, L below n 2^32: every element normalised as it is added
inline void fx_row_sum(const int64_t *hi, const int64_t *lo, size_t n, int64_t *H, int64_t *L) {
  uint64_t h = 0, l = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t u = static_cast<uint64_t>(lo[i]);
    h += static_cast<uint64_t>(hi[i]) + (u >> 32);
    l += u & 0xffffffffull;
  }
  *H = static_cast<int64_t>(h), *L = static_cast<int64_t>(l);
}

// out[i] = (hi[i] 2^32 + lo[i]) quanta, converted once (kernels.hpp fx_limbs_to_double: to nearest, ties to even), times
// q = 2^e; the limbs need not be normalised
inline void fx_row_to_double(const int64_t *hi, const int64_t *lo, size_t n, double q, double *out) {
  for (size_t i = 0; i < n; ++i) {
    const uint64_t u = static_cast<uint64_t>(lo[i]);
    const int64_t h = static_cast<int64_t>(static_cast<uint64_t>(hi[i]) + (u >> 32));
    out[i] = pic1dp::fx_limbs_to_double(h, u & 0xffffffffull) * q;
  }
}

}  // namespace pic1dp_host
