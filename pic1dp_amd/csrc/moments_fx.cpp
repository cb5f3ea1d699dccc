// moments_fx.cpp -- host arithmetic of the exact velocity moments (moments_fx.hpp).  No HIP call.
#include "moments_fx.hpp"

#include <cmath>

#include "kernels.hpp"

namespace pic1dp_host {

bool moments_fx_quanta(int32_t charge_quantum, double v_max, int32_t e[4]) {
  if (!(v_max > 0.0) || !std::isfinite(v_max)) return false;
  int kvm = 0;
  const double f = std::frexp(v_max, &kvm);   // v_max = f 2^kvm, f in [0.5, 1): ceil(log2 v_max) = kvm, or kvm - 1 for a power of two
  if (f == 0.5) kvm -= 1;
  const int kb = charge_quantum + 52;          // |p|, |w| <= 2^kb
  for (int k = 0; k < 4; ++k) e[k] = kb + k * kvm - 40;
  return true;
}

void moments_fx_normalise(int64_t *limbs, int planes, int nx) {
  for (int l = 0; l < planes; ++l) {
    int64_t *hi = limbs + static_cast<size_t>(2 * l) * nx, *lo = hi + nx;
    for (int i = 0; i < nx; ++i) {
      const uint64_t u = static_cast<uint64_t>(lo[i]);
      hi[i] = static_cast<int64_t>(static_cast<uint64_t>(hi[i]) + (u >> 32));   // (wraps as the integer sums themselves do)
      lo[i] = static_cast<int64_t>(u & 0xffffffffull);
    }
  }
}

void moments_fx_convert(const int32_t e[4], const int64_t *limbs, int planes, int nx, double *out) {
  for (int l = 0; l < planes; ++l) {
    const int64_t *hi = limbs + static_cast<size_t>(2 * l) * nx, *lo = hi + nx;
    const double q = std::ldexp(1.0, e[l & 3]);
    for (int i = 0; i < nx; ++i) {   // normalised here, in wrapping arithmetic: any 64-bit pattern is an input, none is undefined
      const uint64_t u = static_cast<uint64_t>(lo[i]);
      const int64_t h = static_cast<int64_t>(static_cast<uint64_t>(hi[i]) + (u >> 32));
      out[static_cast<size_t>(l) * nx + i] = pic1dp::fx_limbs_to_double(h, u & 0xffffffffull) * q;
    }
  }
}

}  // namespace pic1dp_host
