// moments_fx.cpp -- host arithmetic of the exact velocity moments (moments_fx.hpp).  No HIP call.
#include "moments_fx.hpp"

#include <cmath>

#include "fx_limbs.hpp"

namespace pic1dp_host {

bool moments_fx_quanta(int32_t charge_quantum, double v_max, int32_t e[4]) {
  if (!(v_max > 0.0) || !std::isfinite(v_max)) return false;
  const int kvm = ceil_log2(v_max);
  const int kb = charge_quantum + 52;          // |p|, |w| <= 2^kb
  for (int k = 0; k < 4; ++k) e[k] = kb + k * kvm - 40;
  return true;
}

void moments_fx_normalise(int64_t *limbs, int planes, int nx) {
  for (int l = 0; l < planes; ++l) fx_row_normalise(limbs + static_cast<size_t>(2 * l) * nx, limbs + static_cast<size_t>(2 * l + 1) * nx, nx);
}

void moments_fx_convert(const int32_t e[4], const int64_t *limbs, int planes, int nx, double *out) {
  for (int l = 0; l < planes; ++l)
    fx_row_to_double(limbs + static_cast<size_t>(2 * l) * nx, limbs + static_cast<size_t>(2 * l + 1) * nx, nx, std::ldexp(1.0, e[l & 3]),
                     out + static_cast<size_t>(l) * nx);
}

}  // namespace pic1dp_host
