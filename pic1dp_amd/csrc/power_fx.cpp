// power_fx.cpp -- host arithmetic of the exact wave-particle power (power_fx.hpp).  No HIP call.
#include "power_fx.hpp"

#include <cmath>

#include "fx_limbs.hpp"

namespace pic1dp_host {

bool power_fx_base(int32_t charge_quantum, double v_max, int32_t *e_base) {
  if (!(v_max > 0.0) || !std::isfinite(v_max)) return false;
  *e_base = charge_quantum + 52 + ceil_log2(v_max) - 40;   // |p|, |w| <= 2^kb, kb = charge_quantum + 52
  return true;
}

bool power_fx_quantum(int32_t e_base, double max_abs_E, int32_t *e) {
  if (!(max_abs_E >= 0.0) || !std::isfinite(max_abs_E)) return false;
  const int32_t k = e_base + (max_abs_E > 0.0 ? ceil_log2(max_abs_E) : 0);
  *e = k > pic1dp::POWER_FX_MIN_E ? k : pic1dp::POWER_FX_MIN_E;
  return true;
}

void power_fx_normalise(int64_t *limbs, int nsets, int nxo, int nvo) {
  const size_t nxv = static_cast<size_t>(nxo) * nvo;
  for (int j = 0; j < nsets; ++j) {
    int64_t *s = limbs + static_cast<size_t>(j) * (2 * nxv + 2);
    fx_row_normalise(s, s + nxv, nxv);
    fx_row_normalise(s + 2 * nxv, s + 2 * nxv + 1, 1);
  }
}

void power_fx_convert(int32_t e, const int64_t *limbs, int nsets, int nxo, int nvo, double *out) {
  const size_t nxv = static_cast<size_t>(nxo) * nvo;
  const double q = std::ldexp(1.0, e);
  for (int j = 0; j < nsets; ++j) {
    const int64_t *hi = limbs + static_cast<size_t>(j) * (2 * nxv + 2), *lo = hi + nxv;
    double *o = out + static_cast<size_t>(j) * (nxv + nvo + 1);
    fx_row_to_double(hi, lo, nxv, q, o);
    for (int iv = 0; iv < nvo; ++iv) {   // the row's integers first, one conversion
      int64_t H, L;
      fx_row_sum(hi + static_cast<size_t>(iv) * nxo, lo + static_cast<size_t>(iv) * nxo, nxo, &H, &L);
      fx_row_to_double(&H, &L, 1, q, o + nxv + iv);
    }
    fx_row_to_double(hi + 2 * nxv, hi + 2 * nxv + 1, 1, q, o + nxv + nvo);
  }
}

}  // namespace pic1dp_host
