// opt_grid.hpp -- the two lookups every statement of an optimisation event makes per marker, once, for host and device:
// optimize.cpp (the routines), kernels_opt.hip (the kernels) and optcheck.cpp (the host statement of the kernels) are all
// compiled with -ffp-contract=off, so these operations give the same bits wherever they run.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace pic1dp {

// position of velocity v on the nv-point grid over [-v_max, v_max] and the |delta f| there: linear interpolation
// inside, end values outside (src/pic1dp_particle.F90:449-463, repeated at :552-566 and :660-674)
__host__ __device__ __forceinline__ double opt_df(const double *hist, int nv, double v_max, double v, int &cell) {
  const int last = nv - 1;
  const double pos = (v + v_max) / (v_max * 2.0) * static_cast<double>(last);
  const double fl = floor(pos);
  // (the comparison on the double: a velocity far outside must not overflow the conversion)
  if (fl < 0.0) {
    cell = 0;
    return hist[0];
  }
  if (fl >= static_cast<double>(last)) {
    cell = last;
    return hist[last];
  }
  const int c = static_cast<int>(fl);
  cell = c;
  const double left = 1.0 - (pos - static_cast<double>(c));
  return hist[c] * left + hist[c + 1] * (1.0 - left);
}

// x = mod(x, lx); if (x < 0) x = x + lx   (:473-475)
__host__ __device__ __forceinline__ double opt_wrap(double x, double lx) {
  double xx = fmod(x, lx);
  if (xx < 0.0) xx = xx + lx;
  return xx;
}

}  // namespace pic1dp
