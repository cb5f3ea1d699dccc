// moments_fx.hpp -- host arithmetic of the exact velocity moments (include/pic1dp_hip.h pic1dp_hip_moments_exact; DESIGN.md
// 2.15): the quanta from the input's two bounds, the normalisation of the (hi, lo) limbs and their conversion to doubles.
// No context, no HIP call (moments_fx.cpp): the entry points of capi_products.cpp share it, and a stand-alone program can run it
// under the host's sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pic1dp_host {

// e[k] = kb + k kvm - 40 with kb = charge_quantum + 52 and kvm = ceil(log2 v_max); false: v_max is not positive and finite
bool moments_fx_quanta(int32_t charge_quantum, double v_max, int32_t e[4]);
// limbs [planes][2][nx] (hi row, lo row; lo any 64-bit pattern, read as unsigned): hi += lo >> 32, lo &= 2^32 - 1, in place
void moments_fx_normalise(int64_t *limbs, int planes, int nx);
// out[plane nx + ix] = (hi 2^32 + lo) quanta, converted once (round to nearest even), times 2^e[plane % 4]; the limbs need
// not be normalised
void moments_fx_convert(const int32_t e[4], const int64_t *limbs, int planes, int nx, double *out);

}  // namespace pic1dp_host
