// power_fx.hpp -- host arithmetic of the exact wave-particle power (include/pic1dp_hip.h pic1dp_hip_power_exact; DESIGN.md
// 2.19): the quantum from the input's two bounds and max |E|, the normalisation of the (hi, lo) limbs and their conversion
// to doubles, the v-profile as exact integer row sums.  No context, no HIP call (power_fx.cpp): the entry points of
// capi_products.cpp share it, and a stand-alone program runs it under the host's sanitizers (tests/power_fx_check.cpp).
// Limbs per weight set: [hi plane nx_opd nv_opd | lo plane | rest hi | rest lo], the plane's index iv nx_opd + ix.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pic1dp_host {

// *e_base = kb + kvm - 40 with kb = charge_quantum + 52 and kvm = ceil(log2 v_max); false: v_max is not positive and finite
bool power_fx_base(int32_t charge_quantum, double v_max, int32_t *e_base);
// *e = max(e_base + kE, -1000), kE = ceil(log2 max_abs_E), 0 for max_abs_E = 0; false: max_abs_E is negative, infinite or a NaN
bool power_fx_quantum(int32_t e_base, double max_abs_E, int32_t *e);
// limbs [nsets][2 nxv + 2] (lo any 64-bit pattern, read as unsigned): hi += lo >> 32, lo &= 2^32 - 1, in place
void power_fx_normalise(int64_t *limbs, int nsets, int nxo, int nvo);
// out per set [plane | v-profile | rest], as pic1dp_hip_power lays it out: every bin's total (hi 2^32 + lo) quanta converted
// once (round to nearest even) and multiplied by 2^e; the v-profile is the exact integer sum of its row's bins over ix,
// converted once; the limbs need not be normalised
void power_fx_convert(int32_t e, const int64_t *limbs, int nsets, int nxo, int nvo, double *out);

}  // namespace pic1dp_host
