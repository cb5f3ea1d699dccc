// device_fx.hpp -- how a workgroup of the prediction tiles (kernels_step.hip k_step_one) raises the fixed-point bounds of its
// species at its end; shared with the probe library (probe.hip pic1dp_probe_fx_raise), which applies it to sequences of events
#pragma once
#include <hip/hip_runtime.h>

namespace pic1dp {
namespace {

// noted: the workgroup's code of the largest value met within the bound (kernels_step.hip fx_note) -- 0 no marker met, 1
// markers met and none within the bound, 2 + the bits of the float otherwise; start: the bound as the workgroup read it when
// it STARTED (the scale its tiles were summed in).  The bound only grows (atomic max; positive doubles order as integers).
// A workgroup that met none of its markers within 16x start asks for 256 x start -- not 256 x the bound as it stands at its
// end: in one launch the workgroups that finish later would otherwise raise on top of the raises of those that finished
// before them (256^k for k of them).  Every raise then stays below 16x the smallest |value| of the markers that asked for it,
// so the bound stays below 16x the largest value met, whatever the order in which the workgroups finish.
__device__ __forceinline__ void fx_raise(double *bound, unsigned noted, double start) {
  if (noted == 0u) return;
  double want = 0.0;
  if (noted >= 2u) want = static_cast<double>(__uint_as_float(noted - 2u)) * (1.0 + 0x1p-18);   // (rounded twice on the way: not below what was met)
  else if (start > 0.0) want = 256.0 * start;                                                    // markers, and none of them within the bound
  if (!(want < 0x1p120)) return;
  const double cur = __hip_atomic_load(bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (want > cur)
    __hip_atomic_fetch_max(reinterpret_cast<unsigned long long *>(bound), static_cast<unsigned long long>(__double_as_longlong(want)),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace
}  // namespace pic1dp
