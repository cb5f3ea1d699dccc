// step_dispatch.cpp -- launch_step: the derived arguments of a whole-step launch, handed to the translation unit of the
// species' distribution (kernels_step.hip, one object per PIC1DP_STEP_DIST)
#include <algorithm>

#include "step_args.hpp"

namespace pic1dp {

hipError_t launch_step(StepArgs a, bool full, const LaunchCfg &lc, hipStream_t st) {
  StepArgsDev &d = a.d;
  d.snx = d.g.dnx / d.g.lx;
  d.pred_k = d.dt_half * d.s.Z / d.s.m;
  d.dtz_half = d.dt_half * d.s.Z;
  d.dtz_full = d.dt_full * d.s.Z;
  {  // rows of pairs a workgroup takes (static grid stride; the drawn chunks are its own rows), two markers a pair
    const int64_t npair = d.np >> 1, stride = static_cast<int64_t>(lc.blocks) * lc.threads;
    // (at least 4096: a term times its scale then stays below 2^49, inside the 2^51 the conversion's magic number covers)
    d.fx_markers = std::max(4096.0, 2.0 * static_cast<double>((npair + stride - 1) / stride) * lc.threads + 2.0);
    d.fx_cap = 0x1p61 / d.fx_markers;
  }
  // full-f evaluates no f0 derivative: one instantiation (in the DIST 0 unit) serves every distribution
  if (!a.deltaf) return launch_step_dist<0>(a, full, lc, st);
  switch (a.iptcldist) {
    case 1: return launch_step_dist<1>(a, full, lc, st);
    case 2: return d.s.one_exp ? launch_step_dist<4>(a, full, lc, st) : launch_step_dist<2>(a, full, lc, st);
    case 3: return d.s.one_exp ? launch_step_dist<5>(a, full, lc, st) : launch_step_dist<3>(a, full, lc, st);
    default: return launch_step_dist<0>(a, full, lc, st);
  }
}

}  // namespace pic1dp
