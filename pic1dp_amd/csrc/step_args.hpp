// step_args.hpp -- the per-distribution launch entries of the whole-step marker kernels (kernels.hpp StepArgs;
// kernels_step.hip is compiled once per distribution, step_dispatch.cpp picks the instance)
#pragma once
#include "kernels.hpp"

namespace pic1dp {

// DIST: 0 Maxwellian, 1 two-stream1, 2 two-stream2, 3 bump-on-tail (-f0'/f0 in the reference's operation order),
// 4 / 5: two-stream2 / bump-on-tail with the one-exp form (device_math.hpp)
template <int DIST>
hipError_t launch_step_dist(const StepArgs &a, bool full, const LaunchCfg &lc, hipStream_t st);
template <> hipError_t launch_step_dist<0>(const StepArgs &, bool, const LaunchCfg &, hipStream_t);
template <> hipError_t launch_step_dist<1>(const StepArgs &, bool, const LaunchCfg &, hipStream_t);
template <> hipError_t launch_step_dist<2>(const StepArgs &, bool, const LaunchCfg &, hipStream_t);
template <> hipError_t launch_step_dist<3>(const StepArgs &, bool, const LaunchCfg &, hipStream_t);
template <> hipError_t launch_step_dist<4>(const StepArgs &, bool, const LaunchCfg &, hipStream_t);
template <> hipError_t launch_step_dist<5>(const StepArgs &, bool, const LaunchCfg &, hipStream_t);

}  // namespace pic1dp
