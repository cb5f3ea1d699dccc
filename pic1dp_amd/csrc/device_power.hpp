// device_power.hpp -- the wave-particle power on the output grid (include/pic1dp_hip.h pic1dp_hip_power):
// what one marker adds -- the push's gather of E at its wrapped position (device_math.hpp wrap, locate; push_one's two
// products and one sum, from the E tile with its guard cell), c = v e, t_q = c q, and t_q spread over the four cells of the
// output grid's stencil (device_diag.hpp dist_stencil), or into the thread's `rest` sum where the marker has no bins.
// Used by kernels_power.hip, around device_sweep.hpp's pair_sweep.
#pragma once
#include "device_diag.hpp"
#include "device_math.hpp"

namespace pic1dp {
namespace {

// this thread's sums of the terms of markers without bins (|v| >= v_max), per weight set
struct PowerRest {
  double p = 0.0, w = 0.0;
};

// one weight set of one marker: t = c q into the stencil's four cells of plane pl (LDS copy or the global plane), each
// product rounded on its own, in the order c00, c01, c10, c11; no bins: t into the thread's rest sum
template <bool LDS>
__device__ __forceinline__ void power_set(double *pl, const DistStencil &s, bool bins, double t, double &rest) {
  if (!bins) {
    rest += t;
    return;
  }
  bin_add<LDS>(pl + s.c00, s.w00 * t);
  bin_add<LDS>(pl + s.c01, s.w01 * t);
  bin_add<LDS>(pl + s.c10, s.w10 * t);
  bin_add<LDS>(pl + s.c11, s.w11 * t);
}

// one marker.  sE: the workgroup's E tile, nx + 1 cells, cell nx = E[0] (locate folds ix == nx to 0, so ix + 1 <= nx);
// pl: the planes [set][iv * nx_opd + ix] of the pass, nxv = nx_opd nv_opd doubles each
template <bool P, bool W, bool LDS>
__device__ __forceinline__ void power_one(double x, double v, double pp, double pw, const GridConst &g, const DistGeom &dg,
                                          const double *sE, double *pl, int nxv, PowerRest &r) {
  const double px = wrap(x, g.lx);
  int ix;
  double wl;
  locate(px, g, ix, wl);
  double e = sE[ix] * wl;                  // the push's gather, in the push's order (device_math.hpp push_one)
  e = e + sE[ix + 1] * (1.0 - wl);
  const double c = v * e;
  DistStencil s;
  const bool bins = dist_stencil(px, v, dg, s);
  if constexpr (P) power_set<LDS>(pl, s, bins, c * pp, r.p);
  if constexpr (W) power_set<LDS>(pl + (P ? nxv : 0), s, bins, c * pw, r.w);
}

// a thread's rest sum over the workgroup (wave shuffles, then LDS: device_math.hpp block_sum), one global atomic per
// workgroup unless it is zero; scr: 16 doubles
__device__ __forceinline__ void power_rest_flush(double mine, double *scr, double *rest) {
  const double t = block_sum(mine, scr);
  if (threadIdx.x == 0 && t != 0.0) glb_add(rest, t);
}

// the workgroup's planes into the global ones: one global atomic per non-zero word, the start word rotated by workgroup
// (flush_rho's rule); n: the words of the pass's planes, laid out as the global planes are
__device__ __forceinline__ void power_flush(const double *sP, double *planes, int n) {
  rotated_words(n, [&](int j) {
    const double val = sP[j];
    if (val != 0.0) glb_add(&planes[j], val);
  });
}

}  // namespace
}  // namespace pic1dp
