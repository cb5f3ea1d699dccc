// device_zoom.hpp -- the exact phase-space histogram on a caller's window and grid (include/pic1dp_hip.h pic1dp_hip_zoom;
// DESIGN.md 2.20): the rule for one marker as the kernel takes it -- the host's form is zoom_fx.cpp zoom_cell, held against
// this one bit for bit by the tests --, what the marker adds, and the flush of a workgroup's band.  A pass owns a band of
// whole v rows [r0, r0 + rows) of the selected planes, ONE signed 64-bit word per (plane, cell) in the workgroup's LDS
// (device_fxsum.hpp; the window rule: device_sweep.hpp), or -- !LDS -- every row, the terms straight in the global (hi, lo)
// rows.  Used by kernels_zoom.hip, around device_sweep.hpp's pair_sweep.
#pragma once
#include "device_fxsum.hpp"
#include "device_math.hpp"

namespace pic1dp {
namespace {

// the marker's v row inside the band, jr = jv - r0: v against the window, jv against the band's rows -- two compares, one
// difference and one product, before any wrap; false for a NaN v
__device__ __forceinline__ bool zoom_row(double v, const ZoomGeom &g, int r0, int rows, int &jr) {
  if (!(g.v_lo <= v && v < g.v_hi)) return false;
  int jv = static_cast<int>((v - g.v_lo) * g.sv);
  if (jv > g.nvb - 1) jv = g.nvb - 1;   // (the product may reach nvb just below v_hi)
  jr = jv - r0;
  return jr >= 0 && jr < rows;
}

// the marker's column: px = wrap(x) as the deposit wraps (device_math.hpp; pic1dp_hip_select's), not stored; false outside
// the x window and for a NaN px
__device__ __forceinline__ bool zoom_col(double x, const ZoomGeom &g, int &ix) {
  const double px = wrap(x, g.lx);
  const bool in_x = g.straddle ? (px >= g.x_lo || px < g.x_hi) : (g.x_lo <= px && px < g.x_hi);
  if (!in_x) return false;
  double d = px - g.x_lo;
  if (d < 0.0) d = d + g.lx;
  ix = static_cast<int>(d * g.sx);
  if (ix > g.nxb - 1) ix = g.nxb - 1;
  return true;
}

// where a pass sums: the band's words [plane of the pass][rows nxb] (LDS), or the call's global rows (kernels.hpp ZoomArgs)
struct ZoomSums {
  unsigned long long *s;     // the LDS words; unused where !LDS
  unsigned long long *acc;   // [planes][2][cells]
  unsigned long long *rej;   // [3]
  int band;                  // rows nxb: words of one plane in the band
  int cells;                 // nvb nxb
};

// n quanta into plane j of the pass at cell c of the band (!LDS: the band is the plane)
template <bool LDS>
__device__ __forceinline__ void zoom_add(const ZoomSums &z, int j, int c, unsigned long long n) {
  if constexpr (LDS) {
    __hip_atomic_fetch_add(&z.s[j * z.band + c], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  } else {
    unsigned long long *hi = z.acc + static_cast<size_t>(2 * j) * z.cells + c;
    fx_add_limbs(hi, hi + z.cells, n);
  }
}

// one marker: the row test, then the wrap and the column, then the terms -- 1 to markr, p to total, w to pertb, each plane
// judging its own term.  get_p / get_w hand out the marker's p and w (registers, or loads made only now).
template <bool M, bool P, bool W, bool LDS, class GetP, class GetW>
__device__ __forceinline__ void zoom_one(double x, double v, const ZoomGeom &g, int r0, int rows, const ZoomSums &z, double inv_q_p,
                                         double inv_q_w, GetP &&get_p, GetW &&get_w) {
  int jr, ix;
  if (!zoom_row(v, g, r0, rows, jr)) return;
  if (!zoom_col(x, g, ix)) return;
  const int c = jr * g.nxb + ix;
  int j = 0;
  unsigned long long n;
  if constexpr (M) zoom_add<LDS>(z, j++, c, 1ull);
  if constexpr (P) {
    if (fx_word44(get_p(), inv_q_p, &n)) zoom_add<LDS>(z, j, c, n);
    else fx_glb_add(z.rej + 1, 1ull);
    ++j;
  }
  if constexpr (W) {
    if (fx_word44(get_w(), inv_q_w, &n)) zoom_add<LDS>(z, j, c, n);
    else fx_glb_add(z.rej + 2, 1ull);
  }
}

// the workgroup's band into the global rows, zeroed on the way (start word rotated by workgroup); the caller puts barriers
// around it.  nplanes: planes of the pass; row0: the band's first cell in a plane, r0 nxb
__device__ __forceinline__ void zoom_flush(const ZoomSums &z, int nplanes, int row0) {
  rotated_words(nplanes * z.band, [&](int k) {
    const unsigned long long w = z.s[k];
    if (w == 0ull) return;
    z.s[k] = 0ull;
    const int j = k / z.band;
    unsigned long long *hi = z.acc + static_cast<size_t>(2 * j) * z.cells + row0 + (k - j * z.band);
    fx_add_limbs(hi, hi + z.cells, w);
  });
}

}  // namespace
}  // namespace pic1dp
