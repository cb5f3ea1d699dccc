// zoom_fx.hpp -- host arithmetic of the exact phase-space histogram on a caller's window and grid (include/pic1dp_hip.h
// pic1dp_hip_zoom): the argument checks, the window's geometry (formed once, on the host), the rule for one
// marker -- the kernel's form is device_zoom.hpp, held against this one bit for bit by the tests --, the rule over host
// arrays, and the normalisation and conversion of the (hi, lo) limbs over fx_limbs.hpp.  No context, no HIP call
// (zoom_fx.cpp): the entry points of capi_zoom.cpp share it, and a stand-alone program runs it under the host's sanitizers
// (tests/zoom_fx_check.cpp).
// Limbs: [plane j of the selected][h: 0 hi, 1 lo][jv][ix]; planes in the order markr (which & 1), total (& 2), pertb (& 4).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/pic1dp_hip.h"
#include "kernels.hpp"

namespace pic1dp_host {

// planes a mask selects (which in 1..7)
inline int zoom_planes(int which) { return (which & 1) + ((which >> 1) & 1) + ((which >> 2) & 1); }
// why a window and grid cannot be served (null: they can); lx: the box
const char *zoom_refusal(const pic1dp_zoom &z, double lx);
// Lw, sx, sv and the straddle flag of an accepted window
pic1dp::ZoomGeom zoom_geom(const pic1dp_zoom &z, double lx);
// the rule for one valid marker: false outside the window (a NaN px or v is never inside), else *cell = jv nxb + ix
bool zoom_cell(const pic1dp::ZoomGeom &g, double x, double v, int *cell);
// the rule over host arrays of np valid markers: limbs (normalised) of the terms summed, rejected[3] the terms not summed per
// plane markr, total, pertb (2^44 quanta of 2^e or more, NaN); e_p, e_w: the log2 quanta of total and pertb; p / w are read
// only where which selects their plane
void zoom_host_sums(const pic1dp::ZoomGeom &g, int which, int e_p, int e_w, const double *x, const double *v, const double *p,
                    const double *w, int64_t np, int64_t *limbs, int64_t rejected[3]);
// limbs [nplanes][2][cells] (lo any 64-bit pattern, read as unsigned): hi += lo >> 32, lo &= 2^32 - 1, in place
void zoom_fx_normalise(int64_t *limbs, int nplanes, size_t cells);
// out [nplanes][cells]: every cell's total (hi 2^32 + lo) quanta converted once (round to nearest even) and multiplied by
// 2^e of its plane (e[0] markr = 0, e[1] total, e[2] pertb); the limbs need not be normalised
void zoom_fx_convert(const int32_t e[3], int which, const int64_t *limbs, size_t cells, double *out);

}  // namespace pic1dp_host
