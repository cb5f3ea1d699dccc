// zoom_fx.cpp -- host arithmetic of the exact phase-space histogram on a caller's window and grid (zoom_fx.hpp).  No HIP call.
#include "zoom_fx.hpp"

#include <cmath>

#include "fx_limbs.hpp"
#include "select_rule.hpp"

namespace pic1dp_host {

using pic1dp::ZoomGeom;

const char *zoom_refusal(const pic1dp_zoom &z, double lx) {
  if (!std::isfinite(z.x_lo) || !std::isfinite(z.x_hi) || !std::isfinite(z.v_lo) || !std::isfinite(z.v_hi))
    return "a bound of the window is not finite (a grid needs a finite extent)";
  if (!(z.x_lo >= 0.0 && z.x_lo <= lx && z.x_hi >= 0.0 && z.x_hi <= lx)) return "x_lo and x_hi must lie in [0, lx]";
  if (!(z.v_lo < z.v_hi)) return "v_lo < v_hi required";
  if (z.nxb < 1 || z.nvb < 1 || z.nxb > pic1dp::ZOOM_MAX_BINS || z.nvb > pic1dp::ZOOM_MAX_BINS)
    return "nxb and nvb must lie in 1..4096";
  if (static_cast<int64_t>(z.nxb) * z.nvb > pic1dp::ZOOM_MAX_CELLS) return "nxb * nvb must not exceed 2^20";
  const ZoomGeom g = zoom_geom(z, lx);
  if (!std::isfinite(z.v_hi - z.v_lo) || !std::isfinite(g.sv) || (z.x_lo != z.x_hi && !std::isfinite(g.sx)))
    return "the window's extent overflows, or is too small for cells per unit length to be finite";
  return nullptr;
}

ZoomGeom zoom_geom(const pic1dp_zoom &z, double lx) {
  ZoomGeom g{};
  g.lx = lx;
  g.x_lo = z.x_lo, g.x_hi = z.x_hi, g.v_lo = z.v_lo, g.v_hi = z.v_hi;
  g.nxb = z.nxb, g.nvb = z.nvb;
  g.straddle = z.x_lo > z.x_hi ? 1 : 0;
  const double Lw = g.straddle ? (z.x_hi + lx) - z.x_lo : z.x_hi - z.x_lo;
  g.sx = static_cast<double>(z.nxb) / Lw;   // (x_lo == x_hi: the empty window, no marker is looked at)
  g.sv = static_cast<double>(z.nvb) / (z.v_hi - z.v_lo);
  return g;
}

bool zoom_cell(const ZoomGeom &g, double x, double v, int *cell) {
  const double px = pic1dp::select_wrap(x, g.lx);
  const bool in_x = g.straddle ? (px >= g.x_lo || px < g.x_hi) : (g.x_lo <= px && px < g.x_hi);
  if (!in_x || !(g.v_lo <= v && v < g.v_hi)) return false;
  double d = px - g.x_lo;
  if (d < 0.0) d = d + g.lx;
  int ix = static_cast<int>(d * g.sx);
  if (ix > g.nxb - 1) ix = g.nxb - 1;
  int jv = static_cast<int>((v - g.v_lo) * g.sv);
  if (jv > g.nvb - 1) jv = g.nvb - 1;
  *cell = jv * g.nxb + ix;
  return true;
}

namespace {

// n quanta into a normalised (hi, lo) pair, kept normalised
inline void limbs_add(int64_t *hi, int64_t *lo, int64_t n) {
  const uint64_t u = static_cast<uint64_t>(n);
  const uint64_t l = static_cast<uint64_t>(*lo) + (u & 0xffffffffull);   // below 2^33
  *hi = static_cast<int64_t>(static_cast<uint64_t>(*hi) + static_cast<uint64_t>(n >> 32) + (l >> 32));
  *lo = static_cast<int64_t>(l & 0xffffffffull);
}

}  // namespace

void zoom_host_sums(const ZoomGeom &g, int which, int e_p, int e_w, const double *x, const double *v, const double *p,
                    const double *w, int64_t np, int64_t *limbs, int64_t rejected[3]) {
  const size_t cells = static_cast<size_t>(g.nxb) * g.nvb;
  const int nplanes = zoom_planes(which);
  for (size_t i = 0; i < 2 * cells * nplanes; ++i) limbs[i] = 0;
  rejected[0] = rejected[1] = rejected[2] = 0;
  if (g.x_lo == g.x_hi) return;   // the empty window
  const double inv_q[3] = {1.0, std::ldexp(1.0, -e_p), std::ldexp(1.0, -e_w)};
  const double *term[3] = {nullptr, p, w};
  for (int64_t i = 0; i < np; ++i) {
    int c = 0;
    if (!zoom_cell(g, x[i], v[i], &c)) continue;
    int j = 0;
    for (int k = 0; k < 3; ++k) {
      if (!(which & (1 << k))) continue;
      int64_t *hi = limbs + static_cast<size_t>(2 * j) * cells + c;
      ++j;
      long long n = 1;
      if (k > 0 && !pic1dp::diag_fx_quantise(term[k][i], inv_q[k], pic1dp::DIAG_FX_LIMIT, &n)) {
        rejected[k]++;
        continue;
      }
      limbs_add(hi, hi + cells, n);
    }
  }
}

void zoom_fx_normalise(int64_t *limbs, int nplanes, size_t cells) {
  for (int j = 0; j < nplanes; ++j) fx_row_normalise(limbs + static_cast<size_t>(2 * j) * cells, limbs + static_cast<size_t>(2 * j + 1) * cells, cells);
}

void zoom_fx_convert(const int32_t e[3], int which, const int64_t *limbs, size_t cells, double *out) {
  int j = 0;
  for (int k = 0; k < 3; ++k) {
    if (!(which & (1 << k))) continue;
    fx_row_to_double(limbs + static_cast<size_t>(2 * j) * cells, limbs + static_cast<size_t>(2 * j + 1) * cells, cells, std::ldexp(1.0, e[k]),
                     out + static_cast<size_t>(j) * cells);
    ++j;
  }
}

}  // namespace pic1dp_host
