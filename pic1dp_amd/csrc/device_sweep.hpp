// device_sweep.hpp -- the one sweep of the off-path marker kernels over a workgroup's rows of marker pairs (k_ptcldist,
// k_ptcldist_exact: kernels_diag.hip; k_moments, k_moments_exact: kernels_moments.hip; k_power, k_power_exact:
// kernels_power.hip; k_zoom: kernels_zoom.hip), and the window rule of the exact kernels around it.  The rows and the drawn chunks themselves are device_math.hpp's (pair_rows, draw_chunk): the
// step kernels use them too.
#pragma once
#include "device_math.hpp"

namespace pic1dp {
namespace {

// A workgroup's rows of marker pairs (device_math.hpp pair_rows), the last dyn_tail / 16 of them drawn chunk by chunk by
// its waves: with one workgroup of sixteen waves per CU, the waves that are done would idle a quarter of the CU each.
// Pairs as double2 (the marker kernels' access shape), the NEXT trip's loads issued before this trip's work, non-temporal
// loads where NT says so (round 5, kernels_diag.hip).  x and v are always loaded, p where P, w where W: an array a pass
// does not need is not read, and its argument of `one` is 0.  one(x, v, p, w) per marker; after_trip(k) once per trip, k
// the trips done.
template <bool P, bool W, bool NT, class One, class After>
__device__ __forceinline__ void pair_sweep(const double *x, const double *v, const double *p, const double *w, int64_t npair,
                                           const PairRows &rows, unsigned *sDraw, One &&one, After &&after_trip) {
  const double2 *x2 = reinterpret_cast<const double2 *>(x), *v2 = reinterpret_cast<const double2 *>(v);
  const double2 *p2 = reinterpret_cast<const double2 *>(p), *w2 = reinterpret_cast<const double2 *>(w);
  int k = 0;
  int64_t j = rows.first + threadIdx.x;
  bool have = rows.dealt > 0 || draw_chunk(rows, sDraw, j);
  double2 X = make_double2(0.0, 0.0), V = X, Pq = X, Wq = X;
  if (have && j < npair) {
    const int64_t o = tidx2(j);
    X = ld2t<NT>(x2 + o), V = ld2t<NT>(v2 + o);
    if constexpr (P) Pq = ld2t<NT>(p2 + o);
    if constexpr (W) Wq = ld2t<NT>(w2 + o);
  }
  while (have) {
    int64_t jn = j + rows.stride;
    bool have_n = true;
    if (++k >= rows.dealt) have_n = draw_chunk(rows, sDraw, jn);
    double2 Xn = make_double2(0.0, 0.0), Vn = Xn, Pn = Xn, Wn = Xn;
    if (have_n && jn < npair) {  // the next trip's loads are under way while this trip's atomics run
      const int64_t o = tidx2(jn);
      Xn = ld2t<NT>(x2 + o), Vn = ld2t<NT>(v2 + o);
      if constexpr (P) Pn = ld2t<NT>(p2 + o);
      if constexpr (W) Wn = ld2t<NT>(w2 + o);
    }
    if (j < npair) {
      one(X.x, V.x, Pq.x, Wq.x);
      one(X.y, V.y, Pq.y, Wq.y);
    }
    after_trip(k);
    X = Xn, V = Vn, Pq = Pn, Wq = Wn;
    j = jn;
    have = have_n;
  }
}

// The window of the exact kernels, whose LDS holds ONE signed 64-bit word per sum (device_fxsum.hpp).  A workgroup
// flushes its words into the global (hi, lo) rows after every DIAG_FX_WINDOW_TRIPS dealt trips (window_due) and once at
// the end; the drawn rows are capped one below that (window_rows: the surplus is dealt instead), and the kernel takes the
// odd last marker BEFORE the sweep, so it falls into the first window.  Between two flushes a word therefore sees at most
// DIAG_FX_WINDOW_TRIPS trips of 2 x 1024 markers and that marker, or DIAG_FX_WINDOW_TRIPS - 1 dealt and as many drawn
// trips: fewer than 2^17 markers.  A marker adds at most 4 terms to a word in the histograms (its four corners in one
// bin), at most 2 in the moments (nx = 1: ix == ir), each below 2^44 quanta (DIAG_FX_LIMIT): fewer than 2^19 terms, the
// word stays below 2^63 in magnitude in the histograms and below 2^62 in the moments.  The exact power (device_power.hpp
// pfx_*) is the histograms' case: at most 4 terms of a marker in one word (nx_opd = 1 with the top v row keeping the marker),
// 4 x 2^17 x 2^44 = 2^63 -- the STRICT inequality in the marker count is what keeps the word inside.  Its rest sums take one
// term per marker: a thread's register sum and the workgroup's LDS word of a window stay below 2^17 x 2^44 = 2^61.  The zoomed
// histogram (device_zoom.hpp; k_zoom) is the same case: one term per marker into a word of its plane, each below 2^44 quanta
// (markr: 1), fewer than 2^17 markers between two flushes -- a word stays below 2^61; its bounds need no new argument.  The cap,
// the cadence and the place of the odd marker carry these bounds together: change none of them alone.
// The dealt trips are the same number for every thread of a workgroup, so window_due is uniform over it and the barriers
// a kernel puts around its flush inside the sweep are met by all.
__device__ __forceinline__ PairRows window_rows(PairRows rows) {
  const int waves = static_cast<int>(blockDim.x >> 6);
  const int extra = rows.drawn_total / waves - (DIAG_FX_WINDOW_TRIPS - 1);
  if (extra > 0) {
    rows.dealt += extra;
    rows.drawn_total -= extra * waves;
  }
  return rows;
}
// k: the trips done, as pair_sweep hands them to after_trip
__device__ __forceinline__ bool window_due(int k, const PairRows &rows) {
  return k <= rows.dealt && (k & (DIAG_FX_WINDOW_TRIPS - 1)) == 0;
}

}  // namespace
}  // namespace pic1dp
