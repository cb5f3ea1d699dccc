// device_select.hpp -- the kernels' form of the marker selection (include/pic1dp_hip.h pic1dp_hip_select):
// the rule for one marker (the host's form: select_rule.hpp, held against this one bit for bit by the tests), and the one
// sweep of the count pass and the write pass over a workgroup's chunks.  Used by kernels_select.hip.
#pragma once
#include "device_math.hpp"
#include "load_seq.hpp"

namespace pic1dp {
namespace {

// is valid marker i, at (x, v), selected?  px = wrap(x) as the deposit wraps (device_math.hpp), not stored; every comparison
// is false for a NaN px or v; the hash (load_seq.hpp load_draw: the splitmix64 draw g of `key`) only where the window holds
__device__ __forceinline__ bool select_one(double x, double v, int64_t i, const SelectRule &r) {
  const double px = wrap(x, r.lx);
  const bool in_x = r.straddle ? (px >= r.x_lo || px < r.x_hi) : (r.x_lo <= px && px < r.x_hi);
  if (!in_x || !(r.v_lo <= v && v < r.v_hi)) return false;
  if (r.thin == 0ull) return true;
  return load_draw(r.key, r.origin + static_cast<unsigned long long>(i)) < r.thin;
}

// The chunks a workgroup takes, grid-stride over the chunks `want` accepts (a uniform answer: every thread asks the same),
// each in trips of blockDim.x pairs: pairs as double2 through tidx2 (a wave's 64 pairs lie in one tile), the NEXT trip's
// loads -- of this chunk or of the workgroup's next one -- issued before this trip's work, non-temporal where NT says so.
// trip(c, j, valid, X, V) once per trip and thread, j the thread's pair, valid: j lies in chunk c (else X = V = 0);
// end_chunk(c) after a chunk's last trip.  Both are called by every thread of the workgroup alike, so they may hold
// barriers and ballots.  A chunk without pairs (np = 1) has one trip with no valid pair.
template <bool NT, class Want, class Trip, class End>
__device__ __forceinline__ void select_sweep(const double *x, const double *v, int64_t npair, int64_t nchunk, Want &&want,
                                             Trip &&trip, End &&end_chunk) {
  const double2 *x2 = reinterpret_cast<const double2 *>(x), *v2 = reinterpret_cast<const double2 *>(v);
  const int64_t T = blockDim.x, G = gridDim.x;
  auto next_chunk = [&](int64_t c) {
    while (c < nchunk && !want(c)) c += G;
    return c;
  };
  auto chunk_end = [&](int64_t c) {
    const int64_t e = (c + 1) * SELECT_CHUNK_PAIRS;
    return e < npair ? e : npair;
  };
  auto load = [&](int64_t c, int64_t t0, double2 &X, double2 &V) {
    X = V = make_double2(0.0, 0.0);
    if (c >= nchunk) return;
    const int64_t j = t0 + threadIdx.x;
    if (j < chunk_end(c)) {
      const int64_t o = tidx2(j);
      X = ld2t<NT>(x2 + o), V = ld2t<NT>(v2 + o);
    }
  };
  int64_t c = next_chunk(blockIdx.x), t0 = c * SELECT_CHUNK_PAIRS;
  double2 X, V;
  load(c, t0, X, V);
  while (c < nchunk) {
    const int64_t e = chunk_end(c);
    int64_t cn = c, tn = t0 + T;
    const bool last = tn >= e;
    if (last) {
      cn = next_chunk(c + G);
      tn = cn * SELECT_CHUNK_PAIRS;
    }
    double2 Xn, Vn;
    load(cn, tn, Xn, Vn);
    const int64_t j = t0 + threadIdx.x;
    trip(c, j, j < e, X, V);
    if (last) end_chunk(c);
    X = Xn, V = Vn;
    c = cn, t0 = tn;
  }
}

}  // namespace
}  // namespace pic1dp
