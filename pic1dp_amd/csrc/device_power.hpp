// device_power.hpp -- the wave-particle power on the output grid (include/pic1dp_hip.h pic1dp_hip_power):
// what one marker adds -- the push's gather of E at its wrapped position (device_math.hpp wrap, locate; push_one's two
// products and one sum, from the E tile with its guard cell), c = v e, t_q = c q, and t_q spread over the four cells of the
// output grid's stencil (device_diag.hpp dist_stencil), or into the thread's `rest` sum where the marker has no bins.
// The exact kind (pic1dp_hip_power_exact) below it: the same terms as whole quanta in integer planes (pfx_*).
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

// ---------------------------------------------------------------------------
// The exact kind (include/pic1dp_hip.h pic1dp_hip_power_exact): the very terms of power_one, each rounded
// once to whole quanta 2^e and summed as integers (device_fxsum.hpp).  A workgroup's LDS holds, behind the E tile, ONE
// signed 64-bit word per (set, bin), plane-major as the doubles above and byte for byte their size; that a word cannot
// overflow between two flushes is the window rule of device_sweep.hpp.  Global rows per weight set (kernels.hpp
// PowerFxArgs): [hi plane | lo plane | rest hi | rest lo] -- a set's rows are DistBinsFx's with one plane (k = 0).
// ---------------------------------------------------------------------------
// the bits of max |E[0 .. nx)| over the workgroup, staged into the tile on the way (cell nx = E[0]); sMax: one LDS word.
// Every thread gets the same value; the tile is complete when this returns.
__device__ __forceinline__ unsigned long long pfx_stage_tile(const double *E, double *sE, int nx, unsigned long long *sMax) {
  if (threadIdx.x == 0) *sMax = 0ull;
  __syncthreads();
  unsigned long long m = 0ull;
  for (int i = threadIdx.x; i < nx; i += blockDim.x) {
    const double e = E[i];
    sE[i] = e;
    if (i == 0) sE[nx] = e;   // cell nx is cell 0
    const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(e)) & 0x7fffffffffffffffull;
    m = b > m ? b : m;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(m, off, 64);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0 && m) __hip_atomic_fetch_max(sMax, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  return *sMax;
}

// this thread's integer sums of the terms of markers without bins, per weight set: below 2^61 quanta in magnitude between
// two flushes, as the workgroup's (device_sweep.hpp)
struct PowerRestFx {
  unsigned long long p = 0ull, w = 0ull;
};

// one weight set of one marker; b: the set's rows (LDS: b.s its plane of words); rej: the set's two counters (bins, rest)
template <bool LDS>
__device__ __forceinline__ void pfx_set(const DistBinsFx &b, const DistStencil &s, bool bins, double t, double inv_q,
                                        unsigned long long &rest, unsigned long long *rej) {
  unsigned long long n;
  if (!bins) {
    if (fx_word44(t, inv_q, &n)) rest += n;
    else fx_glb_add(rej + 1, 1ull);
    return;
  }
  const int cell[4] = {s.c00, s.c01, s.c10, s.c11};
  const double wt[4] = {s.w00, s.w01, s.w10, s.w11};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (!fx_word44(wt[c] * t, inv_q, &n)) {
      fx_glb_add(rej, 1ull);
    } else if constexpr (LDS) {
      __hip_atomic_fetch_add(&b.s[cell[c]], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
      dfx_limbs_add(b, 0, cell[c], n);
    }
  }
}

// power_one with integer sums.  sP: the pass's LDS planes [set][nxv] (unused where !LDS); acc, rej: the rows and counters
// of the pass's first weight set
template <bool P, bool W, bool LDS>
__device__ __forceinline__ void pfx_one(double x, double v, double pp, double pw, const GridConst &g, const DistGeom &dg,
                                        const double *sE, unsigned long long *sP, unsigned long long *acc, unsigned long long *rej,
                                        int nxv, double inv_q, PowerRestFx &r) {
  const double px = wrap(x, g.lx);
  int ix;
  double wl;
  locate(px, g, ix, wl);
  double e = sE[ix] * wl;                  // power_one's gather
  e = e + sE[ix + 1] * (1.0 - wl);
  const double c = v * e;
  DistStencil s;
  const bool bins = dist_stencil(px, v, dg, s);
  const size_t setw = 2 * static_cast<size_t>(nxv) + 2;
  if constexpr (P) pfx_set<LDS>(DistBinsFx{sP, acc, nxv}, s, bins, c * pp, inv_q, r.p, rej);
  if constexpr (W) pfx_set<LDS>(DistBinsFx{sP + (P ? nxv : 0), acc + (P ? setw : 0), nxv}, s, bins, c * pw, inv_q, r.w, rej + (P ? 2 : 0));
}

// the workgroup's words into the global rows, zeroed on the way (start word rotated by workgroup), and the threads' rest
// sums, wave by wave, into the LDS words sR[set], zeroed too; the caller puts barriers around it and calls pfx_rest_out
// behind the second
template <bool P, bool W, bool LDS>
__device__ __forceinline__ void pfx_flush(unsigned long long *sP, unsigned long long *acc, int nxv, PowerRestFx &r, unsigned long long *sR) {
  constexpr int NS = (P ? 1 : 0) + (W ? 1 : 0);
  const size_t setw = 2 * static_cast<size_t>(nxv) + 2;
  if constexpr (LDS)
    rotated_words(NS * nxv, [&](int j) {
      const unsigned long long w = sP[j];
      if (w == 0ull) return;
      sP[j] = 0ull;
      const int set = j >= nxv ? 1 : 0;
      dfx_limbs_add(DistBinsFx{nullptr, acc + set * setw, nxv}, 0, j - set * nxv, w);
    });
  unsigned long long mine[2] = {P ? r.p : r.w, r.w};
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    unsigned long long t = mine[k];
    for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
    if ((threadIdx.x & 63) == 0 && t) __hip_atomic_fetch_add(&sR[k], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  r.p = r.w = 0ull;
}
// the workgroup's rest words into the (rest hi, rest lo) pairs behind the sets' planes, zeroed on the way
template <int NS>
__device__ __forceinline__ void pfx_rest_out(unsigned long long *sR, unsigned long long *acc, int nxv) {
  if (threadIdx.x < NS) {
    const unsigned long long w = sR[threadIdx.x];
    if (w) {
      sR[threadIdx.x] = 0ull;
      unsigned long long *pair = acc + threadIdx.x * (2 * static_cast<size_t>(nxv) + 2) + 2 * static_cast<size_t>(nxv);
      fx_add_limbs(pair, pair + 1, w);
    }
  }
}

}  // namespace
}  // namespace pic1dp
