// device_moments.hpp -- the velocity moments of the markers on the field grid (include/pic1dp_hip.h pic1dp_hip_moments):
// what one marker adds to a workgroup's LDS planes and the flush of the planes -- as doubles (k_moments) and as whole quanta
// in integer planes (k_moments_exact; pic1dp_hip_moments_exact).  Used by kernels_moments.hip, around device_sweep.hpp's
// pair_sweep.  The wrap and the cell come from device_math.hpp as the deposit takes them.
#pragma once
#include "device_fxsum.hpp"
#include "device_math.hpp"

namespace pic1dp {
namespace {

// planes of a weight set in a pass of powers KMASK (bit k: v^k), and where power k lies among them
template <int KMASK>
constexpr int moments_nk() { return __builtin_popcount(static_cast<unsigned>(KMASK)); }
template <int KMASK>
constexpr int moments_slot(int k) { return __builtin_popcount(static_cast<unsigned>(KMASK) & ((1u << k) - 1u)); }

// One weight set of one marker: a0 = wl q, b0 = (1 - wl) q, a_k = a_(k-1) v, every product rounded on its own (the build
// contracts nothing); the powers of KMASK go to cells ix and ir of their planes sM[slot][cell].  The chain runs through
// the powers a pass does not hold, so a term has the same bits whichever pass adds it.
template <int KMASK>
__device__ __forceinline__ void moments_set(double *sM, int nx, int ix, int ir, double wl, double wr, double q, double v) {
  double a = wl * q, b = wr * q;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k > 0) {
      a = a * v;
      b = b * v;
    }
    if ((KMASK >> k) & 1) {
      double *pl = sM + moments_slot<KMASK>(k) * nx;
      lds_add(pl + ix, a);
      lds_add(pl + ir, b);
    }
    if ((KMASK >> (k + 1)) == 0) break;   // (no higher power in this pass)
  }
}

// one marker: the deposit's wrap (not stored back) and cell; the right-hand neighbour of the last cell is cell 0
template <bool P, bool W, int KMASK>
__device__ __forceinline__ void moments_one(double x, double v, double pp, double pw, const GridConst &g, double *sM) {
  const double px = wrap(x, g.lx);
  int ix;
  double wl;
  locate(px, g, ix, wl);
  const int ir = ix + 1 == g.nx ? 0 : ix + 1;
  const double wr = 1.0 - wl;
  if constexpr (P) moments_set<KMASK>(sM, g.nx, ix, ir, wl, wr, pp, v);
  if constexpr (W) moments_set<KMASK>(sM + (P ? moments_nk<KMASK>() * g.nx : 0), g.nx, ix, ir, wl, wr, pw, v);
}

// the planes of a pass, and the power of v that LDS plane l = (set, slot) holds
template <bool P, bool W, int KMASK>
constexpr int moments_npl() { return ((P ? 1 : 0) + (W ? 1 : 0)) * moments_nk<KMASK>(); }
template <int KMASK>
__device__ __forceinline__ int moments_power(int slot) { return KMASK == 0xC ? slot + 2 : slot; }
// the workgroup's planes into the global ones: one global atomic per non-zero word, the start word rotated by workgroup;
// LDS plane l = (set, slot) is power k of that set: out[(set * 4 + k) * nx + cell]
template <bool P, bool W, int KMASK>
__device__ __forceinline__ void moments_flush(const double *sM, double *out, int nx) {
  constexpr int NK = moments_nk<KMASK>();
  rotated_words(moments_npl<P, W, KMASK>() * nx, [&](int j) {
    const double val = sM[j];
    if (val != 0.0) {
      const int l = j / nx, cell = j - l * nx;
      const int set = l / NK, slot = l - set * NK;
      glb_add(&out[static_cast<size_t>(set * 4 + moments_power<KMASK>(slot)) * nx + cell], val);
    }
  });
}

// ---------------------------------------------------------------------------
// The exact kind (include/pic1dp_hip.h pic1dp_hip_moments_exact): the very terms of moments_set, each
// rounded once to whole quanta 2^e[k] and summed as integers.  A workgroup's LDS holds ONE signed 64-bit word per (plane,
// cell), plane-major as the doubles above and byte for byte their size; the flush splits a word into (hi, lo 32 bits)
// and adds the two into the global rows acc[((set 4 + k) 2 + h) nx + cell], h = 0 hi, 1 lo.
// ---------------------------------------------------------------------------
// one term into its word (device_fxsum.hpp fx_word44); 2^44 quanta or more, or a NaN, is not summed but counted in *rej
__device__ __forceinline__ void mfx_term(unsigned long long *word, double term, double inv_q, unsigned long long *rej) {
  unsigned long long n;
  if (!fx_word44(term, inv_q, &n)) {
    fx_glb_add(rej, 1ull);
    return;
  }
  __hip_atomic_fetch_add(word, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// moments_set with integer planes; rej: this weight set's four counters, by power of v
template <int KMASK>
__device__ __forceinline__ void mfx_set(unsigned long long *sM, int nx, int ix, int ir, double wl, double wr, double q, double v,
                                        const MomentsFxArgs &fx, unsigned long long *rej) {
  double a = wl * q, b = wr * q;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k > 0) {
      a = a * v;
      b = b * v;
    }
    if ((KMASK >> k) & 1) {
      unsigned long long *pl = sM + moments_slot<KMASK>(k) * nx;
      mfx_term(pl + ix, a, fx.inv_q[k], rej + k);
      mfx_term(pl + ir, b, fx.inv_q[k], rej + k);
    }
    if ((KMASK >> (k + 1)) == 0) break;   // (no higher power in this pass)
  }
}
template <bool P, bool W, int KMASK>
__device__ __forceinline__ void mfx_one(double x, double v, double pp, double pw, const GridConst &g, unsigned long long *sM,
                                        const MomentsFxArgs &fx) {
  const double px = wrap(x, g.lx);
  int ix;
  double wl;
  locate(px, g, ix, wl);
  const int ir = ix + 1 == g.nx ? 0 : ix + 1;
  const double wr = 1.0 - wl;
  unsigned long long *rej = reinterpret_cast<unsigned long long *>(fx.rej);
  if constexpr (P) mfx_set<KMASK>(sM, g.nx, ix, ir, wl, wr, pp, v, fx, rej);
  if constexpr (W) mfx_set<KMASK>(sM + (P ? moments_nk<KMASK>() * g.nx : 0), g.nx, ix, ir, wl, wr, pw, v, fx, rej + (P ? 4 : 0));
}
// the workgroup's words into the global (hi, lo) rows, zeroed on the way: two non-returning 64-bit integer atomics per
// non-zero word, the start word rotated by workgroup; the caller puts barriers around it
template <bool P, bool W, int KMASK>
__device__ __forceinline__ void mfx_flush(unsigned long long *sM, const MomentsFxArgs &fx, int nx) {
  constexpr int NK = moments_nk<KMASK>();
  unsigned long long *acc = reinterpret_cast<unsigned long long *>(fx.acc);
  rotated_words(moments_npl<P, W, KMASK>() * nx, [&](int j) {
    const unsigned long long w = sM[j];
    if (w == 0ull) return;
    sM[j] = 0ull;
    const int l = j / nx, cell = j - l * nx;
    const int set = l / NK, slot = l - set * NK;
    unsigned long long *row = acc + static_cast<size_t>(set * 4 + moments_power<KMASK>(slot)) * 2 * nx + cell;
    fx_add_limbs(row, row + nx, w);
  });
}

}  // namespace
}  // namespace pic1dp
