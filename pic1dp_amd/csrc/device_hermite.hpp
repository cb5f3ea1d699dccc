// device_hermite.hpp -- the Fourier-Hermite spectrum of the markers (include/pic1dp_hip.h pic1dp_hip_hermite):
// the recurrence of the orthonormal Hermite polynomials, what one marker contributes to a wave's column tile, the matrix
// products of a trip and the fold of the accumulators.  Used by kernels_hermite.hip and, the recurrence alone, by probe.hip.
#pragma once
#include "device_fxsum.hpp"
#include "device_math.hpp"

namespace pic1dp {
namespace {

typedef double herm_v4d __attribute__((ext_vector_type(4)));
// The tables ra, rb as the sweep reads them: through the constant address space, so a load at a wave-uniform index is a scalar
// load whatever fences lie around it (nothing writes the tables while a kernel runs: the host uploads them once)
typedef const __attribute__((address_space(4))) double *herm_ctab;
__device__ __forceinline__ herm_ctab herm_const_tab(const double *tab) { return (herm_ctab)tab; }
// a tile's hand-off inside a wave: what the lanes wrote before is read by other lanes after, and overwritten only after that
__device__ __forceinline__ void herm_tile_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// psi_(n+1) from (psi_(n-1), psi_n): (u psi_n) ra[n] - psi_(n-1) rb[n], the two products, the scaling and the difference
// each rounded on their own (the build contracts nothing) -- numpy gives the same bits
__device__ __forceinline__ double herm_next(double u, double prev, double cur, double ra, double rb) {
  const double a = u * cur;
  const double b = a * ra;
  const double c = prev * rb;
  return b - c;
}

// psi_0 ... psi_(nherm-1) of one u into out[0 .. nherm), tab: ra[256] then rb[256]
__device__ __forceinline__ void herm_all(double u, int nherm, const double *tab, double *out) {
  double prev = 0.0, cur = 1.0;
  for (int n = 0; n < nherm; ++n) {
    out[n] = cur;
    const double nx = n == 0 ? u : herm_next(u, prev, cur, tab[n], tab[HERM_MAX_N + n]);
    prev = cur, cur = nx;
  }
}

// The columns of one marker into the wave's tile sY[c][lane], c = (set * nmodes + a) * 2 + t: q cos(kk[a] px) and
// q sin(kk[a] px), sets p then w.  px: the deposit's wrap, not stored back.  A tail lane comes with x = 0, q = 0: its columns are 0.
template <bool P, bool W>
__device__ __forceinline__ void herm_columns(double *sY, int lane, double x, double pp, double pw, const HermiteArgs &a) {
  const double px = wrap(x, a.lx);
  for (int m = 0; m < a.nmodes; ++m) {
    double sn, cs;
    sincos(a.kk[m] * px, &sn, &cs);
    if constexpr (P) {
      sY[(2 * m) * HERM_TILE_LD + lane] = pp * cs;
      sY[(2 * m + 1) * HERM_TILE_LD + lane] = pp * sn;
    }
    if constexpr (W) {
      const int c = 2 * ((P ? a.nmodes : 0) + m);
      sY[c * HERM_TILE_LD + lane] = pw * cs;
      sY[(c + 1) * HERM_TILE_LD + lane] = pw * sn;
    }
  }
}

// One trip of a wave, lane = marker: acc[b] += Psi_b Y over the 64 markers, Psi_b[r][i] = psi_(16 b + r)(u_i), Y[i][c] the
// column tile.  v_mfma_f64_16x16x4_f64 takes A[row = lane & 15][k = lane >> 4] and B[k = lane >> 4][col = lane & 15], one
// double per lane, and leaves D[row = (lane >> 4) + 4 reg][col = lane & 15]: sixteen products of four markers a block.
// The tiles are the wave's own; its LDS operations complete in order, and herm_tile_sync keeps the compiler from moving a
// tile's reads across its writes.
template <int NB>
__device__ __forceinline__ void herm_trip(double u, const double *tab, double *sPsi, const double *sY, int lane, herm_v4d (&acc)[NB]) {
  const int frag = (lane & 15) * HERM_TILE_LD + (lane >> 4);
  const herm_ctab ct = herm_const_tab(tab);
  herm_tile_sync();
  double yb[16];
#pragma unroll
  for (int g = 0; g < 16; ++g) yb[g] = sY[frag + 4 * g];
  double prev = 0.0, cur = 1.0;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    // the block's sixteen ra and sixteen rb: scalar loads issued here, block by block (the pointer is opaque to the
    // compiler, so it does not hoist all 2 x 16 NB values out of the sweep and spill them)
    herm_ctab cb = ct + 16 * b;
    asm volatile("" : "+s"(cb));
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = 16 * b + r;
      sPsi[r * HERM_TILE_LD + lane] = cur;
      const double nx = n == 0 ? u : herm_next(u, prev, cur, cb[r], cb[HERM_MAX_N + r]);
      prev = cur, cur = nx;
    }
    herm_tile_sync();
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(sPsi[frag + 4 * g], yb[g], acc[b], 0, 0, 0);
    herm_tile_sync();
  }
}

// a wave's accumulators added into the workgroup's words sG[n * 16 + c] (zeroed, a barrier before and after by the caller)
template <int NB>
__device__ __forceinline__ void herm_fold(const herm_v4d (&acc)[NB], double *sG, int lane) {
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double val = acc[b][r];
      if (val != 0.0) lds_add(&sG[(16 * b + (lane >> 4) + 4 * r) * 16 + (lane & 15)], val);
    }
}

// the workgroup's words into the global ones: one atomic per non-zero word of a row below nherm, the start word rotated by workgroup
__device__ __forceinline__ void herm_flush(const double *sG, double *out, int nherm) {
  rotated_words(nherm * 16, [&](int j) {
    const double val = sG[j];
    if (val != 0.0) glb_add(&out[j], val);
  });
}

}  // namespace
}  // namespace pic1dp
