// kernels_hermite.hip -- off the timed path: the Fourier-Hermite spectrum of a species' markers (include/pic1dp_hip.h
// pic1dp_hip_hermite), G[n][c] = sum_i psi_n(u_i) Y[i][c] -- a matrix product over the marker index, summed
// by the FP64 matrix unit (v_mfma_f64_16x16x4_f64) in accumulator registers.  One streaming pass (launch_policy.cpp
// hermite_plan): workgroups of four waves, every wave sweeps chunks of 64 markers, lane = marker, through two LDS tiles of
// its own.  gfx950, wave64.
#include "device_hermite.hpp"

#include <type_traits>
#include "launch_policy.hpp"

namespace pic1dp {

namespace {

struct HermMarker {
  double x, v, p, w;
};
// marker c * 64 + lane of the species, or zeros for a tail lane: what a tail slot holds is not read
template <bool P, bool W, bool NT>
__device__ __forceinline__ HermMarker herm_load(const double *x, const double *v, const double *p, const double *w, int64_t np,
                                                int64_t c, int lane, bool &valid) {
  HermMarker m{0.0, 0.0, 0.0, 0.0};
  const int64_t i = c * 64 + lane;
  valid = i < np;
  if (valid) {
    const int64_t o = tidx(i);
    if constexpr (NT) {
      m.x = __builtin_nontemporal_load(x + o), m.v = __builtin_nontemporal_load(v + o);
      if constexpr (P) m.p = __builtin_nontemporal_load(p + o);
      if constexpr (W) m.w = __builtin_nontemporal_load(w + o);
    } else {
      m.x = x[o], m.v = v[o];
      if constexpr (P) m.p = p[o];
      if constexpr (W) m.w = w[o];
    }
  }
  return m;
}

// P, W: the weight sets (both: p's columns first); NB: blocks of sixteen Hermite rows in the accumulators, 8 NB registers.
// Dynamic LDS: per wave the column tile Y[16][64] and a block of Psi[16][64], rows HERM_TILE_LD doubles apart; at the end
// the same bytes hold the workgroup's words [16 NB][16].  Chunk c of 64 markers goes to wave c mod (all waves), the next
// chunk's loads issued before this chunk's arithmetic.  A tail lane (marker index >= np) has u = 0 and q = 0: psi stays
// finite and its columns are zero whatever the slot holds.
template <bool P, bool W, int NB, bool NT>
__global__ void __launch_bounds__(256)
k_hermite(const double *x, const double *v, const double *p, const double *w, int64_t np, const HermiteArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  double *sY = reinterpret_cast<double *>(smem) + static_cast<size_t>(wave) * (2 * 16 * HERM_TILE_LD);
  double *sPsi = sY + 16 * HERM_TILE_LD;
  for (int i = lane; i < 16 * HERM_TILE_LD; i += 64) sY[i] = 0.0;   // the columns nobody writes stay zero
  herm_v4d acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = herm_v4d{0.0, 0.0, 0.0, 0.0};
  const int64_t nchunk = (np + 63) >> 6, stride = static_cast<int64_t>(gridDim.x) * waves;
  int64_t c = static_cast<int64_t>(blockIdx.x) * waves + wave;
  bool valid = false, valid_n = false;
  HermMarker m{0.0, 0.0, 0.0, 0.0};
  if (c < nchunk) m = herm_load<P, W, NT>(x, v, p, w, np, c, lane, valid);
  while (c < nchunk) {
    const int64_t cn = c + stride;
    HermMarker mn{0.0, 0.0, 0.0, 0.0};
    valid_n = false;
    if (cn < nchunk) mn = herm_load<P, W, NT>(x, v, p, w, np, cn, lane, valid_n);
    const double d = m.v - a.v0;
    const double u = valid ? d * a.ivt : 0.0;
    herm_columns<P, W>(sY, lane, m.x, m.p, m.w, a);
    herm_trip<NB>(u, a.tab, sPsi, sY, lane, acc);
    m = mn, valid = valid_n, c = cn;
  }
  __syncthreads();
  double *sG = reinterpret_cast<double *>(smem);
  for (int i = threadIdx.x; i < NB * 256; i += blockDim.x) sG[i] = 0.0;
  __syncthreads();
  herm_fold<NB>(acc, sG, lane);
  __syncthreads();
  herm_flush(sG, a.acc, a.nherm);
}

// what the kernel indexes must be what the plan sized
bool check_plan(const HermitePlan &pl, const HermiteArgs &a, int sets) {
  const int waves = pl.threads / 64;
  return (pl.nb == 4 || pl.nb == 8 || pl.nb == 16) && a.nherm >= 1 && a.nherm <= 16 * pl.nb && a.nmodes >= 1 &&
         sets * a.nmodes * 2 <= HERM_MAX_COLS && pl.threads == 256 && pl.blocks >= 1 && pl.bytes == HERM_WAVE_LDS * waves &&
         sizeof(double) * 256 * pl.nb <= pl.bytes && a.tab && a.acc;
}

}  // namespace

hipError_t launch_hermite(const double *x, const double *v, const double *p, const double *w, int64_t np, bool with_p, bool with_w,
                          const HermiteArgs &a, const HermitePlan &pl, hipStream_t st) {
  if (np <= 0) return hipSuccess;
  if (!check_plan(pl, a, (with_p ? 1 : 0) + (with_w ? 1 : 0))) return hipErrorInvalidValue;
  return with_bools(
      [&](auto P, auto W, auto NT) {
        if constexpr (P || W) {
          auto go = [&](auto NB) {
            return launch_kernel(k_hermite<P, W, NB, NT>, dim3(static_cast<unsigned>(pl.blocks)), dim3(static_cast<unsigned>(pl.threads)),
                                 pl.bytes, st, x, v, p, w, np, a);
          };
          if (pl.nb == 4) return go(std::integral_constant<int, 4>{});
          if (pl.nb == 8) return go(std::integral_constant<int, 8>{});
          return go(std::integral_constant<int, 16>{});
        }
        return hipErrorInvalidValue;
      },
      with_p, with_w, pl.nt);
}

}  // namespace pic1dp
