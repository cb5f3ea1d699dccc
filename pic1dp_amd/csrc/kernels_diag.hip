// kernels_diag.hip -- off the timed path: the diagnostics passes of output_all (k_ptcldist and k_ptcldist_exact around one
// pair sweep; their launch shapes: launch_policy.cpp diag_launch), kinetic sums of tail slots, cell indices per marker
// (parity tests), and the copies between contiguous host-side buffers and the tiled marker slabs.  gfx950, wave64.
#include "device_diag.hpp"

#include <algorithm>
#include <cmath>
#include <type_traits>
#include "device_math.hpp"
#include "device_sweep.hpp"
#include "launch_policy.hpp"

namespace pic1dp {

// ---------------------------------------------------------------------------
// diagnostics
// ---------------------------------------------------------------------------
namespace {

// sum v^2, v^2 p, v^2 w (src/pic1dp_output.F90:126-151): per-workgroup partials,
// the host adds them in workgroup order
__global__ void __launch_bounds__(256)
k_energy_sums(const double *v, const double *p, const double *w, int64_t i0, int64_t n, double *partial) {
  __shared__ double scr[16];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < n; k += stride) {
    const int64_t i = tidx(i0 + k);
    const double v2 = v[i] * v[i];
    s0 += v2;
    s1 += v2 * p[i];
    if (w) s2 += v2 * w[i];
  }
  const double t0 = block_sum(s0, scr);
  const double t1 = block_sum(s1, scr);
  const double t2 = block_sum(s2, scr);
  if (threadIdx.x == 0) {
    partial[blockIdx.x * 3 + 0] = t0;
    partial[blockIdx.x * 3 + 1] = t1;
    partial[blockIdx.x * 3 + 2] = t2;
  }
}

__global__ void __launch_bounds__(256)
k_cell_indices(const double *x, int64_t np, const GridConst g, int32_t *ixo,
               unsigned long long *count) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < np; i += stride) {
    int ix;
    double wl;
    locate(x[tidx(i)], g, ix, wl);
    if (ixo) ixo[i] = ix;
    if (count) atomicAdd(&count[ix], 1ULL);
  }
}

}  // namespace

namespace {

// One pass over a species for everything output_all needs from the markers:
// * the (x,v) and v histograms of output_ptcldist, src/pic1dp_output.F90:239-315:
//   4-point bilinear weights on an nx_opd x nv_opd grid, markers with
//   |v| >= v_max skipped (:241);
// * the kinetic sums of output_field, sum v^2, v^2 p, v^2 w over ALL markers
//   (:126-151), as per-workgroup partials the host adds in workgroup order.
// LDS = true keeps a private copy of the histograms per workgroup
// (3*(nxo*nvo)+3*nvo doubles) and flushes it with global atomics.  There the v
// histograms are not accumulated marker by marker (64 hot bins: the LDS atomics
// of a wave collide) but formed once per workgroup as the row sums of its (x,v)
// histograms -- the same numbers in exact arithmetic, (sx + (1-sx))*sv = sv, and
// within rounding (<= 1e-15 relative per term) of the separate accumulation.
// LDS = false (grids too large for 160 KiB) adds everything straight to memory.
// The per-marker part and the finish are shared with the DIAG variant of k_step_full.
//
// Round 5 (profiles/r05/sq_counters_diag.json: 0.85 ms at 1e8 markers = 3.8 TB/s for 32 B per marker): the histogram copy
// leaves room for ONE workgroup of 1024 threads per CU, and with one marker per thread and 8-byte loads those sixteen
// waves had 32 KB of loads in flight per CU -- by Little's law ~4 TB/s at the latency the memory system has under load;
// the LDS pipe (twelve FP64 atomics at random bins per marker) was ~70 % busy BEHIND that, not the first limit.  Hence:
// marker PAIRS per thread (16-byte loads, the marker kernels' access shape), the NEXT trip's loads issued before this
// trip's atomics (twice the bytes in flight again), non-temporal loads once the state outgrows the Infinity Cache, the
// two divisions by constants without the hardware's division sequence (bit for bit the same quotients), and the three
// planes interleaved so that a corner's three atomics share one address computation (device_diag.hpp).
// FX: the LDS copy as 64-bit fixed-point sums (device_diag.hpp DistScale): the atomics at 1.9x the rate.
template <bool LDS, bool DELTAF, bool NT, bool FX>
__global__ void __launch_bounds__(1024)
k_ptcldist(const double *x, const double *v, const double *p, const double *w, int64_t np, const DistGeom dg,
           double *out, double *partial, const DistScale fx, int dyn_tail) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ntot = 3 * dg.nxo * dg.nvo + 3 * dg.nvo;
  DistBins b{LDS ? reinterpret_cast<double *>(smem) : out, dg.nxo * dg.nvo, dg.nvo};
  double *scr = reinterpret_cast<double *>(smem) + (LDS ? ntot : 0);  // [16]
  unsigned *sDraw = reinterpret_cast<unsigned *>(scr + 16);            // the drawn chunks' counter
  if constexpr (LDS)
    for (int i = threadIdx.x; i < ntot; i += blockDim.x) b.h[i] = 0.0;
  if (threadIdx.x == 0) *sDraw = 0u;
  __syncthreads();
  DistSums sm;
  auto one = [&](double px, double pv, double pp, double pw) { ptcldist_one<LDS, DELTAF, FX>(px, pv, pp, pw, dg, b, sm, &fx); };
  pair_sweep<true, DELTAF, NT>(x, v, p, w, np >> 1, pair_rows(np >> 1, dyn_tail), sDraw, one, [](int) {});
  if ((np & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // (after the pairs: the FP64 kinetic sums depend on the order)
    const int64_t i = tidx(np - 1);
    one(x[i], v[i], p[i], DELTAF ? w[i] : 0.0);
  }
  ptcldist_finish<LDS, DELTAF, FX>(dg, b, sm, scr, out, partial, &fx);
}

}  // namespace

// bound_p / bound_w: max |p|, max |w| the markers are known not to exceed (with the caller's margin), or <= 0: unknown --
// the pass then sums in doubles.  partial: [blocks][DIAG_PART] = the kinetic sums, max |p|, max |w|, overflow flag per workgroup
hipError_t launch_ptcldist(const double *x, const double *v, const double *p, const double *w, int64_t np, const DistGeom &dg,
                           bool deltaf, double bound_p, double bound_w, double *out, double *partial, const DiagLaunch &dl,
                           int dyn_tail, hipStream_t st, bool *fixed_point) {
  bool nt = dl.nt;   // (PIC1DP_DIAG_NT=0 / 1 insists)
  if (const char *e = tuning_env("PIC1DP_DIAG_NT")) nt = std::atoi(e) != 0;
  DistScale fx{};
  const bool use_fx = dl.lds && make_dist_scale(np, dl.blocks, deltaf, bound_p, bound_w, &fx, dl.threads);
  if (fixed_point) *fixed_point = use_fx;
  return with_bools(
      [&](auto LDS, auto DELTAF, auto NT, auto FX) {
        return launch_kernel(k_ptcldist<LDS, DELTAF, NT, LDS && FX>, dim3(static_cast<unsigned>(dl.blocks)), dim3(dl.threads),
                             dl.bytes, st, x, v, p, w, np, dg, out, partial, fx, dyn_tail);
      },
      dl.lds, deltaf, nt, use_fx);
}

// ---------------------------------------------------------------------------
// kind 1 of the diagnostics sum: the exact pass (kernels.hpp DiagFxArgs, device_diag.hpp)
// ---------------------------------------------------------------------------
namespace {

// The sweep of k_ptcldist with integer sums: no max |p|, max |w| or overflow bookkeeping and no repeat pass (the quanta
// come from the input), the kinetic sums reduced over the workgroup as integers.  LDS: the workgroup's copy is flushed by the
// window rule of device_sweep.hpp, with the odd last marker before the sweep.
template <bool LDS, bool DELTAF, bool NT>
__global__ void __launch_bounds__(1024)
k_ptcldist_exact(const double *x, const double *v, const double *p, const double *w, int64_t np, const DistGeom dg,
                 const DiagFxArgs a, int dyn_tail) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nxv = dg.nxo * dg.nvo;
  unsigned long long *sK = reinterpret_cast<unsigned long long *>(smem);   // [6] kinetic sums, then the drawn chunks' counter
  unsigned *sDraw = reinterpret_cast<unsigned *>(sK + 6);
  const DistBinsFx b{sK + 8, reinterpret_cast<unsigned long long *>(a.acc), nxv};
  if constexpr (LDS)
    for (int i = threadIdx.x; i < 3 * nxv; i += blockDim.x) b.s[i] = 0ull;
  if (threadIdx.x < 6) sK[threadIdx.x] = 0ull;
  if (threadIdx.x == 0) *sDraw = 0u;
  __syncthreads();
  KinFx sm;
  auto one = [&](double px, double pv, double pp, double pw) { ptcldist_one_exact<LDS, DELTAF>(px, pv, pp, pw, dg, b, sm, a); };
  if ((np & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // (before the pairs: inside the first window)
    const int64_t i = tidx(np - 1);
    one(x[i], v[i], p[i], DELTAF ? w[i] : 0.0);
  }
  const PairRows rows = window_rows(pair_rows(np >> 1, dyn_tail));
  pair_sweep<true, DELTAF, NT>(x, v, p, w, np >> 1, rows, sDraw, one, [&](int k) {
    if constexpr (LDS) {
      if (window_due(k, rows)) {
        __syncthreads();
        dfx_flush(b);
        __syncthreads();
      }
    }
  });
  dfx_kin_finish(sm, b, sK);
  if constexpr (LDS) {
    __syncthreads();
    dfx_flush(b);
  }
}

// the tail slots' kinetic terms into the same accumulators
template <bool DELTAF>
__global__ void __launch_bounds__(256)
k_energy_sums_exact(const double *v, const double *p, const double *w, int64_t i0, int64_t n, int nxv, const DiagFxArgs a) {
  __shared__ unsigned long long sK[6];
  const DistBinsFx b{nullptr, reinterpret_cast<unsigned long long *>(a.acc), nxv};
  if (threadIdx.x < 6) sK[threadIdx.x] = 0ull;
  __syncthreads();
  KinFx sm;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < n; k += stride) {
    const int64_t i = tidx(i0 + k);
    kinetic_one_exact<DELTAF>(v[i], p[i], DELTAF ? w[i] : 0.0, b, sm, a);
  }
  dfx_kin_finish(sm, b, sK);
}

}  // namespace

hipError_t launch_ptcldist_exact(const double *x, const double *v, const double *p, const double *w, int64_t np,
                                 const DistGeom &dg, bool deltaf, const DiagFxArgs &a, const DiagLaunch &dl, int dyn_tail,
                                 hipStream_t st) {
  return with_bools(
      [&](auto LDS, auto DELTAF, auto NT) {
        return launch_kernel(k_ptcldist_exact<LDS, DELTAF, NT>, dim3(static_cast<unsigned>(dl.blocks)), dim3(dl.threads),
                             dl.bytes, st, x, v, p, w, np, dg, a, dyn_tail);
      },
      dl.lds, deltaf, dl.nt);
}

hipError_t launch_energy_sums_exact(const double *v, const double *p, const double *w, int64_t i0, int64_t n,
                                    const DiagFxArgs &a, int nxv, hipStream_t st) {
  const int blocks = tail_sum_blocks(n);
  if (blocks == 0) return hipSuccess;
  if (w) return launch_kernel(k_energy_sums_exact<true>, dim3(blocks), dim3(256), 0, st, v, p, w, i0, n, nxv, a);
  return launch_kernel(k_energy_sums_exact<false>, dim3(blocks), dim3(256), 0, st, v, p, w, i0, n, nxv, a);
}

namespace {
__global__ void __launch_bounds__(256) k_pack_record(const PackArgs a, double *out) {
  const int seg = blockIdx.y;
  if (seg >= a.count) return;
  const double *src = a.src[seg];
  double *dst = out + a.dst[seg];
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n[seg]; i += gridDim.x * blockDim.x) dst[i] = src[i];
}
}  // namespace
hipError_t launch_pack_record(const PackArgs &a, double *out, hipStream_t st) {
  if (a.count <= 0) return hipSuccess;
  return launch_kernel(k_pack_record, dim3(16, a.count), dim3(256), 0, st, a, out);
}

hipError_t launch_energy_sums(const double *v, const double *p, const double *w, int64_t i0, int64_t n,
                              double *partial, int blocks, hipStream_t st) {
  return launch_kernel(k_energy_sums, dim3(blocks), dim3(256), 0, st, v, p, w, i0, n, partial);
}

namespace {

// host arrays are contiguous, marker arrays tiled: the two meet in these kernels
__global__ void __launch_bounds__(256) k_tile_scatter(double *arr, int64_t i0, const double *src, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < n; k += stride)
    arr[tidx(i0 + k)] = src[k];
}
__global__ void __launch_bounds__(256) k_tile_gather(const double *arr, int64_t i0, double *dst, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < n; k += stride)
    dst[k] = arr[tidx(i0 + k)];
}
__global__ void __launch_bounds__(256) k_tile_copy(double *dst, const double *src, int64_t n) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < n; k += stride)
    dst[tidx(k)] = src[tidx(k)];
}

int copy_blocks(int64_t n) {
  int64_t b = (n + 255) / 256;
  return static_cast<int>(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

hipError_t launch_tile_scatter(double *arr, int64_t i0, const double *src, int64_t n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  return launch_kernel(k_tile_scatter, dim3(copy_blocks(n)), dim3(256), 0, st, arr, i0, src, n);
}
hipError_t launch_tile_gather(const double *arr, int64_t i0, double *dst, int64_t n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  return launch_kernel(k_tile_gather, dim3(copy_blocks(n)), dim3(256), 0, st, arr, i0, dst, n);
}
hipError_t launch_tile_copy(double *dst, const double *src, int64_t n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  return launch_kernel(k_tile_copy, dim3(copy_blocks(n)), dim3(256), 0, st, dst, src, n);
}

hipError_t launch_cell_indices(const double *x, int64_t np, const GridConst &g, int32_t *ix,
                               unsigned long long *count, hipStream_t st) {
  int blocks = static_cast<int>((np + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return launch_kernel(k_cell_indices, dim3(blocks), dim3(256), 0, st, x, np, g, ix, count);
}

}  // namespace pic1dp
