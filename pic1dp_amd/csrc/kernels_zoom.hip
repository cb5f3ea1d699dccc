// kernels_zoom.hip -- off the timed path: the exact phase-space histogram of a species' markers on a caller-chosen window
// and grid (include/pic1dp_hip.h pic1dp_hip_zoom).  One streaming pass per band of whole v rows
// (launch_policy.cpp zoom_plan) in k_moments_exact's / k_power_exact's shape: one workgroup of 1024 threads per CU, marker
// pairs as double2, the band's planes as whole quanta in 64-bit integer words in the workgroup's LDS -- or, where the grid
// would need more band passes than the plan allows, one pass whose terms go straight into the global rows.  gfx950, wave64.
#include "device_zoom.hpp"

#include <type_traits>
#include "device_sweep.hpp"
#include "launch_policy.hpp"

// 1: a band pass loads p and w only for the markers that lie in its band (16 instead of 32 B per marker outside it, at the
// price of divergent loads outside the sweep's prologue); 0: pair_sweep loads them with x and v.  DESIGN.md 2.20 has the
// measurement that chose.  The form that lost (1) was timed, not tested: run tests/test_gpu_zoom.py against it before use.
#ifndef PIC1DP_ZOOM_SKIP
#define PIC1DP_ZOOM_SKIP 0
#endif

namespace pic1dp {

namespace {

constexpr bool kZoomSkip = PIC1DP_ZOOM_SKIP != 0;

template <bool NT>
__device__ __forceinline__ double zoom_ld(const double *a) {
  if constexpr (NT) return __builtin_nontemporal_load(a);
  else return *a;
}

// M, P, W: the planes of the pass (markr, total, pertb, in that order).  LDS: the dynamic LDS (ZoomPass::bytes) holds the
// band's words [plane][row - r0][ix], zeroed by the workgroup and flushed into the global rows, which the host zeroed on the
// stream, by the window rule of device_sweep.hpp: the odd last marker before the sweep, a flush after every
// DIAG_FX_WINDOW_TRIPS dealt trips and once at the end.  One term per marker and word, each below 2^44 quanta (markr: 1),
// fewer than 2^17 markers between two flushes: a word stays below 2^61.  !LDS: r0 = 0, rows = nvb, a term's limbs go
// straight into the global rows, nothing to flush.
// Per marker: two compares, a difference and a product for the row; only for a marker of the band the wrap, the column, one
// fx_word44 and one LDS atomic per plane.  SKIP (P or W, LDS): x and v alone travel through the sweep, every row dealt (no
// drawn chunks: a dealt trip's pair is first + k stride, so the lambda knows its marker), p and w are loaded inside it.
template <bool M, bool P, bool W, bool LDS, bool NT, bool SKIP>
__global__ void __launch_bounds__(1024)
k_zoom(const double *x, const double *v, const double *p, const double *w, int64_t np, const ZoomGeom g, const ZoomArgs a, int r0,
       int rows, int dyn_tail) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ unsigned sDraw;    // the drawn chunks' counter
  constexpr int NP = (M ? 1 : 0) + (P ? 1 : 0) + (W ? 1 : 0);
  ZoomSums z;
  z.s = reinterpret_cast<unsigned long long *>(smem);
  z.acc = reinterpret_cast<unsigned long long *>(a.acc), z.rej = reinterpret_cast<unsigned long long *>(a.rej);
  z.band = rows * g.nxb, z.cells = g.nvb * g.nxb;
  if (threadIdx.x == 0) sDraw = 0u;
  if constexpr (LDS)
    for (int i = threadIdx.x; i < NP * z.band; i += blockDim.x) z.s[i] = 0ull;
  __syncthreads();
  auto flush = [&]() {
    if constexpr (LDS) {
      __syncthreads();
      zoom_flush(z, NP, r0 * g.nxb);
      __syncthreads();
    }
  };
  if ((np & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // the odd last marker (before the pairs: inside the first window)
    const int64_t i = tidx(np - 1);
    zoom_one<M, P, W, LDS>(x[i], v[i], g, r0, rows, z, a.inv_q_p, a.inv_q_w, [&] { return p[i]; }, [&] { return w[i]; });
  }
  const int64_t npair = np >> 1;
  if constexpr (SKIP) {
    const PairRows pr = window_rows(pair_rows(npair, 0));
    int64_t j = pr.first + threadIdx.x;
    int h = 0;   // which marker of pair j
    auto one = [&](double px, double pv, double, double) {
      const int64_t i = 2 * tidx2(j) + h++;
      zoom_one<M, P, W, LDS>(px, pv, g, r0, rows, z, a.inv_q_p, a.inv_q_w, [&] { return zoom_ld<NT>(p + i); }, [&] { return zoom_ld<NT>(w + i); });
    };
    pair_sweep<false, false, NT>(x, v, p, w, npair, pr, &sDraw, one, [&](int k) {
      j += pr.stride, h = 0;
      if (window_due(k, pr)) flush();
    });
  } else {
    const PairRows pr = window_rows(pair_rows(npair, dyn_tail));
    auto one = [&](double px, double pv, double pp, double pw) {
      zoom_one<M, P, W, LDS>(px, pv, g, r0, rows, z, a.inv_q_p, a.inv_q_w, [&] { return pp; }, [&] { return pw; });
    };
    pair_sweep<P, W, NT>(x, v, p, w, npair, pr, &sDraw, one, [&](int k) {
      if (window_due(k, pr)) flush();
    });
  }
  flush();
}

// what the kernel indexes must be what the plan sized: the LDS holds exactly the band's words, a pass in memory every row
bool check_pass(const ZoomPass &ps, const ZoomGeom &g, int which) {
  if (which < 1 || which > 7 || ps.planes != which || g.nxb < 1 || g.nvb < 1 || g.nxb > ZOOM_MAX_BINS || g.nvb > ZOOM_MAX_BINS ||
      static_cast<int64_t>(g.nxb) * g.nvb > ZOOM_MAX_CELLS)
    return false;
  const int n = (which & 1) + ((which >> 1) & 1) + ((which >> 2) & 1);
  if (ps.threads != 1024 || ps.blocks < 1 || ps.first_row < 0 || ps.rows < 1 || ps.first_row + ps.rows > g.nvb) return false;
  if (!ps.lds) return ps.bytes == 0 && ps.first_row == 0 && ps.rows == g.nvb;
  return ps.bytes == sizeof(unsigned long long) * static_cast<size_t>(n) * ps.rows * g.nxb && ps.bytes <= kDiagLdsCap;
}

}  // namespace

hipError_t launch_zoom(const double *x, const double *v, const double *p, const double *w, int64_t np, const ZoomGeom &zg,
                       int which, const ZoomArgs &a, const ZoomPass &ps, int dyn_tail, hipStream_t st) {
  if (np <= 0) return hipSuccess;
  if (!check_pass(ps, zg, which) || !a.acc || !a.rej) return hipErrorInvalidValue;
  return with_bools(
      [&](auto M, auto P, auto W, auto LDS, auto NT) {
        if constexpr (M || P || W) {
          constexpr bool SKIP = kZoomSkip && LDS && (P || W);
          return launch_kernel(k_zoom<M, P, W, LDS, NT, SKIP>, dim3(static_cast<unsigned>(ps.blocks)),
                               dim3(static_cast<unsigned>(ps.threads)), ps.bytes, st, x, v, p, w, np, zg, a, ps.first_row, ps.rows,
                               dyn_tail);
        }
        return hipErrorInvalidValue;
      },
      (which & 1) != 0, (which & 2) != 0, (which & 4) != 0, ps.lds, ps.nt);
}

}  // namespace pic1dp
