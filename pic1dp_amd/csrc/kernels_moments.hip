// kernels_moments.hip -- off the timed path: the velocity moments of a species' markers on the field grid
// (include/pic1dp_hip.h pic1dp_hip_moments).  One streaming pass per group of planes (launch_policy.cpp
// moments_plan), k_ptcldist's shape: one workgroup of 1024 threads per CU, marker pairs as double2, the planes as doubles
// in the workgroup's LDS -- or, the exact kind (pic1dp_hip_moments_exact; moments_plan_exact), as whole quanta
// in 64-bit integer words of the same size.  gfx950, wave64.
#include "device_moments.hpp"

#include <type_traits>
#include "device_sweep.hpp"
#include "launch_policy.hpp"

namespace pic1dp {

namespace {

// P, W: the weight sets of the pass (p: total f, w: delta f; both: p's planes first); KMASK: the powers of v it holds
// (0xF all four, 0x3 {0, 1}, 0xC {2, 3}).  Dynamic LDS: the planes [plane][cell] and nothing else (MomentsPass::bytes) --
// four planes of nx 4800 are the whole of kDiagLdsCap, so the drawn chunks' counter is static.  Plane-major: a cell-major
// layout needs an odd stride (9, 5 or 3 doubles per cell) against bank conflicts, and with it four planes of nx 4096 no
// longer fit.  Where both fit the counters do not tell them apart: 0.34 bank-conflict cycles per active LDS cycle here,
// with eight planes as with four, against 0.35 in k_ptcldist's cell-major copy of stride 3 in the same run
// (profiles/r18/moments_lds_counters.log) -- the conflicts of 64 lanes adding 8-byte words at random cells.
// The kernel zeroes its planes, adds two LDS atomics per plane and marker, and flushes them into the global planes, which
// the host zeroed on the stream.  Only the arrays the planes need are loaded.
template <bool P, bool W, int KMASK, bool NT>
__global__ void __launch_bounds__(1024)
k_moments(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst g, double *out,
          int dyn_tail) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ unsigned sDraw;   // the drawn chunks' counter
  double *sM = reinterpret_cast<double *>(smem);
  for (int i = threadIdx.x; i < moments_npl<P, W, KMASK>() * g.nx; i += blockDim.x) sM[i] = 0.0;
  if (threadIdx.x == 0) sDraw = 0u;
  __syncthreads();
  auto one = [&](double px, double pv, double pp, double pw) { moments_one<P, W, KMASK>(px, pv, pp, pw, g, sM); };
  pair_sweep<P, W, NT>(x, v, p, w, np >> 1, pair_rows(np >> 1, dyn_tail), &sDraw, one, [](int) {});
  if ((np & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // the odd last marker
    const int64_t i = tidx(np - 1);
    one(x[i], v[i], P ? p[i] : 0.0, W ? w[i] : 0.0);
  }
  __syncthreads();
  moments_flush<P, W, KMASK>(sM, out, g.nx);
}

// The exact kind: k_moments' sweep over integer planes (device_moments.hpp mfx_*).  The LDS holds one signed 64-bit word per
// (plane, cell) and nothing else; it is flushed by the window rule of device_sweep.hpp, with the odd last marker before the sweep.
template <bool P, bool W, int KMASK, bool NT>
__global__ void __launch_bounds__(1024)
k_moments_exact(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst g,
                const MomentsFxArgs a, int dyn_tail) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ unsigned sDraw;   // the drawn chunks' counter
  unsigned long long *sM = reinterpret_cast<unsigned long long *>(smem);
  for (int i = threadIdx.x; i < moments_npl<P, W, KMASK>() * g.nx; i += blockDim.x) sM[i] = 0ull;
  if (threadIdx.x == 0) sDraw = 0u;
  __syncthreads();
  auto one = [&](double px, double pv, double pp, double pw) { mfx_one<P, W, KMASK>(px, pv, pp, pw, g, sM, a); };
  if ((np & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // the odd last marker (before the pairs: inside the first window)
    const int64_t i = tidx(np - 1);
    one(x[i], v[i], P ? p[i] : 0.0, W ? w[i] : 0.0);
  }
  const PairRows rows = window_rows(pair_rows(np >> 1, dyn_tail));
  pair_sweep<P, W, NT>(x, v, p, w, np >> 1, rows, &sDraw, one, [&](int k) {
    if (window_due(k, rows)) {
      __syncthreads();
      mfx_flush<P, W, KMASK>(sM, a, g.nx);
      __syncthreads();
    }
  });
  __syncthreads();
  mfx_flush<P, W, KMASK>(sM, a, g.nx);
}

// what the kernel indexes must be what the plan sized: the LDS holds exactly the pass's planes, in words of word_bytes
bool check_pass(const MomentsPass &ps, const GridConst &g, size_t word_bytes) {
  const int sets = (ps.p ? 1 : 0) + (ps.w ? 1 : 0);
  const int nk = ps.kmask == 0xF ? 4 : 2;
  return sets != 0 && ps.planes == sets * nk && ps.bytes == word_bytes * static_cast<size_t>(ps.planes) * g.nx && ps.threads == 1024 &&
         ps.blocks >= 1 && (sets == 1 || ps.kmask == 0xF);
}

// f(P, W, KMASK, NT) with a pass's weight sets, powers and loads as compile-time constants: the seven (P, W, KMASK)
// combinations moments_plan hands out -- both sets with all four powers, one set with 0xF, 0x3 or 0xC --, each with and
// without non-temporal loads, and no others
template <class F>
hipError_t with_pass(const MomentsPass &ps, F &&f) {
  return with_bools(
      [&](auto P, auto W, auto NT) {
        if constexpr (P || W) {
          if (ps.kmask == 0xF) return f(P, W, std::integral_constant<int, 0xF>{}, NT);
          if constexpr (!(P && W)) {
            if (ps.kmask == 0x3) return f(P, W, std::integral_constant<int, 0x3>{}, NT);
            if (ps.kmask == 0xC) return f(P, W, std::integral_constant<int, 0xC>{}, NT);
          }
        }
        return hipErrorInvalidValue;
      },
      ps.p, ps.w, ps.nt);
}

}  // namespace

hipError_t launch_moments(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst &g,
                          double *out, const MomentsPass &ps, int dyn_tail, hipStream_t st) {
  if (np <= 0) return hipSuccess;
  if (!check_pass(ps, g, sizeof(double))) return hipErrorInvalidValue;
  double *dst = out + static_cast<size_t>(ps.first_plane / 4) * 4 * g.nx;   // the first plane of the pass's (first) weight set
  return with_pass(ps, [&](auto P, auto W, auto KMASK, auto NT) {
    return launch_kernel(k_moments<P, W, KMASK, NT>, dim3(static_cast<unsigned>(ps.blocks)), dim3(static_cast<unsigned>(ps.threads)),
                         ps.bytes, st, x, v, p, w, np, g, dst, dyn_tail);
  });
}

// ps: a pass of moments_plan_exact
hipError_t launch_moments_exact(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst &g,
                                const MomentsFxArgs &a, const MomentsPass &ps, int dyn_tail, hipStream_t st) {
  if (np <= 0) return hipSuccess;
  if (!check_pass(ps, g, sizeof(long long)) || !a.acc || !a.rej) return hipErrorInvalidValue;
  MomentsFxArgs b = a;   // the first plane and the counters of the pass's (first) weight set
  b.acc = a.acc + static_cast<size_t>(ps.first_plane / 4) * 4 * 2 * g.nx;
  b.rej = a.rej + (ps.first_plane / 4) * 4;
  return with_pass(ps, [&](auto P, auto W, auto KMASK, auto NT) {
    return launch_kernel(k_moments_exact<P, W, KMASK, NT>, dim3(static_cast<unsigned>(ps.blocks)),
                         dim3(static_cast<unsigned>(ps.threads)), ps.bytes, st, x, v, p, w, np, g, b, dyn_tail);
  });
}

}  // namespace pic1dp
