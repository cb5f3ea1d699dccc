// kernels_moments.hip -- off the timed path: the velocity moments of a species' markers on the field grid
// (include/pic1dp_hip.h pic1dp_hip_moments).  One streaming pass per group of planes (launch_policy.cpp
// moments_plan), k_ptcldist's shape: one workgroup of 1024 threads per CU, marker pairs as double2, the planes as doubles
// in the workgroup's LDS -- or, the exact kind (pic1dp_hip_moments_exact; moments_plan_exact), as whole quanta
// in 64-bit integer words of the same size.  gfx950, wave64.
#include "device_moments.hpp"

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
  constexpr int NPL = ((P ? 1 : 0) + (W ? 1 : 0)) * moments_nk<KMASK>();
  for (int i = threadIdx.x; i < NPL * g.nx; i += blockDim.x) sM[i] = 0.0;
  if (threadIdx.x == 0) sDraw = 0u;
  __syncthreads();
  auto one = [&](double px, double pv, double pp, double pw) { moments_one<P, W, KMASK>(px, pv, pp, pw, g, sM); };
  moments_sweep<P, W, NT>(x, v, p, w, np >> 1, pair_rows(np >> 1, dyn_tail), &sDraw, one, [](int) {});
  if ((np & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // the odd last marker
    const int64_t i = tidx(np - 1);
    one(x[i], v[i], P ? p[i] : 0.0, W ? w[i] : 0.0);
  }
  __syncthreads();
  moments_flush<P, W, KMASK>(sM, out, g.nx);
}

template <bool P, bool W, int KMASK>
hipError_t launch_one(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst &g,
                      double *out, const MomentsPass &ps, int dyn_tail, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(ps.blocks)), block(static_cast<unsigned>(ps.threads));
  if (ps.nt) return launch_kernel(k_moments<P, W, KMASK, true>, grid, block, ps.bytes, st, x, v, p, w, np, g, out, dyn_tail);
  return launch_kernel(k_moments<P, W, KMASK, false>, grid, block, ps.bytes, st, x, v, p, w, np, g, out, dyn_tail);
}

// The exact kind: k_moments' sweep over integer planes (device_moments.hpp mfx_*).  The LDS holds one signed 64-bit word per
// (plane, cell) and nothing else.  The window: a workgroup flushes its words into the global (hi, lo) rows every
// DIAG_FX_WINDOW_TRIPS dealt trips and once at the end; the drawn rows are capped one below that, and the odd last marker is
// taken BEFORE the sweep, so it falls into the first window.  Between two flushes a word therefore sees at most
// DIAG_FX_WINDOW_TRIPS trips of 2 x 1024 markers and that marker, or DIAG_FX_WINDOW_TRIPS - 1 dealt and as many drawn
// trips: fewer than 2^17 markers.  A marker adds one term to a word (nx >= 2), or two (nx = 1: ix == ir), each below 2^44
// quanta: fewer than 2^18 terms, the word stays below 2^62 in magnitude.  The dealt trips are the same number for every thread
// of the workgroup, so the barriers around a flush inside the sweep are met by all.
template <bool P, bool W, int KMASK, bool NT>
__global__ void __launch_bounds__(1024)
k_moments_exact(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst g,
                const MomentsFxArgs a, int dyn_tail) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ unsigned sDraw;   // the drawn chunks' counter
  unsigned long long *sM = reinterpret_cast<unsigned long long *>(smem);
  constexpr int NPL = ((P ? 1 : 0) + (W ? 1 : 0)) * moments_nk<KMASK>();
  for (int i = threadIdx.x; i < NPL * g.nx; i += blockDim.x) sM[i] = 0ull;
  if (threadIdx.x == 0) sDraw = 0u;
  __syncthreads();
  auto one = [&](double px, double pv, double pp, double pw) { mfx_one<P, W, KMASK>(px, pv, pp, pw, g, sM, a); };
  if ((np & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // the odd last marker (before the pairs: inside the first window)
    const int64_t i = tidx(np - 1);
    one(x[i], v[i], P ? p[i] : 0.0, W ? w[i] : 0.0);
  }
  PairRows rows = pair_rows(np >> 1, dyn_tail);
  {
    const int waves = static_cast<int>(blockDim.x >> 6);
    const int extra = rows.drawn_total / waves - (DIAG_FX_WINDOW_TRIPS - 1);
    if (extra > 0) {
      rows.dealt += extra;
      rows.drawn_total -= extra * waves;
    }
  }
  moments_sweep<P, W, NT>(x, v, p, w, np >> 1, rows, &sDraw, one, [&](int k) {
    if (k <= rows.dealt && (k & (DIAG_FX_WINDOW_TRIPS - 1)) == 0) {   // (k: dealt trips done -- uniform over the workgroup)
      __syncthreads();
      mfx_flush<P, W, KMASK>(sM, a, g.nx);
      __syncthreads();
    }
  });
  __syncthreads();
  mfx_flush<P, W, KMASK>(sM, a, g.nx);
}

template <bool P, bool W, int KMASK>
hipError_t launch_one_exact(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst &g,
                            const MomentsFxArgs &a, const MomentsPass &ps, int dyn_tail, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(ps.blocks)), block(static_cast<unsigned>(ps.threads));
  if (ps.nt) return launch_kernel(k_moments_exact<P, W, KMASK, true>, grid, block, ps.bytes, st, x, v, p, w, np, g, a, dyn_tail);
  return launch_kernel(k_moments_exact<P, W, KMASK, false>, grid, block, ps.bytes, st, x, v, p, w, np, g, a, dyn_tail);
}

}  // namespace

// the seven (P, W, KMASK) combinations moments_plan hands out, each with and without non-temporal loads
hipError_t launch_moments(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst &g,
                          double *out, const MomentsPass &ps, int dyn_tail, hipStream_t st) {
  if (np <= 0) return hipSuccess;
  const int sets = (ps.p ? 1 : 0) + (ps.w ? 1 : 0);
  const int nk = ps.kmask == 0xF ? 4 : 2;
  // what the kernel indexes must be what the plan sized: the LDS holds exactly the pass's planes
  if (sets == 0 || ps.planes != sets * nk || ps.bytes != sizeof(double) * static_cast<size_t>(ps.planes) * g.nx || ps.threads != 1024 ||
      ps.blocks < 1 || (sets == 2 && ps.kmask != 0xF))
    return hipErrorInvalidValue;
  double *dst = out + static_cast<size_t>(ps.first_plane / 4) * 4 * g.nx;   // the first plane of the pass's (first) weight set
  if (ps.p && ps.w) return launch_one<true, true, 0xF>(x, v, p, w, np, g, dst, ps, dyn_tail, st);
  if (ps.p) {
    if (ps.kmask == 0xF) return launch_one<true, false, 0xF>(x, v, p, w, np, g, dst, ps, dyn_tail, st);
    if (ps.kmask == 0x3) return launch_one<true, false, 0x3>(x, v, p, w, np, g, dst, ps, dyn_tail, st);
    if (ps.kmask == 0xC) return launch_one<true, false, 0xC>(x, v, p, w, np, g, dst, ps, dyn_tail, st);
  } else {
    if (ps.kmask == 0xF) return launch_one<false, true, 0xF>(x, v, p, w, np, g, dst, ps, dyn_tail, st);
    if (ps.kmask == 0x3) return launch_one<false, true, 0x3>(x, v, p, w, np, g, dst, ps, dyn_tail, st);
    if (ps.kmask == 0xC) return launch_one<false, true, 0xC>(x, v, p, w, np, g, dst, ps, dyn_tail, st);
  }
  return hipErrorInvalidValue;
}

// the same seven combinations for the passes of moments_plan_exact
hipError_t launch_moments_exact(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst &g,
                                const MomentsFxArgs &a, const MomentsPass &ps, int dyn_tail, hipStream_t st) {
  if (np <= 0) return hipSuccess;
  const int sets = (ps.p ? 1 : 0) + (ps.w ? 1 : 0);
  const int nk = ps.kmask == 0xF ? 4 : 2;
  // what the kernel indexes must be what the plan sized: the LDS holds exactly the pass's planes, as 64-bit words
  if (sets == 0 || ps.planes != sets * nk || ps.bytes != sizeof(long long) * static_cast<size_t>(ps.planes) * g.nx || ps.threads != 1024 ||
      ps.blocks < 1 || (sets == 2 && ps.kmask != 0xF) || !a.acc || !a.rej)
    return hipErrorInvalidValue;
  MomentsFxArgs b = a;   // the first plane and the counters of the pass's (first) weight set
  b.acc = a.acc + static_cast<size_t>(ps.first_plane / 4) * 4 * 2 * g.nx;
  b.rej = a.rej + (ps.first_plane / 4) * 4;
  if (ps.p && ps.w) return launch_one_exact<true, true, 0xF>(x, v, p, w, np, g, b, ps, dyn_tail, st);
  if (ps.p) {
    if (ps.kmask == 0xF) return launch_one_exact<true, false, 0xF>(x, v, p, w, np, g, b, ps, dyn_tail, st);
    if (ps.kmask == 0x3) return launch_one_exact<true, false, 0x3>(x, v, p, w, np, g, b, ps, dyn_tail, st);
    if (ps.kmask == 0xC) return launch_one_exact<true, false, 0xC>(x, v, p, w, np, g, b, ps, dyn_tail, st);
  } else {
    if (ps.kmask == 0xF) return launch_one_exact<false, true, 0xF>(x, v, p, w, np, g, b, ps, dyn_tail, st);
    if (ps.kmask == 0x3) return launch_one_exact<false, true, 0x3>(x, v, p, w, np, g, b, ps, dyn_tail, st);
    if (ps.kmask == 0xC) return launch_one_exact<false, true, 0xC>(x, v, p, w, np, g, b, ps, dyn_tail, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace pic1dp
