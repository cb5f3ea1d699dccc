// kernels_power.hip -- off the timed path: the velocity-resolved wave-particle power q v E(x) of a species' markers on the
// (x, v) output grid (include/pic1dp_hip.h pic1dp_hip_power).  One streaming pass per group of weight sets
// (launch_policy.cpp power_plan) in k_moments' / k_ptcldist's shape: one workgroup of 1024 threads per CU, marker pairs as
// double2, the field as the push's E tile in the workgroup's LDS and the planes as doubles behind it -- or, the exact kind
// (pic1dp_hip_power_exact; power_plan_exact), as whole quanta in 64-bit integer words of the same size, the
// quantum taken from max |E| of the tile.  gfx950, wave64.
#include "device_power.hpp"

#include <type_traits>
#include "device_sweep.hpp"
#include "launch_policy.hpp"

namespace pic1dp {

namespace {

// P, W: the weight sets of the pass (p: total f, w: delta f; both: p's plane first).  Dynamic LDS (PowerPass::bytes): the E
// tile -- nx + 1 doubles, cell nx = E[0], the push's guard, staged from field_electric by the workgroup -- and, 16-byte
// aligned behind it (power_tile_bytes), LDS: the pass's planes [set][iv * nx_opd + ix], zeroed by the workgroup and flushed
// into the global planes, which the host zeroed on the stream.  !LDS (a plane that does not fit): the four terms per set go
// straight into the global planes; the tile stays.  Plane-major as k_moments' planes: the four cells of a marker are two
// pairs of neighbours either way, and a set's plane is what a pass per set holds.
// Per marker: one wrap, one locate, two LDS reads, the stencil, four LDS atomics per set; the terms of markers without bins
// in a register sum per thread and set, one global atomic per set and workgroup at the end.
template <bool P, bool W, bool LDS, bool NT>
__global__ void __launch_bounds__(1024)
k_power(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst g, const DistGeom dg,
        const double *E, double *planes, double *rest, int dyn_tail) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ unsigned sDraw;    // the drawn chunks' counter
  __shared__ double sScr[16];   // block_sum's partials
  constexpr int NS = (P ? 1 : 0) + (W ? 1 : 0);
  const int nxv = dg.nxo * dg.nvo;
  double *sE = reinterpret_cast<double *>(smem);
  double *sP = LDS ? reinterpret_cast<double *>(smem + power_tile_bytes(g.nx)) : planes;
  for (int i = threadIdx.x; i < g.nx; i += blockDim.x) sE[i] = E[i];
  if (threadIdx.x == 0) {
    sE[g.nx] = E[0];   // cell nx is cell 0
    sDraw = 0u;
  }
  if constexpr (LDS)
    for (int i = threadIdx.x; i < NS * nxv; i += blockDim.x) sP[i] = 0.0;
  __syncthreads();
  PowerRest r;
  auto one = [&](double px, double pv, double pp, double pw) { power_one<P, W, LDS>(px, pv, pp, pw, g, dg, sE, sP, nxv, r); };
  pair_sweep<P, W, NT>(x, v, p, w, np >> 1, pair_rows(np >> 1, dyn_tail), &sDraw, one, [](int) {});
  if ((np & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // the odd last marker
    const int64_t i = tidx(np - 1);
    one(x[i], v[i], P ? p[i] : 0.0, W ? w[i] : 0.0);
  }
  if constexpr (P) power_rest_flush(r.p, sScr, rest);
  if constexpr (W) power_rest_flush(r.w, sScr, rest + (P ? 1 : 0));
  if constexpr (LDS) {
    __syncthreads();
    power_flush(sP, planes, NS * nxv);
  }
}

// The exact kind: k_power's sweep over integer planes (device_power.hpp pfx_*).  The dynamic LDS is k_power's, byte for
// byte: the E tile, and behind it (LDS) one signed 64-bit word per (set, bin).  The workgroup that stages the tile takes
// max |E| from it -- every workgroup the same bits --, and with it the call's quantum 2^e (kernels.hpp power_fx_exponent);
// workgroup 0 leaves e, the non-finite flag and the bits of max |E| in a.scale.  A field with an infinity or a NaN: the
// workgroup ends there, no marker is read.  Flushed by the window rule of device_sweep.hpp, the odd last marker before the
// sweep; the rest sums leave with every flush.  !LDS: a term's limbs go straight into the global rows; the tile stays.
template <bool P, bool W, bool LDS, bool NT>
__global__ void __launch_bounds__(1024)
k_power_exact(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst g, const DistGeom dg,
              const double *E, const PowerFxArgs a, int dyn_tail) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ unsigned sDraw;                 // the drawn chunks' counter
  __shared__ unsigned long long sMax;        // the bits of max |E|
  __shared__ unsigned long long sRest[2];    // the workgroup's rest sums of a window, per set
  constexpr int NS = (P ? 1 : 0) + (W ? 1 : 0);
  const int nxv = dg.nxo * dg.nvo;
  double *sE = reinterpret_cast<double *>(smem);
  unsigned long long *sP = reinterpret_cast<unsigned long long *>(smem + power_tile_bytes(g.nx));
  unsigned long long *acc = reinterpret_cast<unsigned long long *>(a.acc), *rej = reinterpret_cast<unsigned long long *>(a.rej);
  if (threadIdx.x == 0) sDraw = 0u;
  if (threadIdx.x < 2) sRest[threadIdx.x] = 0ull;
  if constexpr (LDS)
    for (int i = threadIdx.x; i < NS * nxv; i += blockDim.x) sP[i] = 0ull;
  const unsigned long long mx = pfx_stage_tile(E, sE, g.nx, &sMax);   // (its barriers: the zeroes above are seen too)
  const bool finite = mx < POWER_FX_NONFINITE;
  const int e = finite ? power_fx_exponent(a.e_base, mx) : 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.scale[0] = e;
    a.scale[1] = finite ? 0 : 1;
    a.scale[2] = static_cast<long long>(mx);
  }
  if (!finite) return;
  const double inv_q = ldexp(1.0, -e);
  PowerRestFx r;
  auto one = [&](double px, double pv, double pp, double pw) { pfx_one<P, W, LDS>(px, pv, pp, pw, g, dg, sE, sP, acc, rej, nxv, inv_q, r); };
  auto flush = [&]() {
    __syncthreads();
    pfx_flush<P, W, LDS>(sP, acc, nxv, r, sRest);
    __syncthreads();
    pfx_rest_out<NS>(sRest, acc, nxv);
  };
  if ((np & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // the odd last marker (before the pairs: inside the first window)
    const int64_t i = tidx(np - 1);
    one(x[i], v[i], P ? p[i] : 0.0, W ? w[i] : 0.0);
  }
  const PairRows rows = window_rows(pair_rows(np >> 1, dyn_tail));
  pair_sweep<P, W, NT>(x, v, p, w, np >> 1, rows, &sDraw, one, [&](int k) {
    if (window_due(k, rows)) flush();
  });
  flush();
}

// what the kernel indexes must be what the plan sized: the LDS holds exactly the tile, and the pass's planes where they
// live there
bool check_pass(const PowerPass &ps, const GridConst &g, const DistGeom &dg) {
  const int sets = (ps.p ? 1 : 0) + (ps.w ? 1 : 0);
  const size_t plane = sizeof(double) * static_cast<size_t>(dg.nxo) * static_cast<size_t>(dg.nvo);
  return sets != 0 && ps.sets == sets && g.nx >= 1 && dg.nxo >= 1 && dg.nvo >= 2 &&
         ps.bytes == power_tile_bytes(g.nx) + (ps.lds ? sets * plane : 0) && ps.threads == 1024 && ps.blocks >= 1 &&
         ps.first_set >= 0 && ps.first_set + sets <= 2;
}

}  // namespace

hipError_t launch_power(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst &g,
                        const DistGeom &dg, const double *E, double *planes, double *rest, const PowerPass &ps, int dyn_tail,
                        hipStream_t st) {
  if (np <= 0) return hipSuccess;
  if (!check_pass(ps, g, dg) || !E || !planes || !rest) return hipErrorInvalidValue;
  double *dst = planes + static_cast<size_t>(ps.first_set) * dg.nxo * dg.nvo;   // the plane of the pass's (first) weight set
  return with_bools(
      [&](auto P, auto W, auto LDS, auto NT) {
        if constexpr (P || W) {
          return launch_kernel(k_power<P, W, LDS, NT>, dim3(static_cast<unsigned>(ps.blocks)), dim3(static_cast<unsigned>(ps.threads)),
                               ps.bytes, st, x, v, p, w, np, g, dg, E, dst, rest + ps.first_set, dyn_tail);
        }
        return hipErrorInvalidValue;
      },
      ps.p, ps.w, ps.lds, ps.nt);
}

// ps: a pass of power_plan_exact -- the same bytes (a 64-bit word is a double's size), so the same check
hipError_t launch_power_exact(const double *x, const double *v, const double *p, const double *w, int64_t np, const GridConst &g,
                              const DistGeom &dg, const double *E, const PowerFxArgs &a, const PowerPass &ps, int dyn_tail,
                              hipStream_t st) {
  if (np <= 0) return hipSuccess;
  static_assert(sizeof(unsigned long long) == sizeof(double), "the planes of words are the planes of doubles, byte for byte");
  if (!check_pass(ps, g, dg) || !E || !a.acc || !a.rej || !a.scale) return hipErrorInvalidValue;
  PowerFxArgs b = a;   // the rows and the counters of the pass's (first) weight set
  b.acc = a.acc + static_cast<size_t>(ps.first_set) * power_fx_set_words(dg.nxo, dg.nvo);
  b.rej = a.rej + ps.first_set * 2;
  return with_bools(
      [&](auto P, auto W, auto LDS, auto NT) {
        if constexpr (P || W) {
          return launch_kernel(k_power_exact<P, W, LDS, NT>, dim3(static_cast<unsigned>(ps.blocks)),
                               dim3(static_cast<unsigned>(ps.threads)), ps.bytes, st, x, v, p, w, np, g, dg, E, b, dyn_tail);
        }
        return hipErrorInvalidValue;
      },
      ps.p, ps.w, ps.lds, ps.nt);
}

}  // namespace pic1dp
