// device_fxsum.hpp -- what the exact (integer) sums off the timed path share on the device: a term as a whole number of
// quanta in one two's-complement 64-bit word, the word's split into (hi, lo 32 bits) limbs and their way into the global
// rows, and the workgroup-rotated flush loop.  Used by the exact diagnostics (device_diag.hpp dfx_*) and the
// exact moments (device_moments.hpp mfx_*); how many terms a word may take between two flushes is
// device_sweep.hpp's window rule.
// (Kind 1 of the charge sum lives in the step kernels and keeps its own copy of the split -- device_math.hpp rho_add,
// flush_rho_fx with two LDS words per cell and the limit 2^62 -- so that nothing here can move the timed path.)
#pragma once
#include "device_math.hpp"

namespace pic1dp {
namespace {

// n = rint(term 2^-e) (term 2^-e itself is exact: ONE rounding, to nearest even) as a two's-complement word; false: 2^44
// quanta (DIAG_FX_LIMIT) or more, or a NaN -- not summed, the caller counts it.  For |n| < 2^44 the sum with 1.5 2^52 is
// exact and its low bits are n.
__device__ __forceinline__ bool fx_word44(double term, double inv_q, unsigned long long *n) {
  const double t = __builtin_rint(term * inv_q);
  if (!(fabs(t) < DIAG_FX_LIMIT)) return false;
  *n = static_cast<unsigned long long>(__double_as_longlong(t + 6755399441055744.0)) - 0x4338000000000000ull;
  return true;
}
// a word's limbs: w = hi 2^32 + lo, lo below 2^32, the sign with hi (an arithmetic shift)
__device__ __forceinline__ unsigned long long fx_hi(unsigned long long w) {
  return static_cast<unsigned long long>(static_cast<long long>(w) >> 32);
}
__device__ __forceinline__ unsigned long long fx_lo(unsigned long long w) { return w & 0xffffffffull; }
__device__ __forceinline__ void fx_glb_add(unsigned long long *p, unsigned long long v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// a word into a (hi, lo) pair of global sums: one non-returning 64-bit atomic per non-zero limb
__device__ __forceinline__ void fx_add_limbs(unsigned long long *hi, unsigned long long *lo, unsigned long long w) {
  const unsigned long long h = fx_hi(w), l = fx_lo(w);
  if (h) fx_glb_add(hi, h);
  if (l) fx_glb_add(lo, l);
}
// f(j) for the n words of a workgroup's LDS copy, each once, the start word rotated by workgroup (flush_rho): the
// workgroups of a launch do not all begin at the same global addresses
template <class F>
__device__ __forceinline__ void rotated_words(int n, F &&f) {
  const int rot = static_cast<int>((static_cast<long long>(blockIdx.x) * n) / gridDim.x);
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    int j = i + rot;
    if (j >= n) j -= n;
    f(j);
  }
}

}  // namespace
}  // namespace pic1dp
