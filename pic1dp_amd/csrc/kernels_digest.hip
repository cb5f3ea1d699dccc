// kernels_digest.hip -- the state digest (include/pic1dp_hip.h pic1dp_hip_state_digest; the mixing: digest.hpp): one
// streaming pass over a species' slab, 32 B read per slot, nothing written but four words per workgroup.  gfx950, wave64.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "digest.hpp"
#include "kernels.hpp"
#include "launch_policy.hpp"

namespace pic1dp {

namespace {

// Slots [0, nalloc) of the four arrays, pair by pair as double2 (the diagnostics pass's sweep shape; a wave's 64 pairs lie
// in one tile: kernels.hpp tidx2).  Slot i of array k comes from cur[k] while i < np and from first[k] beyond (the tail
// slots are only defined in set 0: pic1dp_hip_particles_download); the slab holds nalloc + 2 slots, so the pair that
// straddles nalloc is read whole and its second slot left out of the sum.  i is the logical index: 2 j and 2 j + 1.
// Every thread keeps four sums; wave by shuffles, workgroup through the LDS, then one non-returning 64-bit integer
// atomic per array and workgroup.  Integer sums: the result does not depend on the launch shape.
// The 64-bit multiplies (two per slot; the slot's multiple of the golden ratio is one multiply per pair and one addition)
// are a handful of 32-bit multiplies each, well inside what the loads leave idle.
template <bool NT>
__global__ void __launch_bounds__(256)
k_state_digest(const DigestArgs a) {
  __shared__ unsigned long long scr[4][4];
  unsigned long long s[4] = {0ull, 0ull, 0ull, 0ull};
  const int64_t npair = (a.nalloc + 1) >> 1;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t j = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < npair; j += stride) {
    const int64_t i0 = 2 * j, i1 = i0 + 1, o = tidx2(j);
    const bool from_cur = i0 < a.np, from_first = i1 >= a.np, second = i1 < a.nalloc;
    double2 c[4], f[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      c[k] = f[k] = make_double2(0.0, 0.0);
      if (from_cur) c[k] = ld2t<NT>(reinterpret_cast<const double2 *>(a.cur[k]) + o);
      if (from_first) f[k] = ld2t<NT>(reinterpret_cast<const double2 *>(a.first[k]) + o);
    }
    const unsigned long long g0 = static_cast<unsigned long long>(i0 + 1) * DIGEST_GOLD, g1 = g0 + DIGEST_GOLD;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double e0 = from_cur ? c[k].x : f[k].x, e1 = from_first ? f[k].y : c[k].y;
      s[k] += digest_mix(static_cast<unsigned long long>(__double_as_longlong(e0)), g0);
      if (second) s[k] += digest_mix(static_cast<unsigned long long>(__double_as_longlong(e1)), g1);
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned long long t = s[k];
    for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
    if (lane == 0) scr[k][wave] = t;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    unsigned long long t = 0ull;
    for (int w = 0; w < static_cast<int>(blockDim.x >> 6); ++w) t += scr[threadIdx.x][w];
    (void)__hip_atomic_fetch_add(a.out + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace

hipError_t launch_state_digest(const DigestArgs &a, const DigestLaunch &dl, hipStream_t st) {
  if (a.nalloc <= 0) return hipSuccess;
  if (dl.threads != 256 || dl.blocks < 1) return hipErrorInvalidValue;  // (the kernel's scratch holds four waves)
  return dl.nt ? launch_kernel(k_state_digest<true>, dim3(dl.blocks), dim3(dl.threads), 0, st, a)
               : launch_kernel(k_state_digest<false>, dim3(dl.blocks), dim3(dl.threads), 0, st, a);
}

}  // namespace pic1dp
