// kernels_load.hip -- the on-device particle load (include/pic1dp_hip.h pic1dp_hip_particle_load_device; the definition:
// load_seq.hpp; the per-marker part: device_load.hpp): one streaming pass that writes a species' slab, 32 B per slot, and
// reads nothing.  gfx950, wave64.
#include <hip/hip_runtime.h>

#include "device_load.hpp"
#include "kernels.hpp"
#include "launch_policy.hpp"

namespace pic1dp {

namespace {

// Slots [0, nalloc) of the four arrays, pair by pair as double2 (kernels.hpp tidx2).  A workgroup takes whole chunks of
// LOAD_CHUNK markers = one tile group: the x, v, w and p tiles of a group lie side by side in the slab, so the workgroup
// writes 128 KiB in one piece, the layout's own stream.  Slot i < np is global marker g0 + i, made from its index alone;
// slots in [np, nalloc) get +0.0; an odd nalloc's last slot is stored by one thread as a single double.  Every thread
// keeps max |p| and max |w| of its valid markers (a NaN is never the larger); wave by shuffles, workgroup through the LDS,
// then one non-returning 64-bit integer max per word and workgroup on the bit patterns.
template <int DIST, int KIND, bool NONLINEAR, bool NT>
__global__ void __launch_bounds__(256)
k_load(const LoadArgs a) {
  __shared__ unsigned long long scr[2][4];
  exp_table_init();
  __syncthreads();
  double maxp = 0.0, maxw = 0.0;
  const int64_t nchunk = (a.nalloc + LOAD_CHUNK - 1) / LOAD_CHUNK;
  for (int64_t t = blockIdx.x; t < nchunk; t += gridDim.x) {
    const int64_t jbase = t * (LOAD_CHUNK / 2);
    for (int jj = threadIdx.x; jj < static_cast<int>(LOAD_CHUNK / 2); jj += blockDim.x) {
      const int64_t j = jbase + jj, i0 = 2 * j, i1 = i0 + 1;
      if (i0 >= a.nalloc) break;
      double x[2] = {0.0, 0.0}, v[2] = {0.0, 0.0}, p[2] = {0.0, 0.0}, w[2] = {0.0, 0.0};
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (i0 + e < a.np) {
          double uv, ux;
          load_uniforms_dev<KIND>(a.key, a.g0 + static_cast<unsigned long long>(i0 + e), uv, ux);
          load_marker<DIST, NONLINEAR>(a.k, uv, ux, x[e], v[e], p[e], w[e]);
          const double ap = fabs(p[e]), aw = fabs(w[e]);
          if (ap > maxp) maxp = ap;
          if (aw > maxw) maxw = aw;
        }
      }
      if (i1 < a.nalloc) {
        const int64_t o = tidx2(j);
        st2t<NT>(reinterpret_cast<double2 *>(a.x) + o, x[0], x[1]);
        st2t<NT>(reinterpret_cast<double2 *>(a.v) + o, v[0], v[1]);
        st2t<NT>(reinterpret_cast<double2 *>(a.w) + o, w[0], w[1]);
        st2t<NT>(reinterpret_cast<double2 *>(a.p) + o, p[0], p[1]);
      } else {  // the odd last slot
        const int64_t o = tidx(i0);
        a.x[o] = x[0];
        a.v[o] = v[0];
        a.w[o] = w[0];
        a.p[o] = p[0];
      }
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned long long m[2] = {static_cast<unsigned long long>(__double_as_longlong(maxp)),
                             static_cast<unsigned long long>(__double_as_longlong(maxw))};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    unsigned long long t = m[k];
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long u = __shfl_down(t, off, 64);
      t = u > t ? u : t;
    }
    if (lane == 0) scr[k][wave] = t;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long t = 0ull;
    for (int wv = 0; wv < static_cast<int>(blockDim.x >> 6); ++wv) t = scr[threadIdx.x][wv] > t ? scr[threadIdx.x][wv] : t;
    if (t) (void)__hip_atomic_fetch_max(a.maxpw + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <int DIST, int KIND, bool NONLINEAR>
hipError_t launch_nt(const LoadArgs &a, const LoadLaunch &ll, hipStream_t st) {
  return ll.nt ? launch_kernel(k_load<DIST, KIND, NONLINEAR, true>, dim3(ll.blocks), dim3(ll.threads), 0, st, a)
               : launch_kernel(k_load<DIST, KIND, NONLINEAR, false>, dim3(ll.blocks), dim3(ll.threads), 0, st, a);
}
template <int DIST>
hipError_t launch_dist(const LoadArgs &a, int kind, bool nonlinear, const LoadLaunch &ll, hipStream_t st) {
  if (kind == LOAD_RANDOM)
    return nonlinear ? launch_nt<DIST, LOAD_RANDOM, true>(a, ll, st) : launch_nt<DIST, LOAD_RANDOM, false>(a, ll, st);
  return nonlinear ? launch_nt<DIST, LOAD_QUIET, true>(a, ll, st) : launch_nt<DIST, LOAD_QUIET, false>(a, ll, st);
}

}  // namespace

hipError_t launch_load(const LoadArgs &a, int kind, int iptcldist, bool nonlinear, const LoadLaunch &ll, hipStream_t st) {
  if (a.nalloc <= 0) return hipSuccess;
  if (kind != LOAD_RANDOM && kind != LOAD_QUIET) return hipErrorInvalidValue;
  if (ll.threads != 256 || ll.blocks < 1 || a.np < 0 || a.np > a.nalloc) return hipErrorInvalidValue;  // (the kernel's scratch holds four waves)
  switch (iptcldist) {
    case 1: return launch_dist<1>(a, kind, nonlinear, ll, st);
    case 2: return launch_dist<2>(a, kind, nonlinear, ll, st);
    case 3: return launch_dist<3>(a, kind, nonlinear, ll, st);
    default: return launch_dist<0>(a, kind, nonlinear, ll, st);
  }
}

}  // namespace pic1dp
