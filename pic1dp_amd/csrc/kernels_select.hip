// kernels_select.hip -- off the timed path: select and gather markers on the device (include/pic1dp_hip.h pic1dp_hip_select,
// pic1dp_hip_gather).  An order-preserving stream compaction in three launches with no waiting between
// workgroups -- no spins, no look-back, no atomics: k_select_count (one count per fixed chunk of the markers),
// k_select_scan (one workgroup: the exclusive prefix of the counts and the total), k_select_write (the same chunks again,
// the predicate recomputed, ranks inside a chunk from wave ballots).  The chunks depend on np alone and the ranks on the
// logical index alone, so the output is in ascending logical index whatever the launch shape.  k_gather: one thread per
// entry.  gfx950, wave64.
#include <hip/hip_runtime.h>

#include "device_select.hpp"
#include "kernels.hpp"
#include "launch_policy.hpp"

namespace pic1dp {

namespace {

// a thread's count over the workgroup: wave by shuffles, workgroup through scr[16] (the caller alternates two of them, so
// one barrier per sum is enough: a wave passes the next sum's barrier only after its reads of this one)
__device__ __forceinline__ unsigned select_block_sum(unsigned mine, unsigned *scr) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = static_cast<int>(blockDim.x >> 6);
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
  if (lane == 0) scr[wave] = mine;
  __syncthreads();
  unsigned t = 0u;
  for (int w = 0; w < nw; ++w) t += scr[w];
  return t;
}

// counts[c] <- the markers of chunk c the rule selects.  A thread counts its pairs trip by trip in a register; at the end
// of a chunk the workgroup adds up (the odd last marker, np odd, is thread 0's in the last chunk) and thread 0 stores.
template <bool NT>
__global__ void __launch_bounds__(1024)
k_select_count(const double *x, const double *v, int64_t np, int64_t nchunk, const SelectRule r, unsigned long long *counts) {
  __shared__ unsigned sRed[2][16];
  unsigned acc = 0u;
  int par = 0;
  select_sweep<NT>(
      x, v, np >> 1, nchunk, [](int64_t) { return true; },
      [&](int64_t, int64_t j, bool valid, const double2 &X, const double2 &V) {
        if (valid) {
          acc += select_one(X.x, V.x, 2 * j, r) ? 1u : 0u;
          acc += select_one(X.y, V.y, 2 * j + 1, r) ? 1u : 0u;
        }
      },
      [&](int64_t c) {
        if (c == nchunk - 1 && (np & 1) && threadIdx.x == 0) {
          const int64_t o = tidx(np - 1);
          acc += select_one(x[o], v[o], np - 1, r) ? 1u : 0u;
        }
        const unsigned t = select_block_sum(acc, sRed[par]);
        par ^= 1;
        if (threadIdx.x == 0) counts[c] = t;
        acc = 0u;
      });
}

// counts[c] <- counts[0] + ... + counts[c - 1] in place for c < nchunk, counts[nchunk] <- the total.  One workgroup, rounds
// of blockDim.x counts with a running carry: a wave's inclusive scan by shuffles, the waves' totals through the LDS.
__global__ void __launch_bounds__(1024)
k_select_scan(unsigned long long *counts, int64_t nchunk) {
  __shared__ unsigned long long sW[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = static_cast<int>(blockDim.x >> 6);
  unsigned long long carry = 0ull;
  for (int64_t base = 0; base < nchunk; base += blockDim.x) {
    const int64_t i = base + threadIdx.x;
    const unsigned long long val = i < nchunk ? counts[i] : 0ull;
    unsigned long long incl = val;
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    if (lane == 63) sW[wave] = incl;
    __syncthreads();
    unsigned long long before = 0ull, total = 0ull;
    for (int w = 0; w < nw; ++w) {
      const unsigned long long t = sW[w];
      if (w < wave) before += t;
      total += t;
    }
    if (i < nchunk) counts[i] = carry + before + (incl - val);
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[nchunk] = carry;
}

// selected marker i of global rank rk: stored where rk < cap; p and w are loaded only then
__device__ __forceinline__ void select_emit(unsigned long long rk, int64_t cap, int64_t i, double xv, double vv, const SelectArrays &a,
                                            const SelectOut &out) {
  if (rk >= static_cast<unsigned long long>(cap)) return;
  const int64_t o = tidx(i);
  if (out.index) out.index[rk] = i;
  if (out.x) out.x[rk] = xv;
  if (out.v) out.v[rk] = vv;
  if (out.p) out.p[rk] = a.p[o];
  if (out.w) out.w[rk] = a.w[o];
}

// The chunks again, those that hold a selected marker of rank below cap (prefix[c] < prefix[c + 1] and prefix[c] < cap: the
// others are not read).  Per trip a lane holds markers 2 j and 2 j + 1 and contributes 0, 1 or 2; the order is lane-major:
// a marker's rank inside the wave's trip is the selected markers of the lanes below (two ballots, two popcounts) and, for
// the second marker, the lane's first; the waves' totals go through the LDS (two buffers in turn: one barrier per trip)
// and the chunk's running base is carried from trip to trip.  The odd last marker comes after the last chunk's pairs.
template <bool NT>
__global__ void __launch_bounds__(1024)
k_select_write(const SelectArrays a, int64_t np, int64_t nchunk, const SelectRule r, const unsigned long long *prefix, int64_t cap,
               const SelectOut out) {
  __shared__ unsigned sW[2][16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = static_cast<int>(blockDim.x >> 6);
  const unsigned long long below = (1ull << lane) - 1ull, ucap = static_cast<unsigned long long>(cap);
  unsigned long long base = 0ull;
  bool fresh = true;
  int par = 0;
  select_sweep<NT>(
      a.x, a.v, np >> 1, nchunk,
      [&](int64_t c) {
        const unsigned long long p0 = prefix[c];
        return prefix[c + 1] > p0 && p0 < ucap;
      },
      [&](int64_t c, int64_t j, bool valid, const double2 &X, const double2 &V) {
        if (fresh) {
          base = prefix[c];
          fresh = false;
        }
        const bool s0 = valid && select_one(X.x, V.x, 2 * j, r), s1 = valid && select_one(X.y, V.y, 2 * j + 1, r);
        const unsigned long long b0 = __ballot(s0), b1 = __ballot(s1);
        const unsigned before = static_cast<unsigned>(__popcll(b0 & below) + __popcll(b1 & below));
        if (lane == 0) sW[par][wave] = static_cast<unsigned>(__popcll(b0) + __popcll(b1));
        __syncthreads();
        unsigned waves_before = 0u, total = 0u;
        for (int w = 0; w < nw; ++w) {
          const unsigned t = sW[par][w];
          if (w < wave) waves_before += t;
          total += t;
        }
        par ^= 1;
        unsigned long long rk = base + waves_before + before;
        if (s0) select_emit(rk++, cap, 2 * j, X.x, V.x, a, out);
        if (s1) select_emit(rk, cap, 2 * j + 1, X.y, V.y, a, out);
        base += total;
      },
      [&](int64_t c) {
        if (c == nchunk - 1 && (np & 1) && threadIdx.x == 0) {
          const int64_t o = tidx(np - 1);
          const double xv = a.x[o], vv = a.v[o];
          if (select_one(xv, vv, np - 1, r)) select_emit(base, cap, np - 1, xv, vv, a, out);
        }
        fresh = true;
      });
}

// one thread per entry: four loads at tidx(index), four stores
__global__ void __launch_bounds__(256)
k_gather(const SelectArrays cur, const SelectArrays tail, int64_t np, const long long *index, int64_t n, const SelectOut out) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int64_t i = index[k], o = tidx(i);
  const SelectArrays &s = i < np ? cur : tail;
  if (out.x) out.x[k] = s.x[o];
  if (out.v) out.v[k] = s.v[o];
  if (out.p) out.p[k] = s.p[o];
  if (out.w) out.w[k] = s.w[o];
}

// what the kernels index must be what the plan sized
bool check_plan(const SelectPlan &pl, int64_t np) {
  const int64_t npair = np >> 1;
  return np > 0 && pl.chunk_pairs == SELECT_CHUNK_PAIRS && pl.nchunk >= 1 && (pl.nchunk - 1) * pl.chunk_pairs <= npair &&
         npair <= pl.nchunk * pl.chunk_pairs && pl.threads >= 64 && pl.threads <= 1024 && pl.threads % 64 == 0 && pl.blocks >= 1 &&
         pl.scan_threads >= 64 && pl.scan_threads <= 1024 && pl.scan_threads % 64 == 0;
}

}  // namespace

hipError_t launch_select_count(const SelectArrays &a, int64_t np, const SelectRule &r, unsigned long long *counts,
                               const SelectPlan &pl, hipStream_t st) {
  if (!check_plan(pl, np) || !a.x || !a.v || !counts) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(pl.blocks)), block(static_cast<unsigned>(pl.threads));
  return pl.nt ? launch_kernel(k_select_count<true>, grid, block, 0, st, a.x, a.v, np, pl.nchunk, r, counts)
               : launch_kernel(k_select_count<false>, grid, block, 0, st, a.x, a.v, np, pl.nchunk, r, counts);
}

hipError_t launch_select_scan(unsigned long long *counts, const SelectPlan &pl, hipStream_t st) {
  if (pl.nchunk < 1 || pl.scan_threads < 64 || pl.scan_threads > 1024 || pl.scan_threads % 64 || !counts) return hipErrorInvalidValue;
  return launch_kernel(k_select_scan, dim3(1), dim3(static_cast<unsigned>(pl.scan_threads)), 0, st, counts, pl.nchunk);
}

hipError_t launch_select_write(const SelectArrays &a, int64_t np, const SelectRule &r, const unsigned long long *prefix,
                               int64_t cap, const SelectOut &out, const SelectPlan &pl, hipStream_t st) {
  if (cap <= 0) return hipSuccess;
  if (!check_plan(pl, np) || !a.x || !a.v || !a.p || !a.w || !prefix) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(pl.blocks)), block(static_cast<unsigned>(pl.threads));
  return pl.nt ? launch_kernel(k_select_write<true>, grid, block, 0, st, a, np, pl.nchunk, r, prefix, cap, out)
               : launch_kernel(k_select_write<false>, grid, block, 0, st, a, np, pl.nchunk, r, prefix, cap, out);
}

hipError_t launch_gather(const SelectArrays &cur, const SelectArrays &tail, int64_t np, const long long *index, int64_t n,
                         const SelectOut &out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!index || !cur.x || !cur.v || !cur.p || !cur.w || !tail.x || !tail.v || !tail.p || !tail.w) return hipErrorInvalidValue;
  const int64_t blocks = (n + 255) / 256;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  return launch_kernel(k_gather, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, st, cur, tail, np, index, n, out);
}

}  // namespace pic1dp
