// device_moments.hpp -- the velocity moments of the markers on the field grid (include/pic1dp_hip.h pic1dp_hip_moments):
// what one marker adds to a workgroup's LDS planes, the sweep over a workgroup's marker pairs, and the flush of the planes --
// as doubles (k_moments) and as whole quanta in integer planes (k_moments_exact; pic1dp_hip_moments_exact).
// Used by kernels_moments.hip.  The wrap and the cell come from device_math.hpp as the deposit takes them.
#pragma once
#include "device_math.hpp"

namespace pic1dp {
namespace {

// planes of a weight set in a pass of powers KMASK (bit k: v^k), and where power k lies among them
template <int KMASK>
constexpr int moments_nk() { return __builtin_popcount(static_cast<unsigned>(KMASK)); }
template <int KMASK>
constexpr int moments_slot(int k) { return __builtin_popcount(static_cast<unsigned>(KMASK) & ((1u << k) - 1u)); }

// One weight set of one marker: a0 = wl q, b0 = (1 - wl) q, a_k = a_(k-1) v, every product rounded on its own (the build
// contracts nothing); the powers of KMASK go to cells ix and ir of their planes sM[slot][cell].  The chain runs through
// the powers a pass does not hold, so a term has the same bits whichever pass adds it.
template <int KMASK>
__device__ __forceinline__ void moments_set(double *sM, int nx, int ix, int ir, double wl, double wr, double q, double v) {
  double a = wl * q, b = wr * q;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k > 0) {
      a = a * v;
      b = b * v;
    }
    if ((KMASK >> k) & 1) {
      double *pl = sM + moments_slot<KMASK>(k) * nx;
      lds_add(pl + ix, a);
      lds_add(pl + ir, b);
    }
    if ((KMASK >> (k + 1)) == 0) break;   // (no higher power in this pass)
  }
}

// one marker: the deposit's wrap (not stored back) and cell; the right-hand neighbour of the last cell is cell 0
template <bool P, bool W, int KMASK>
__device__ __forceinline__ void moments_one(double x, double v, double pp, double pw, const GridConst &g, double *sM) {
  const double px = wrap(x, g.lx);
  int ix;
  double wl;
  locate(px, g, ix, wl);
  const int ir = ix + 1 == g.nx ? 0 : ix + 1;
  const double wr = 1.0 - wl;
  if constexpr (P) moments_set<KMASK>(sM, g.nx, ix, ir, wl, wr, pp, v);
  if constexpr (W) moments_set<KMASK>(sM + (P ? moments_nk<KMASK>() * g.nx : 0), g.nx, ix, ir, wl, wr, pw, v);
}

// The sweep of k_ptcldist (kernels_diag.hip pair_sweep) over a workgroup's rows of marker pairs -- pairs as double2, the
// NEXT trip's loads issued before this trip's atomics, dealt and drawn rows (device_math.hpp pair_rows) -- loading only
// the arrays the pass's planes need: x, v, and p and / or w.  one(x, v, p, w) per marker; after_trip(k) once per trip, k
// the trips done.
// (A second body of pair_sweep's dealt-and-drawn-rows loop, to be kept in step with it until the two are one sweep with
// the loads as template flags: DESIGN.md 8.)
template <bool P, bool W, bool NT, class One, class After>
__device__ __forceinline__ void moments_sweep(const double *x, const double *v, const double *p, const double *w, int64_t npair,
                                              const PairRows &rows, unsigned *sDraw, One &&one, After &&after_trip) {
  const double2 *x2 = reinterpret_cast<const double2 *>(x), *v2 = reinterpret_cast<const double2 *>(v);
  const double2 *p2 = reinterpret_cast<const double2 *>(p), *w2 = reinterpret_cast<const double2 *>(w);
  int k = 0;
  int64_t j = rows.first + threadIdx.x;
  bool have = rows.dealt > 0 || draw_chunk(rows, sDraw, j);
  double2 X = make_double2(0.0, 0.0), V = X, Pq = X, Wq = X;
  if (have && j < npair) {
    const int64_t o = tidx2(j);
    X = ld2t<NT>(x2 + o), V = ld2t<NT>(v2 + o);
    if constexpr (P) Pq = ld2t<NT>(p2 + o);
    if constexpr (W) Wq = ld2t<NT>(w2 + o);
  }
  while (have) {
    int64_t jn = j + rows.stride;
    bool have_n = true;
    if (++k >= rows.dealt) have_n = draw_chunk(rows, sDraw, jn);
    double2 Xn = make_double2(0.0, 0.0), Vn = Xn, Pn = Xn, Wn = Xn;
    if (have_n && jn < npair) {  // the next trip's loads are under way while this trip's atomics run
      const int64_t o = tidx2(jn);
      Xn = ld2t<NT>(x2 + o), Vn = ld2t<NT>(v2 + o);
      if constexpr (P) Pn = ld2t<NT>(p2 + o);
      if constexpr (W) Wn = ld2t<NT>(w2 + o);
    }
    if (j < npair) {
      one(X.x, V.x, Pq.x, Wq.x);
      one(X.y, V.y, Pq.y, Wq.y);
    }
    after_trip(k);
    X = Xn, V = Vn, Pq = Pn, Wq = Wn;
    j = jn;
    have = have_n;
  }
}

// the workgroup's planes into the global ones: one global atomic per non-zero word, the start word rotated by workgroup
// (flush_rho); LDS plane l = (set, slot) is power k(slot) of that set: out[(set * 4 + k) * nx + cell]
template <bool P, bool W, int KMASK>
__device__ __forceinline__ void moments_flush(const double *sM, double *out, int nx) {
  constexpr int NK = moments_nk<KMASK>();
  constexpr int NPL = ((P ? 1 : 0) + (W ? 1 : 0)) * NK;
  const int ntot = NPL * nx;
  const int rot = static_cast<int>((static_cast<long long>(blockIdx.x) * ntot) / gridDim.x);
  for (int i = threadIdx.x; i < ntot; i += blockDim.x) {
    int j = i + rot;
    if (j >= ntot) j -= ntot;
    const double val = sM[j];
    if (val != 0.0) {
      const int l = j / nx, cell = j - l * nx;
      const int set = l / NK, slot = l - set * NK;
      const int k = KMASK == 0xF ? slot : (KMASK == 0x3 ? slot : slot + 2);
      glb_add(&out[static_cast<size_t>(set * 4 + k) * nx + cell], val);
    }
  }
}

// ---------------------------------------------------------------------------
// The exact kind (include/pic1dp_hip.h pic1dp_hip_moments_exact): the very terms of moments_set, each
// rounded once to whole quanta 2^e[k] and summed as integers.  A workgroup's LDS holds ONE signed 64-bit word per (plane,
// cell), plane-major as the doubles above and byte for byte their size; the flush splits a word into (hi, lo 32 bits)
// and adds the two into the global rows acc[((set 4 + k) 2 + h) nx + cell], h = 0 hi, 1 lo.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void mfx_glb_add(unsigned long long *p, unsigned long long v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one term into its word: n = rint(term 2^-e) (term 2^-e is exact: ONE rounding, to nearest even); 2^44 quanta or more, or a
// NaN, is not summed but counted in *rej.  The integer as two's complement as dfx_bin_add forms it (device_diag.hpp): for
// |n| < 2^44 the sum with 1.5 2^52 is exact and its low bits are n.
__device__ __forceinline__ void mfx_term(unsigned long long *word, double term, double inv_q, unsigned long long *rej) {
  const double t = __builtin_rint(term * inv_q);
  if (!(fabs(t) < DIAG_FX_LIMIT)) {
    mfx_glb_add(rej, 1ull);
    return;
  }
  const unsigned long long n = static_cast<unsigned long long>(__double_as_longlong(t + 6755399441055744.0)) - 0x4338000000000000ull;
  __hip_atomic_fetch_add(word, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// moments_set with integer planes; rej: this weight set's four counters, by power of v
template <int KMASK>
__device__ __forceinline__ void mfx_set(unsigned long long *sM, int nx, int ix, int ir, double wl, double wr, double q, double v,
                                        const MomentsFxArgs &fx, unsigned long long *rej) {
  double a = wl * q, b = wr * q;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k > 0) {
      a = a * v;
      b = b * v;
    }
    if ((KMASK >> k) & 1) {
      unsigned long long *pl = sM + moments_slot<KMASK>(k) * nx;
      mfx_term(pl + ix, a, fx.inv_q[k], rej + k);
      mfx_term(pl + ir, b, fx.inv_q[k], rej + k);
    }
    if ((KMASK >> (k + 1)) == 0) break;   // (no higher power in this pass)
  }
}
template <bool P, bool W, int KMASK>
__device__ __forceinline__ void mfx_one(double x, double v, double pp, double pw, const GridConst &g, unsigned long long *sM,
                                        const MomentsFxArgs &fx) {
  const double px = wrap(x, g.lx);
  int ix;
  double wl;
  locate(px, g, ix, wl);
  const int ir = ix + 1 == g.nx ? 0 : ix + 1;
  const double wr = 1.0 - wl;
  unsigned long long *rej = reinterpret_cast<unsigned long long *>(fx.rej);
  if constexpr (P) mfx_set<KMASK>(sM, g.nx, ix, ir, wl, wr, pp, v, fx, rej);
  if constexpr (W) mfx_set<KMASK>(sM + (P ? moments_nk<KMASK>() * g.nx : 0), g.nx, ix, ir, wl, wr, pw, v, fx, rej + (P ? 4 : 0));
}
// the workgroup's words into the global (hi, lo) rows, zeroed on the way: two non-returning 64-bit integer atomics per
// non-zero word, the start word rotated by workgroup; the caller puts barriers around it
template <bool P, bool W, int KMASK>
__device__ __forceinline__ void mfx_flush(unsigned long long *sM, const MomentsFxArgs &fx, int nx) {
  constexpr int NK = moments_nk<KMASK>();
  constexpr int NPL = ((P ? 1 : 0) + (W ? 1 : 0)) * NK;
  const int ntot = NPL * nx;
  unsigned long long *acc = reinterpret_cast<unsigned long long *>(fx.acc);
  const int rot = static_cast<int>((static_cast<long long>(blockIdx.x) * ntot) / gridDim.x);
  for (int i = threadIdx.x; i < ntot; i += blockDim.x) {
    int j = i + rot;
    if (j >= ntot) j -= ntot;
    const unsigned long long w = sM[j];
    if (w == 0ull) continue;
    sM[j] = 0ull;
    const int l = j / nx, cell = j - l * nx;
    const int set = l / NK, slot = l - set * NK;
    const int k = KMASK == 0xC ? slot + 2 : slot;
    unsigned long long *row = acc + static_cast<size_t>(set * 4 + k) * 2 * nx + cell;
    const unsigned long long lo = w & 0xffffffffull;
    const unsigned long long hi = static_cast<unsigned long long>(static_cast<long long>(w) >> 32);   // (arithmetic: the sign goes with hi)
    if (hi) mfx_glb_add(row, hi);
    if (lo) mfx_glb_add(row + nx, lo);
  }
}

}  // namespace
}  // namespace pic1dp
