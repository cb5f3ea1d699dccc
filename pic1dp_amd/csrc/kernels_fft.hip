// kernels_fft.hip -- the opt-in FFT transform of the mode-filter field solve (pic1dp_hip_set_field_transform(ctx, 1);
// DESIGN.md 2.11).  The same solve as k_field_solve / the wide pair (kernels_field.hip): the kept modes from the DFT of
// field_chargeden, E from them -- but the DFT comes from a mixed-radix (2, 3, 4, 5) Stockham FFT in one workgroup's LDS
// instead of dense cos / -sin tables, so only the sums differ.  gfx950, wave64, FP64.
//
// nx even: the nx real points are packed into n = nx / 2 complex ones, z[j] = rho[2j] + i rho[2j+1], and untangled after
// the transform (and the other way round for E); nx odd: n = nx complex points with zero imaginary parts.  One launch:
// forward FFT, kept-mode pick and scaling, the Hermitian spectrum of E, inverse FFT, E, int E^2 dx.
#include "device_field.hpp"
#include "device_math.hpp"

#include <cmath>
#include <vector>

namespace pic1dp {
namespace {

constexpr int FFT_THREADS = 512;

// one complex double of padding after every 16 (256 B: one row of the 64 four-byte banks), so that the 16-byte accesses
// of a Stockham pass at power-of-two strides spread over the banks
__device__ __host__ __forceinline__ int fft_pad(int i) { return i + (i >> 4); }

__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return double2{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return double2{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return double2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ double2 cscale(double2 a, double s) { return double2{a.x * s, a.y * s}; }
// a times -i (forward) or +i (inverse): the sign of the transform's exponent
template <bool INV>
__device__ __forceinline__ double2 rot(double2 a) {
  return INV ? double2{-a.y, a.x} : double2{a.y, -a.x};
}

// y[q] = sum_r v[r] e^{-+2 pi i r q / R}, in place
template <int R, bool INV>
__device__ __forceinline__ void dft(double2 (&v)[R]) {
  if constexpr (R == 2) {
    const double2 a = v[0], b = v[1];
    v[0] = cadd(a, b);
    v[1] = csub(a, b);
  } else if constexpr (R == 3) {
    constexpr double s = 0.86602540378443864676;  // sin(2 pi / 3)
    const double2 t = cadd(v[1], v[2]);
    const double2 u = csub(v[0], cscale(t, 0.5));
    const double2 w = rot<INV>(cscale(csub(v[1], v[2]), s));
    v[0] = cadd(v[0], t);
    v[1] = cadd(u, w);
    v[2] = csub(u, w);
  } else if constexpr (R == 4) {
    const double2 a = cadd(v[0], v[2]), b = csub(v[0], v[2]), c = cadd(v[1], v[3]), d = rot<INV>(csub(v[1], v[3]));
    v[0] = cadd(a, c);
    v[2] = csub(a, c);
    v[1] = cadd(b, d);
    v[3] = csub(b, d);
  } else {
    static_assert(R == 5, "radix 2, 3, 4 or 5");
    constexpr double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410;  // cos(2 pi / 5), cos(4 pi / 5)
    constexpr double s1 = 0.95105651629515357212, s2 = 0.58778525229247312917;   // sin(2 pi / 5), sin(4 pi / 5)
    const double2 t1 = cadd(v[1], v[4]), t2 = cadd(v[2], v[3]), t3 = csub(v[1], v[4]), t4 = csub(v[2], v[3]);
    const double2 a1 = cadd(cadd(v[0], cscale(t1, c1)), cscale(t2, c2));
    const double2 a2 = cadd(cadd(v[0], cscale(t1, c2)), cscale(t2, c1));
    const double2 b1 = rot<INV>(cadd(cscale(t3, s1), cscale(t4, s2)));
    const double2 b2 = rot<INV>(csub(cscale(t3, s2), cscale(t4, s1)));
    v[0] = cadd(cadd(v[0], t1), t2);
    v[1] = cadd(a1, b1);
    v[4] = csub(a1, b1);
    v[2] = cadd(a2, b2);
    v[3] = csub(a2, b2);
  }
}

// One Stockham pass of radix R over n points: ns = the product of the radices before it.  Butterfly j reads
// src[j + r n/R], twists input r by w_n^(r (j mod ns) n / (ns R)), and writes dst[(j - j mod ns) R + j mod ns + r ns].
// tw holds w_nx^k (k < nx); w_n^k = tw[k tws] with tws = nx / n.
template <int R, bool INV>
__device__ __forceinline__ void fft_pass(const double2 *src, double2 *dst, const double2 *tw, int n, int ns, int tws) {
  const int nb = n / R, step = (n / (ns * R)) * tws;
  for (int j = threadIdx.x; j < nb; j += blockDim.x) {
    const int k = j % ns;
    double2 w[R];
#pragma unroll
    for (int r = 1; r < R; ++r) {
      w[r] = tw[k * r * step];
      if (INV) w[r].y = -w[r].y;
    }
    double2 v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = src[fft_pad(j + r * nb)];
#pragma unroll
    for (int r = 1; r < R; ++r) v[r] = cmul(v[r], w[r]);
    dft<R, INV>(v);
    const int d = (j - k) * R + k;
#pragma unroll
    for (int r = 0; r < R; ++r) dst[fft_pad(d + r * ns)] = v[r];
  }
}

// all passes; returns the buffer that holds the result (the other one is free)
template <bool INV>
__device__ double2 *fft_run(const FftArgs &p, double2 *src, double2 *dst, int tws) {
  int ns = 1;
  for (int s = 0; s < p.npass; ++s) {
    const int R = p.radix[s];
    if (R == 4)
      fft_pass<4, INV>(src, dst, p.tw, p.n, ns, tws);
    else if (R == 2)
      fft_pass<2, INV>(src, dst, p.tw, p.n, ns, tws);
    else if (R == 3)
      fft_pass<3, INV>(src, dst, p.tw, p.n, ns, tws);
    else
      fft_pass<5, INV>(src, dst, p.tw, p.n, ns, tws);
    ns *= R;
    double2 *t = src;
    src = dst;
    dst = t;
    __syncthreads();
  }
  return src;
}

// X[b] = sum_ix rho[ix] e^{-2 pi i b ix / nx} (b < nx) from the forward transform Zc: X[nx - b] = conj X[b] for the real
// rho, so from the lower half; nx even: untangled from the packed transform, X[k] = Ze[k] + w_nx^k Zo[k] with
// Ze = (Zc[k] + conj Zc[n - k]) / 2, Zo = (Zc[k] - conj Zc[n - k]) / 2i
__device__ __forceinline__ double2 spectrum_bin(const FftArgs &p, const double2 *Zc, int nx, int b) {
  const bool upper = 2 * b > nx;
  const int k = upper ? nx - b : b, n = p.n;
  double2 x;
  if (2 * n == nx) {
    const double2 a = Zc[fft_pad(k % n)], c = Zc[fft_pad((n - k) % n)];
    const double2 ze{0.5 * (a.x + c.x), 0.5 * (a.y - c.y)};
    const double2 zo{0.5 * (a.y + c.y), -0.5 * (a.x - c.x)};
    x = cadd(ze, cmul(p.tw[k], zo));
  } else {
    x = Zc[fft_pad(k)];
  }
  if (k == 0) x.y = 0.0;  // (sin 0 = 0: no imaginary part at all, whatever the rounding of the transform)
  if (upper) x.y = -x.y;
  return x;
}

// kept mode m as the direct solve scales it (device_field.hpp mode_scale): R = Re X, I = Im X of its bin,
// mode_re from I, mode_im from R -- as (re, im)
__device__ __forceinline__ double2 kept_mode(const FieldArgs &f, const FftArgs &p, const double2 *Zc, int m) {
  const double2 x = spectrum_bin(p, Zc, f.nx, p.mode_bin[m]);
  return double2{mode_scale(f, false, x.y, f.grad_inv[m]), mode_scale(f, true, x.x, f.grad_inv[m])};
}

// bin k (< nx) of the Hermitian spectrum of E = 2 sum_m (re_m cos - im_m sin)(2 pi m ix / nx) = sum_k S[k] e^{+2 pi i k ix / nx}:
// S[k] = sum of c_m over the modes in bin k + sum of conj c_m over the modes in bin nx - k, c_m = re_m + i im_m
// (ascending m within a bin: duplicated modes count twice, in a fixed order)
__device__ __forceinline__ double2 hermitian_bin(const FieldArgs &f, const FftArgs &p, const double2 *Zc, int k) {
  double2 s{0.0, 0.0};
  for (int i = p.bin_start[k]; i < p.bin_start[k + 1]; ++i) s = cadd(s, kept_mode(f, p, Zc, p.bin_mode[i]));
  const int kc = k == 0 ? 0 : f.nx - k;
  for (int i = p.bin_start[kc]; i < p.bin_start[kc + 1]; ++i) {
    const double2 c = kept_mode(f, p, Zc, p.bin_mode[i]);
    s = double2{s.x + c.x, s.y - c.y};
  }
  return s;
}

__global__ void __launch_bounds__(FFT_THREADS) k_field_fft(const FieldArgs f, const FftArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nx = f.nx, n = p.n, nm = f.nmode;
  const int tws = nx / n;  // 2: packed real transform, 1: complex
  const int np = fft_pad(n - 1) + 1;
  double2 *A = reinterpret_cast<double2 *>(smem), *B = A + np;  // [np] each: the ping-pong buffers
  double *sScr = reinterpret_cast<double *>(B + np);           // [16]
  for (int j = threadIdx.x; j < n; j += blockDim.x)
    A[fft_pad(j)] = tws == 2 ? double2{f.chargeden[2 * j], f.chargeden[2 * j + 1]} : double2{f.chargeden[j], 0.0};
  __syncthreads();
  const double2 *Zc = fft_run<false>(p, A, B, tws);
  double2 *V = Zc == A ? B : A;  // free
  // the kept modes (:234-247) and, beside them, the spectrum of E for the inverse transform -- both read Zc only
  for (int m = threadIdx.x; m < nm; m += blockDim.x) {
    const double2 c = kept_mode(f, p, Zc, m);
    f.mode_re[m] = c.x;
    f.mode_im[m] = c.y;
  }
  for (int k = threadIdx.x; k < n; k += blockDim.x) {
    double2 v;
    if (tws == 2) {  // packed: V[k] = (S[k] + S[k + n]) + i (S[k] - S[k + n]) w_nx^-k, whose inverse is E[2j] + i E[2j+1]
      const double2 s0 = hermitian_bin(f, p, Zc, k), s1 = hermitian_bin(f, p, Zc, k + n);
      double2 w = p.tw[k];
      w.y = -w.y;
      const double2 t = cmul(csub(s0, s1), w);
      v = double2{s0.x + s1.x - t.y, s0.y + s1.y + t.x};
    } else {
      v = hermitian_bin(f, p, Zc, k);
    }
    V[fft_pad(k)] = v;
  }
  __syncthreads();
  const double2 *Y = fft_run<true>(p, V, V == A ? B : A, tws);
  double e2 = 0.0;
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    const double2 y = Y[fft_pad(j)];
    if (tws == 2) {
      f.E[2 * j] = y.x;
      f.E[2 * j + 1] = y.y;
      e2 += y.x * y.x;
      e2 += y.y * y.y;
    } else {
      f.E[j] = y.x;
      e2 += y.x * y.x;
    }
  }
  if (f.history) field_energy_store(e2, sScr, f.lx, f.dnx, f.history);
}

size_t fft_lds_bytes(int n) { return 2 * sizeof(double2) * static_cast<size_t>(fft_pad(n - 1) + 1) + 16 * sizeof(double); }

// n = 2^a 3^b 5^c into passes: fours first, then a two, threes, fives; false for any other prime factor
bool fft_radices(int n, FftArgs *p) {
  int np = 0;
  const int order[4] = {4, 2, 3, 5};
  for (int r : order) {
    while (n % r == 0 && (r != 2 || n % 4 != 0)) {
      if (np == FFT_MAX_PASSES) return false;
      if (p) p->radix[np] = r;
      ++np;
      n /= r;
    }
  }
  if (p) p->npass = np;
  return n == 1;
}

}  // namespace

bool fft_supported(int nx) {
  if (nx < 2 || nx > FFT_MAX_NX) return false;
  if (nx % 2 != 0 && nx > FFT_MAX_ODD_NX) return false;
  const int n = nx % 2 == 0 ? nx / 2 : nx;
  return fft_radices(n, nullptr) && fft_lds_bytes(n) <= PARTICLE_LDS_CAP;
}

hipError_t fft_plan_upload(int nx, const int32_t *modes, int nmode, FftArgs &p, double **d_tw, int **d_idx) {
  if (!fft_supported(nx)) return hipErrorInvalidValue;
  p = FftArgs{};
  p.n = nx % 2 == 0 ? nx / 2 : nx;
  fft_radices(p.n, &p);
  // w_nx^k = e^{-2 pi i k / nx}: k is the angle reduced exactly (an integer below nx); cos / sin in long double, the
  // exact values at the quarter turns, and w^(nx - k) = conj w^k
  std::vector<double> tw(2 * static_cast<size_t>(nx));
  const long double two_pi = 6.283185307179586476925286766559005768L;
  for (int k = 0; 2 * k <= nx; ++k) {
    double c, s;
    if (k == 0) {
      c = 1.0, s = 0.0;
    } else if (2 * k == nx) {
      c = -1.0, s = 0.0;
    } else if (4 * k == nx) {
      c = 0.0, s = 1.0;
    } else {
      const long double a = two_pi * static_cast<long double>(k) / static_cast<long double>(nx);
      c = static_cast<double>(cosl(a));
      s = static_cast<double>(sinl(a));
    }
    tw[2 * static_cast<size_t>(k)] = c;
    tw[2 * static_cast<size_t>(k) + 1] = -s;
    if (k != 0 && 2 * k != nx) {
      tw[2 * static_cast<size_t>(nx - k)] = c;
      tw[2 * static_cast<size_t>(nx - k) + 1] = s;
    }
  }
  // the kept modes by bin b = m mod nx: idx = [bin_start (nx + 1) | bin_mode (nmode) | mode_bin (nmode)]
  std::vector<int> idx(static_cast<size_t>(nx) + 1 + 2 * static_cast<size_t>(nmode), 0);
  int *start = idx.data(), *by_bin = start + nx + 1, *bin = by_bin + nmode;
  for (int m = 0; m < nmode; ++m) {
    bin[m] = static_cast<int>(static_cast<long long>(modes[m]) % nx);
    start[bin[m] + 1]++;
  }
  for (int b = 0; b < nx; ++b) start[b + 1] += start[b];
  std::vector<int> fill(start, start + nx);
  for (int m = 0; m < nmode; ++m) by_bin[fill[bin[m]]++] = m;
  if (!*d_tw) {
    hipError_t e = hipMalloc(d_tw, sizeof(double) * tw.size());
    if (e != hipSuccess) return e;
  }
  if (!*d_idx) {
    hipError_t e = hipMalloc(d_idx, sizeof(int) * idx.size());
    if (e != hipSuccess) return e;
  }
  hipError_t e = hipMemcpy(*d_tw, tw.data(), sizeof(double) * tw.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(*d_idx, idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice);
  p.tw = reinterpret_cast<const double2 *>(*d_tw);
  p.bin_start = *d_idx;
  p.bin_mode = *d_idx + nx + 1;
  p.mode_bin = *d_idx + nx + 1 + nmode;
  return e;
}

hipError_t launch_field_fft(const FieldArgs &f, const FftArgs &p, bool with_local, bool from_chargeden, hipStream_t st) {
  if (!p.tw || (2 * p.n != f.nx && p.n != f.nx)) return hipErrorInvalidValue;
  if (!from_chargeden) {
    hipError_t e = launch_chargeden(f, with_local, st);
    if (e != hipSuccess) return e;
  }
  const int threads = p.n >= 1024 ? FFT_THREADS : 256;
  return launch_kernel(k_field_fft, dim3(1), dim3(threads), fft_lds_bytes(p.n), st, f, p);
}

}  // namespace pic1dp
