// device_load.hpp -- the per-marker part of the on-device particle load (kernels_load.hip k_load; the probe library's check
// of the index function, probe.hip): global marker index -> (u_v, u_x) -> (x, v, p, w).  The definition is load_seq.hpp's;
// this is the kernel's form of it, held against the host's bit for bit (tests/test_gpu_load_device.py).
#pragma once
#include "device_math.hpp"
#include "load_seq.hpp"

namespace pic1dp {
namespace {

// the `digits` base-3 digits of a (a < 3^digits <= 3^11) reversed: 32-bit arithmetic, the division by 3 a multiply-high
__device__ __forceinline__ uint32_t load_rev3(uint32_t a, int digits) {
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < digits; ++i) {
    const uint32_t q = a / 3u;
    r = r * 3u + (a - q * 3u);
    a = q;
  }
  return r;
}
// load_r3 for g < 3^21: g = hi 3^10 + lo by ONE 64-bit division; digit i of g goes to place 20 - i, so the ten digits of
// lo land above the eleven of hi
__device__ __forceinline__ uint64_t load_r3_dev(uint64_t g) {
  const uint64_t hi = g / 59049ull;                                    // 3^10; hi < 3^11
  const uint32_t lo = static_cast<uint32_t>(g - hi * 59049ull);
  return static_cast<uint64_t>(load_rev3(lo, 10)) * 177147ull + load_rev3(static_cast<uint32_t>(hi), 11);   // 3^11
}
__device__ __forceinline__ uint64_t load_bitrev64_dev(uint64_t g) {
  return (static_cast<uint64_t>(__brev(static_cast<uint32_t>(g))) << 32) | __brev(static_cast<uint32_t>(g >> 32));
}
__device__ __forceinline__ double load_unit_dev(uint64_t r) {
  return static_cast<double>(static_cast<long long>(r >> 11)) * 0x1p-53;   // (< 2^53: exact)
}

template <int KIND>
__device__ __forceinline__ void load_uniforms_dev(uint64_t key, uint64_t g, double &uv, double &ux) {
  if constexpr (KIND == LOAD_RANDOM) {
    uv = load_unit_dev(load_draw(key, 2ull * g));
    ux = load_unit_dev(load_draw(key, 2ull * g + 1ull));
  } else {
    uv = load_unit_dev(load_bitrev64_dev(g));
    ux = static_cast<double>(static_cast<long long>(load_r3_dev(g))) / static_cast<double>(LOAD_R3_SPAN);
  }
}

// The marker of (u_v, u_x): the imarker = 2 branch of loader.cpp load_block_species in its operation order (the unit is
// built without FMA contraction), exp as pexp, sin / cos as the device's sincos.  DIST: iptcldist 1..3, 0 the Maxwellian.
template <int DIST, bool NONLINEAR>
__device__ __forceinline__ void load_marker(const LoadConst &k, double uv, double ux, double &x, double &v, double &p, double &w) {
  const double vi = (uv - 0.5) * 2.0 * k.vmax;
  double f;
  if constexpr (DIST == 1) {
    const double q = vi * vi;
    f = k.pref * q * pexp(-q / 2.0) / k.gs;
  } else if constexpr (DIST == 2) {
    const double up = vi + k.v0, um = vi - k.v0;
    f = k.pref * (pexp(-(up * up) / k.a1) + pexp(-(um * um) / k.a1)) / k.g8;
  } else if constexpr (DIST == 3) {
    const double um = vi - k.v0;
    f = k.pref * (k.den * pexp(-(vi * vi) / k.a1) / k.g1 + k.beam * pexp(-(um * um) / k.a2) / k.g2);
  } else {
    const double um = vi - k.v0;
    f = k.pref * pexp(-(um * um) / k.a1) / k.g1;
  }
  const double xi = ux * k.lx;
  double amp = 0.0;
  for (int j = 0; j < k.nim; ++j) {
    double sn, cs;
    sincos(k.kk[j] * xi, &sn, &cs);
    amp = amp + k.mcos[j] * cs + k.msin[j] * sn;
  }
  const double wi = amp * f * 1.0;
  x = xi;
  v = vi;
  w = wi;
  p = NONLINEAR ? f + wi : f;
}

}  // namespace
}  // namespace pic1dp
