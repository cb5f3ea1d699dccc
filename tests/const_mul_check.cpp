// const_mul_check.cpp -- a program of its own (tests/test_const_mul_host.py builds it with the host sanitizers): the decision
// procedure of pic1dp_amd/csrc/const_mul.cpp -- is  fma(yh, x, RN(yl x))  the correctly rounded x / lx for EVERY double x? --
// held against the division itself, bit for bit, on
//   (a) 10^8 random doubles in [0, lx] per proven constant,
//   (b) every double within +-2 ulp of k lx / nx, k = 0 ... nx, nx in {2, 192, 1024, 8192},
//   (c) the procedure's own worst cases: the significands whose quotient lies nearest to a rounding boundary (what the
//       extended Euclidean algorithm on 2^55 / L names), at their own scale and at others -- compared, not assumed;
// and, for a constant the procedure does NOT prove (found by search on the CPU, `const_mul_check --search`, kept as a
// literal), that an operand really rounds differently and that a context's grid constants take the five operations.
// Operands below 2^-500 (0, subnormals) are outside the proof's no-underflow range: there the CELL and WEIGHT locate derives
// from either quotient are compared, which is what device_math.hpp argues for them.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../pic1dp_amd/csrc/const_mul.hpp"
#include "../pic1dp_amd/csrc/kernels.hpp"

using pic1dp::ConstMul;

namespace {

// 2 pi / 0.36 is the default input's box (the literal is that quotient's double), 0x1.8p-6 = 3 * 2^-7
const double kLx[] = {0x1.1740afa84ad8ap+4, 0x1.921fb54442d18p+3, 1.0, 17.0, 0.1, 0x1.8p-6};
// not proven: found by `const_mul_check --search` (the first lx = 12 + (2 k + 1) 2^-49 the procedure rejects)
const double kNotProven = 0x1.800000000019fp+3;   // 12.000000000000737: one of its twelve candidates rounds the other way

bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rng() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

// locate's (cell, weight) from a quotient (device_math.hpp, both forms of the fraction agree for s >= 0)
void cell_of(double q, int nx, long long *ix, double *wl) {
  const double s = q * nx, fl = std::floor(s);
  *ix = static_cast<long long>(fl);
  *wl = 1.0 - (s - fl);
}

long long g_compared = 0;

// one operand: the two operations against the division (outside the no-underflow range: the cells and weights)
bool agree(double x, double lx, const ConstMul &c) {
  ++g_compared;
  const double q2 = pic1dp::const_mul_quotient(x, c.hi, c.lo), qd = x / lx;
  if (std::fabs(x) >= 0x1p-500 && std::fabs(x) <= 0x1p+500) return same(q2, qd);
  for (int nx : {2, 192, 1024, 8192}) {
    long long i2, id;
    double w2, wd;
    cell_of(q2, nx, &i2, &w2);
    cell_of(qd, nx, &id, &wd);
    if (i2 != id || !same(w2, wd)) return false;
  }
  return true;
}

int search(long long n) {
  for (long long k = 1; k <= n; ++k) {
    const double lx = 12.0 + static_cast<double>(2 * k + 1) * 0x1p-49;  // odd significands
    const ConstMul c = pic1dp::const_mul_decide(lx);
    if (!c.proven) {
      std::printf("%a  (%.17g): %d candidates, %d fail\n", lx, lx, c.candidates, c.failed);
      return 0;
    }
  }
  std::printf("none in %lld\n", n);
  return 1;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "--search") == 0) return search(argc > 2 ? std::atoll(argv[2]) : 1000000);
  const long long nrandom = argc > 1 ? std::atoll(argv[1]) : 100000000ll;
  long long bad = 0;
  int proven = 0;
  for (double lx : kLx) {
    std::vector<double> worst;
    const ConstMul c = pic1dp::const_mul_decide(lx, &worst);
    const pic1dp::GridConst g = pic1dp::make_grid_const(lx, 1024);
    std::printf("lx %a: %s, %d candidates, %d fail; context: %s\n", lx, c.proven ? "proven" : "NOT proven", c.candidates, c.failed,
                g.mul2 ? "two operations" : "five operations");
    if (g.mul2 != c.proven || (c.proven && !same(g.rlx_lo, c.lo)) || !same(g.rlx, 1.0 / lx)) {
      std::printf("  the context's constants do not follow the decision\n");
      ++bad;
    }
    if (!c.proven) continue;
    ++proven;
    long long b0 = bad;
    for (long long i = 0; i < nrandom; ++i) {  // (a)
      const double x = lx * (static_cast<double>(rng() >> 11) * 0x1p-53);
      if (!agree(x, lx, c)) ++bad;
    }
    for (int nx : {2, 192, 1024, 8192})        // (b)
      for (int k = 0; k <= nx; ++k) {
        const double b = static_cast<double>(k) * lx / static_cast<double>(nx);
        double lo = b, hi = b;
        if (!agree(b, lx, c)) ++bad;
        for (int u = 0; u < 2; ++u) {
          lo = std::nextafter(lo, -INFINITY);
          hi = std::nextafter(hi, INFINITY);
          if (!agree(lo, lx, c)) ++bad;
          if (!agree(hi, lx, c)) ++bad;
        }
      }
    for (double x : worst)                     // (c): at the scale of the proof, at others, and with either sign
      for (int e : {0, -52, -48, -60, -300, 7, 300})
        for (double sgn : {1.0, -1.0})
          if (!agree(sgn * std::ldexp(x, e), lx, c)) ++bad;
    std::printf("  %lld operands differ\n", bad - b0);
  }
  {  // the constant the procedure rejects: an operand that really differs, and a context that takes the five operations
    std::vector<double> worst;
    const ConstMul c = pic1dp::const_mul_decide(kNotProven, &worst);
    int differ = 0;
    for (double x : worst)
      if (!same(pic1dp::const_mul_quotient(x, c.hi, c.lo), x / kNotProven)) ++differ;
    const pic1dp::GridConst g = pic1dp::make_grid_const(kNotProven, 1024);
    std::printf("lx %a: %s, %d candidates, %d fail, %d of the worst cases differ; context: %s\n", kNotProven,
                c.proven ? "proven" : "NOT proven", c.candidates, c.failed, differ, g.mul2 ? "two operations" : "five operations");
    if (c.proven || differ == 0 || differ != c.failed || g.mul2 != 0) ++bad;
    // ... whose five operations ARE the division on those very operands (Markstein)
    for (double x : worst) {
      const double y = g.rlx, q0 = x * y, q1 = std::fma(std::fma(-g.lx, q0, x), y, q0), q = std::fma(std::fma(-g.lx, q1, x), y, q1);
      if (!same(q, x / kNotProven)) ++bad;
    }
  }
  const double insane[] = {0.0, -1.0, std::nan(""), HUGE_VAL, 0x1p-300, 0x1p+300, 0x1p-1060};
  for (double lx : insane)  // nothing is proven outside the sane range
    if (pic1dp::const_mul_decide(lx).proven || pic1dp::make_grid_const(lx, 8).mul2) ++bad;
  std::printf("%d constants proven, %lld operands compared, %lld differ\n", proven, g_compared, bad);
  return bad == 0 ? 0 : 1;
}
