// const_mul.cpp -- decides, for one constant lx, whether  q = fma(yh, x, RN(yl x))  with yh = RN(1/lx),
// yl = RN(1/lx - yh) is RN(x / lx) for EVERY double x (const_mul.hpp).  create() asks once per context; locate
// (device_math.hpp) then divides in two operations instead of Markstein's five.
//
// The argument (Brisebarre and Muller's, specialised to C = 1/lx, a rational whose continued fraction is the
// Euclidean algorithm on integers below 2^108 -- it fits unsigned __int128):
//
//   Write lx = L 2^a and x = X 2^b with integers L, X in [2^52, 2^53).  Every operation of the two-operation form
//   scales exactly with a and b (nothing underflows or overflows for 2^-200 <= lx <= 2^200, 2^-500 <= |x| <= 2^500),
//   so the outcome depends on (L, X) alone; take x = X.  In units where G = 2^52 / L lies in (1/2, 1) (L = 2^52, a
//   power of two, is exact in one operation) and X' = X 2^-52 lies in [1, 2):
//     gh = RN(G), |G - gh| <= 2^-54;  gl = RN(G - gh), |gl| <= 2^-54, |G - gh - gl| <= 2^-108;
//     u = RN(gl X'): |gl X'| < 2^-53, so |u - gl X'| <= 2^-107;
//     V = gh X' + u is what the fma rounds, and |V - G X'| < 2^-108 * 2 + 2^-107 = 2^-106.
//   RN is monotone and constant between neighbouring rounding boundaries (midpoints of adjacent doubles), so
//   RN(V) != RN(G X') needs a midpoint m with |G X' - m| < 2^-106.  G X' = X / L lies in (1/2, 2); every midpoint of
//   the binades [1/4, 4) is a multiple of 2^-55.  Hence an integer k with
//         |2^55 X - k L| < 2^-106 * 2^55 * L = L 2^-51 < 4.
//   r = 2^55 X - k L is an integer:
//     r = 0: X / L = k 2^-55 exactly.  In lowest terms k' / 2^j with k' odd, X 2^j = k' L, so 2^j divides L (j <= 52)
//            and k' = (X / L) 2^j < 2^(j + 1) <= 2^53: the quotient IS a double, V lies within 2^-106 of it, far inside
//            its rounding interval: safe.
//     r != 0: X solves the linear congruence 2^55 X = r (mod L) -- the extended Euclidean algorithm (the continued
//            fraction of 2^55 / L) names every solution in [2^52, 2^53): a handful.  These are the operands nearest
//            to a rounding boundary; each is EVALUATED, two operations against the IEEE division, bit for bit.
//   All |r| <= 6 are enumerated (a superset of |r| <= 3).  If every candidate agrees, every double does.
#include "const_mul.hpp"

#include <cmath>
#include <cstring>

namespace pic1dp {

namespace {

typedef unsigned __int128 u128;
typedef __int128 i128;

uint64_t mulmod(uint64_t a, uint64_t b, uint64_t m) { return static_cast<uint64_t>(static_cast<u128>(a) * b % m); }

// a^-1 mod m for gcd(a, m) = 1, m > 1 (extended Euclid: the convergents of a / m)
uint64_t invmod(uint64_t a, uint64_t m) {
  i128 r0 = m, r1 = a % m, t0 = 0, t1 = 1;
  while (r1 != 0) {
    const i128 q = r0 / r1;
    const i128 r2 = r0 - q * r1, t2 = t0 - q * t1;
    r0 = r1, r1 = r2, t0 = t1, t1 = t2;
  }
  // r0 = gcd = 1
  i128 t = t0 % static_cast<i128>(m);
  if (t < 0) t += m;
  return static_cast<uint64_t>(t);
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

}  // namespace

double const_mul_quotient(double x, double hi, double lo) {
  const double u = lo * x;
  return std::fma(hi, x, u);
}

ConstMul const_mul_decide(double lx, std::vector<double> *worst) {
  ConstMul c;
  if (worst) worst->clear();
  if (!(lx >= 0x1p-200 && lx <= 0x1p+200)) return c;  // (NaN, zero, negative, extreme: not proven)
  int e;
  const double mant = std::frexp(lx, &e);                                   // lx = mant 2^e, mant in [1/2, 1)
  const uint64_t L = static_cast<uint64_t>(std::ldexp(mant, 53));           // exact: an integer in [2^52, 2^53)
  c.hi = 1.0 / lx;                                                          // RN(C): IEEE division
  // C - yh = (1 - yh lx) / lx, and the residual of a correctly rounded quotient is a double: the fma is exact
  const double res = std::fma(-c.hi, lx, 1.0);
  c.lo = res / lx;                                                          // RN(C - yh)
  if (L == (1ull << 52)) {  // a power of two: yh = C exactly, yl = 0, one exact scaling
    c.proven = 1;
    return c;
  }
  const int v = __builtin_ctzll(L);
  const uint64_t g = v < 3 ? (1ull << v) : 8ull;    // gcd(2^55, L), as far as |r| <= 6 can see it
  const uint64_t Lp = L >> v;                       // odd, >= 2^52 / 2^51 > 1
  constexpr int R = 6;
  if (v < 3) {
    // 2^(55 - v) X = r / g (mod L'), L' odd: a unique X mod L'
    const uint64_t A = static_cast<uint64_t>((static_cast<u128>(1) << (55 - v)) % Lp);
    const uint64_t Ainv = invmod(A, Lp);
    for (int r = -R; r <= R; ++r) {
      if (r == 0 || (r % static_cast<int>(g)) != 0) continue;
      const int rg = r / static_cast<int>(g);
      const uint64_t rm = rg >= 0 ? static_cast<uint64_t>(rg) % Lp : Lp - (static_cast<uint64_t>(-rg) % Lp);
      const uint64_t X0 = mulmod(rm % Lp, Ainv, Lp);
      // every X = X0 + t L' in [2^52, 2^53)
      const uint64_t lo_x = 1ull << 52, hi_x = 1ull << 53;
      uint64_t X = X0;
      if (X < lo_x) X += (lo_x - X + Lp - 1) / Lp * Lp;
      for (; X < hi_x; X += Lp) {
        const double x = static_cast<double>(X);   // exact
        ++c.candidates;
        if (worst) worst->push_back(x);
        if (!same_bits(const_mul_quotient(x, c.hi, c.lo), x / lx)) ++c.failed;
      }
    }
  }
  // (v >= 3: 8 divides L and 2^55, so it divides every r = 2^55 X - k L; none of 1 ... 6: no candidate at all)
  c.proven = c.failed == 0 ? 1 : 0;
  return c;
}

}  // namespace pic1dp
