// fx_limbs_check.cpp -- a stand-alone host program (tests/test_moments_exact_host.py builds it with
// -fsanitize=address,undefined and runs it): the host limb arithmetic of the exact sums (pic1dp_amd/csrc/fx_limbs.hpp)
// against __int128 arithmetic and the compiler's own __int128 -> double conversion.  A pair (hi, lo) means the value
// hi 2^32 + lo with lo read as unsigned, and the sum hi + (lo >> 32) wraps modulo 2^64 as the integer sums on the device do.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../pic1dp_amd/csrc/fx_limbs.hpp"

using namespace pic1dp_host;

namespace {

int checks = 0, failed = 0;
void expect(bool ok, const char *what, long long a = 0, unsigned long long b = 0) {
  ++checks;
  if (!ok) {
    ++failed;
    std::printf("FAILED: %s (hi %lld, lo %llu)\n", what, a, b);
  }
}

typedef __int128 i128;
const i128 TWO32 = static_cast<i128>(1) << 32;

// the value of a pair: hi wrapped as a 64-bit sum, then exact
i128 value_of(int64_t hi, int64_t lo) {
  const uint64_t u = static_cast<uint64_t>(lo);
  const int64_t h = static_cast<int64_t>(static_cast<uint64_t>(hi) + (u >> 32));
  return static_cast<i128>(h) * TWO32 + static_cast<i128>(u & 0xffffffffull);
}
// (hi, lo) normalised, of a total that fits 96 bits
void limbs_of(i128 t, int64_t *hi, int64_t *lo) {
  const i128 l = ((t % TWO32) + TWO32) % TWO32;
  *lo = static_cast<int64_t>(l);
  *hi = static_cast<int64_t>((t - l) / TWO32);
}
uint64_t state = 0x243f6a8885a308d3ull;
uint64_t splitmix64() {
  uint64_t z = (state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

void check_pairs(const std::vector<int64_t> &hi, const std::vector<int64_t> &lo) {
  const size_t n = hi.size();
  const double qs[3] = {1.0, std::ldexp(1.0, -20), std::ldexp(1.0, 7)};
  for (double q : qs) {
    std::vector<double> out(n, -1.0);
    fx_row_to_double(hi.data(), lo.data(), n, q, out.data());
    for (size_t i = 0; i < n; ++i) {
      const double want = static_cast<double>(value_of(hi[i], lo[i])) * q;   // one rounding to nearest even, then an exact scaling
      expect(out[i] == want && std::signbit(out[i]) == std::signbit(want), "fx_row_to_double against the __int128 conversion", hi[i],
             static_cast<uint64_t>(lo[i]));
    }
  }
  std::vector<int64_t> h2 = hi, l2 = lo;
  fx_row_normalise(h2.data(), l2.data(), n);
  std::vector<double> a(n), b(n);
  fx_row_to_double(hi.data(), lo.data(), n, 1.0, a.data());
  fx_row_to_double(h2.data(), l2.data(), n, 1.0, b.data());
  for (size_t i = 0; i < n; ++i) {
    expect(l2[i] >= 0 && l2[i] < (1ll << 32), "normalised lo lies in [0, 2^32)", hi[i], static_cast<uint64_t>(lo[i]));
    expect(static_cast<i128>(h2[i]) * TWO32 + l2[i] == value_of(hi[i], lo[i]), "normalising keeps the value", hi[i], static_cast<uint64_t>(lo[i]));
    expect(a[i] == b[i], "the conversion does not depend on normalising first", hi[i], static_cast<uint64_t>(lo[i]));
    const uint64_t u = static_cast<uint64_t>(lo[i]);
    const i128 plain = static_cast<i128>(hi[i]) * TWO32 + static_cast<i128>(u);   // where hi + (lo >> 32) does not wrap, the plain sum
    const i128 hs = static_cast<i128>(hi[i]) + static_cast<i128>(u >> 32);
    if (hs >= std::numeric_limits<int64_t>::min() && hs <= std::numeric_limits<int64_t>::max())
      expect(plain == value_of(hi[i], lo[i]), "value_of is hi 2^32 + lo", hi[i], u);
  }
}

}  // namespace

int main() {
  const int64_t MIN = std::numeric_limits<int64_t>::min(), MAX = std::numeric_limits<int64_t>::max();
  const int64_t ALL = static_cast<int64_t>(~0ull);   // lo = 2^64 - 1
  std::vector<int64_t> hi, lo;
  auto add = [&](int64_t h, int64_t l) { hi.push_back(h), lo.push_back(l); };
  // the edges
  for (int64_t h : {int64_t(0), int64_t(-1), int64_t(5), int64_t(-5), MIN, MAX, MIN + 1, MAX - 1})
    for (int64_t l : {int64_t(0), int64_t(1), (int64_t(1) << 32) - 1, int64_t(1) << 32, ALL, MIN, MAX}) add(h, l);
  add(-1, 1);
  const i128 p53 = static_cast<i128>(1) << 53, p54 = static_cast<i128>(1) << 54;
  for (i128 t : {p53 - 1, p53, p53 + 1, p53 + 2, p53 + 3, p54 + 2, p54 + 6, p54 + 1, p54 + 3, (static_cast<i128>(1) << 60), (static_cast<i128>(1) << 94) + 1,
                 ((static_cast<i128>(1) << 44) - 1) << 18})
    for (int sign : {1, -1}) {
      int64_t h, l;
      limbs_of(sign * t, &h, &l);
      add(h, l);
      add(h - 5, l + 5 * (int64_t(1) << 32));   // the same total, lo beyond 2^32 (as after a sum over ranks)
      add(h + 3 - (int64_t(1) << 32), l - 3 * (int64_t(1) << 32));   // ... and lo negative as int64: its top bits count 2^64 as unsigned
    }
  expect(static_cast<double>(p53 + 1) == 9007199254740992.0 && static_cast<double>(p53 + 3) == 9007199254740996.0 &&
             static_cast<double>(p54 + 2) == 18014398509481984.0 && static_cast<double>(p54 + 6) == 18014398509481992.0,
         "the compiler's conversion sends ties to even");
  // pseudo-random pairs: all 64 bits, small magnitudes, magnitudes around 2^53 and 2^54
  for (int i = 0; i < 4000; ++i) {
    const uint64_t a = splitmix64(), b = splitmix64();
    switch (i & 3) {
      case 0: add(static_cast<int64_t>(a), static_cast<int64_t>(b)); break;
      case 1: add(static_cast<int64_t>(a) >> 40, static_cast<int64_t>(b)); break;
      case 2: add(static_cast<int64_t>(a) >> (32 + (b & 15)), static_cast<int64_t>(b >> 32)); break;
      default: add(static_cast<int64_t>(a) >> (b & 63), static_cast<int64_t>(b >> (a & 63))); break;
    }
  }
  check_pairs(hi, lo);

  // ceil(log2 b)
  expect(ceil_log2(0.5) == -1, "ceil_log2(0.5)");
  expect(ceil_log2(1.0) == 0, "ceil_log2(1)");
  expect(ceil_log2(std::nextafter(1.0, 2.0)) == 1, "ceil_log2(1 + ulp)");
  expect(ceil_log2(3.0) == 2, "ceil_log2(3)");
  expect(ceil_log2(std::numeric_limits<double>::denorm_min()) == -1074, "ceil_log2(2^-1074)");
  expect(ceil_log2(std::ldexp(1.0, 1023)) == 1023, "ceil_log2(2^1023)");

  // the row sums of the exact diagnostics' v histograms (capi_diag.cpp dfx_convert: fx_row_sum, then fx_row_to_double of the
  // pair): a row of nx_opd = 192 bins whose lo limbs are all 2^64 - 1
  {
    const int nxo = 192;
    std::vector<int64_t> rh(nxo), rl(nxo, ALL);
    i128 want = 0;
    for (int ix = 0; ix < nxo; ++ix) {
      rh[ix] = static_cast<int64_t>(splitmix64()) >> 24;   // (|hi| < 2^39: the row's total fits the 96 bits of a pair)
      want += static_cast<i128>(rh[ix]) * TWO32 + static_cast<i128>(~0ull);
    }
    int64_t H, L;
    fx_row_sum(rh.data(), rl.data(), nxo, &H, &L);
    expect(L >= 0 && L < nxo * (1ll << 32), "the row's lo sum stays below nx_opd 2^32");
    expect(static_cast<i128>(H) * TWO32 + L == want, "fx_row_sum against the __int128 sum");
    double got = 0.0;
    fx_row_to_double(&H, &L, 1, std::ldexp(1.0, -40), &got);
    expect(got == static_cast<double>(want) * std::ldexp(1.0, -40), "the row sum converted once");
    // hi limbs that wrap: still defined, and the sum modulo 2^64 of the normalised his
    std::vector<int64_t> wh(nxo, MAX);
    fx_row_sum(wh.data(), rl.data(), nxo, &H, &L);
    expect(static_cast<uint64_t>(H) == static_cast<uint64_t>(nxo) * (static_cast<uint64_t>(MAX) + 0xffffffffull), "fx_row_sum wraps in unsigned");
  }
  std::printf("%d checks, %d failed\n", checks, failed);
  return failed ? 1 : 0;
}
