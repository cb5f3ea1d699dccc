// power_fx_check.cpp -- a stand-alone host program (tests/test_power_exact_host.py builds it with
// -fsanitize=address,undefined and runs it): the host arithmetic of the exact wave-particle power (pic1dp_amd/csrc/power_fx.cpp
// over fx_limbs.hpp) against __int128 arithmetic and the compiler's own __int128 -> double conversion, and the device's
// ceil(log2) from a double's bits (kernels.hpp fx_ceil_log2_bits, power_fx_exponent) against the host's rule (fx_limbs.hpp
// ceil_log2, power_fx_quantum) -- the two must agree at every double.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../pic1dp_amd/csrc/power_fx.cpp"

using namespace pic1dp_host;

namespace {

int checks = 0, failed = 0;
void expect(bool ok, const char *what, double a = 0.0, long long b = 0) {
  ++checks;
  if (!ok) {
    ++failed;
    std::printf("FAILED: %s (%a, %lld)\n", what, a, b);
  }
}

typedef __int128 i128;
const i128 TWO32 = static_cast<i128>(1) << 32;

i128 value_of(int64_t hi, int64_t lo) {   // hi wrapped as a 64-bit sum, then exact (lo read as unsigned)
  const uint64_t u = static_cast<uint64_t>(lo);
  const int64_t h = static_cast<int64_t>(static_cast<uint64_t>(hi) + (u >> 32));
  return static_cast<i128>(h) * TWO32 + static_cast<i128>(u & 0xffffffffull);
}
void limbs_of(i128 t, int64_t *hi, int64_t *lo) {
  const i128 l = ((t % TWO32) + TWO32) % TWO32;
  *lo = static_cast<int64_t>(l);
  *hi = static_cast<int64_t>((t - l) / TWO32);
}
uint64_t state = 0x13198a2e03707344ull;
uint64_t splitmix64() {
  uint64_t z = (state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
uint64_t bits_of(double d) {
  uint64_t u;
  std::memcpy(&u, &d, sizeof u);
  return u;
}
double double_of(uint64_t u) {
  double d;
  std::memcpy(&d, &u, sizeof d);
  return d;
}

void check_log2(double b) {
  expect(pic1dp::fx_ceil_log2_bits(bits_of(b)) == ceil_log2(b), "fx_ceil_log2_bits against ceil_log2", b);
  for (int e_base : {-60, 0, -1100, 37}) {
    int32_t e = 0;
    expect(power_fx_quantum(e_base, b, &e) && e == pic1dp::power_fx_exponent(e_base, bits_of(b)), "power_fx_exponent against power_fx_quantum", b,
           e_base);
  }
}

// nsets sets of nvo x nxo bins from `totals` (cycled), written as limbs by `style` (0 normalised, 1 lo beyond 2^32, 2 lo negative
// as int64), converted and held against the __int128 values
void check_convert(const std::vector<i128> &totals, int nsets, int nxo, int nvo, int style, int e) {
  const size_t nxv = static_cast<size_t>(nxo) * nvo, setw = 2 * nxv + 2;
  std::vector<int64_t> limbs(nsets * setw);
  std::vector<i128> val(nsets * (nxv + 1));
  size_t k = 0;
  auto put = [&](i128 t, int64_t *hi, int64_t *lo) {
    limbs_of(t, hi, lo);
    if (style == 1) *hi -= 5, *lo += 5 * (int64_t(1) << 32);
    if (style == 2) *hi += 3 - (int64_t(1) << 32), *lo -= 3 * (int64_t(1) << 32);
    expect(value_of(*hi, *lo) == t, "the limbs hold the total");
  };
  for (int j = 0; j < nsets; ++j) {
    int64_t *s = limbs.data() + j * setw;
    for (size_t b = 0; b <= nxv; ++b) {
      const i128 t = totals[k++ % totals.size()];
      val[j * (nxv + 1) + b] = t;
      if (b < nxv) put(t, s + b, s + nxv + b);
      else put(t, s + 2 * nxv, s + 2 * nxv + 1);
    }
  }
  const double q = std::ldexp(1.0, e);
  std::vector<double> out(nsets * (nxv + nvo + 1), -1.0);
  power_fx_convert(e, limbs.data(), nsets, nxo, nvo, out.data());
  for (int j = 0; j < nsets; ++j) {
    const double *o = out.data() + j * (nxv + nvo + 1);
    const i128 *v = val.data() + j * (nxv + 1);
    for (size_t b = 0; b < nxv; ++b) expect(o[b] == static_cast<double>(v[b]) * q, "a bin converted once");
    for (int iv = 0; iv < nvo; ++iv) {
      i128 row = 0;
      for (int ix = 0; ix < nxo; ++ix) row += v[static_cast<size_t>(iv) * nxo + ix];
      expect(o[nxv + iv] == static_cast<double>(row) * q, "the v-profile is the integer row sum, converted once");
    }
    expect(o[nxv + nvo] == static_cast<double>(v[nxv]) * q, "rest converted once");
  }
  // normalising keeps every value and leaves lo in [0, 2^32)
  std::vector<int64_t> norm = limbs;
  power_fx_normalise(norm.data(), nsets, nxo, nvo);
  for (int j = 0; j < nsets; ++j) {
    const int64_t *a = limbs.data() + j * setw, *b = norm.data() + j * setw;
    for (size_t i = 0; i <= nxv; ++i) {
      const size_t h = i < nxv ? i : 2 * nxv, l = i < nxv ? nxv + i : 2 * nxv + 1;
      expect(b[l] >= 0 && b[l] < (1ll << 32), "normalised lo lies in [0, 2^32)");
      expect(static_cast<i128>(b[h]) * TWO32 + b[l] == value_of(a[h], a[l]), "normalising keeps the value");
    }
  }
  std::vector<double> out2(out.size(), -2.0);
  power_fx_convert(e, norm.data(), nsets, nxo, nvo, out2.data());
  expect(std::memcmp(out.data(), out2.data(), sizeof(double) * out.size()) == 0, "the conversion does not depend on normalising first");
}

}  // namespace

int main() {
  // ---- ceil(log2) from the bits against frexp, and e with it ----
  for (int k = -1074; k <= 1023; ++k) {
    const double p = std::ldexp(1.0, k);
    check_log2(p);
    check_log2(std::nextafter(p, std::numeric_limits<double>::infinity()));
    if (k > -1074) check_log2(std::nextafter(p, 0.0));
  }
  check_log2(std::numeric_limits<double>::max());
  check_log2(std::numeric_limits<double>::min());
  check_log2(std::numeric_limits<double>::denorm_min());
  check_log2(1e-300);
  check_log2(3.0);
  for (int i = 0; i < 200000; ++i) {
    const uint64_t u = splitmix64() & 0x7fffffffffffffffull;
    if (u >= pic1dp::POWER_FX_NONFINITE || u == 0) continue;
    check_log2(double_of(u));
  }
  for (int i = 0; i < 20000; ++i) check_log2(double_of((splitmix64() & 0x000fffffffffffffull) | 1ull));   // subnormals
  expect(pic1dp::fx_ceil_log2_bits(bits_of(2.0)) == 1 && pic1dp::fx_ceil_log2_bits(bits_of(std::nextafter(2.0, 3.0))) == 2 &&
             pic1dp::fx_ceil_log2_bits(bits_of(std::nextafter(2.0, 0.0))) == 1,
         "2 and its neighbours");
  {
    int32_t e = 0;
    expect(power_fx_quantum(-50, 0.0, &e) && e == -50 && pic1dp::power_fx_exponent(-50, 0ull) == -50, "a field of zeros: kE = 0");
    expect(power_fx_quantum(-50, 1e-300, &e) && e == -1000, "the clamp");
    expect(!power_fx_quantum(0, std::numeric_limits<double>::infinity(), &e) && !power_fx_quantum(0, std::nan(""), &e) && !power_fx_quantum(0, -1.0, &e),
           "max |E| infinite, NaN or negative is refused");
    expect(bits_of(std::numeric_limits<double>::infinity()) >= pic1dp::POWER_FX_NONFINITE && bits_of(std::nan("")) >= pic1dp::POWER_FX_NONFINITE &&
               bits_of(std::numeric_limits<double>::max()) < pic1dp::POWER_FX_NONFINITE,
           "the non-finite patterns lie at and above the flag's threshold");
    int32_t b = 0;
    expect(power_fx_base(-63, 8.0, &b) && b == -63 + 52 + 3 - 40, "e_base");
    expect(power_fx_base(-63, 8.000001, &b) && b == -63 + 52 + 4 - 40, "e_base just above a power of two");
    expect(!power_fx_base(0, 0.0, &b) && !power_fx_base(0, std::nan(""), &b) && !power_fx_base(0, std::numeric_limits<double>::infinity(), &b), "v_max refused");
  }

  // ---- the conversion ----
  const i128 p53 = static_cast<i128>(1) << 53, p54 = static_cast<i128>(1) << 54;
  std::vector<i128> totals = {0, 1, -1, p53 + 1, -(p53 + 1), p53 + 3, -(p53 + 3), TWO32, -TWO32, TWO32 - 1, 1 - TWO32, p54 + 2, p54 + 6,
                              (static_cast<i128>(1) << 60), -(static_cast<i128>(1) << 60), ((static_cast<i128>(1) << 44) - 1) << 19, p53 - 1, p53};
  for (int i = 0; i < 300; ++i) {
    const int64_t a = static_cast<int64_t>(splitmix64());
    totals.push_back(static_cast<i128>(a >> (splitmix64() & 31)) * ((i & 1) ? 1 : 257));
  }
  expect(static_cast<double>(p53 + 1) == 9007199254740992.0 && static_cast<double>(p53 + 3) == 9007199254740996.0, "the compiler's conversion sends ties to even");
  for (int style = 0; style < 3; ++style)
    for (int e : {0, -37, 12}) {
      check_convert(totals, 1, 1, 2, style, e);
      check_convert(totals, 2, 3, 5, style, e);
      check_convert(totals, 2, 64, 7, style, e);
    }
  // a row whose converted bins do not add up to its converted sum: 2^53 + 1 three times (each converts to 2^53; the sum
  // 3 2^53 + 3 converts to 3 2^53 + 4)
  {
    std::vector<i128> t3 = {p53 + 1};
    check_convert(t3, 1, 3, 2, 0, 0);
    expect(3.0 * static_cast<double>(p53 + 1) != static_cast<double>(3 * (p53 + 1)), "the sum of converted bins differs from the converted sum");
  }
  std::printf("%d checks, %d failed\n", checks, failed);
  return failed ? 1 : 0;
}
