// select_check.cpp -- a stand-alone host program (tests/test_select_host.py builds it with -fsanitize=address,undefined
// together with select_host.cpp, and runs it): the host entry points of the marker selection (include/pic1dp_hip.h
// pic1dp_hip_host_select, pic1dp_hip_select_thin) on crafted markers -- every edge position against every edge velocity,
// the four kinds of window, truncation into buffers of exactly min(count, max) elements, the refusals.  It brings the
// library's error convention itself (pic1dp_host::fail), so nothing else of the library is linked.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../include/pic1dp_hip.h"
#include "../pic1dp_amd/csrc/select_rule.hpp"

namespace pic1dp_host {
std::string last_error;
int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  last_error = buf;
  return code;
}
}  // namespace pic1dp_host

namespace {

int checks = 0, failed = 0;
void expect(bool ok, const char *what) {
  ++checks;
  if (!ok) {
    ++failed;
    std::printf("FAILED: %s\n", what);
  }
}

const double kInf = std::numeric_limits<double>::infinity(), kNan = std::numeric_limits<double>::quiet_NaN();

// the rule once more, written out without the library's helpers
bool keeps(const pic1dp_select &s, double lx, double x, double v, int64_t i) {
  double px = std::fmod(x, lx);
  if (px < 0.0) px = px + lx;
  const bool in_x = s.x_lo <= s.x_hi ? (s.x_lo <= px && px < s.x_hi) : (px >= s.x_lo || px < s.x_hi);
  const bool in_v = s.v_lo <= v && v < s.v_hi;
  uint64_t z = s.key + (static_cast<uint64_t>(s.origin) + static_cast<uint64_t>(i) + 1ull) * 0x9E3779B97F4A7C15ull;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return in_x && in_v && (s.thin == 0 || z < s.thin);
}

}  // namespace

int main() {
  // select_thin
  uint64_t t = 99;
  expect(pic1dp_hip_select_thin(1.0, &t) == 0 && t == 0, "fraction 1 keeps all");
  expect(pic1dp_hip_select_thin(2.0, &t) == 0 && t == 0, "fraction 2 keeps all");
  expect(pic1dp_hip_select_thin(0.5, &t) == 0 && t == 1ull << 63, "fraction 1/2");
  expect(pic1dp_hip_select_thin(0x1p-64, &t) == 0 && t == 1, "fraction 2^-64");
  expect(pic1dp_hip_select_thin(0x1p-80, &t) == 0 && t == 1, "a fraction below 2^-64 still keeps h = 0");
  expect(pic1dp_hip_select_thin(1.0 - 0x1p-53, &t) == 0 && t == 0xFFFFFFFFFFFFF800ull, "fraction 1 - 2^-53");
  t = 99;
  expect(pic1dp_hip_select_thin(0.0, &t) == PIC1DP_ERR_ARG && pic1dp_hip_select_thin(-1.0, &t) == PIC1DP_ERR_ARG &&
             pic1dp_hip_select_thin(kNan, &t) == PIC1DP_ERR_ARG && t == 99,
         "fractions 0, -1 and NaN are refused and nothing is written");
  expect(pic1dp_host::last_error.find("fraction") != std::string::npos, "... with a message");
  expect(pic1dp_hip_select_thin(0.5, nullptr) == PIC1DP_ERR_ARG, "null threshold");

  // crafted markers
  pic1dp_input in;
  std::memset(&in, 0, sizeof in);
  in.lx = 2.0 * 3.1415926535897932384626 / 0.36;
  const double lx = in.lx, v_lo = -1.5, v_hi = 2.25;
  const double xs[] = {0.0, -0.0, lx, std::nextafter(lx, 0.0), lx + 1e-13, -1e-300, 7.3 * lx, -7.3 * lx, kNan};
  const double vs[] = {v_lo, std::nextafter(v_lo, -kInf), v_hi, std::nextafter(v_hi, -kInf), kNan, kInf, -kInf};
  std::vector<double> x, v;
  for (double a : xs)
    for (double b : vs) x.push_back(a), v.push_back(b);
  uint64_t state = 12345;   // a few hundred more from a small generator
  auto unit = [&]() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<double>(state >> 11) * 0x1p-53;
  };
  for (int i = 0; i < 300; ++i) x.push_back((5.0 * unit() - 2.0) * lx), v.push_back(v_lo - 2.0 + (v_hi - v_lo + 4.0) * unit());
  const int64_t np = static_cast<int64_t>(x.size());

  const pic1dp_select windows[] = {
      {0.25 * lx, 0.75 * lx, v_lo, v_hi, 0, 0, 0},                      // plain
      {0.75 * lx, 0.25 * lx, v_lo, v_hi, 0, 0, 0},                      // straddling
      {std::nextafter(lx, 0.0), 1e-300, -kInf, kInf, 0, 0, 0},          // straddling, the two ends of the period alone
      {0.5 * lx, 0.5 * lx, -kInf, kInf, 0, 0, 0},                       // empty
      {-kInf, kInf, -kInf, kInf, 0, 0, 0},                              // everything
      {-kInf, kInf, -kInf, kInf, 1ull << 62, 7, 100000000},             // a hashed quarter of everything
      {0.0, lx, v_lo, kInf, 1ull << 63, 0xFFFFFFFFFFFFFFFFull, -3},     // a key and an origin that wrap around
  };
  int64_t seen[7] = {0};
  int wi = 0;
  for (const pic1dp_select &s : windows) {
    std::vector<int64_t> want;
    for (int64_t i = 0; i < np; ++i)
      if (keeps(s, lx, x[i], v[i], i)) want.push_back(i);
    const int64_t total = static_cast<int64_t>(want.size());
    seen[wi++] = total;
    int64_t count = -1;
    expect(pic1dp_hip_host_select(&in, &s, x.data(), v.data(), np, 0, &count, nullptr) == 0 && count == total, "count with max 0 and no buffer");
    for (int64_t max : {int64_t{0}, int64_t{1}, total - 1, total, total + 1}) {
      if (max < 0) continue;
      const int64_t n = max < total ? max : total;
      std::vector<int64_t> index(static_cast<size_t>(n));   // exactly min(count, max) elements: one write too many is a heap overflow
      count = -1;
      expect(pic1dp_hip_host_select(&in, &s, x.data(), v.data(), np, max, &count, index.data()) == 0, "host_select runs");
      expect(count == total, "count is the total whatever max is");
      bool same = true;
      for (int64_t k = 0; k < n; ++k) same = same && index[static_cast<size_t>(k)] == want[static_cast<size_t>(k)];
      expect(same, "the first min(count, max) indices in ascending order");
    }
    // the library's own statement of the rule agrees marker by marker
    bool agree = true;
    for (int64_t i = 0; i < np; ++i) agree = agree && pic1dp::select_keeps(s, lx, x[i], v[i], i) == keeps(s, lx, x[i], v[i], i);
    expect(agree, "select_keeps");
  }
  expect(seen[3] == 0, "x_lo == x_hi is empty");
  expect(seen[0] > 0 && seen[1] > 0 && seen[2] > 0, "the windows hold markers");
  int64_t finite = 0;
  for (int64_t i = 0; i < np; ++i) finite += !std::isnan(std::fmod(x[i], lx)) && !std::isnan(v[i]) && v[i] != kInf;
  expect(seen[4] == finite && finite < np, "everything is every marker without a NaN and with v < +inf (the bound is strict)");
  expect(seen[5] > 0 && seen[5] < seen[4], "a hashed quarter");

  // refusals: nothing is written
  const pic1dp_select all = {-kInf, kInf, -kInf, kInf, 0, 0, 0};
  int64_t count = -7, idx[4] = {-7, -7, -7, -7};
  for (int k = 0; k < 4; ++k) {
    pic1dp_select bad = all;
    (k == 0 ? bad.x_lo : k == 1 ? bad.x_hi : k == 2 ? bad.v_lo : bad.v_hi) = kNan;
    expect(pic1dp_hip_host_select(&in, &bad, x.data(), v.data(), np, 4, &count, idx) == PIC1DP_ERR_ARG, "a NaN bound");
    expect(pic1dp_host::last_error.find("NaN") != std::string::npos, "... named");
  }
  expect(pic1dp_hip_host_select(&in, &all, x.data(), v.data(), np, -1, &count, idx) == PIC1DP_ERR_ARG, "negative max");
  expect(pic1dp_hip_host_select(&in, &all, x.data(), v.data(), -1, 4, &count, idx) == PIC1DP_ERR_ARG, "negative np");
  expect(pic1dp_hip_host_select(nullptr, &all, x.data(), v.data(), np, 4, &count, idx) == PIC1DP_ERR_ARG, "null input");
  expect(pic1dp_hip_host_select(&in, nullptr, x.data(), v.data(), np, 4, &count, idx) == PIC1DP_ERR_ARG, "null selection");
  expect(pic1dp_hip_host_select(&in, &all, x.data(), v.data(), np, 4, nullptr, idx) == PIC1DP_ERR_ARG, "null count");
  expect(pic1dp_hip_host_select(&in, &all, nullptr, v.data(), np, 4, &count, idx) == PIC1DP_ERR_ARG, "null x");
  expect(count == -7 && idx[0] == -7 && idx[3] == -7, "refusals write nothing");
  expect(pic1dp_hip_host_select(&in, &all, nullptr, nullptr, 0, 4, &count, idx) == 0 && count == 0, "no markers: no arrays needed");

  std::printf("%d checks, %d failed\n", checks, failed);
  return failed ? 1 : 0;
}
