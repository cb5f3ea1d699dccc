// zoom_fx_check.cpp -- a stand-alone host program (tests/test_zoom_host.py builds it with -fsanitize=address,undefined and
// runs it): the host arithmetic of the exact phase-space histogram (pic1dp_amd/csrc/zoom_fx.cpp over fx_limbs.hpp) against
// __int128 arithmetic -- the rule over host arrays against a marker-by-marker restatement that sums in __int128, on random
// windows with their edge points and into buffers of exactly the lengths the entry points promise; the normalisation; the
// conversion against the compiler's own __int128 -> double conversion; the refusals.  Nothing else of the library is linked.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../pic1dp_amd/csrc/zoom_fx.cpp"

using namespace pic1dp_host;

namespace {

int checks = 0, failed = 0;
void expect(bool ok, const char *what, double a = 0.0, long long b = 0) {
  ++checks;
  if (!ok) {
    ++failed;
    if (failed < 20) std::printf("FAILED: %s (%a, %lld)\n", what, a, b);
  }
}

typedef __int128 i128;
const i128 TWO32 = static_cast<i128>(1) << 32;
const double kInf = std::numeric_limits<double>::infinity(), kNan = std::numeric_limits<double>::quiet_NaN();

i128 value_of(int64_t hi, int64_t lo) {   // hi wrapped as a 64-bit sum, then exact (lo read as unsigned)
  const uint64_t u = static_cast<uint64_t>(lo);
  const int64_t h = static_cast<int64_t>(static_cast<uint64_t>(hi) + (u >> 32));
  return static_cast<i128>(h) * TWO32 + static_cast<i128>(u & 0xffffffffull);
}
uint64_t state = 0x243f6a8885a308d3ull;
uint64_t splitmix64() {
  uint64_t z = (state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
double uniform() { return static_cast<double>(splitmix64() >> 11) * 0x1p-53; }

// the rule once more, written out without the library's helpers; -1: outside
int cell_of(const pic1dp_zoom &z, double lx, double x, double v) {
  double px = std::fmod(x, lx);
  if (px < 0.0) px = px + lx;
  const bool in_x = z.x_lo <= z.x_hi ? (z.x_lo <= px && px < z.x_hi) : (px >= z.x_lo || px < z.x_hi);
  const bool in_v = z.v_lo <= v && v < z.v_hi;
  if (!in_x || !in_v) return -1;
  const double Lw = z.x_lo <= z.x_hi ? z.x_hi - z.x_lo : (z.x_hi + lx) - z.x_lo;
  const double sx = static_cast<double>(z.nxb) / Lw, sv = static_cast<double>(z.nvb) / (z.v_hi - z.v_lo);
  double d = px - z.x_lo;
  if (d < 0.0) d = d + lx;
  int ix = static_cast<int>(d * sx), jv = static_cast<int>((v - z.v_lo) * sv);
  expect(ix >= 0 && ix <= z.nxb && jv >= 0 && jv <= z.nvb, "the raw index overshoots by one cell at most", x, ix);
  if (ix > z.nxb - 1) ix = z.nxb - 1;
  if (jv > z.nvb - 1) jv = z.nvb - 1;
  return jv * z.nxb + ix;
}

void check_window(const pic1dp_zoom &z, double lx, int which, int e_p, int e_w, int nrandom) {
  expect(zoom_refusal(z, lx) == nullptr, "an accepted window");
  std::vector<double> x, v, p, w;
  const double xe[] = {z.x_lo, z.x_hi, std::nextafter(z.x_lo, kInf), std::nextafter(z.x_lo, -kInf), std::nextafter(z.x_hi, 0.0),
                       std::nextafter(z.x_hi, kInf), 0.0, -0.0, lx, -1e-300, -lx, 2.0 * lx, kNan, kInf, std::nextafter(lx, 0.0)};
  const double ve[] = {z.v_lo, z.v_hi, std::nextafter(z.v_lo, -kInf), std::nextafter(z.v_lo, kInf), std::nextafter(z.v_hi, -kInf),
                       0.0, -0.0, kNan, kInf, -kInf, 0.5 * (z.v_lo + z.v_hi)};
  const double qp = std::ldexp(1.0, e_p), qw = std::ldexp(1.0, e_w);
  for (double a : xe)
    for (double b : ve) x.push_back(a), v.push_back(b), p.push_back(qp * 2.5), w.push_back(-qw * 3.5);
  for (int i = 0; i < nrandom; ++i) {
    x.push_back((3.0 * uniform() - 1.0) * lx);
    v.push_back(z.v_lo + (1.5 * uniform() - 0.25) * (z.v_hi - z.v_lo));
    p.push_back(qp * 0x1p40 * (uniform() - 0.25));
    w.push_back(qw * 0x1p43 * (2.0 * uniform() - 1.0));
  }
  // terms that are not summed, inside the window
  const double mid_x = std::fmod(z.x_lo + 1e-3 * (z.x_lo <= z.x_hi ? z.x_hi - z.x_lo : (z.x_hi + lx) - z.x_lo), lx), mid_v = 0.5 * (z.v_lo + z.v_hi);
  const double bad[] = {qp * 0x1p44, -qp * 0x1p44, kNan, kInf, qp * (0x1p44 - 1.0)};
  for (double b : bad) x.push_back(mid_x), v.push_back(mid_v), p.push_back(b), w.push_back(b == qp * (0x1p44 - 1.0) ? qw : kNan);
  const int nplanes = zoom_planes(which);
  const size_t cells = static_cast<size_t>(z.nxb) * z.nvb;
  std::vector<int64_t> limbs(2 * cells * nplanes, -1);   // exactly zoom_limbs_len words: a write past them is the sanitizer's
  int64_t rej[3] = {-1, -1, -1};
  zoom_host_sums(zoom_geom(z, lx), which, e_p, e_w, x.data(), v.data(), (which & 2) ? p.data() : nullptr, (which & 4) ? w.data() : nullptr,
                 static_cast<int64_t>(x.size()), limbs.data(), rej);
  std::vector<i128> want(cells * 3, 0);
  int64_t want_rej[3] = {0, 0, 0};
  const bool empty = z.x_lo == z.x_hi;
  for (size_t i = 0; i < x.size() && !empty; ++i) {
    const int c = cell_of(z, lx, x[i], v[i]);
    if (c < 0) continue;
    want[c] += 1;
    const double t[3] = {0.0, p[i], w[i]}, iq[3] = {1.0, std::ldexp(1.0, -e_p), std::ldexp(1.0, -e_w)};
    for (int k = 1; k < 3; ++k) {
      if (!(which & (1 << k))) continue;
      const double r = std::rint(t[k] * iq[k]);
      if (!(std::fabs(r) < 0x1p44)) want_rej[k]++;
      else want[k * cells + c] += static_cast<i128>(static_cast<long long>(r));
    }
  }
  int j = 0;
  for (int k = 0; k < 3; ++k) {
    if (!(which & (1 << k))) continue;
    const int64_t *hi = limbs.data() + static_cast<size_t>(2 * j) * cells, *lo = hi + cells;
    for (size_t c = 0; c < cells; ++c) {
      expect(value_of(hi[c], lo[c]) == want[k * cells + c], "host sums against __int128", static_cast<double>(c), k);
      expect(lo[c] >= 0 && lo[c] < (int64_t{1} << 32), "host limbs are normalised", static_cast<double>(c), k);
    }
    expect(rej[k] == want_rej[k], "terms not summed", 0.0, rej[k]);
    ++j;
  }
  if (!(which & 2)) expect(rej[1] == 0, "no plane, no count");
  expect(rej[0] == 0, "markr rejects nothing");
}

void check_limbs() {
  // unnormalised rows (as after an element-wise sum over ranks, lo beyond 2^32, hi negative): normalise keeps the value,
  // convert equals the compiler's conversion of the exact integer
  const size_t cells = 37;
  const int which = 7;
  std::vector<int64_t> limbs(2 * cells * 3);
  for (auto &t : limbs) t = static_cast<int64_t>(splitmix64() >> (1 + splitmix64() % 40)) * ((splitmix64() & 1) ? 1 : -1);
  for (int j = 0; j < 3; ++j)
    for (size_t c = 0; c < cells; ++c) {
      int64_t &hi = limbs[static_cast<size_t>(2 * j) * cells + c];
      hi = hi >> 20;                                            // |value| below 2^76: inside the double's range with any e here
      if (c % 5 == 0) limbs[static_cast<size_t>(2 * j + 1) * cells + c] = static_cast<int64_t>(splitmix64());   // lo: any 64-bit pattern
    }
  const int32_t e[3] = {0, -43, 17};
  std::vector<double> out(3 * cells, -1.0);
  zoom_fx_convert(e, which, limbs.data(), cells, out.data());
  std::vector<int64_t> norm = limbs;
  zoom_fx_normalise(norm.data(), 3, cells);
  std::vector<double> out2(3 * cells, -1.0);
  zoom_fx_convert(e, which, norm.data(), cells, out2.data());
  for (int j = 0; j < 3; ++j)
    for (size_t c = 0; c < cells; ++c) {
      const size_t h = static_cast<size_t>(2 * j) * cells + c, l = h + cells;
      const i128 val = value_of(limbs[h], limbs[l]);
      expect(value_of(norm[h], norm[l]) == val && norm[l] >= 0 && norm[l] < (int64_t{1} << 32), "normalise keeps the value", 0.0, j);
      const double want = std::ldexp(static_cast<double>(val), e[j]);
      expect(std::memcmp(&want, &out[j * cells + c], 8) == 0, "convert against the compiler's __int128 -> double", want, j);
      expect(std::memcmp(&out[j * cells + c], &out2[j * cells + c], 8) == 0, "convert of normalised limbs is the same", want, j);
    }
  // a subset of the planes: the rows follow the mask's order
  std::vector<double> one(cells, -1.0);
  zoom_fx_convert(e, 4, limbs.data(), cells, one.data());
  expect(one[0] == std::ldexp(static_cast<double>(value_of(limbs[0], limbs[cells])), e[2]), "which = 4 converts with pertb's quantum");
}

void check_refusals(double lx) {
  const pic1dp_zoom ok{1.0, 2.0, -1.0, 1.0, 4, 4};
  expect(zoom_refusal(ok, lx) == nullptr, "a plain window");
  auto refused = [&](pic1dp_zoom z, const char *what) { expect(zoom_refusal(z, lx) != nullptr, what); };
  pic1dp_zoom z = ok;
  z.x_lo = kNan, refused(z, "NaN x_lo");
  z = ok, z.x_hi = kInf, refused(z, "infinite x_hi");
  z = ok, z.v_lo = -kInf, refused(z, "infinite v_lo");
  z = ok, z.v_hi = kNan, refused(z, "NaN v_hi");
  z = ok, z.x_lo = -1e-300, refused(z, "x_lo below 0");
  z = ok, z.x_hi = std::nextafter(lx, kInf), refused(z, "x_hi above lx");
  z = ok, z.v_hi = z.v_lo, refused(z, "v_lo == v_hi");
  z = ok, z.v_hi = -2.0, refused(z, "v_lo > v_hi");
  z = ok, z.nxb = 0, refused(z, "nxb 0");
  z = ok, z.nvb = 4097, refused(z, "nvb 4097");
  z = ok, z.nxb = 2048, z.nvb = 513, refused(z, "more than 2^20 cells");
  z = ok, z.v_lo = -1.7e308, z.v_hi = 1.7e308, refused(z, "v extent overflows");
  z = ok, z.x_lo = 0.0, z.x_hi = 5e-324, z.nxb = 4096, refused(z, "cells per unit length overflow");
  z = ok, z.x_lo = 0.0, z.x_hi = lx, expect(zoom_refusal(z, lx) == nullptr, "the whole box");
  z = ok, z.x_lo = lx, z.x_hi = 0.0, refused(z, "the straddling window from lx to 0: its extent is zero, but px == lx would be inside");
  z = ok, z.x_lo = lx, z.x_hi = 1.0, expect(zoom_refusal(z, lx) == nullptr, "the straddling window from lx to 1");
  z = ok, z.x_hi = z.x_lo, expect(zoom_refusal(z, lx) == nullptr, "the empty window");
  z = ok, z.nxb = 1024, z.nvb = 1024, expect(zoom_refusal(z, lx) == nullptr, "2^20 cells");
}

}  // namespace

int main() {
  const double lx = 0x1.1740afa84ad8ap+4;
  check_refusals(lx);
  check_limbs();
  // the two windows at which the clamp is reached
  {
    const pic1dp_zoom zx{0x1.db7810db9b148p+1, 0x1.287245922309ep+1, -1.0, 1.0, 1, 3};
    const ZoomGeom g = zoom_geom(zx, lx);
    double d = std::nextafter(zx.x_hi, 0.0) - zx.x_lo;
    d = d + lx;
    expect(static_cast<int>(d * g.sx) == 1, "the x clamp is reached", d * g.sx);
    int c = -1;
    expect(zoom_cell(g, std::nextafter(zx.x_hi, 0.0), 0.0, &c) && c == 1 * 1 + 0, "... and clamped", 0.0, c);
    check_window(zx, lx, 7, -43, -43, 2000);
    const pic1dp_zoom zv{1.0, 3.0, -0x1.b1ac38e155210p-1, 0x1.68d948684dcdap+2, 3, 2};
    const ZoomGeom gv = zoom_geom(zv, lx);
    const double vv = std::nextafter(zv.v_hi, -kInf);
    expect(static_cast<int>((vv - zv.v_lo) * gv.sv) == 2, "the v clamp is reached", (vv - zv.v_lo) * gv.sv);
    expect(zoom_cell(gv, 1.0, vv, &c) && c == 1 * 3 + 0, "... and clamped", 0.0, c);
    check_window(zv, lx, 7, -43, -43, 2000);
  }
  // random windows of every kind, every mask
  for (int t = 0; t < 400; ++t) {
    pic1dp_zoom z{};
    z.x_lo = uniform() * lx, z.x_hi = uniform() * lx;
    if (t % 7 == 0) z.x_lo = 0.0, z.x_hi = lx;
    if (t % 11 == 0) z.x_hi = z.x_lo;
    if (t % 13 == 0) z.x_lo = lx, z.x_hi = 0.25 * lx;
    z.v_lo = 16.0 * uniform() - 8.0;
    z.v_hi = z.v_lo + 8.0 * uniform() + 1e-6;
    z.nxb = 1 + static_cast<int>(splitmix64() % 40), z.nvb = 1 + static_cast<int>(splitmix64() % 40);
    if (t % 17 == 0) z.nxb = 1;
    if (t % 19 == 0) z.nvb = 1;
    check_window(z, lx, 1 + t % 7, -43 + t % 3, -50 + t % 5, 300);
  }
  std::printf("%d checks, %d failed\n", checks, failed);
  return failed ? 1 : 0;
}
