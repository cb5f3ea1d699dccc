// load_seq_check.cpp -- a stand-alone host program (tests/test_load_device_host.py builds it with
// -fsanitize=address,undefined together with load_seq.cpp, loader.cpp and multirand.cpp, and runs it): the definition of
// the on-device particle load (pic1dp_amd/csrc/load_seq.hpp) -- the known answers of the counter-based stream, the two
// radical inverses at their corners and beyond 2^32, the origin of a rank's markers, the refusals, the constants.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "../pic1dp_amd/csrc/load_seq.hpp"
#include "../pic1dp_amd/csrc/loader.hpp"

using namespace pic1dp;

namespace {

int checks = 0, failed = 0;
void expect(bool ok, const char *what) {
  ++checks;
  if (!ok) {
    ++failed;
    std::printf("FAILED: %s\n", what);
  }
}

pic1dp_input small_input(int64_t nmax, int64_t ninit) {
  pic1dp_input in;
  std::memset(&in, 0, sizeof in);
  in.abi_version = PIC1DP_ABI_VERSION;
  in.nspecies = 2;
  in.imarker = 2;
  in.iptcldist = 3;
  in.nparticle_max = nmax;
  in.lx = 17.0, in.v_max = 10.0;
  in.init_nmode = 2;
  in.init_mode[0] = 1, in.init_mode[1] = 3;
  in.init_mode_cos[0] = 1e-3, in.init_mode_sin[1] = 2e-3;
  for (int s = 0; s < 2; ++s) {
    in.species_nparticle_init[s] = ninit - s;
    in.species_mass[s] = 1.0 + s, in.species_temperature[s] = 1.0, in.species_temperature2[s] = 0.5;
    in.species_density[s] = 0.9, in.species_v0[s] = 5.0;
  }
  return in;
}

}  // namespace

int main() {
  // the published splitmix64 outputs of state 1234567
  const uint64_t known[5] = {6457827717110365317ull, 3203168211198807973ull, 9817491932198370423ull, 4593380528125082431ull,
                             16408922859458223821ull};
  for (uint64_t c = 0; c < 5; ++c) expect(load_draw(1234567ull, c) == known[c], "splitmix64 known answer");
  expect(load_key(0, 0) == load_mix64(LOAD_KEY_BASE), "key of member 0, species 0");
  expect(load_key(3, 1) == load_mix64(LOAD_KEY_BASE + 769ull), "key of member 3, species 1");

  expect(load_bitrev64(1ull) == 1ull << 63 && load_bitrev64(1ull << 63) == 1ull, "bit reversal, ends");
  expect(load_bitrev64(0x00000001FFFFFFFFull) == 0xFFFFFFFF80000000ull, "bit reversal across the 32-bit halves");
  uint64_t p3[22] = {1};
  for (int i = 1; i < 22; ++i) p3[i] = p3[i - 1] * 3ull;
  expect(p3[21] == LOAD_R3_SPAN, "3^21");
  expect(load_r3(0) == 0 && load_r3(1) == p3[20] && load_r3(2) == 2 * p3[20], "R3 of one digit");
  expect(load_r3(LOAD_R3_SPAN - 1) == LOAD_R3_SPAN - 1, "R3 of all twos");
  expect(load_r3(p3[20]) == 1 && load_r3(p3[10]) == p3[10], "R3 of a power of three");
  for (uint64_t g : {uint64_t{0}, uint64_t{5}, (uint64_t{1} << 32) - 3, (uint64_t{1} << 33) + 1, LOAD_R3_SPAN - 8}) {
    expect(load_r3(load_r3(g)) == g, "R3 is an involution");
    expect(load_bitrev64(load_bitrev64(g)) == g, "bit reversal is an involution");
    for (int kind = 1; kind <= 2; ++kind) {
      double uv = -1.0, ux = -1.0;
      load_uniforms(kind, load_key(0, 0), g, &uv, &ux);
      expect(uv >= 0.0 && uv < 1.0 && ux >= 0.0 && ux < 1.0, "uniforms lie in [0, 1)");
    }
  }
  {  // a quiet start's first markers: 0, 1/2, 1/4, 3/4 in v against 0, 1/3, 2/3, 1/9 in x
    double uv[4], ux[4];
    for (uint64_t g = 0; g < 4; ++g) load_uniforms(LOAD_QUIET, 0, g, &uv[g], &ux[g]);
    expect(uv[0] == 0.0 && uv[1] == 0.5 && uv[2] == 0.25 && uv[3] == 0.75, "base-2 radical inverse");
    expect(ux[0] == 0.0 && ux[1] == 1.0 / 3.0 && ux[2] == 2.0 / 3.0 && ux[3] == 1.0 / 9.0, "base-3 radical inverse");
  }

  // origin: the valid markers of the blocks before a rank's first one
  const pic1dp_input in = small_input(1003, 1001);
  for (int npe : {1, 3, 4}) {
    int64_t sum[2] = {0, 0};
    for (int b = 0; b < npe; ++b)
      for (int s = 0; s < 2; ++s) {
        expect(load_origin(in, s, b, npe) == sum[s], "origin is the running sum of block_np");
        sum[s] += block_np(in, s, b, npe);
      }
    expect(sum[0] == 1001 && sum[1] == 1000, "the blocks' valid markers add up to the species' count");
  }

  // refusals
  expect(load_refusal(in, 1, 0) == nullptr && load_refusal(in, 2, 0) == nullptr && load_refusal(in, 1, 7) == nullptr, "accepted");
  expect(load_refusal(in, 0, 0) && load_refusal(in, 3, 0), "kind out of range");
  expect(load_refusal(in, 2, 1) && std::strstr(load_refusal(in, 2, 1), "seed offset"), "quiet start with a seed offset");
  pic1dp_input g = in;
  g.imarker = 1;
  expect(load_refusal(g, 1, 0) && std::strstr(load_refusal(g, 1, 0), "imarker"), "Gaussian markers");
  pic1dp_input big = small_input(static_cast<int64_t>(LOAD_R3_SPAN) + 5, static_cast<int64_t>(LOAD_R3_SPAN) + 1);
  expect(load_refusal(big, 2, 0) && std::strstr(load_refusal(big, 2, 0), "3^21"), "more than 3^21 markers");
  expect(load_refusal(big, 1, 0) == nullptr, "... which kind 1 serves");
  expect(load_origin(big, 0, 1, 2) == block_np(big, 0, 0, 2), "origin beyond 2^32");

  // constants: loader.cpp's expressions
  const LoadConst k = make_load_const(in, 1);
  expect(k.nim == 2 && k.kk[1] == 2.0 * 3.14159265358979323846264 / 17.0 * 3.0 && k.kk[2] == 0.0, "wave numbers");
  expect(k.pref == 1.0 * 17.0 * 2.0 * 10.0 / 1000.0 && k.a1 == 1.0 && k.a2 == 0.5 && k.beam == 1.0 - 0.9, "prefactors");
  expect(k.g2 == std::sqrt(2.0 * 3.14159265358979323846264 * 0.5 / 2.0), "Gaussian norms");

  std::printf("%d checks, %d failed\n", checks, failed);
  return failed ? 1 : 0;
}
