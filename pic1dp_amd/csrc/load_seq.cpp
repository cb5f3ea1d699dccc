// load_seq.cpp -- see load_seq.hpp.  Host code, no HIP call; compiled without FMA contraction so that the constants equal
// loader.cpp's.
#include "load_seq.hpp"

#include <cmath>

#include "loader.hpp"

namespace pic1dp {

namespace {
constexpr double kPi = 3.14159265358979323846264;  // PETSC_PI
}

LoadConst make_load_const(const pic1dp_input &in, int isp) {
  LoadConst k{};
  const double T = in.species_temperature[isp], T2 = in.species_temperature2[isp];
  const double m = in.species_mass[isp], den = in.species_density[isp];
  const double ninit = static_cast<double>(in.species_nparticle_init[isp]);
  k.lx = in.lx;
  k.vmax = in.v_max;
  // (loader.cpp load_block_species, the imarker = 2 branch: the same expressions in the same order)
  k.pref = (in.iptcldist == 3 ? 1.0 : den) * in.lx * 2.0 * in.v_max / ninit;
  k.a1 = 2.0 * T / m;
  k.a2 = 2.0 * T2 / m;
  k.g1 = std::sqrt(2.0 * kPi * T / m);
  k.g2 = std::sqrt(2.0 * kPi * T2 / m);
  k.g8 = std::sqrt(8.0 * kPi * T / m);
  k.gs = std::sqrt(2.0 * kPi);
  k.den = den;
  k.beam = 1.0 - den;
  k.v0 = in.species_v0[isp];
  k.nim = in.init_nmode;
  for (int j = 0; j < PIC1DP_MAX_INIT_MODES; ++j) {
    const bool on = j < in.init_nmode;
    k.kk[j] = on ? 2.0 * kPi / in.lx * static_cast<double>(in.init_mode[j]) : 0.0;
    k.mcos[j] = on ? in.init_mode_cos[j] : 0.0;
    k.msin[j] = on ? in.init_mode_sin[j] : 0.0;
  }
  return k;
}

int64_t load_origin(const pic1dp_input &in, int isp, int blk0, int npe) {
  int64_t g0 = 0;
  for (int b = 0; b < blk0; ++b) g0 += block_np(in, isp, b, npe);
  return g0;
}

const char *load_refusal(const pic1dp_input &in, int kind, int seed_offset) {
  if (kind != LOAD_RANDOM && kind != LOAD_QUIET) return "load kind must be 1 (counter-based random) or 2 (quiet start)";
  if (in.imarker != 2) return "the device load draws uniform markers only: imarker = 1 (Gaussian markers) is not built";
  if (kind == LOAD_QUIET) {
    if (seed_offset != 0) return "a quiet start (kind 2) is one sequence: it takes no seed offset";
    for (int s = 0; s < in.nspecies; ++s)
      if (in.species_nparticle_init[s] < 0 || static_cast<uint64_t>(in.species_nparticle_init[s]) > LOAD_R3_SPAN)
        return "a quiet start (kind 2) serves at most 3^21 markers per species";
  }
  return nullptr;
}

}  // namespace pic1dp
