// mode_tables_check.cpp -- a stand-alone host program (tests/test_context_plan_host.py builds it with
// -fsanitize=address,undefined together with context_plan.cpp and settings.cpp, and runs it): the mode tables of
// mode_tables() against a literal copy of the loops pic1dp_hip_create held before, byte for byte, for nx 7, 192, 1024 and
// the kept modes {1}, {1, 2, 3}; plan_context() and settings_from_env() run under the sanitizers on the way.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../pic1dp_amd/csrc/context_plan.hpp"

using namespace pic1dp;

namespace {

constexpr double kPi = 3.14159265358979323846264;  // PETSC_PI

struct Old {
  std::vector<double> fre, fim, gi, ta, tb;
  PredTab pt{};
};

// create()'s own loops as they were (capi.cpp before context_plan.cpp)
Old old_tables(const pic1dp_input *in, int pred_kind) {
  const int nx = in->nx, nm = in->nmode;
  Old o;
  std::vector<double> fre(static_cast<size_t>(nm) * nx), fim(static_cast<size_t>(nm) * nx), gi(nm);
  for (int m = 0; m < nm; ++m) {
    const double mode = static_cast<double>(in->modes[m]);
    gi[m] = 1.0 / (2.0 * kPi / in->lx * mode);
    double (*volatile cos_fn)(double) = std::cos;
    double (*volatile sin_fn)(double) = std::sin;
    for (int ix = 0; ix < nx; ++ix) {
      const double th = 2.0 * kPi / static_cast<double>(nx) * mode * static_cast<double>(ix);
      fre[static_cast<size_t>(m) * nx + ix] = cos_fn(th);
    }
    for (int ix = 0; ix < nx; ++ix) {
      const double th = 2.0 * kPi / static_cast<double>(nx) * mode * static_cast<double>(ix);
      fim[static_cast<size_t>(m) * nx + ix] = -sin_fn(th);
    }
  }
  if (pred_kind) {
    std::vector<double> ta(fre.size()), tb(fim.size());
    for (size_t i = 0; i < fre.size(); ++i) ta[i] = 2.0 * fre[i], tb[i] = 2.0 * fim[i];
    if (pred_kind == 2) {
      PredTab &pt = o.pt;
      for (int ix = 0; ix < nx; ++ix) {
        pt.sum_fre += fre[ix], pt.sum_fim += fim[ix];
        pt.g11 += fre[ix] * fre[ix], pt.g22 += fim[ix] * fim[ix], pt.g12 += fre[ix] * fim[ix];
      }
    }
    o.ta = ta, o.tb = tb;
  }
  o.fre = fre, o.fim = fim, o.gi = gi;
  return o;
}

bool same(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}

}  // namespace

int main() {
  int bad = 0, cases = 0;
  const int grids[3] = {7, 192, 1024};
  for (int nx : grids)
    for (int nm : {1, 3})
      for (int kind = 0; kind <= 2; ++kind) {
        if (kind == 2 && nm != 1) continue;  // the six sums serve one kept mode
        pic1dp_input in{};
        in.nx = nx, in.nmode = nm, in.nspecies = 1, in.lx = 2.0 * kPi / 0.36;
        in.nparticle_max = in.species_nparticle_init[0] = 100001;
        for (int m = 0; m < nm; ++m) in.modes[m] = m + 1;
        const ModeTables t = mode_tables(in, kind);
        const Old o = old_tables(&in, kind);
        const bool ok = same(t.fre, o.fre) && same(t.fim, o.fim) && same(t.ginv, o.gi) && same(t.tabA, o.ta) && same(t.tabB, o.tb) &&
                        std::memcmp(&t.pred_tab, &o.pt, sizeof(PredTab)) == 0;
        if (!ok) {
          std::printf("nx %d, %d kept modes, pred_kind %d: the tables differ\n", nx, nm, kind);
          ++bad;
        }
        ++cases;
        // the plan the same input gets, on one rank and as the second of two ranks with eight reference blocks
        Settings cfg = settings_from_env();
        cfg.pred_kind_req = kind;
        for (const pic1dp_layout &lay : {pic1dp_layout{0, 1, 0, -1}, pic1dp_layout{1, 2, 8, -1}}) {
          const ContextPlan p = plan_context(in, lay, cfg);
          int64_t slots = 0;
          for (int64_t a : p.blk_alloc) slots += a;
          if (slots != p.nalloc || p.np[0] != p.nalloc || static_cast<int>(p.blk_np[0].size()) != p.nblk) {
            std::printf("nx %d, %d kept modes: the plan's blocks do not add up\n", nx, nm);
            ++bad;
          }
        }
      }
  std::printf("%d cases, %d differ\n", cases, bad);
  return bad ? 1 : 0;
}
