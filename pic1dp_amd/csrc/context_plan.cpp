// context_plan.cpp -- create()'s decisions and the mode tables (context_plan.hpp).  No context, no HIP call.
#include "context_plan.hpp"

#include <cmath>

#include "launch_policy.hpp"
#include "loader.hpp"

namespace pic1dp {

namespace {
constexpr double kPi = 3.14159265358979323846264;  // PETSC_PI
}

ContextPlan plan_context(const pic1dp_input &in, const pic1dp_layout &lay, const Settings &cfg) {
  ContextPlan p;
  const int nx = in.nx, nm = in.nmode, ns = in.nspecies;
  p.npe = lay.npe <= 0 ? lay.nranks : lay.npe;
  p.nblk = p.npe / lay.nranks;
  p.blk0 = lay.rank * p.nblk;
  // particle storage: valid markers of the owned blocks packed first, block
  // tails (allocated but unloaded slots) behind them
  p.blk_alloc.resize(p.nblk);
  p.blk_np.assign(ns, std::vector<int64_t>(p.nblk, 0));
  for (int b = 0; b < p.nblk; ++b) {
    p.blk_alloc[b] = block_alloc(in.nparticle_max, p.blk0 + b, p.npe);
    p.nalloc += p.blk_alloc[b];
    for (int s = 0; s < ns; ++s) {
      p.blk_np[s][b] = block_np(in, s, p.blk0 + b, p.npe);
      p.np[s] += p.blk_np[s][b];
    }
  }
  // particle_init, src/pic1dp_particle.F90:73-87
  p.imerge = in.nmerge > 0 ? 1 : 0;
  p.iremove = in.nremove > 0 ? 1 : 0;
  p.isplit = in.nsplit > 0 ? 1 : 0;

  // species charge accumulators in gcopies copies: workgroup b adds its LDS tile into copy b % gcopies,
  // so an address receives 1/gcopies of the flush atomics; the field kernels add the copies up.
  // Measured (tools/fresh_and_flush.sh): the flush into ONE copy costs 4.8 % of a step at 6.4e6
  // markers / nx 192, 1.5 % at 1e7 / 256, 0.9 % at 1e8 / 1024.  Eight copies (tools/ab_global_copies.sh)
  // win back 2 % of the step at nx 192, nothing at nx 256, and LOSE 4 % at 1.25e7 markers / nx 1024: the
  // one-workgroup field kernel then reads and re-zeroes 8 x nx words on the critical path.  So: eight
  // copies for small grids only.  PIC1DP_RHO_GLOBAL_COPIES overrides.
  p.gcopies = nx <= 256 ? 8 : 1;
  if (cfg.gcopies_req) p.gcopies = cfg.gcopies_req;
  p.gstride = ns * nx;
  p.rho_set_doubles = static_cast<size_t>(p.gcopies) * ns * nx;

  // one pass per step: with prediction tiles where they fit the LDS (k_step_one), as six sums for larger
  // grids with one kept mode (k_step_sums); PIC1DP_PRED_KIND=1|2|3 insists on tiles | sums | sums in registers (tests)
  const bool private_fits = 2 * (step_one_private_lds_bytes(nx) + kStaticLds) <= kCuLds;
  // The prediction tiles cost 2 + 4 nm LDS atomics at random cells per marker.  Measured against the two passes
  // (profiles/r04/experiments/ab_kept_modes.log, 1e8 markers / nx 1024, ms per step): two kept modes 1.23 against 1.46,
  // three 1.49 against 1.45, four 2.05 (nx 512) against 1.46.  With the tiles as fixed-point sums (round 6: kernels_step.hip
  // FxTiles) two kept modes run 1.06 and three 1.17 ms against the two passes' 1.40 (profiles/r06/experiments/ab_fx_tiles.log,
  // ab_nm3.log): the tiles serve up to three kept modes, four and more take the two passes.
  if (nm <= PRED_MAX_MODES && step_one_lds_bytes(nx, nm) <= PARTICLE_LDS_CAP)
    p.pred_kind = 1;
  // (the six sums travel in the head of an nx-vector on the call-site path: nx >= 8)
  else if (nm == 1 && nx >= 8 && step_sums_lds_bytes(nx) <= PARTICLE_LDS_CAP)
    p.pred_kind = 2;
  // One kept mode: the six sums in thread-private LDS slots (k_step_one<PRIV>) beat the tiles, whose six atomics per
  // marker at random cells pay ~3x in bank conflicts: -2 % at 1e8 markers / nx 1024 (profiles/r03/experiments/
  // ab_private_sums.log), and on the small grids too once the step is timed without per-kernel events in the stream:
  // 6.4e6 / nx 192 83.8 -> 76.6 us per step, 1e7 / nx 256 123.7 -> 116.5 (profiles/r04/experiments/ab_fused_solve.log)
  // -- wherever the slots of two workgroups fit (nx >= 8: the sums travel in the head of an nx-vector on the
  // call-site path).
  if (p.pred_kind == 1 && nm == 1 && nx >= 8 && private_fits) p.pred_kind = 2;
  bool sums_in_registers = false;
  {
    const int k = cfg.pred_kind_req;
    if ((k == 2 || k == 3) && nm == 1 && nx >= 8 && step_sums_lds_bytes(nx) <= PARTICLE_LDS_CAP) p.pred_kind = 2;
    if (k == 3) sums_in_registers = true;  // k_step_sums also where the private slots would fit (tests: the large-grid kernel at a small grid)
    // 1: the tiles wherever they fit (else the choice above stands)
    if (k == 1 && nm <= PRED_MAX_MODES && step_one_lds_bytes(nx, nm) <= PARTICLE_LDS_CAP) p.pred_kind = 1;
  }
  if (p.pred_kind == 2 && private_fits && !sums_in_registers) p.pred_private = 1;
  if (p.pred_kind) {
    p.pred_set_doubles = p.pred_kind == 2 ? 8 * PRED_SUM_COPIES : static_cast<size_t>(ns) * (1 + 2 * nm) * nx;
    p.pack_doubles = pack_doubles(nx, nm, p.pred_kind);
  }

  p.field_npe = cfg.field_one_rank_order ? 1 : p.npe;  // the summation order of the reference run being reproduced (PIC1DP_FIELD_ONE_RANK_ORDER=1: tests)
  p.tab_lds = (static_cast<size_t>(2) * nm * nx * sizeof(double) <= 96 * 1024) ? 1 : 0;
  p.sc_re = 1.0 / static_cast<double>(nx);    // src/pic1dp_field.F90:239
  p.sc_im = -1.0 / static_cast<double>(nx);   // :234
  return p;
}

ModeTables mode_tables(const pic1dp_input &in, int pred_kind) {
  const int nx = in.nx, nm = in.nmode;
  ModeTables t;
  std::vector<double> &fre = t.fre, &fim = t.fim, &gi = t.ginv;
  fre.resize(static_cast<size_t>(nm) * nx), fim.resize(static_cast<size_t>(nm) * nx), gi.resize(nm);
  for (int m = 0; m < nm; ++m) {
    const double mode = static_cast<double>(in.modes[m]);
    gi[m] = 1.0 / (2.0 * kPi / in.lx * mode);  // :166
    // two loops, plain cos() and plain sin(), as the reference's two fills
    // (:186-189, :194-197): a paired sincos can differ in the last bit
    double (*volatile cos_fn)(double) = std::cos;
    double (*volatile sin_fn)(double) = std::sin;
    for (int ix = 0; ix < nx; ++ix) {
      const double th = 2.0 * kPi / static_cast<double>(nx) * mode * static_cast<double>(ix);  // :188
      fre[static_cast<size_t>(m) * nx + ix] = cos_fn(th);
    }
    for (int ix = 0; ix < nx; ++ix) {
      const double th = 2.0 * kPi / static_cast<double>(nx) * mode * static_cast<double>(ix);  // :196
      fim[static_cast<size_t>(m) * nx + ix] = -sin_fn(th);
    }
  }
  if (pred_kind) {  // the tables: E = 2*(cos re + (-sin) im) (src/pic1dp_field.F90:251-257)
    t.tabA.resize(fre.size()), t.tabB.resize(fim.size());
    for (size_t i = 0; i < fre.size(); ++i) t.tabA[i] = 2.0 * fre[i], t.tabB[i] = 2.0 * fim[i];
    if (pred_kind == 2) {
      PredTab &pt = t.pred_tab;
      for (int ix = 0; ix < nx; ++ix) {
        pt.sum_fre += fre[ix], pt.sum_fim += fim[ix];
        pt.g11 += fre[ix] * fre[ix], pt.g22 += fim[ix] * fim[ix], pt.g12 += fre[ix] * fim[ix];
      }
    }
  }
  return t;
}

}  // namespace pic1dp
