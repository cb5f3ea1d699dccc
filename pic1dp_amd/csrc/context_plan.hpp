// context_plan.hpp -- what create() decides before its first allocation, as a pure function of the input, the layout and
// the settings: the owned blocks and slots, the accumulators' copies, which one-pass kernel the context runs (the
// decision every headline number rests on), the sizes of its buffers -- and the mode tables of field_init, filled on the
// host with libm.  No context, no HIP call; tests/test_context_plan_host.py pins the plan against a table recorded from
// create()'s own formulas (include/pic1dp_probe.h), tests/mode_tables_check.cpp the tables bit for bit.
#pragma once
#include <vector>

#include "kernels.hpp"
#include "settings.hpp"

namespace pic1dp {

struct ContextPlan {
  // owned reference blocks [blk0, blk0 + nblk) of the npe blocks the reference run had ranks
  int npe = 1, nblk = 1, blk0 = 0;
  std::vector<int64_t> blk_alloc;            // [nblk] allocated slots of each owned block
  std::vector<std::vector<int64_t>> blk_np;  // [nspecies][nblk] valid markers as the loader leaves them
  int64_t nalloc = 0;                        // slots of every species: the owned blocks' together
  int64_t np[PIC1DP_MAX_SPECIES] = {0};      // valid markers of each species as the loader leaves them
  int imerge = 0, iremove = 0, isplit = 0;   // particle_imerge / _iremove / _isplit as particle_init leaves them
  // species charge accumulators
  int gcopies = 1, gstride = 0;              // GridConst
  size_t rho_set_doubles = 0;                // one of the three sets (kernels.hpp FusedSolve)
  // one pass per step
  int pred_kind = 0;                         // 0 no one-pass step here, 1 prediction tiles (k_step_one), 2 six sums (k_step_sums)
  int pred_private = 0;                      // pred_kind 2 and E0, Eh, the table tiles and the private sums of two workgroups fit a
                                             // CU's LDS: the sums are taken by k_step_one<PRIV> (thread-private LDS slots)
  size_t pred_set_doubles = 0;               // one of the three sets of prediction accumulators (0: none)
  size_t pack_doubles = 0;                   // d_pack (0: none)
  // field
  int tab_lds = 0;                           // FieldArgs: the tables are staged in LDS (they fit)
  int field_npe = 1;                         // FieldArgs::npe: the summation order
  double sc_re = 0.0, sc_im = 0.0;           // FieldArgs
};

ContextPlan plan_context(const pic1dp_input &in, const pic1dp_layout &lay, const Settings &cfg);

// the operators of field_init (src/pic1dp_field.F90:158-210), stored mode-major, and what the prediction makes of them
struct ModeTables {
  std::vector<double> fre, fim, ginv;  // [nmode][nx] cos, -sin; [nmode] 1 / k
  std::vector<double> tabA, tabB;      // pred_kind != 0: E = sum re_m A_m + im_m B_m
  PredTab pred_tab{};                  // pred_kind 2: sums / Gram matrix of the kept mode's tables
};
ModeTables mode_tables(const pic1dp_input &in, int pred_kind);

}  // namespace pic1dp
