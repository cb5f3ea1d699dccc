// settings.hpp -- what a context takes from the environment, read once by create() (settings.cpp: no HIP call) and
// constant from then on: pic1dp_ctx::cfg.  The product variables are those of INTEGRATION.md section 6; the others only a
// -DPIC1DP_TUNING build looks at (kernels.hpp tuning_env).  The request pred_kind_req is kept as given:
// context_plan.cpp decides whether it can be served.  Variables read per call (PIC1DP_LOAD_THREADS, PIC1DP_OPT_*,
// PIC1DP_XCHG_*, PIC1DP_NT_FORCE, ...) stay where they are read.
#pragma once

namespace pic1dp {

struct Settings {
  int fuse_solve = 1;     // PIC1DP_FUSE_SOLVE=0: the field solve always in a launch of its own; 2: fused whatever the grid
  int tail_on = 1;        // PIC1DP_TAIL=0: the packing of this rank's charge in a launch of its own (kernels.hpp StepTail)
  int call_pair = 1;      // PIC1DP_CALL_PAIR=0: the three launches per step of rounds 2-4 (ctx.hpp "Pair" states)
  int lazy_calls = 1;     // PIC1DP_LAZY_CALLS=0: every call launches its own kernel at once
  int predict = 1;        // PIC1DP_PREDICT=0: always two passes per step
  int carry = -1;         // whole-step kernels carry -f0'/f0 between them: -1 where measured to pay, 0 never
                          // (PIC1DP_CARRY=0), 1 wherever -f0'/f0 bears an exp, 2 also two-stream2 between k_step_half / _full
  int osub_req = 0;       // PIC1DP_OSUB: grid size of the marker kernels in units of the resident one (0: auto)
  int dyn_tail = 8;       // PIC1DP_DYN_TAIL: sixteenths of a workgroup's 64-pair chunks its waves DRAW from an LDS counter (every whole-step kernel)
  int dyn_tail_full = 16; // ... of k_step_full (PIC1DP_DYN_TAIL sets both, PIC1DP_DYN_TAIL_FULL this one)
  // marker state (bytes) above which k_step_half / k_step_full stream non-temporally
  // The two kernels leave the caches to each other, so the pairs were compared inside
  // one process on the same arrays (tools/ab_nt.py, nx = 1024, half + full in ms):
  //   markers   plain/plain   nt/nt    half nt, full plain   half plain, full nt
  //   6.4e6       0.102*      0.114         0.105                 0.106
  //   1e7         0.159       0.169         0.158*                0.158*
  //   2e7         0.372       0.332         0.326                 0.319*
  //   3e7         0.539       0.497         0.492                 0.483*
  //   5e7         0.886       0.829*        0.835                 0.828*
  //   1e8         1.745       1.657*        1.676                 1.678
  // => both plain below 288 MiB of marker state, the full kernel non-temporal above
  //    it, the half kernel only above 2 GiB
  double nt_threshold_half = 2048.0 * 1048576.0, nt_threshold_full = 288.0 * 1048576.0;
  int diag_fx = 1;                  // PIC1DP_DIAG_FX=0: the diagnostics' histograms always as double sums
  double diag_fx_margin_w = 16.0;   // bound on |w| = this x the last pass's max |w| (PIC1DP_DIAG_FX_MARGIN: tests)
  int pred_kind_req = 0;            // PIC1DP_PRED_KIND=1|2|3 insists on tiles | sums | sums in registers (tests); 0: the library's choice
  int chain_mfma_req = -1;          // PIC1DP_CHAIN_MFMA: -1 unset (the matrix unit if create()'s self-test agrees), 0 never, 1 insisted on
  int gcopies_req = 0;              // PIC1DP_RHO_GLOBAL_COPIES: copies of the species accumulators asked for (0: the measured choice)
  int field_one_rank_order = 0;     // PIC1DP_FIELD_ONE_RANK_ORDER=1: the field's sums in the one-rank order whatever npe (tests)
  int chain_selftest_verbose = 0;   // PIC1DP_CHAIN_SELFTEST_VERBOSE=1: create()'s self-test reports to stderr
};

// PIC1DP_RHO_GLOBAL_COPIES as given -> gcopies_req: powers of two 1 ... 64 only, anything else is no request
inline int accepted_gcopies(int k) { return (k >= 1 && k <= 64 && (k & (k - 1)) == 0) ? k : 0; }

Settings settings_from_env();

}  // namespace pic1dp
