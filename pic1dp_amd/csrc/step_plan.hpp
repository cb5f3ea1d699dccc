// step_plan.hpp -- what a time step launches, decided in one place as pure functions of plain data: which marker kernel
// runs and how, whether -f0'/f0 is carried, whether the launch streams non-temporally, whether it carries the previous
// step's solve or leaves its own to the next launch, whether its tail packs or posts the charge, and which field launch
// follows.  No context, no HIP call: capi_step.cpp fills StepFacts from the context (facts_of), asks, and keeps the
// actions -- pointers, versions, counters, spans, the order of every enqueue.  tests/test_step_plan_host.py pins every
// answer against a table recorded from the conditions as capi_step.cpp held them (tests/golden/gen_step_plan.py), through
// include/pic1dp_probe.h.
#pragma once
#include "context_plan.hpp"
#include "launch_policy.hpp"
#include "settings.hpp"
#include "timing.hpp"

namespace pic1dp {

constexpr bool kCarryOneExpDefault = false;  // k_step_one with the one-exp form of -f0'/f0: carry it (72 B) or evaluate it again (56 B)

// what the decisions look at besides input, plan and settings: what setters and the communicator change
struct StepFacts {
  const pic1dp_input *in;
  const ContextPlan *plan;
  const Settings *cfg;
  LaunchPolicy pol;
  int charge_sum, diag_sum, fuse_output, step_mode, field_solver, field_transform;
  bool several_ranks;  // the layout says so, or a communicator exists
  bool xchg_active;    // the one-hop exchange sums the charge
  bool has_comm;       // an RCCL communicator exists
  int field_npe;       // FieldArgs::npe
  int chain_mfma;      // FieldArgs::chain_mfma
  bool has_pred;       // the prediction accumulators exist (d_pred)
  int64_t np[PIC1DP_MAX_SPECIES];
  bool pow2[PIC1DP_MAX_SPECIES], one_exp[PIC1DP_MAX_SPECIES];  // SpeciesConst
};

// which path: predicates of the context, evaluated once per API call
struct StepCaps {
  // The fused and predicted paths -- the pair solves, the solve in a marker launch's prologue (kernels.hpp FusedSolve), the
  // prediction tiles and sums, Eh from its kept modes, the tail, the exchange inside the solve's launch -- reproduce the
  // dense-table solve of the mode-filter solver, and only that: not the finite differences (field_solver 1), not the FFT
  // (field_transform 1), under which every solve goes through the plain launch.
  bool dft_paths;
  bool six_sums_one_mode;       // the prediction is the six sums of ONE kept mode: what the pair solve of the call sites, the fused solve and the tail are written for
  bool modes_fit_field_kernel;  // the kept modes fit the one-workgroup field kernels
  bool exp_bearing;             // -f0'/f0 of the distribution bears an exp (two-stream2, bump-on-tail)
  bool step_recompute_ok;       // the whole-step kernels run (step mode 0 and their tiles fit the LDS; kind 1 of the charge sum: up to nx 5080)
  // One pass per step (k_step_one) needs: the mode-filter solver (the kept modes must describe E), few kept modes, and LDS
  // for E0, Eh, the mode tables and the four accumulators (kind 1 of the charge sum: no prediction -- two passes per step)
  bool predict_capable;
  // Does a step that output_all follows take the diagnostics inside its marker kernel (k_step_full<DIAG>)?  fuse_output 2:
  // always.  1 (what a host that calls output_all at the reference's cadence asks for): only where the step is not a
  // predicted one-pass step anyway.  Where it is, k_step_full<DIAG> costs the prediction -- the step after the output pays a
  // first-sub-step pass again: 10 steps + output_all at 1e8 markers 10.57 ms against 9.5 for ten plain steps --, whereas
  // k_step_one followed by the diagnostics' own pass costs that pass alone (profiles/r05/experiments/diag_bench.log).
  // (kind 1 of the charge sum or of the diagnostics sum: never -- the diagnostics keep their own pass and summation)
  bool diag_in_step;
  bool priv;  // k_step_one<PRIV>: Eh from its tile
  // One launch per time step (kernels.hpp FusedSolve): may the solve of a step be left to the prologue of the next step's
  // marker launch?  One rank, the six-sum prediction of one kept mode, the mode-filter solver, partial chains of an
  // npe-rank order that fit the prologue's scratch (npe <= 32), a grid of at most the resident workgroups -- EVERY
  // workgroup runs the solve, an oversubscribed grid pays it per round (profiles/r04/experiments/ab_fused_solve.log) -- and
  // serial forward sums of at most 1024 terms (nx / 3 through the matrix unit in the one-rank order, nx / npe otherwise;
  // ab_fused_solve_mfma_chain.log).  PIC1DP_FUSE_SOLVE=2 fuses whatever the length.
  bool fuse_capable;
  bool lazy_calls_ok;       // a push may be noted (unless an optimisation is due: lazy_ok)
  bool pair_serves_collect;  // call sites: a collect_charge after push(1) is served from the previous pair solve (if Eh is current)
  bool pair_in_solve_field;  // call sites: the solve_field behind the collect_charge of push(2) solves both fields (if the prediction is usable)
};
StepCaps step_caps(const StepFacts &f);
inline bool lazy_ok(const StepCaps &k, bool optimize_due) { return k.lazy_calls_ok && !optimize_due; }

// -f0'/f0 through memory (Species::t2) instead of a second evaluation
enum class Carry : int { None, HalfToFull, OnePass };

struct SpeciesLaunch {
  bool launched;        // the species has markers
  StepFamily family;    // pred only
  LaunchCfg lc;
  int dyn_tail;         // sixteenths of a workgroup's chunks its waves draw
  int64_t plain_chunks; // pred only: chunks at the slab's head that stay in the Infinity Cache
  Carry carry;
  bool tail;            // this launch's last workgroup packs / posts the charge (unless it carries a fused solve)
  char name[64];        // what kernel_bytes reports (the wiring appends " + field solve")
};
// what the marker launches of one sub-step of the whole-step path do
struct MarkerPlan {
  bool pred;          // k_step_one / k_step_sums: the full step + the prediction of the next first sub-step's charge
  bool priv;          // k_step_one<PRIV>
  bool diag;          // k_step_full<DIAG>: the diagnostics of output_all in the same pass
  int tail_mode;      // kernels.hpp StepTail: 0 none, 1 packed for one all-reduce, 2 posted into the peers' exchange slots ...
  int tail_species;   // ... by the launch of this species (the last one that has markers; -1: none)
  int stream_nt;      // 1: non-temporal loads and stores
  int solve_species;  // pred: the first species launched, whose prologue carries a pending fused solve (-1: none) ...
  bool solve_fits;    // ... and can (launch_policy.hpp fits_fused_solve), in workgroups of solve_threads
  int solve_threads;
  int tag;            // timing.hpp kTagStepOne / kTagStepFull / kTagStepHalf
  double rd, wr;      // bytes per marker read and written: x, v, p (+ w) read; x (+ v) (+ w) written by a full step
  SpeciesLaunch sp[PIC1DP_MAX_SPECIES];
};
// nt_force: PIC1DP_NT_FORCE of a tuning build (-1: unset); eh_modes: where the kept mode of Eh lies (0 nowhere)
MarkerPlan plan_markers(const StepFacts &f, const StepCaps &k, bool full, bool diag, bool pred, bool tail_ok, int eh_modes,
                        int nt_force);
// bytes per marker a carry moves: loaded says that the launch reads values stored for these very markers
inline double carry_bytes(Carry c, bool loaded) { return c == Carry::OnePass ? (loaded ? 16.0 : 8.0) : (c == Carry::HalfToFull ? 8.0 : 0.0); }

// charge sum over ranks and field solve behind the marker launches of a sub-step
enum class SolveLaunch : int {
  Plain,             // enqueue_field_solve: the mode-filter solve by tables or FFT, or the finite differences behind it
  Exchange,          // the exchange inside the solve's launch
  PairAccumulators,  // both fields in one launch, the charge from the accumulators (one rank)
  PairPacked,        // ... from the packed all-reduce
  PairExchange,      // ... from ONE exchange: charge2 and the prediction slices travel together
  PairPosted,        // ... whose own half the marker launch's tail has posted already
};
struct SolvePlan {
  int refused;        // 0; 1: a packed charge nobody reduces; 2: a posted charge nobody waits for
  bool reduce_first;  // reduce_charge in front of the solve
  bool pack_reduce;   // one all-reduce of the packed vector (both charge sums of the step) ...
  bool pack_first;    // ... packed by a launch of its own (the tail has not)
  SolveLaunch launch;
  bool with_local;    // Plain: the species sum is the launch's (one rank)
};
// pred_fresh: a predicting launch ran and its sums belong to the markers as they are; tail_done: what its tail did;
// into_E: the solve writes field_electric
SolvePlan plan_solve(const StepFacts &f, const StepCaps &k, bool pred_fresh, int tail_done, bool into_E);

// one iteration of pic1dp_hip_step
struct StepMoment {
  bool pending;       // the previous launch left its solve to this one (fused_pending)
  bool have_eh;       // d_Ehn is the half-step field of the step about to be taken
  int steps_left;     // of this call, this one included
  bool output_now;    // output_all follows this step ...
  bool output_next;   // ... the next one
  bool optimize_now;  // a marker optimisation is due in this step ...
  bool optimize_next; // ... in the next one
};
struct WholeStepPlan {
  bool substeps;        // the step goes through the sub-step kernels (an optimisation is due, or no whole-step kernel here)
  bool finish_pending;  // the pending solve gets a launch of its own first (then ask again: it may leave a current Eh)
  bool diag, pred;      // what the full launch is asked for (plan_markers has the last word)
  bool fused_in;        // its prologue solves the previous step's field
  bool adopt_eh;        // Eh of this step is the predicted one (d_Ehn)
  bool half_pass;       // ... or comes from a first-sub-step pass over the markers, which leaves eh_modes = half_eh_modes
  int half_eh_modes;
  bool fuse_out;        // this step's solve is left to the next launch
};
WholeStepPlan plan_whole_step(const StepFacts &f, const StepCaps &k, const StepMoment &m);

}  // namespace pic1dp
