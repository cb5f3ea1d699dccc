// call_plan.hpp -- the call sites' lazy state machine decided in one place as a pure function of plain data:
// for a call arriving in a state, what is enqueued in which order and which state follows.  No context, no HIP call:
// capi_step.cpp fills CallState and CallMoment from the context (call_state_of, call_moment_of), asks plan_call, walks the
// actions through its enqueue helpers and stores the state that follows (run_call).  tests/test_call_plan_host.py pins every
// answer against a table transcribed from the conditions as capi_step.cpp and the intruding entry points held them
// (tests/golden/gen_call_plan.py), and tests/call_plan_check.cpp walks the whole state space.
#pragma once
#include <cstdint>

#include "step_plan.hpp"

namespace pic1dp {

// ---------------------------------------------------------------------------
// The call sites' state.  Two variables, each an enum, and a table of the pairs that can occur -- until round 6 this was
// lz, half_pair, half_solved and cd_lazy, 4 x 2 x 2 x 6 combinations of which 20 are legal, policed from outside by
// pic1dp_hip_check_state; now an illegal one cannot be stored (plan_call refuses it, set_call_state again).
//
// Seq: where the host stands in the reference's sequence push(1), collect_charge, solve_field, push(2), collect_charge,
// solve_field of a time step (src/pic1dp.F90:79-90), and -- the "Pair" states, one rank, six sums -- whether the half
// step is being served from the PREVIOUS step's pair solve: the half-step field then lies in d_Ehn / d_mode_h,
// field_electric still holds the step-start field, d_E0 is not filled.
enum class Seq : uint8_t {
  Clean,            // memory is what eager calls would have left; nothing noted
  Push1,            // push(1) noted
  Half,             // ... and its collect_charge served (k_step_half ran, or the prediction was taken); the half-step markers are not in memory
  HalfPair,         // Half, served from the pair solve: nothing was launched; the host has not yet called solve_field for the half step
  HalfPairSolved,   // ... and now it has: what it may SEE from here on is the half-step field (every reader settles first)
  Push2,            // push(2) noted after Half
  Push2Pair,        // push(2) noted after HalfPair (the host skipped the half step's solve_field: it pushes with the old field)
  Push2PairSolved,  // push(2) noted after HalfPairSolved: the next collect_charge runs k_step_one with E0 = field_electric, Eh = d_Ehn
  N
};
// Owed: what collect_charge has left to the launch of the solve_field that follows (one launch less per sub-step)
enum class Owed : uint8_t {
  Nothing,         // field_chargeden is current
  Scale,           // d_charge holds the summed charge1: the scaling into chargeden
  SumScale,        // (one rank) the species accumulators hold the deposits: species sum + scaling -- with a usable six-sum prediction: the pair solve
  PredTiles,       // (one rank, tiles) the prediction accumulators hold the half-step charge as coefficients: combine + sum + scale
  PredSums,        // (one rank, six sums) the kept mode's content of chargeden follows from the six sums
  AdoptHalfField,  // nothing to launch: field_electric / its kept mode / chargeden <- what the pair solve left in d_Ehn / d_mode_h / d_cd_h
  N
};
enum { LZ_CLEAN = 0, LZ_PUSH1, LZ_HALF, LZ_PUSH2 };   // the four positions of the sequence (Seq without the pair's colours)
constexpr int lz_of(Seq s) {
  return s == Seq::Clean ? LZ_CLEAN : s == Seq::Push1 ? LZ_PUSH1 : (s == Seq::Half || s == Seq::HalfPair || s == Seq::HalfPairSolved) ? LZ_HALF : LZ_PUSH2;
}
constexpr bool pair_of(Seq s) { return s == Seq::HalfPair || s == Seq::HalfPairSolved || s == Seq::Push2Pair || s == Seq::Push2PairSolved; }
constexpr bool solved_of(Seq s) { return s == Seq::HalfPairSolved || s == Seq::Push2PairSolved; }
// the same position with the pair settled (memory as the eager calls leave it)
constexpr Seq unpaired(Seq s) { return lz_of(s) == LZ_HALF ? Seq::Half : lz_of(s) == LZ_PUSH2 ? Seq::Push2 : s; }
// push(2) noted at a half step
constexpr Seq push2_noted(Seq s) { return s == Seq::HalfPair ? Seq::Push2Pair : s == Seq::HalfPairSolved ? Seq::Push2PairSolved : Seq::Push2; }
// Which (Seq, Owed) pairs occur.  Scale / SumScale: right behind a collect_charge (every other call that looks at the
// charge settles it first).  PredTiles / PredSums: behind the collect_charge of a noted push(1) -- and still owed after a
// look at the MARKERS has put the half-step state into memory (particles_download materialises the markers, not the
// charge: Clean with a prediction owed; the fuzz campaign of round 6 found that one, 5 seeds in 4 500).
// AdoptHalfField is set with HalfPair and outlives it when a look at the field settles the pair before solve_field came
// (the field is then adopted by copying); it ends with the solve_field of the half step, hence never with a Solved state.
// It is made for the half-step charge density, so it never outlives the half step: whatever puts the markers into memory
// while it is owed deposits that charge density for real instead -- never Clean or Push1 -- and whatever writes
// field_chargeden drops it (CallState::adopt_current, pic1dp_hip_check_state).
constexpr bool kCallStateLegal[static_cast<int>(Seq::N)][static_cast<int>(Owed::N)] = {
    //                   Nothing Scale  SumScale PredTiles PredSums Adopt
    /* Clean           */ {true, true,  true,    true,     true,    false},
    /* Push1           */ {true, false, false,   false,    false,   false},
    /* Half            */ {true, true,  true,    true,     true,    true},
    /* HalfPair        */ {false, false, false,  false,    false,   true},
    /* HalfPairSolved  */ {true, false, false,   false,    false,   false},
    /* Push2           */ {true, false, false,   false,    false,   true},
    /* Push2Pair       */ {false, false, false,  false,    false,   true},
    /* Push2PairSolved */ {true, false, false,   false,    false,   false},
};

// what the machine remembers between two calls
struct CallState {
  Seq seq = Seq::Clean;
  Owed owed = Owed::Nothing;
  // The collect_charge of a push(2) noted after a pair-solved half step (Push2PairSolved) runs the whole step with
  // E0 = field_electric and leaves field_electric holding the STEP-START field, the kept modes too: the solve_field that
  // follows overwrites both.  Everything that reads them before it first copies the half-step field (d_Eh / d_mode_h) in
  bool e_step_start = false;
  // field_chargeden holds only the kept mode's content of the half-step charge density (collect_charge after a noted
  // push(1) served from the six sums): all solve_field looks at, but not what the reference holds there
  bool cd_kept_mode_only = false;
  // an owed AdoptHalfField stands for a solve from the field_chargeden the eager calls hold NOW (the context: cd_version
  // has not moved since the collect_charge that set it); false whenever nothing of the kind is owed
  bool adopt_current = false;
  bool charge_pending = false;       // charge_local ran, waiting for charge_reduced
  bool charge_pending_pred = false;  // ... and handed out the six sums, not a charge vector
  // where the host stands in the six calls by the calls alone: 0 between time steps, 1 ... 5 after the first ... fifth
  int8_t call_phase = 0;
  int8_t eh_modes = 0;  // where the kept mode of the Eh about to be used lies: 0 nowhere, 1 fa.mode_*, 2 d_mode_h
};
inline bool operator==(const CallState &a, const CallState &b) {
  return a.seq == b.seq && a.owed == b.owed && a.e_step_start == b.e_step_start && a.cd_kept_mode_only == b.cd_kept_mode_only &&
         a.adopt_current == b.adopt_current && a.charge_pending == b.charge_pending && a.charge_pending_pred == b.charge_pending_pred &&
         a.call_phase == b.call_phase && a.eh_modes == b.eh_modes;
}

// what a decision looks at besides the state and the StepCaps.  The first block is the context's own (settings, layout,
// switches); the second changes from call to call
struct CallMoment {
  bool lazy_calls = true;      // cfg.lazy_calls
  bool call_pair = true;       // cfg.call_pair
  bool loaded = true;          // markers exist
  bool several_ranks = false;
  bool fp64_rank_sum = false;  // ... and their charge is summed in FP64 (kind 0 of the charge sum)
  int charge_sum = 0;
  int pred_kind = 0;           // plan.pred_kind
  bool tab_lds = false;        // fa.tab_lds: the field kernels hold the mode tables in the LDS

  bool field_differs = false;  // SwitchField: the solver or transform asked for is not the one an owed field was solved with
  bool pred_usable = false;    // the prediction in d_pred belongs to the markers and the field as they are, and may be used
  bool eh_current = false;     // d_Ehn is the half-step field of the markers and the field as they are
  bool modes_current = false;  // the kept modes describe field_electric (modes_field_version == field_version)
  bool optimize_due_any = false;
  bool output_follows = false;
};

// The kinds of call, by what they do to memory
enum class Call : uint8_t {
  Push1, Push2, CollectCharge, ChargeLocal, ChargeReduced, ChargeLocalExact, ChargeExactHandedOut, ChargeReducedExact, SolveField,
  Markers,          // reads or writes markers or accumulators: memory first becomes what the eager calls would have left
  ReadMarkers,      // reads markers only (downloads, the products, the digest): a noted push becomes memory, the charge stays owed
  WholeSteps,       // Markers, then pic1dp_hip_step(n > 0): field_chargeden is rewritten, the host stands between time steps
  Substep1, Substep2,  // Markers, then pic1dp_hip_substep
  ReadField,        // reads the field only (field_energy, the power products)
  GetField,         // ... and the charge settled (get_field that does not ask for chargeden)
  GetFieldCd,       // reads field and chargeden: the whole vector where only the kept mode's content was formed
  OutputAll,        // Markers, then GetField (output_all that does not ask for chargeden)
  OutputAllCd,      // Markers, then GetFieldCd
  WriteElectric,    // writes field_electric
  WriteChargeden,   // writes field_chargeden
  ReplaceMarkers,   // particle_load, particle_load_device
  UploadMarkers,    // particles_upload: one species' markers replaced
  SwitchField,      // switches solver or transform
  BetweenSteps,     // must stand between time steps (set_charge_sum, set_diag_sum): a refusal, not an action
  Checkpoint,       // ... and checkpoint_write, which settles what a time step's end may still owe
  N
};

// today's enqueue helpers, named; the bookkeeping they do beside a launch is theirs unless it is listed here
enum class Act : uint8_t {
  SaveStepStartField,   // d_E0 <- field_electric
  AdoptHalfField,       // field_chargeden, field_electric and its kept modes <- d_cd_h, d_Ehn, d_mode_h
  AdoptHalfModes,       // the kept modes alone
  CopyEhToE,            // field_electric <- d_Eh
  PushEager1,           // k_push, sub-step 1, with field_electric
  PushEager1FromE0,     // ... with d_E0, the field the noted push(1) saw
  PushEager2,
  WrapOnly,             // the deposit's wrap of x, charge discarded
  Deposit,
  HalfPass,             // the whole-step path's first-sub-step pass (k_step_half)
  SwapEh,               // d_Eh <-> d_Ehn
  FullPass,             // the whole-step kernel: arg = FullPassArg bits
  FxSettle,
  ReduceCharge,
  Chargeden,            // charge -> field_chargeden
  ChargedenSum,         // ... with the species sum
  PredChargeden,        // the six sums -> the kept mode's content of field_chargeden
  PredChargedenSummed,  // ... from the sums as they came back summed over ranks in d_charge
  PredCombine,          // the tiles -> charge
  PredToCharge,         // the six sums -> the head of d_charge
  PredReduce,           // d_charge summed over ranks
  ChargeLocal,          // the species sum into d_charge, for the host to sum over ranks
  FxToRho,              // the exact limbs the host summed -> the species accumulators
  SolvePair,            // both fields in one launch
  SolvePredTiles, SolvePredSums,
  SolvePlain,           // arg bit 0: with the species sum; bit 1: from field_chargeden
  // bookkeeping beside the launches
  StateVersion,         // state_version++
  CdVersion,            // cd_version++
  FieldWrittenBySolve,  // field_written(by_solve)
  CallPairSkip,         // call_pair_skips++
  PredConsumed,         // pred_version = 0
  MarkEhCurrent,
  // timer spans: what lies between a begin and SpanEnd is booked under it (a whole-step kernel books itself under "push particle")
  SpanCollect, SpanField, SpanEnd,
  N
};
// FullPass: bit 0 E0 = d_E0 (else field_electric); bit 1 Eh = field_electric (else d_Eh); bit 2 diag; bit 3 pred; bits 4-5 eh_modes
enum : uint8_t { kFullE0Saved = 1, kFullEhIsE = 2, kFullDiag = 4, kFullPred = 8, kFullEhModesShift = 4 };

enum class Refusal : uint8_t {
  None,
  NotLoaded,               // no particles
  ChargeWaiting,           // charge_local is waiting for charge_reduced
  IllegalState,            // internal: a (Seq, Owed) pair that cannot occur (CallPlan::bad_seq, bad_owed)
  EagerNoted,              // internal: a push noted by eager call sites
  WantsExactLocal, WantsExactReduced,   // exact charge sum: the FP64 split phase is refused
  NeedsExactSum,           // the exact split phase without set_charge_sum(1)
  ReducedWithoutLocal,
  NotBetweenSteps,         // BetweenSteps: a push, a charge or a solve is pending
  CheckpointChargeWaiting, CheckpointPushNoted, CheckpointInsideStep,
  CheckpointKeptMode,      // refused AFTER the plan's actions (CallPlan::refused_after): the settling has been done by then
  PlanTooLong,             // internal: more than kMaxActs actions (no call comes near)
  N
};

constexpr int kMaxActs = 24;
struct CallPlan {
  uint8_t n = 0;
  Act act[kMaxActs] = {};
  uint8_t arg[kMaxActs] = {};
  CallState next;
  Refusal refusal = Refusal::None;
  bool refused_after = false;   // the actions run and the state is stored, then the call fails
  Seq bad_seq = Seq::Clean;     // IllegalState: the pair
  Owed bad_owed = Owed::Nothing;
};

CallPlan plan_call(const CallState &s, const CallMoment &m, const StepCaps &k, Call call);

// the prediction -> chargeden of the next first sub-step, for the call sites and for the step path: the launches in order
// (PredConsumed first).  defer (call sites): leave what the solve_field that follows can take over to it -- *owed says what
struct PredPlan {
  uint8_t n = 0;
  Act act[4] = {};
  Owed owed = Owed::Nothing;
};
PredPlan plan_pred_chargeden(const CallMoment &m, const StepCaps &k, bool defer);

// the relations between the parts of the state, and between the state and the context it is held in, that hold between
// any two calls: nullptr, or the text of the first one that does not
const char *call_state_invariants(const CallState &s, const CallMoment &m, const StepCaps &k);

const char *call_name(Call c);

}  // namespace pic1dp
