// call_plan.cpp -- the decisions of the call sites' state machine (call_plan.hpp): conditions only.  The builder below keeps
// the shape the enqueuing functions of capi_step.cpp had -- one small function per way of settling -- but appends to a flat
// list and works on a copy of the state; plan_call has one case per kind of call.
#include "call_plan.hpp"

namespace pic1dp {

namespace {

struct Builder {
  CallState s;
  const CallMoment &m;
  const StepCaps &k;
  CallPlan p;
  bool markers_moved = false;  // an action of this plan bumps state_version: prediction and predicted field are stale from there

  bool refused() const { return p.refusal != Refusal::None; }
  bool refuse(Refusal r) {
    if (!refused()) p.refusal = r;
    return false;
  }
  void add(Act a, int arg = 0) {
    if (refused()) return;
    if (p.n == kMaxActs) {
      refuse(Refusal::PlanTooLong);
      return;
    }
    if (a == Act::PushEager1 || a == Act::PushEager1FromE0 || a == Act::PushEager2 || a == Act::Deposit || a == Act::StateVersion)
      markers_moved = true;
    p.act[p.n] = a;
    p.arg[p.n++] = static_cast<uint8_t>(arg);
  }
  bool pred_usable() const { return m.pred_usable && !markers_moved; }
  bool eh_current() const { return m.eh_current && !markers_moved; }

  // the one writer of (seq, owed): a pair that cannot occur is an internal error at the call that would have produced it
  bool set(Seq seq, Owed owed) {
    if (refused()) return false;
    if (seq >= Seq::N || owed >= Owed::N || !kCallStateLegal[static_cast<int>(seq)][static_cast<int>(owed)]) {
      p.bad_seq = seq, p.bad_owed = owed;
      return refuse(Refusal::IllegalState);
    }
    if (seq != Seq::Clean && !m.lazy_calls) return refuse(Refusal::EagerNoted);
    s.seq = seq, s.owed = owed;
    return true;
  }
  bool set_seq(Seq seq) { return set(seq, s.owed); }
  bool set_owed(Owed owed) { return set(s.seq, owed); }

  // field_electric and its kept modes as the eager calls leave them after push(2), collect_charge of a pair-solved step: the
  // half-step field (the whole-step kernel read the step-start field from field_electric; d_Eh / d_mode_h hold the half step's)
  void settle_step_start_field() {
    if (!s.e_step_start) return;
    s.e_step_start = false;
    add(Act::CopyEhToE);
    add(Act::AdoptHalfModes);
  }
  // field_chargeden (and d_charge, and zeroed accumulators) as collect_charge would have left them at once
  void materialize_cd() {
    const Owed pending = s.owed;
    if (pending == Owed::AdoptHalfField || pending == Owed::Nothing) return;  // (a half-step FIELD waiting to be adopted: no charge to settle)
    set_owed(Owed::Nothing);
    if (pending == Owed::PredSums) {
      add(Act::PredChargeden);
      return;
    }
    if (pending == Owed::PredTiles) add(Act::PredCombine);
    add(pending == Owed::SumScale ? Act::ChargedenSum : Act::Chargeden);
  }
  // The half-step field the pair solve left in d_Ehn / d_mode_h, and the step-start field still in field_electric, put where
  // the eager calls would have them -- d_E0 <- E, and, once the host has called solve_field for the half step, E <- the
  // half-step field with its kept modes (not yet called: it stays owed, AdoptHalfField, and copies when it comes)
  void settle_half_pair() {
    if (!pair_of(s.seq)) return;
    add(Act::SaveStepStartField);
    const bool solved = solved_of(s.seq);
    set_seq(unpaired(s.seq));
    if (solved) add(Act::AdoptHalfField);
  }
  // for readers of the field only: nothing to do until the host has called solve_field for the half step -- until then
  // field_electric is the step-start field, which is what d_E holds
  void settle_field_view() {
    settle_step_start_field();
    if (solved_of(s.seq)) settle_half_pair();
  }
  // field_chargeden as the reference holds it between the sub-steps where only the kept mode's content was formed, or where
  // a half-step field waits to be adopted: the half-step state is pushed into memory after all and deposited for real.  One
  // rank only -- on several ranks the reduction is a collective that an inspection on one of them must not start
  void rebuild_half_step_chargeden() {
    if (m.several_ranks) return;
    if (lz_of(s.seq) != LZ_HALF && lz_of(s.seq) != LZ_PUSH2) return;
    settle_half_pair();
    if (s.owed == Owed::AdoptHalfField) set_owed(Owed::Nothing);  // (its copy of the kept mode's content would overwrite the whole vector)
    const bool push2_was_noted = lz_of(s.seq) == LZ_PUSH2;
    add(Act::PushEager1FromE0);
    set_seq(Seq::Clean);  // memory now holds the half-step state (x not yet wrapped): the deposit wraps and stores it
    add(Act::Deposit);
    if (m.charge_sum == 1) add(Act::FxSettle);
    add(Act::ChargedenSum);
    s.cd_kept_mode_only = false;
    if (push2_was_noted) add(Act::PushEager2);  // (the field it sees is the one solve_field wrote after the half step)
  }
  // a noted push becomes memory: the ordinary kernels with the right field, bit for bit what the eager calls would have left
  void materialize() {
    settle_half_pair();
    const int lz = lz_of(s.seq);
    if (lz == LZ_CLEAN) return;
    // a half-step field waits to be adopted: it was solved from the half-step charge density, which leaves with the markers'
    // half-step state -- that state is deposited for real on its way into memory
    if (s.owed == Owed::AdoptHalfField) return rebuild_half_step_chargeden();
    set_seq(Seq::Clean);
    if (lz == LZ_PUSH1) return add(Act::PushEager1);  // the field has not changed since
    add(Act::PushEager1FromE0);                       // LZ_HALF / LZ_PUSH2: push(1) saw d_E0; its deposit wrapped x
    add(Act::WrapOnly);
    if (lz == LZ_PUSH2) add(Act::PushEager2);
  }
  // checks and the settling every call site that takes part in the lazy scheme begins with
  bool require_loaded_keep_lazy() {
    if (!m.loaded) return refuse(Refusal::NotLoaded);
    if (s.charge_pending) return refuse(Refusal::ChargeWaiting);
    settle_step_start_field();  // (a push or a step reads field_electric)
    materialize_cd();
    return !refused();
  }
  bool require_loaded() {
    if (!require_loaded_keep_lazy()) return false;
    materialize();
    return !refused();
  }
  // the deposit of collect_charge / charge_local into the species accumulators: the whole-step kernel of a noted push, or the
  // plain wrap + deposit
  void deposit_or_step() {
    if (s.seq == Seq::Push1) {
      add(Act::SaveStepStartField);
      add(Act::HalfPass);
      set_seq(Seq::Half);
      return;
    }
    if (lz_of(s.seq) == LZ_PUSH2) {
      if (s.seq == Seq::Push2Pair) settle_half_pair();  // (push(2) without the solve_field of the half step: it sees the old field)
      add(Act::StateVersion);
      const bool diag = k.diag_in_step && m.output_follows;
      const int want = (diag ? kFullDiag : kFullPred);
      if (s.seq == Seq::Push2PairSolved) {  // the half-step field came out of the previous step's pair solve: E0 is still in d_E
        add(Act::SwapEh);
        s.eh_modes = 2;  // its kept mode: d_mode_h
        add(Act::FullPass, want | (2 << kFullEhModesShift));
        s.e_step_start = true;  // (field_electric: still the step-start field -- the solve_field that follows overwrites it)
        set_seq(Seq::Clean);
        return;
      }
      // Eh = d_E: the kept modes describe it when the mode-filter solve wrote it last
      s.eh_modes = (k.dft_paths && m.modes_current) ? 1 : 0;
      add(Act::FullPass, want | kFullE0Saved | kFullEhIsE | (s.eh_modes << kFullEhModesShift));
      set_seq(Seq::Clean);
      return;
    }
    materialize();
    add(Act::Deposit);
  }
  void pred_to_chargeden(bool defer) {
    const PredPlan pp = plan_pred_chargeden(m, k, defer);
    if (m.pred_kind == 2) s.cd_kept_mode_only = true;
    for (int i = 0; i < pp.n; ++i) add(pp.act[i]);
    if (pp.owed != Owed::Nothing) set_owed(pp.owed);
  }
  // the call record: a collected charge and a solved field move on only from the call they follow in the reference's order
  void phase_collect() {
    if (s.call_phase == 1 || s.call_phase == 4) s.call_phase++;
  }
  void cd_version() {
    add(Act::CdVersion);
    s.adopt_current = false;
  }
  // the opening collect_charge and charge_local share.  The two differ, as they did as two copies: charge_local (split) does
  // not know the pair's short cut, drops a stale adoption BEFORE the predicted path where collect_charge does so behind it
  // (by storing (Half, Nothing)), and leaves cd_kept_mode_only alone on the predicted path.  Kept, not judged.
  // true: served without a pass over the markers
  bool collect_opening(bool split) {
    if (pair_of(s.seq) && s.seq != Seq::Push2PairSolved) settle_half_pair();  // out of sequence: memory as the eager calls leave it
    if (split && s.owed == Owed::AdoptHalfField) set_owed(Owed::Nothing);
    if (!split && s.seq == Seq::Push1 && k.pair_serves_collect && eh_current()) {
      // the half-step FIELD is solved already (the previous solve_field's pair): nothing to launch at all
      s.cd_kept_mode_only = true;  // (field_chargeden is not the half step's: asking for it rebuilds)
      s.adopt_current = true;
      set(Seq::HalfPair, Owed::AdoptHalfField);
      return true;
    }
    if (s.seq == Seq::Push1 && pred_usable()) {  // predicted by the previous step's kernel: no marker pass
      add(Act::SaveStepStartField);
      if (split) {
        set_seq(Seq::Half);
        if (m.pred_kind == 2) {  // the six sums in charge2[0..5], zeros behind: the host's sum over ranks sums them
          add(Act::PredToCharge);
          s.charge_pending_pred = true;
        } else {
          add(Act::PredCombine);
        }
        add(Act::PredConsumed);
      } else {
        set(Seq::Half, Owed::Nothing);  // (a stale AdoptHalfField ends here)
        add(Act::SpanCollect);
        pred_to_chargeden(m.lazy_calls);
        add(Act::SpanEnd);
      }
      return true;
    }
    s.cd_kept_mode_only = false;  // a deposit follows: the whole vector again
    if (s.owed == Owed::AdoptHalfField) set_owed(Owed::Nothing);  // (left over by an inspection that settled a pair before its solve_field)
    return false;
  }
};

}  // namespace

PredPlan plan_pred_chargeden(const CallMoment &m, const StepCaps &k, bool defer) {
  PredPlan p;
  auto add = [&p](Act a) { p.act[p.n++] = a; };
  add(Act::PredConsumed);
  const bool multi = m.several_ranks;
  if (m.pred_kind == 2) {
    if (defer && !multi && k.dft_paths && m.tab_lds) {  // the sums' combination, chargeden and the solve in the launch of
      p.owed = Owed::PredSums;                          // the solve_field that follows
    } else if (!multi) {
      add(Act::PredChargeden);
    } else {
      add(Act::PredToCharge);
      add(Act::PredReduce);
      add(Act::PredChargedenSummed);
    }
    return p;
  }
  if (defer && !multi && k.dft_paths && k.modes_fit_field_kernel) {  // all of it in the launch of the solve_field that follows
    p.owed = Owed::PredTiles;
    return p;
  }
  add(Act::PredCombine);
  if (multi) add(Act::PredReduce);
  if (defer) p.owed = Owed::Scale;
  else add(Act::Chargeden);
  return p;
}

CallPlan plan_call(const CallState &s0, const CallMoment &m, const StepCaps &k, Call call) {
  Builder b{s0, m, k, CallPlan{}};
  CallState &s = b.s;
  switch (call) {
    case Call::Push1:
    case Call::Push2: {
      const int irk = call == Call::Push1 ? 1 : 2;
      if (!b.require_loaded_keep_lazy()) break;
      if (irk == 1 && s.seq == Seq::Clean && lazy_ok(k, m.optimize_due_any)) {
        b.set_seq(Seq::Push1);
      } else if (irk == 2 && lz_of(s.seq) == LZ_HALF) {
        b.set_seq(push2_noted(s.seq));
      } else {
        b.materialize();
        b.add(irk == 1 ? Act::PushEager1 : Act::PushEager2);
      }
      s.call_phase = irk == 1 ? 1 : 4;  // a push opens its sub-step wherever the host stood
      break;
    }
    case Call::CollectCharge: {
      if (!b.require_loaded_keep_lazy()) break;
      b.phase_collect();
      b.cd_version();
      if (b.collect_opening(false)) break;
      // a whole-step kernel run for a noted push is booked under "push particle"; "collect charge" then covers the
      // reduction and scaling only
      const bool noted = lz_of(s.seq) == LZ_PUSH1 || lz_of(s.seq) == LZ_PUSH2;
      if (noted) b.deposit_or_step();
      b.add(Act::SpanCollect);
      if (!noted) b.deposit_or_step();
      if (m.charge_sum == 1) b.add(Act::FxSettle);  // exact sums over ranks, into the species accumulators: the one-rank path follows
      if (m.fp64_rank_sum) b.add(Act::ReduceCharge);
      if (m.lazy_calls) b.set_owed(m.fp64_rank_sum ? Owed::Scale : Owed::SumScale);  // the rest: in the launch of the solve_field that follows
      else b.add(m.fp64_rank_sum ? Act::Chargeden : Act::ChargedenSum);
      b.add(Act::SpanEnd);
      break;
    }
    case Call::ChargeLocal:
      if (m.charge_sum == 1) {
        b.refuse(Refusal::WantsExactLocal);
        break;
      }
      if (!b.require_loaded_keep_lazy()) break;
      if (!b.collect_opening(true)) {
        b.deposit_or_step();
        b.add(Act::ChargeLocal);
      }
      s.charge_pending = true;
      break;
    case Call::ChargeReduced:
      if (m.charge_sum == 1) b.refuse(Refusal::WantsExactReduced);
      else if (!s.charge_pending) b.refuse(Refusal::ReducedWithoutLocal);
      if (b.refused()) break;
      s.charge_pending = false;
      b.phase_collect();
      b.cd_version();
      if (s.charge_pending_pred) {  // what came back are the summed prediction sums
        s.charge_pending_pred = false;
        s.cd_kept_mode_only = true;
        b.add(Act::PredChargedenSummed);
      } else if (m.lazy_calls) {
        b.set_owed(Owed::Scale);
      } else {
        b.add(Act::Chargeden);
      }
      break;
    case Call::ChargeLocalExact:
      if (m.charge_sum != 1) {
        b.refuse(Refusal::NeedsExactSum);
        break;
      }
      if (!b.require_loaded_keep_lazy()) break;
      s.cd_kept_mode_only = false;
      b.deposit_or_step();
      break;
    case Call::ChargeExactHandedOut:  // (the limbs have reached the host and none was left out: only then is a charge pending)
      s.charge_pending = true;
      break;
    case Call::ChargeReducedExact:
      if (m.charge_sum != 1) b.refuse(Refusal::NeedsExactSum);
      else if (!s.charge_pending) b.refuse(Refusal::ReducedWithoutLocal);
      if (b.refused()) break;
      s.charge_pending = false;
      b.phase_collect();
      b.cd_version();
      b.add(Act::FxToRho);
      if (m.lazy_calls) b.set_owed(Owed::SumScale);
      else b.add(Act::ChargedenSum);
      break;
    case Call::SolveField: {
      if (s.seq == Seq::HalfPair) {  // the half-step field is solved already (the pair below): nothing to launch
        b.set(Seq::HalfPairSolved, Owed::Nothing);
        b.add(Act::CallPairSkip);
        b.add(Act::FieldWrittenBySolve);  // from now on field_electric IS the half-step field, as far as anybody can tell
      } else {
        b.settle_half_pair();
        if (lz_of(s.seq) == LZ_PUSH1 || lz_of(s.seq) == LZ_PUSH2) b.materialize();  // a noted push has to see the field of its own moment
        b.add(Act::SpanField);
        Owed pending = s.owed;  // what collect_charge left to this launch
        b.set_owed(Owed::Nothing);
        if (pending == Owed::AdoptHalfField && !s.adopt_current) pending = Owed::Nothing;  // (made for a charge density since overwritten: a safety net)
        // One rank, behind the collect_charge of push(2) whose kernel has predicted the next half-step charge: BOTH fields
        // in one launch -- the next step's push(1), collect_charge, solve_field then launch nothing
        if (pending == Owed::SumScale && k.pair_in_solve_field && s.seq == Seq::Clean && b.pred_usable()) {
          b.add(Act::SolvePair);
          b.add(Act::FieldWrittenBySolve);
          b.add(Act::PredConsumed);
          b.add(Act::MarkEhCurrent);
        } else {
          if (pending == Owed::AdoptHalfField) {  // (the fast path was left by an inspection in between: the field is adopted by copying)
            b.add(Act::AdoptHalfField);
          } else if (pending == Owed::PredTiles && k.dft_paths) {
            b.add(Act::SolvePredTiles);
          } else if (pending == Owed::PredSums && k.dft_paths) {
            b.add(Act::SolvePredSums);
          } else {
            if (pending == Owed::PredSums) b.add(Act::PredChargeden);
            if (pending == Owed::PredTiles) b.add(Act::PredCombine);
            b.add(Act::SolvePlain, (pending == Owed::SumScale ? 1 : 0) | ((pending == Owed::Nothing || pending == Owed::PredSums) ? 2 : 0));
          }
          b.add(Act::FieldWrittenBySolve);
        }
        b.add(Act::SpanEnd);
      }
      s.e_step_start = false;  // (every writer writes the whole of field_electric)
      if (s.call_phase == 2) s.call_phase = 3;  // (only a solve_field that was served moves the record on)
      else if (s.call_phase == 5) s.call_phase = 0;
      break;
    }
    case Call::Markers:
      b.require_loaded();
      break;
    case Call::ReadMarkers:  // (no refusal of its own: before the first load nothing is noted)
      b.materialize();
      break;
    case Call::WholeSteps:
    case Call::Substep1:
    case Call::Substep2:
      if (!b.require_loaded()) break;
      s.cd_kept_mode_only = false;  // every step and sub-step ends with a deposit of its own
      b.cd_version();
      s.call_phase = call == Call::Substep1 ? 3 : 0;  // (push, collect_charge and solve_field of the sub-step in one)
      break;
    case Call::ReadField:
      b.settle_field_view();
      break;
    case Call::OutputAll:
    case Call::OutputAllCd:
      if (!b.require_loaded()) break;
      [[fallthrough]];
    case Call::GetField:
    case Call::GetFieldCd:
      b.settle_field_view();
      b.materialize_cd();
      if ((call == Call::GetFieldCd || call == Call::OutputAllCd) && s.cd_kept_mode_only) b.rebuild_half_step_chargeden();
      break;
    case Call::WriteElectric:
      b.settle_step_start_field();  // (the kept modes stay the half step's, as after eager calls)
      b.settle_half_pair();         // (d_E0 keeps the step-start field a noted push(1) saw)
      if (lz_of(s.seq) == LZ_PUSH1 || lz_of(s.seq) == LZ_PUSH2) b.materialize();
      break;
    case Call::WriteChargeden:
      b.materialize_cd();  // pending deposits are consumed, then overwritten
      // a half-step field waiting to be adopted, or adopted as far as the host can tell but not yet copied: memory first
      // becomes what the eager calls leave -- the adoption writes field_chargeden too --, then the host's vector rules
      b.settle_half_pair();
      if (s.owed == Owed::AdoptHalfField) b.set_owed(Owed::Nothing);
      b.cd_version();
      s.cd_kept_mode_only = false;
      break;
    case Call::ReplaceMarkers:
      b.materialize_cd();  // deposits of the old markers are consumed, not mixed with the new ones
      // a half-step field waiting to be adopted: field_chargeden becomes the half-step charge density the eager
      // collect_charge left (markers still there)
      if (s.owed == Owed::AdoptHalfField) b.rebuild_half_step_chargeden();
      b.set(Seq::Clean, Owed::Nothing);  // a noted push of markers that are about to be replaced is void
      s.call_phase = 0;                  // (new markers: between time steps)
      break;
    case Call::UploadMarkers:
      b.materialize_cd();  // (first: what collect_charge left pending is settled before the sequence is left)
      if (m.loaded) b.materialize();
      s.call_phase = 0;
      break;
    case Call::SwitchField:
      // a half-step field of the OTHER solver or transform waits to be adopted: the half-step charge is deposited for real instead
      if (s.owed == Owed::AdoptHalfField && m.field_differs) {
        b.rebuild_half_step_chargeden();
        b.set_owed(Owed::Nothing);
      }
      break;
    case Call::BetweenSteps:
      if (s.seq != Seq::Clean || s.owed != Owed::Nothing || s.charge_pending) b.refuse(Refusal::NotBetweenSteps);
      break;
    case Call::Checkpoint:
      if (!m.loaded) b.refuse(Refusal::NotLoaded);
      else if (s.charge_pending) b.refuse(Refusal::CheckpointChargeWaiting);
      else if (lz_of(s.seq) != LZ_CLEAN) b.refuse(Refusal::CheckpointPushNoted);
      else if (s.call_phase != 0) b.refuse(Refusal::CheckpointInsideStep);  // (eager call sites note no push, and behind the second collect_charge nothing is noted either)
      if (b.refused()) break;
      b.settle_step_start_field();
      b.materialize_cd();
      if (s.cd_kept_mode_only && !b.refused()) {
        b.p.refusal = Refusal::CheckpointKeptMode;
        b.p.refused_after = true;
      }
      break;
    default:
      b.refuse(Refusal::IllegalState);
      break;
  }
  if (s.owed != Owed::AdoptHalfField) s.adopt_current = false;
  if (b.refused() && !b.p.refused_after) {  // nothing happens
    b.p.n = 0;
    b.p.next = s0;
  } else {
    b.p.next = s;
  }
  return b.p;
}

const char *call_state_invariants(const CallState &s, const CallMoment &m, const StepCaps &k) {
#define INVARIANT(cond) \
  if (!(cond)) return #cond
  const bool one_rank = !m.several_ranks;
  INVARIANT(s.seq < Seq::N && s.owed < Owed::N && kCallStateLegal[static_cast<int>(s.seq)][static_cast<int>(s.owed)]);
  INVARIANT(s.seq == Seq::Clean || (m.lazy_calls && m.loaded));  // a push is only noted by the lazy call sites
  INVARIANT(s.owed == Owed::Nothing || m.lazy_calls);
  INVARIANT(s.owed < Owed::SumScale || one_rank || m.charge_sum == 1);  // species sum / prediction left to solve_field: one rank
                                                                        // (or exact sums, already summed over ranks)
  // kind 1 of the charge sum: no tiles, sums or half-step field owed
  INVARIANT(m.charge_sum == 0 || (s.owed != Owed::PredTiles && s.owed != Owed::PredSums && s.owed != Owed::AdoptHalfField && !pair_of(s.seq)));
  INVARIANT(s.owed != Owed::PredTiles || m.pred_kind == 1);
  INVARIANT((s.owed != Owed::PredSums && s.owed != Owed::AdoptHalfField && !pair_of(s.seq)) || k.six_sums_one_mode);
  INVARIANT(!pair_of(s.seq) || m.call_pair);
  INVARIANT(!s.cd_kept_mode_only || m.pred_kind == 2);
  // an owed adoption is current: made for the field_chargeden the eager calls hold now (and, by kCallStateLegal, while the
  // markers still stand at the half step)
  INVARIANT(s.owed != Owed::AdoptHalfField || s.adopt_current);
  INVARIANT(!s.e_step_start || (s.seq == Seq::Clean && s.eh_modes == 2));  // (the half-step field: d_Eh / d_mode_h)
  // the call record: a noted push lies inside a time step (checkpoint_write goes by the record alone)
  INVARIANT(s.call_phase >= 0 && s.call_phase <= 5);
  INVARIANT(lz_of(s.seq) == LZ_CLEAN || s.call_phase != 0);
  INVARIANT(s.eh_modes >= 0 && s.eh_modes <= 2);
  INVARIANT(!s.charge_pending_pred || s.charge_pending);
#undef INVARIANT
  return nullptr;
}

const char *call_name(Call c) {
  static const char *const names[] = {"push1", "push2", "collect_charge", "charge_local", "charge_reduced", "charge_local_exact",
                                      "charge_exact_handed_out", "charge_reduced_exact", "solve_field", "markers", "read_markers",
                                      "whole_steps", "substep1", "substep2", "read_field", "get_field", "get_field_cd", "output_all",
                                      "output_all_cd", "write_electric", "write_chargeden", "replace_markers", "upload_markers",
                                      "switch_field", "between_steps", "checkpoint"};
  static_assert(sizeof names / sizeof *names == static_cast<int>(Call::N), "a name per kind of call");
  return c < Call::N ? names[static_cast<int>(c)] : "?";
}

}  // namespace pic1dp
