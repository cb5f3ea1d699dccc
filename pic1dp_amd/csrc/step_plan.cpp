// step_plan.cpp -- the decisions of the step path (step_plan.hpp): arithmetic and conditions only
#include "step_plan.hpp"

#include <algorithm>
#include <cstdio>

#include "field_lds.hpp"

namespace pic1dp {

// the one-pass kernels (k_step_one, k_step_one<PRIV>, k_step_sums)
static PredLaunch pred_launch(const StepFacts &f, const StepCaps &k, int64_t np) {
  return pred_launch(f.pol, f.in->nx, f.in->nmode, np, k.priv, f.plan->pred_kind, k.exp_bearing);
}

StepCaps step_caps(const StepFacts &f) {
  const pic1dp_input &in = *f.in;
  const ContextPlan &plan = *f.plan;
  const Settings &cfg = *f.cfg;
  StepCaps k{};
  k.dft_paths = f.field_solver == 0 && f.field_transform == 0;
  k.six_sums_one_mode = plan.pred_kind == 2 && in.nmode == 1;
  k.modes_fit_field_kernel = 2 * in.nmode <= FIELD_THREADS;
  k.exp_bearing = in.deltaf && (in.iptcldist == 2 || in.iptcldist == 3);
  k.step_recompute_ok = f.step_mode == 0 && step_lds_bytes(in.nx, true, f.charge_sum == 1) <= PARTICLE_LDS_CAP;
  k.predict_capable = f.charge_sum == 0 && cfg.predict && plan.pred_kind != 0 && f.has_pred && k.dft_paths && k.step_recompute_ok;
  k.diag_in_step = f.charge_sum == 0 && f.diag_sum == 0 && (f.fuse_output == 2 || (f.fuse_output == 1 && !k.predict_capable));
  k.priv = plan.pred_kind == 2 && plan.pred_private && f.pol.threads_req <= 0;
  k.lazy_calls_ok = cfg.lazy_calls && k.step_recompute_ok;
  k.pair_serves_collect = cfg.call_pair && cfg.lazy_calls && !f.several_ranks && k.predict_capable && k.six_sums_one_mode;
  k.pair_in_solve_field = cfg.call_pair && cfg.lazy_calls && k.dft_paths && k.predict_capable && k.six_sums_one_mode;
  if (cfg.fuse_solve && !f.several_ranks && k.six_sums_one_mode && k.dft_paths && f.field_npe <= 32 && k.predict_capable) {
    // the length that counts is the chain's cost in terms: a third with the sums through the matrix unit (one-rank order)
    const int chain_terms = (f.field_npe == 1 && f.chain_mfma) ? in.nx / 3 : in.nx / std::max(1, f.field_npe);
    if (cfg.fuse_solve == 2 || chain_terms <= 1024)
      for (int s = 0; s < in.nspecies; ++s) {  // the first species launched carries the solve
        if (f.np[s] <= 0) continue;
        k.fuse_capable = fits_fused_solve(pred_launch(f, k, f.np[s]));
        break;
      }
  }
  return k;
}

// a species with general divisor constants and an exp-bearing f0 is FP64-issue-bound: its -f0'/f0 at the step-start
// velocity goes from k_step_half to k_step_full through memory (8 B per marker) instead of being evaluated twice.
// Measured at 1e8 markers (tools/ab_pipe_carry.sh): bump-on-tail with T = 1.3, T2 = 0.7, m = 1.1 8.9e10 -> 9.85e10
// updates/s; two-stream2 (one division fewer per exp pair) 1.05e11 either way, so only bump-on-tail carries.
// PIC1DP_CARRY=0 switches it off, 2 also carries for two-stream2.
// One pass per step: -f0'/f0 at the new velocity is what the NEXT step's recomputation of the half-step state needs: it
// goes there through memory (16 B per marker and step; k_step_one 1.45 -> 1.33 ms at 1e8 markers, tools/ab_pred.sh) -- only
// where it costs something: two-stream2 and bump-on-tail (two exp and a division).  With the one-exp form
// (device_math.hpp) an evaluation costs about what its carry traffic costs (profiles/r03/experiments/ab_one_exp.log):
// evaluated again; PIC1DP_CARRY=1 / 0 insists either way.
static Carry carry_of(const StepFacts &f, const StepCaps &k, int s, bool pred) {
  const pic1dp_input &in = *f.in;
  const int carry = f.cfg->carry;
  if (!pred) {
    const bool carry2 = carry != 0 && in.deltaf && !f.pow2[s] && !f.one_exp[s] && (in.iptcldist == 3 || (carry == 2 && in.iptcldist == 2));
    return carry2 ? Carry::HalfToFull : Carry::None;
  }
  const bool carry_one = carry < 0 ? (f.one_exp[s] ? kCarryOneExpDefault : true) : carry > 0;
  return k.exp_bearing && carry_one ? Carry::OnePass : Carry::None;
}

MarkerPlan plan_markers(const StepFacts &f, const StepCaps &k, bool full, bool diag, bool pred, bool tail_ok, int eh_modes,
                        int nt_force) {
  const pic1dp_input &in = *f.in;
  const int pred_kind = f.plan->pred_kind;
  const bool exact = f.charge_sum == 1;
  MarkerPlan pl{};
  if (pred && (!full || diag || !k.predict_capable)) pred = false;
  pl.priv = k.priv;
  if (pred && pred_kind == 2 && !pl.priv && eh_modes == 0) pred = false;  // k_step_sums forms Eh from its kept mode
  pl.pred = pred;
  // the diagnostics of output_all inside k_step_full: when asked for, and the LDS holds them
  if (diag) {
    const size_t need = step_lds_bytes(in.nx, true) + step_diag_lds_bytes(in.nx, in.nx_opd, in.nv_opd);
    if (!full || in.nx_opd < 1 || in.nv_opd < 2 || need > PARTICLE_LDS_CAP) diag = false;
  }
  pl.diag = diag;
  // several ranks, the six sums of one kept mode, the mode-filter solver: the packing of this rank's charge for the sum
  // over ranks rides in the tail of the last marker launch (RCCL: one all-reduce follows; exchange: posted at once)
  pl.tail_species = -1;
  if (tail_ok && pred && f.cfg->tail_on && k.six_sums_one_mode && k.dft_paths && f.several_ranks) {
    pl.tail_mode = f.xchg_active ? 2 : (f.has_comm ? 1 : 0);
    for (int s = 0; s < in.nspecies; ++s)
      if (f.np[s] > 0) pl.tail_species = s;
    if (pl.tail_species < 0) pl.tail_mode = 0;
  }
  // x, v, w, p of all species against the 256 MiB Infinity Cache
  int64_t np_all = 0;
  for (int s = 0; s < in.nspecies; ++s) np_all += f.np[s];
  double state_bytes = 0.0;
  for (int s = 0; s < in.nspecies; ++s) state_bytes += 32.0 * static_cast<double>(f.np[s]);
  pl.stream_nt = state_bytes > (full ? f.cfg->nt_threshold_full : f.cfg->nt_threshold_half) ? 1 : 0;
  if (nt_force == 0) pl.stream_nt = 0;
  if (nt_force == 1) pl.stream_nt = 1;
  if (nt_force == 2) pl.stream_nt = full ? 0 : 1;
  if (nt_force == 3) pl.stream_nt = full ? 1 : 0;
  pl.tag = pred ? pic1dp_host::kTagStepOne : (full ? pic1dp_host::kTagStepFull : pic1dp_host::kTagStepHalf);
  pl.rd = 8.0 * (3 + (in.deltaf ? 1 : 0));
  pl.wr = full ? 8.0 * (1 + (in.linear ? 0 : 1) + (in.deltaf ? 1 : 0)) : 0.0;
  pl.solve_species = -1;
  for (int s = 0; s < in.nspecies; ++s) {
    SpeciesLaunch &L = pl.sp[s];
    if (f.np[s] <= 0) continue;
    L.launched = true;
    // the drawn chunk tail of every whole-step kernel: half a workgroup's chunks, all of them for k_step_full (two passes
    // per step at 1e8 markers: 0.913 -> 0.898 ms with 16/16 against 8/16, profiles/r05/experiments/ab_dyn_tail_other.log)
    L.dyn_tail = (full && !pred) ? f.cfg->dyn_tail_full : f.cfg->dyn_tail;
    L.lc = step_launch(f.pol, in.nx, f.np[s], full, exact);
    L.carry = carry_of(f, k, s, pred);
    if (pred) {
      L.family = pred_kind == 2 ? (pl.priv ? StepFamily::PrivateSums : StepFamily::Sums) : StepFamily::Tiles;
      const PredLaunch p = pred_launch(f, k, f.np[s]);
      L.lc = p.lc;
      // a non-temporal launch keeps the head of the slab in the Infinity Cache (launch_policy.hpp)
      L.plain_chunks = stream_plain_chunks(np_all, f.np[s], pl.stream_nt != 0);
      if (pl.solve_species < 0) pl.solve_species = s, pl.solve_fits = fits_fused_solve(p), pl.solve_threads = p.lc.threads;
      L.tail = pl.tail_mode != 0 && s == pl.tail_species;
    }
    if (pl.diag) L.lc = step_diag_launch(f.pol, in.nx, f.np[s], exact, in.nx_opd, in.nv_opd);
    std::snprintf(L.name, sizeof L.name, "%s%s%s",
                  pred ? (pred_kind == 2 ? (pl.priv ? "k_step_one<sums>" : "k_step_sums") : "k_step_one")
                       : (full ? (pl.diag ? "k_step_full<DIAG>" : "k_step_full") : "k_step_half"),
                  exact ? "<EXACT>" : "", f.one_exp[s] && in.deltaf ? " (one-exp -f0'/f0)" : "");
  }
  return pl;
}

SolvePlan plan_solve(const StepFacts &f, const StepCaps &k, bool pred_fresh, int tail_done, bool into_E) {
  SolvePlan sp{};
  const bool multi = f.charge_sum == 0 && f.several_ranks;  // (kind 1: summed over ranks as integers already -- the one-rank path)
  const bool fused_xchg = multi && f.xchg_active && k.dft_paths;  // exchange inside the solve's launch
  // RCCL path of a one-pass step: everything the two charge sums of the step need in one all-reduce
  const bool will_pack = pred_fresh && multi && !fused_xchg && f.has_comm && !f.xchg_active && k.dft_paths &&
                         k.modes_fit_field_kernel && into_E;
  if (tail_done == 1 && !will_pack) sp.refused = 1;
  else if (tail_done == 2 && !(fused_xchg && pred_fresh)) sp.refused = 2;
  if (sp.refused) return sp;
  sp.pack_reduce = will_pack;
  sp.pack_first = will_pack && tail_done != 1;  // the species sum and the packing are collect_charge's share of the step
  sp.reduce_first = !will_pack && multi && !fused_xchg;
  sp.with_local = !multi;
  // one-pass step on one rank or with the exchange: both fields (the new state's, and the next step's half-step field
  // from the prediction) in ONE launch
  const bool pair = pred_fresh && (!multi || fused_xchg || will_pack) && k.dft_paths && k.modes_fit_field_kernel && into_E;
  if (pair)
    sp.launch = will_pack ? SolveLaunch::PairPacked
                          : (fused_xchg ? (tail_done == 2 ? SolveLaunch::PairPosted : SolveLaunch::PairExchange) : SolveLaunch::PairAccumulators);
  else
    sp.launch = fused_xchg ? SolveLaunch::Exchange : SolveLaunch::Plain;
  return sp;
}

WholeStepPlan plan_whole_step(const StepFacts &, const StepCaps &k, const StepMoment &m) {
  WholeStepPlan w{};
  // a step in which a marker optimisation is due goes through the sub-steps
  if (!k.step_recompute_ok || m.optimize_now) {
    w.substeps = true;
    w.finish_pending = m.pending;
    return w;
  }
  // the host can only call output_all after the last step of this call
  w.diag = k.diag_in_step && m.steps_left == 1 && m.output_now;
  w.pred = k.predict_capable && !w.diag;
  // the previous step left its solve to this step's marker launch (one launch per step, kernels.hpp FusedSolve)
  w.fused_in = m.pending && w.pred && k.fuse_capable;
  w.finish_pending = m.pending && !w.fused_in;
  // Eh of this step: predicted by the previous step's kernel (one pass per step), or from a first-sub-step pass
  w.adopt_eh = !w.fused_in && k.predict_capable && m.have_eh;
  w.half_pass = !w.fused_in && !w.adopt_eh;
  w.half_eh_modes = k.dft_paths ? 1 : 0;  // that pass's solve leaves the kept modes in fa.mode_re / mode_im
  // may the NEXT step's launch take this step's solve?  Only if that step will be an ordinary predicted one (the step
  // after an output, an optimisation step or the last step of the call need the field in memory first)
  if (w.pred && m.steps_left > 1 && k.fuse_capable) {
    const bool next_diag = k.diag_in_step && m.steps_left == 2 && m.output_next;
    w.fuse_out = !next_diag && !m.optimize_next;
  }
  return w;
}

}  // namespace pic1dp
