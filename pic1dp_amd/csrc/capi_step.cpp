// capi_step.cpp -- the ACTIONS of the hot path behind the C ABI of include/pic1dp_hip.h: the three call sites (push /
// collect_charge / solve_field), pic1dp_hip_step, the prediction of the half-step charge, the solve inside the marker launch,
// the split-phase deposit.  What a step launches is DECIDED in step_plan.cpp, what a call of the call sites' lazy state
// machine enqueues and which state follows in call_plan.cpp (both pure, pinned on the host): here are the wiring (pointers,
// versions, counters, spans), the bridges from the context to the plans (facts_of; call_state_of, call_moment_of) and the one
// executor that walks a call's plan through the enqueue helpers and stores the state (run_call).
// Launch shapes: launch_policy.cpp; the other units: ctx.hpp.  In order of dependency: the bridges and the currency
// relations, the marker launches, prediction and solve, pic1dp_hip_step, the call sites' executor and entry points, the
// split-phase deposit, pic1dp_hip_check_state.
// (the entry points are declared extern "C" in include/pic1dp_hip.h; their definitions here inherit that linkage)
#include <optional>

#include "ctx.hpp"

// ---------------------------------------------------------------------------
// which path: the plan (step_plan.hpp) and what it is asked with
// ---------------------------------------------------------------------------
// launch shapes (launch_policy.hpp) for this context
static LaunchPolicy policy_of(const pic1dp_ctx *c) { return LaunchPolicy{c->num_cu, c->threads_req, c->bpc_req, c->cfg.osub_req}; }
// THE bridge from the context to the plan: the facts, and the predicates that follow from them.  Taken once per API call
// (nothing inside a call changes them but an optimisation event: pic1dp_hip_step takes them again behind one)
struct Step {
  StepFacts f;
  StepCaps k;
};
static Step facts_of(const pic1dp_ctx *c) {
  Step s{};
  StepFacts &f = s.f;
  f.in = &c->in, f.plan = &c->plan, f.cfg = &c->cfg;
  f.pol = policy_of(c);
  f.charge_sum = c->charge_sum, f.diag_sum = c->diag_sum, f.fuse_output = c->fuse_output;
  f.step_mode = c->step_mode, f.field_solver = c->field_solver, f.field_transform = c->field_transform;
  f.several_ranks = several_ranks(c), f.xchg_active = xchg_active(c), f.has_comm = c->comm != nullptr;
  f.field_npe = c->fa.npe, f.chain_mfma = c->fa.chain_mfma;
  f.has_pred = c->d_pred != nullptr;
  for (int i = 0; i < c->in.nspecies; ++i) f.np[i] = c->sp[i].np, f.pow2[i] = c->sp[i].sc.pow2, f.one_exp[i] = c->sp[i].sc.one_exp;
  s.k = step_caps(f);
  return s;
}
// the currency relations between the versions: the prediction in d_pred belongs to the markers as they are ...
static bool pred_fresh(const pic1dp_ctx *c) { return c->pred_version != 0 && c->pred_version == c->state_version; }
// ... d_Ehn is the half-step field of the markers and the field as they are
static bool eh_current(const pic1dp_ctx *c) { return c->eh_version == c->state_version && c->eh_field_version == c->field_version; }
static void mark_eh_current(pic1dp_ctx *c) {
  c->eh_version = c->state_version;
  c->eh_field_version = c->field_version;
}
static LaunchCfg particle_launch(const pic1dp_ctx *c, int64_t np, bool with_E, bool with_rho, bool exact = false) {
  return particle_launch(policy_of(c), c->in.nx, np, with_E, with_rho, exact);
}
// does output_all follow the step that is being taken?  (src/pic1dp.F90:98-107 evaluated one step ahead)
static bool output_follows_at(const pic1dp_ctx *c, int32_t itime0, double time0) {  // (counters at the start of the step)
  const pic1dp_input &in = c->in;
  if (!(in.output_interval > 0.0)) return false;
  const double t = time0 + in.dt;
  if (itime0 + 1 >= in.ntime_max || t + kSqrtEps >= in.time_max) return true;
  return std::fmod(t + kSqrtEps, in.output_interval) < std::fmod(t + kSqrtEps - in.dt, in.output_interval);
}
static bool output_follows(const pic1dp_ctx *c) { return output_follows_at(c, c->itime, c->time); }

// the accumulator set the marker kernels deposit into from now on (d_rho_all / d_pred_all hold three)
static void use_accumulators(pic1dp_ctx *c, int idx) {
  c->acc_idx = idx;
  c->d_rho_sp = c->d_rho_all + static_cast<size_t>(idx) * c->plan.rho_set_doubles;
  for (int s = 0; s < c->in.nspecies; ++s) c->sp[s].rho = c->d_rho_sp + static_cast<size_t>(s) * c->in.nx;
  c->fa.rho_sp = c->d_rho_sp;
  if (c->d_pred_all) c->d_pred = c->d_pred_all + static_cast<size_t>(idx) * c->plan.pred_set_doubles;
}

// the prediction in d_pred describes the next first sub-step of the markers as they are, and the kept
// modes describe the field as it is
static bool pred_usable(const pic1dp_ctx *c, const Step &s) {
  return pred_fresh(c) && c->modes_field_version == c->field_version && s.k.predict_capable;
}

// THE bridge from the context to the call sites' plan (call_plan.hpp): what the machine remembers ...
static CallState call_state_of(const pic1dp_ctx *c) {
  CallState s;
  s.seq = c->seq, s.owed = c->owed;
  s.e_step_start = c->e_step_start, s.cd_kept_mode_only = c->cd_kept_mode_only;
  s.adopt_current = c->owed == Owed::AdoptHalfField && c->adopt_cd_version == c->cd_version;
  s.charge_pending = c->charge_pending, s.charge_pending_pred = c->charge_pending_pred;
  s.call_phase = static_cast<int8_t>(c->call_phase), s.eh_modes = static_cast<int8_t>(c->eh_modes);
  return s;
}
// ... and what a decision looks at besides (the clock's two questions only for the calls that ask them)
static CallMoment call_moment_of(const pic1dp_ctx *c, const Step &s, Call call, bool field_differs = false) {
  CallMoment m;
  m.lazy_calls = c->cfg.lazy_calls != 0, m.call_pair = c->cfg.call_pair != 0, m.loaded = c->loaded;
  m.several_ranks = several_ranks(c), m.fp64_rank_sum = fp64_rank_sum(c);
  m.charge_sum = c->charge_sum, m.pred_kind = c->plan.pred_kind, m.tab_lds = c->fa.tab_lds != 0;
  m.field_differs = field_differs;
  m.pred_usable = pred_usable(c, s), m.eh_current = eh_current(c);
  m.modes_current = c->modes_field_version == c->field_version;
  m.optimize_due_any = call == Call::Push1 && optimize_due_any(c);
  m.output_follows = (call == Call::CollectCharge || call == Call::ChargeLocal || call == Call::ChargeLocalExact) && output_follows(c);
  return m;
}

// both fields in one launch: what every pair solve is handed
// (cd_h: the tiles' scratch; with the six sums the kept mode's content of the half-step charge density -- what the call
// sites adopt into field_chargeden when the host's next push(1), collect_charge, solve_field are served from this solve,
// which they are after a step() as after the call sites' own pair: round 6's fuzz campaign found the stale copy)
static PairArgs pair_args(const pic1dp_ctx *c) {
  return PairArgs{c->d_pred, c->d_Ehn, c->d_mode_h, c->d_cd_h, nullptr, c->plan.pred_kind, c->pred_tab, 0};
}
// bookkeeping behind a pair solve: field_electric is the new state's field, d_Ehn / d_mode_h the next step's half-step field
static void pair_solved(pic1dp_ctx *c) {
  field_written(c, true);
  c->pred_version = 0;  // consumed
  mark_eh_current(c);
}
// d_E0 <- field_electric: the field a noted push(1) saw
static int save_step_start_field(pic1dp_ctx *c) {
  HIP_TRY(hipMemcpyAsync(c->d_E0, c->d_E, sizeof(double) * c->in.nx, hipMemcpyDeviceToDevice, c->st));
  return 0;
}
// the kept modes of field_electric <- those of the half-step field (d_mode_h)
static int adopt_half_modes(pic1dp_ctx *c) {
  const size_t nm = c->in.nmode;
  HIP_TRY(hipMemcpyAsync(c->fa.mode_re, c->d_mode_h, sizeof(double) * nm, hipMemcpyDeviceToDevice, c->st));
  HIP_TRY(hipMemcpyAsync(c->fa.mode_im, c->d_mode_h + nm, sizeof(double) * nm, hipMemcpyDeviceToDevice, c->st));
  return 0;
}

// ---------------------------------------------------------------------------
// marker launches
// ---------------------------------------------------------------------------
static PushArgs make_push_args(pic1dp_ctx *c, int isp, int irk, const double *E) {
  Species &S = c->sp[isp];
  PushArgs a{};
  a.src = S.set[c->cur];
  a.base = irk == 2 ? S.set[1 - c->cur] : S.set[c->cur];
  a.dst = S.set[1 - c->cur];
  a.p = S.p;
  a.E = E ? E : c->d_E;
  a.rho = S.rho;
  a.np = S.np;
  a.dt = irk == 1 ? 0.5 * c->in.dt : c->in.dt;  // src/pic1dp_interaction.F90:179,192
  a.g = c->grid;
  a.s = S.sc;
  a.iptcldist = c->in.iptcldist;
  a.deltaf = c->in.deltaf;
  a.linear = c->in.linear;
  a.irk = irk;
  a.fx = fx_args(c, isp);
  return a;
}

static int enqueue_deposit(pic1dp_ctx *c) {
  c->state_version++;  // the wrap is stored back into x
  for (int s = 0; s < c->in.nspecies; ++s) {
    Species &S = c->sp[s];
    if (S.np <= 0) continue;
    double *x = S.set[c->cur].x;
    const double *q = c->in.deltaf ? S.set[c->cur].w : S.p;  // :84-91
    const bool exact = c->charge_sum == 1;
    LaunchCfg lc = particle_launch(c, S.np, false, true, exact);
    {
      KernelBytes &kb = c->tm.kbytes[kTagDeposit];
      kb.rd = 16.0, kb.wr = 8.0, kb.carry = 0.0;  // x, q read; wrapped x written
      std::snprintf(kb.name, sizeof kb.name, "%s", exact ? "k_deposit<EXACT>" : "k_deposit");
    }
    Span ks(c->tm, kTagDeposit, c->tm.stats_on);
    HIP_TRY(launch_deposit(x, q, S.rho, fx_args(c, s), S.np, c->grid, lc, c->st));
    if (int rc = ks.end()) return rc;
  }
  return 0;
}

static int enqueue_push(pic1dp_ctx *c, int irk, bool fused, const double *E = nullptr) {
  if (int rc = ensure_second_set(c)) return rc;
  // kind 1 of the charge sum: where the E tile and the exact rho tile do not fit the LDS together (nx > 6780), the push
  // and the deposit run as two launches (same positions and contributions, hence the same integers)
  const bool exact = c->charge_sum == 1;
  const bool deposit_apart = fused && exact && particle_launch(c, 2, true, true, true).lds > PARTICLE_LDS_CAP;
  if (deposit_apart) fused = false;
  c->state_version++;
  for (int s = 0; s < c->in.nspecies; ++s) {
    PushArgs a = make_push_args(c, s, irk, E);
    if (a.np <= 0) continue;
    LaunchCfg lc = particle_launch(c, a.np, true, fused, exact);
    {  // irk 1 reads x, v, p (+ w); irk 2 also the RK base x (+ v) (+ w); both write x (+ v) (+ w)
      KernelBytes &kb = c->tm.kbytes[fused ? kTagFused : kTagPush];
      const double pushed = 8.0 * (1 + (c->in.linear ? 0 : 1) + (c->in.deltaf ? 1 : 0));
      kb.rd = 8.0 * (3 + (c->in.deltaf ? 1 : 0)) + (irk == 2 ? pushed : 0.0);
      kb.wr = pushed;
      kb.carry = 0.0;
      std::snprintf(kb.name, sizeof kb.name, "%s", fused ? (exact ? "k_push<FUSED, EXACT>" : "k_push<FUSED>") : "k_push");
    }
    Span tm(c->tm, PIC1DP_IWT_PUSH_PARTICLE, c->tm.timers_on);
    Span ks(c->tm, fused ? kTagFused : kTagPush, c->tm.stats_on);
    HIP_TRY(launch_push(a, fused, lc, c->st));
    if (int rc = ks.end()) return rc;
    if (int rc = tm.end()) return rc;
  }
  c->cur = 1 - c->cur;
  if (deposit_apart) return enqueue_deposit(c);
  return 0;
}

static int carry_buffer(pic1dp_ctx *c, Species &S) {
  if (!S.t2) HIP_TRY(c->mem.alloc(&S.t2, static_cast<size_t>(S.nalloc + 2)));
  return 0;
}

// -f0'/f0 through memory (Species::t2) instead of a second evaluation: from k_step_half to k_step_full of a step, or from
// one one-pass step to the next (which species carries: step_plan.cpp carry_of).  A launch may only load what an earlier
// one stored for these very markers
static int wire_carry(pic1dp_ctx *c, Species &S, StepArgsDev &a, bool full, Carry carry) {
  if (carry == Carry::None) return 0;
  if (int rc = carry_buffer(c, S)) return rc;
  const bool stored = S.t2_version == (full ? c->state_version - 1 : c->state_version);
  if (carry == Carry::HalfToFull) {
    if (!full || stored) a.t2 = S.t2;
    if (!full) S.t2_version = c->state_version;
    return 0;
  }
  a.t2 = S.t2;
  a.t2_mode = stored ? 2 : 1;
  S.t2_version = c->state_version;
  return 0;
}

// this launch's last workgroup packs (mode 1) or posts (mode 2) this rank's charge; c->tail_done tells solve_phase
static void wire_tail(pic1dp_ctx *c, StepTail &t, int tail_mode) {
  t.mode = tail_mode;
  t.ticket = c->d_ticket;
  t.rho_sp = c->fa.rho_sp;
  t.rho_copies = c->fa.rho_copies;
  t.rho_stride = c->fa.rho_stride;
  t.nspecies = c->in.nspecies;
  t.nx = c->in.nx;
  for (int k = 0; k < 8; ++k) t.Z[k] = c->fa.Z[k];
  t.sums = c->d_pred;
  t.pack = c->d_pack;
  if (tail_mode == 2) {
    c->tail_x = next_xchg_args(c);
    t.x = c->tail_x;
    t.x.ticks = nullptr;  // (the field launch's half of the exchange is the one the attribution times)
  }
  c->tail_done = tail_mode;
  c->cnt.tail_launches++;
}

// k_step_full<DIAG> of species s: its histograms and partial sums, what the collector has to know
static int wire_diag(pic1dp_ctx *c, int s, StepArgsDev &a, const LaunchCfg &lc) {
  const size_t ntot = dist_len(c->in);
  a.dg = dist_geom(c);
  a.dist_out = c->d_dist + ntot * s;
  a.dist_partial = diag_part_dev(c, s);
  HIP_TRY(hipMemsetAsync(a.dist_out, 0, sizeof(double) * ntot, c->st));
  // the histograms as 64-bit fixed-point sums where the diagnostics' own pass would take them so (capi_diag.cpp
  // diag_fx_bounds; a marker beyond the bounds: the collector repeats in doubles)
  double bp = 0.0, bw = 0.0;
  a.diag_fx = diag_fx_bounds(c, s, &bp, &bw) && make_dist_scale(a.np, lc.blocks, c->in.deltaf == 1, bp, bw, &a.dscale, lc.threads) ? 1 : 0;
  diag_note_pass(c, s, lc.blocks, a.diag_fx != 0, false);  // (the caller has bumped state_version for this step already)
  return 0;
}

// the marker launch of species s
static int launch_step_species(pic1dp_ctx *c, int s, bool full, const double *E0, const double *Eh, const MarkerPlan &pl) {
  Species &S = c->sp[s];
  const SpeciesLaunch &L = pl.sp[s];
  StepArgs sa{};
  sa.iptcldist = c->in.iptcldist;
  sa.deltaf = c->in.deltaf;
  sa.linear = c->in.linear;
  sa.family = L.family;
  StepArgsDev &a = sa.d;
  a.x = S.set[c->cur].x;
  a.v = S.set[c->cur].v;
  a.w = S.set[c->cur].w;
  a.p = S.p;
  a.E0 = E0;
  a.Eh = Eh;
  a.rho = S.rho;
  a.np = S.np;
  a.dt_half = 0.5 * c->in.dt;  // src/pic1dp_interaction.F90:179
  a.dt_full = c->in.dt;        // :192
  a.g = c->grid;
  a.s = S.sc;
  a.nt = pl.stream_nt;
  a.dyn_tail = L.dyn_tail;
  a.fx = fx_args(c, s);
  if (pl.pred && c->fuse_args.on) {  // this launch's prologue solves the previous step's field (first species launched)
    if (s != pl.solve_species || !pl.solve_fits)  // what fuse_capable promised (checked at the launch too)
      return fail(PIC1DP_ERR_STATE, "internal: fused field solve in a launch of %d threads", pl.solve_threads);
    a.fused = c->fuse_args;
    c->fuse_args.on = 0;
    c->cnt.fused_solves++;
  }
  if (int rc = wire_carry(c, S, a, full, L.carry)) return rc;
  if (pl.pred) {  // k_step_one: the full step + the prediction of the next first sub-step's charge
    const bool sums = c->plan.pred_kind == 2;
    a.tabA = c->d_tabA;
    a.tabB = c->d_tabB;
    a.pred = sums ? c->d_pred  // six sums, all species together (Z folded in)
                  : c->d_pred + static_cast<size_t>(s) * (1 + 2 * c->in.nmode) * c->in.nx;
    a.pred_nm = c->in.nmode;
    a.fxb = S.fxb;
    if (sums) {
      a.eh_re = c->eh_modes == 2 ? c->d_mode_h : c->fa.mode_re;
      a.eh_im = c->eh_modes == 2 ? c->d_mode_h + 1 : c->fa.mode_im;
    }
    a.plain_chunks = static_cast<int>(L.plain_chunks);
#ifdef PIC1DP_TUNING
    a.plain_every = 0;
    if (const char *e = tuning_env("PIC1DP_PLAIN_ROWS"))
      if (std::atoi(e) != 0 && a.plain_chunks > 0) {  // the same share of the state as whole rows, evenly through the sweep
        const int64_t stride = static_cast<int64_t>(L.lc.blocks) * L.lc.threads;
        const int64_t rows = ((S.np >> 1) + stride - 1) / stride;
        const int64_t plain_rows = std::max<int64_t>(1, static_cast<int64_t>(a.plain_chunks) * 64 / stride);
        a.plain_every = static_cast<int>(std::max<int64_t>(1, (rows + plain_rows - 1) / plain_rows));
      }
#endif
    if (L.tail && !a.fused.on) wire_tail(c, a.tail, pl.tail_mode);
  }
  if (pl.diag)
    if (int rc = wire_diag(c, s, a, L.lc)) return rc;
  {  // what this instantiation moves per marker (k_step_one's carry: 8 read when loaded + 8 written)
    KernelBytes &kb = c->tm.kbytes[pl.tag];
    kb.rd = pl.rd, kb.wr = pl.wr;
    kb.carry = a.t2 ? carry_bytes(L.carry, a.t2_mode == 2) : 0.0;
    std::snprintf(kb.name, sizeof kb.name, "%s%s", L.name, a.fused.on ? " + field solve" : "");
  }
  Span tm(c->tm, PIC1DP_IWT_PUSH_PARTICLE, c->tm.timers_on);
  Span ks(c->tm, pl.tag, c->tm.stats_on);
  HIP_TRY(launch_step(sa, full, L.lc, c->st));
  if (int rc = ks.end()) return rc;
  return tm.end();
}

// the particle kernel(s) of one sub-step of the whole-step path: E0 = field at the start of the step, Eh = field after
// the first sub-step (full only).
// full = true: the caller has bumped state_version for this step; the state the kernel READS is version - 1
// tail_ok (the step() path on several ranks): the last species' launch may pack / post this rank's charge in its tail
// (kernels.hpp StepTail) -- c->tail_done tells solve_phase what it did
static int step_particles(pic1dp_ctx *c, const Step &s, bool full, const double *E0, const double *Eh, bool diag = false,
                          bool pred = false, bool tail_ok = false) {
  c->tail_done = 0;
  const char *nt = tuning_env("PIC1DP_NT_FORCE");  // tuning build only, read per launch (tools/ab_nt.py)
  const MarkerPlan pl = plan_markers(s.f, s.k, full, diag, pred, tail_ok, c->eh_modes, nt ? std::atoi(nt) : -1);
  if (pl.pred && c->pred_version != 0)  // a prediction nobody used: the accumulators start from zero
    HIP_TRY(hipMemsetAsync(c->d_pred, 0, sizeof(double) * c->plan.pred_set_doubles, c->st));
  if (pl.diag)
    if (int rc = diag_buffers(c)) return rc;
  for (int i = 0; i < c->in.nspecies; ++i)
    if (pl.sp[i].launched)
      if (int rc = launch_step_species(c, i, full, E0, Eh, pl)) return rc;
  if (c->fuse_args.on) return fail(PIC1DP_ERR_STATE, "internal: a fused field solve found no marker launch to run in");
  if (pl.pred) c->pred_version = c->state_version;
  return 0;
}

// ---------------------------------------------------------------------------
// prediction and solve
// ---------------------------------------------------------------------------
// d_E has been written: by the mode-filter solve (the kept modes describe it) or by something else
void pic1dp_host::field_written(pic1dp_ctx *c, bool by_solve) {
  c->field_version++;
  if (by_solve && c->field_solver == 0) c->modes_field_version = c->field_version;
}

// field_solve_electric: the reference's mode-filter solve (its DFT by the dense tables, or by the FFT under
// field_transform 1), optionally followed by the finite-difference alternative overwriting E (field_solver = 1)
static int enqueue_field_solve(pic1dp_ctx *c, FieldArgs f, bool with_local, bool from_chargeden) {
  double *hist = f.history;
  if (c->field_solver == 1) f.history = nullptr;
  if (c->field_transform == 1)
    HIP_TRY(launch_field_fft(f, c->fft, with_local, from_chargeden, c->st));
  else
    HIP_TRY(launch_field_solve(f, with_local, from_chargeden, c->st));
  if (c->field_solver == 1)
    HIP_TRY(launch_field_fd(f.chargeden, f.E, hist, f.nx, f.lx, f.dnx, c->st));
  return 0;
}

// the local result of the prediction summed over ranks in d_charge
static int pred_reduce(pic1dp_ctx *c) {
  if (xchg_active(c)) {
    Span sp(c->tm, PIC1DP_IWT_MPIALLREDU, c->tm.timers_on);
    XchgArgs x = next_xchg_args(c);
    x.local_in_charge = 1;
    HIP_TRY(launch_charge_exchange(c->fa, x, c->st));
    return sp.end();
  }
  return allreduce_charge(c);
}

// one action of a plan (call_plan.hpp Act), through the helpers above.  f: the field arguments the charge-density and solve
// launches take -- c->fa at the call sites, a copy aimed at scratch vectors on the step path
static int enqueue_wrap_only(pic1dp_ctx *c);
static int adopt_half_field(pic1dp_ctx *c);
static int run_act(pic1dp_ctx *c, const Step &s, Act act, int arg, const FieldArgs &f) {
  const size_t nx = c->in.nx;
  switch (act) {
    case Act::SaveStepStartField: return save_step_start_field(c);
    case Act::AdoptHalfField: return adopt_half_field(c);
    case Act::AdoptHalfModes: return adopt_half_modes(c);
    case Act::CopyEhToE: HIP_TRY(hipMemcpyAsync(c->d_E, c->d_Eh, sizeof(double) * nx, hipMemcpyDeviceToDevice, c->st)); return 0;
    case Act::PushEager1: return enqueue_push(c, 1, false);
    case Act::PushEager1FromE0: return enqueue_push(c, 1, false, c->d_E0);
    case Act::PushEager2: return enqueue_push(c, 2, false);
    case Act::WrapOnly: return enqueue_wrap_only(c);
    case Act::Deposit: return enqueue_deposit(c);
    case Act::HalfPass: return step_particles(c, s, false, c->d_E, c->d_Eh);
    case Act::SwapEh: std::swap(c->d_Eh, c->d_Ehn); return 0;  // d_Eh: the half-step field of the step being taken
    case Act::FullPass:
      c->eh_modes = arg >> kFullEhModesShift;
      return step_particles(c, s, true, (arg & kFullE0Saved) ? c->d_E0 : c->d_E, (arg & kFullEhIsE) ? c->d_E : c->d_Eh,
                            (arg & kFullDiag) != 0, (arg & kFullPred) != 0);
    case Act::FxSettle: return fx_settle(c);
    case Act::ReduceCharge: return reduce_charge(c);
    case Act::Chargeden: HIP_TRY(launch_chargeden(f, false, c->st)); return 0;
    case Act::ChargedenSum: HIP_TRY(launch_chargeden(f, true, c->st)); return 0;
    case Act::PredChargeden: HIP_TRY(launch_pred_chargeden(f, c->pred_tab, c->d_pred, nullptr, c->st)); return 0;
    case Act::PredChargedenSummed: HIP_TRY(launch_pred_chargeden(f, c->pred_tab, nullptr, c->d_charge, c->st)); return 0;
    case Act::PredCombine: HIP_TRY(launch_pred_combine(c->fa, c->d_pred, c->in.nmode, c->st)); return 0;
    case Act::PredToCharge: HIP_TRY(launch_pred_to_charge(c->fa, c->d_pred, c->st)); return 0;
    case Act::PredReduce: return pred_reduce(c);
    case Act::ChargeLocal: HIP_TRY(launch_charge_local(c->fa, c->st)); return 0;
    case Act::FxToRho: HIP_TRY(launch_fx_to_rho(c->d_fx, c->fa.rho_sp, c->in.nspecies, c->in.nx, c->fx_q, c->st)); return 0;
    case Act::SolvePair: HIP_TRY(launch_field_solve_pair(f, pair_args(c), nullptr, c->st)); return 0;
    case Act::SolvePredTiles: HIP_TRY(launch_field_solve_pred(f, c->d_pred, c->in.nmode, c->st)); return 0;
    case Act::SolvePredSums: HIP_TRY(launch_field_solve_pred_sums(f, c->pred_tab, c->d_pred, c->st)); return 0;
    case Act::SolvePlain: return enqueue_field_solve(c, f, (arg & 1) != 0, (arg & 2) != 0);
    case Act::StateVersion: c->state_version++; return 0;
    case Act::CdVersion: c->cd_version++; return 0;
    case Act::FieldWrittenBySolve: field_written(c, true); return 0;
    case Act::CallPairSkip: c->cnt.call_pair_skips++; return 0;
    case Act::PredConsumed: c->pred_version = 0; return 0;  // the accumulators are zero again afterwards
    case Act::MarkEhCurrent: mark_eh_current(c); return 0;
    default: return fail(PIC1DP_ERR_STATE, "internal: action %d of a call plan has no executor", static_cast<int>(act));
  }
}

// step() path: Eh of the NEXT step from the prediction, right after the field of the new state is solved
static int predict_half_field(pic1dp_ctx *c, const Step &s) {
  FieldArgs f = c->fa;
  f.chargeden = c->d_cd_h;
  // prediction -> chargeden of the next first sub-step, into the scratch vector: tiles combined locally, summed over ranks,
  // scaled; six sums summed over ranks, then the kept mode's content of that charge density -- all the solve looks at
  const PredPlan pp = plan_pred_chargeden(call_moment_of(c, s, Call::WholeSteps), s.k, /*defer=*/false);
  for (int i = 0; i < pp.n; ++i)
    if (int rc = run_act(c, s, pp.act[i], 0, f)) return rc;
  Span tm(c->tm, PIC1DP_IWT_FIELD_ELECTRIC, c->tm.timers_on);
  f.E = c->d_Ehn;
  f.mode_re = c->d_mode_h;
  f.mode_im = c->d_mode_h + c->in.nmode;
  f.history = nullptr;
  HIP_TRY(launch_field_solve(f, false, true, c->st));
  mark_eh_current(c);
  return tm.end();
}

// charge sum over ranks and field solve(s) behind the marker kernel(s) of a sub-step: what plan_solve says, enqueued
static int solve_phase(pic1dp_ctx *c, const Step &s, double *Eout, bool record, bool pred) {
  if (c->charge_sum == 1)  // exact sums over ranks, into the species accumulators: what follows is the one-rank path
    if (int rc = fx_settle(c)) return rc;
  const int tail_done = c->tail_done;  // what the marker launch's tail has done already (kernels.hpp StepTail)
  c->tail_done = 0;
  const SolvePlan sp = plan_solve(s.f, s.k, pred && pred_fresh(c), tail_done, Eout == c->d_E);
  if (sp.refused) return fail(PIC1DP_ERR_STATE, sp.refused == 1 ? "internal: a packed charge nobody reduces" : "internal: a posted charge nobody waits for");
  if (sp.pack_reduce) {  // RCCL path of a one-pass step: everything the two charge sums of the step need in one all-reduce
    if (sp.pack_first) {  // the species sum and the packing are collect_charge's share of the step (src/pic1dp_interaction.F90:126-127)
      Span pk(c->tm, PIC1DP_IWT_COLLECT_CHARGE, c->tm.timers_on);
      HIP_TRY(launch_charge_pack(c->fa, c->d_pred, c->in.nmode, c->plan.pred_kind, c->d_pack, c->st));
      if (int rc = pk.end()) return rc;
    }
    Span ar(c->tm, PIC1DP_IWT_MPIALLREDU, c->tm.timers_on);
    ncclResult_t r = rccl().AllReduce(c->d_pack, c->d_pack, c->plan.pack_doubles, ncclDouble, ncclSum, c->comm, c->st);
    if (r != ncclSuccess) return fail(PIC1DP_ERR_COMM, "ncclAllReduce: %s", rccl().GetErrorString(r));
    if (int rc = ar.end()) return rc;
  } else if (sp.reduce_first) {
    if (int rc = reduce_charge(c)) return rc;
  }
  Span tm(c->tm, PIC1DP_IWT_FIELD_ELECTRIC, c->tm.timers_on);
  FieldArgs f = c->fa;
  f.E = Eout;
  if (record && c->hist_count < kHistCap) f.history = c->d_hist + c->hist_count++;
  if (c->fused_dirty >= 0) {  // the set the last fused launch read: no launch follows that would zero it
    HIP_TRY(hipMemsetAsync(c->d_rho_all + static_cast<size_t>(c->fused_dirty) * c->plan.rho_set_doubles, 0,
                           sizeof(double) * c->plan.rho_set_doubles, c->st));
    HIP_TRY(hipMemsetAsync(c->d_pred_all + static_cast<size_t>(c->fused_dirty) * c->plan.pred_set_doubles, 0,
                           sizeof(double) * c->plan.pred_set_doubles, c->st));
    c->fused_dirty = -1;
  }
  switch (sp.launch) {
    case SolveLaunch::Plain:
      if (int rc = enqueue_field_solve(c, f, sp.with_local, false)) return rc;
      break;
    case SolveLaunch::Exchange:
      HIP_TRY(launch_field_solve_xchg(f, next_xchg_args(c), c->st));
      break;
    default: {  // both fields (the new state's, and the next step's half-step field from the prediction) in ONE launch
      PairArgs pa = pair_args(c);
      XchgArgs x1;
      const XchgArgs *xchg = nullptr;
      if (sp.launch == SolveLaunch::PairPacked) {  // both charge sums of the step came in ONE all-reduce (pack_doubles)
        pa.pack = c->d_pack;
      } else if (sp.launch == SolveLaunch::PairPosted) {  // this rank's half of the exchange is under way since the marker launch's tail
        x1 = c->tail_x;
        x1.ticks = c->tm.timers_on ? c->xc.ticks : nullptr;
        pa.posted = 1;
        xchg = &x1;
      } else if (sp.launch == SolveLaunch::PairExchange) {  // ONE exchange: charge2 and the prediction slices travel together
        x1 = next_xchg_args(c);
        xchg = &x1;
      }
      HIP_TRY(launch_field_solve_pair(f, pa, xchg, c->st));
      pair_solved(c);
      return tm.end();
    }
  }
  if (Eout == c->d_E) field_written(c, true);
  return tm.end();
}

// the solve of a step whose marker launch left it pending, in a launch of its own after all
static int finish_pending_solve(pic1dp_ctx *c, const Step &s) {
  c->fused_pending = false;
  return solve_phase(c, s, c->d_E, true, true);
}

// the previous step's marker launch left its solve (field of the state the markers are in, Eh of this step) to the next
// launch's prologue: what that prologue has to solve, the accumulators' rotation, and what the dedicated launch would
// have recorded
static void wire_fused_solve(pic1dp_ctx *c) {
  FusedSolve &fs = c->fuse_args;
  fs = FusedSolve{};
  fs.on = 1;
  fs.f = c->fa;  // rho_sp: the set the previous launch deposited into
  if (c->hist_count < kHistCap) fs.f.history = c->d_hist + c->hist_count++;
  fs.pt = c->pred_tab;
  fs.pred_in = c->d_pred;
  fs.E_h = c->d_Eh;
  fs.mode_h = c->d_mode_h;
  const int read = c->acc_idx, dirty = c->fused_dirty;
  fs.zero_rho = c->d_rho_all + static_cast<size_t>(dirty >= 0 ? dirty : read) * c->plan.rho_set_doubles;
  fs.zero_rho_n = dirty >= 0 ? static_cast<int64_t>(c->plan.rho_set_doubles) : 0;
  fs.zero_pred = dirty >= 0 ? c->d_pred_all + static_cast<size_t>(dirty) * c->plan.pred_set_doubles
                            : c->d_pred_all + static_cast<size_t>((read + 2) % 3) * c->plan.pred_set_doubles;  // (zero already)
  use_accumulators(c, (read + 1) % 3);  // zero: nobody has deposited into it since it was last zeroed
  c->fused_dirty = read;
  c->fused_pending = false;
  // what the dedicated launch would have recorded: E and its kept mode are the new state's, Eh is this step's
  field_written(c, true);
  c->pred_version = 0;
  c->eh_modes = 2;
}

// sub-step of the whole-step path: particle kernel(s), charge, field into Eout
// fused_in: this launch's prologue solves the previous step's field; fuse_out: this step's solve is left to the next
// launch likewise (fused_pending)
static int step_phase(pic1dp_ctx *c, const Step &s, bool full, double *Eout, bool record, bool diag = false, bool pred = false,
                      bool fused_in = false, bool fuse_out = false) {
  if (full) c->state_version++;
  if (fused_in) wire_fused_solve(c);
  if (int rc = step_particles(c, s, full, c->d_E, c->d_Eh, diag, pred, /*tail_ok=*/full && Eout == c->d_E)) return rc;
  if (fuse_out && pred && pred_fresh(c)) {
    c->fused_pending = true;
    return 0;
  }
  return solve_phase(c, s, Eout, record, pred);
}

// ---------------------------------------------------------------------------
// whole steps and sub-steps in one call
// ---------------------------------------------------------------------------
static int run_call(pic1dp_ctx *c, const Step &s, Call call, const char *who = nullptr, bool field_differs = false);
static int substep_impl(pic1dp_ctx *c, const Step &s, int irk, bool record) {
  if (irk == 2 && optimize_due_any(c)) {
    // src/pic1dp.F90:80-88: push, particle_optimize, collect_charge -- the pushed
    // state has to exist in memory for the host-side optimisation
    if (int rc = enqueue_push(c, irk, false)) return rc;
    if (int rc = pic1dp_hip_particle_optimize(c, irk, nullptr)) return rc;
    if (int rc = enqueue_deposit(c)) return rc;
  } else if (int rc = enqueue_push(c, irk, true)) {
    return rc;
  }
  // (no prediction: reduce, then the plain solve or the exchange's; nothing of a fused launch or a tail is left over here)
  return solve_phase(c, s, c->d_E, record, false);
}

int pic1dp_hip_step(pic1dp_ctx *c, int32_t nsteps) {
  CHECK_CTX(c);
  if (nsteps < 0) return fail(PIC1DP_ERR_ARG, "nsteps < 0");
  Step s = facts_of(c);
  if (int rc = run_call(c, s, nsteps > 0 ? Call::WholeSteps : Call::Markers)) return rc;  // (every step ends with the deposit of the new state)
  for (int it = 0; it < nsteps; ++it) {
    StepMoment m{};
    m.pending = c->fused_pending;
    m.have_eh = eh_current(c);
    m.steps_left = nsteps - it;
    m.output_now = output_follows(c);
    m.output_next = output_follows_at(c, c->itime + 1, c->time + c->in.dt);
    m.optimize_now = optimize_due_any(c);
    bool due[3];
    optimize_due_at(c, c->time + c->in.dt, due);
    m.optimize_next = due[0] || due[1] || due[2];
    WholeStepPlan w = plan_whole_step(s.f, s.k, m);
    if (w.finish_pending) {  // (its pair solve may leave the Eh of this step: asked again)
      if (int rc = finish_pending_solve(c, s)) return rc;
      m.pending = false;
      m.have_eh = eh_current(c);
      w = plan_whole_step(s.f, s.k, m);
    }
    if (w.substeps) {
      const bool event = m.optimize_now;
      if (int rc = substep_impl(c, s, 1, false)) return rc;
      HIP_TRY(hipMemcpyAsync(c->d_Eh, c->d_E, sizeof(double) * c->in.nx, hipMemcpyDeviceToDevice, c->st));
      if (int rc = substep_impl(c, s, 2, true)) return rc;
      if (event) s = facts_of(c);  // (the event changed the marker counts)
    } else {
      // E0 = d_E stays untouched until the second solve overwrites it
      if (w.adopt_eh) {
        std::swap(c->d_Eh, c->d_Ehn);  // d_Eh: the half-step field of the step being taken
        c->eh_modes = 2;               // its kept modes: d_mode_h
      } else if (w.half_pass) {
        if (int rc = step_phase(c, s, false, c->d_Eh, false)) return rc;
        c->eh_modes = w.half_eh_modes;
      }
      if (int rc = step_phase(c, s, true, c->d_E, true, w.diag, w.pred, w.fused_in, w.fuse_out)) return rc;
      if (w.pred && !c->fused_pending && pred_fresh(c))  // not already turned into Eh by the paired solve
        if (int rc = predict_half_field(c, s)) return rc;
    }
    c->itime += 1;                  // src/pic1dp.F90:92
    c->time = c->time + c->in.dt;   // :93
  }
  if (c->fused_pending)  // (the last step of a call never leaves its solve pending; a safety net)
    if (int rc = finish_pending_solve(c, s)) return rc;
  return 0;
}


// ---------------------------------------------------------------------------
// Lazy call sites.  The reference driver calls push(irk), collect_charge,
// solve_field per sub-step (src/pic1dp.F90:80-89).  Run one kernel per call, that
// sequence streams 136 B + 2 x 24 B per marker and step; the whole-step kernels
// need 88 B.  So push() only notes the request and the collect_charge() that
// follows runs k_step_half (after push(1): deposit of the half-step state,
// nothing stored) or k_step_full (after push(2): the whole RK2 step in place).
//   LZ_CLEAN --push(1)--> LZ_PUSH1 --collect--> LZ_HALF --push(2)--> LZ_PUSH2 --collect--> LZ_CLEAN
// Memory then lags behind what the reference would hold (the half-step state is
// never written).  Every other entry point that looks at or changes markers,
// accumulators or the field a noted push depends on first asks for its kind of
// call (call_plan.hpp Call), whose plan runs the ordinary kernels (k_push with the
// right field, wrap) so that memory is bit for bit what the eager calls would have
// left; results of the lazy path itself are the whole-step path's (tests:
// test_lazy_call_sites_*).  WHAT a call enqueues and which state follows is
// plan_call's answer (call_plan.cpp); here is the executor.
// ---------------------------------------------------------------------------
// THE place the call sites' state is written: a pair that cannot occur (call_plan.hpp kCallStateLegal) is an internal error
// here, at the call that would have produced it, instead of a wrong field some calls later
static int set_call_state(pic1dp_ctx *c, Seq seq, Owed owed) {
  if (seq >= Seq::N || owed >= Owed::N || !kCallStateLegal[static_cast<int>(seq)][static_cast<int>(owed)])
    return fail(PIC1DP_ERR_STATE, "internal: call-site state (%d, %d) cannot occur (from (%d, %d))", static_cast<int>(seq),
                static_cast<int>(owed), static_cast<int>(c->seq), static_cast<int>(c->owed));
  if (seq != Seq::Clean && !c->cfg.lazy_calls) return fail(PIC1DP_ERR_STATE, "internal: a push noted by eager call sites");
  c->seq = seq;
  c->owed = owed;
  return 0;
}
// ... and what the machine remembers beside the pair (the executor's store)
static int store_call_state(pic1dp_ctx *c, const CallState &n) {
  if (int rc = set_call_state(c, n.seq, n.owed)) return rc;
  c->e_step_start = n.e_step_start, c->cd_kept_mode_only = n.cd_kept_mode_only;
  c->adopt_cd_version = n.adopt_current ? c->cd_version : 0;  // (an adoption holds while cd_version stays where it is)
  c->charge_pending = n.charge_pending, c->charge_pending_pred = n.charge_pending_pred;
  c->call_phase = n.call_phase, c->eh_modes = n.eh_modes;
  return 0;
}

// What a checkpoint does not carry, in a defined state: call sites Clean with nothing owed; the markers count as changed
// (state_version), so no prediction, no predicted half-step field, no carried -f0'/f0 and no cached diagnostics belong to
// them; the field counts as written by something else than a solve (its kept modes are data, not a description the
// one-pass kernels may build Eh from); every accumulator set and the exact accumulators zero, set 0 the current one;
// nothing of a fused solve or a tail left over.  The step after it takes two passes.
int pic1dp_host::reset_derived_state(pic1dp_ctx *c) {
  c->cd_version++;
  if (int rc = store_call_state(c, CallState{})) return rc;
  c->state_version++;
  c->pred_version = c->eh_version = 0;
  c->eh_field_version = 0;
  c->field_version++;
  c->modes_field_version = 0;
  for (Species &S : c->sp) S.t2_version = 0;
  for (DiagSpecies &D : c->diag) {
    D.version = 0;
    D.pending = false;
    D.blocks = 0;
    D.sums[0] = D.sums[1] = D.sums[2] = 0.0;
  }
  c->fused_pending = false;
  c->fused_dirty = -1;
  c->fuse_args = FusedSolve{};
  c->tail_done = 0;
  c->tail_x = XchgArgs{};
  use_accumulators(c, 0);
  HIP_TRY(hipMemsetAsync(c->d_rho_all, 0, sizeof(double) * 3 * c->plan.rho_set_doubles, c->st));
  if (c->d_pred_all) HIP_TRY(hipMemsetAsync(c->d_pred_all, 0, sizeof(double) * 3 * c->plan.pred_set_doubles, c->st));
  if (c->d_fx) HIP_TRY(hipMemsetAsync(c->d_fx, 0, sizeof(long long) * 2 * static_cast<size_t>(c->in.nspecies) * c->in.nx, c->st));
  HIP_TRY(hipMemsetAsync(c->d_ticket, 0, 64, c->st));
  HIP_TRY(hipMemsetAsync(c->d_Eh, 0, sizeof(double) * c->in.nx, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));
  return 0;
}

// wrap of x stored back, as the deposit of collect_charge does, charge discarded
static int enqueue_wrap_only(pic1dp_ctx *c) {
  for (int s = 0; s < c->in.nspecies; ++s) {
    Species &S = c->sp[s];
    if (S.np <= 0) continue;
    const double *q = c->in.deltaf ? S.set[c->cur].w : S.p;
    LaunchCfg lc = particle_launch(c, S.np, false, true);
    HIP_TRY(launch_deposit(S.set[c->cur].x, q, c->d_rho_dummy, FxArgs{}, S.np, c->grid, lc, c->st));
  }
  return 0;
}

// field_electric and its kept modes <- the half-step field the pair solve left in d_Ehn / d_mode_h, and field_chargeden
// <- the kept mode's content of the half-step charge density it left in d_cd_h (what collect_charge leaves there when it
// is served from the six sums, Owed::PredSums): a solve_field that solves from field_chargeden again reproduces the half-step
// field, as it does after eager calls
static int adopt_half_field(pic1dp_ctx *c) {
  const size_t nx = c->in.nx;
  HIP_TRY(hipMemcpyAsync(c->d_chargeden, c->d_cd_h, sizeof(double) * nx, hipMemcpyDeviceToDevice, c->st));
  HIP_TRY(hipMemcpyAsync(c->d_E, c->d_Ehn, sizeof(double) * nx, hipMemcpyDeviceToDevice, c->st));
  return adopt_half_modes(c);
}

// what a refusal of the plan says (the texts the entry points had)
static int refusal_error(const pic1dp_ctx *c, const CallPlan &p, const char *who) {
  who = who ? who : "the call";
  switch (p.refusal) {
    case Refusal::NotLoaded: return fail(PIC1DP_ERR_STATE, "no particles: call particle_load or particles_upload first");
    case Refusal::ChargeWaiting: return fail(PIC1DP_ERR_STATE, "charge_local is waiting for charge_reduced");
    case Refusal::IllegalState:
      return fail(PIC1DP_ERR_STATE, "internal: call-site state (%d, %d) cannot occur (from (%d, %d))", static_cast<int>(p.bad_seq),
                  static_cast<int>(p.bad_owed), static_cast<int>(c->seq), static_cast<int>(c->owed));
    case Refusal::EagerNoted: return fail(PIC1DP_ERR_STATE, "internal: a push noted by eager call sites");
    case Refusal::WantsExactLocal:
      return fail(PIC1DP_ERR_STATE, "exact charge sum: a sum of doubles over ranks cannot be exact; use charge_local_exact");
    case Refusal::WantsExactReduced:
      return fail(PIC1DP_ERR_STATE, "exact charge sum: a sum of doubles over ranks cannot be exact; use charge_reduced_exact");
    case Refusal::NeedsExactSum: return fail(PIC1DP_ERR_STATE, "%s needs the exact charge sum (set_charge_sum(1))", who);
    case Refusal::ReducedWithoutLocal:
      return fail(PIC1DP_ERR_STATE, "%s without charge_local%s", who, c->charge_sum == 1 ? "_exact" : "");
    case Refusal::NotBetweenSteps:
      return fail(PIC1DP_ERR_STATE, "%s while a push, a charge or a solve is pending: call it between time steps", who);
    case Refusal::CheckpointChargeWaiting:
      return fail(PIC1DP_ERR_STATE, "checkpoint_write: charge_local is waiting for charge_reduced");
    case Refusal::CheckpointPushNoted:
      return fail(PIC1DP_ERR_STATE, "checkpoint_write: a push is noted -- checkpoints are written between time steps only");
    case Refusal::CheckpointInsideStep:
      return fail(PIC1DP_ERR_STATE, "checkpoint_write: call %d of the six of a time step was the last -- checkpoints are written between time steps only",
                  c->call_phase);
    case Refusal::CheckpointKeptMode:
      return fail(PIC1DP_ERR_STATE, "checkpoint_write: field_chargeden holds a half step's kept mode only -- checkpoints are written between time steps only");
    default: return fail(PIC1DP_ERR_STATE, "internal: a call plan of more than %d actions", kMaxActs);
  }
}

// THE executor: the call's plan, its actions in order through the helpers and the timer spans, then the state that follows.
// (a whole-step kernel run for a noted push books itself under "push particle", step_particles; the span the plan opens
// around the rest of a collect_charge covers the reduction and scaling only)
static int plan_of(const pic1dp_ctx *c, const Step &s, Call call, const char *who, bool field_differs, CallPlan *p) {
  *p = plan_call(call_state_of(c), call_moment_of(c, s, call, field_differs), s.k, call);
  return p->refusal != Refusal::None && !p->refused_after ? refusal_error(c, *p, who) : 0;
}
static int run_plan(pic1dp_ctx *c, const Step &s, const CallPlan &p, const char *who) {
  HIP_TRY(hipSetDevice(c->device));
  std::optional<Span> span;
  for (int i = 0; i < p.n; ++i) {
    int rc = 0;
    switch (p.act[i]) {
      case Act::SpanCollect: span.emplace(c->tm, PIC1DP_IWT_COLLECT_CHARGE, c->tm.timers_on); break;
      case Act::SpanField: span.emplace(c->tm, PIC1DP_IWT_FIELD_ELECTRIC, c->tm.timers_on); break;
      case Act::SpanEnd: rc = span->end(); break;
      default: rc = run_act(c, s, p.act[i], p.arg[i], c->fa);
    }
    if (rc) return rc;
  }
  if (int rc = store_call_state(c, p.next)) return rc;
  return p.refused_after ? refusal_error(c, p, who) : 0;
}
static int run_call(pic1dp_ctx *c, const Step &s, Call call, const char *who, bool field_differs) {
  CallPlan p;
  if (int rc = plan_of(c, s, call, who, field_differs, &p)) return rc;
  return run_plan(c, s, p, who);
}
// what the other units ask for (ctx.hpp)
int pic1dp_host::call_site(pic1dp_ctx *c, Call call, const char *who, bool field_differs) {
  return run_call(c, facts_of(c), call, who, field_differs);
}
int pic1dp_host::require_loaded(pic1dp_ctx *c) { return call_site(c, Call::Markers); }

// ---------------------------------------------------------------------------
// the call sites: check the arguments, name the call, execute
// ---------------------------------------------------------------------------
int pic1dp_hip_push(pic1dp_ctx *c, int32_t irk) {
  CHECK_CTX(c);
  if (irk != 1 && irk != 2) return fail(PIC1DP_ERR_ARG, "irk must be 1 or 2");
  return run_call(c, facts_of(c), irk == 1 ? Call::Push1 : Call::Push2);
}

int pic1dp_hip_collect_charge(pic1dp_ctx *c) {
  CHECK_CTX(c);
  return run_call(c, facts_of(c), Call::CollectCharge);
}

int pic1dp_hip_solve_field(pic1dp_ctx *c) {
  CHECK_CTX(c);
  return run_call(c, facts_of(c), Call::SolveField);
}

int pic1dp_hip_substep(pic1dp_ctx *c, int32_t irk) {
  CHECK_CTX(c);
  if (irk != 1 && irk != 2) return fail(PIC1DP_ERR_ARG, "irk must be 1 or 2");
  const Step s = facts_of(c);
  if (int rc = run_call(c, s, irk == 1 ? Call::Substep1 : Call::Substep2)) return rc;
  return substep_impl(c, s, irk, false);
}

int pic1dp_hip_set_field_solver(pic1dp_ctx *c, int32_t kind) {
  CHECK_CTX(c);
  if (kind != 0 && kind != 1) return fail(PIC1DP_ERR_ARG, "field solver must be 0 (reference mode filter) or 1 (finite differences)");
  if (kind == 1 && (c->in.nx < 3 || c->in.nx > 4096))
    return fail(PIC1DP_ERR_ARG, "the finite-difference solver needs 3 <= nx <= 4096");
  if (int rc = call_site(c, Call::SwitchField, nullptr, kind != c->field_solver)) return rc;
  c->field_solver = kind;
  return 0;
}

int pic1dp_hip_field_transform_supported(int32_t nx, int32_t transform, int32_t *supported) {
  if (!supported) return fail(PIC1DP_ERR_ARG, "null argument");
  if (transform != 0 && transform != 1) return fail(PIC1DP_ERR_ARG, "field transform must be 0 (direct partial DFT) or 1 (FFT)");
  *supported = transform == 0 ? (nx >= 2 && nx <= 8192) : fft_supported(nx);
  return 0;
}

int pic1dp_hip_set_field_transform(pic1dp_ctx *c, int32_t transform) {
  CHECK_CTX(c);
  if (transform != 0 && transform != 1) return fail(PIC1DP_ERR_ARG, "field transform must be 0 (direct partial DFT) or 1 (FFT)");
  if (transform == 1 && !fft_supported(c->in.nx))
    return fail(PIC1DP_ERR_ARG, "the FFT field transform needs nx = 2^a 3^b 5^c, even up to %d or odd up to %d (nx = %d)", FFT_MAX_NX,
                FFT_MAX_ODD_NX, c->in.nx);
  HIP_TRY(hipSetDevice(c->device));
  if (transform == 1 && !c->fft.tw) {
    const bool had_tw = c->d_fft_tw != nullptr, had_idx = c->d_fft_idx != nullptr;
    const hipError_t e = fft_plan_upload(c->in.nx, c->in.modes, c->in.nmode, c->fft, &c->d_fft_tw, &c->d_fft_idx);
    if (!had_tw) c->mem.adopt(c->d_fft_tw);  // (the plan builder allocates what is missing: the context owns it from here)
    if (!had_idx) c->mem.adopt(c->d_fft_idx);
    HIP_TRY(e);
  }
  if (int rc = call_site(c, Call::SwitchField, nullptr, transform != c->field_transform)) return rc;
  c->field_transform = transform;
  return 0;
}

int pic1dp_hip_set_step_mode(pic1dp_ctx *c, int32_t mode) {
  CHECK_CTX(c);
  if (mode != 0 && mode != 1) return fail(PIC1DP_ERR_ARG, "step mode must be 0 or 1");
  c->step_mode = mode;
  return 0;
}

int pic1dp_hip_predict_kind(pic1dp_ctx *c, int32_t *kind) {
  CHECK_CTX(c);
  if (!kind) return fail(PIC1DP_ERR_ARG, "null argument");
  *kind = facts_of(c).k.predict_capable ? c->plan.pred_kind : 0;
  return 0;
}

int pic1dp_hip_set_output_fusion(pic1dp_ctx *c, int32_t on) {
  CHECK_CTX(c);
  if (on < 0 || on > 2) return fail(PIC1DP_ERR_ARG, "output fusion must be 0 (off), 1 (where it pays) or 2 (always)");
  c->fuse_output = on;
  return 0;
}

int pic1dp_hip_chargeden_state(pic1dp_ctx *c, int32_t *kept_mode_only) {
  CHECK_CTX(c);
  if (!kept_mode_only) return fail(PIC1DP_ERR_ARG, "null output");
  *kept_mode_only = call_state_of(c).cd_kept_mode_only ? 1 : 0;
  return 0;
}

// ---------------------------------------------------------------------------
// split-phase deposit
// ---------------------------------------------------------------------------
int pic1dp_hip_charge_local(pic1dp_ctx *c, double *charge2) {
  CHECK_CTX(c);
  if (!charge2) return fail(PIC1DP_ERR_ARG, "null array");
  if (int rc = run_call(c, facts_of(c), Call::ChargeLocal)) return rc;
  HIP_TRY(hipStreamSynchronize(c->st));
  HIP_TRY(hipMemcpy(charge2, c->d_charge, sizeof(double) * c->in.nx, hipMemcpyDeviceToHost));
  return 0;
}

int pic1dp_hip_charge_reduced(pic1dp_ctx *c, const double *charge1) {
  CHECK_CTX(c);
  if (!charge1) return fail(PIC1DP_ERR_ARG, "null array");
  const Step s = facts_of(c);
  CallPlan p;
  if (int rc = plan_of(c, s, Call::ChargeReduced, "charge_reduced", false, &p)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpy(c->d_charge, charge1, sizeof(double) * c->in.nx, hipMemcpyHostToDevice));
  return run_plan(c, s, p, "charge_reduced");
}

// kind 1 of the charge sum: the split phase with integers (include/pic1dp_hip.h has the layout)
int pic1dp_hip_charge_local_exact(pic1dp_ctx *c, int64_t *limbs) {
  CHECK_CTX(c);
  if (!limbs) return fail(PIC1DP_ERR_ARG, "null array");
  const Step s = facts_of(c);
  if (int rc = run_call(c, s, Call::ChargeLocalExact, "charge_local_exact")) return rc;
  const size_t n = 2 * static_cast<size_t>(c->in.nspecies) * c->in.nx;
  HIP_TRY(launch_fx_normalise(c->d_fx, c->in.nspecies, c->in.nx, c->st));
  HIP_TRY(hipMemcpyAsync(limbs, c->d_fx, sizeof(int64_t) * n, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipMemsetAsync(c->d_fx, 0, sizeof(int64_t) * n, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));
  if (int rc = fx_check(c)) return rc;  // (a contribution left out: no charge to hand out)
  return run_call(c, s, Call::ChargeExactHandedOut);
}

int pic1dp_hip_charge_reduced_exact(pic1dp_ctx *c, const int64_t *limbs) {
  CHECK_CTX(c);
  if (!limbs) return fail(PIC1DP_ERR_ARG, "null array");
  const Step s = facts_of(c);
  CallPlan p;
  if (int rc = plan_of(c, s, Call::ChargeReducedExact, "charge_reduced_exact", false, &p)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = 2 * static_cast<size_t>(c->in.nspecies) * c->in.nx;
  HIP_TRY(hipMemcpy(c->d_fx, limbs, sizeof(int64_t) * n, hipMemcpyHostToDevice));
  return run_plan(c, s, p, "charge_reduced_exact");
}

// ---------------------------------------------------------------------------
// pic1dp_hip_check_state: the relations between the flags of the state machine above (the table of
// invariants) checked at an API boundary -- between two calls of the library every one of them has to hold, whatever the
// calls were.  deep != 0 also looks at device memory (one stream synchronisation and small copies): the accumulator sets
// nobody owes anything to are zero, the tail's ticket is back at zero.  A debugging aid and what the randomised call-
// sequence tests call after EVERY call (tests/test_gpu_fuzz.py); nothing on the hot path calls it.
// ---------------------------------------------------------------------------
int pic1dp_hip_check_state(pic1dp_ctx *c, int32_t deep) {
  CHECK_CTX(c);
#define INVARIANT(cond)                                                                                   \
  do {                                                                                                    \
    if (!(cond))                                                                                          \
      return fail(PIC1DP_ERR_STATE, "state invariant violated: %s (call-site state %d, owed %d)", #cond, \
                  static_cast<int>(st.seq), static_cast<int>(st.owed));                                   \
  } while (0)
  // The call sites' state is one (Seq, Owed) pair written by set_call_state alone, which refuses the pairs that cannot
  // occur (call_plan.hpp kCallStateLegal): what used to be a dozen relations between lz, cd_lazy, half_pair and half_solved
  // checked here cannot be violated any more.  What relates the parts of the state to each other and to the context it is
  // held in is call_state_invariants' (pure: the host walk of tests/call_plan_check.cpp asks it too); what relates it to the
  // versions follows here
  const Step s = facts_of(c);
  const CallState st = call_state_of(c);
  if (const char *broken = call_state_invariants(st, call_moment_of(c, s, Call::N), s.k))
    return fail(PIC1DP_ERR_STATE, "state invariant violated: %s (call-site state %d, owed %d)", broken, static_cast<int>(st.seq),
                static_cast<int>(st.owed));
  INVARIANT(c->charge_sum == 0 || c->pred_version == 0);   // kind 1 of the charge sum: no prediction pending
  INVARIANT(!pair_of(st.seq) || c->eh_version == c->state_version);   // the field in d_Ehn belongs to the state in memory
  // whole-step path: nothing of a step() is left over between calls
  INVARIANT(!c->fused_pending);
  INVARIANT(c->fuse_args.on == 0);
  INVARIANT(c->fused_dirty == -1);
  INVARIANT(c->tail_done == 0);
  INVARIANT(c->acc_idx >= 0 && c->acc_idx < 3);
  // versions only ever point backwards
  INVARIANT(c->pred_version <= c->state_version);
  INVARIANT(c->eh_version <= c->state_version);
  INVARIANT(c->eh_field_version <= c->field_version);
  INVARIANT(c->modes_field_version <= c->field_version);
  for (int s = 0; s < c->in.nspecies; ++s) {
    INVARIANT(c->diag[s].version <= c->state_version);
    INVARIANT(c->sp[s].t2_version <= c->state_version);
  }
  if (!deep) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->st));
  unsigned ticket = 0;
  HIP_TRY(hipMemcpy(&ticket, c->d_ticket, sizeof ticket, hipMemcpyDeviceToHost));
  INVARIANT(ticket == 0u);
  if (c->d_fx) {  // the exact accumulators are settled (or handed out) by the call that deposited into them
    std::vector<long long> fx(2 * static_cast<size_t>(c->in.nspecies) * c->in.nx);
    HIP_TRY(hipMemcpy(fx.data(), c->d_fx, sizeof(long long) * fx.size(), hipMemcpyDeviceToHost));
    for (long long v : fx) INVARIANT(v == 0 && "exact deposits nobody is going to sum");
  }
  // accumulators: the sets the marker kernels do not deposit into are zero; the current one holds something only while
  // a collect_charge has left its end to solve_field (Owed::SumScale, PredTiles: deposits; with a usable prediction: the six sums / tiles)
  auto nonzero = [](const std::vector<double> &v, size_t off, size_t n) {
    for (size_t i = 0; i < n; ++i)
      if (v[off + i] != 0.0) return true;  // (NaN != 0: a poisoned accumulator counts)
    return false;
  };
  std::vector<double> h(3 * c->plan.rho_set_doubles);
  HIP_TRY(hipMemcpy(h.data(), c->d_rho_all, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
  for (int k = 0; k < 3; ++k) {
    const bool nz = nonzero(h, k * c->plan.rho_set_doubles, c->plan.rho_set_doubles);
    if (k != c->acc_idx) INVARIANT(!nz && "a species accumulator set that is not the current one holds deposits");
    else if (st.owed != Owed::SumScale && st.owed != Owed::PredTiles && !st.charge_pending) INVARIANT(!nz && "deposits nobody is going to sum");
  }
  if (c->d_pred_all && c->plan.pred_set_doubles) {
    h.assign(3 * c->plan.pred_set_doubles, 0.0);
    HIP_TRY(hipMemcpy(h.data(), c->d_pred_all, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; ++k) {
      const bool nz = nonzero(h, k * c->plan.pred_set_doubles, c->plan.pred_set_doubles);
      if (k != c->acc_idx) INVARIANT(!nz && "a prediction accumulator set that is not the current one holds sums");
      else if (c->pred_version == 0 && st.owed != Owed::PredTiles && st.owed != Owed::PredSums && !st.charge_pending)
        INVARIANT(!nz && "prediction sums that belong to no state");
    }
  }
#undef INVARIANT
  return 0;
}
