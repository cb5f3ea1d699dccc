// capi_step.cpp -- the ACTIONS of the hot path behind the C ABI of include/pic1dp_hip.h: the three call sites and their
// lazy state machine (push / collect_charge / solve_field), pic1dp_hip_step, the prediction of the half-step charge, the
// solve inside the marker launch, the split-phase deposit.  What a step launches is DECIDED in step_plan.cpp (pure, pinned
// on the host): here are the wiring (pointers, versions, counters, spans), the state transitions and the order of enqueues.
// Launch shapes: launch_policy.cpp; the other units: ctx.hpp.  In order of dependency: facts_of and the currency relations,
// the marker launches, prediction and solve, pic1dp_hip_step, the call sites, the split-phase deposit, pic1dp_hip_check_state.
// (the entry points are declared extern "C" in include/pic1dp_hip.h; their definitions here inherit that linkage)
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
  c->e_step_start = false;  // (every writer writes the whole of field_electric; set_electric settles the kept modes first)
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

// prediction -> chargeden of the next first sub-step (f.chargeden: field_chargeden, or a scratch vector).
// Tiles: combined locally, summed over ranks, scaled.  Six sums: summed over ranks, then the kept mode's
// content of that charge density -- all the solve looks at (k_pred_chargeden).
// defer (call sites, f = c->fa): leave the scaling of the summed charge to the solve_field that follows (Owed)
static int pred_to_chargeden(pic1dp_ctx *c, const Step &s, const FieldArgs &f, bool defer = false) {
  c->pred_version = 0;  // consumed: the accumulators are zero again afterwards
  const bool multi = several_ranks(c);
  if (c->plan.pred_kind == 2) {
    if (f.chargeden == c->d_chargeden) c->cd_kept_mode_only = true;
    if (defer && !multi && s.k.dft_paths && f.tab_lds)  // the sums' combination, chargeden and the solve in the
      return set_owed(c, Owed::PredSums);               // launch of the solve_field that follows
    if (!multi) {
      HIP_TRY(launch_pred_chargeden(f, c->pred_tab, c->d_pred, nullptr, c->st));
      return 0;
    }
    HIP_TRY(launch_pred_to_charge(c->fa, c->d_pred, c->st));
    if (int rc = pred_reduce(c)) return rc;
    HIP_TRY(launch_pred_chargeden(f, c->pred_tab, nullptr, c->d_charge, c->st));
    return 0;
  }
  if (defer && !multi && s.k.dft_paths && s.k.modes_fit_field_kernel)
    return set_owed(c, Owed::PredTiles);  // all of it in the launch of the solve_field that follows
  HIP_TRY(launch_pred_combine(c->fa, c->d_pred, c->in.nmode, c->st));
  if (multi)
    if (int rc = pred_reduce(c)) return rc;
  if (defer) return set_owed(c, Owed::Scale);
  HIP_TRY(launch_chargeden(f, false, c->st));
  return 0;
}

// step() path: Eh of the NEXT step from the prediction, right after the field of the new state is solved
static int predict_half_field(pic1dp_ctx *c, const Step &s) {
  FieldArgs f = c->fa;
  f.chargeden = c->d_cd_h;
  if (int rc = pred_to_chargeden(c, s, f)) return rc;
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
static int substep_impl(pic1dp_ctx *c, const Step &s, int irk, bool record) {
  c->cd_kept_mode_only = false;
  c->cd_version++;
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
  if (int rc = require_loaded(c)) return rc;
  if (nsteps > 0) {  // every step ends with the deposit of the new state
    c->cd_kept_mode_only = false;
    c->cd_version++;
    c->call_phase = 0;
  }
  Step s = facts_of(c);
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
// the call sites and what settles their state
// ---------------------------------------------------------------------------
// field_chargeden (and d_charge, and zeroed accumulators) as collect_charge would have left them at once
int pic1dp_host::materialize_cd(pic1dp_ctx *c) {
  const Owed pending = c->owed;
  if (pending == Owed::AdoptHalfField) return 0;  // (a half-step FIELD waiting to be adopted by solve_field: no charge to settle)
  if (pending == Owed::Nothing) return 0;
  if (int rc = set_owed(c, Owed::Nothing)) return rc;
  if (pending == Owed::PredSums) {  // the six sums of a predicted push(1): the kept mode's content of chargeden, directly
    HIP_TRY(launch_pred_chargeden(c->fa, c->pred_tab, c->d_pred, nullptr, c->st));
    return 0;
  }
  if (pending == Owed::PredTiles) HIP_TRY(launch_pred_combine(c->fa, c->d_pred, c->in.nmode, c->st));
  HIP_TRY(launch_chargeden(c->fa, pending == Owed::SumScale, c->st));
  return 0;
}

// THE place the call sites' state is written: a pair that cannot occur (ctx.hpp kCallStateLegal) is an internal error
// here, at the call that would have produced it, instead of a wrong field some calls later
int pic1dp_host::set_call_state(pic1dp_ctx *c, Seq seq, Owed owed) {
  if (seq >= Seq::N || owed >= Owed::N || !kCallStateLegal[static_cast<int>(seq)][static_cast<int>(owed)])
    return fail(PIC1DP_ERR_STATE, "internal: call-site state (%d, %d) cannot occur (from (%d, %d))", static_cast<int>(seq),
                static_cast<int>(owed), static_cast<int>(c->seq), static_cast<int>(c->owed));
  if (seq != Seq::Clean && !c->cfg.lazy_calls) return fail(PIC1DP_ERR_STATE, "internal: a push noted by eager call sites");
  c->seq = seq;
  c->owed = owed;
  return 0;
}
int pic1dp_host::set_seq(pic1dp_ctx *c, Seq seq) { return set_call_state(c, seq, c->owed); }
int pic1dp_host::set_owed(pic1dp_ctx *c, Owed owed) { return set_call_state(c, c->seq, owed); }

// What a checkpoint does not carry, in a defined state: call sites Clean with nothing owed; the markers count as changed
// (state_version), so no prediction, no predicted half-step field, no carried -f0'/f0 and no cached diagnostics belong to
// them; the field counts as written by something else than a solve (its kept modes are data, not a description the
// one-pass kernels may build Eh from); every accumulator set and the exact accumulators zero, set 0 the current one;
// nothing of a fused solve or a tail left over.  The step after it takes two passes.
int pic1dp_host::reset_derived_state(pic1dp_ctx *c) {
  if (int rc = set_call_state(c, Seq::Clean, Owed::Nothing)) return rc;
  c->state_version++;
  c->pred_version = c->eh_version = 0;
  c->eh_field_version = 0;
  c->field_version++;
  c->modes_field_version = 0;
  c->eh_modes = 0;
  c->e_step_start = false;
  c->cd_kept_mode_only = false;
  c->cd_version++;
  c->adopt_cd_version = 0;
  c->charge_pending = c->charge_pending_pred = false;
  c->call_phase = 0;
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

// ctx.hpp call_phase: a push opens its sub-step wherever the host stood; a collected charge (collect_charge, charge_reduced)
// and a solved field move on only from the call they follow in the reference's order -- a second collect_charge or
// solve_field of the same sub-step stays where it is
static void call_phase_push(pic1dp_ctx *c, int irk) { c->call_phase = irk == 1 ? 1 : 4; }
static void call_phase_collect(pic1dp_ctx *c) {
  if (c->call_phase == 1 || c->call_phase == 4) c->call_phase++;
}
static void call_phase_solve(pic1dp_ctx *c) {
  if (c->call_phase == 2) c->call_phase = 3;
  else if (c->call_phase == 5) c->call_phase = 0;
}

// checks only: for the call sites that take part in the lazy scheme themselves
static int require_loaded_keep_lazy(pic1dp_ctx *c) {
  if (!c->loaded) return fail(PIC1DP_ERR_STATE, "no particles: call particle_load or particles_upload first");
  if (c->charge_pending) return fail(PIC1DP_ERR_STATE, "charge_local is waiting for charge_reduced");
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail(PIC1DP_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
  if (int rc = settle_step_start_field(c)) return rc;   // (a push or a step reads field_electric)
  return materialize_cd(c);
}

// every other entry point that reads or writes markers or charge accumulators:
// memory first becomes what the eager calls would have left
int pic1dp_host::require_loaded(pic1dp_ctx *c) {
  if (int rc = require_loaded_keep_lazy(c)) return rc;
  return materialize(c);
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
// accumulators or the field a noted push depends on first calls materialize(),
// which runs the ordinary kernels (k_push with the right field, wrap) so that
// memory is bit for bit what the eager calls would have left; results of the lazy
// path itself are the whole-step path's (tests: test_lazy_call_sites_*).
// ---------------------------------------------------------------------------
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

// Call sites (ctx.hpp Seq, the Pair states): the half-step field the pair solve left in d_Ehn / d_mode_h, and the step-start
// field still in field_electric, put where the eager calls would have them -- d_E0 <- E, and, once the host has called
// solve_field for the half step, E <- the half-step field with its kept modes.  Everything that looks at the field, or
// leaves the sequence push(1), collect_charge, solve_field, push(2), collect_charge, comes through here first.
int pic1dp_host::settle_half_pair(pic1dp_ctx *c) {
  if (!pair_of(c->seq)) return 0;
  if (int rc = save_step_start_field(c)) return rc;
  const bool solved = solved_of(c->seq);
  if (int rc = set_seq(c, unpaired(c->seq))) return rc;
  // solve_field has been called for the half step: field_electric has to BE the half-step field now (field_version was
  // bumped when it was called); not yet called: it stays owed (AdoptHalfField) and copies when it comes
  if (solved) return adopt_half_field(c);
  return 0;
}
// for readers of the field only: nothing to do until the host has called solve_field for the half step -- until then
// field_electric is the step-start field, which is what d_E holds
int pic1dp_host::settle_field_view(pic1dp_ctx *c) {
  if (int rc = settle_step_start_field(c)) return rc;
  return solved_of(c->seq) ? settle_half_pair(c) : 0;
}
// field_electric and its kept modes as the eager calls leave them after push(2), collect_charge of a pair-solved step: the
// half-step field (the whole-step kernel read the step-start field from field_electric; d_Eh / d_mode_h hold the half step's)
int pic1dp_host::settle_step_start_field(pic1dp_ctx *c) {
  if (!c->e_step_start) return 0;
  c->e_step_start = false;
  HIP_TRY(hipMemcpyAsync(c->d_E, c->d_Eh, sizeof(double) * c->in.nx, hipMemcpyDeviceToDevice, c->st));
  return adopt_half_modes(c);
}
// field_electric and its kept modes <- the half-step field the pair solve left in d_Ehn / d_mode_h, and field_chargeden
// <- the kept mode's content of the half-step charge density it left in d_cd_h (what collect_charge leaves there when it
// is served from the six sums, Owed::PredSums): a solve_field that solves from field_chargeden again reproduces the half-step
// field, as it does after eager calls
int pic1dp_host::adopt_half_field(pic1dp_ctx *c) {
  const size_t nx = c->in.nx;
  HIP_TRY(hipMemcpyAsync(c->d_chargeden, c->d_cd_h, sizeof(double) * nx, hipMemcpyDeviceToDevice, c->st));
  HIP_TRY(hipMemcpyAsync(c->d_E, c->d_Ehn, sizeof(double) * nx, hipMemcpyDeviceToDevice, c->st));
  return adopt_half_modes(c);
}

int pic1dp_host::materialize(pic1dp_ctx *c) {
  if (int rc = settle_half_pair(c)) return rc;
  const int lz = lz_of(c->seq);
  if (lz == LZ_CLEAN) return 0;
  // a half-step field waits to be adopted: it was solved from the half-step charge density, which leaves with the markers'
  // half-step state -- that state is deposited for real on its way into memory (what the eager collect_charge left in
  // field_chargeden), and the solve_field that follows solves from it (a step or substep in between overwrote d_Ehn / d_cd_h)
  if (c->owed == Owed::AdoptHalfField) return rebuild_half_step_chargeden(c);
  if (int rc = set_seq(c, Seq::Clean)) return rc;
  if (lz == LZ_PUSH1) return enqueue_push(c, 1, false);           // the field has not changed since
  // LZ_HALF / LZ_PUSH2: push(1) saw d_E0; its deposit wrapped x
  if (int rc = enqueue_push(c, 1, false, c->d_E0)) return rc;
  if (int rc = enqueue_wrap_only(c)) return rc;
  if (lz == LZ_PUSH2) return enqueue_push(c, 2, false);
  return 0;
}

// the deposit of collect_charge / charge_local into the species accumulators:
// the whole-step kernel of a noted push, or the plain wrap + deposit
static int deposit_or_step(pic1dp_ctx *c, const Step &s) {
  if (c->seq == Seq::Push1) {
    if (int rc = save_step_start_field(c)) return rc;
    if (int rc = step_particles(c, s, false, c->d_E, c->d_Eh)) return rc;
    return set_seq(c, Seq::Half);
  }
  if (lz_of(c->seq) == LZ_PUSH2) {
    if (c->seq == Seq::Push2Pair)  // (push(2) without the solve_field of the half step: it sees the old field)
      if (int rc = settle_half_pair(c)) return rc;
    c->state_version++;
    const bool diag = s.k.diag_in_step && output_follows(c);
    if (c->seq == Seq::Push2PairSolved) {  // the half-step field came out of the previous step's pair solve: E0 is still in d_E
      std::swap(c->d_Eh, c->d_Ehn);
      c->eh_modes = 2;  // its kept mode: d_mode_h
      if (int rc = step_particles(c, s, true, c->d_E, c->d_Eh, diag, !diag)) return rc;
      c->e_step_start = true;  // (field_electric: still the step-start field -- the solve_field that follows overwrites it)
      return set_seq(c, Seq::Clean);
    }
    // Eh = d_E: the kept modes describe it when the mode-filter solve wrote it last
    c->eh_modes = (s.k.dft_paths && c->modes_field_version == c->field_version) ? 1 : 0;
    if (int rc = step_particles(c, s, true, c->d_E0, c->d_E, diag, !diag)) return rc;
    return set_seq(c, Seq::Clean);
  }
  if (int rc = materialize(c)) return rc;
  return enqueue_deposit(c);
}

int pic1dp_hip_collect_charge(pic1dp_ctx *c) {
  CHECK_CTX(c);
  if (int rc = require_loaded_keep_lazy(c)) return rc;
  call_phase_collect(c);
  const Step s = facts_of(c);
  c->cd_version++;
  // a whole-step kernel run for a noted push is booked under "push particle"
  // (step_particles); "collect charge" then covers the reduction and scaling only
  // after a noted push(1) whose charge the previous step's kernel has predicted (k_step_one): no
  // pass over the markers at all -- combine, reduce, scale
  if (pair_of(c->seq) && c->seq != Seq::Push2PairSolved)  // out of sequence: memory as the eager calls leave it
    if (int rc = settle_half_pair(c)) return rc;
  // after a noted push(1) whose half-step FIELD the previous solve_field has already solved (the pair, below): nothing
  // to launch at all
  // (the six sums of one kept mode: with the tiles collect_charge owes the host the whole half-step charge density)
  if (c->seq == Seq::Push1 && s.k.pair_serves_collect && eh_current(c)) {
    c->cd_kept_mode_only = true;  // (field_chargeden is not the half step's: asking for it rebuilds, get_field)
    c->adopt_cd_version = c->cd_version;
    return set_call_state(c, Seq::HalfPair, Owed::AdoptHalfField);  // what the solve_field that follows has to do: adopt the half-step field
  }
  if (c->seq == Seq::Push1 && pred_usable(c, s)) {
    if (int rc = save_step_start_field(c)) return rc;
    if (int rc = set_call_state(c, Seq::Half, Owed::Nothing)) return rc;   // (a stale AdoptHalfField ends here)
    Span tm(c->tm, PIC1DP_IWT_COLLECT_CHARGE, c->tm.timers_on);
    if (int rc = pred_to_chargeden(c, s, c->fa, c->cfg.lazy_calls != 0)) return rc;
    return tm.end();
  }
  c->cd_kept_mode_only = false;  // a deposit follows: the whole vector again
  if (c->owed == Owed::AdoptHalfField)   // (left over by an inspection that settled a pair before its solve_field: void now)
    if (int rc = set_owed(c, Owed::Nothing)) return rc;
  const bool noted = lz_of(c->seq) == LZ_PUSH1 || lz_of(c->seq) == LZ_PUSH2;
  if (noted)
    if (int rc = deposit_or_step(c, s)) return rc;
  Span tm(c->tm, PIC1DP_IWT_COLLECT_CHARGE, c->tm.timers_on);
  if (!noted)
    if (int rc = deposit_or_step(c, s)) return rc;
  if (c->charge_sum == 1)  // exact sums over ranks, into the species accumulators: what follows is the one-rank path
    if (int rc = fx_settle(c)) return rc;
  const bool multi = fp64_rank_sum(c);
  if (multi)
    if (int rc = reduce_charge(c)) return rc;
  if (c->cfg.lazy_calls) {  // the species sum (one rank) and the scaling: in the launch of the solve_field that follows
    if (int rc = set_owed(c, multi ? Owed::Scale : Owed::SumScale)) return rc;
  } else {
    HIP_TRY(launch_chargeden(c->fa, !multi, c->st));
  }
  return tm.end();
}

int pic1dp_hip_set_field_solver(pic1dp_ctx *c, int32_t kind) {
  CHECK_CTX(c);
  if (kind != 0 && kind != 1) return fail(PIC1DP_ERR_ARG, "field solver must be 0 (reference mode filter) or 1 (finite differences)");
  if (kind == 1 && (c->in.nx < 3 || c->in.nx > 4096))
    return fail(PIC1DP_ERR_ARG, "the finite-difference solver needs 3 <= nx <= 4096");
  if (c->owed == Owed::AdoptHalfField && kind != c->field_solver) {  // a half-step field of the OTHER solver waits to be adopted:
    HIP_TRY(hipSetDevice(c->device));                                // the half-step charge is deposited for real instead
    if (int rc = rebuild_half_step_chargeden(c)) return rc;
    if (int rc = set_owed(c, Owed::Nothing)) return rc;
  }
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
  if (c->owed == Owed::AdoptHalfField && transform != c->field_transform) {  // a half-step field of the OTHER transform waits
    if (int rc = rebuild_half_step_chargeden(c)) return rc;                // to be adopted: the half-step charge is deposited
    if (int rc = set_owed(c, Owed::Nothing)) return rc;                    // for real instead
  }
  c->field_transform = transform;
  return 0;
}

static int solve_field_call(pic1dp_ctx *c);
int pic1dp_hip_solve_field(pic1dp_ctx *c) {
  CHECK_CTX(c);
  HIP_TRY(hipSetDevice(c->device));
  if (int rc = solve_field_call(c)) return rc;
  call_phase_solve(c);   // (only a solve_field that was served moves the record on)
  return 0;
}

static int solve_field_call(pic1dp_ctx *c) {
  if (c->seq == Seq::HalfPair) {  // the half-step field is solved already (the pair below): nothing to launch
    if (int rc = set_call_state(c, Seq::HalfPairSolved, Owed::Nothing)) return rc;
    c->cnt.call_pair_skips++;
    field_written(c, true);  // from now on field_electric IS the half-step field, as far as anybody can tell
    return 0;
  }
  if (int rc = settle_half_pair(c)) return rc;
  // a noted push has to see the field of its own moment
  if (lz_of(c->seq) == LZ_PUSH1 || lz_of(c->seq) == LZ_PUSH2)
    if (int rc = materialize(c)) return rc;
  const Step s = facts_of(c);
  Span tm(c->tm, PIC1DP_IWT_FIELD_ELECTRIC, c->tm.timers_on);
  FieldArgs f = c->fa;
  Owed pending = c->owed;  // what collect_charge left to this launch
  if (int rc = set_owed(c, Owed::Nothing)) return rc;
  if (pending == Owed::AdoptHalfField && c->adopt_cd_version != c->cd_version)  // (made for a charge density since overwritten:
    pending = Owed::Nothing;                                                     // check_state refuses that state; a safety net)
  // One rank, behind the collect_charge of push(2) whose kernel has predicted the next half-step charge: BOTH fields in
  // one launch, as pic1dp_hip_step solves them -- the next step's push(1), collect_charge, solve_field then launch nothing
  // and a time step through the three call sites is two launches (round 5; three and a copy before)
  if (pending == Owed::SumScale && s.k.pair_in_solve_field && c->seq == Seq::Clean && pred_usable(c, s)) {
    HIP_TRY(launch_field_solve_pair(f, pair_args(c), nullptr, c->st));
    pair_solved(c);
    return tm.end();
  }
  if (pending == Owed::AdoptHalfField) {  // (the fast path above was left by an inspection in between: the field is adopted by copying)
    if (int rc = adopt_half_field(c)) return rc;
  } else if (pending == Owed::PredTiles && s.k.dft_paths) {
    HIP_TRY(launch_field_solve_pred(f, c->d_pred, c->in.nmode, c->st));
  } else if (pending == Owed::PredSums && s.k.dft_paths) {
    HIP_TRY(launch_field_solve_pred_sums(f, c->pred_tab, c->d_pred, c->st));
  } else {
    if (pending == Owed::PredSums) HIP_TRY(launch_pred_chargeden(c->fa, c->pred_tab, c->d_pred, nullptr, c->st));
    if (pending == Owed::PredTiles) HIP_TRY(launch_pred_combine(c->fa, c->d_pred, c->in.nmode, c->st));
    if (int rc = enqueue_field_solve(c, f, pending == Owed::SumScale, pending == Owed::Nothing || pending == Owed::PredSums)) return rc;
  }
  field_written(c, true);
  return tm.end();
}

int pic1dp_hip_push(pic1dp_ctx *c, int32_t irk) {
  CHECK_CTX(c);
  if (irk != 1 && irk != 2) return fail(PIC1DP_ERR_ARG, "irk must be 1 or 2");
  if (int rc = require_loaded_keep_lazy(c)) return rc;
  int rc;
  if (irk == 1 && c->seq == Seq::Clean && lazy_ok(facts_of(c).k, optimize_due_any(c))) rc = set_seq(c, Seq::Push1);
  else if (irk == 2 && lz_of(c->seq) == LZ_HALF) rc = set_seq(c, push2_noted(c->seq));
  else if ((rc = materialize(c)) == 0) rc = enqueue_push(c, irk, false);
  if (rc == 0) call_phase_push(c, irk);   // (a push that failed has opened nothing)
  return rc;
}

int pic1dp_hip_substep(pic1dp_ctx *c, int32_t irk) {
  CHECK_CTX(c);
  if (irk != 1 && irk != 2) return fail(PIC1DP_ERR_ARG, "irk must be 1 or 2");
  if (int rc = require_loaded(c)) return rc;
  if (int rc = substep_impl(c, facts_of(c), irk, false)) return rc;
  c->call_phase = irk == 1 ? 3 : 0;   // (push, collect_charge and solve_field of the sub-step in one)
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

// field_chargeden as the reference holds it between the sub-steps, when the collect_charge after a noted push(1)
// was served from the six sums (the kept mode's content only): the half-step state is pushed into memory after all
// (as every inspection of a noted push does) and deposited for real.  One rank only -- on several ranks the
// reduction is a collective that an inspection on one of them must not start: there chargeden keeps the kept
// mode's content (include/pic1dp_hip.h says so).  The field solved from either is the same to rounding: the
// solve only looks at the kept mode.
int pic1dp_host::rebuild_half_step_chargeden(pic1dp_ctx *c) {
  // the flag is cleared only when the vector has actually been rebuilt: on several ranks, or when the
  // markers have left the half-step state through calls outside the sequence, chargeden keeps the kept mode's
  // content and pic1dp_hip_chargeden_state says so
  if (several_ranks(c)) return 0;
  if (lz_of(c->seq) != LZ_HALF && lz_of(c->seq) != LZ_PUSH2) return 0;
  if (int rc = settle_half_pair(c)) return rc;
  // the vector becomes the whole half-step charge density, and a solve from it is what the eager solve_field does: a half-step
  // field owed for adoption is dropped (its copy of the kept mode's content would overwrite the whole vector, flag "full")
  if (c->owed == Owed::AdoptHalfField)
    if (int rc = set_owed(c, Owed::Nothing)) return rc;
  const bool push2_was_noted = lz_of(c->seq) == LZ_PUSH2;
  if (int rc = enqueue_push(c, 1, false, c->d_E0)) return rc;
  if (int rc = set_seq(c, Seq::Clean)) return rc;  // memory now holds the half-step state (x not yet wrapped): the deposit wraps and stores it
  if (int rc = enqueue_deposit(c)) return rc;
  if (c->charge_sum == 1)
    if (int rc = fx_settle(c)) return rc;
  HIP_TRY(launch_chargeden(c->fa, true, c->st));
  c->cd_kept_mode_only = false;
  // a push(2) that had been noted: memory as the eager calls would have left it (the field it sees, d_E, is the one
  // solve_field wrote after the half step)
  if (push2_was_noted)
    if (int rc = enqueue_push(c, 2, false)) return rc;
  return 0;
}

// ---------------------------------------------------------------------------
// split-phase deposit
// ---------------------------------------------------------------------------
int pic1dp_hip_charge_local(pic1dp_ctx *c, double *charge2) {
  CHECK_CTX(c);
  if (!charge2) return fail(PIC1DP_ERR_ARG, "null array");
  if (c->charge_sum == 1) return fail(PIC1DP_ERR_STATE, "exact charge sum: a sum of doubles over ranks cannot be exact; use charge_local_exact");
  if (int rc = require_loaded_keep_lazy(c)) return rc;
  const Step s = facts_of(c);
  if (pair_of(c->seq) && c->seq != Seq::Push2PairSolved)  // out of sequence (as in collect_charge): memory as the eager calls leave it
    if (int rc = settle_half_pair(c)) return rc;
  if (c->owed == Owed::AdoptHalfField)   // (left over by a pair settled before its solve_field: void now)
    if (int rc = set_owed(c, Owed::Nothing)) return rc;
  if (c->seq == Seq::Push1 && pred_usable(c, s)) {  // predicted by the previous step's kernel: no marker pass
    if (int rc = save_step_start_field(c)) return rc;
    if (int rc = set_seq(c, Seq::Half)) return rc;
    if (c->plan.pred_kind == 2) {  // the six sums in charge2[0..5], zeros behind: the host's sum over ranks sums them
      HIP_TRY(launch_pred_to_charge(c->fa, c->d_pred, c->st));
      c->charge_pending_pred = true;
    } else {
      HIP_TRY(launch_pred_combine(c->fa, c->d_pred, c->in.nmode, c->st));
    }
    c->pred_version = 0;
  } else {
    c->cd_kept_mode_only = false;
    if (int rc = deposit_or_step(c, s)) return rc;
    HIP_TRY(launch_charge_local(c->fa, c->st));
  }
  HIP_TRY(hipStreamSynchronize(c->st));
  HIP_TRY(hipMemcpy(charge2, c->d_charge, sizeof(double) * c->in.nx, hipMemcpyDeviceToHost));
  c->charge_pending = true;
  return 0;
}

int pic1dp_hip_charge_reduced(pic1dp_ctx *c, const double *charge1) {
  CHECK_CTX(c);
  if (!charge1) return fail(PIC1DP_ERR_ARG, "null array");
  if (c->charge_sum == 1) return fail(PIC1DP_ERR_STATE, "exact charge sum: a sum of doubles over ranks cannot be exact; use charge_reduced_exact");
  if (!c->charge_pending) return fail(PIC1DP_ERR_STATE, "charge_reduced without charge_local");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpy(c->d_charge, charge1, sizeof(double) * c->in.nx, hipMemcpyHostToDevice));
  c->charge_pending = false;
  call_phase_collect(c);
  c->cd_version++;
  if (c->charge_pending_pred) {  // what came back are the summed prediction sums
    c->charge_pending_pred = false;
    c->cd_kept_mode_only = true;
    HIP_TRY(launch_pred_chargeden(c->fa, c->pred_tab, nullptr, c->d_charge, c->st));
    return 0;
  }
  if (c->cfg.lazy_calls) return set_owed(c, Owed::Scale);
  HIP_TRY(launch_chargeden(c->fa, false, c->st));
  return 0;
}

// kind 1 of the charge sum: the split phase with integers (include/pic1dp_hip.h has the layout)
int pic1dp_hip_charge_local_exact(pic1dp_ctx *c, int64_t *limbs) {
  CHECK_CTX(c);
  if (!limbs) return fail(PIC1DP_ERR_ARG, "null array");
  if (c->charge_sum != 1) return fail(PIC1DP_ERR_STATE, "charge_local_exact needs the exact charge sum (set_charge_sum(1))");
  if (int rc = require_loaded_keep_lazy(c)) return rc;
  c->cd_kept_mode_only = false;
  if (int rc = deposit_or_step(c, facts_of(c))) return rc;
  const size_t n = 2 * static_cast<size_t>(c->in.nspecies) * c->in.nx;
  HIP_TRY(launch_fx_normalise(c->d_fx, c->in.nspecies, c->in.nx, c->st));
  HIP_TRY(hipMemcpyAsync(limbs, c->d_fx, sizeof(int64_t) * n, hipMemcpyDeviceToHost, c->st));
  HIP_TRY(hipMemsetAsync(c->d_fx, 0, sizeof(int64_t) * n, c->st));
  HIP_TRY(hipStreamSynchronize(c->st));
  if (int rc = fx_check(c)) return rc;  // (a contribution left out: no charge to hand out)
  c->charge_pending = true;
  return 0;
}

int pic1dp_hip_charge_reduced_exact(pic1dp_ctx *c, const int64_t *limbs) {
  CHECK_CTX(c);
  if (!limbs) return fail(PIC1DP_ERR_ARG, "null array");
  if (c->charge_sum != 1) return fail(PIC1DP_ERR_STATE, "charge_reduced_exact needs the exact charge sum (set_charge_sum(1))");
  if (!c->charge_pending) return fail(PIC1DP_ERR_STATE, "charge_reduced_exact without charge_local_exact");
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = 2 * static_cast<size_t>(c->in.nspecies) * c->in.nx;
  HIP_TRY(hipMemcpy(c->d_fx, limbs, sizeof(int64_t) * n, hipMemcpyHostToDevice));
  c->charge_pending = false;
  call_phase_collect(c);
  c->cd_version++;
  HIP_TRY(launch_fx_to_rho(c->d_fx, c->fa.rho_sp, c->in.nspecies, c->in.nx, c->fx_q, c->st));
  if (c->cfg.lazy_calls) return set_owed(c, Owed::SumScale);
  HIP_TRY(launch_chargeden(c->fa, true, c->st));
  return 0;
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
                  static_cast<int>(c->seq), static_cast<int>(c->owed));                                   \
  } while (0)
  // The call sites' state is one (Seq, Owed) pair written by set_call_state alone, which refuses the pairs that cannot
  // occur (ctx.hpp kCallStateLegal): what used to be a dozen relations between lz, cd_lazy, half_pair and half_solved
  // checked here cannot be violated any more.  What is left relates the state to the CONTEXT it is held in:
  const bool one_rank = !several_ranks(c);
  const Step s = facts_of(c);
  const bool six_sums_one_mode = s.k.six_sums_one_mode;
  INVARIANT(kCallStateLegal[static_cast<int>(c->seq)][static_cast<int>(c->owed)]);
  INVARIANT(c->seq == Seq::Clean || (c->cfg.lazy_calls && c->loaded));    // a push is only noted by the lazy call sites
  INVARIANT(c->owed == Owed::Nothing || c->cfg.lazy_calls);
  INVARIANT(c->owed < Owed::SumScale || one_rank || c->charge_sum == 1);  // species sum / prediction left to solve_field: one rank
                                                                      // (or exact sums, already summed over ranks)
  // kind 1 of the charge sum: no prediction pending, no tiles, sums or half-step field owed
  INVARIANT(c->charge_sum == 0 || c->pred_version == 0);
  INVARIANT(c->charge_sum == 0 || (c->owed != Owed::PredTiles && c->owed != Owed::PredSums && c->owed != Owed::AdoptHalfField &&
                                   !pair_of(c->seq)));
  INVARIANT(c->owed != Owed::PredTiles || c->plan.pred_kind == 1);
  INVARIANT((c->owed != Owed::PredSums && c->owed != Owed::AdoptHalfField && !pair_of(c->seq)) || six_sums_one_mode);
  INVARIANT(!pair_of(c->seq) || (s.f.cfg->call_pair && c->eh_version == c->state_version));   // the field in d_Ehn belongs to the state in memory
  INVARIANT(!c->cd_kept_mode_only || c->plan.pred_kind == 2);
  // an owed adoption is current: made for the field_chargeden the eager calls hold now (and, by kCallStateLegal, while the
  // markers still stand at the half step)
  INVARIANT(c->owed != Owed::AdoptHalfField || c->adopt_cd_version == c->cd_version);
  INVARIANT(!c->e_step_start || (c->seq == Seq::Clean && c->eh_modes == 2));   // (the half-step field: d_Eh / d_mode_h)
  // whole-step path: nothing of a step() is left over between calls
  INVARIANT(!c->fused_pending);
  // the call record: a noted push lies inside a time step (checkpoint_write goes by the record alone)
  INVARIANT(c->call_phase >= 0 && c->call_phase <= 5);
  INVARIANT(lz_of(c->seq) == LZ_CLEAN || c->call_phase != 0);
  INVARIANT(c->fuse_args.on == 0);
  INVARIANT(c->fused_dirty == -1);
  INVARIANT(c->tail_done == 0);
  INVARIANT(c->acc_idx >= 0 && c->acc_idx < 3);
  // versions only ever point backwards
  INVARIANT(c->pred_version <= c->state_version);
  INVARIANT(c->eh_version <= c->state_version);
  INVARIANT(c->eh_field_version <= c->field_version);
  INVARIANT(c->modes_field_version <= c->field_version);
  INVARIANT(c->eh_modes >= 0 && c->eh_modes <= 2);
  for (int s = 0; s < c->in.nspecies; ++s) {
    INVARIANT(c->diag[s].version <= c->state_version);
    INVARIANT(c->sp[s].t2_version <= c->state_version);
  }
  INVARIANT(!c->charge_pending_pred || c->charge_pending);
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
    else if (c->owed != Owed::SumScale && c->owed != Owed::PredTiles && !c->charge_pending) INVARIANT(!nz && "deposits nobody is going to sum");
  }
  if (c->d_pred_all && c->plan.pred_set_doubles) {
    h.assign(3 * c->plan.pred_set_doubles, 0.0);
    HIP_TRY(hipMemcpy(h.data(), c->d_pred_all, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; ++k) {
      const bool nz = nonzero(h, k * c->plan.pred_set_doubles, c->plan.pred_set_doubles);
      if (k != c->acc_idx) INVARIANT(!nz && "a prediction accumulator set that is not the current one holds sums");
      else if (c->pred_version == 0 && c->owed != Owed::PredTiles && c->owed != Owed::PredSums && !c->charge_pending)
        INVARIANT(!nz && "prediction sums that belong to no state");
    }
  }
#undef INVARIANT
  return 0;
}
