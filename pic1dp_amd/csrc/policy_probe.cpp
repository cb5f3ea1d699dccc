// policy_probe.cpp -- the launch policy (launch_policy.hpp), the LDS layouts of the field kernels (field_lds.hpp) and the
// decisions of create() (settings.hpp, context_plan.hpp) behind the C ABI of the probe library, for the host tests that pin
// them (tests/test_launch_policy_host.py, tests/test_field_lds_host.py, tests/test_diag_launch_host.py,
// tests/test_context_plan_host.py, tests/test_step_plan_host.py, tests/test_call_plan_host.py, tests/test_moments_host.py, tests/test_moments_exact_host.py, tests/test_load_device_host.py), and the layout of a species' blocks (block_layout.hpp; tests/test_block_layout_host.py).  Test support (libpic1dp_probe.so), no GPU needed.
#include <cmath>
#include <cstdio>

#include "../../include/pic1dp_probe.h"
#include "block_layout.hpp"
#include "call_plan.hpp"
#include "context_plan.hpp"
#include "field_lds.hpp"
#include "launch_policy.hpp"
#include "step_plan.hpp"

using namespace pic1dp;

extern "C" int pic1dp_probe_host_launch_shape(const pic1dp_probe_launch_query *q, int64_t shape[4]) {
  if (!q || !shape) return 1;
  const LaunchPolicy p{q->num_cu, q->threads_req, q->bpc_req, q->osub_req};
  PredLaunch pl{};
  switch (q->family) {
    case 0: pl.lc = particle_launch(p, q->nx, q->np, q->with_E != 0, q->with_rho != 0, q->exact != 0); break;
    case 1: pl.lc = step_launch(p, q->nx, q->np, q->full != 0, q->exact != 0); break;
    case 2: pl.lc = step_diag_launch(p, q->nx, q->np, q->exact != 0, q->nx_opd, q->nv_opd); break;
    case 3: pl = pred_launch(p, q->nx, q->nmode, q->np, q->priv != 0, q->pred_kind, q->exp_bearing != 0); break;
    default: return 1;
  }
  shape[0] = pl.lc.threads;
  shape[1] = pl.lc.blocks;
  shape[2] = static_cast<int64_t>(pl.lc.lds);
  shape[3] = pl.resident;
  return 0;
}

extern "C" int pic1dp_probe_host_field_lds(int32_t family, int32_t nx, int32_t nmode, int32_t npe, int32_t tab_lds,
                                           int32_t with_xchg, int32_t pred_kind, int64_t out[3]) {
  if (!out) return 1;
  FieldLaunch fl{};
  switch (family) {
    case 0: fl = solve_launch(nx, nmode, tab_lds != 0); break;
    case 1: fl = pair_launch(nx, nmode, npe, tab_lds != 0, with_xchg != 0, pred_kind); break;
    default: return 1;
  }
  out[0] = static_cast<int64_t>(fl.bytes);
  out[1] = fl.threads;
  out[2] = fl.family;
  return 0;
}

extern "C" int pic1dp_probe_host_diag_launch(int32_t kind, int64_t np, int32_t nx_opd, int32_t nv_opd, int32_t num_cu,
                                             int64_t ntail, int64_t out[6]) {
  if (!out || (kind != 0 && kind != 1)) return 1;
  const DiagLaunch d = diag_launch(kind, np, nx_opd, nv_opd, num_cu);
  out[0] = d.blocks;
  out[1] = d.threads;
  out[2] = d.lds;
  out[3] = static_cast<int64_t>(d.bytes);
  out[4] = d.nt;
  out[5] = tail_sum_blocks(ntail);
  return 0;
}

extern "C" int pic1dp_probe_host_load_launch(int64_t nalloc, int32_t num_cu, int64_t out[4]) {
  if (!out || nalloc < 0 || num_cu < 1) return 1;
  const LoadLaunch l = load_launch(nalloc, num_cu);
  out[0] = l.blocks;
  out[1] = l.threads;
  out[2] = l.nt;
  out[3] = LOAD_CHUNK;
  return 0;
}

extern "C" int pic1dp_probe_host_block_layout(const int64_t *blk_alloc, const int64_t *blk_np, int32_t nblk, int64_t *out, int64_t *np) {
  if (!blk_alloc || !blk_np || !out || !np || nblk < 1) return 1;
  const BlockLayout L = block_layout(std::vector<int64_t>(blk_alloc, blk_alloc + nblk), std::vector<int64_t>(blk_np, blk_np + nblk));
  for (int b = 0; b < nblk; ++b) {
    const int64_t v[4] = {L.blk[b].voff, L.blk[b].np, L.blk[b].toff, L.blk[b].ntail};
    for (int k = 0; k < 4; ++k) out[4 * b + k] = v[k];
  }
  *np = L.np;
  return 0;
}

extern "C" int pic1dp_probe_host_plain_chunks(int64_t np_all_species, int64_t np_species, int32_t nt, int64_t *chunks) {
  if (!chunks || np_all_species < 0 || np_species < 0) return 1;
  *chunks = stream_plain_chunks(np_all_species, np_species, nt != 0);
  return 0;
}

static int moments_plan_words(const MomentsPlan &m, int64_t out[35]) {
  if (!out) return 1;
  for (int i = 0; i < 35; ++i) out[i] = 0;
  out[0] = m.npass, out[1] = m.selected, out[2] = m.group;
  for (int i = 0; i < m.npass; ++i) {
    const MomentsPass &ps = m.pass[i];
    const int64_t v[8] = {ps.blocks, ps.threads, ps.nt, static_cast<int64_t>(ps.bytes), (ps.p ? 1 : 0) | (ps.w ? 2 : 0), ps.kmask,
                          ps.first_plane, ps.planes};
    for (int k = 0; k < 8; ++k) out[3 + 8 * i + k] = v[k];
  }
  return 0;
}

extern "C" int pic1dp_probe_host_moments_plan(int32_t nx, int32_t which, int32_t deltaf, int64_t np, int32_t num_cu, int64_t out[35]) {
  return moments_plan_words(moments_plan(nx, which, deltaf, np, num_cu), out);
}

extern "C" int pic1dp_probe_host_moments_plan_exact(int32_t nx, int32_t which, int32_t deltaf, int64_t np, int32_t num_cu,
                                                    int64_t out[35]) {
  return moments_plan_words(moments_plan_exact(nx, which, deltaf, np, num_cu), out);
}

static int power_plan_words(const PowerPlan &m, int64_t out[20]) {
  if (!out) return 1;
  for (int i = 0; i < 20; ++i) out[i] = 0;
  out[0] = m.npass, out[1] = m.selected, out[2] = static_cast<int64_t>(m.tile), out[3] = static_cast<int64_t>(m.plane);
  for (int i = 0; i < m.npass; ++i) {
    const PowerPass &ps = m.pass[i];
    const int64_t v[8] = {ps.blocks, ps.threads, ps.nt, static_cast<int64_t>(ps.bytes), (ps.p ? 1 : 0) | (ps.w ? 2 : 0), ps.lds,
                          ps.first_set, ps.sets};
    for (int k = 0; k < 8; ++k) out[4 + 8 * i + k] = v[k];
  }
  return 0;
}

extern "C" int pic1dp_probe_host_power_plan(int32_t nx, int32_t nx_opd, int32_t nv_opd, int32_t which, int32_t deltaf, int64_t np,
                                            int32_t num_cu, int64_t out[20]) {
  return power_plan_words(power_plan(nx, nx_opd, nv_opd, which, deltaf, np, num_cu), out);
}

extern "C" int pic1dp_probe_host_power_plan_exact(int32_t nx, int32_t nx_opd, int32_t nv_opd, int32_t which, int32_t deltaf, int64_t np,
                                                  int32_t num_cu, int64_t out[20]) {
  return power_plan_words(power_plan_exact(nx, nx_opd, nv_opd, which, deltaf, np, num_cu), out);
}

extern "C" int pic1dp_probe_host_zoom_plan(int32_t nxb, int32_t nvb, int32_t which, int32_t deltaf, int64_t np, int32_t num_cu,
                                           int32_t pass_cap, int64_t out[515]) {
  if (!out) return 1;
  const ZoomPlan m = zoom_plan(nxb, nvb, which, deltaf, np, num_cu, pass_cap > 0 ? pass_cap : kZoomPassCap);
  for (int i = 0; i < 515; ++i) out[i] = 0;
  out[0] = m.npass, out[1] = m.selected, out[2] = kZoomPassCap;
  for (int i = 0; i < m.npass; ++i) {
    const ZoomPass &ps = m.pass[i];
    const int64_t v[8] = {ps.blocks, ps.threads, ps.nt, static_cast<int64_t>(ps.bytes), ps.planes, ps.lds, ps.first_row, ps.rows};
    for (int k = 0; k < 8; ++k) out[3 + 8 * i + k] = v[k];
  }
  return 0;
}

extern "C" int pic1dp_probe_host_hermite_plan(int32_t nherm, int32_t nmodes, int32_t which, int32_t deltaf, int64_t np, int32_t num_cu,
                                               int64_t out[6]) {
  if (!out) return 1;
  const HermitePlan h = hermite_plan(nherm, nmodes, which, deltaf, np, num_cu);
  const int64_t v[6] = {h.blocks, h.threads, h.nt, static_cast<int64_t>(h.bytes), h.nb, h.partials};
  for (int k = 0; k < 6; ++k) out[k] = v[k];
  return 0;
}

extern "C" int pic1dp_probe_host_select_plan(int64_t np, int32_t num_cu, int32_t threads_req, int32_t bpc_req, int64_t out[6]) {
  if (!out) return 1;
  const SelectPlan s = select_plan(np, num_cu, threads_req, bpc_req);
  const int64_t v[6] = {s.chunk_pairs, s.nchunk, s.blocks, s.threads, s.nt, s.scan_threads};
  for (int k = 0; k < 6; ++k) out[k] = v[k];
  return 0;
}

extern "C" int pic1dp_probe_host_dist_scale(int64_t np, int32_t blocks, int32_t deltaf, double bound_p, double bound_w,
                                            int32_t threads, int32_t out[4]) {
  if (!out) return 1;
  DistScale fx{};
  out[0] = make_dist_scale(np, blocks, deltaf != 0, bound_p, bound_w, &fx, threads);
  for (int k = 0; k < 3; ++k) out[1 + k] = fx.sc[k] > 0.0 ? std::ilogb(fx.sc[k]) : 0;
  return 0;
}

extern "C" int pic1dp_probe_host_context_plan(const pic1dp_input *in, const pic1dp_layout *lay, int32_t pred_kind_req,
                                              int32_t gcopies_req, int32_t one_rank_order, int64_t *out, int64_t cap,
                                              double sc[2]) {
  if (!in || !lay || !out || !sc || in->nspecies < 1 || in->nspecies > PIC1DP_MAX_SPECIES || lay->nranks < 1) return 1;
  Settings cfg;
  cfg.pred_kind_req = pred_kind_req;
  cfg.gcopies_req = accepted_gcopies(gcopies_req);  // (as settings_from_env takes it)
  cfg.field_one_rank_order = one_rank_order;
  const ContextPlan p = plan_context(*in, *lay, cfg);
  const int ns = in->nspecies;
  if (cap < 16 + ns + static_cast<int64_t>(p.nblk) * (1 + ns)) return 1;
  const int64_t head[16] = {p.npe, p.nblk, p.blk0, p.nalloc, p.imerge, p.iremove, p.isplit, p.gcopies, p.gstride,
                            static_cast<int64_t>(p.rho_set_doubles), p.pred_kind, p.pred_private,
                            static_cast<int64_t>(p.pred_set_doubles), static_cast<int64_t>(p.pack_doubles), p.tab_lds, p.field_npe};
  int64_t *o = out;
  for (int64_t v : head) *o++ = v;
  for (int s = 0; s < ns; ++s) *o++ = p.np[s];
  for (int b = 0; b < p.nblk; ++b) *o++ = p.blk_alloc[b];
  for (int s = 0; s < ns; ++s)
    for (int b = 0; b < p.nblk; ++b) *o++ = p.blk_np[s][b];
  sc[0] = p.sc_re, sc[1] = p.sc_im;
  return 0;
}

extern "C" int pic1dp_probe_host_settings(int32_t iv[15], double dv[3]) {
  if (!iv || !dv) return 1;
  const Settings s = settings_from_env();
  const int32_t v[15] = {s.fuse_solve, s.tail_on, s.call_pair, s.lazy_calls, s.predict, s.carry, s.osub_req, s.dyn_tail,
                         s.dyn_tail_full, s.diag_fx, s.pred_kind_req, s.chain_mfma_req, s.gcopies_req, s.field_one_rank_order,
                         s.chain_selftest_verbose};
  for (int i = 0; i < 15; ++i) iv[i] = v[i];
  dv[0] = s.nt_threshold_half, dv[1] = s.nt_threshold_full, dv[2] = s.diag_fx_margin_w;
  return 0;
}

extern "C" int pic1dp_probe_host_step_plan(const pic1dp_input *in, const pic1dp_layout *lay, const pic1dp_probe_step_query *q,
                                           int64_t out[112], char names[8][64]) {
  if (!in || !lay || !q || !out || !names || in->nspecies < 1 || in->nspecies > PIC1DP_MAX_SPECIES || lay->nranks < 1) return 1;
  Settings cfg;
  cfg.fuse_solve = q->fuse_solve, cfg.tail_on = q->tail_on, cfg.call_pair = q->call_pair, cfg.lazy_calls = q->lazy_calls;
  cfg.predict = q->predict, cfg.carry = q->carry, cfg.osub_req = q->osub_req, cfg.dyn_tail = q->dyn_tail, cfg.dyn_tail_full = q->dyn_tail_full;
  cfg.pred_kind_req = q->pred_kind_req, cfg.gcopies_req = accepted_gcopies(q->gcopies_req), cfg.field_one_rank_order = q->one_rank_order;
  if (q->nt_threshold_half > 0.0) cfg.nt_threshold_half = q->nt_threshold_half;
  if (q->nt_threshold_full > 0.0) cfg.nt_threshold_full = q->nt_threshold_full;
  const ContextPlan plan = plan_context(*in, *lay, cfg);
  StepFacts f{};
  f.in = in, f.plan = &plan, f.cfg = &cfg;
  f.pol = LaunchPolicy{q->num_cu, q->threads_req, q->bpc_req, cfg.osub_req};
  f.charge_sum = q->charge_sum, f.diag_sum = q->diag_sum, f.fuse_output = q->fuse_output;
  f.step_mode = q->step_mode, f.field_solver = q->field_solver, f.field_transform = q->field_transform;
  f.several_ranks = lay->nranks > 1 || q->comm != 0, f.xchg_active = q->xchg != 0, f.has_comm = q->comm != 0;
  f.field_npe = q->field_npe > 0 ? q->field_npe : plan.field_npe, f.chain_mfma = q->chain_mfma;
  f.has_pred = q->has_pred < 0 ? plan.pred_kind != 0 : q->has_pred != 0;
  for (int s = 0; s < in->nspecies; ++s)
    f.np[s] = q->np[s] < 0 ? plan.np[s] : q->np[s], f.pow2[s] = q->pow2[s] != 0, f.one_exp[s] = q->one_exp[s] != 0;
  const StepCaps k = step_caps(f);
  const MarkerPlan m = plan_markers(f, k, q->full != 0, q->diag != 0, q->pred != 0, q->tail_ok != 0, q->eh_modes, q->nt_force);
  const SolvePlan sp = plan_solve(f, k, q->pred_fresh != 0, q->tail_done, q->into_E != 0);
  const StepMoment mo{q->pending != 0, q->have_eh != 0, q->steps_left, q->output_now != 0, q->output_next != 0, q->optimize_now != 0,
                      q->optimize_next != 0};
  const WholeStepPlan w = plan_whole_step(f, k, mo);
  int64_t *o = out;
  for (int64_t v : {int64_t(k.dft_paths), int64_t(k.six_sums_one_mode), int64_t(k.modes_fit_field_kernel), int64_t(k.exp_bearing),
                    int64_t(k.step_recompute_ok), int64_t(k.predict_capable), int64_t(k.diag_in_step), int64_t(k.priv),
                    int64_t(k.fuse_capable), int64_t(k.lazy_calls_ok), int64_t(k.pair_serves_collect), int64_t(k.pair_in_solve_field),
                    int64_t(plan.pred_kind)})
    *o++ = v;
  for (int64_t v : {int64_t(m.pred), int64_t(m.priv), int64_t(m.diag), int64_t(m.tail_mode), int64_t(m.tail_species), int64_t(m.stream_nt),
                    int64_t(m.solve_species), int64_t(m.solve_fits), int64_t(m.solve_threads), int64_t(m.tag), int64_t(m.rd), int64_t(m.wr)})
    *o++ = v;
  for (int s = 0; s < 8; ++s) {
    const SpeciesLaunch &L = m.sp[s];
    for (int64_t v : {int64_t(L.launched), int64_t(L.family), int64_t(L.lc.threads), int64_t(L.lc.blocks), int64_t(L.lc.lds), int64_t(L.dyn_tail),
                      L.plain_chunks, int64_t(L.carry), int64_t(L.tail)})
      *o++ = v;
    std::snprintf(names[s], 64, "%s", L.name);
  }
  for (int64_t v : {int64_t(sp.refused), int64_t(sp.reduce_first), int64_t(sp.pack_reduce), int64_t(sp.pack_first), int64_t(sp.launch),
                    int64_t(sp.with_local)})
    *o++ = v;
  for (int64_t v : {int64_t(w.substeps), int64_t(w.finish_pending), int64_t(w.diag), int64_t(w.pred), int64_t(w.fused_in), int64_t(w.adopt_eh),
                    int64_t(w.half_pass), int64_t(w.half_eh_modes), int64_t(w.fuse_out)})
    *o++ = v;
  return 0;
}

extern "C" int pic1dp_probe_host_call_plan(const int32_t st[9], const int32_t mo[14], const int32_t caps[8], int32_t call, int32_t out[64]) {
  if (!st || !mo || !caps || !out || call < 0 || call >= static_cast<int>(Call::N)) return 1;
  CallState s;
  s.seq = static_cast<Seq>(st[0]), s.owed = static_cast<Owed>(st[1]);
  s.e_step_start = st[2] != 0, s.cd_kept_mode_only = st[3] != 0, s.adopt_current = st[4] != 0;
  s.charge_pending = st[5] != 0, s.charge_pending_pred = st[6] != 0;
  s.call_phase = static_cast<int8_t>(st[7]), s.eh_modes = static_cast<int8_t>(st[8]);
  CallMoment m;
  m.lazy_calls = mo[0] != 0, m.call_pair = mo[1] != 0, m.loaded = mo[2] != 0, m.several_ranks = mo[3] != 0, m.fp64_rank_sum = mo[4] != 0;
  m.charge_sum = mo[5], m.pred_kind = mo[6], m.tab_lds = mo[7] != 0;
  m.field_differs = mo[8] != 0, m.pred_usable = mo[9] != 0, m.eh_current = mo[10] != 0, m.modes_current = mo[11] != 0;
  m.optimize_due_any = mo[12] != 0, m.output_follows = mo[13] != 0;
  StepCaps k{};
  k.dft_paths = caps[0] != 0, k.six_sums_one_mode = caps[1] != 0, k.modes_fit_field_kernel = caps[2] != 0, k.predict_capable = caps[3] != 0;
  k.diag_in_step = caps[4] != 0, k.lazy_calls_ok = caps[5] != 0, k.pair_serves_collect = caps[6] != 0, k.pair_in_solve_field = caps[7] != 0;
  const CallPlan p = plan_call(s, m, k, static_cast<Call>(call));
  for (int i = 0; i < 64; ++i) out[i] = 0;
  const CallState &n = p.next;
  const int32_t head[14] = {static_cast<int32_t>(p.refusal), p.refused_after, static_cast<int32_t>(p.bad_seq), static_cast<int32_t>(p.bad_owed),
                            static_cast<int32_t>(n.seq), static_cast<int32_t>(n.owed), n.e_step_start, n.cd_kept_mode_only, n.adopt_current,
                            n.charge_pending, n.charge_pending_pred, n.call_phase, n.eh_modes, p.n};
  for (int i = 0; i < 14; ++i) out[i] = head[i];
  for (int i = 0; i < p.n; ++i) out[14 + 2 * i] = static_cast<int32_t>(p.act[i]), out[15 + 2 * i] = p.arg[i];
  out[63] = call_state_invariants(n, m, k) == nullptr;
  return 0;
}
