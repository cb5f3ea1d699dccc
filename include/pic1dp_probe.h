/* pic1dp_probe.h -- C ABI of libpic1dp_probe.so: MEASUREMENT and test support, not part of the drop-in boundary
 * (that is include/pic1dp_hip.h).  Streaming-rate probes with the marker kernels' access shapes, and array
 * evaluations of the device functions the marker kernels call, built from the same device headers as the product
 * library (pic1dp_amd/csrc/device_math.hpp).  Loaded by bench.py, tools/ and tests/ only (pic1dp_amd/probe.py).
 * All functions return 0 on success; pic1dp_probe_last_error() describes the last failure of the calling thread. */
#ifndef PIC1DP_PROBE_H
#define PIC1DP_PROBE_H

#include <stdint.h>

#include "pic1dp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *pic1dp_probe_last_error(void);

/* nread (1, 2, 4, 7) arrays of n doubles read and nwrite (0, 1, 3) written, 16 B per lane, grid-stride, reps launches
 * after one warm-up; variant 0 plain, 1 non-temporal (the marker kernels' accesses), 2 plain with two pairs per
 * lane.  blocks / threads 0: the sub-step kernels' launch shape (four workgroups of 512 per CU). */
int pic1dp_probe_stream(int32_t device, int32_t nread, int32_t nwrite, int64_t n, int32_t reps, int32_t blocks,
                        int32_t threads, int32_t variant, double *gbytes_per_s);

/* the traffic of the second sub-step's kernel (4 arrays read, 3 written back in place, non-temporal) over a fresh
 * slab of n markers: ms[0] four arrays apart (SoA, a 2 MiB multiple + stagger_bytes), ms[1] interleaved in tiles of
 * 2^log2_tile markers (the product's layout, src: pic1dp_amd/csrc/kernels.hpp), ms[2], ms[3] the same read-only,
 * ms[4], ms[5] tiled with one workgroup per tile.  keep != 0 leaves the slab allocated (the next call lands in
 * other physical memory) until pic1dp_probe_release.  blocks / threads 0: two workgroups of 768 per CU. */
int pic1dp_probe_layout(int32_t device, int64_t n, int32_t log2_tile, int64_t stagger_bytes, int32_t reps, int32_t keep,
                        int32_t blocks, int32_t threads, double ms[6]);
int pic1dp_probe_release(void);

/* launch pairs of the tiled read/write traffic above, back to back over ONE slab of n markers, in 64-pair chunks:
 * alternate 0 every launch forward, 1 forward and backward (mirrored chunk addresses) in turn, so that a launch starts
 * on the pairs the one before it ended on.  plain_bytes: the marker state (32 B per marker) at either slab end that
 * is accessed with plain loads and stores (head_only != 0: at the slab's head alone), the rest non-temporal; 0 non-temporal
 * everywhere, < 0 plain everywhere.
 * Two pairs of warm-up, then ms[t], t < trials: ms per LAUNCH over `pairs` pairs.  blocks / threads 0: two workgroups
 * of 768 per CU. */
int pic1dp_probe_sweep(int32_t device, int64_t n, int32_t log2_tile, int32_t alternate, int64_t plain_bytes, int32_t head_only,
                       int32_t pairs, int32_t trials, int32_t blocks, int32_t threads, double *ms);

/* x / lx by reciprocal + two FMA corrections (div_lx) against the IEEE division on n generated positions (cell
 * boundaries +- a few ulp, wide exponent range): *mismatches counts results that differ in any bit.  On the device,
 * and the same algorithm with the host's fma. */
int pic1dp_probe_div_lx(int32_t device, double lx, int32_t nx, int64_t n, uint64_t seed, int64_t *mismatches);
int pic1dp_probe_host_div_lx(double lx, int32_t nx, int64_t n, uint64_t seed, int64_t *mismatches);
/* a / divisor for a species constant (div_const), likewise */
int pic1dp_probe_div_const(int32_t device, double divisor, int64_t n, uint64_t seed, int64_t *mismatches);
int pic1dp_probe_host_div_const(double divisor, int64_t n, uint64_t seed, int64_t *mismatches);
/* the diagnostics' divisions (diag_div: positions by lx, v + v_max by 2 v_max, an nx_opd x nv_opd grid's boundaries
 * +- a few ulps, 0 and subnormal dividends included), likewise */
int pic1dp_probe_diag_div(int32_t device, double lx, int32_t nxo, double vmax, int32_t nvo, int64_t n, uint64_t seed,
                          int64_t *mismatches);
int pic1dp_probe_host_diag_div(double lx, int32_t nxo, double vmax, int32_t nvo, int64_t n, uint64_t seed, int64_t *mismatches);

/* The sequential walks of the GPU marker optimisation (pic1dp_amd/csrc/optimize.hpp plan_merge / plan_remove /
 * plan_split: one key per marker) against the routines on whole markers they restate (opt_merge / opt_remove /
 * opt_split, src/pic1dp_particle.F90:411-746), on the HOST: np generated markers in nalloc slots, the event (kind 0
 * merge, 1 remove, 2 split) applied both ways, *mismatches = slots that differ in v, p, w (and x inside the new count);
 * -1: the marker counts differ, -2: the random stream was consumed differently; *np_after (may be NULL) = the marker
 * count the routine leaves.  No GPU needed. */
int pic1dp_probe_host_optimize(int32_t kind, int32_t typeremove, int32_t nx, int32_t nv, int32_t split_ngroup, double threshold,
                               uint64_t seed, int64_t np, int64_t nalloc, int64_t *mismatches, int64_t *np_after);

/* (ix[i], wl[i]) = cell and left weight of position x[i] as the marker kernels' locate gives them, n <= 2^20 host
 * arrays, for a grid of nx cells over lx.  form 0: x / lx in five operations; form 1: in two operations where the host
 * proves them for this lx (GridConst::mul2), else five again.  *two_ops: 1 when the run took the two operations. */
int pic1dp_probe_locate(int32_t device, double lx, int32_t nx, int32_t form, const double *x, int32_t *ix, double *wl, int64_t n,
                        int32_t *two_ops);

/* y[i] = exp(x[i]) as the marker kernels evaluate it (pexp; host arrays) */
int pic1dp_probe_exp(int32_t device, const double *x, double *y, int64_t n);

/* the prediction tiles' raise of a fixed-point bound (pic1dp_amd/csrc/device_fx.hpp fx_raise), as the end of n workgroups
 * applies it: one device thread starts from *bound = bound0 and applies the events (noted[i], start[i]) in order -- noted:
 * the workgroup's code (0 no marker met, 1 none within the bound, 2 + the bits of a float: the largest value met within it),
 * start: the bound the workgroup started with.  *bound: the final value. */
int pic1dp_probe_fx_raise(int32_t device, double bound0, const uint32_t *noted, const double *start, int64_t n, double *bound);

/* one species of the input (src/pic1dp_input.F90:43-72) */
typedef struct pic1dp_probe_species {
  int32_t iptcldist;
  double charge, mass, temperature, temperature2, density, v0;
} pic1dp_probe_species;
/* which division short cuts and which form of -f0'/f0 the library would take for it, and the folded constants of
 * the one-exp form f = {fq2, fq1, fq0, fm1, fm0, fd1, fd0}: L(v) = (fq2 v + fq1) v + fq0,
 * -f0'/f0 = (fm1 v + fm0) + (fd1 v + fd0) tanh(L / 2) */
int pic1dp_probe_species_const(const pic1dp_probe_species *sp, int32_t *pow2, int32_t *unit, int32_t *fastc, int32_t *one_exp,
                               double f[7]);
/* y[i] = -f0'/f0 at v[i] as the marker kernels evaluate it (src/pic1dp_interaction.F90:274-326): form 0 in the
 * reference's operation order, form 1 the one-exp form (iptcldist 2, 3) */
int pic1dp_probe_dlnf0(int32_t device, const pic1dp_probe_species *sp, int32_t form, const double *v, double *y, int64_t n);

/* The launch shape the product library picks for a marker kernel (pic1dp_amd/csrc/launch_policy.hpp), on the HOST: no GPU
 * needed.  num_cu ... osub_req: the policy's view of the context; family: 0 sub-step kernels (with_E, with_rho, exact),
 * 1 whole-step kernels (full, exact), 2 k_step_full<DIAG> (exact, nx_opd, nv_opd), 3 one-pass kernels (priv, pred_kind,
 * nmode, exp_bearing: -f0'/f0 of the distribution bears an exp); fields a family does not name are ignored.
 * shape = {threads, blocks, dynamic LDS bytes, resident workgroups (family 3; 0 otherwise)}; a shape whose LDS exceeds
 * what a kernel may ask for is returned as it is.  Nonzero: null argument or unknown family (no message). */
typedef struct pic1dp_probe_launch_query {
  int32_t num_cu, threads_req, bpc_req, osub_req;
  int32_t family, nx, nmode;
  int64_t np;
  int32_t full, exact, with_E, with_rho, priv, pred_kind, exp_bearing, nx_opd, nv_opd;
} pic1dp_probe_launch_query;
int pic1dp_probe_host_launch_shape(const pic1dp_probe_launch_query *q, int64_t shape[4]);

/* The dynamic LDS and the workgroup size of a one-workgroup field launch (pic1dp_amd/csrc/field_lds.hpp: the layout the
 * kernel itself takes its pointers from), on the HOST: no GPU needed.  family 0: k_field_solve and its _pred, _pred_sums,
 * _xchg siblings (nx, nmode, tab_lds); family 1: what launch_field_solve_pair runs for (nx, nmode, npe, tab_lds, with_xchg:
 * the one-hop exchange inside the launch, pred_kind 1 tiles / 2 sums).  out = {bytes, threads, kernel: 0 k_field_solve...,
 * 1 k_field_solve_pair, 2 k_field_solve_pair1, 3 k_field_solve_pair_sums1}.  Nonzero: null argument or unknown family. */
int pic1dp_probe_host_field_lds(int32_t family, int32_t nx, int32_t nmode, int32_t npe, int32_t tab_lds, int32_t with_xchg,
                                int32_t pred_kind, int64_t out[3]);

/* The launch shape of a diagnostics pass of output_all (launch_policy.hpp diag_launch), on the HOST: kind 0 k_ptcldist,
 * 1 k_ptcldist_exact.  out = {blocks, threads, histograms in the LDS (1) or straight into memory (0), dynamic LDS bytes,
 * non-temporal loads, workgroups that sum ntail tail slots}.  Nonzero: null argument or unknown kind. */
int pic1dp_probe_host_diag_launch(int32_t kind, int64_t np, int32_t nx_opd, int32_t nv_opd, int32_t num_cu, int64_t ntail,
                                  int64_t out[6]);
/* The scales of a fixed-point diagnostics pass (kernels.hpp make_dist_scale), on the HOST: out = {1 fixed point / 0 double
 * sums, log2 of the scale of the planes markr, total, pertb}. */
int pic1dp_probe_host_dist_scale(int64_t np, int32_t blocks, int32_t deltaf, double bound_p, double bound_w, int32_t threads,
                                 int32_t out[4]);

/* The passes of one pic1dp_hip_moments call (launch_policy.hpp moments_plan), on the HOST: out[0] = passes (0: an unknown
 * `which`, w asked of a full-f run, nx out of range), out[1] = planes selected (4 or 8), out[2] = planes per pass (8, 4, 2),
 * then per pass i eight words at out[3 + 8 i]: {blocks, threads, non-temporal loads, dynamic LDS bytes, weight sets (bit 0
 * p, bit 1 w), powers of v (bit k: v^k), first plane in the output, planes}.  out holds 3 + 8 * 4 words.  Nonzero: null
 * argument. */
int pic1dp_probe_host_moments_plan(int32_t nx, int32_t which, int32_t deltaf, int64_t np, int32_t num_cu, int64_t out[35]);
/* ... and of one pic1dp_hip_moments_exact call (launch_policy.hpp moments_plan_exact): the same words; only `blocks`
 * differs, max(1, min(num_cu, ceil(np / 2^17))). */
int pic1dp_probe_host_moments_plan_exact(int32_t nx, int32_t which, int32_t deltaf, int64_t np, int32_t num_cu, int64_t out[35]);

/* The passes of one pic1dp_hip_power call (launch_policy.hpp power_plan), on the HOST: out[0] = passes (0: an unknown `which`,
 * w asked of a full-f run, a grid out of range), out[1] = weight sets selected (1 or 2), out[2] = bytes of the E tile,
 * out[3] = bytes of one plane, then per pass i eight words at out[4 + 8 i]: {blocks, threads, non-temporal loads, dynamic
 * LDS bytes, weight sets (bit 0 p, bit 1 w), planes in LDS (1) or straight in memory (0), first set in the output, sets}.
 * out holds 4 + 8 * 2 words.  Nonzero: null argument. */
int pic1dp_probe_host_power_plan(int32_t nx, int32_t nx_opd, int32_t nv_opd, int32_t which, int32_t deltaf, int64_t np,
                                 int32_t num_cu, int64_t out[20]);
/* ... and of one pic1dp_hip_power_exact call (launch_policy.hpp power_plan_exact): the same words; only `blocks` differs,
 * max(1, min(num_cu, ceil(np / 2^17))). */
int pic1dp_probe_host_power_plan_exact(int32_t nx, int32_t nx_opd, int32_t nv_opd, int32_t which, int32_t deltaf, int64_t np,
                                       int32_t num_cu, int64_t out[20]);

/* The passes of one pic1dp_hip_zoom call (launch_policy.hpp zoom_plan), on the HOST: out[0] = passes (0: arguments out of
 * range, pertb asked of a full-f run), out[1] = planes selected, out[2] = the library's pass cap (kZoomPassCap), then per
 * pass i eight words at out[3 + 8 i]: {blocks, threads, non-temporal loads, dynamic LDS bytes, the planes' mask, band in LDS
 * (1) or every row straight in memory (0), first v row, rows}.  pass_cap <= 0: the library's.  out holds 3 + 8 * 64 words.
 * Nonzero: null argument. */
int pic1dp_probe_host_zoom_plan(int32_t nxb, int32_t nvb, int32_t which, int32_t deltaf, int64_t np, int32_t num_cu,
                                int32_t pass_cap, int64_t out[515]);

/* The pass of one pic1dp_hip_hermite call (launch_policy.hpp hermite_plan), on the HOST: out = {workgroups (0: arguments out
 * of range, w asked of a full-f run), threads, non-temporal loads, dynamic LDS bytes, blocks of sixteen Hermite rows in the
 * accumulators (4, 8 or 16), the partial sums the launch merges into one output word}.  Nonzero: null argument. */
int pic1dp_probe_host_hermite_plan(int32_t nherm, int32_t nmodes, int32_t which, int32_t deltaf, int64_t np, int32_t num_cu,
                                   int64_t out[6]);
/* The device's Hermite recurrence alone (device_hermite.hpp herm_all, what k_hermite runs), on the current device:
 * out[i * nherm + k] = psi_k(u[i]), i < n, k < nherm <= 256. */
int pic1dp_probe_hermite(const double *u, int64_t n, int32_t nherm, double *out);

/* The count and write passes of a selection over np valid markers (launch_policy.hpp select_plan), on the HOST: out = {pairs
 * of a chunk, chunks, workgroups, threads, non-temporal loads, threads of the prefix sum's one workgroup}.  Chunk c holds the
 * logical pairs [c * pairs, min((c + 1) * pairs, np / 2)), and the odd last marker (np odd) belongs to the last chunk; np = 0:
 * no chunk, nothing is launched (the grid is still reported as 1).  threads_req / bpc_req: pic1dp_hip_set_launch's (0: the
 * library's choice).  Nonzero: null argument. */
int pic1dp_probe_host_select_plan(int64_t np, int32_t num_cu, int32_t threads_req, int32_t bpc_req, int64_t out[6]);

/* What pic1dp_hip_create decides before its first allocation (pic1dp_amd/csrc/context_plan.hpp plan_context), on the HOST,
 * for an input, a layout and the three requests of the settings that bear on it (0: none): PIC1DP_PRED_KIND,
 * PIC1DP_RHO_GLOBAL_COPIES as given (refused like settings_from_env refuses it), PIC1DP_FIELD_ONE_RANK_ORDER.  The input is taken as it is (not validated).
 * out (cap words, at least 16 + nspecies + nblk (1 + nspecies)) = {npe, nblk, blk0, nalloc, imerge, iremove, isplit,
 * gcopies, gstride, rho_set_doubles, pred_kind, pred_private, pred_set_doubles, pack_doubles, tab_lds, the field's npe,
 * np[nspecies], blk_alloc[nblk], blk_np[nspecies][nblk]}; sc = {sc_re, sc_im}.  Nonzero: null argument, nspecies or
 * nranks out of range, cap too small. */
int pic1dp_probe_host_context_plan(const pic1dp_input *in, const pic1dp_layout *lay, int32_t pred_kind_req, int32_t gcopies_req,
                                   int32_t one_rank_order, int64_t *out, int64_t cap, double sc[2]);
/* The settings a context created now would take from the environment (pic1dp_amd/csrc/settings.hpp settings_from_env):
 * iv = {fuse_solve, tail_on, call_pair, lazy_calls, predict, carry, osub_req, dyn_tail, dyn_tail_full, diag_fx,
 * pred_kind_req, chain_mfma_req, gcopies_req, field_one_rank_order, chain_selftest_verbose}, dv = {nt_threshold_half,
 * nt_threshold_full, diag_fx_margin_w}. */
int pic1dp_probe_host_settings(int32_t iv[15], double dv[3]);

/* What a time step launches (pic1dp_amd/csrc/step_plan.hpp), on the HOST: step_caps, plan_markers, plan_solve and
 * plan_whole_step for an input, a layout (plan_context makes the context's plan of them) and this query. */
typedef struct pic1dp_probe_step_query {
  /* settings (settings.hpp; nt_threshold_* <= 0: the default) */
  int32_t fuse_solve, tail_on, call_pair, lazy_calls, predict, carry, osub_req, dyn_tail, dyn_tail_full, pred_kind_req, gcopies_req,
      one_rank_order;
  double nt_threshold_half, nt_threshold_full;
  /* the device and pic1dp_hip_set_launch */
  int32_t num_cu, threads_req, bpc_req;
  /* what setters and the communicator change; field_npe 0: the plan's; has_pred < 0: the plan has a one-pass kernel */
  int32_t charge_sum, diag_sum, fuse_output, step_mode, field_solver, field_transform, comm, xchg, field_npe, chain_mfma, has_pred;
  int32_t pow2[8], one_exp[8]; /* SpeciesConst of each species */
  int64_t np[8];               /* valid markers of each species (< 0: the plan's) */
  /* plan_markers */
  int32_t full, diag, pred, tail_ok, eh_modes, nt_force;
  /* plan_solve */
  int32_t pred_fresh, tail_done, into_E;
  /* plan_whole_step: StepMoment */
  int32_t pending, have_eh, steps_left, output_now, output_next, optimize_now, optimize_next;
} pic1dp_probe_step_query;
/* out[112] = 13 words of StepCaps {dft_paths, six_sums_one_mode, modes_fit_field_kernel, exp_bearing, step_recompute_ok,
 * predict_capable, diag_in_step, priv, fuse_capable, lazy_calls_ok, pair_serves_collect, pair_in_solve_field, the plan's
 * pred_kind}; 12 of MarkerPlan {pred, priv, diag, tail_mode, tail_species, stream_nt, solve_species, solve_fits,
 * solve_threads, tag, bytes read, bytes written}; 8 x 9 of its species {launched, family, threads, blocks, LDS bytes,
 * dyn_tail, plain_chunks, carry, tail}; 6 of SolvePlan {refused, reduce_first, pack_reduce, pack_first, launch, with_local};
 * 9 of WholeStepPlan {substeps, finish_pending, diag, pred, fused_in, adopt_eh, half_pass, half_eh_modes, fuse_out}.
 * names[s]: what kernel_bytes would report of species s' launch.  Nonzero: null argument, nspecies or nranks out of range. */
int pic1dp_probe_host_step_plan(const pic1dp_input *in, const pic1dp_layout *lay, const pic1dp_probe_step_query *q, int64_t out[112],
                                char names[8][64]);

/* What a call of the call sites' lazy state machine enqueues and which state follows (pic1dp_amd/csrc/call_plan.hpp), on
 * the HOST: plan_call for
 *   state[9]   = CallState {seq, owed, e_step_start, cd_kept_mode_only, adopt_current, charge_pending, charge_pending_pred,
 *                call_phase, eh_modes},
 *   moment[14] = CallMoment {lazy_calls, call_pair, loaded, several_ranks, fp64_rank_sum, charge_sum, pred_kind, tab_lds,
 *                field_differs, pred_usable, eh_current, modes_current, optimize_due_any, output_follows},
 *   caps[8]    = the StepCaps it reads {dft_paths, six_sums_one_mode, modes_fit_field_kernel, predict_capable, diag_in_step,
 *                lazy_calls_ok, pair_serves_collect, pair_in_solve_field}
 * and a kind of call (the index of enum Call).  out[64] = {refusal, refused_after, the refused pair's seq and owed, the 9
 * words of the state that follows, the number n of actions, n x {action, argument}}, zeros behind; out[63]: 1 where
 * call_state_invariants holds of the state that follows under this moment and these caps.  Nonzero: null argument or no such
 * kind of call. */
int pic1dp_probe_host_call_plan(const int32_t state[9], const int32_t moment[14], const int32_t caps[8], int32_t call, int32_t out[64]);

/* The launch shape of the on-device particle load's pass over nalloc slots (launch_policy.hpp load_launch), on the HOST:
 * out = {workgroups, threads, non-temporal stores, markers a workgroup takes at a time}.  Workgroup b takes the chunks b,
 * b + workgroups, ... of [0, nalloc).  Nonzero: null argument, nalloc < 0 or num_cu < 1. */
int pic1dp_probe_host_load_launch(int64_t nalloc, int32_t num_cu, int64_t out[4]);
/* Where the owned reference blocks of one species lie in its packed arrays (pic1dp_amd/csrc/block_layout.hpp), on the HOST:
 * from the slots blk_alloc[nblk] and the valid markers blk_np[nblk] of the blocks, out[4 nblk] = per block {voff, np, toff,
 * ntail} -- valid markers [voff, voff + np), tail slots [toff, toff + ntail) -- and *np the species' valid markers.
 * Nonzero: null argument or nblk < 1. */
int pic1dp_probe_host_block_layout(const int64_t *blk_alloc, const int64_t *blk_np, int32_t nblk, int64_t *out, int64_t *np);
/* The 64-pair chunks at the head of a species' slab that a one-pass launch accesses with plain loads and stores while the
 * rest streams non-temporally (launch_policy.hpp stream_plain_chunks), on the HOST; nt: the launch is a non-temporal one.
 * Nonzero: null argument or a negative count. */
int pic1dp_probe_host_plain_chunks(int64_t np_all_species, int64_t np_species, int32_t nt, int64_t *chunks);
/* GB/s of the load kernel's stores WITHOUT its arithmetic: slots [0, n) of the four arrays of a tiled slab written as the
 * kernel writes them (launch_policy.hpp load_launch: chunks of one tile group per workgroup, non-temporal above the
 * threshold), reps launches between two events after one warm-up -- the stream k_load is measured against. */
int pic1dp_probe_write_stream(int32_t device, int64_t n, int32_t reps, double *gbytes_per_s);
/* The load kernel's index function (pic1dp_amd/csrc/device_load.hpp load_uniforms_dev) on the DEVICE over a list of n global
 * marker indices g (kind 2: below 3^21): uv[i], ux[i] as k_load forms them for marker g[i] of species ispecies -- to be held
 * against pic1dp_hip_host_load_uniforms bit for bit, beyond 2^32 too, without allocating that many markers. */
int pic1dp_probe_load_uniforms(int32_t device, int32_t kind, int32_t seed_offset, int32_t ispecies, const int64_t *g, int64_t n,
                               double *uv, double *ux);

#ifdef __cplusplus
}
#endif
#endif
