// ctx.hpp -- what the translation units behind the C ABI share: the context (one process = one GPU = one HIP stream),
// the error convention, and the internal entry points one unit offers the others.
//   capi.cpp           context (create: settings -> plan -> tables -> allocate -> self-test), input, transfers, field access, knobs
//   capi_timing.cpp    timers and kernel statistics: switches, reads, reset (timing.hpp: pic1dp_ctx::tm, the event spans)
//   settings.cpp       what a context takes from the environment, read once (settings.hpp: pic1dp_ctx::cfg; no HIP call)
//   context_plan.cpp   create()'s decisions as a pure function, and the mode tables (context_plan.hpp: pic1dp_ctx::plan; no HIP call)
//   device_mem.hpp     the one owner of a context's device and pinned memory (pic1dp_ctx::mem)
//   capi_step.cpp      the hot path's actions: the three call sites, the executor of their lazy state machine (call_site), pic1dp_hip_step, the prediction
//   call_plan.cpp      the call sites' decisions: for a kind of call arriving in a state, what is enqueued in which order and which state follows (call_plan.hpp: no context, no HIP call)
//   step_plan.cpp      the hot path's decisions: which marker kernel, carry, streaming, fused solve, tail, field launch (step_plan.hpp: no context, no HIP call)
//   launch_policy.cpp  the launch shapes of the marker kernels and of the diagnostics passes (launch_policy.hpp: no context, no HIP call)
//   capi_comm.cpp      RCCL communicator, the one-hop exchange's set-up, the charge sum over ranks
//   capi_diag.cpp      diagnostics of output_all
//   capi_products.cpp  read-only marker products on demand (pic1dp_hip_moments, _moments_exact, _power); what they share with select and gather
//   capi_select.cpp    select and gather markers on the device (pic1dp_hip_select_count, _select, _gather); the rule on the
//                      host and the thinning threshold: select_host.cpp (select_rule.hpp; no HIP call)
//   capi_zoom.cpp      the exact phase-space histogram on a caller's window and grid (pic1dp_hip_zoom; its host arithmetic: zoom_fx.cpp, no HIP call)
//   capi_hermite.cpp   the Fourier-Hermite spectrum of the markers, summed on the matrix unit (pic1dp_hip_hermite)
//   capi_optimize.cpp  marker optimisation events (merge / remove / split): one |delta f|(v), one driver of the blocks' workers, one piece per kind (the blocks' places in a species' arrays: block_layout.hpp; the per-marker lookups: opt_grid.hpp)
//   capi_checkpoint.cpp  the state digest, checkpoint and restart (the file itself: checkpoint.cpp, no HIP call)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/pic1dp_hip.h"
#include "block_layout.hpp"
#include "call_plan.hpp"
#include "context_plan.hpp"
#include "device_mem.hpp"
#include "kernels.hpp"
#include "launch_policy.hpp"
#include "loader.hpp"
#include "multirand.hpp"
#include "optimize.hpp"
#include "rccl_dyn.hpp"
#include "settings.hpp"
#include "step_plan.hpp"
#include "timing.hpp"

using namespace pic1dp;

namespace pic1dp_host {

// the message pic1dp_hip_last_error() hands out (thread-local, capi.cpp); returns code
int fail(int code, const char *fmt, ...);


#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(PIC1DP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                                    \
  } while (0)

#define CHECK_CTX(c) \
  if (!(c)) return fail(PIC1DP_ERR_ARG, "null context")

constexpr double kPi = 3.14159265358979323846264;        // PETSC_PI
constexpr double kSqrtEps = 1.490116119384766e-08;       // PETSC_SQRT_MACHINE_EPSILON
constexpr int64_t kHistCap = 1 << 20;
struct OptWorker;  // capi_optimize.cpp
struct Species {
  int64_t nalloc = 0, np = 0;
  PSet set[2] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
  double *p = nullptr;
  double *t2 = nullptr;   // carry of -f0'/f0 between the whole-step kernels
  uint64_t t2_version = 0;  // state_version whose step-start velocities the values in t2 belong to (0: none)
  double *slab[2] = {nullptr, nullptr};  // tiled storage of set 0 (+ p) and of the RK ping-pong set (kernels.hpp)
  double *rho = nullptr;  // slice of rho_sp
  double *fxb = nullptr;  // device [2]: bounds on |q| and |c| of this species' markers for the prediction tiles' fixed-point
                          // sums (kernels_step.hip FxTiles): seeded from the markers the host loads, raised by the kernels
  SpeciesConst sc{};
};

// Marker diagnostics of output_all, per species: one fused pass (histograms + kinetic sums; a launch of its own, or inside
// k_step_full<DIAG>), collected once and kept until the markers change (capi_diag.cpp)
struct DiagSpecies {
  uint64_t version = 0;               // state_version the cached results belong to
  double sums[3] = {0.0, 0.0, 0.0};   // the kinetic sums
  bool pending = false;               // a pass ran, its partial sums are still on the device
  int blocks = 0;                     // workgroups of that pass
  bool fixed = false;                 // ... which summed its histograms in 64-bit fixed point (device_diag.hpp DistScale)
  double max_p = 0.0, max_w = 0.0;    // max |p|, |w| as the last pass saw them: the next pass's scales (0: unknown -- doubles)
};

// what the context counts for pic1dp_hip_kernel_stats (capi_timing.cpp: the table's rows name these members), pic1dp_hip_power_exact_stats and pic1dp_hip_zoom_stats; nothing reads them to decide
struct Counters {
  int64_t diag_passes = 0;                 // separate k_ptcldist passes launched so far (kernel_stats 5)
  int64_t fused_solves = 0;                // marker launches whose prologue solved the previous step's field (7)
  int64_t opt_pcie_bytes = 0;              // bytes marker optimisation events have moved between host and device (8)
  int64_t tail_launches = 0;               // marker launches that carried a tail so far (10)
  int64_t call_pair_skips = 0;             // solve_field calls of a half step served without a launch (11)
  int64_t diag_fx_passes = 0, diag_fx_repeats = 0;   // fixed-point passes so far; passes repeated in doubles after an overflow (12)
  int64_t dfx_rejected = 0;                // terms the exact passes of the diagnostics did not sum so far (15)
  int64_t moments_passes = 0;              // k_moments passes launched so far (16)
  int64_t moments_exact_passes = 0;        // k_moments_exact passes launched so far (17)
  int64_t moments_exact_rejected = 0;      // terms they did not sum so far (18)
  int64_t load_passes = 0;                 // k_load passes launched so far (19)
  int64_t power_passes = 0;                // k_power passes launched so far (20)
  int64_t select_passes = 0;               // k_select_count and k_select_write passes launched so far (21)
  int64_t gather_launches = 0;             // k_gather launches so far (22)
  int64_t power_exact_passes = 0;          // k_power_exact passes that swept markers so far (pic1dp_hip_power_exact_stats)
  int64_t power_exact_rejected = 0;        // terms they did not sum so far (the same)
  int64_t zoom_passes = 0;                 // k_zoom passes that swept markers so far (pic1dp_hip_zoom_stats)
  int64_t zoom_rejected = 0;               // terms they did not sum so far (the same)
  int64_t hermite_passes = 0;              // k_hermite passes launched so far (pic1dp_hip_hermite_stats)
};

}  // namespace pic1dp_host
using namespace pic1dp_host;

struct pic1dp_ctx {
  pic1dp_input in{};
  pic1dp_layout lay{};
  Settings cfg{};      // the environment as create() found it: constants of the context
  ContextPlan plan{};  // what create() derived from input, layout and settings: constants too (blocks, one-pass kind, sizes)
  DeviceMem mem;       // owns every device and pinned buffer below (allocated at create() or lazily; released by destroy())
  Timing tm;           // timers and kernel statistics (timing.hpp)
  Counters cnt;        // what kernel_stats reports besides times
  int device = 0, num_cu = 256;
  hipStream_t st = nullptr;
  int cur = 0;  // which particle set is particle_x/v/w right now
  std::vector<Species> sp;
  std::vector<std::vector<int64_t>> blk_np;       // [nspecies][nblk] valid markers of the owned blocks now (plan.blk_np: as loaded)
  std::vector<Multirand> blk_rng;                 // [nblk] generators as particle_load left them
  bool rng_ready = false;
  int imerge = 0, iremove = 0, isplit = 0;        // particle_imerge / _iremove / _isplit
  bool loaded = false;
  bool charge_pending = false;  // charge_local ran, waiting for charge_reduced
  // Where the host stands in the reference's six calls push(1), collect_charge, solve_field, push(2), collect_charge,
  // solve_field, by the calls alone (eager call sites note no push, and after the second collect_charge nothing is noted
  // either): 0 between time steps, 1 ... 5 after the first ... fifth call.  Read by checkpoint_write's plan only (call_plan.cpp Call::Checkpoint).
  int call_phase = 0;
  // field
  double *d_rho_sp = nullptr, *d_charge = nullptr, *d_chargeden = nullptr, *d_E = nullptr;
  // The species accumulators and the six sums of the prediction exist three times (kernels.hpp FusedSolve): d_rho_sp /
  // Species::rho / fa.rho_sp / d_pred always name the set the marker kernels deposit into NOW (acc_idx); all sets are
  // zero whenever no fused launch sequence is under way
  double *d_rho_all = nullptr, *d_pred_all = nullptr;
  int acc_idx = 0;
  bool fused_pending = false;   // step(): the last marker launch left the solve of its step to the next launch's prologue
  int fused_dirty = -1;         // accumulator set the last fused launch read (still holding that step's deposits), or -1
  FusedSolve fuse_args{};       // what the next marker launch's prologue has to solve (on = 1), consumed by step_particles
  double *d_mode_re = nullptr, *d_mode_im = nullptr, *d_fre = nullptr, *d_fim = nullptr;
  double *d_ginv = nullptr, *d_hist = nullptr, *d_scratch = nullptr, *d_dist = nullptr;
  // one pass per step (kernels_step.hip k_step_one): mode tables with E = sum re_m A_m + im_m B_m, the
  // prediction accumulators [nspecies][1 + 2 nm][nx], the combined half-step charge density
  double *d_tabA = nullptr, *d_tabB = nullptr, *d_pred = nullptr, *d_cd_h = nullptr, *d_mode_h = nullptr;
  PredTab pred_tab{};              // kind 2: sums / Gram matrix of the kept mode's tables (host, libm)
  int eh_modes = 0;                // kind 2: where the kept mode of the Eh about to be used lies: 0 nowhere, 1 fa.mode_*, 2 d_mode_h
  bool charge_pending_pred = false;  // kind 2: charge_local handed out the six sums, not a charge vector
  double *d_Ehn = nullptr;         // half-step field predicted for the NEXT step (d_Eh stays the last step's)
  double *d_pack = nullptr;        // [2 + 2 nmode][nx] one all-reduce per one-pass step (RCCL path)
  // several ranks, six-sum prediction: the marker launch's last workgroup packs / posts this rank's charge (kernels.hpp
  // StepTail) instead of a launch of its own in front of the sum over ranks.  cfg.tail_on 0: the separate launch
  unsigned int *d_ticket = nullptr;  // the tail's arrival counter (zero between launches)
  int tail_done = 0;                 // what the last marker launch's tail did: 0 nothing, 1 packed into d_pack, 2 posted (tail_x)
  XchgArgs tail_x{};                 // tail_done == 2: the exchange the field launch has to finish
  uint64_t pred_version = 0;       // state_version the accumulators in d_pred belong to (0: none)
  uint64_t eh_version = 0;         // state_version d_Eh has been predicted for (step() path)
  uint64_t field_version = 1, eh_field_version = 0, modes_field_version = 0;  // who wrote d_E last
  double *d_stage = nullptr;  // contiguous staging buffer between host arrays and the tiled marker arrays
  unsigned long long *d_loadmax = nullptr;  // [nspecies][2] bit patterns of max |p|, max |w| of a device load (capi.cpp; allocated at the first one)
  unsigned long long *d_digest = nullptr;  // [nspecies][4] the state digest's words (capi_checkpoint.cpp; allocated at the first digest)
  double *d_Eh = nullptr;  // field after the first sub-step of the last whole-step call
  // The reference's three call sites at whole-step cost (see "lazy call sites"
  // below): a push is only noted; the collect_charge that follows runs the
  // whole-step kernel instead of push + deposit (cfg.lazy_calls).
  // Call sites, one rank: the solve_field that follows the collect_charge of push(2) solves BOTH fields in one launch
  // (the pair kernels of pic1dp_hip_step) -- the new state's into field_electric, the next step's half-step field from the
  // prediction into d_Ehn / d_mode_h.  The next push(1) / collect_charge / solve_field then launch nothing: the
  // "Pair" states of Seq say that the half-step field lies in d_Ehn (field_electric still holds the step-start field, d_E0 is
  // not filled), the "Solved" ones that the host has called solve_field for it -- what it may look at from then on is the
  // half-step field, so every inspection first settles (call_plan.cpp settle_half_pair: copies, memory as eager calls leave it).
  // cfg.call_pair 0: the three launches per step of rounds 2-4.
  // collect_charge leaves its last step to the solve_field that follows (one launch less per sub-step): settled (call_plan.cpp
  // materialize_cd) before anything else looks at charge, chargeden or the accumulators.
  // The machine's variables -- seq, owed, e_step_start, cd_kept_mode_only, adopt_cd_version, charge_pending[_pred], call_phase,
  // eh_modes -- are read by capi_step.cpp's bridge (call_state_of) and written by its store alone: every other unit asks call_site().
  Owed owed = Owed::Nothing;
  // field_chargeden holds only the kept mode's content of the half-step charge density (collect_charge after a
  // noted push(1) served from the six sums, pred_kind 2): all solve_field looks at, but not what the reference
  // holds there.  get_field rebuilds the full vector on one rank (call_plan.cpp rebuild_half_step_chargeden); cleared by
  // everything that writes field_chargeden.
  bool cd_kept_mode_only = false;
  // field_chargeden as the eager calls leave it changes with every collect_charge, charge_reduced, set_chargeden, substep and
  // step: cd_version counts those calls, adopt_cd_version is its value when the collect_charge set AdoptHalfField -- the
  // adoption stands for a solve from THAT charge density and only holds while the two agree
  uint64_t cd_version = 1, adopt_cd_version = 0;
  Seq seq = Seq::Clean;          // (call_plan.hpp) written by set_call_state only (capi_step.cpp)
  // The collect_charge of a push(2) noted after a pair-solved half step (Push2PairSolved) runs the whole step with
  // E0 = field_electric and leaves field_electric holding the STEP-START field, the kept modes too: the solve_field that
  // follows overwrites both.  Everything that reads them before it first copies the half-step field (d_Eh / d_mode_h) in
  // -- what the eager calls hold there (call_plan.cpp settle_step_start_field).
  bool e_step_start = false;
  double *d_E0 = nullptr;        // field the noted push(1) saw
  double *d_rho_dummy = nullptr; // accumulator of a wrap-only deposit
  int step_mode = 0;       // 0 auto (recompute path when the LDS allows), 1 two fused sub-steps
  int field_solver = 0;    // 0 the reference's mode-filter DFT solve, 1 finite-difference tridiagonal (opt-in)
  // how the mode-filter solve computes its DFT (pic1dp_hip_set_field_transform; kernels_fft.hip): 0 the dense tables, the
  // reference's sums; 1 the FFT (plan built at the first switch).  Transform 1 runs none of the fused or predicted paths
  // (step_plan.hpp StepCaps::dft_paths).
  int field_transform = 0;
  FftArgs fft{};
  double *d_fft_tw = nullptr;
  int *d_fft_idx = nullptr;
  int64_t hist_count = 0;
  // marker diagnostics of output_all: one fused pass per species (histograms +
  // kinetic sums), kept until the markers change
  uint64_t state_version = 1;              // bumped by everything that writes marker arrays
  std::vector<DiagSpecies> diag;           // [nspecies]
  double *d_diag_part = nullptr;           // [nspecies][diag_max_blocks][DIAG_PART] per-workgroup partial sums of the pass
  int fuse_output = 0;                     // take the diagnostics inside k_step_full on steps output_all follows
  double *d_rec = nullptr;                 // output_all's record gathered on the device (kernels.hpp PackArgs), grow-only
  size_t d_rec_doubles = 0;
  double *h_pin = nullptr;                 // pinned host staging of the small device-to-host transfers (output_all's calls:
  size_t h_pin_doubles = 0;                // pageable copies cost a synchronous call each, ~20 us; grow-only, capi_diag.cpp pinned)
  DistGeom dist_geom_v{};                  // output_ptcldist's histogram geometry (capi_diag.cpp dist_geom)
  bool dist_geom_ready = false;
  std::vector<OptWorker *> opt_workers;    // streams and staging of the events' block workers (capi_optimize.cpp OptWorker), kept between events
  // the marker products on demand (capi_products.cpp): one device buffer for whichever runs, grow-only, zeroed by every call over what it uses
  double *d_prod = nullptr;
  size_t d_prod_words = 0;                 // its capacity in 8-byte words
  double *d_herm = nullptr;                // the Hermite spectrum's tables ra, rb [2][256] and its words [256][16] (capi_hermite.cpp; allocated at the first call)
  int chain_selftest = 0;                  // create()'s verdict on the serial sums through the matrix unit: 1 identical, 0 differs, -1 could not run
  int32_t itime = 0;
  double time = 0.0;
  int seed_offset = 0;                     // ensemble member: block b draws from stream mype = b + seed_offset (pic1dp_hip_set_seed_offset)
  GridConst grid{};
  FieldArgs fa{};
  // comm
  ncclComm_t comm = nullptr;
  // one-hop charge exchange (kernels_field.hip exchange_charge): the own area, the peers'
  // areas as mapped through hipIpc, and the running exchange number
  struct Xchg {
    void *local = nullptr;                       // flags + slots of this rank
    void *peer[XCHG_MAX_RANKS] = {nullptr};      // every rank's area as mapped here (own: local)
    bool opened[XCHG_MAX_RANKS] = {false};       // peer[q] came from hipIpcOpenMemHandle
    unsigned long long *err = nullptr;           // pinned host word the kernel reports a time-out in
    unsigned long long epoch = 0;
    long long timeout_ticks = 0;
    unsigned long long *ticks = nullptr;         // device [2]: ticks inside exchanges, exchanges timed (while timers are on)
    bool connected = false;
    int memkind = 0;                             // 1 fine-grained, 2 uncached, 3 plain hipMalloc
  } xc;
  int allreduce_kind = 0;  // 0 auto (RCCL when a communicator exists), 1 RCCL, 2 one-hop exchange
  // kind 1 of the charge sum (pic1dp_hip_set_charge_sum, exact_charge.cpp; kernels.hpp FxArgs): the deposits go into
  // exact integer accumulators, which the settle step (fx_settle) sums over ranks and turns into the species accumulators
  // before anything reads them -- from there on the FP64 path runs as on one rank.  No prediction, no fused solve, no
  // tail, no diagnostics inside the step while it is set.
  int charge_sum = 0;
  long long *d_fx = nullptr;                 // [nspecies][2][nx] (hi row, lo row); zero between calls
  unsigned long long *h_fx_ovf = nullptr;    // pinned [8]: contributions beyond 2^62 quanta so far, per species
  unsigned long long fx_ovf_seen[8] = {0};   // ... of which the host has reported
  int fx_e[8] = {0};                         // e_s of the quantum 2^e_s
  double fx_q[8] = {0}, fx_inv_q[8] = {0};   // 2^e_s, 2^-e_s
  // kind 1 of the diagnostics sum (pic1dp_hip_set_diag_sum, capi_diag.cpp; kernels.hpp DiagFxArgs): output_all's
  // diagnostics from exact integer sums, always in their own pass (no k_step_full<DIAG> while it is set); independent of
  // charge_sum.  The cached pass of a species is d_dfx's slot, valid while DiagSpecies::version says so.
  int diag_sum = 0;
  long long *d_dfx = nullptr;                // [nspecies + 1][diag_fx_words]: per species, + the copy summed over ranks
  int dfx_e[8][6] = {{0}};                   // the six log2 quanta per species (pic1dp_hip_diag_quanta)
  // launch
  int threads_req = 0, bpc_req = 0;
};

namespace pic1dp_host {

// several ranks share the run: the layout says so, or a communicator exists
inline bool several_ranks(const pic1dp_ctx *c) { return c->lay.nranks > 1 || c->comm != nullptr; }
// ... and their charge is summed in FP64 (kind 0 of the charge sum; kind 1 sums exact integers in fx_settle, after which
// the one-rank path runs)
inline bool fp64_rank_sum(const pic1dp_ctx *c) { return c->charge_sum == 0 && several_ranks(c); }

// ---- capi.cpp ----
int ensure_second_set(pic1dp_ctx *c);     // the second slab (RK ping-pong set; re-packing target of the optimiser)
void wire_species(Species &S, const pic1dp_input &in);  // set[0], p and -- where slab[1] exists -- set[1] from the slabs: THE array bases of a species
int put_range(pic1dp_ctx *c, double *arr, int64_t off, const double *host, int64_t cnt);
int get_range(pic1dp_ctx *c, const double *arr, int64_t off, double *host, int64_t cnt);
// ---- capi_step.cpp (the hot path and the executor of the lazy call sites' state machine) ----
// THE entry of everything that intrudes on the call sites' sequence: the plan of this kind of call (call_plan.hpp Call) in
// the state the context is in, its actions enqueued, the state that follows stored; a refusal is the error returned.
// who: the caller's name where the refusal's message names it; field_differs: Call::SwitchField's question
int call_site(pic1dp_ctx *c, Call call, const char *who = nullptr, bool field_differs = false);
int require_loaded(pic1dp_ctx *c);        // call_site(Call::Markers): markers loaded, no charge_local pending; memory as eager calls would have left it
void field_written(pic1dp_ctx *c, bool by_solve);  // d_E changed: versions, what a noted push may still assume
// Everything a checkpoint file does not carry put into ONE defined state: checkpoint_write and
// checkpoint_read both end here, so the writing context and one restored from its file continue identically
int reset_derived_state(pic1dp_ctx *c);
// ---- capi_comm.cpp ----
int allreduce_charge(pic1dp_ctx *c);
int allreduce_doubles(pic1dp_ctx *c, double *d, size_t n);
int reduce_charge(pic1dp_ctx *c);
bool xchg_active(const pic1dp_ctx *c);
XchgArgs next_xchg_args(pic1dp_ctx *c);
int xchg_check(pic1dp_ctx *c);
void comm_release(pic1dp_ctx *c);         // communicator and exchange mappings, for destroy
int xchg_vec(const pic1dp_ctx *c);      // vectors of nx doubles one exchange slot holds
// ---- capi_optimize.cpp ----
void optimize_due_at(const pic1dp_ctx *c, double time0, bool due[3]);  // which events a step starting at time0 fires
void optimize_due(const pic1dp_ctx *c, bool due[3]);
bool optimize_due_any(const pic1dp_ctx *c);
void optimize_release(pic1dp_ctx *c);     // the optimisation events' workers (streams, pinned and device staging), for destroy
// ---- exact_charge.cpp (kind 1 of the charge sum) ----
FxArgs fx_args(const pic1dp_ctx *c, int isp);   // the marker kernels' exact accumulators of species isp (acc null in kind 0)
int fx_settle(pic1dp_ctx *c);             // deposits -> summed over ranks -> the species accumulators (copy 0)
int fx_check(pic1dp_ctx *c);              // PIC1DP_ERR_ARG once per batch of contributions beyond 2^62 quanta
// ---- capi_diag.cpp ----
int diag_buffers(pic1dp_ctx *c);
int diag_max_blocks(const pic1dp_ctx *c);
double *diag_part_dev(const pic1dp_ctx *c, int isp);   // species isp's slice of d_diag_part
void diag_void_bounds(pic1dp_ctx *c);                   // new or changed p, w: the fixed-point passes' bounds are void
bool diag_fx_bounds(const pic1dp_ctx *c, int isp, double *bound_p, double *bound_w);  // may the next pass sum in fixed point?
void diag_note_pass(pic1dp_ctx *c, int isp, int blocks, bool fixed, bool launched);   // a pass is enqueued
const DistGeom &dist_geom(pic1dp_ctx *c);
int pinned(pic1dp_ctx *c, size_t ndoubles, double **out);   // the context's pinned staging with room for ndoubles
size_t dist_len(const pic1dp_input &in);
// ---- capi_products.cpp (what every read-only pass over a species' markers begins with and is made of) ----
int product_begin(pic1dp_ctx *c, const char *who, int32_t isp);   // species index and markers checked, the device current, a noted push in memory; who: for the message
int product_check(pic1dp_ctx *c, const char *who, int32_t isp);   // ... its refusals alone (gather: what it checks next needs the species)
// npass launches under one tag, each bracketed and counted; none when the species has no valid marker
template <class Launch>
int run_passes(pic1dp_ctx *c, int tag, int64_t &counter, int npass, int64_t np, Launch launch) {
  for (int i = 0; i < npass && np > 0; ++i) {
    Span ks(c->tm, tag, c->tm.stats_on);
    HIP_TRY(launch(i));
    if (int rc = ks.end()) return rc;
    counter++;
  }
  return 0;
}

// ---- what the calls with buffers of their own share (capi_select.cpp, capi_zoom.cpp) ----
constexpr int64_t kSliceWords = static_cast<int64_t>(4) << 20;  // 32 MiB of pinned staging per transfer, as the checkpoint's

// a device buffer that lives for one call (capi_select.cpp, capi_zoom.cpp): taken from the context's owner, given back when it goes out of scope
template <class T>
struct CallBuf {
  DeviceMem &mem;
  T *p = nullptr;
  explicit CallBuf(DeviceMem &m) : mem(m) {}
  CallBuf(const CallBuf &) = delete;
  CallBuf &operator=(const CallBuf &) = delete;
  ~CallBuf() {
    if (p) mem.release(&p);
  }
  // 0, or PIC1DP_ERR_NOMEM / PIC1DP_ERR_HIP with the message set
  int take(size_t n, const char *who, const char *what) {
    const hipError_t e = mem.alloc(&p, n);
    if (e == hipSuccess) return 0;
    (void)hipGetLastError();
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation)
      return fail(PIC1DP_ERR_NOMEM, "%s: no device memory for %s (%zu bytes)", who, what, n * sizeof(T));
    return fail(PIC1DP_ERR_HIP, "%s: allocating %s failed: %s", who, what, hipGetErrorString(e));
  }
};

// n 8-byte words from the device to the host through the pinned staging, slice by slice
inline int words_to_host(pic1dp_ctx *c, void *host, const void *dev, int64_t n) {
  if (n <= 0 || !host) return 0;
  double *h = nullptr;
  if (int rc = pinned(c, static_cast<size_t>(std::min(n, kSliceWords)), &h)) return rc;
  for (int64_t done = 0; done < n; done += kSliceWords) {
    const int64_t m = std::min(kSliceWords, n - done);
    HIP_TRY(hipMemcpyAsync(h, static_cast<const double *>(dev) + done, sizeof(double) * m, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    std::memcpy(static_cast<double *>(host) + done, h, sizeof(double) * m);
  }
  return 0;
}

}  // namespace pic1dp_host
