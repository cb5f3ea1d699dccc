// capi_timing.cpp -- the timers and the per-kernel statistics behind the C ABI of include/pic1dp_hip.h (timing.hpp): switching,
// resolving, reading and resetting them; pic1dp_hip_kernel_stats is one table row per `which`.
#include "ctx.hpp"

namespace pic1dp_host {

int ev_resolve(Timing &t) {
  if (t.ev_used == 0) return 0;
  HIP_TRY(hipStreamSynchronize(t.st));
  for (size_t i = 0; i < t.ev_used; ++i) {
    float ms = 0.f;
    const EvPair &p = t.evpool[i];
    HIP_TRY(hipEventElapsedTime(&ms, p.a, p.b));
    (p.head ? t.head_ms : t.acc_ms)[p.tag] += ms;
    (p.head ? t.head_n : t.acc_n)[p.tag] += 1;
  }
  t.ev_used = 0;
  return 0;
}

}  // namespace pic1dp_host

namespace {

// pic1dp_hip_kernel_stats: what row `which` hands out.  A tag: *ms is the device time of the launches bracketed under it while
// kernel stats were enabled (the recorded pairs are resolved first: one stream synchronisation if any are pending).  A
// counter: *launches is that member of pic1dp_ctx::cnt; without one, the launches timed under the tag.  A row with neither
// is one of the four functions below the struct.
struct StatsRow {
  int tag;                                        // -1: none, *ms = 0 and the stream is not looked at
  int64_t Counters::*counter;
  int (*special)(pic1dp_ctx *, double *, int64_t *);
};

int stats_chain(pic1dp_ctx *c, double *ms, int64_t *n) {
  *ms = static_cast<double>(c->chain_selftest), *n = c->fa.chain_mfma;
  return 0;
}
int stats_diag_fx(pic1dp_ctx *c, double *ms, int64_t *n) {
  *ms = static_cast<double>(c->cnt.diag_fx_repeats), *n = c->cnt.diag_fx_passes;
  return 0;
}
int stats_pred_tiles(pic1dp_ctx *c, double *ms, int64_t *n) {
  HIP_TRY(hipStreamSynchronize(c->st));
  *n = 0, *ms = 0.0;
  for (size_t s = 0; s < c->sp.size(); ++s) {
    double h[3] = {0.0, 0.0, 0.0};
    HIP_TRY(hipMemcpy(h, c->sp[s].fxb, sizeof h, hipMemcpyDeviceToHost));
    int64_t k;
    std::memcpy(&k, &h[2], sizeof k);
    *n += k;
    if (s == 0) *ms = h[0];
  }
  return 0;
}
int stats_charge_fx(pic1dp_ctx *c, double *ms, int64_t *n) {
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->st));
  *n = 0, *ms = 0.0;
  if (c->h_fx_ovf)
    for (int s = 0; s < c->in.nspecies; ++s) *n += static_cast<int64_t>(reinterpret_cast<volatile unsigned long long *>(c->h_fx_ovf)[s]);
  return 0;
}

constexpr StatsRow kStatsRows[] = {
    /*  0 */ {kTagFused, nullptr, nullptr},       // the marker kernels, by tag: 0 fused, 1 push, 2 deposit, 3 half step, 4 whole step
    /*  1 */ {kTagPush, nullptr, nullptr},
    /*  2 */ {kTagDeposit, nullptr, nullptr},
    /*  3 */ {kTagStepHalf, nullptr, nullptr},
    /*  4 */ {kTagStepFull, nullptr, nullptr},
    /*  5 */ {-1, &Counters::diag_passes, nullptr},          // counters: ctx.hpp says what each counts
    /*  6 */ {kTagStepOne, nullptr, nullptr},     // the one-pass step
    /*  7 */ {-1, &Counters::fused_solves, nullptr},
    /*  8 */ {-1, &Counters::opt_pcie_bytes, nullptr},
    /*  9 */ {-1, nullptr, stats_chain},       // how the serial forward sums of the one-rank order run: 0 chains of additions, 1 the matrix unit; *ms: create()'s self-test (1 identical, 0 differs, -1 could not run)
    /* 10 */ {-1, &Counters::tail_launches, nullptr},
    /* 11 */ {-1, &Counters::call_pair_skips, nullptr},
    /* 12 */ {-1, nullptr, stats_diag_fx},     // diagnostics passes with 64-bit fixed-point histogram sums; *ms: of them, repeated in doubles (overflow)
    /* 13 */ {-1, nullptr, stats_pred_tiles},  // prediction tiles: terms that went past the fixed-point sums (beyond 16x the bound); *ms: the first species' bound on |q|
    /* 14 */ {-1, nullptr, stats_charge_fx},   // kind 1 of the charge sum: contributions beyond 2^62 quanta so far (not summed; reported as PIC1DP_ERR_ARG)
    /* 15 */ {-1, &Counters::dfx_rejected, nullptr},
    /* 16 */ {kTagMoments, &Counters::moments_passes, nullptr},   // passes of a product or of the device load, and their device time
    /* 17 */ {kTagMomentsExact, &Counters::moments_exact_passes, nullptr},
    /* 18 */ {-1, &Counters::moments_exact_rejected, nullptr},
    /* 19 */ {kTagLoad, &Counters::load_passes, nullptr},
    /* 20 */ {kTagPower, &Counters::power_passes, nullptr},
    /* 21 */ {kTagSelect, &Counters::select_passes, nullptr},
    /* 22 */ {kTagGather, &Counters::gather_launches, nullptr},
};
constexpr int kNumStatsRows = static_cast<int>(sizeof kStatsRows / sizeof kStatsRows[0]);

}  // namespace

extern "C" {

int pic1dp_hip_timers_enable(pic1dp_ctx *c, int32_t on) {
  CHECK_CTX(c);
  if (on < 0) return fail(PIC1DP_ERR_ARG, "timers_enable: 0 off, 1 every launch, n >= 2 every n-th launch of a timer");
  if (int rc = ev_resolve(c->tm)) return rc;
  c->tm.timers_on = on != 0;
  c->tm.timer_every = on > 1 ? on : 1;
  return 0;
}

int pic1dp_hip_timer_ms(pic1dp_ctx *c, int32_t iwt, double *ms) {
  CHECK_CTX(c);
  if (iwt < 0 || iwt >= 100 || !ms) return fail(PIC1DP_ERR_ARG, "bad timer id");
  Timing &t = c->tm;
  if (int rc = ev_resolve(t)) return rc;
  *ms = t.acc_ms[iwt];
  // sampled timers: the spans that were timed stand for the ones that were only counted -- apart from the first block of
  // the timer id (first launches, the run's first step), which is always timed and enters as it is
  const int64_t later = t.span_seen[iwt] - t.head_n[iwt];
  if (t.acc_n[iwt] > 0 && later > t.acc_n[iwt]) *ms *= static_cast<double>(later) / static_cast<double>(t.acc_n[iwt]);
  *ms += t.head_ms[iwt];
  // (no later block timed yet -- a short run, or a timer id with few launches: the first block's mean stands for them)
  if (t.acc_n[iwt] == 0 && t.head_n[iwt] > 0 && later > 0)
    *ms += t.head_ms[iwt] * static_cast<double>(later) / static_cast<double>(t.head_n[iwt]);
  return 0;
}

int pic1dp_hip_timers_reset(pic1dp_ctx *c) {
  CHECK_CTX(c);
  Timing &t = c->tm;
  if (int rc = ev_resolve(t)) return rc;
  for (int i = 0; i < kNumTags; ++i) {
    t.acc_ms[i] = t.head_ms[i] = 0.0;
    t.acc_n[i] = t.head_n[i] = t.span_seen[i] = 0;
  }
  return 0;
}

int pic1dp_hip_kernel_stats_enable(pic1dp_ctx *c, int32_t on) {
  CHECK_CTX(c);
  c->tm.stats_on = on != 0;
  return 0;
}

int pic1dp_hip_kernel_stats(pic1dp_ctx *c, int32_t which, double *ms, int64_t *launches) {
  CHECK_CTX(c);
  if (which < 0 || which >= kNumStatsRows) return fail(PIC1DP_ERR_ARG, "which must be 0..%d", kNumStatsRows - 1);
  const StatsRow &row = kStatsRows[which];
  double t = 0.0;
  int64_t n = 0;
  if (row.special) {
    if (int rc = row.special(c, &t, &n)) return rc;
  } else {
    if (row.tag >= 0) {
      if (int rc = ev_resolve(c->tm)) return rc;
      t = c->tm.acc_ms[row.tag];
    }
    n = row.counter ? c->cnt.*row.counter : c->tm.acc_n[row.tag];
  }
  if (ms) *ms = t;
  if (launches) *launches = n;
  return 0;
}

// the exact power's passes are not a row of kernel_stats (its rows end at 22): an entry point of their own
int pic1dp_hip_power_exact_stats(pic1dp_ctx *c, double *ms, int64_t *passes, int64_t *rejected) {
  CHECK_CTX(c);
  if (int rc = ev_resolve(c->tm)) return rc;
  if (ms) *ms = c->tm.acc_ms[kTagPowerExact];
  if (passes) *passes = c->cnt.power_exact_passes;
  if (rejected) *rejected = c->cnt.power_exact_rejected;
  return 0;
}

// ... and so are the zoom's
int pic1dp_hip_zoom_stats(pic1dp_ctx *c, double *ms, int64_t *passes, int64_t *rejected) {
  CHECK_CTX(c);
  if (int rc = ev_resolve(c->tm)) return rc;
  if (ms) *ms = c->tm.acc_ms[kTagZoom];
  if (passes) *passes = c->cnt.zoom_passes;
  if (rejected) *rejected = c->cnt.zoom_rejected;
  return 0;
}

// ... and the Hermite spectrum's
int pic1dp_hip_hermite_stats(pic1dp_ctx *c, double *ms, int64_t *passes) {
  CHECK_CTX(c);
  if (int rc = ev_resolve(c->tm)) return rc;
  if (ms) *ms = c->tm.acc_ms[kTagHermite];
  if (passes) *passes = c->cnt.hermite_passes;
  return 0;
}

int pic1dp_hip_kernel_bytes(pic1dp_ctx *c, int32_t which, double *read_bytes, double *written_bytes, double *carry_bytes,
                            char *name, int32_t name_len) {
  CHECK_CTX(c);
  if (which < 0 || which > 6 || which == 5) return fail(PIC1DP_ERR_ARG, "which must be 0..4 or 6");
  const KernelBytes &kb = c->tm.kbytes[kStatsRows[which].tag];
  if (read_bytes) *read_bytes = kb.rd;
  if (written_bytes) *written_bytes = kb.wr;
  if (carry_bytes) *carry_bytes = kb.carry;
  if (name && name_len > 0) std::snprintf(name, static_cast<size_t>(name_len), "%s", kb.name);
  return 0;
}

}  // extern "C"
